// An expert's rows description for the decode-step GEMM's K loop, written once for moe_gemm_kernel (moe.hip),
// moe_gemm_w8_kernel (moe_w8.hip) and moe_gemm_w4_kernel (moe_w4.hip), in two pieces of text around the form's K-loop set-up
// (gemm_skinny_w16_head.inc / gemm_skinny_w8_head.inc / gemm_skinny_w4_head.inc, which say why this is text): this one in front of it, moe_rows_gather.inc behind it.  MF and the
// launch's arguments `p` (a MoeDev) come from the including kernel.
//
// This piece: the expert's rows, sorted positions [r0, r0 + cnt).  No rows: nothing of this expert is read and no barrier is met,
// the same for all the workgroup's threads.  The weight starts e * expert_stride into p.w; the fragments the cnt rows reach are live.
  const int e = blockIdx.z;
  const int r0 = max(0, min(p.offsets[e], p.rows));
  const int cnt = min(min(p.offsets[e + 1], p.rows) - r0, MF * 16);  // (an expert has at most T <= 16 MF rows)
  if (cnt <= 0) return;
  const int nf = (cnt + 15) >> 4;  // live row fragments (workgroup-uniform)
  constexpr bool all_live = false;
  const auto wbase = [&] { return (int64_t)e * p.estride; };

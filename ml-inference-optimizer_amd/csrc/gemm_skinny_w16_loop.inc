// The K loop of the decode-step GEMM on 16-bit weights, included behind gemm_skinny_w16_head.inc (which says why this is text).
// Lane (c, q) loads the 16-byte pieces of its weight row at k + 8 q straight into VGPRs as the MFMA A operand; the x rows of a
// chunk are staged once per workgroup through LDS, 16-byte piece p of row r at p ^ (r & 15), and read back as the B operand.
// What varies between the including kernels is the rows description, which they define between the two pieces:
//   nf, all_live   row fragments of 16 that are live: only these are stored to LDS and multiplied.  Workgroup-uniform.  The dense
//                  GEMM's is the constant MF, which all_live = true says at compile time; an expert's is ceil(its rows / 16).
//   xhas(i, r)     whether a row of x lies behind staged row r (piece i of this thread's XPT pieces); where none does the stage
//                  holds zeros that are never read from memory
//   xrow(i, r)     which row of x that is
// The loop leaves the slice's sums behind for skinny_write: acc, accg (lane (c, q): rows 16 mf + c, columns n0 + 4 q .. + 3).
  auto load_w = [&](u32x4_t (&wr)[KS], u32x4_t (&gr)[GLU ? KS : 1], int ch) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int k = kb + ch * SKC + ks * SKINNY_KSTEP + 8 * q;
      const bool ok = active && k < ke;
      wr[ks] = (u32x4_t){0u, 0u, 0u, 0u};
      if (ok) wr[ks] = *(const u32x4_t*)(wrow + k);
      if constexpr (GLU) {
        gr[ks] = (u32x4_t){0u, 0u, 0u, 0u};
        if (ok) gr[ks] = *(const u32x4_t*)(grow + k);
      }
    }
  };
  auto stage_x = [&](int ch, int buf) {
    u32x4_t v[XPT];
#pragma unroll
    for (int i = 0; i < XPT; ++i) {
      const int idx = tid + i * 256, row = idx / PCS, pc = idx % PCS;
      const int k = kb + ch * SKC + pc * 8;
      v[i] = (u32x4_t){0u, 0u, 0u, 0u};
      if (xhas(i, row) && k < ke) v[i] = *(const u32x4_t*)(xg + (int64_t)xrow(i, row) * p.ldx + k);
    }
#pragma unroll
    for (int i = 0; i < XPT; ++i) {
      const int idx = tid + i * 256, row = idx / PCS, pc = idx % PCS;
      if (all_live || row < nf * 16) *(u32x4_t*)(sx[buf] + row * ROWB + ((pc ^ (row & 15)) * 16)) = v[i];
    }
  };

  f32x4_t acc[MF], accg[GLU ? MF : 1];
#pragma unroll
  for (int mf = 0; mf < MF; ++mf) {
    acc[mf] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    if constexpr (GLU) accg[mf] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  }
  auto compute = [&](const u32x4_t (&wr)[KS], const u32x4_t (&gr)[GLU ? KS : 1], int buf) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
      for (int mf = 0; mf < MF; ++mf) {
        if (mf < nf) {  // (workgroup-uniform)
          const X8 xf = __builtin_bit_cast(X8, *(const u32x4_t*)(sx[buf] + (mf * 16 + c) * ROWB + (((ks * 4 + q) ^ c) * 16)));
          acc[mf] = DT<T>::mfma16(__builtin_bit_cast(X8, wr[ks]), xf, acc[mf]);
          if constexpr (GLU) accg[mf] = DT<T>::mfma16(__builtin_bit_cast(X8, gr[ks]), xf, accg[mf]);
        }
      }
    }
  };

  // Two register sets: the loads of chunk ch + 1 are issued before chunk ch is multiplied.  One barrier per chunk: the x buffer
  // written for chunk ch was last read for chunk ch - 2, before the barrier of chunk ch - 1.
  u32x4_t wa[KS], wb[KS], ga[GLU ? KS : 1], gb[GLU ? KS : 1];
  if (nc > 0) load_w(wa, ga, 0);
  for (int ch = 0; ch < nc; ch += 2) {
    stage_x(ch, 0);
    __syncthreads();
    if (ch + 1 < nc) load_w(wb, gb, ch + 1);
    compute(wa, ga, 0);
    if (ch + 1 >= nc) break;
    stage_x(ch + 1, 1);
    __syncthreads();
    if (ch + 2 < nc) load_w(wa, ga, ch + 2);
    compute(wb, gb, 1);
  }

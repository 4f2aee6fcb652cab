// Mixture-of-experts decode step on MXFP4 expert weights (T <= 64 tokens, E <= 256 experts, top_k <= 8): the grouped GEMM's kernel
// over e2m1 nibbles with one e8m0 scale byte per expert, output channel and 32 k; the C-ABI entry points mio_moe_up_w4,
// mio_moe_down_w4 and their host queries (semantics: include/mio_hip.h).  This file owns the K-loop kernel of the
// half-byte form and the entry points' argument marshalling.  Everything else is shared with the 16-bit and e4m3fn units (moe.hip,
// moe_w8.hip): the launch's arguments, the checks, the host queries, both launches and up's reduction are moe_gemm_common.h's under
// the form SKINNY_W4 and MOE_SCALES_BLOCK, an expert's rows description is moe_rows_head.inc / moe_rows_gather.inc, down's finishing
// launch is moe_common.h's with SCALED = false, the plan is moe_plan.h's, the router is moe.hip's.  The K loop is the MXFP4
// decode-step GEMM's (gemm_skinny_w4_head.inc, gemm_skinny_w4_loop.inc): the block scales go in inside the conversion, so they
// travel in the launch's arguments to this kernel and to nothing behind it; partials are finished fp32 sums by sorted position and
// the epilogues are the 16-bit unit's.  bf16 only, as the dense unit (gemm_skinny_w4.hip) says.
//
// The kernel.  Grid (ceil(N / 64), slices, E).  A workgroup whose expert has no rows returns before any weight or scale load and
// before any barrier: an idle expert's weight bytes and scale bytes are never read.
//
// What keeps every load in bounds: what gemm_skinny_w4.hip lists, in expert e < E's weight at e * expert_stride and scales at
// e * scale_expert_stride (multiples of 16 and of 4 bytes); a gathered row index is clamped into [0, T - 1] (up) or is a sorted
// position < T k (down); biases are read at (e, min(n, N - 1)) of an expert that has rows.
#include "moe_gemm_common.h"

constexpr SkinnyForm FORM = SKINNY_W4;  // this unit's weight form (gemm_skinny_plan.h)

template <typename T, int MF, bool GLU>
__global__ __launch_bounds__(256) void moe_gemm_w4_kernel(const MoeDev<MOE_SCALES_BLOCK> p) {
#include "moe_rows_head.inc"
  const auto wscale = [&] { return p.scale + (int64_t)e * p.sstride; };
  const auto wscale_g = [&] { return p.scale_g + (int64_t)e * p.sstride; };
#include "gemm_skinny_w4_head.inc"
#include "moe_rows_gather.inc"
#include "gemm_skinny_w4_loop.inc"

  if (!active) return;
  const int n = n0 + 4 * q;
  if (n >= p.N) return;
  // lane (c, q): rows 16 mf + c of the expert, i.e. sorted positions r0 + 16 mf + c, columns n .. n + 3
  skinny_write<T, MF, GLU, false>(moe_finish_args<MOE_SCALES_BLOCK>(p, e), p.ws, p.nsplit, p.rows, s, c, n, r0, cnt, acc, accg);
}

// bf16 only: the fp16 rows of the table stay empty, and every launch refuses fp16 before it reads the table
static const MoeKernelTable<MOE_SCALES_BLOCK> KERNELS = {
    {{MOE_KERNELS(moe_gemm_w4_kernel, __bf16, true, MOE_SCALES_BLOCK), MOE_KERNELS(moe_gemm_w4_kernel, __bf16, false, MOE_SCALES_BLOCK)},
     {}},
    {moe_down_finish_kernel<__bf16, 3, false>, nullptr}};

// ---- the C ABI: argument marshalling over moe_gemm_common.h's host side ---------------------------------------------------------
extern "C" int mio_moe_up_w4_splits(int32_t T, int32_t top_k, int32_t E, int32_t N, int32_t K, int32_t act) {
  return moe_query_splits(FORM, "mio_moe_up_w4_splits", T, top_k, E, N, K, act);
}

extern "C" size_t mio_moe_up_w4_workspace_bytes(int32_t T, int32_t top_k, int32_t E, int32_t N, int32_t K, int32_t act) {
  return moe_query_workspace_bytes(FORM, "mio_moe_up_w4_workspace_bytes", false, T, top_k, E, N, K, act);
}

extern "C" int mio_moe_down_w4_splits(int32_t T, int32_t top_k, int32_t E, int32_t N, int32_t K) {
  return moe_query_splits(FORM, "mio_moe_down_w4_splits", T, top_k, E, N, K, MIO_ACT_NONE);
}

extern "C" size_t mio_moe_down_w4_workspace_bytes(int32_t T, int32_t top_k, int32_t E, int32_t N, int32_t K) {
  return moe_query_workspace_bytes(FORM, "mio_moe_down_w4_workspace_bytes", true, T, top_k, E, N, K, MIO_ACT_NONE);
}

extern "C" int mio_moe_up_w4(const void* x, const void* w4_up, const void* s_up, const void* b_up, const void* w4_gate,
                             const void* s_gate, const void* b_gate, const int32_t* expert_offsets, const int32_t* sorted_rows,
                             void* h, void* workspace, int32_t T, int32_t top_k, int32_t E, int32_t I, int32_t d, int64_t ldx,
                             int64_t ldw, int64_t expert_stride, int64_t lds, int64_t scale_expert_stride, int64_t ldh, int32_t act,
                             int32_t dtype, void* stream) {
  return moe_run_up(FORM, KERNELS, "mio_moe_up_w4", x, w4_up, s_up, b_up, w4_gate, s_gate, b_gate, expert_offsets, sorted_rows, h,
                    workspace, T, top_k, E, I, d, ldx, ldw, expert_stride, ldh, act, dtype, stream, lds, scale_expert_stride);
}

extern "C" int mio_moe_down_w4(const void* h, const void* w4_down, const void* s_down, const void* b_down, const int32_t* ids,
                               const float* weights, const int32_t* expert_offsets, const int32_t* row_pos, const void* residual,
                               void* y, void* workspace, int32_t T, int32_t top_k, int32_t E, int32_t d, int32_t I, int64_t ldh,
                               int64_t ldw, int64_t expert_stride, int64_t lds, int64_t scale_expert_stride, int64_t ldy, int64_t ldr,
                               int32_t dtype, void* stream) {
  return moe_run_down(FORM, KERNELS, "mio_moe_down_w4", h, w4_down, s_down, b_down, ids, weights, expert_offsets, row_pos, residual,
                      y, workspace, T, top_k, E, d, I, ldh, ldw, expert_stride, ldy, ldr, dtype, stream, lds, scale_expert_stride);
}

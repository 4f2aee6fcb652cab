// Mixture-of-experts decode step on weight-only FP8 expert weights (T <= 64 tokens, E <= 256 experts, top_k <= 8): the grouped
// GEMM's kernel over e4m3fn weight bytes with one fp32 scale per expert and output channel; the C-ABI entry points
// mio_moe_up_w8, mio_moe_down_w8 and their host queries (semantics: include/mio_hip.h).  This file owns the K-loop
// kernel of the one-byte form and the entry points' argument marshalling.  Everything else is shared with the 16-bit unit
// (moe.hip): the launch's arguments, the checks, the host queries, both launches and up's reduction are moe_gemm_common.h's under
// the form SKINNY_W8 and SCALED = true, an expert's rows description is moe_rows_head.inc / moe_rows_gather.inc, down's finishing
// launch is moe_common.h's with SCALED = true, the plan is moe_plan.h's.  The router is moe.hip's: the routing arrays are read as
// mio_moe_route wrote them.  The K loop is the FP8 decode-step GEMM's (gemm_skinny_w8_head.inc, gemm_skinny_w8_loop.inc); the
// slice range, the slice sum, the partial store and the epilogue are gemm_skinny_plan.h's skinny_slice_range and
// gemm_skinny_common.h's skinny_slice_sum, skinny_write and skinny_finish<.., SCALED = true>, the ones gemm_skinny_w8.hip runs.
// Every e4m3fn value is exact in bf16 and fp16: the bytes are widened in registers at scale 1 (kv8_to_x8) and multiplied on the
// 16-bit MFMA.  FP8 is a storage form of the expert weights here, not a compute precision.
//
// The kernel.  Grid (ceil(N / 64), slices, E).  A workgroup reads offsets[e], offsets[e + 1], clamped into [0, T k], and returns
// at once when its expert has no rows: before any weight load and before any barrier, the same for all its threads.  The x stage
// gathers rows through sorted_rows (up: routed row / top_k is the token) or by sorted position (down: h is stored that way); rows
// past the expert's count are zeros that are never read from memory.  The kernel is built for the host's bound on an expert's
// rows, MF = ceil(T / 16) fragments; a workgroup stores to LDS and multiplies only the nf = ceil(count / 16) fragments its expert
// reaches.  The k mapping, the x stage and the register ring of SKINNY_W8.sets(GLU) chunks are the loop's (gemm_skinny_w8_loop.inc).
// The scales stay out of the K loop; partials are unscaled fp32 sums by sorted position.  The epilogues apply z = fma(sum,
// scale[e, n], bias[e, n]): up's in the first kernel with one slice, up's reduce launch, and down's finishing launch, where the
// scale of the slot's expert goes in before the routing weight.
//
// What keeps every load in bounds (K % 16 == 0, ldw % 16 == 0 and expert_stride % 16 == 0 in bytes, ldw >= K):
//   * a weight load is issued only for k < ke <= K, k a multiple of 16: its 16 bytes end at or before K;
//   * the weight row is min(n0 + c, N - 1) of expert e < E: a lane past the last column computes a copy of the last row and
//     stores nothing;
//   * x rows past the expert's count and x pieces at k >= ke are zeros written to LDS, never read from memory; a gathered row
//     index is clamped into [0, T - 1] (up) or is a sorted position < T k (down); weight bytes not loaded are 0x00, which is +0.0,
//     so no padding byte of any operand reaches a product;
//   * scales and biases are read at (e, min(n, N - 1)) of an expert that has rows.
#include "kv8_cvt.h"
#include "moe_gemm_common.h"

constexpr SkinnyForm FORM = SKINNY_W8;  // this unit's weight form (gemm_skinny_plan.h)

template <typename T, int MF, bool GLU>
__global__ __launch_bounds__(256) void moe_gemm_w8_kernel(const MoeDev<MOE_SCALES_CHANNEL> p) {
#include "moe_rows_head.inc"
#include "gemm_skinny_w8_head.inc"
#include "moe_rows_gather.inc"
#include "gemm_skinny_w8_loop.inc"

  if (!active) return;
  const int n = n0 + 4 * q;
  if (n >= p.N) return;
  // lane (c, q): rows 16 mf + c of the expert, i.e. sorted positions r0 + 16 mf + c, columns n .. n + 3: unscaled partials, or
  // the scaled epilogue with the expert's scale and bias rows
  skinny_write<T, MF, GLU, true>(moe_finish_args<MOE_SCALES_CHANNEL>(p, e), p.ws, p.nsplit, p.rows, s, c, n, r0, cnt, acc, accg);
}

static const MoeKernelTable<MOE_SCALES_CHANNEL> KERNELS = MOE_KERNEL_TABLE(moe_gemm_w8_kernel, 2, MOE_SCALES_CHANNEL);

// ---- the C ABI: argument marshalling over moe_gemm_common.h's host side ---------------------------------------------------------
extern "C" int mio_moe_up_w8_splits(int32_t T, int32_t top_k, int32_t E, int32_t N, int32_t K, int32_t act) {
  return moe_query_splits(FORM, "mio_moe_up_w8_splits", T, top_k, E, N, K, act);
}

extern "C" size_t mio_moe_up_w8_workspace_bytes(int32_t T, int32_t top_k, int32_t E, int32_t N, int32_t K, int32_t act) {
  return moe_query_workspace_bytes(FORM, "mio_moe_up_w8_workspace_bytes", false, T, top_k, E, N, K, act);
}

extern "C" int mio_moe_down_w8_splits(int32_t T, int32_t top_k, int32_t E, int32_t N, int32_t K) {
  return moe_query_splits(FORM, "mio_moe_down_w8_splits", T, top_k, E, N, K, MIO_ACT_NONE);
}

extern "C" size_t mio_moe_down_w8_workspace_bytes(int32_t T, int32_t top_k, int32_t E, int32_t N, int32_t K) {
  return moe_query_workspace_bytes(FORM, "mio_moe_down_w8_workspace_bytes", true, T, top_k, E, N, K, MIO_ACT_NONE);
}

extern "C" int mio_moe_up_w8(const void* x, const void* w8_up, const float* s_up, const void* b_up, const void* w8_gate,
                             const float* s_gate, const void* b_gate, const int32_t* expert_offsets, const int32_t* sorted_rows,
                             void* h, void* workspace, int32_t T, int32_t top_k, int32_t E, int32_t I, int32_t d, int64_t ldx,
                             int64_t ldw, int64_t expert_stride, int64_t ldh, int32_t act, int32_t dtype, void* stream) {
  return moe_run_up(FORM, KERNELS, "mio_moe_up_w8", x, w8_up, s_up, b_up, w8_gate, s_gate, b_gate, expert_offsets, sorted_rows, h,
                    workspace, T, top_k, E, I, d, ldx, ldw, expert_stride, ldh, act, dtype, stream);
}

extern "C" int mio_moe_down_w8(const void* h, const void* w8_down, const float* s_down, const void* b_down, const int32_t* ids,
                               const float* weights, const int32_t* expert_offsets, const int32_t* row_pos, const void* residual,
                               void* y, void* workspace, int32_t T, int32_t top_k, int32_t E, int32_t d, int32_t I, int64_t ldh,
                               int64_t ldw, int64_t expert_stride, int64_t ldy, int64_t ldr, int32_t dtype, void* stream) {
  return moe_run_down(FORM, KERNELS, "mio_moe_down_w8", h, w8_down, s_down, b_down, ids, weights, expert_offsets, row_pos, residual,
                      y, workspace, T, top_k, E, d, I, ldh, ldw, expert_stride, ldy, ldr, dtype, stream);
}

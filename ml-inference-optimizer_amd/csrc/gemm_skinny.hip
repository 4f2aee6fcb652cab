// Decode-step GEMM (1 <= M <= 64): y[M,N] = act(x[M,K] w[N,K]^T + bias) (+ residual), SwiGLU with a second weight; the C-ABI
// entry points mio_gemm_skinny* (include/mio_hip.h).  This file is the kernel's K loop and the entry points' argument marshalling:
// the plan (shape checks, split of K, workspace, tuning values) is gemm_skinny_plan.h under the form SKINNY_W16, and the launch's
// checks, the launcher, the host queries, the epilogue and the reduction are gemm_skinny_common.h, all shared with the fp8-weight
// unit (gemm_skinny_w8.hip).
//
// A decode step's linear layers stream their weights from HBM once and do almost no arithmetic on them, so the kernel is built
// as the decode attention kernels are: many workgroups with loads in flight, none of them waiting on another.
//   * v_mfma_f32_16x16x32 with a 16-row x 32-k WEIGHT fragment as the A operand, loaded straight from the row-major [N, K] weight
//     into VGPRs in 16-byte pieces (lane (c, q) = (lane & 15, lane >> 4): row n0 + c, k + 8 q): no LDS round trip for the operand
//     that is read once.  One chunk of K (SKC k) of loads is issued while the chunk before it is multiplied.
//   * 16 activation rows are the B operand; M is padded to MF = 1 .. 4 row fragments.  The x slice of a chunk is staged once per
//     workgroup through LDS in whole rows (consecutive lanes, consecutive 16-byte pieces), rows >= M and k past the slice as
//     zeros that are never read from memory; 16-byte piece p of row r sits at p ^ (r & 15), so the fragment read (16 rows x 4
//     pieces per ds_read_b128) spreads over all banks.
//   * accumulator: lane (c, q) holds row m = 16 mf + c and the 4 consecutive columns n0 + 4 q + (0..3).
//   * split-K in two launches, as decode does it: workgroup (column tile, slice) writes fp32 partials [nsplit][M][N], and
//     gemm_skinny_reduce_kernel sums the slices in index order, applies the epilogue and rounds once.  With one slice the first
//     kernel runs the same epilogue itself.  No atomics, counters or barriers between workgroups: results are bit-reproducible.
#include "gemm_skinny_common.h"

constexpr SkinnyForm FORM = SKINNY_W16;  // this unit's weight form (gemm_skinny_plan.h)

// The K loop itself is gemm_skinny_w16_head.inc + gemm_skinny_w16_loop.inc, shared with the mixture-of-experts unit (moe.hip).
// The dense rows description: the weight starts at p.w, all MF fragments are live, staged row r < M is row r of x.
template <typename T, int MF, bool GLU>
__global__ __launch_bounds__(256) void gemm_skinny_kernel(const SkinnyDev p) {
  const auto wbase = [] { return (int64_t)0; };
#include "gemm_skinny_w16_head.inc"
  constexpr int nf = MF;
  constexpr bool all_live = true;
  const auto xhas = [&](int, int r) { return r < p.M; };
  const auto xrow = [](int, int r) { return r; };
#include "gemm_skinny_w16_loop.inc"

  if (!active) return;
  const int n = n0 + 4 * q;
  if (n >= p.N) return;
  skinny_write<T, MF, GLU, false>(skinny_finish_args(p), p.ws, p.nsplit, p.M, s, c, n, 0, p.M, acc, accg);
}

#define SKINNY_KERNELS(T, GLU)                                                                                        \
  {{gemm_skinny_kernel<T, 1, GLU>, gemm_skinny_kernel<T, 2, GLU>, gemm_skinny_kernel<T, 3, GLU>, gemm_skinny_kernel<T, 4, GLU>}, \
   gemm_skinny_reduce_kernel<T, GLU, false>}
static const SkinnyKernelTable KERNELS = {{SKINNY_KERNELS(__bf16, true), SKINNY_KERNELS(__bf16, false)},
                                          {SKINNY_KERNELS(_Float16, true), SKINNY_KERNELS(_Float16, false)}};
#undef SKINNY_KERNELS

// ---- the C ABI: argument marshalling over gemm_skinny_common.h's host side -------------------------------------------
extern "C" int mio_gemm_skinny_splits(int64_t M, int32_t N, int32_t K, int32_t act) {
  return skinny_query_splits(FORM, "mio_gemm_skinny_splits", M, N, K, act);
}

extern "C" size_t mio_gemm_skinny_workspace_bytes(int64_t M, int32_t N, int32_t K, int32_t act) {
  return skinny_query_workspace_bytes(FORM, "mio_gemm_skinny_workspace_bytes", M, N, K, act);
}

extern "C" int mio_gemm_skinny_slice(int64_t M, int32_t N, int32_t K, int32_t act, int32_t slice, int32_t* k_begin, int32_t* k_end) {
  return skinny_query_slice(FORM, "mio_gemm_skinny_slice", M, N, K, act, slice, k_begin, k_end);
}

extern "C" int mio_gemm_skinny_chunk_k(int32_t act) { return skinny_query_chunk_k(FORM, "mio_gemm_skinny_chunk_k", act); }

extern "C" int mio_gemm_skinny_ok(int64_t M, int32_t N, int32_t K, int32_t act) {
  return skinny_query_ok(FORM, "mio_gemm_skinny_ok", M, N, K, act);
}

extern "C" int mio_gemm_skinny(const void* x, const void* w, const void* bias, const void* w_gate, const void* bias_gate,
                               const void* residual, void* y, void* workspace, int64_t M, int32_t N, int32_t K, int64_t ldx,
                               int64_t ldw, int64_t ldy, int64_t ldr, int32_t act, int32_t dtype, void* stream) {
  return skinny_run(FORM, KERNELS, x, w, nullptr, bias, w_gate, nullptr, bias_gate, residual, y, workspace, M, N, K, ldx, ldw, ldy,
                    ldr, act, dtype, stream);
}


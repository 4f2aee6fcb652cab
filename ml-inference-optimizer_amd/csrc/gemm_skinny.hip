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
constexpr int SKINNY_KSTEP = FORM.kstep;
static_assert(FORM.sets(false) == 2 && FORM.sets(true) == 2, "the K loop below is double-buffered");

template <typename T, int MF, bool GLU>
__global__ __launch_bounds__(256) void gemm_skinny_kernel(const SkinnyDev p) {
  using X8 = typename DT<T>::x8;
  constexpr int SKC = FORM.chunk(GLU);  // k per chunk
  constexpr int KS = SKC / SKINNY_KSTEP, PCS = SKC / 8, ROWS = MF * 16, ROWB = SKC * 2;
  constexpr int XPT = ROWS * PCS / 256;  // 16-byte pieces of the x chunk per thread
  static_assert(PCS >= 16 && ROWS * PCS % 256 == 0, "chunk shape");
  __shared__ __attribute__((aligned(16))) char sx[2][ROWS * ROWB];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, q = lane >> 4;
  const int n0 = blockIdx.x * SKINNY_BN + wave * 16;
  const bool active = n0 < p.N;  // (a wave past the last column stages x and keeps the barriers, nothing else)
  const int s = blockIdx.y;
  const int kb = (int)((int64_t)s * p.steps / p.nsplit) * SKINNY_KSTEP;
  const int ke = min(p.K, (int)((int64_t)(s + 1) * p.steps / p.nsplit) * SKINNY_KSTEP);
  const int nc = (ke - kb + SKC - 1) / SKC;

  const int nrow = min(n0 + c, p.N - 1);
  const T* wrow = (const T*)p.w + (int64_t)nrow * p.ldw;
  const T* grow = GLU ? (const T*)p.wg + (int64_t)nrow * p.ldw : nullptr;
  const T* xg = (const T*)p.x;

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
      if (row < p.M && k < ke) v[i] = *(const u32x4_t*)(xg + (int64_t)row * p.ldx + k);
    }
#pragma unroll
    for (int i = 0; i < XPT; ++i) {
      const int idx = tid + i * 256, row = idx / PCS, pc = idx % PCS;
      *(u32x4_t*)(sx[buf] + row * ROWB + ((pc ^ (row & 15)) * 16)) = v[i];
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
        const X8 xf = __builtin_bit_cast(X8, *(const u32x4_t*)(sx[buf] + (mf * 16 + c) * ROWB + (((ks * 4 + q) ^ c) * 16)));
        acc[mf] = DT<T>::mfma16(__builtin_bit_cast(X8, wr[ks]), xf, acc[mf]);
        if constexpr (GLU) accg[mf] = DT<T>::mfma16(__builtin_bit_cast(X8, gr[ks]), xf, accg[mf]);
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

  if (!active) return;
  const int n = n0 + 4 * q;
  if (n >= p.N) return;
  skinny_write<T, MF, GLU, false>(p, s, c, n, acc, accg);
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


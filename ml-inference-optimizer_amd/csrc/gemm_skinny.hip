// Decode-step GEMM (1 <= M <= 64): y[M,N] = act(x[M,K] w[N,K]^T + bias) (+ residual), SwiGLU with a second weight; the C-ABI
// entry points mio_gemm_skinny* (include/mio_hip.h).  The plan (checks, split of K, workspace) is gemm_skinny_plan.h.
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
//     The epilogue, the partial stores and the reduction are gemm_skinny_common.h, shared with the fp8-weight unit.
#include <string>

#include "gemm_skinny_common.h"
#include "gemm_skinny_plan.h"

template <typename T, int MF, bool GLU>
__global__ __launch_bounds__(256) void gemm_skinny_kernel(const SkinnyDev p) {
  using X8 = typename DT<T>::x8;
  constexpr int SKC = GLU ? SKINNY_CHUNK_K_GLU : SKINNY_CHUNK_K;  // k per chunk (gemm_skinny_plan.h)
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

template <typename T, int MF, bool GLU>
static void skinny_launch_mf(const SkinnyDev& p, const SkinnyPlan& pl, hipStream_t st) {
  hipLaunchKernelGGL((gemm_skinny_kernel<T, MF, GLU>), dim3((unsigned)pl.tiles_n, (unsigned)pl.nsplit), dim3(256), 0, st, p);
}

template <typename T, bool GLU>
static void skinny_launch(const SkinnyDev& p, const SkinnyPlan& pl, hipStream_t st) {
  switch (pl.mf) {
    case 1: skinny_launch_mf<T, 1, GLU>(p, pl, st); break;
    case 2: skinny_launch_mf<T, 2, GLU>(p, pl, st); break;
    case 3: skinny_launch_mf<T, 3, GLU>(p, pl, st); break;
    default: skinny_launch_mf<T, 4, GLU>(p, pl, st); break;
  }
  if (pl.nsplit > 1) {
    const int64_t threads = (int64_t)p.M * ((p.N + 3) / 4);
    hipLaunchKernelGGL((gemm_skinny_reduce_kernel<T, GLU>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, p);
  }
}

// ---- host queries ------------------------------------------------------------------------------------------------------
extern "C" int mio_gemm_skinny_splits(int64_t M, int32_t N, int32_t K, int32_t act) {
  std::string err;
  if (!skinny_shape_ok("mio_gemm_skinny_splits", M, N, K, act, err)) return mio_fail(err);
  return skinny_plan(M, N, K, act).nsplit;
}

extern "C" size_t mio_gemm_skinny_workspace_bytes(int64_t M, int32_t N, int32_t K, int32_t act) {
  std::string err;
  if (!skinny_shape_ok("mio_gemm_skinny_workspace_bytes", M, N, K, act, err)) {
    mio_set_error(err);
    return 0;
  }
  return skinny_workspace_bytes(skinny_plan(M, N, K, act), M, N);
}

extern "C" int mio_gemm_skinny_slice(int64_t M, int32_t N, int32_t K, int32_t act, int32_t slice, int32_t* k_begin, int32_t* k_end) {
  std::string err;
  if (!skinny_shape_ok("mio_gemm_skinny_slice", M, N, K, act, err)) return mio_fail(err);
  const SkinnyPlan pl = skinny_plan(M, N, K, act);
  MIO_CHECK(k_begin && k_end && slice >= 0 && slice < pl.nsplit, "mio_gemm_skinny_slice: slice must be in [0, mio_gemm_skinny_splits)");
  skinny_slice(pl, K, slice, *k_begin, *k_end);
  return 0;
}

extern "C" int mio_gemm_skinny_chunk_k(int32_t act) {
  std::string err;
  if (!skinny_shape_ok("mio_gemm_skinny_chunk_k", 0, 0, 0, act, err)) return mio_fail(err);
  return act == MIO_ACT_SWIGLU ? SKINNY_CHUNK_K_GLU : SKINNY_CHUNK_K;
}

extern "C" int mio_gemm_skinny_ok(int64_t M, int32_t N, int32_t K, int32_t act) {
  std::string err;
  return (skinny_shape_ok("mio_gemm_skinny_ok", M, N, K, act, err) && skinny_advised(M, N, K, act)) ? 1 : 0;
}

// ---- launch ------------------------------------------------------------------------------------------------------------
extern "C" int mio_gemm_skinny(const void* x, const void* w, const void* bias, const void* w_gate, const void* bias_gate,
                               const void* residual, void* y, void* workspace, int64_t M, int32_t N, int32_t K, int64_t ldx,
                               int64_t ldw, int64_t ldy, int64_t ldr, int32_t act, int32_t dtype, void* stream) {
  const char* who = "mio_gemm_skinny";
#define SKINNY_CHECK(cond, text) MIO_CHECK(cond, std::string(who) + (text))
  std::string err;
  if (!skinny_shape_ok(who, M, N, K, act, err)) return mio_fail(err);
  SKINNY_CHECK(dtype == MIO_BF16 || dtype == MIO_FP16, ": dtype must be bf16 or fp16");
  const bool glu = act == MIO_ACT_SWIGLU;
  SKINNY_CHECK(glu == (w_gate != nullptr), ": w_gate is required iff act == SWIGLU");
  SKINNY_CHECK(glu || bias_gate == nullptr, ": bias_gate belongs to act == SWIGLU");
  SKINNY_CHECK(ldx % 8 == 0 && ldw % 8 == 0 && ldy % 8 == 0 && (!residual || ldr % 8 == 0), ": row strides must be multiples of 8 elements");
  SKINNY_CHECK(ldx >= K && ldw >= K && ldy >= N && (!residual || ldr >= N), ": row stride smaller than row length");
  SKINNY_CHECK(w && (M == 0 || (x && y)), ": x, w, y must be non-null");
  SKINNY_CHECK(mio_aligned16(x) && mio_aligned16(w) && mio_aligned16(y) && mio_aligned16(w_gate) && mio_aligned16(residual) &&
                   mio_aligned16(bias) && mio_aligned16(bias_gate) && mio_aligned16(workspace),
               ": pointers must be 16-byte aligned");
  const SkinnyPlan pl = skinny_plan(M, N, K, act);
  if (M == 0 || N == 0) return 0;
  SKINNY_CHECK(pl.nsplit == 1 || workspace != nullptr, ": workspace required (mio_gemm_skinny_workspace_bytes) when the plan splits K");
#undef SKINNY_CHECK
  SkinnyDev p;
  p.x = x; p.w = w; p.wg = w_gate; p.bias = bias; p.bias_g = bias_gate; p.res = residual; p.y = y;
  p.ws = pl.nsplit > 1 ? (float*)workspace : nullptr;
  p.scale = nullptr; p.scale_g = nullptr;
  p.ldx = ldx; p.ldw = ldw; p.ldy = ldy; p.ldr = ldr;
  p.M = (int)M; p.N = N; p.K = K; p.act = act; p.nsplit = pl.nsplit; p.steps = pl.steps;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == MIO_BF16) {
    if (glu) skinny_launch<__bf16, true>(p, pl, st); else skinny_launch<__bf16, false>(p, pl, st);
  } else {
    if (glu) skinny_launch<_Float16, true>(p, pl, st); else skinny_launch<_Float16, false>(p, pl, st);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mio_fail(std::string("mio_gemm_skinny launch: ") + hipGetErrorString(e));
  return 0;
}

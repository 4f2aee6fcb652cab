// FP8 x FP8 GEMM for tall inputs (W8A8) on gfx950's v_mfma_f32_16x16x128_f8f6f4:
//   z[m, n] = (x_scale[m] * w_scale[n]) * sum_k x8[m, k] w8[n, k] + bias[n],   y = round16(act(z) + residual)
//   SwiGLU: y = round16(silu(z_gate) * z_up + residual), the gate with its own bytes, scales and bias.
// x8 [M, K] and w8 [N, K] are OCP e4m3fn bytes, row-major: x8 with one fp32 scale per row (mio_weight_quant_w8 on the activation
// matrix: per-token dynamic quantisation), w8 with one per output column (the copy mio_gemm_skinny_w8 reads; nothing is
// pre-permuted).  The C-ABI entry points mio_gemm_f8, mio_gemm_f8_ok, mio_gemm_f8_route (include/mio_hip.h); the plan is
// gemm_f8_plan.h.  The activations and the packing are gemm_kernel.h's / gemm_skinny_common.h's (gemm_act, skinny_act, pack2).
//
//   * One workgroup per 256 x 256 tile (SwiGLU: 256 rows x 128 columns, the weight tile 128 gate + 128 up rows), 512 threads =
//     8 waves as 2 (rows) x 4 (weight rows); a wave owns 128 x 64: 8 x 4 fragments of 16 x 16, 128 accumulator registers.  The
//     tile order over the grid is gemm_tile_coords.
//   * K step = 128 bytes = one MFMA deep.  Global -> registers -> LDS: thread t carries the 16-byte chunk t & 7 of the rows
//     (t >> 3) + 64 i, i < 4, of both tiles (8 lanes read the 128 contiguous bytes of a row).  A chunk is loaded only if its row
//     is below M (N) and its 16 bytes end at or before K (K % 16 == 0); otherwise the registers hold zeros, 0x00 = +0.0, and
//     nothing is read: rows past the edge and the K tail never touch memory the launch does not own.
//   * Two LDS stages of 64 KiB (x tile 32 KiB + weight tile 32 KiB) and the third step in flight in registers: step s + 1 is
//     stored to the other stage at the top of step s (its loads were issued a whole step earlier), then the loads of step s + 2
//     are issued, then step s is multiplied.  One barrier per step.  Three LDS stages would be 192 KiB of the CU's 160.
//   * LDS rows are 128 bytes: chunk c of row r is stored at c ^ ((r >> 1) & 7).  The 16 lanes of a fragment read (16 rows, one
//     chunk) and the 16 lanes of a store (2 rows, 8 chunks) then cover the 64 banks once.
//   * Fragments.  Lane (c, q) = (lane & 15, lane >> 4) reads row c of the fragment and the chunks 2 q, 2 q + 1 of the step: bytes
//     32 q .. 32 q + 31 as its 8 dwords, the same for both operands (an MFMA sums over the (lane group, byte) slots; which k sits
//     in a slot is free as long as both operands agree).  The WEIGHT fragment is the A operand: acc[i] of lane (c, q) is then
//     output row m = c and column n = 4 q + i of the fragment, so the read-out is lane-local and stores 8-byte row pieces.
//   * SwiGLU.  Tile weight row wn * 64 + h * 32 + j comes from (h ? w8 : w8_gate)[n0 + wn * 32 + j]: a wave's fragments 0, 1 are
//     the gate and 2, 3 the up accumulators of the same 32 columns, in the same lanes.  Address arithmetic in the loader only.
//   * Read-out: s = x_scale[m] * w_scale[n] (one fp32 product), z = fma(acc, s, bias), activation, residual, one rounding.  No
//     split of K, no atomics: bit-identical reruns, graph-capturable.  Scales and biases are read element by element at clamped
//     owned indices; y and the residual in 8-byte pieces where four columns are below N.
#include <mutex>

#include "gemm_f8_plan.h"
#include "gemm_skinny_common.h"

typedef __attribute__((ext_vector_type(8))) int i32x8_t;

struct F8Dev {
  const uint8_t* x;
  const uint8_t* w;
  const uint8_t* wg;
  const float* xs;
  const float* ws;
  const float* wsg;
  const void* bias;
  const void* bias_g;
  const void* res;
  void* y;
  int64_t M, ldx, ldw, ldy, ldr;
  int N, K, act, steps, tiles_m, tiles_n;
};

constexpr int F8_CPT = F8_TILE_BYTES / 16 / F8_NT;  // 16-byte chunks of one tile per thread (4), 64 rows apart
constexpr int F8_MF = 8, F8_NF = 4;                 // a wave's fragments: rows of x, weight rows

template <typename T, bool GLU>
__global__ __launch_bounds__(F8_NT) void gemm_f8_kernel(const F8Dev p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int c = lane & 15, q = lane >> 4;
  int tm, tn;
  gemm_tile_coords(blockIdx.x, p.tiles_m, p.tiles_n, tm, tn);
  const int64_t m0 = (int64_t)tm * F8_BM;
  const int n0 = tn * (GLU ? F8_BN_GLU : F8_BN);

  // ---- the loader: chunk lc of tile rows lr + 64 i ------------------------------------------------------------------
  const int lr = tid >> 3, lc = tid & 7;
  const uint8_t* xsrc = p.x + (m0 + lr) * p.ldx + 16 * lc;
  // weight row of tile row lr + 64 i: plain n0 + lr + 64 i; SwiGLU n0 + 32 i + (lr & 31) of the gate (lr < 32) or the up weight
  const int nrow = GLU ? n0 + (lr & 31) : n0 + lr;
  constexpr int NSTEP = GLU ? 32 : 64;
  const uint8_t* wsrc = ((GLU && lr < 32) ? p.wg : p.w) + (int64_t)nrow * p.ldw + 16 * lc;
  const int st_off = lr * F8_BK + ((lc ^ ((lr >> 1) & 7)) << 4);  // (64 i rows further down the swizzle term is the same)

  auto load = [&](u32x4_t (&xr)[F8_CPT], u32x4_t (&wr)[F8_CPT], int step) {
    const bool kok = step * F8_BK + 16 * lc < p.K;
#pragma unroll
    for (int i = 0; i < F8_CPT; ++i) {
      xr[i] = (u32x4_t){0u, 0u, 0u, 0u};
      wr[i] = (u32x4_t){0u, 0u, 0u, 0u};
      if (kok && m0 + lr + 64 * i < p.M) xr[i] = *(const u32x4_t*)(xsrc + (int64_t)(64 * i) * p.ldx + step * F8_BK);
      if (kok && nrow + NSTEP * i < p.N) wr[i] = *(const u32x4_t*)(wsrc + (int64_t)(NSTEP * i) * p.ldw + step * F8_BK);
    }
  };
  auto put = [&](const u32x4_t (&xr)[F8_CPT], const u32x4_t (&wr)[F8_CPT], int stage) {
    char* base = smem + stage * F8_STAGE_BYTES + st_off;
#pragma unroll
    for (int i = 0; i < F8_CPT; ++i) {
      *(u32x4_t*)(base + i * 64 * F8_BK) = xr[i];
      *(u32x4_t*)(base + F8_TILE_BYTES + i * 64 * F8_BK) = wr[i];
    }
  };

  // ---- the fragments: row c, chunks 2 q and 2 q + 1 -----------------------------------------------------------------
  const int sw = (c >> 1) & 7;  // (fragment rows start at multiples of 16: the swizzle term is the lane's own)
  const int f_off0 = c * F8_BK + (((2 * q) ^ sw) << 4), f_off1 = c * F8_BK + (((2 * q + 1) ^ sw) << 4);
  auto frag = [&](const char* tile, int row0) {
    const u32x4_t lo = *(const u32x4_t*)(tile + row0 * F8_BK + f_off0);
    const u32x4_t hi = *(const u32x4_t*)(tile + row0 * F8_BK + f_off1);
    return (i32x8_t){(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
  };

  f32x4_t acc[F8_MF][F8_NF];
#pragma unroll
  for (int mf = 0; mf < F8_MF; ++mf)
#pragma unroll
    for (int nf = 0; nf < F8_NF; ++nf) acc[mf][nf] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  auto compute = [&](int stage) {
    const char* xt = smem + stage * F8_STAGE_BYTES + wm * (F8_MF * 16) * F8_BK;
    const char* wt = smem + stage * F8_STAGE_BYTES + F8_TILE_BYTES + wn * (F8_NF * 16) * F8_BK;
    i32x8_t wf[F8_NF];
#pragma unroll
    for (int nf = 0; nf < F8_NF; ++nf) wf[nf] = frag(wt, nf * 16);
#pragma unroll
    for (int mf = 0; mf < F8_MF; ++mf) {
      const i32x8_t xf = frag(xt, mf * 16);
#pragma unroll
      for (int nf = 0; nf < F8_NF; ++nf)
        acc[mf][nf] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf[nf], xf, acc[mf][nf], 0, 0, 0, 0, 0, 0);
    }
  };

  // ---- the K loop: LDS stage s & 1 holds step s, the registers step s + 1 -------------------------------------------
  const int steps = p.steps;
  u32x4_t xr[F8_CPT], wr[F8_CPT];
  if (steps > 0) {
    load(xr, wr, 0);
    put(xr, wr, 0);
    if (steps > 1) load(xr, wr, 1);
    __syncthreads();
  }
  for (int s = 0; s < steps; ++s) {
    // stage (s + 1) & 1 was last read in step s - 1, before the barrier that ended it
    if (s + 1 < steps) put(xr, wr, (s + 1) & 1);
    if (s + 2 < steps) load(xr, wr, s + 2);
    compute(s & 1);
    __syncthreads();
  }

  // ---- the read-out -------------------------------------------------------------------------------------------------
  const T* bias = (const T*)p.bias;
  const T* bias_g = (const T*)p.bias_g;
  int64_t mrow[F8_MF];
  float xs[F8_MF];
#pragma unroll
  for (int mf = 0; mf < F8_MF; ++mf) {
    mrow[mf] = m0 + wm * (F8_MF * 16) + mf * 16 + c;
    xs[mf] = mrow[mf] < p.M ? p.xs[mrow[mf]] : 0.f;
  }
  constexpr int NOUT = GLU ? F8_NF / 2 : F8_NF;  // output fragments of a wave
#pragma unroll
  for (int nf = 0; nf < NOUT; ++nf) {
    const int n = n0 + wn * (NOUT * 16) + nf * 16 + 4 * q;
    if (n >= p.N) continue;
    const bool full = n + 3 < p.N;
    float wsc[4], b[4], gsc[4], bg[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int nn = n + i < p.N ? n + i : p.N - 1;  // (clamped: computed, not stored)
      wsc[i] = p.ws[nn];
      b[i] = bias ? (float)bias[nn] : 0.f;
      if constexpr (GLU) {
        gsc[i] = p.wsg[nn];
        bg[i] = bias_g ? (float)bias_g[nn] : 0.f;
      }
    }
#pragma unroll
    for (int mf = 0; mf < F8_MF; ++mf) {
      if (mrow[mf] >= p.M) continue;
      T* yrow = (T*)p.y + mrow[mf] * p.ldy + n;
      const T* rrow = p.res ? (const T*)p.res + mrow[mf] * p.ldr + n : nullptr;
      float r[4] = {0.f, 0.f, 0.f, 0.f};
      if (rrow) {
        if (full) {
          const typename DT<T>::x4 rv = *(const typename DT<T>::x4*)rrow;
#pragma unroll
          for (int i = 0; i < 4; ++i) r[i] = (float)rv[i];
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (n + i < p.N) r[i] = (float)rrow[i];
        }
      }
      float o[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float z;
        if constexpr (GLU) {
          const float zu = __builtin_fmaf(acc[mf][nf + NOUT][i], xs[mf] * wsc[i], b[i]);
          const float zg = __builtin_fmaf(acc[mf][nf][i], xs[mf] * gsc[i], bg[i]);
          z = gemm_act<MIO_ACT_SILU>(zg) * zu;
        } else {
          z = skinny_act(p.act, __builtin_fmaf(acc[mf][nf][i], xs[mf] * wsc[i], b[i]));
        }
        if (rrow) z += r[i];
        o[i] = z;
      }
      if (full) {
        *(u32x2_t*)yrow = (u32x2_t){pack2<T>(o[0], o[1]), pack2<T>(o[2], o[3])};
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (n + i < p.N) yrow[i] = (T)o[i];
      }
    }
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------------
template <typename T, bool GLU>
static int f8_launch(const F8Dev& p, hipStream_t st) {
  auto kern = gemm_f8_kernel<T, GLU>;
  static std::once_flag once;  // > 64 KiB dynamic LDS needs the opt-in once per kernel
  static hipError_t ea = hipSuccess;
  std::call_once(once, [&] { ea = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, F8_LDS_BYTES); });
  if (ea != hipSuccess) return mio_fail(std::string("mio_gemm_f8: hipFuncSetAttribute: ") + hipGetErrorString(ea));
  hipLaunchKernelGGL(kern, dim3((unsigned)(p.tiles_m * p.tiles_n)), dim3(F8_NT), F8_LDS_BYTES, st, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mio_fail(std::string("mio_gemm_f8 launch: ") + hipGetErrorString(e));
  return 0;
}

static inline bool f8_aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

extern "C" int mio_gemm_f8(const void* x8, int64_t ldx, const float* x_scale, const void* w8, int64_t ldw, const float* w_scale,
                           const void* bias, const void* w8_gate, const float* w_scale_gate, const void* bias_gate,
                           const void* residual, int64_t ldr, void* y, int64_t ldy, int64_t M, int32_t N, int32_t K, int32_t act,
                           int32_t out_dtype, void* stream) {
  const std::string who = "mio_gemm_f8";
  std::string err;
  if (!f8_shape_ok(who.c_str(), M, N, K, act, err)) return mio_fail(err);
  MIO_CHECK(out_dtype == MIO_BF16 || out_dtype == MIO_FP16, who + ": out_dtype must be bf16 or fp16");
  const bool glu = act == MIO_ACT_SWIGLU;
  MIO_CHECK(glu == (w8_gate != nullptr) && glu == (w_scale_gate != nullptr),
            who + ": w8_gate and w_scale_gate are given together, iff act == SWIGLU");
  MIO_CHECK(glu || bias_gate == nullptr, who + ": bias_gate belongs to act == SWIGLU");
  MIO_CHECK(ldx % 16 == 0 && ldw % 16 == 0, who + ": ldx and ldw must be multiples of 16 bytes");
  MIO_CHECK(ldy % 8 == 0 && (!residual || ldr % 8 == 0), who + ": ldy and ldr must be multiples of 8 elements");
  MIO_CHECK(ldx >= K && ldw >= K && ldy >= N && (!residual || ldr >= N), who + ": row stride smaller than row length");
  MIO_CHECK(mio_aligned16(x8) && mio_aligned16(w8) && mio_aligned16(w8_gate) && mio_aligned16(residual) && mio_aligned16(y),
            who + ": x8, w8, w8_gate, residual and y must be 16-byte aligned");
  MIO_CHECK(f8_aligned(x_scale, 4) && f8_aligned(w_scale, 4) && f8_aligned(w_scale_gate, 4) && f8_aligned(bias, 2) &&
                f8_aligned(bias_gate, 2),
            who + ": scales must be 4-byte aligned, biases 2-byte aligned");
  if (M == 0 || N == 0) return 0;
  MIO_CHECK(x8 && x_scale && w8 && w_scale && y, who + ": x8, x_scale, w8, w_scale, y must be non-null");
  const F8Plan pl = f8_plan(M, N, K, act);
  F8Dev p;
  p.x = (const uint8_t*)x8; p.w = (const uint8_t*)w8; p.wg = (const uint8_t*)w8_gate;
  p.xs = x_scale; p.ws = w_scale; p.wsg = w_scale_gate;
  p.bias = bias; p.bias_g = bias_gate; p.res = residual; p.y = y;
  p.M = M; p.ldx = ldx; p.ldw = ldw; p.ldy = ldy; p.ldr = ldr;
  p.N = N; p.K = K; p.act = act; p.steps = pl.steps; p.tiles_m = (int)pl.tiles_m; p.tiles_n = pl.tiles_n;
  hipStream_t st = (hipStream_t)stream;
  if (out_dtype == MIO_BF16) return glu ? f8_launch<__bf16, true>(p, st) : f8_launch<__bf16, false>(p, st);
  return glu ? f8_launch<_Float16, true>(p, st) : f8_launch<_Float16, false>(p, st);
}

extern "C" int mio_gemm_f8_ok(int64_t M, int32_t N, int32_t K, int32_t act) {
  std::string err;
  return (f8_shape_ok("mio_gemm_f8_ok", M, N, K, act, err) && f8_advised(M, N, K, act)) ? 1 : 0;
}

extern "C" const char* mio_gemm_f8_route(int64_t M, int32_t N, int32_t K, int32_t act) {
  std::string err;
  if (!f8_shape_ok("mio_gemm_f8_route", M, N, K, act, err)) {
    mio_set_error(err);
    return nullptr;
  }
  return f8_route_name(M, N, f8_plan(M, N, K, act));
}

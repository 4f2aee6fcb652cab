// Decode-step GEMM on weight-only FP8 (1 <= M <= 64): y[M,N] = act(scale[n] * (x[M,K] w8[N,K]^T) + bias[n]) (+ residual), SwiGLU
// with a second weight and its own scales; and the one-time quantiser that makes (w8, scale) from a 16-bit weight.  The C-ABI
// entry points mio_gemm_skinny_w8* and mio_weight_quant_w8 (include/mio_hip.h).  This file is the kernel's K loop, the quantiser
// and the entry points' argument marshalling: the plan (shape checks, split of K, workspace, tuning values) is gemm_skinny_plan.h
// under the form SKINNY_W8, and the launch's checks, the launcher, the host queries, the epilogue and the reduction are
// gemm_skinny_common.h, all shared with gemm_skinny.hip.  Weights are OCP e4m3fn bytes (torch.float8_e4m3fn), row-major [N, K], with
// one fp32 scale per output column; x, bias, residual and y stay bf16 / fp16.  Every e4m3fn value is exact in bf16 and fp16, so
// the bytes are widened in registers at scale 1 (kv8_to_x8) and multiplied on the 16-bit MFMA: the arithmetic is the 16-bit
// kernel's plus one fp32 fma per output.  FP8 is a storage form of the weights here, not a compute precision.
//
//   * 256 threads, 4 waves x 16 output columns; v_mfma_f32_16x16x32 with the widened weight fragment as the A operand.
//   * The k mapping.  Lane (c, q) = (lane & 15, lane >> 4) loads the 16 bytes of row n0 + c at k0 + 16 q, k0 the begin of a
//     64-k step.  One load feeds two MFMAs: MFMA j (0, 1) takes bytes 8 j .. 8 j + 7, true k = k0 + 16 q + 8 j .. + 7, as the
//     lane's 8 A elements.  Its B operand must be the same true k of x: the 16-byte piece k0 / 8 + 2 q + j of row c, read from
//     LDS.  (An MFMA sums over the 32 (lane group, element) slots; which k sits in a slot is free as long as A and B agree.)
//   * x is staged once per workgroup through LDS in whole rows, 16-byte piece p of row r at p ^ (r & 15), rows >= M and k past
//     the slice as zeros that are never read from memory.  Two LDS buffers, one barrier per chunk.
//   * Loads in flight.  A chunk is the form's chunk_k k (SwiGLU chunk_k_glu); the weight registers are a ring of depth sets, one chunk
//     each, so DEPTH - 1 chunks of loads are outstanding while one is multiplied.  The x pieces of a chunk are loaded into
//     registers immediately BEFORE that chunk's weight loads and stored to LDS only when the chunk is due: the vector memory
//     counter retires loads in issue order, so waiting for an x load issued behind younger weight loads would drain the ring.
//   * accumulator: lane (c, q) holds row m = 16 mf + c and the 4 consecutive columns n0 + 4 q + (0..3).
//   * split-K in two launches: fp32 partials [nsplit][M][N] (SwiGLU: up, then gate), summed in slice order by
//     gemm_skinny_reduce_kernel, which applies the scale, bias, activation and residual and rounds once.  No atomics, counters
//     or waits between workgroups: graph-capturable and bit-reproducible.
//
// What keeps every load in bounds (K % 16 == 0, ldw % 16 == 0 bytes, ldw >= K):
//   * a weight load is issued only for k < ke <= K, k a multiple of 16: its 16 bytes end at or before K;
//   * the weight row is min(n0 + c, N - 1): a lane past the last column computes a copy of the last row and stores nothing;
//   * x rows >= M and x pieces at k >= ke are zeros written to LDS, never read from memory; weight bytes not loaded are 0x00,
//     which is +0.0, so no padding byte of any operand reaches a product.
#include "gemm_skinny_common.h"
#include "kv8_cvt.h"

constexpr SkinnyForm FORM = SKINNY_W8;  // this unit's weight form (gemm_skinny_plan.h)
constexpr int SKW8_KSTEP = FORM.kstep;

template <typename T, int MF, bool GLU>
__global__ __launch_bounds__(256) void gemm_skinny_w8_kernel(const SkinnyDev p) {
  using X8 = typename DT<T>::x8;
  constexpr int SKC = FORM.chunk(GLU);  // k per chunk
  constexpr int D = FORM.sets(GLU);     // register sets in the ring
  constexpr int KS = SKC / SKW8_KSTEP, PCS = SKC / 8, ROWS = MF * 16, ROWB = SKC * 2;
  constexpr int XPT = ROWS * PCS / 256;  // 16-byte pieces of the x chunk per thread
  static_assert(PCS >= 16 && ROWS * PCS % 256 == 0 && SKC % SKW8_KSTEP == 0 && D >= 2, "chunk shape");
  __shared__ __attribute__((aligned(16))) char sx[2][ROWS * ROWB];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, q = lane >> 4;
  const int n0 = blockIdx.x * SKINNY_BN + wave * 16;
  const bool active = n0 < p.N;  // (a wave past the last column stages x and keeps the barriers, nothing else)
  const int s = blockIdx.y;
  int kb, ke;
  skinny_slice_range(p.steps, p.nsplit, SKW8_KSTEP, p.K, s, kb, ke);
  const int nc = (ke - kb + SKC - 1) / SKC;

  const int nrow = min(n0 + c, p.N - 1);
  const uint8_t* wrow = (const uint8_t*)p.w + (int64_t)nrow * p.ldw;
  const uint8_t* grow = GLU ? (const uint8_t*)p.wg + (int64_t)nrow * p.ldw : nullptr;
  const T* xg = (const T*)p.x;

  auto load_w = [&](u32x4_t (&wr)[KS], u32x4_t (&gr)[GLU ? KS : 1], int ch) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int k = kb + ch * SKC + ks * SKW8_KSTEP + 16 * q;
      const bool ok = active && k < ke;
      wr[ks] = (u32x4_t){0u, 0u, 0u, 0u};
      if (ok) wr[ks] = *(const u32x4_t*)(wrow + k);
      if constexpr (GLU) {
        gr[ks] = (u32x4_t){0u, 0u, 0u, 0u};
        if (ok) gr[ks] = *(const u32x4_t*)(grow + k);
      }
    }
  };
  auto load_x = [&](u32x4_t (&v)[XPT], int ch) {
#pragma unroll
    for (int i = 0; i < XPT; ++i) {
      const int idx = tid + i * 256, row = idx / PCS, pc = idx % PCS;
      const int k = kb + ch * SKC + pc * 8;
      v[i] = (u32x4_t){0u, 0u, 0u, 0u};
      if (row < p.M && k < ke) v[i] = *(const u32x4_t*)(xg + (int64_t)row * p.ldx + k);
    }
  };
  auto put_x = [&](const u32x4_t (&v)[XPT], int buf) {
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
      for (int j = 0; j < 2; ++j) {  // bytes 8 j .. 8 j + 7 of the piece: k0 + 16 q + 8 j, x piece ks * 8 + 2 q + j
        const X8 wf = kv8_to_x8<T>((u32x2_t){wr[ks][2 * j], wr[ks][2 * j + 1]});
        X8 gf;
        if constexpr (GLU) gf = kv8_to_x8<T>((u32x2_t){gr[ks][2 * j], gr[ks][2 * j + 1]});
#pragma unroll
        for (int mf = 0; mf < MF; ++mf) {
          const X8 xf = __builtin_bit_cast(X8, *(const u32x4_t*)(sx[buf] + (mf * 16 + c) * ROWB + (((ks * 8 + 2 * q + j) ^ c) * 16)));
          acc[mf] = DT<T>::mfma16(wf, xf, acc[mf]);
          if constexpr (GLU) accg[mf] = DT<T>::mfma16(gf, xf, accg[mf]);
        }
      }
    }
  };

  // A ring of D register sets.  Chunk ch lives in set ch % D: its x pieces and then its weight bytes are requested D - 1 chunks
  // ahead, into the set the chunk before the current one has just left.  One barrier per chunk: the x buffer written for chunk
  // ch was last read for chunk ch - 2, before the barrier of chunk ch - 1.
  u32x4_t wr[D][KS], gr[D][GLU ? KS : 1], xr[D][XPT];
#pragma unroll
  for (int j = 0; j < D - 1; ++j)
    if (j < nc) {
      load_x(xr[j], j);
      load_w(wr[j], gr[j], j);
    }
  for (int ch = 0; ch < nc; ch += D) {
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const int cur = ch + j;
      if (cur < nc) {  // (the same in every thread of the workgroup)
        put_x(xr[j], cur & 1);
        __syncthreads();
        if (cur + D - 1 < nc) {
          load_x(xr[(j + D - 1) % D], cur + D - 1);
          load_w(wr[(j + D - 1) % D], gr[(j + D - 1) % D], cur + D - 1);
        }
        compute(wr[j], gr[j], cur & 1);
      }
    }
  }

  if (!active) return;
  const int n = n0 + 4 * q;
  if (n >= p.N) return;
  skinny_write<T, MF, GLU, true>(skinny_finish_args(p), p.ws, p.nsplit, p.M, s, c, n, 0, p.M, acc, accg);
}

// One-time preparation of a weight: one wave per row.  a = max |w[n, :]| in fp32 (NaN elements ignored), scale[n] = a / 448
// (1.0 where a == 0), w8[n, k] = e4m3(clamp(float(w) * (1.0f / scale[n]), -448, 448)) rounded to nearest even, a NaN element
// sign | 0x7f: the formula and NaN rule of the fp8 KV-cache writes (kv8_quant16).
template <typename T>
__global__ __launch_bounds__(256) void weight_quant_w8_kernel(const T* w, int64_t ldw, uint8_t* w8, int64_t ldw8, float* scale,
                                                              int N, int K) {
  using X8 = typename DT<T>::x8;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= N) return;
  const T* src = w + (int64_t)row * ldw;
  float a = 0.f;
  for (int k = lane * 8; k < K; k += 512) {
    const X8 v = __builtin_bit_cast(X8, *(const u32x4_t*)(src + k));
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float f = __builtin_fabsf((float)v[i]);
      a = f > a ? f : a;  // (false for a NaN)
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const float o = __shfl_xor(a, d, 64);
    a = o > a ? o : a;
  }
  const float sc = a == 0.f ? 1.0f : a / 448.0f;
  const float inv = 1.0f / sc;
  if (lane == 0) scale[row] = sc;
  uint8_t* dst = w8 + (int64_t)row * ldw8;
  for (int k = lane * 16; k < K; k += 1024)
    *(u32x4_t*)(dst + k) = kv8_quant16<T>(*(const u32x4_t*)(src + k), *(const u32x4_t*)(src + k + 8), inv);
}

// ---- the quantiser's launch ----------------------------------------------------------------------------------------
extern "C" int mio_weight_quant_w8(const void* w, int64_t ldw, void* w8, int64_t ldw8, float* scale, int32_t N, int32_t K,
                                   int32_t dtype, void* stream) {
  const std::string who = "mio_weight_quant_w8";
  MIO_CHECK(N >= 0 && K >= 0, who + ": N, K must not be negative");
  MIO_CHECK(K % 16 == 0, who + ": K must be a multiple of 16");
  MIO_CHECK(dtype == MIO_BF16 || dtype == MIO_FP16, who + ": dtype must be bf16 or fp16");
  MIO_CHECK(ldw % 8 == 0 && ldw >= K, who + ": ldw must be a multiple of 8 elements and at least K");
  MIO_CHECK(ldw8 % 16 == 0 && ldw8 >= K, who + ": ldw8 must be a multiple of 16 bytes and at least K");
  if (N == 0) return 0;
  MIO_CHECK(w && w8 && scale, who + ": w, w8, scale must be non-null");
  MIO_CHECK(mio_aligned16(w) && mio_aligned16(w8) && (reinterpret_cast<uintptr_t>(scale) & 3) == 0,
            who + ": w and w8 must be 16-byte aligned, scale 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((N + 3) / 4));
  if (dtype == MIO_BF16)
    hipLaunchKernelGGL((weight_quant_w8_kernel<__bf16>), grid, dim3(256), 0, st, (const __bf16*)w, ldw, (uint8_t*)w8, ldw8, scale, N, K);
  else
    hipLaunchKernelGGL((weight_quant_w8_kernel<_Float16>), grid, dim3(256), 0, st, (const _Float16*)w, ldw, (uint8_t*)w8, ldw8, scale, N, K);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mio_fail(who + " launch: " + hipGetErrorString(e));
  return 0;
}

#define SKINNY_KERNELS(T, GLU)                                                                         \
  {{gemm_skinny_w8_kernel<T, 1, GLU>, gemm_skinny_w8_kernel<T, 2, GLU>, gemm_skinny_w8_kernel<T, 3, GLU>, \
    gemm_skinny_w8_kernel<T, 4, GLU>},                                                                 \
   gemm_skinny_reduce_kernel<T, GLU, true>}
static const SkinnyKernelTable KERNELS = {{SKINNY_KERNELS(__bf16, true), SKINNY_KERNELS(__bf16, false)},
                                          {SKINNY_KERNELS(_Float16, true), SKINNY_KERNELS(_Float16, false)}};
#undef SKINNY_KERNELS

// ---- the C ABI of the GEMM: argument marshalling over gemm_skinny_common.h's host side -----------------------------
extern "C" int mio_gemm_skinny_w8_splits(int64_t M, int32_t N, int32_t K, int32_t act) {
  return skinny_query_splits(FORM, "mio_gemm_skinny_w8_splits", M, N, K, act);
}

extern "C" size_t mio_gemm_skinny_w8_workspace_bytes(int64_t M, int32_t N, int32_t K, int32_t act) {
  return skinny_query_workspace_bytes(FORM, "mio_gemm_skinny_w8_workspace_bytes", M, N, K, act);
}

extern "C" int mio_gemm_skinny_w8_slice(int64_t M, int32_t N, int32_t K, int32_t act, int32_t slice, int32_t* k_begin,
                                        int32_t* k_end) {
  return skinny_query_slice(FORM, "mio_gemm_skinny_w8_slice", M, N, K, act, slice, k_begin, k_end);
}

extern "C" int mio_gemm_skinny_w8_chunk_k(int32_t act) { return skinny_query_chunk_k(FORM, "mio_gemm_skinny_w8_chunk_k", act); }

extern "C" int mio_gemm_skinny_w8_depth(int32_t act) { return skinny_query_depth(FORM, "mio_gemm_skinny_w8_depth", act); }

extern "C" int mio_gemm_skinny_w8_ok(int64_t M, int32_t N, int32_t K, int32_t act) {
  return skinny_query_ok(FORM, "mio_gemm_skinny_w8_ok", M, N, K, act);
}

extern "C" int mio_gemm_skinny_w8(const void* x, const void* w8, const float* w_scale, const void* bias, const void* w8_gate,
                                  const float* w_scale_gate, const void* bias_gate, const void* residual, void* y, void* workspace,
                                  int64_t M, int32_t N, int32_t K, int64_t ldx, int64_t ldw, int64_t ldy, int64_t ldr, int32_t act,
                                  int32_t dtype, void* stream) {
  return skinny_run(FORM, KERNELS, x, w8, w_scale, bias, w8_gate, w_scale_gate, bias_gate, residual, y, workspace, M, N, K, ldx, ldw,
                    ldy, ldr, act, dtype, stream);
}

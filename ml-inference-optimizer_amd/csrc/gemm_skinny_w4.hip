// Decode-step GEMM on MXFP4 weights (1 <= M <= 64): y[M,N] = act(x[M,K] deq(w4, w_scale)[N,K]^T + bias[n]) (+ residual), SwiGLU
// with a second weight and its own block scales; and the one-time quantiser that makes (w4, w_scale) from a 16-bit weight.  The
// C-ABI entry points mio_gemm_skinny_w4* and mio_weight_quant_mxfp4 (include/mio_hip.h).  This file is the kernel under the dense
// rows description, the quantiser and the entry points' argument marshalling: the K loop is gemm_skinny_w4_head.inc +
// gemm_skinny_w4_loop.inc, shared with the mixture-of-experts unit on MXFP4 expert weights (moe_w4.hip); the plan is
// gemm_skinny_plan.h under the form SKINNY_W4, and the launch's checks, the epilogue and the reduction are gemm_skinny_common.h's
// with SCALED = false, shared with gemm_skinny.hip and gemm_skinny_w8.hip.
//
// The storage form is OCP microscaling FP4: w4 holds e2m1 elements (sign, 2 exponent bits, 1 mantissa bit: +-{0, 0.5, 1, 1.5, 2,
// 3, 4, 6}), two per byte, element 2 i in the low nibble of byte i, row-major [N, K / 2]; w_scale holds one e8m0 byte per 32
// consecutive k, [N, K / 32], byte b meaning 2^(b - 127).  deq(w4, w_scale)[n, k] = e2m1(w4[n, k]) * 2^(w_scale[n, k / 32] - 127).
// Every such product with 2 <= b <= 252 is exact in bf16, so MXFP4 is a storage form of the weights here, not a compute precision:
// the conversion instruction widens two nibbles to bf16 with the scale applied, the arithmetic is the 16-bit MFMA with fp32
// accumulation, and nothing is left for the epilogue to scale.  bf16 only: in fp16 the product is exact only inside a narrow
// exponent range.
//
//   * 256 threads, 4 waves x 16 output columns; v_mfma_f32_16x16x32_bf16 with the widened weight fragment as the A operand.
//   * The k mapping, the scale traffic and the register ring: gemm_skinny_w4_loop.inc.
//   * accumulator, split-K in two launches, no atomics: as gemm_skinny_w8.hip states.
//
// What keeps every load in bounds (K % 32 == 0; ldw % 16 == 0 and ldw >= K / 2 bytes; lds % 4 == 0 and lds >= K / 32 bytes):
//   * a weight load is issued only for k < ke <= K, k a multiple of 32: its 16 bytes end at or before byte K / 2 of the row;
//   * a scale load is 2 bytes at byte k / 32 of the row, k < ke a multiple of 64: the byte behind it is below lds, a multiple of 4;
//   * the weight and scale row is min(n0 + c, N - 1): a lane past the last column computes a copy of the last row and stores nothing;
//   * x rows >= M and x pieces at k >= ke are zeros written to LDS, never read from memory.
#include "gemm_skinny_common.h"

constexpr SkinnyForm FORM = SKINNY_W4;  // this unit's weight form (gemm_skinny_plan.h)

// the launch's arguments: the shared ones (whose fp32 scale pointers stay null: nothing is left for the epilogue to scale), the
// weights' e8m0 block scales and their row stride in bytes
struct SkinnyW4Dev : SkinnyDev {
  const uint8_t* bscale;
  const uint8_t* bscale_g;  // SwiGLU: the gate weight's
  int64_t lds;
};

template <typename T, int MF, bool GLU>
__global__ __launch_bounds__(256) void gemm_skinny_w4_kernel(const SkinnyW4Dev p) {
  const auto wbase = [] { return (int64_t)0; };
  const auto wscale = [&] { return p.bscale; };
  const auto wscale_g = [&] { return p.bscale_g; };
#include "gemm_skinny_w4_head.inc"
  constexpr int nf = MF;
  constexpr bool all_live = true;
  const auto xhas = [&](int, int r) { return r < p.M; };
  const auto xrow = [](int, int r) { return r; };
#include "gemm_skinny_w4_loop.inc"

  if (!active) return;
  const int n = n0 + 4 * q;
  if (n >= p.N) return;
  skinny_write<T, MF, GLU, false>(skinny_finish_args(p), p.ws, p.nsplit, p.M, s, c, n, 0, p.M, acc, accg);
}

// One-time preparation of a weight by the OCP MX rule: one thread per block of 32.  a = max |v| in fp32 (NaN elements ignored),
// e = clamp(floor(log2 a) - 2, -127, 127), 0 where a == 0; the scale byte is e + 127; an element is v * 2^-e rounded to nearest
// even on the e2m1 grid, saturating at +-6 (floor: the block maximum may saturate); +-Inf gives +-6, NaN a signed zero.
__device__ __forceinline__ uint32_t mxfp4_code(float v, int e) {  // (the sign is v's own, a NaN's too)
  const float t = __builtin_ldexpf(v, -e);
  const float a = __builtin_fabsf(t);  // ties go to the even code: 0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4
  const uint32_t m = (a > 0.25f) + (a >= 0.75f) + (a > 1.25f) + (a >= 1.75f) + (a > 2.5f) + (a >= 3.5f) + (a > 5.0f);  // (0 for a NaN)
  return ((__float_as_uint(v) >> 28) & 8u) | m;
}

template <typename T>
__global__ __launch_bounds__(256) void weight_quant_mxfp4_kernel(const T* w, int64_t ldw, uint8_t* w4, int64_t ldw4, uint8_t* scale,
                                                                 int64_t lds, int N, int K) {
  using X8 = typename DT<T>::x8;
  const int nb = K >> 5;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)N * nb) return;
  const int row = (int)(idx / nb), b = (int)(idx % nb);
  const T* src = w + (int64_t)row * ldw + b * 32;
  X8 v[4];
  float a = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[i] = __builtin_bit_cast(X8, *(const u32x4_t*)(src + 8 * i));
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float f = __builtin_fabsf((float)v[i][j]);
      a = f > a ? f : a;  // (false for a NaN)
    }
  }
  int e = 0;
  if (a != 0.f) {
    const int field = (int)((__float_as_uint(a) >> 23) & 0xffu);  // floor(log2 a) + 127 of a normal; 0: below 2^-126; 255: Inf
    e = field == 255 ? 127 : max(field - 129, -127);
  }
  scale[(int64_t)row * lds + b] = (uint8_t)(e + 127);
  u32x4_t out;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    uint32_t d = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) d |= mxfp4_code((float)v[i][j], e) << (4 * j);
    out[i] = d;
  }
  *(u32x4_t*)(w4 + (int64_t)row * ldw4 + b * 16) = out;
}

// ---- the quantiser's launch ----------------------------------------------------------------------------------------
extern "C" int mio_weight_quant_mxfp4(const void* w, int64_t ldw, void* w4, int64_t ldw4, void* scale, int64_t lds, int32_t N,
                                      int32_t K, int32_t dtype, void* stream) {
  const std::string who = "mio_weight_quant_mxfp4";
  MIO_CHECK(N >= 0 && K >= 0, who + ": N, K must not be negative");
  MIO_CHECK(K % 32 == 0, who + ": K must be a multiple of 32 (whole MX blocks)");
  MIO_CHECK(dtype == MIO_BF16 || dtype == MIO_FP16, who + ": dtype must be bf16 or fp16");
  MIO_CHECK(ldw % 8 == 0 && ldw >= K, who + ": ldw must be a multiple of 8 elements and at least K");
  MIO_CHECK(ldw4 % 16 == 0 && ldw4 >= K / 2, who + ": ldw4 must be a multiple of 16 bytes and at least K / 2");
  MIO_CHECK(lds >= K / 32, who + ": lds must be at least K / 32 bytes");
  if (N == 0 || K == 0) return 0;
  MIO_CHECK(w && w4 && scale, who + ": w, w4, scale must be non-null");
  MIO_CHECK(mio_aligned16(w) && mio_aligned16(w4), who + ": w and w4 must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int64_t blocks = (int64_t)N * (K / 32);
  const dim3 grid((unsigned)((blocks + 255) / 256));
  if (dtype == MIO_BF16)
    hipLaunchKernelGGL((weight_quant_mxfp4_kernel<__bf16>), grid, dim3(256), 0, st, (const __bf16*)w, ldw, (uint8_t*)w4, ldw4,
                       (uint8_t*)scale, lds, N, K);
  else
    hipLaunchKernelGGL((weight_quant_mxfp4_kernel<_Float16>), grid, dim3(256), 0, st, (const _Float16*)w, ldw, (uint8_t*)w4, ldw4,
                       (uint8_t*)scale, lds, N, K);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mio_fail(who + " launch: " + hipGetErrorString(e));
  return 0;
}

// The second launch of a split call: gemm_skinny_reduce_kernel's body (gemm_skinny_common.h) at SCALED = false under a name of this
// unit's own, so that no kernel symbol is registered from two objects (the 16-bit unit carries that instantiation).
template <typename T, bool GLU>
__global__ __launch_bounds__(256) void gemm_skinny_w4_reduce_kernel(const SkinnyDev p) {
  const int ngrp = (p.N + 3) / 4;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)p.M * ngrp) return;
  const int m = (int)(idx / ngrp), n = (int)(idx % ngrp) * 4;
  float v[4], g[4];
  skinny_slice_sum<GLU>(p.ws, p.nsplit, (int64_t)p.M * p.N, p.N, m, n, v, g);
  skinny_finish<T, GLU, false>(skinny_finish_args(p), m, n, v, g);
}

// bf16 only: [SwiGLU / plain] K-loop kernels at 1 .. 4 row fragments, and the reduction
using SkinnyW4Kernel = void (*)(const SkinnyW4Dev);
#define SKINNY_KERNELS(GLU) \
  {gemm_skinny_w4_kernel<__bf16, 1, GLU>, gemm_skinny_w4_kernel<__bf16, 2, GLU>, gemm_skinny_w4_kernel<__bf16, 3, GLU>, \
   gemm_skinny_w4_kernel<__bf16, 4, GLU>}
static const SkinnyW4Kernel MAIN[2][4] = {SKINNY_KERNELS(true), SKINNY_KERNELS(false)};
#undef SKINNY_KERNELS
static const SkinnyKernel REDUCE[2] = {gemm_skinny_w4_reduce_kernel<__bf16, true>, gemm_skinny_w4_reduce_kernel<__bf16, false>};

// ---- the C ABI of the GEMM: argument marshalling over gemm_skinny_common.h's host side -----------------------------
extern "C" int mio_gemm_skinny_w4_splits(int64_t M, int32_t N, int32_t K, int32_t act) {
  return skinny_query_splits(FORM, "mio_gemm_skinny_w4_splits", M, N, K, act);
}

extern "C" size_t mio_gemm_skinny_w4_workspace_bytes(int64_t M, int32_t N, int32_t K, int32_t act) {
  return skinny_query_workspace_bytes(FORM, "mio_gemm_skinny_w4_workspace_bytes", M, N, K, act);
}

extern "C" int mio_gemm_skinny_w4_slice(int64_t M, int32_t N, int32_t K, int32_t act, int32_t slice, int32_t* k_begin,
                                        int32_t* k_end) {
  return skinny_query_slice(FORM, "mio_gemm_skinny_w4_slice", M, N, K, act, slice, k_begin, k_end);
}

extern "C" int mio_gemm_skinny_w4_chunk_k(int32_t act) { return skinny_query_chunk_k(FORM, "mio_gemm_skinny_w4_chunk_k", act); }

extern "C" int mio_gemm_skinny_w4_depth(int32_t act) { return skinny_query_depth(FORM, "mio_gemm_skinny_w4_depth", act); }

extern "C" int mio_gemm_skinny_w4_ok(int64_t M, int32_t N, int32_t K, int32_t act) {
  return skinny_query_ok(FORM, "mio_gemm_skinny_w4_ok", M, N, K, act);
}

extern "C" int mio_gemm_skinny_w4(const void* x, const void* w4, const void* w_scale, const void* bias, const void* w4_gate,
                                  const void* w_scale_gate, const void* bias_gate, const void* residual, void* y, void* workspace,
                                  int64_t M, int32_t N, int32_t K, int64_t ldx, int64_t ldw, int64_t lds, int64_t ldy, int64_t ldr,
                                  int32_t act, int32_t dtype, void* stream) {
  SkinnyW4Dev p;
  SkinnyPlan pl;
  bool launch;
  MIO_CHECK(K < 0 || K % 32 != 0 || skinny_lds_ok(lds, K), std::string(FORM.name) + ": lds must be a multiple of 4 bytes and at least K / 32");
  if (int rc = skinny_prepare(FORM, x, w4, w_scale, bias, w4_gate, w_scale_gate, bias_gate, residual, y, workspace, M, N, K, ldx, ldw,
                              ldy, ldr, act, dtype, p, pl, launch))
    return rc;
  if (!launch) return 0;
  p.bscale = (const uint8_t*)w_scale; p.bscale_g = (const uint8_t*)w_scale_gate; p.lds = lds;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(MAIN[pl.glu ? 0 : 1][pl.mf - 1], dim3((unsigned)pl.tiles_n, (unsigned)pl.nsplit), dim3(256), 0, st, p);
  if (pl.nsplit > 1) {
    const int64_t threads = (int64_t)p.M * ((p.N + 3) / 4);
    hipLaunchKernelGGL(REDUCE[pl.glu ? 0 : 1], dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, (const SkinnyDev&)p);
  }
  return skinny_launched(FORM);
}

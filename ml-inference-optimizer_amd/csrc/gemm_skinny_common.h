// What the two decode-step GEMM units share (gemm_skinny.hip: 16-bit weights; gemm_skinny_w8.hip: e4m3fn weights with one fp32
// scale per output column).  On the device: the launch's arguments, the one epilogue and the split-K reduction.  SCALED is the
// only difference between the units behind the accumulator: z = fma(acc, scale[n], bias[n]) in place of z = acc + bias[n].  With
// the flag off nothing of the scales is read and the arithmetic is that of the 16-bit kernel alone.  On the host (the end of
// this file): the launcher, the checks and argument fill of a launch and the host queries, each written once over the unit's
// SkinnyForm (gemm_skinny_plan.h) and its table of kernels.  A unit keeps its K loop and its extern "C" wrappers.
#pragma once
#include <string>

#include "gemm_kernel.h"
#include "gemm_skinny_plan.h"

struct SkinnyDev {
  const void* x;
  const void* w;
  const void* wg;
  const void* bias;
  const void* bias_g;
  const void* res;
  void* y;
  float* ws;  // [nsplit][M][N] fp32 (SwiGLU: then the gate half); nullptr with one slice
  int64_t ldx, ldw, ldy, ldr;
  int M, N, K, act, nsplit, steps;
  const float* scale;    // SCALED only: fp32 [N], the weight's per-column scale
  const float* scale_g;  // SCALED and SwiGLU only: the gate weight's
};

// What the epilogue reads, and nothing else: a launch's (skinny_finish_args) or, in moe.hip, one expert's.
struct SkinnyFinish {
  const void* bias;
  const void* bias_g;
  const void* res;
  void* y;
  int64_t ldy, ldr;
  int N, act;
  const float* scale;
  const float* scale_g;
};

__device__ __forceinline__ SkinnyFinish skinny_finish_args(const SkinnyDev& p) {
  return {p.bias, p.bias_g, p.res, p.y, p.ldy, p.ldr, p.N, p.act, p.scale, p.scale_g};
}

// The shape of the 16-bit K loop (gemm_skinny_w16_head.inc, gemm_skinny_w16_loop.inc) at MF row fragments, from the form's values
constexpr int SKINNY_KSTEP = SKINNY_W16.kstep;
static_assert(SKINNY_W16.sets(false) == 2 && SKINNY_W16.sets(true) == 2, "the 16-bit K loop is double-buffered");
template <int MF, bool GLU>
struct SkinnyW16Tile {
  static constexpr int SKC = SKINNY_W16.chunk(GLU);  // k per chunk
  static constexpr int KS = SKC / SKINNY_KSTEP, PCS = SKC / 8, ROWS = MF * 16, ROWB = SKC * 2;
  static constexpr int XPT = ROWS * PCS / 256;  // 16-byte pieces of the x chunk per thread
  static_assert(PCS >= 16 && ROWS * PCS % 256 == 0, "chunk shape");
};

__device__ __forceinline__ float skinny_act(int act, float v) {
  switch (act) {
    case MIO_ACT_GELU_TANH: return gemm_act<MIO_ACT_GELU_TANH>(v);
    case MIO_ACT_GELU_ERF: return gemm_act<MIO_ACT_GELU_ERF>(v);
    case MIO_ACT_RELU: return gemm_act<MIO_ACT_RELU>(v);
    case MIO_ACT_SILU: return gemm_act<MIO_ACT_SILU>(v);
    default: return v;
  }
}

// the pre-activation value of one column from its fp32 sum: the bias add, behind the column's scale where the weight has one
template <bool SCALED>
__device__ __forceinline__ float skinny_pre(float acc, const float* scale, float b, int nn) {
  if constexpr (SCALED) return __builtin_fmaf(acc, scale[nn], b);
  else return acc + b;
}

// The one epilogue, of both kernels: row m, columns n .. n + 3 (those below N), from the fp32 sums v (and g, the gate's).
template <typename T, bool GLU, bool SCALED = false>
__device__ __forceinline__ void skinny_finish(const SkinnyFinish& p, int m, int n, const float (&v)[4], const float (&g)[4]) {
  const T* bias = (const T*)p.bias;
  const T* bias_g = (const T*)p.bias_g;
  const T* rrow = p.res ? (const T*)p.res + (int64_t)m * p.ldr : nullptr;
  T* yrow = (T*)p.y + (int64_t)m * p.ldy;
  float o[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int nn = n + i < p.N ? n + i : p.N - 1;  // (clamped: computed, not stored)
    float z = skinny_pre<SCALED>(v[i], p.scale, bias ? (float)bias[nn] : 0.f, nn);
    if constexpr (GLU) z = gemm_act<MIO_ACT_SILU>(skinny_pre<SCALED>(g[i], p.scale_g, bias_g ? (float)bias_g[nn] : 0.f, nn)) * z;
    else z = skinny_act(p.act, z);
    if (rrow) z += (float)rrow[nn];
    o[i] = z;
  }
  if (n + 3 < p.N) {
    *(u32x2_t*)(yrow + n) = (u32x2_t){pack2<T>(o[0], o[1]), pack2<T>(o[2], o[3])};
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (n + i < p.N) yrow[n + i] = (T)o[i];
  }
}

// A lane's share of a workgroup's result, lane (c, q) of the wave at columns n0: of the cnt rows at r0 (the dense units: all M
// from 0; an expert: its sorted positions) rows r0 + 16 mf + c, columns n = n0 + 4 q .. + 3, through the epilogue (ws null: one
// slice) or into slice s of the fp32 partials ws [nsplit][rows][N] (SwiGLU: then the gate half).  The launch's values come by
// reference, so that they are read where they are used, as they were when every kernel read its own launch arguments here: by
// value the compiler orders the K-loop kernels' code differently.
template <typename T, int MF, bool GLU, bool SCALED>
__device__ __forceinline__ void skinny_write(const SkinnyFinish& f, float* const& ws, const int& nsplit, const int& rows, int s, int c,
                                             int n, const int& r0, const int& cnt, const f32x4_t (&acc)[MF],
                                             const f32x4_t (&accg)[GLU ? MF : 1]) {
#pragma unroll
  for (int mf = 0; mf < MF; ++mf) {
    const int m = mf * 16 + c;
    if (m >= cnt) continue;
    const int pos = r0 + m;
    if (ws == nullptr) {
      const float v[4] = {acc[mf][0], acc[mf][1], acc[mf][2], acc[mf][3]};
      float g[4] = {0.f, 0.f, 0.f, 0.f};
      if constexpr (GLU) {
#pragma unroll
        for (int i = 0; i < 4; ++i) g[i] = accg[mf][i];
      }
      skinny_finish<T, GLU, SCALED>(f, pos, n, v, g);
    } else {
      const int64_t plane = (int64_t)rows * f.N;
      float* dst = ws + (int64_t)s * plane + (int64_t)pos * f.N + n;
      if ((f.N & 3) == 0) {  // (n + 3 < N then, and the partial rows are 16-byte aligned)
        *(f32x4_t*)dst = acc[mf];
        if constexpr (GLU) *(f32x4_t*)(dst + (int64_t)nsplit * plane) = accg[mf];
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (n + i < f.N) {
            dst[i] = acc[mf][i];
            if constexpr (GLU) dst[(int64_t)nsplit * plane + i] = accg[mf][i];
          }
      }
    }
  }
}

// The slice sum: the partials ws [nsplit][rows][N] of row pos, columns n .. n + 3 (those below N), added in slice order
// starting from 0.f into v; GLU: and the gate half's, which follows the nsplit planes of rows * N, into g.
template <bool GLU>
__device__ __forceinline__ void skinny_slice_sum(const float* ws, int nsplit, int64_t plane, int N, int pos, int n, float (&v)[4],
                                                 float (&g)[4]) {
  const float* src = ws + (int64_t)pos * N + n;
  const float* srcg = src + (int64_t)nsplit * plane;
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = g[i] = 0.f;
  if ((N & 3) == 0) {
    for (int s = 0; s < nsplit; ++s) {
      const f32x4_t t = *(const f32x4_t*)(src + s * plane);
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] += t[i];
      if constexpr (GLU) {
        const f32x4_t u = *(const f32x4_t*)(srcg + s * plane);
#pragma unroll
        for (int i = 0; i < 4; ++i) g[i] += u[i];
      }
    }
  } else {
    for (int s = 0; s < nsplit; ++s)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (n + i < N) {
          v[i] += src[s * plane + i];
          if constexpr (GLU) g[i] += srcg[s * plane + i];
        }
  }
}

// The second launch: one thread per (row, 4 columns) sums the slices' partials in index order and runs the epilogue.
template <typename T, bool GLU, bool SCALED = false>
__global__ __launch_bounds__(256) void gemm_skinny_reduce_kernel(const SkinnyDev p) {
  const int ngrp = (p.N + 3) / 4;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)p.M * ngrp) return;
  const int m = (int)(idx / ngrp), n = (int)(idx % ngrp) * 4;
  float v[4], g[4];
  skinny_slice_sum<GLU>(p.ws, p.nsplit, (int64_t)p.M * p.N, p.N, m, n, v, g);
  skinny_finish<T, GLU, SCALED>(skinny_finish_args(p), m, n, v, g);
}

// ---- host side -----------------------------------------------------------------------------------------------------------
// The kernels of one (dtype, SwiGLU or not) pair of a unit: its K-loop kernel at 1 .. 4 row fragments and the reduction.
using SkinnyKernel = void (*)(const SkinnyDev);
struct SkinnyKernels {
  SkinnyKernel main[4], reduce;
};
// a unit's table: [MIO_BF16 / MIO_FP16][SwiGLU / plain]
using SkinnyKernelTable = SkinnyKernels[2][2];

static inline void skinny_launch(const SkinnyKernels& k, const SkinnyDev& p, const SkinnyPlan& pl, hipStream_t st) {
  hipLaunchKernelGGL(k.main[pl.mf - 1], dim3((unsigned)pl.tiles_n, (unsigned)pl.nsplit), dim3(256), 0, st, p);
  if (pl.nsplit > 1) {
    const int64_t threads = (int64_t)p.M * ((p.N + 3) / 4);
    hipLaunchKernelGGL(k.reduce, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, p);
  }
}

// A launch of either unit: every check, the plan, the empty call, the device arguments and the launches.  scale / scale_g are
// the weights' per-column scales (null for a form without them); ldw counts in the unit the form's ldw_multiple does.
static inline int skinny_run(const SkinnyForm& f, const SkinnyKernelTable& kernels, const void* x, const void* w, const float* scale,
                             const void* bias, const void* w_gate, const float* scale_g, const void* bias_gate, const void* residual,
                             void* y, void* workspace, int64_t M, int32_t N, int32_t K, int64_t ldx, int64_t ldw, int64_t ldy,
                             int64_t ldr, int32_t act, int32_t dtype, void* stream) {
#define SKINNY_CHECK(cond, text) MIO_CHECK(cond, std::string(f.name) + (text))
  std::string err;
  if (!skinny_shape_ok(f, f.name, M, N, K, act, err)) return mio_fail(err);
  SKINNY_CHECK(dtype == MIO_BF16 || dtype == MIO_FP16, f.dtype_text);
  const bool glu = act == MIO_ACT_SWIGLU;
  SKINNY_CHECK(glu == (w_gate != nullptr) && (!f.scaled || glu == (scale_g != nullptr)), f.gate_text);
  SKINNY_CHECK(glu || bias_gate == nullptr, ": bias_gate belongs to act == SWIGLU");
  SKINNY_CHECK(ldw % f.ldw_multiple == 0, f.ldw_multiple_text);
  SKINNY_CHECK(ldw >= K, f.ldw_short_text);
  SKINNY_CHECK(ldx % 8 == 0 && ldy % 8 == 0 && (!residual || ldr % 8 == 0), f.ld_multiple_text);
  SKINNY_CHECK(ldx >= K && ldy >= N && (!residual || ldr >= N), ": row stride smaller than row length");
  SKINNY_CHECK(w && (!f.scaled || scale) && (M == 0 || (x && y)), f.null_text);
  SKINNY_CHECK(mio_aligned16(x) && mio_aligned16(w) && mio_aligned16(y) && mio_aligned16(w_gate) && mio_aligned16(residual) &&
                   mio_aligned16(bias) && mio_aligned16(bias_gate) && mio_aligned16(workspace) && mio_aligned16(scale) &&
                   mio_aligned16(scale_g),
               ": pointers must be 16-byte aligned");
  const SkinnyPlan pl = skinny_plan(f, M, N, K, act);
  if (M == 0 || N == 0) return 0;
  SKINNY_CHECK(pl.nsplit == 1 || workspace != nullptr, std::string(": workspace required (") + f.name + "_workspace_bytes) when the plan splits K");
#undef SKINNY_CHECK
  SkinnyDev p;
  p.x = x; p.w = w; p.wg = w_gate; p.bias = bias; p.bias_g = bias_gate; p.res = residual; p.y = y;
  p.ws = pl.nsplit > 1 ? (float*)workspace : nullptr;
  p.scale = scale; p.scale_g = scale_g;
  p.ldx = ldx; p.ldw = ldw; p.ldy = ldy; p.ldr = ldr;
  p.M = (int)M; p.N = N; p.K = K; p.act = act; p.nsplit = pl.nsplit; p.steps = pl.steps;
  skinny_launch(kernels[dtype == MIO_BF16 ? 0 : 1][glu ? 0 : 1], p, pl, (hipStream_t)stream);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mio_fail(std::string(f.name) + " launch: " + hipGetErrorString(e));
  return 0;
}

// The host queries; who is the extern "C" entry point that asks.
static inline int skinny_query_splits(const SkinnyForm& f, const char* who, int64_t M, int32_t N, int32_t K, int32_t act) {
  std::string err;
  if (!skinny_shape_ok(f, who, M, N, K, act, err)) return mio_fail(err);
  return skinny_plan(f, M, N, K, act).nsplit;
}

static inline size_t skinny_query_workspace_bytes(const SkinnyForm& f, const char* who, int64_t M, int32_t N, int32_t K, int32_t act) {
  std::string err;
  if (!skinny_shape_ok(f, who, M, N, K, act, err)) {
    mio_set_error(err);
    return 0;
  }
  return skinny_workspace_bytes(skinny_plan(f, M, N, K, act), M, N);
}

static inline int skinny_query_slice(const SkinnyForm& f, const char* who, int64_t M, int32_t N, int32_t K, int32_t act, int32_t slice,
                                     int32_t* k_begin, int32_t* k_end) {
  std::string err;
  if (!skinny_shape_ok(f, who, M, N, K, act, err)) return mio_fail(err);
  const SkinnyPlan pl = skinny_plan(f, M, N, K, act);
  MIO_CHECK(k_begin && k_end && slice >= 0 && slice < pl.nsplit, std::string(who) + ": slice must be in [0, " + f.name + "_splits)");
  skinny_slice(f, pl, K, slice, *k_begin, *k_end);
  return 0;
}

static inline int skinny_query_chunk_k(const SkinnyForm& f, const char* who, int32_t act) {
  std::string err;
  if (!skinny_shape_ok(f, who, 0, 0, 0, act, err)) return mio_fail(err);
  return f.chunk(act == MIO_ACT_SWIGLU);
}

static inline int skinny_query_depth(const SkinnyForm& f, const char* who, int32_t act) {
  std::string err;
  if (!skinny_shape_ok(f, who, 0, 0, 0, act, err)) return mio_fail(err);
  return f.sets(act == MIO_ACT_SWIGLU);
}

static inline int skinny_query_ok(const SkinnyForm& f, const char* who, int64_t M, int32_t N, int32_t K, int32_t act) {
  std::string err;
  return (skinny_shape_ok(f, who, M, N, K, act, err) && f.advised(M, N, K, act)) ? 1 : 0;
}

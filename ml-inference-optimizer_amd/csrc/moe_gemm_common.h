// What the mixture-of-experts decode units share (moe.hip: 16-bit expert weights; moe_w8.hip: e4m3fn expert weights with one
// fp32 scale per expert and output channel; moe_w4.hip: MXFP4 expert weights with e8m0 block scales), in the manner of gemm_skinny_common.h.  On the device: the launch's arguments, an
// expert's epilogue arguments and up's reduction; an expert's rows description is moe_rows_head.inc + moe_rows_gather.inc, down's
// finishing launch moe_common.h's.  SCALED is the only difference between the units behind the accumulator, as in the decode-step
// GEMM.  On the host (the end of this file): the operand checks, the host queries and the two launches, each written once over
// the unit's SkinnyForm (gemm_skinny_plan.h) and its table of kernels.  A unit keeps its K-loop kernel and its extern "C" wrappers.
#pragma once
#include <string>

#include "moe_common.h"
#include "moe_plan.h"

// The launch's arguments, one statement for both forms.  The scales are a base that is empty for a form without them, and they
// sit behind the weights: each unit's K-loop kernels then read their arguments at the offsets they always had, which is what
// keeps their instructions what they were (with two scale pointers at the end of one plain struct the FP8 kernels compile to
// another order, with them here in one plain struct two of the 16-bit kernels do).
struct MoeDevWeights {
  const void* x;   // up: the tokens [T, ldx]; down: h by sorted position [T k, ldx]
  const void* w;   // [E][N, ldw], experts expert_stride apart (strides in the unit the form's ldw_multiple counts in)
  const void* wg;  // SwiGLU: the gate weight, same strides
};
// what scales a unit's weights carry: none, fp32 per expert and output channel (applied in the epilogues: SCALED there), or e8m0
// block bytes per expert, output channel and 32 k (applied inside the K loop: they travel to the kernel and to nothing behind it)
constexpr int MOE_SCALES_NONE = 0, MOE_SCALES_CHANNEL = 1, MOE_SCALES_BLOCK = 2;
template <int SCALES>
struct MoeDevScales {};
template <>
struct MoeDevScales<MOE_SCALES_CHANNEL> {
  const float* scale;    // fp32 [E, N]
  const float* scale_g;  // SwiGLU: the gate weight's
};
template <>
struct MoeDevScales<MOE_SCALES_BLOCK> {
  const uint8_t* scale;    // e8m0 [E][N, lds], experts sstride apart (bytes)
  const uint8_t* scale_g;  // SwiGLU: the gate weight's, same strides
  int64_t lds, sstride;
};
template <int SCALES>
struct MoeDev : MoeDevWeights, MoeDevScales<SCALES> {
  const void* bias;  // [E, N] or null
  const void* bias_g;
  void* y;           // up with one slice: h [T k, ldy]
  float* ws;         // fp32 partials [nsplit][T k][N] by sorted position (SwiGLU: then the gate half); null: finish in the kernel
  const int32_t* offsets;
  const int32_t* sorted_rows;  // up: routed row of a sorted position; null (down): x rows ARE sorted positions
  int64_t ldx, ldw, estride, ldy;
  int T, topk, E, rows, N, K, act, nsplit, steps;
};

// the epilogue's arguments for expert e: its biases (SCALED: and its scales), no residual
template <int SCALES>
__device__ __forceinline__ SkinnyFinish moe_finish_args(const MoeDev<SCALES>& p, int e) {
  SkinnyFinish f = {};
  f.bias = p.bias ? (const char*)p.bias + (int64_t)e * p.N * 2 : nullptr;
  f.bias_g = p.bias_g ? (const char*)p.bias_g + (int64_t)e * p.N * 2 : nullptr;
  f.y = p.y;
  f.ldy = p.ldy;
  f.N = p.N;
  f.act = p.act;
  if constexpr (SCALES == MOE_SCALES_CHANNEL) {
    f.scale = p.scale + (int64_t)e * p.N;
    f.scale_g = p.scale_g ? p.scale_g + (int64_t)e * p.N : nullptr;
  }
  return f;
}

// Up's second launch: one thread per (sorted position, 4 columns) sums the slices' partials in index order and runs the epilogue
// with the biases (and scales) of the position's expert: the e with offsets[e] <= pos < offsets[e + 1].
template <typename T, bool GLU, int SCALES>
__global__ __launch_bounds__(256) void moe_up_reduce_kernel(const MoeDev<SCALES> p) {
  const int ngrp = (p.N + 3) / 4;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)p.rows * ngrp) return;
  const int pos = (int)(idx / ngrp), n = (int)(idx % ngrp) * 4;
  int lo = 0, hi = p.E - 1;
  while (lo < hi) {  // the largest e with offsets[e] <= pos (offsets[0] = 0; empty experts repeat an offset)
    const int mid = (lo + hi + 1) >> 1;
    if (p.offsets[mid] <= pos) lo = mid;
    else hi = mid - 1;
  }
  float v[4], g[4];
  skinny_slice_sum<GLU>(p.ws, p.nsplit, (int64_t)p.rows * p.N, p.N, pos, n, v, g);
  skinny_finish<T, GLU, SCALES == MOE_SCALES_CHANNEL>(moe_finish_args<SCALES>(p, lo), pos, n, v, g);
}

// ---- host side -----------------------------------------------------------------------------------------------------------
// A unit's kernels: per (dtype, SwiGLU or not) its K-loop kernel at 1 .. 4 row fragments and up's reduction, and per dtype down's
// finishing launch.
template <int SCALES>
struct MoeKernels {
  void (*main[4])(const MoeDev<SCALES>);
  void (*reduce)(const MoeDev<SCALES>);
};
template <int SCALES>
struct MoeKernelTable {
  MoeKernels<SCALES> gemm[2][2];             // [MIO_BF16 / MIO_FP16][SwiGLU / plain]
  void (*down_finish[2])(const MoeDownDev);  // [MIO_BF16 / MIO_FP16]
};
#define MOE_KERNELS(KERNEL, T, GLU, SCALED) \
  {{KERNEL<T, 1, GLU>, KERNEL<T, 2, GLU>, KERNEL<T, 3, GLU>, KERNEL<T, 4, GLU>}, moe_up_reduce_kernel<T, GLU, SCALED>}
#define MOE_KERNEL_TABLE(KERNEL, UNIT, SCALED)                                                                  \
  {{{MOE_KERNELS(KERNEL, __bf16, true, SCALED), MOE_KERNELS(KERNEL, __bf16, false, SCALED)},                    \
    {MOE_KERNELS(KERNEL, _Float16, true, SCALED), MOE_KERNELS(KERNEL, _Float16, false, SCALED)}},               \
   {moe_down_finish_kernel<__bf16, UNIT, (SCALED) == MOE_SCALES_CHANNEL>, moe_down_finish_kernel<_Float16, UNIT, (SCALED) == MOE_SCALES_CHANNEL>}}

static inline bool moe_aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

// what up and down check alike: the grouped GEMM's operands (x rows of K 16-bit elements, weights [E][N, ldw], outputs of N)
static inline int moe_gemm_checks(const SkinnyForm& f, const std::string& fn, int64_t T, int32_t k, int32_t E, int32_t N, int32_t K,
                                  int32_t act, int32_t dtype, int64_t ldx, int64_t ldw, int64_t estride, int64_t ldy) {
  std::string err;
  if (!moe_shape_ok(f, fn.c_str(), T, k, E, N, K, act, err)) return mio_fail(err);
  MIO_CHECK(dtype == MIO_BF16 || (dtype == MIO_FP16 && !f.block_scaled), fn + f.dtype_text);
  MIO_CHECK(ldw % f.ldw_multiple == 0 && estride % f.ldw_multiple == 0, fn + f.moe.ldw_multiple);
  MIO_CHECK(ldx % 8 == 0 && ldy % 8 == 0, fn + f.moe.ld_multiple);
  MIO_CHECK(ldx >= K && ldw >= skinny_row_units(f, K) && ldy >= N, fn + ": row stride smaller than row length");
  MIO_CHECK(N == 0 || estride >= (int64_t)(N - 1) * ldw + skinny_row_units(f, K), fn + ": expert_stride smaller than one expert's weight");
  return 0;
}

// the block-scale operands of a block-scaled form: [E][N, lds] bytes, experts sstride apart
static inline int moe_block_scale_checks(const std::string& fn, int32_t N, int32_t K, int64_t lds, int64_t sstride) {
  MIO_CHECK(skinny_lds_ok(lds, K) && sstride % 4 == 0, fn + ": lds and scale_expert_stride must be multiples of 4 bytes, lds at least K / 32");
  MIO_CHECK(N == 0 || sstride >= (int64_t)(N - 1) * lds + K / 32, fn + ": scale_expert_stride smaller than one expert's scales");
  return 0;
}

// The host queries of up and down (down: act = MIO_ACT_NONE); who is the extern "C" entry point that asks.
static inline int moe_query_splits(const SkinnyForm& f, const char* who, int32_t T, int32_t k, int32_t E, int32_t N, int32_t K,
                                   int32_t act) {
  std::string err;
  if (!moe_shape_ok(f, who, T, k, E, N, K, act, err)) return mio_fail(err);
  return moe_plan(f, T, k, E, N, K, act).nsplit;
}

static inline size_t moe_query_workspace_bytes(const SkinnyForm& f, const char* who, bool down, int32_t T, int32_t k, int32_t E,
                                               int32_t N, int32_t K, int32_t act) {
  std::string err;
  if (!moe_shape_ok(f, who, T, k, E, N, K, act, err)) {
    mio_set_error(err);
    return 0;
  }
  const MoePlan pl = moe_plan(f, T, k, E, N, K, act);
  return down ? moe_down_workspace_bytes(pl, N) : moe_up_workspace_bytes(pl, N);
}

// the grouped GEMM's launch arguments, what up and down fill alike
template <int SCALES>
static inline MoeDev<SCALES> moe_dev(const MoePlan& pl, const void* x, const void* w, const void* w_gate, const void* scale,
                                     const void* scale_g, int64_t lds, int64_t sstride, const int32_t* offsets, int32_t T, int32_t k, int32_t E, int32_t N,
                                     int32_t K, int64_t ldx, int64_t ldw, int64_t estride, int32_t act) {
  MoeDev<SCALES> p = {};
  p.x = x; p.w = w; p.wg = w_gate; p.offsets = offsets;
  if constexpr (SCALES == MOE_SCALES_CHANNEL) {
    p.scale = (const float*)scale; p.scale_g = (const float*)scale_g;
  } else if constexpr (SCALES == MOE_SCALES_BLOCK) {
    p.scale = (const uint8_t*)scale; p.scale_g = (const uint8_t*)scale_g;
    p.lds = lds; p.sstride = sstride;
  }
  p.ldx = ldx; p.ldw = ldw; p.estride = estride;
  p.T = T; p.topk = k; p.E = E; p.rows = pl.rows; p.N = N; p.K = K; p.act = act; p.nsplit = pl.nsplit; p.steps = pl.steps;
  return p;
}

static inline int moe_launched(const std::string& fn) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mio_fail(fn + " launch: " + hipGetErrorString(e));
  return 0;
}

// The up launch of either unit, entry point fn: every check, the plan, the empty call, the device arguments and the launches.
// scale / scale_g are the weights' scales (fp32 [E, I], or e8m0 bytes [E][I, lds] sstride apart; null for a form without them).
template <int SCALES>
static inline int moe_run_up(const SkinnyForm& f, const MoeKernelTable<SCALES>& kernels, const std::string& fn, const void* x, const void* w_up,
                             const void* scale, const void* b_up, const void* w_gate, const void* scale_g, const void* b_gate,
                             const int32_t* expert_offsets, const int32_t* sorted_rows, void* h, void* workspace, int32_t T,
                             int32_t top_k, int32_t E, int32_t I, int32_t d, int64_t ldx, int64_t ldw, int64_t expert_stride,
                             int64_t ldh, int32_t act, int32_t dtype, void* stream, int64_t lds = 0, int64_t sstride = 0) {
  if (int rc = moe_gemm_checks(f, fn, T, top_k, E, I, d, act, dtype, ldx, ldw, expert_stride, ldh)) return rc;
  if constexpr (SCALES == MOE_SCALES_BLOCK)
    if (int rc = moe_block_scale_checks(fn, I, d, lds, sstride)) return rc;
  const bool glu = act == MIO_ACT_SWIGLU, has_scales = SCALES != MOE_SCALES_NONE;
  MIO_CHECK(glu == (w_gate != nullptr) && (!has_scales || glu == (scale_g != nullptr)), fn + f.moe.gate);
  MIO_CHECK(glu || b_gate == nullptr, fn + ": b_gate belongs to act == SWIGLU");
  MIO_CHECK(!has_scales || scale != nullptr, fn + f.moe.up_scale);
  MIO_CHECK(w_up && (T == 0 || (x && h && expert_offsets && sorted_rows)), fn + f.moe.up_null);
  MIO_CHECK(mio_aligned16(x) && mio_aligned16(w_up) && mio_aligned16(w_gate) && mio_aligned16(b_up) && mio_aligned16(b_gate) &&
                mio_aligned16(h) && mio_aligned16(workspace) && moe_aligned4(scale) && moe_aligned4(scale_g) &&
                moe_aligned4(expert_offsets) && moe_aligned4(sorted_rows),
            fn + f.moe.aligned);
  const MoePlan pl = moe_plan(f, T, top_k, E, I, d, act);
  if (T == 0 || I == 0) return 0;
  MIO_CHECK(pl.nsplit == 1 || workspace != nullptr, fn + ": workspace required (" + fn + "_workspace_bytes) when the plan splits K");
  MoeDev<SCALES> p = moe_dev<SCALES>(pl, x, w_up, w_gate, scale, scale_g, lds, sstride, expert_offsets, T, top_k, E, I, d, ldx, ldw, expert_stride, act);
  p.bias = b_up; p.bias_g = b_gate; p.y = h; p.ldy = ldh;
  p.ws = pl.nsplit > 1 ? (float*)workspace : nullptr;
  p.sorted_rows = sorted_rows;
  const MoeKernels<SCALES>& kn = kernels.gemm[dtype == MIO_BF16 ? 0 : 1][glu ? 0 : 1];
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(kn.main[pl.mf - 1], dim3((unsigned)pl.tiles_n, (unsigned)pl.nsplit, (unsigned)E), dim3(256), 0, st, p);
  if (pl.nsplit > 1) {
    const int64_t threads = (int64_t)pl.rows * ((I + 3) / 4);
    hipLaunchKernelGGL(kn.reduce, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, p);
  }
  return moe_launched(fn);
}

// The down launch of either unit: the grouped GEMM into the partials, always, and the finishing launch where a token's slots meet.
template <int SCALES>
static inline int moe_run_down(const SkinnyForm& f, const MoeKernelTable<SCALES>& kernels, const std::string& fn, const void* h,
                               const void* w_down, const void* scale, const void* b_down, const int32_t* ids, const float* weights,
                               const int32_t* expert_offsets, const int32_t* row_pos, const void* residual, void* y, void* workspace,
                               int32_t T, int32_t top_k, int32_t E, int32_t d, int32_t I, int64_t ldh, int64_t ldw,
                               int64_t expert_stride, int64_t ldy, int64_t ldr, int32_t dtype, void* stream, int64_t lds = 0,
                               int64_t sstride = 0) {
  if (int rc = moe_gemm_checks(f, fn, T, top_k, E, d, I, MIO_ACT_NONE, dtype, ldh, ldw, expert_stride, ldy)) return rc;
  if constexpr (SCALES == MOE_SCALES_BLOCK)
    if (int rc = moe_block_scale_checks(fn, d, I, lds, sstride)) return rc;
  MIO_CHECK(!residual || (ldr % 8 == 0 && ldr >= d), fn + ": ldr must be a multiple of 8 elements and at least d");
  MIO_CHECK(SCALES == MOE_SCALES_NONE || scale != nullptr, fn + f.moe.down_scale);
  MIO_CHECK(w_down && (T == 0 || (h && y && ids && weights && expert_offsets && row_pos)), fn + f.moe.down_null);
  MIO_CHECK(mio_aligned16(h) && mio_aligned16(w_down) && mio_aligned16(b_down) && mio_aligned16(residual) && mio_aligned16(y) &&
                mio_aligned16(workspace) && moe_aligned4(scale) && moe_aligned4(ids) && moe_aligned4(weights) &&
                moe_aligned4(expert_offsets) && moe_aligned4(row_pos),
            fn + f.moe.aligned);
  const MoePlan pl = moe_plan(f, T, top_k, E, d, I, MIO_ACT_NONE);
  if (T == 0 || d == 0) return 0;
  MIO_CHECK(workspace != nullptr, fn + ": workspace required (" + fn + "_workspace_bytes)");
  MoeDev<SCALES> p = moe_dev<SCALES>(pl, h, w_down, nullptr, scale, nullptr, lds, sstride, expert_offsets, T, top_k, E, d, I, ldh, ldw, expert_stride, MIO_ACT_NONE);
  p.ws = (float*)workspace;
  // (the finishing launch applies per-channel scales only: block scales went in inside the K loop)
  const MoeDownDev fin = {(const float*)workspace, SCALES == MOE_SCALES_CHANNEL ? (const float*)scale : nullptr, b_down, residual, y, ids, weights, row_pos, ldy, ldr, T, top_k, E, pl.rows,
                          d, pl.nsplit};
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(kernels.gemm[dtype == MIO_BF16 ? 0 : 1][1].main[pl.mf - 1],
                     dim3((unsigned)pl.tiles_n, (unsigned)pl.nsplit, (unsigned)E), dim3(256), 0, st, p);
  const int64_t threads = (int64_t)T * ((d + 3) / 4);
  hipLaunchKernelGGL(kernels.down_finish[dtype == MIO_BF16 ? 0 : 1], dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, fin);
  return moe_launched(fn);
}

// Mixture-of-experts MLP for decode steps (T <= 64 tokens, E <= 256 experts, top_k <= 8): the router and the two grouped GEMMs;
// the C-ABI entry points mio_moe_route, mio_moe_up, mio_moe_down and their host queries (semantics: include/mio_hip.h, DESIGN
// 4.2d).  The plan (shape checks, split of K, workspaces) is moe_plan.h.  The grouped GEMM's K loop is the decode-step GEMM's,
// the same text (gemm_skinny_w16_head.inc, gemm_skinny_w16_loop.inc) under an expert's rows description; the slice range, the
// slice sum and the epilogue arithmetic are gemm_skinny_plan.h's skinny_slice_range and gemm_skinny_common.h's skinny_slice_sum
// and skinny_finish, the ones the decode-step GEMM runs.
//
// Router: ONE workgroup of 16 waves, a wave per token (tokens wave, wave + 16, ...).  A lane holds the logits of experts lane,
// lane + 64, lane + 128, lane + 192 as fp32 (exact for bf16 / fp16) and their order-preserving keys; top_k rounds of a wave max
// over (key, ~index) pick the experts in the stated order, and the softmax sums run in a fixed shape (a lane's four in index
// order, then the xor butterfly), so reruns give the same bits.  Then a counting sort in LDS with integers only: thread e walks
// the <= 512 chosen ids in routed-row order, which yields its count, and -- behind a prefix over the counts -- its rows in
// ascending order by construction.  No atomic of any kind.
//
// Grouped GEMM: the decode-step GEMM's K loop (gemm_skinny_w16_loop.inc: a 16 x 32 weight fragment as the MFMA A operand straight from
// the row-major weight into VGPRs, x rows staged through LDS with the p ^ (r & 15) swizzle, two register sets, one barrier per
// chunk, v_mfma_f32_16x16x32) with the expert as the grid's third dimension.  A workgroup reads offsets[e], offsets[e + 1] and
// returns at once when its expert has no rows: before any weight load and before any barrier, and the same for all its threads.
// The x stage gathers rows through sorted_rows (up: routed row / top_k is the token) or by sorted position (down: h is stored
// that way); rows past the expert's count are zeros that are never read from memory.  The kernel is instantiated for the host's
// bound on an expert's rows, ceil(T / 16) fragments, and a workgroup stages and multiplies only the fragments its expert's
// count reaches.  Split-K as in the decode-step GEMM: fp32 partials by sorted position, a second launch that sums them in slice
// order.  Up finishes in the first kernel when there is one slice; down always goes through the partials, because its second
// launch is where the top_k slots of a token meet: slice sum, bias, routing weight, slot sum in slot order, residual, one
// rounding.  No atomics, counters or barriers between workgroups.
#include <cfloat>

#include "gemm_skinny_common.h"
#include "moe_plan.h"

typedef unsigned long long moe_u64;

// ---- router ------------------------------------------------------------------------------------------------------------------
struct MoeRouteDev {
  const void* logits;
  int64_t ld;
  int32_t* ids;
  float* weights;
  int32_t* offsets;
  int32_t* sorted_rows;
  int32_t* row_pos;
  int T, E, topk, renorm;
};

constexpr int MOE_RT_NT = 1024, MOE_RT_NW = MOE_RT_NT / 64;
static_assert(MOE_E_MAX <= 4 * 64 && MOE_E_MAX <= MOE_RT_NT, "four logits per lane; one sorting thread per expert");

// the order-preserving key of a canonical fp32 (no NaN, no -0) and its inverse
__device__ __forceinline__ uint32_t moe_key(float x) {
  const uint32_t h = __float_as_uint(x);
  return (h & 0x80000000u) ? ~h : (h | 0x80000000u);
}
__device__ __forceinline__ float moe_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

// exp(x - m) for x <= m, m finite: 1 at the maximum, 0 for -inf
__device__ __forceinline__ float moe_w(float x, float m) {
  const float d = x - m;
  const float t = d * 1.4426950408889634f;
  const float w = (t == t) ? fast_exp2(t) : 0.f;
  return d == 0.f ? 1.f : fminf(w, 1.f);
}

template <typename L>
__global__ __launch_bounds__(MOE_RT_NT) void moe_route_kernel(const MoeRouteDev a) {
  __shared__ int32_t s_ids[MOE_T_MAX * MOE_TOPK_MAX];
  __shared__ int32_t s_cnt[MOE_E_MAX];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t key_ninf = moe_key(-INFINITY);

  for (int t = wave; t < a.T; t += MOE_RT_NW) {  // (wave-uniform)
    const L* row = (const L*)a.logits + (int64_t)t * a.ld;
    float x[4];
    moe_u64 cand[4];
    moe_u64 best = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = lane + 64 * i;
      x[i] = -INFINITY;
      cand[i] = 0;  // (below every expert's: the smallest key, -inf's, is not 0)
      if (e < a.E) {
        float v = (float)row[e];
        if (v != v) v = -INFINITY;
        if (v == 0.f) v = 0.f;  // -0 -> +0
        x[i] = fminf(v, FLT_MAX);
        cand[i] = ((moe_u64)moe_key(v) << 32) | (uint32_t)~(uint32_t)e;
      }
      best = cand[i] > best ? cand[i] : best;
    }
    for (int o = 32; o >= 1; o >>= 1) {
      const moe_u64 u = __shfl_xor(best, o, 64);
      best = u > best ? u : best;
    }
    const uint32_t kmax = (uint32_t)(best >> 32);
    int my_id = lane;  // lane j < top_k ends up with slot j
    float my_w = 0.f;
    if (kmax != key_ninf) {  // (else no finite logit: ids 0 .. top_k - 1, weights 0)
      const float m = fminf(moe_unkey(kmax), FLT_MAX);
      float z = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) z += (lane + 64 * i < a.E) ? moe_w(x[i], m) : 0.f;
      for (int o = 32; o >= 1; o >>= 1) z += __shfl_xor(z, o, 64);
      for (int j = 0; j < a.topk; ++j) {
        moe_u64 b = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) b = cand[i] > b ? cand[i] : b;
        for (int o = 32; o >= 1; o >>= 1) {
          const moe_u64 u = __shfl_xor(b, o, 64);
          b = u > b ? u : b;
        }
        const int idx = (int)~(uint32_t)b;
        const float pj = moe_w(fminf(moe_unkey((uint32_t)(b >> 32)), FLT_MAX), m) / z;
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (lane + 64 * i == idx) cand[i] = 0;
        if (lane == j) my_id = idx, my_w = pj;
      }
      if (a.renorm) {
        float s = 0.f;
        for (int j = 0; j < a.topk; ++j) s += __shfl(my_w, j, 64);  // slot order
        my_w = my_w / s;  // (s > 0: slot 0 is the maximum, whose weight is 1 / z)
      }
    }
    if (lane < a.topk) {
      const int r = t * a.topk + lane;
      a.ids[r] = my_id;
      a.weights[r] = my_w;
      s_ids[r] = my_id;
    }
  }
  __syncthreads();

  // counting sort: thread e owns expert e
  const int rows = a.T * a.topk;
  int cnt = 0;
  if (tid < a.E)
    for (int r = 0; r < rows; ++r) cnt += s_ids[r] == tid;
  if (tid < MOE_E_MAX) s_cnt[tid] = cnt;
  __syncthreads();
  if (tid < a.E) {
    int off = 0;
    for (int e = 0; e < tid; ++e) off += s_cnt[e];
    a.offsets[tid] = off;
    if (tid == a.E - 1) a.offsets[a.E] = off + cnt;
    for (int r = 0; r < rows; ++r)
      if (s_ids[r] == tid) {
        a.sorted_rows[off] = r;
        a.row_pos[r] = off;
        ++off;
      }
  }
}

// ---- grouped GEMM -------------------------------------------------------------------------------------------------------------
struct MoeDev {
  const void* x;     // up: the tokens [T, ldx]; down: h by sorted position [T k, ldx]
  const void* w;     // [E][N, ldw], experts expert_stride elements apart
  const void* wg;    // SwiGLU: the gate weight, same strides
  const void* bias;  // [E, N] or null
  const void* bias_g;
  void* y;           // up with one slice: h [T k, ldy]
  float* ws;         // fp32 partials [nsplit][T k][N] by sorted position (SwiGLU: then the gate half); null: finish in the kernel
  const int32_t* offsets;
  const int32_t* sorted_rows;  // up: routed row of a sorted position; null (down): x rows ARE sorted positions
  int64_t ldx, ldw, estride, ldy;
  int T, topk, E, rows, N, K, act, nsplit, steps;
};

// the epilogue's arguments for expert e: its biases, no residual, no scales
__device__ __forceinline__ SkinnyFinish moe_finish_args(const MoeDev& p, int e) {
  SkinnyFinish f = {};
  f.bias = p.bias ? (const char*)p.bias + (int64_t)e * p.N * 2 : nullptr;
  f.bias_g = p.bias_g ? (const char*)p.bias_g + (int64_t)e * p.N * 2 : nullptr;
  f.y = p.y;
  f.ldy = p.ldy;
  f.N = p.N;
  f.act = p.act;
  return f;
}

// The K loop itself is gemm_skinny_w16_head.inc + gemm_skinny_w16_loop.inc, the decode-step GEMM's.  An expert's rows description:
// the weight starts e * expert_stride into p.w; the fragments its cnt rows reach are live; staged row r < cnt is the x row behind
// sorted position r0 + r, through sorted_rows (up: routed row / top_k is the token) or the position itself (down: h is stored so).
template <typename T, int MF, bool GLU>
__global__ __launch_bounds__(256) void moe_gemm_kernel(const MoeDev p) {
  // the expert's rows: sorted positions [r0, r0 + cnt).  No rows: nothing of this expert is read and no barrier is met, the same
  // for all the workgroup's threads.
  const int e = blockIdx.z;
  const int r0 = max(0, min(p.offsets[e], p.rows));
  const int cnt = min(min(p.offsets[e + 1], p.rows) - r0, MF * 16);  // (an expert has at most T <= 16 MF rows)
  if (cnt <= 0) return;
  const int nf = (cnt + 15) >> 4;
  constexpr bool all_live = false;
  const auto wbase = [&] { return (int64_t)e * p.estride; };
#include "gemm_skinny_w16_head.inc"
  // the x row behind each piece this thread stages (the same for every chunk); -1: a row past the expert's count
  int xsrc[XPT];
#pragma unroll
  for (int i = 0; i < XPT; ++i) {
    const int row = (tid + i * 256) / PCS;
    xsrc[i] = -1;
    if (row < cnt) {
      const int pos = r0 + row;
      xsrc[i] = p.sorted_rows ? min(max(p.sorted_rows[pos] / p.topk, 0), p.T - 1) : pos;
    }
  }
  const auto xhas = [&](int i, int) { return xsrc[i] >= 0; };
  const auto xrow = [&](int i, int) { return xsrc[i]; };
#include "gemm_skinny_w16_loop.inc"

  if (!active) return;
  const int n = n0 + 4 * q;
  if (n >= p.N) return;
  // lane (c, q): rows 16 mf + c of the expert, i.e. sorted positions r0 + 16 mf + c, columns n .. n + 3.  This is skinny_write
  // (gemm_skinny_common.h) at (r0, cnt), written out: through the call these kernels compile to other instructions, not these.
  const SkinnyFinish sd = moe_finish_args(p, e);
#pragma unroll
  for (int mf = 0; mf < MF; ++mf) {
    const int m = mf * 16 + c;
    if (m >= cnt) continue;
    const int pos = r0 + m;
    if (p.ws == nullptr) {
      const float v[4] = {acc[mf][0], acc[mf][1], acc[mf][2], acc[mf][3]};
      float g[4] = {0.f, 0.f, 0.f, 0.f};
      if constexpr (GLU) {
#pragma unroll
        for (int i = 0; i < 4; ++i) g[i] = accg[mf][i];
      }
      skinny_finish<T, GLU, false>(sd, pos, n, v, g);
    } else {
      const int64_t plane = (int64_t)p.rows * p.N;
      float* dst = p.ws + (int64_t)s * plane + (int64_t)pos * p.N + n;
      if ((p.N & 3) == 0) {  // (n + 3 < N then, and the partial rows are 16-byte aligned)
        *(f32x4_t*)dst = acc[mf];
        if constexpr (GLU) *(f32x4_t*)(dst + (int64_t)p.nsplit * plane) = accg[mf];
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (n + i < p.N) {
            dst[i] = acc[mf][i];
            if constexpr (GLU) dst[(int64_t)p.nsplit * plane + i] = accg[mf][i];
          }
      }
    }
  }
}

// Up's second launch: one thread per (sorted position, 4 columns) sums the slices' partials in index order and runs the epilogue
// with the biases of the position's expert: the e with offsets[e] <= pos < offsets[e + 1].
template <typename T, bool GLU>
__global__ __launch_bounds__(256) void moe_up_reduce_kernel(const MoeDev p) {
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
  skinny_finish<T, GLU, false>(moe_finish_args(p, lo), pos, n, v, g);
}

// Down's second launch: one thread per (token, 4 columns).  Per slot j in order: the slices' partials of the slot's sorted
// position in slice order, the bias of its expert, times the routing weight; then the residual and the one rounding.
struct MoeDownDev {
  const float* ws;
  const void* bias;  // [E, N] or null
  const void* res;
  void* y;
  const int32_t* ids;
  const float* weights;
  const int32_t* row_pos;
  int64_t ldy, ldr;
  int T, topk, E, rows, N, nsplit;
};

template <typename T>
__global__ __launch_bounds__(256) void moe_down_finish_kernel(const MoeDownDev p) {
  const int ngrp = (p.N + 3) / 4;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)p.T * ngrp) return;
  const int t = (int)(idx / ngrp), n = (int)(idx % ngrp) * 4;
  const int64_t plane = (int64_t)p.rows * p.N;
  const T* bias = (const T*)p.bias;
  float o[4] = {0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < p.topk; ++j) {
    const int r = t * p.topk + j;
    const int e = min(max(p.ids[r], 0), p.E - 1);
    const int pos = min(max(p.row_pos[r], 0), p.rows - 1);
    const float wj = p.weights[r];
    float z[4], unused[4];
    skinny_slice_sum<false>(p.ws, p.nsplit, plane, p.N, pos, n, z, unused);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int nn = n + i < p.N ? n + i : p.N - 1;  // (clamped: computed, not stored)
      const float zz = z[i] + (bias ? (float)bias[(int64_t)e * p.N + nn] : 0.f);
      o[i] = j == 0 ? wj * zz : o[i] + wj * zz;
    }
  }
  const T* rrow = p.res ? (const T*)p.res + (int64_t)t * p.ldr : nullptr;
  T* yrow = (T*)p.y + (int64_t)t * p.ldy;
  if (rrow) {
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] += (float)rrow[n + i < p.N ? n + i : p.N - 1];
  }
  if (n + 3 < p.N) {
    *(u32x2_t*)(yrow + n) = (u32x2_t){pack2<T>(o[0], o[1]), pack2<T>(o[2], o[3])};
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (n + i < p.N) yrow[n + i] = (T)o[i];
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
using MoeKernel = void (*)(const MoeDev);
struct MoeKernels {
  MoeKernel main[4], reduce;
};
#define MOE_KERNELS(T, GLU) \
  {{moe_gemm_kernel<T, 1, GLU>, moe_gemm_kernel<T, 2, GLU>, moe_gemm_kernel<T, 3, GLU>, moe_gemm_kernel<T, 4, GLU>}, moe_up_reduce_kernel<T, GLU>}
// [MIO_BF16 / MIO_FP16][SwiGLU / plain]
static const MoeKernels MOE_TABLE[2][2] = {{MOE_KERNELS(__bf16, true), MOE_KERNELS(__bf16, false)},
                                           {MOE_KERNELS(_Float16, true), MOE_KERNELS(_Float16, false)}};
#undef MOE_KERNELS

static inline bool moe_aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

extern "C" int mio_moe_route(const void* logits, int64_t ld, int32_t* ids, float* weights, int32_t* expert_offsets,
                             int32_t* sorted_rows, int32_t* row_pos, int32_t T, int32_t E, int32_t top_k, int32_t renormalize,
                             int32_t dtype, void* stream) {
  const std::string fn = "mio_moe_route";
  std::string err;
  if (!moe_route_shape_ok(fn.c_str(), T, top_k, E, err)) return mio_fail(err);
  MIO_CHECK(dtype == MIO_BF16 || dtype == MIO_FP16 || dtype == MIO_FP32, fn + ": dtype must be bf16, fp16 or fp32");
  MIO_CHECK(ld >= E, fn + ": ld < E");
  if (T == 0) return 0;
  MIO_CHECK(logits && ids && weights && expert_offsets && sorted_rows && row_pos, fn + ": null logits or output");
  MIO_CHECK(mio_aligned16(logits), fn + ": logits must be 16-byte aligned");
  MIO_CHECK(moe_aligned4(ids) && moe_aligned4(weights) && moe_aligned4(expert_offsets) && moe_aligned4(sorted_rows) &&
                moe_aligned4(row_pos),
            fn + ": outputs must be aligned to their element size");
  const MoeRouteDev a = {logits, ld, ids, weights, expert_offsets, sorted_rows, row_pos, T, E, top_k, renormalize ? 1 : 0};
  hipStream_t st = (hipStream_t)stream;
  if (dtype == MIO_BF16) hipLaunchKernelGGL(moe_route_kernel<__bf16>, dim3(1), dim3(MOE_RT_NT), 0, st, a);
  else if (dtype == MIO_FP16) hipLaunchKernelGGL(moe_route_kernel<_Float16>, dim3(1), dim3(MOE_RT_NT), 0, st, a);
  else hipLaunchKernelGGL(moe_route_kernel<float>, dim3(1), dim3(MOE_RT_NT), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mio_fail(fn + " launch: " + hipGetErrorString(e));
  return 0;
}

// what mio_moe_up and mio_moe_down check alike: the grouped GEMM's operands (x rows of K, weights [E][N, ldw], outputs of N)
static int moe_gemm_checks(const std::string& fn, int64_t T, int32_t k, int32_t E, int32_t N, int32_t K, int32_t act, int32_t dtype,
                           int64_t ldx, int64_t ldw, int64_t estride, int64_t ldy) {
  std::string err;
  if (!moe_shape_ok(fn.c_str(), T, k, E, N, K, act, err)) return mio_fail(err);
  MIO_CHECK(dtype == MIO_BF16 || dtype == MIO_FP16, fn + ": dtype must be bf16 or fp16");
  MIO_CHECK(ldx % 8 == 0 && ldw % 8 == 0 && ldy % 8 == 0 && estride % 8 == 0, fn + ": row and expert strides must be multiples of 8 elements");
  MIO_CHECK(ldx >= K && ldw >= K && ldy >= N, fn + ": row stride smaller than row length");
  MIO_CHECK(N == 0 || estride >= (int64_t)(N - 1) * ldw + K, fn + ": expert_stride smaller than one expert's weight");
  return 0;
}

extern "C" int mio_moe_up_splits(int32_t T, int32_t top_k, int32_t E, int32_t N, int32_t K, int32_t act) {
  std::string err;
  if (!moe_shape_ok("mio_moe_up_splits", T, top_k, E, N, K, act, err)) return mio_fail(err);
  return moe_plan(T, top_k, E, N, K, act).nsplit;
}

extern "C" size_t mio_moe_up_workspace_bytes(int32_t T, int32_t top_k, int32_t E, int32_t N, int32_t K, int32_t act) {
  std::string err;
  if (!moe_shape_ok("mio_moe_up_workspace_bytes", T, top_k, E, N, K, act, err)) {
    mio_set_error(err);
    return 0;
  }
  return moe_up_workspace_bytes(moe_plan(T, top_k, E, N, K, act), N);
}

extern "C" int mio_moe_down_splits(int32_t T, int32_t top_k, int32_t E, int32_t N, int32_t K) {
  std::string err;
  if (!moe_shape_ok("mio_moe_down_splits", T, top_k, E, N, K, MIO_ACT_NONE, err)) return mio_fail(err);
  return moe_plan(T, top_k, E, N, K, MIO_ACT_NONE).nsplit;
}

extern "C" size_t mio_moe_down_workspace_bytes(int32_t T, int32_t top_k, int32_t E, int32_t N, int32_t K) {
  std::string err;
  if (!moe_shape_ok("mio_moe_down_workspace_bytes", T, top_k, E, N, K, MIO_ACT_NONE, err)) {
    mio_set_error(err);
    return 0;
  }
  return moe_down_workspace_bytes(moe_plan(T, top_k, E, N, K, MIO_ACT_NONE), N);
}

extern "C" int mio_moe_up(const void* x, const void* w_up, const void* b_up, const void* w_gate, const void* b_gate,
                          const int32_t* expert_offsets, const int32_t* sorted_rows, void* h, void* workspace, int32_t T,
                          int32_t top_k, int32_t E, int32_t I, int32_t d, int64_t ldx, int64_t ldw, int64_t expert_stride,
                          int64_t ldh, int32_t act, int32_t dtype, void* stream) {
  const std::string fn = "mio_moe_up";
  if (int rc = moe_gemm_checks(fn, T, top_k, E, I, d, act, dtype, ldx, ldw, expert_stride, ldh)) return rc;
  const bool glu = act == MIO_ACT_SWIGLU;
  MIO_CHECK(glu == (w_gate != nullptr), fn + ": w_gate is required iff act == SWIGLU");
  MIO_CHECK(glu || b_gate == nullptr, fn + ": b_gate belongs to act == SWIGLU");
  MIO_CHECK(w_up && (T == 0 || (x && h && expert_offsets && sorted_rows)), fn + ": x, w_up, h, expert_offsets, sorted_rows must be non-null");
  MIO_CHECK(mio_aligned16(x) && mio_aligned16(w_up) && mio_aligned16(w_gate) && mio_aligned16(b_up) && mio_aligned16(b_gate) &&
                mio_aligned16(h) && mio_aligned16(workspace) && moe_aligned4(expert_offsets) && moe_aligned4(sorted_rows),
            fn + ": pointers must be 16-byte aligned (the route's arrays: 4-byte)");
  const MoePlan pl = moe_plan(T, top_k, E, I, d, act);
  if (T == 0 || I == 0) return 0;
  MIO_CHECK(pl.nsplit == 1 || workspace != nullptr, fn + ": workspace required (mio_moe_up_workspace_bytes) when the plan splits K");
  MoeDev p;
  p.x = x; p.w = w_up; p.wg = w_gate; p.bias = b_up; p.bias_g = b_gate; p.y = h;
  p.ws = pl.nsplit > 1 ? (float*)workspace : nullptr;
  p.offsets = expert_offsets; p.sorted_rows = sorted_rows;
  p.ldx = ldx; p.ldw = ldw; p.estride = expert_stride; p.ldy = ldh;
  p.T = T; p.topk = top_k; p.E = E; p.rows = pl.rows; p.N = I; p.K = d; p.act = act; p.nsplit = pl.nsplit; p.steps = pl.steps;
  const MoeKernels& k = MOE_TABLE[dtype == MIO_BF16 ? 0 : 1][glu ? 0 : 1];
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k.main[pl.mf - 1], dim3((unsigned)pl.tiles_n, (unsigned)pl.nsplit, (unsigned)E), dim3(256), 0, st, p);
  if (pl.nsplit > 1) {
    const int64_t threads = (int64_t)pl.rows * ((I + 3) / 4);
    hipLaunchKernelGGL(k.reduce, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, p);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mio_fail(fn + " launch: " + hipGetErrorString(e));
  return 0;
}

extern "C" int mio_moe_down(const void* h, const void* w_down, const void* b_down, const int32_t* ids, const float* weights,
                            const int32_t* expert_offsets, const int32_t* row_pos, const void* residual, void* y, void* workspace,
                            int32_t T, int32_t top_k, int32_t E, int32_t d, int32_t I, int64_t ldh, int64_t ldw,
                            int64_t expert_stride, int64_t ldy, int64_t ldr, int32_t dtype, void* stream) {
  const std::string fn = "mio_moe_down";
  if (int rc = moe_gemm_checks(fn, T, top_k, E, d, I, MIO_ACT_NONE, dtype, ldh, ldw, expert_stride, ldy)) return rc;
  MIO_CHECK(!residual || (ldr % 8 == 0 && ldr >= d), fn + ": ldr must be a multiple of 8 elements and at least d");
  MIO_CHECK(w_down && (T == 0 || (h && y && ids && weights && expert_offsets && row_pos)),
            fn + ": h, w_down, y, ids, weights, expert_offsets, row_pos must be non-null");
  MIO_CHECK(mio_aligned16(h) && mio_aligned16(w_down) && mio_aligned16(b_down) && mio_aligned16(residual) && mio_aligned16(y) &&
                mio_aligned16(workspace) && moe_aligned4(ids) && moe_aligned4(weights) && moe_aligned4(expert_offsets) &&
                moe_aligned4(row_pos),
            fn + ": pointers must be 16-byte aligned (the route's arrays: 4-byte)");
  const MoePlan pl = moe_plan(T, top_k, E, d, I, MIO_ACT_NONE);
  if (T == 0 || d == 0) return 0;
  MIO_CHECK(workspace != nullptr, fn + ": workspace required (mio_moe_down_workspace_bytes)");
  MoeDev p;
  p.x = h; p.w = w_down; p.wg = nullptr; p.bias = nullptr; p.bias_g = nullptr; p.y = nullptr;
  p.ws = (float*)workspace;
  p.offsets = expert_offsets; p.sorted_rows = nullptr;
  p.ldx = ldh; p.ldw = ldw; p.estride = expert_stride; p.ldy = 0;
  p.T = T; p.topk = top_k; p.E = E; p.rows = pl.rows; p.N = d; p.K = I; p.act = MIO_ACT_NONE; p.nsplit = pl.nsplit; p.steps = pl.steps;
  const MoeDownDev f = {(const float*)workspace, b_down, residual, y, ids, weights, row_pos, ldy, ldr, T, top_k, E, pl.rows, d, pl.nsplit};
  const MoeKernels& k = MOE_TABLE[dtype == MIO_BF16 ? 0 : 1][1];
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k.main[pl.mf - 1], dim3((unsigned)pl.tiles_n, (unsigned)pl.nsplit, (unsigned)E), dim3(256), 0, st, p);
  const int64_t threads = (int64_t)T * ((d + 3) / 4);
  if (dtype == MIO_BF16) hipLaunchKernelGGL(moe_down_finish_kernel<__bf16>, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, f);
  else hipLaunchKernelGGL(moe_down_finish_kernel<_Float16>, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, f);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mio_fail(fn + " launch: " + hipGetErrorString(e));
  return 0;
}

// What the mixture-of-experts units share on the device (moe.hip, moe_w8.hip: decode steps, T <= 64, on 16-bit and e4m3fn expert
// weights; moe_prefill.hip: tall inputs): a token's routing -- the order, the choice, the softmax weights -- as one device
// function, so that the two routers cannot drift, and down's finishing launch, which has no bound on T: one thread per (token, 4
// columns) over the slots in slot order, with the expert's scale in front of the bias where the weights carry scales.  What only
// the two decode units share is moe_gemm_common.h.
#pragma once
#include <cfloat>

#include "gemm_skinny_common.h"

typedef unsigned long long moe_u64;

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

// One token's routing by one wave: row is its E <= 256 logits.  A lane holds the logits of experts lane, lane + 64, lane + 128,
// lane + 192 as fp32 (exact for bf16 / fp16) and their order-preserving keys; top_k rounds of a wave max over (key, ~index) pick
// the experts in the stated order, and the softmax sums run in a fixed shape (a lane's four in index order, then the xor
// butterfly), so reruns give the same bits.  Lane j < top_k ends with slot j's expert in my_id and its weight in my_w.
template <typename L>
__device__ __forceinline__ void moe_route_token(const L* row, int E, int topk, int renorm, int lane, int& my_id, float& my_w) {
  const uint32_t key_ninf = moe_key(-INFINITY);
  float x[4];
  moe_u64 cand[4];
  moe_u64 best = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int e = lane + 64 * i;
    x[i] = -INFINITY;
    cand[i] = 0;  // (below every expert's: the smallest key, -inf's, is not 0)
    if (e < E) {
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
  my_id = lane;  // lane j < top_k ends up with slot j
  my_w = 0.f;
  if (kmax != key_ninf) {  // (else no finite logit: ids 0 .. top_k - 1, weights 0)
    const float m = fminf(moe_unkey(kmax), FLT_MAX);
    float z = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) z += (lane + 64 * i < E) ? moe_w(x[i], m) : 0.f;
    for (int o = 32; o >= 1; o >>= 1) z += __shfl_xor(z, o, 64);
    for (int j = 0; j < topk; ++j) {
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
    if (renorm) {
      float s = 0.f;
      for (int j = 0; j < topk; ++j) s += __shfl(my_w, j, 64);  // slot order
      my_w = my_w / s;  // (s > 0: slot 0 is the maximum, whose weight is 1 / z)
    }
  }
}

// Down's second launch: one thread per (token, 4 columns).  Per slot j in order: the slices' partials of the slot's sorted
// position in slice order, z = sum + bias[e, n] with the slot's expert e (SCALED, e4m3fn expert weights: fma(sum, scale[e, n],
// bias[e, n]), the scale going in before the routing weight), times the routing weight; then the residual and the one rounding.
// UNIT names the including unit (0: moe.hip, 1: moe_prefill.hip, 2: moe_w8.hip, 3: moe_w4.hip), so that each object carries a
// kernel symbol of its own.
struct MoeDownDev {
  const float* ws;
  const float* scale;  // SCALED only: fp32 [E, N]; null otherwise
  const void* bias;  // [E, N] or null
  const void* res;
  void* y;
  const int32_t* ids;
  const float* weights;
  const int32_t* row_pos;
  int64_t ldy, ldr;
  int T, topk, E, rows, N, nsplit;
};

template <typename T, int UNIT, bool SCALED = false>
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
      const int64_t at = (int64_t)e * p.N + nn;
      float zz;
      if constexpr (SCALED) zz = __builtin_fmaf(z[i], p.scale[at], bias ? (float)bias[at] : 0.f);
      else zz = z[i] + (bias ? (float)bias[at] : 0.f);
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

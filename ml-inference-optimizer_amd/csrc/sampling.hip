// On-device token sampling for CDNA4 (gfx950): greedy, temperature, top-k, top-p and min-p over a [B, V] logits matrix in one
// launch, per-row parameters and the caller's uniforms read from device memory (semantics: include/mio_hip.h).
//
// One workgroup of 1024 threads (16 waves) per row.  The row is never sorted.  Tokens are ordered by the order-preserving
// integer key of the stored logit (16 bits for bf16 / fp16, 32 for fp32; NaN takes -inf's key, -0 takes +0's) and, inside a
// key, by index.  Every filter keeps a prefix of that order, so the kept set is always "key > K, or key == K and index <= I":
//   max pass      max of (key, ~index): the row maximum m and the greedy token
//   top-k         radix select on the key, 8 bits a level, by COUNT: the key K whose ties straddle rank k; where the cut
//                 falls inside the ties, the index I of the last one kept
//   top-p         the mass Z1 of that set, then the same select by MASS: the key at which the descending mass crosses p * Z1
//   min-p         a threshold on w itself (w_max = 1): a predicate of the final pass, no select
//   final pass    kept count, mass Z and the per-wave masses of the kept set; the draw; the probabilities
// Masses are 64-bit fixed point, quantum 2^-40: w = exp2((x - m) * (log2 e / T)) in fp32, truncated to a multiple of 2^-40.
// Integer sums are exactly associative, so the LDS histogram adds (integer atomics; no float atomic anywhere) and the
// reductions give the same bits in any order.  A row of 2^20 tokens sums to at most 2^60.
//
// Element-to-thread assignment (fixed for a row, the same in every pass).  The row is cut into the 16-byte chunks of global
// memory it touches (8 or 4 elements; the first and the last may be partial: they are loaded element by element under the
// row's bounds, every other chunk with one 16-byte load -- nothing outside [row, row + V) is read).  Wave w owns the chunks
// [w * cpw, (w + 1) * cpw); lane l takes chunk l, l + 64, ... of them.  So index order is wave, then iteration, then lane, then
// element: a prefix in index order (the tie cut, the draw) is a sum over whole waves, a walk of ONE wave's iterations with a
// wave scan each, and a walk of one lane's chunk.
//
// Histogram.  Logits crowd into a few exponent bins, so the 256 bins are kept in 8 copies, a lane adding into copy lane & 7:
// the lanes of a wave that meet in one bin spread over 8 addresses (8 banks).  The copies are summed by the 256 threads that
// scan the bins.
//
// Residency.  A 16-bit row of up to 65536 tokens (128 KiB of the 160 KiB LDS, next to 16.5 KiB of histogram and scratch) is
// canonicalised into LDS by the max pass and every later pass reads it there; longer rows and fp32 rows are re-read from L2.
#include <cfloat>
#include <cmath>
#include <mutex>

#include "mio_common.h"

constexpr int SP_NT = 1024, SP_NW = SP_NT / 64;
constexpr int SP_BINS = 256, SP_COPIES = 8;
constexpr int SP_HIST_BYTES = SP_BINS * SP_COPIES * 8;  // 16 KiB of 64-bit bins
constexpr int SP_MISC_WORDS = 64;                       // 64-bit words of reduction scratch behind the histogram
constexpr int SP_FIXED_BYTES = SP_HIST_BYTES + SP_MISC_WORDS * 8;
constexpr int SP_RESIDENT_V = 65536;                    // 16-bit rows up to this many tokens live in LDS
constexpr float SP_ONE = 0x1p40f;                       // 1.0 in the masses' fixed point

typedef unsigned long long u64;

// ---- stored formats: raw bits, the canonical form (NaN -> -inf, -0 -> +0), the value and the order-preserving key ----------
template <typename T>
struct SpT;
template <>
struct SpT<__bf16> {
  using raw = uint16_t;
  static constexpr int KB = 16, EPC = 8;
  static constexpr uint32_t SIGN = 0x8000u, MAG = 0x7fffu, INF = 0x7f80u;
  static __device__ __forceinline__ float val(uint32_t h) { return __uint_as_float(h << 16); }
};
template <>
struct SpT<_Float16> {
  using raw = uint16_t;
  static constexpr int KB = 16, EPC = 8;
  static constexpr uint32_t SIGN = 0x8000u, MAG = 0x7fffu, INF = 0x7c00u;
  static __device__ __forceinline__ float val(uint32_t h) { return (float)__builtin_bit_cast(_Float16, (uint16_t)h); }
};
template <>
struct SpT<float> {
  using raw = uint32_t;
  static constexpr int KB = 32, EPC = 4;
  static constexpr uint32_t SIGN = 0x80000000u, MAG = 0x7fffffffu, INF = 0x7f800000u;
  static __device__ __forceinline__ float val(uint32_t h) { return __uint_as_float(h); }
};

template <typename T>
__device__ __forceinline__ uint32_t sp_canon(uint32_t h) {
  using S = SpT<T>;
  const uint32_t mag = h & S::MAG;
  if (mag == 0) return 0;
  if (mag > S::INF) return S::SIGN | S::INF;
  return h;
}
template <typename T>
__device__ __forceinline__ uint32_t sp_key(uint32_t h) {  // of a canonical h
  using S = SpT<T>;
  return (h & S::SIGN) ? (~h & (S::SIGN | S::MAG)) : (h | S::SIGN);
}
template <typename T>
__device__ __forceinline__ uint32_t sp_unkey(uint32_t k) {
  using S = SpT<T>;
  return (k & S::SIGN) ? (k ^ S::SIGN) : (~k & (S::SIGN | S::MAG));
}
// the value a stored logit counts as: +inf is the largest finite fp32
template <typename T>
__device__ __forceinline__ float sp_val(uint32_t h) {
  return fminf(SpT<T>::val(h), FLT_MAX);
}

// ---- the row ---------------------------------------------------------------------------------------------------------------
struct SpRow {
  const uint8_t* g;  // the 16-byte aligned address at or below the row's first element
  int off;           // elements between g and the row's first element
  int V;
  int nck;           // 16-byte chunks the row touches
  int cpw;           // chunks per wave
};

// chunk c of the row as canonical raw values; elements outside the row are 0 and are never looked at
template <typename T, bool FROM_LDS>
__device__ __forceinline__ void sp_chunk(const SpRow& r, const uint8_t* lds_row, int c, uint32_t* v) {
  using S = SpT<T>;
  using raw = typename S::raw;
  constexpr int E = S::EPC;
  if (FROM_LDS) {
    const u32x4_t q = *(const u32x4_t*)(lds_row + (size_t)c * 16);
#pragma unroll
    for (int e = 0; e < E; ++e) v[e] = sizeof(raw) == 2 ? (q[e >> 1] >> ((e & 1) * 16)) & 0xffffu : q[e];
    return;
  }
  const int lo = c * E - r.off;
  const uint8_t* p = r.g + (size_t)c * 16;
  if (lo >= 0 && lo + E <= r.V) {
    const u32x4_t q = *(const u32x4_t*)p;
#pragma unroll
    for (int e = 0; e < E; ++e) v[e] = sp_canon<T>(sizeof(raw) == 2 ? (q[e >> 1] >> ((e & 1) * 16)) & 0xffffu : q[e]);
  } else {
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int i = lo + e;
      v[e] = (i >= 0 && i < r.V) ? sp_canon<T>((uint32_t)((const raw*)p)[e]) : 0u;
    }
  }
}

// f(index, canonical raw value) for every element this thread owns, in ascending index order
template <typename T, bool FROM_LDS, typename F>
__device__ __forceinline__ void sp_for_each(const SpRow& r, const uint8_t* lds_row, F&& f) {
  constexpr int E = SpT<T>::EPC;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int c_end = min(r.nck, (wave + 1) * r.cpw);
  for (int c = wave * r.cpw + lane; c < c_end; c += 64) {
    uint32_t v[E];
    sp_chunk<T, FROM_LDS>(r, lds_row, c, v);
    const int lo = c * E - r.off;
#pragma unroll
    for (int e = 0; e < E; ++e)
      if ((unsigned)(lo + e) < (unsigned)r.V) f(lo + e, v[e]);
  }
}

// ---- reductions over the workgroup (integers: any order gives the same bits) ------------------------------------------------
__device__ __forceinline__ u64 sp_wave_sum(u64 v) {
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ u64 sp_wave_max(u64 v) {
  for (int o = 32; o >= 1; o >>= 1) {
    const u64 t = __shfl_xor(v, o, 64);
    v = t > v ? t : v;
  }
  return v;
}
// inclusive scan over the lanes of a wave
__device__ __forceinline__ u64 sp_wave_scan(u64 v) {
  const int lane = threadIdx.x & 63;
  for (int o = 1; o < 64; o <<= 1) {
    const u64 t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}
// every wave's total into slot[0 .. 16) and the workgroup's sum to every thread; slot is free to reuse after the next barrier
__device__ __forceinline__ u64 sp_block_sum(u64 v, u64* slot) {
  v = sp_wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
  __syncthreads();
  u64 s = 0;
#pragma unroll
  for (int w = 0; w < SP_NW; ++w) s += slot[w];
  return s;
}
__device__ __forceinline__ u64 sp_block_max(u64 v, u64* slot) {
  v = sp_wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
  __syncthreads();
  u64 s = 0;
#pragma unroll
  for (int w = 0; w < SP_NW; ++w) s = slot[w] > s ? slot[w] : s;
  return s;
}

// ---- the weight ------------------------------------------------------------------------------------------------------------
// w = exp2((x - m) * c), c = log2(e) / T, in fp32; 1 at the maximum, 0 for -inf and where the product is not a number
__device__ __forceinline__ float sp_w(float x, float m, float c) {
  const float d = x - m;
  const float t = d * c;
  const float w = (t == t) ? fast_exp2(t) : 0.f;
  return d == 0.f ? 1.f : fminf(w, 1.f);
}
// w in 64-bit fixed point, truncated to a multiple of 2^-40 (w <= 1: at most 2^40)
__device__ __forceinline__ u64 sp_fix(float w) {
  const float s = w * SP_ONE;                        // exact: a power of two
  const uint32_t hi = (uint32_t)(s * 0x1p-32f);      // truncates
  const float rem = s - (float)hi * 0x1p32f;         // exact
  return ((u64)hi << 32) | (u64)(uint32_t)rem;
}

// the kept prefix of the order: key > K, or key == K and index <= I
struct SpCut {
  uint32_t K;
  int I;
  __device__ __forceinline__ bool has(uint32_t key, int idx) const { return key > K || (key == K && idx <= I); }
};

// ---- radix select ------------------------------------------------------------------------------------------------------------
// Over the elements of `in`, each worth val(h) (1, or its fixed-point mass), in descending key order: the key K at which the
// running sum reaches P, i.e. above(K) < P <= above(K) + bin(K), above(K) the worth of the keys greater than K and bin(K) > 0
// the worth of key K itself.  False (nothing written) when the whole of `in` is worth less than P.
template <typename T, bool FROM_LDS, typename Val>
__device__ __forceinline__ bool sp_select(const SpRow& r, const uint8_t* lds_row, u64* hist, u64* misc, const SpCut in, const u64 P,
                                          Val&& val, uint32_t& K, u64& above, u64& bin) {
  constexpr int LV = SpT<T>::KB / 8;
  const int tid = threadIdx.x, lane = tid & 63;
  uint32_t prefix = 0;
  u64 A = 0, binval = 0;
  for (int lvl = LV - 1; lvl >= 0; --lvl) {
    const int shift = 8 * lvl;
    __syncthreads();
    hist[tid] = 0;
    hist[tid + SP_NT] = 0;
    if (tid == 0) misc[SP_NW] = ~0ull;
    __syncthreads();
    sp_for_each<T, FROM_LDS>(r, lds_row, [&](int idx, uint32_t h) __attribute__((always_inline)) {
      const uint32_t key = sp_key<T>(h);
      const bool match = lvl == LV - 1 || (key >> (shift + 8)) == prefix;
      if (match && in.has(key, idx)) atomicAdd(&hist[((key >> shift) & 255u) * SP_COPIES + (lane & (SP_COPIES - 1))], val(h));
    });
    __syncthreads();
    // thread i < 256 owns bin 255 - i: the running sum in descending key order
    u64 s = 0;
    const int b = 255 - tid;
    if (tid < SP_BINS) {
#pragma unroll
      for (int c = 0; c < SP_COPIES; ++c) s += hist[b * SP_COPIES + c];
    }
    u64 incl = sp_wave_scan(s);
    if (lane == 63) misc[tid >> 6] = incl;
    __syncthreads();
    if (tid < SP_BINS) {
      for (int w = 0; w < (tid >> 6); ++w) incl += misc[w];
      const u64 excl = incl - s, need = P - A;
      if (s > 0 && excl < need && need <= incl) {
        misc[SP_NW] = (u64)b;
        misc[SP_NW + 1] = A + excl;
        misc[SP_NW + 2] = s;
      }
    }
    __syncthreads();
    const u64 d = misc[SP_NW];
    if (d == ~0ull) return false;
    prefix = (prefix << 8) | (uint32_t)d;
    A = misc[SP_NW + 1];
    binval = misc[SP_NW + 2];
  }
  K = prefix, above = A, bin = binval;
  return true;
}

// ---- a prefix in index order ---------------------------------------------------------------------------------------------------
// The smallest index whose inclusive running sum of val(index, h), taken in index order, exceeds target.  wave_tot[0 .. 16) holds
// every wave's sum of val and target is below their total.  One wave walks its own chunks; the result comes back through misc.
template <typename T, bool FROM_LDS, typename Val>
__device__ __forceinline__ int sp_find(const SpRow& r, const uint8_t* lds_row, const u64* wave_tot, u64* res, const u64 target,
                                       Val&& val) {
  constexpr int E = SpT<T>::EPC;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (threadIdx.x == 0) *res = 0;
  __syncthreads();
  u64 pre = 0;
  int ws = -1;
#pragma unroll
  for (int w = 0; w < SP_NW; ++w) {
    const u64 t = wave_tot[w];
    if (ws < 0 && target < pre + t) ws = w;
    if (ws < 0) pre += t;
  }
  if (wave == ws) {
    u64 run = pre;
    const int c0 = wave * r.cpw, c_end = min(r.nck, c0 + r.cpw);
    for (int cb = c0; cb < c_end; cb += 64) {  // the same trip count in every lane
      const int c = cb + lane;
      uint32_t v[E];
      u64 mine = 0;
      const int lo = c * E - r.off;
      if (c < c_end) {
        sp_chunk<T, FROM_LDS>(r, lds_row, c, v);
#pragma unroll
        for (int e = 0; e < E; ++e)
          if ((unsigned)(lo + e) < (unsigned)r.V) mine += val(lo + e, v[e]);
      }
      const u64 incl = sp_wave_scan(mine);
      const u64 tot = __shfl(incl, 63, 64);
      if (target < run + tot) {
        u64 at = run + incl - mine;
        if (c < c_end && at <= target && target < at + mine) {
          int found = -1;
#pragma unroll
          for (int e = 0; e < E; ++e)
            if ((unsigned)(lo + e) < (unsigned)r.V) {
              at += val(lo + e, v[e]);
              if (found < 0 && target < at) found = lo + e;
            }
          *res = (u64)found;
        }
        break;
      }
      run += tot;
    }
  }
  __syncthreads();
  return (int)*res;
}

struct SpArgs {
  const void* logits;
  int64_t ld;
  const float* temperature;
  const int32_t* top_k;
  const float* top_p;
  const float* min_p;
  const float* u;
  int64_t* tokens;
  int32_t* kept;
  float* probs;
  int64_t ld_probs;
  int32_t V;
};

// a row with a single answer: token t (or -1: none), probabilities one-hot or zero
__device__ __forceinline__ void sp_write_single(const SpArgs& a, int b, int t) {
  if (threadIdx.x == 0) {
    if (a.tokens) a.tokens[b] = t;
    if (a.kept) a.kept[b] = t >= 0 ? 1 : 0;
  }
  if (a.probs) {
    float* pr = a.probs + (int64_t)b * a.ld_probs;
    for (int i = threadIdx.x; i < a.V; i += SP_NT) pr[i] = i == t ? 1.f : 0.f;
  }
}

template <typename T, bool RES>
__global__ __launch_bounds__(SP_NT) void sample_tokens_kernel(const SpArgs a) {
  using S = SpT<T>;
  using raw = typename S::raw;
  constexpr int E = S::EPC;
  extern __shared__ __attribute__((aligned(16))) uint8_t sp_smem[];
  u64* hist = (u64*)sp_smem;
  u64* misc = hist + SP_BINS * SP_COPIES;       // [0, 16) wave slots, [16, 19) the select's answer, [20] a found index
  u64* wtot = misc + 32;                        // [0, 16) the per-wave sums a prefix search runs on
  uint8_t* lds_row = sp_smem + SP_FIXED_BYTES;  // the resident row, chunk by chunk

  const int b = blockIdx.x, tid = threadIdx.x;
  const int V = a.V;
  const uint8_t* row0 = (const uint8_t*)a.logits + (int64_t)b * a.ld * (int64_t)sizeof(raw);
  SpRow r;
  r.off = (int)(((uintptr_t)row0 & 15) / sizeof(raw));
  r.g = row0 - r.off * (int)sizeof(raw);
  r.V = V;
  r.nck = (r.off + V + E - 1) / E;
  r.cpw = (r.nck + SP_NW - 1) / SP_NW;

  // ---- max pass: the first token of the order; a resident row goes into LDS
  u64 best = 0;
  {
    const int wave = tid >> 6, lane = tid & 63;
    const int c_end = min(r.nck, (wave + 1) * r.cpw);
    for (int c = wave * r.cpw + lane; c < c_end; c += 64) {
      uint32_t v[E];
      sp_chunk<T, false>(r, nullptr, c, v);
      if (RES) {
        u32x4_t q;
#pragma unroll
        for (int e = 0; e < 4; ++e) q[e] = sizeof(raw) == 2 ? (v[2 * e] | (v[2 * e + 1] << 16)) : v[e];
        *(u32x4_t*)(lds_row + (size_t)c * 16) = q;
      }
      const int lo = c * E - r.off;
#pragma unroll
      for (int e = 0; e < E; ++e)
        if ((unsigned)(lo + e) < (unsigned)V) {
          const u64 cand = ((u64)sp_key<T>(v[e]) << 32) | (uint32_t)~(uint32_t)(lo + e);
          best = cand > best ? cand : best;
        }
    }
  }
  best = sp_block_max(best, misc);  // its barriers also publish the resident row
  const uint32_t kmax = (uint32_t)(best >> 32);
  const int imax = (int)~(uint32_t)best;
  if (kmax == sp_key<T>(S::SIGN | S::INF)) {  // no finite logit
    sp_write_single(a, b, -1);
    return;
  }
  const float temp = a.temperature[b];
  if (!(temp > 0.f)) {  // greedy: T <= 0 or NaN
    sp_write_single(a, b, imax);
    return;
  }
  const float m = sp_val<T>(sp_unkey<T>(kmax));
  const float cT = 1.4426950408889634f / temp;
  auto wfix = [&](uint32_t h) __attribute__((always_inline)) { return sp_fix(sp_w(sp_val<T>(h), m, cT)); };

  const int k = a.top_k ? a.top_k[b] : 0;
  const float p = a.top_p ? a.top_p[b] : 1.f;
  const float q = a.min_p ? a.min_p[b] : 0.f;
  const bool k_on = k > 0 && k < V, p_on = p < 1.f, q_on = q > 0.f;

  SpCut cut = {0u, V};  // everything
  if (k_on) {
    uint32_t K;
    u64 above, bin;
    if (sp_select<T, RES>(r, lds_row, hist, misc, cut, (u64)k, [](uint32_t) { return (u64)1; }, K, above, bin)) {
      const u64 n = (u64)k - above;  // ties of K that stay, 1 <= n <= bin
      int I = V;
      if (n < bin) {
        u64 cnt = 0;
        sp_for_each<T, RES>(r, lds_row, [&](int, uint32_t h) __attribute__((always_inline)) { cnt += sp_key<T>(h) == K; });
        cnt = sp_wave_sum(cnt);
        __syncthreads();
        if ((tid & 63) == 0) wtot[tid >> 6] = cnt;
        __syncthreads();
        I = sp_find<T, RES>(r, lds_row, wtot, misc + 20, n - 1,
                            [&](int, uint32_t h) __attribute__((always_inline)) { return (u64)(sp_key<T>(h) == K); });
      }
      cut.K = K, cut.I = I;
    }
  }
  if (p_on) {
    u64 z1 = 0;
    sp_for_each<T, RES>(r, lds_row, [&](int idx, uint32_t h) __attribute__((always_inline)) {
      if (cut.has(sp_key<T>(h), idx)) z1 += wfix(h);
    });
    z1 = sp_block_sum(z1, misc);
    // the first token with "mass before it" >= P is the first one out; the first token of all (mass before it 0) always stays
    u64 P = 1;
    if (p > 0.f) {
      const double t = ceil((double)p * (double)z1);
      P = t < 1.0 ? 1 : (u64)t;
      P = P > z1 ? z1 : P;
    }
    uint32_t K;
    u64 above, bin;
    if (sp_select<T, RES>(r, lds_row, hist, misc, cut, P, wfix, K, above, bin)) {
      const u64 wk = wfix(sp_unkey<T>(K));  // > 0: bin > 0
      const u64 n = (P - above + wk - 1) / wk, c = bin / wk;
      int I = K == cut.K ? cut.I : V;
      if (n < c) {
        const SpCut in = cut;
        u64 cnt = 0;
        sp_for_each<T, RES>(r, lds_row, [&](int idx, uint32_t h) __attribute__((always_inline)) {
          const uint32_t key = sp_key<T>(h);
          cnt += key == K && in.has(key, idx);
        });
        cnt = sp_wave_sum(cnt);
        __syncthreads();
        if ((tid & 63) == 0) wtot[tid >> 6] = cnt;
        __syncthreads();
        I = sp_find<T, RES>(r, lds_row, wtot, misc + 20, n - 1, [&](int idx, uint32_t h) __attribute__((always_inline)) {
          const uint32_t key = sp_key<T>(h);
          return (u64)(key == K && in.has(key, idx));
        });
      }
      cut.K = K, cut.I = I;
    }
  }

  // ---- final pass: the kept set S3 = cut and w >= q (the first token always); its count, its mass, the mass per wave
  auto kept_w = [&](int idx, uint32_t h, float& w) __attribute__((always_inline)) {
    w = sp_w(sp_val<T>(h), m, cT);
    return cut.has(sp_key<T>(h), idx) && (!q_on || w >= q || idx == imax);
  };
  u64 mass = 0, cnt = 0;
  sp_for_each<T, RES>(r, lds_row, [&](int idx, uint32_t h) __attribute__((always_inline)) {
    float w;
    if (kept_w(idx, h, w)) mass += sp_fix(w), cnt += 1;
  });
  cnt = sp_block_sum(cnt, misc);
  mass = sp_wave_sum(mass);
  __syncthreads();
  if ((tid & 63) == 0) wtot[tid >> 6] = mass;
  __syncthreads();
  u64 Z = 0;
#pragma unroll
  for (int w = 0; w < SP_NW; ++w) Z += wtot[w];  // >= 2^40: the first token is kept and weighs 1
  if (tid == 0 && a.kept) a.kept[b] = (int32_t)cnt;

  if (a.tokens) {
    float u = a.u[b];
    u = u >= 0.f ? u : 0.f;  // NaN as well
    u = fminf(u, 0x1.fffffep-1f);
    u64 target = (u64)((double)u * (double)Z);
    target = target < Z ? target : Z - 1;
    const int tok = sp_find<T, RES>(r, lds_row, wtot, misc + 20, target, [&](int idx, uint32_t h) __attribute__((always_inline)) {
      float w;
      return kept_w(idx, h, w) ? sp_fix(w) : (u64)0;
    });
    if (tid == 0) a.tokens[b] = tok;
  }
  if (a.probs) {
    const float zf = (float)((double)Z * 0x1p-40);
    float* pr = a.probs + (int64_t)b * a.ld_probs;
    sp_for_each<T, RES>(r, lds_row, [&](int idx, uint32_t h) __attribute__((always_inline)) {
      float w;
      pr[idx] = kept_w(idx, h, w) ? w / zf : 0.f;
    });
  }
}

// ---- host --------------------------------------------------------------------------------------------------------------------
template <typename T, bool RES>
static int sp_launch(const SpArgs& a, int32_t B, size_t smem, hipStream_t st) {
  auto kern = sample_tokens_kernel<T, RES>;
  if (RES) {  // above the 64 KiB a kernel gets without asking
    static std::once_flag once;
    static hipError_t ea = hipSuccess;
    std::call_once(once, [&] {
      ea = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, SP_FIXED_BYTES + (SP_RESIDENT_V + 16) * 2);
    });
    if (ea != hipSuccess) return mio_fail(std::string("mio_sample_tokens: hipFuncSetAttribute: ") + hipGetErrorString(ea));
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)B), dim3(SP_NT), smem, st, a);
  return 0;
}

extern "C" int mio_sample_tokens(const void* logits, int64_t ld, const float* temperature, const int32_t* top_k,
                                 const float* top_p, const float* min_p, const float* u, int64_t* tokens_out, int32_t* kept_out,
                                 float* probs_out, int64_t ld_probs, int32_t B, int32_t V, int32_t dtype, void* stream) {
  const std::string fn = "mio_sample_tokens";
  MIO_CHECK(dtype == MIO_BF16 || dtype == MIO_FP16 || dtype == MIO_FP32, fn + ": dtype must be bf16, fp16 or fp32");
  MIO_CHECK(V >= 1 && V <= (1 << 20), fn + ": V must be in [1, 2^20]");
  MIO_CHECK(B >= 0, fn + ": B must not be negative");
  MIO_CHECK(tokens_out || kept_out || probs_out, fn + ": every output is null");
  MIO_CHECK(ld >= V, fn + ": ld < V");
  MIO_CHECK(!probs_out || ld_probs >= V, fn + ": ld_probs < V");
  if (B == 0) return 0;
  MIO_CHECK(logits && temperature, fn + ": null logits or temperature");
  MIO_CHECK(u || !tokens_out, fn + ": null u");
  MIO_CHECK(mio_aligned16(logits), fn + ": 16-byte alignment (logits)");
  MIO_CHECK((((uintptr_t)temperature | (uintptr_t)top_k | (uintptr_t)top_p | (uintptr_t)min_p | (uintptr_t)u |
              (uintptr_t)kept_out | (uintptr_t)probs_out) & 3) == 0 && ((uintptr_t)tokens_out & 7) == 0,
            fn + ": parameter and output arrays must be aligned to their element size");
  const SpArgs a = {logits, ld, temperature, top_k, top_p, min_p, u, tokens_out, kept_out, probs_out, ld_probs, V};
  hipStream_t st = (hipStream_t)stream;
  const bool res = dtype != MIO_FP32 && V <= SP_RESIDENT_V;
  // the resident row: every chunk the row can touch (up to 7 elements of slack in front of it)
  const size_t smem = SP_FIXED_BYTES + (res ? (size_t)((V + 7 + 7) / 8) * 16 : 0);
  int rc;
  if (dtype == MIO_FP32) rc = sp_launch<float, false>(a, B, smem, st);
  else if (dtype == MIO_BF16) rc = res ? sp_launch<__bf16, true>(a, B, smem, st) : sp_launch<__bf16, false>(a, B, smem, st);
  else rc = res ? sp_launch<_Float16, true>(a, B, smem, st) : sp_launch<_Float16, false>(a, B, smem, st);
  if (rc != 0) return rc;
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mio_fail(fn + " launch: " + hipGetErrorString(e));
  return 0;
}

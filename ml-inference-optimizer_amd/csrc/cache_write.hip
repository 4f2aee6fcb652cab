// Writes into the paged KV cache for CDNA4 (gfx950), and rotary position embedding.  The unit holds
//   cache_write_kernel            mio_reshape_and_cache(_kv8): the one new token of every sequence
//   cache_write_varlen_kernel     mio_reshape_and_cache_varlen(_kv8): packed new tokens, many per sequence
//   rope_and_cache_varlen_kernel  mio_rope_and_cache_varlen(_kv8): the varlen write with the rotation of q and k fused in
//   rope_rows_kernel              mio_rope_rows: the rotation alone (the dense path); here because it shares rope_row16
// and one host plan (cw_plan) and launcher (cw_launch) for the six writes: an entry point fills a CwCall and names its form.
// Cache layout [num_blocks, num_layers, block_size, Hkv, D], 16-bit elements of the source's dtype or (KV8) one e4m3fn byte
// each: e4m3(clamp(x * (1 / scale), -448, 448)), kv8_cvt.h.  Bandwidth-bound: 16-byte global loads and stores only, registers
// only (no LDS, no scratch).
//
// Rotation: the first rot elements of a head are rotated by the angle of (position, pair): y1 = x1 c - x2 s, y2 = x2 c + x1 s
// in fp32, c / s read from the caller's fp32 tables [max_position, rot / 2] (never computed here), rounded once to the stored
// format.  Pairing: neox (IL false) pairs element i with i + rot / 2, interleaved (IL true, GPT-J) pairs 2 i with 2 i + 1.
//
// Thread mapping of the rotating kernels: a head row is cut into units of E elements -- E = 8 (one 16-byte chunk of 16 bits)
// or, for the K / V rows of an fp8 cache, E = 16 (one 16-byte chunk of e4m3; two chunks of the 16-bit source).  A rotated unit
// of the neox pairing is a chunk AND its partner chunk rot / 2 further on, so a thread holds both halves of every pair it
// writes; of the interleaved pairing it is one chunk (pairs are neighbours).  Units past rot copy.  Consecutive threads take
// consecutive units, heads and tokens, so a wave reads and writes whole rows of a token at 16 bytes per lane.
#include "mio_common.h"

#include "kv8_cvt.h"

// what the rotating kernel reads (the plain kernels take the fields they read as scalars); filled by cw_plan
struct CwDev {
  const void* q;   // [total, H, D] by (token, head) strides; may be qo
  void* qo;
  const void* k;   // [total, Hkv, D]
  const void* v;
  void* kc;        // [num_blocks, L, bs, Hkv, D]
  void* vc;
  const float* ksc;  // fp8 cache: the layer's scales
  const float* vsc;
  const float* cos;  // [maxpos, rot / 2]
  const float* sin;
  const int32_t* bt;
  const int32_t* cu;
  const int32_t* cl;
  const int32_t* positions;  // null: the cache position
  int64_t qs_t, qs_h, os_t, os_h, ks_t, ks_h, vs_t, vs_h;
  int B, total, H, Hkv, D, rot, maxpos, num_blocks, L, layer, bs, max_blocks;
};

// ---- the cache row of a packed token ---------------------------------------------------------------------------------------
// The cache row of packed token t of a varlen write (cache_write_varlen_kernel, rope_and_cache_varlen_kernel): write(row) when
// the token is written.  Its sequence is the last b with cu[b] <= t (binary search over the clamped offsets, then checked: a
// token outside its sequence's clamped range is skipped, so offsets that disagree with total write nothing out of place); a
// position before the sequence, past its block-table row or in a block outside the cache is skipped too.  The two halves are
// usable apart: cw_tok (the sequence and the cache position, false for a token outside its sequence's range) and cw_row_at
// (the row of a position); cw_row is one after the other.
__device__ __forceinline__ bool cw_tok(int t, const int32_t* cu, const int32_t* cl, int B, int total, int& b, int& pos) {
  auto cu_at = [&](int b) { const int x = cu[b]; return x < 0 ? 0 : (x > total ? total : x); };
  int lo = 0, hi = B;  // the sequence: last b in [0, B) with cu[b] <= t
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (cu_at(mid) <= t) lo = mid; else hi = mid;
  }
  const int s0 = cu_at(lo), s1e = cu_at(lo + 1), s1 = s1e > s0 ? s1e : s0;
  b = lo;
  if (t < s0 || t >= s1) return false;
  pos = cl[lo] - (s1 - s0) + (t - s0);
  return true;
}

template <typename F>
__device__ __forceinline__ void cw_row_at(int b, int pos, const int32_t* bt, int num_blocks, int L, int layer, int bs,
                                          int max_blocks, F&& write) {
  if (pos < 0 || pos / bs >= max_blocks) return;  // before the sequence / past its block-table row
  const int pb = bt[(int64_t)b * max_blocks + pos / bs];
  if (pb < 0 || pb >= num_blocks) return;
  write(((int64_t)pb * L + layer) * bs + pos % bs);
}

template <typename F>
__device__ __forceinline__ void cw_row(int t, const int32_t* bt, const int32_t* cu, const int32_t* cl, int B, int total,
                                       int num_blocks, int L, int layer, int bs, int max_blocks, F&& write) {
  int b, pos;
  if (!cw_tok(t, cu, cl, B, total, b, pos)) return;
  cw_row_at(b, pos, bt, num_blocks, L, layer, bs, max_blocks, write);
}

// ---- one 16-byte chunk of the cache ----------------------------------------------------------------------------------------
// T: the 16-bit source type; a 16-bit cache only moves bits, so its plain kernels are instantiated once, over uint16_t.
// 1 / scale of an fp8 cache (1 for a 16-bit one, which has no scale to read)
template <bool KV8>
__device__ __forceinline__ float cw_inv(const float* scale) {
  if constexpr (KV8) return 1.0f / scale[0];
  else return 1.f;
}

// The chunk store every write shares: one chunk of a cached K or V row from its 16-bit source.  16-bit cache: one 16-byte load
// and one 16-byte store of 8 elements; fp8 cache: two loads (16 elements), kv8_quant16 and one store.
template <typename T, bool KV8>
__device__ __forceinline__ void cw_store(void* dst, const T* src, float inv) {
  if constexpr (KV8) *(u32x4_t*)dst = kv8_quant16<T>(*(const u32x4_t*)src, *(const u32x4_t*)(src + 8), inv);
  else *(u32x4_t*)dst = *(const u32x4_t*)src;
}

// ---- plain writes ------------------------------------------------------------------------------------------------------
// cache_write_kernel: one workgroup per sequence, the token at context_lengths[b] - 1 (attention_kernels.py:858); the
// workgroup's threads stride over the 16-byte chunks of the cached (Hkv, D) row.
template <typename T, bool KV8>
__global__ __launch_bounds__(256) void cache_write_kernel(
    const T* __restrict__ key, const T* __restrict__ value, uint8_t* __restrict__ kc, uint8_t* __restrict__ vc,
    const float* __restrict__ ksc, const float* __restrict__ vsc, const int32_t* __restrict__ bt,
    const int32_t* __restrict__ cl, int64_t ks_b, int64_t ks_h, int64_t vs_b, int64_t vs_h, int Hkv, int D, int L, int layer,
    int bs, int max_blocks) {
  constexpr int E = KV8 ? 16 : 8;  // elements per chunk
  using C = std::conditional_t<KV8, uint8_t, T>;  // a cached element
  const int b = blockIdx.x;
  const int pos = cl[b] - 1;
  if (pos < 0 || pos / bs >= max_blocks) return;  // empty sequence / context longer than the block table row: nothing written
  const int pb = bt[(int64_t)b * max_blocks + pos / bs];
  const float kinv = cw_inv<KV8>(ksc), vinv = cw_inv<KV8>(vsc);  // once, before the loop
  const int64_t tok_stride = (int64_t)Hkv * D;
  const int64_t dst = ((int64_t)pb * L + layer) * bs * tok_stride + (int64_t)(pos % bs) * tok_stride;
  const int cpr = D >> (KV8 ? 4 : 3);
  for (int i = threadIdx.x; i < Hkv * cpr; i += 256) {
    const int hh = i / cpr, c = i % cpr;
    cw_store<T, KV8>((C*)kc + dst + (int64_t)hh * D + E * c, key + b * ks_b + hh * ks_h + E * c, kinv);
    cw_store<T, KV8>((C*)vc + dst + (int64_t)hh * D + E * c, value + b * vs_b + hh * vs_h + E * c, vinv);
  }
}

// cache_write_varlen_kernel: many new tokens per sequence, one thread per 16-byte chunk of the cached K and V rows.  Thread i
// of the grid owns chunk i % (Hkv * D / E) of packed token i / (Hkv * D / E); the token's cache row and the skipping rules are
// cw_row's.  The scales are read inside the row callback: a skipped token reads none.
template <typename T, bool KV8>
__global__ __launch_bounds__(256) void cache_write_varlen_kernel(
    const T* __restrict__ key, const T* __restrict__ value, uint8_t* __restrict__ kc, uint8_t* __restrict__ vc,
    const float* __restrict__ ksc, const float* __restrict__ vsc, const int32_t* __restrict__ bt,
    const int32_t* __restrict__ cu, const int32_t* __restrict__ cl, int64_t ks_t, int64_t ks_h, int64_t vs_t, int64_t vs_h,
    int B, int total, int Hkv, int D, int num_blocks, int L, int layer, int bs, int max_blocks) {
  constexpr int E = KV8 ? 16 : 8;
  using C = std::conditional_t<KV8, uint8_t, T>;
  const int cpr = D >> (KV8 ? 4 : 3), cpt = Hkv * cpr;  // 16-byte chunks per head row / per token
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)total * cpt) return;
  const int t = (int)(i / cpt), c = (int)(i % cpt), hh = c / cpr, cc = c % cpr;
  cw_row(t, bt, cu, cl, B, total, num_blocks, L, layer, bs, max_blocks, [&](int64_t row) __attribute__((always_inline)) {
    const int64_t dst = row * ((int64_t)Hkv * D) + (int64_t)hh * D + E * cc;
    cw_store<T, KV8>((C*)kc + dst, key + t * ks_t + hh * ks_h + E * cc, cw_inv<KV8>(ksc));
    cw_store<T, KV8>((C*)vc + dst, value + t * vs_t + hh * vs_h + E * cc, cw_inv<KV8>(vsc));
  });
}

// ---- rotation ------------------------------------------------------------------------------------------------------------
// E 16-bit elements (E / 8 16-byte loads) as fp32
template <typename T, int E>
__device__ __forceinline__ void rope_ld(const T* p, float* f) {
#pragma unroll
  for (int j = 0; j < E / 8; ++j) {
    const typename DT<T>::x8 x = __builtin_bit_cast(typename DT<T>::x8, *(const u32x4_t*)(p + 8 * j));
#pragma unroll
    for (int i = 0; i < 8; ++i) f[8 * j + i] = (float)x[i];
  }
}

// E fp32 -> E 16-bit elements (round to nearest even), 16-byte stores
template <typename T, int E>
__device__ __forceinline__ void rope_st(T* p, const float* f) {
#pragma unroll
  for (int j = 0; j < E / 8; ++j)
    *(u32x4_t*)(p + 8 * j) = (u32x4_t){pack2<T>(f[8 * j], f[8 * j + 1]), pack2<T>(f[8 * j + 2], f[8 * j + 3]),
                                       pack2<T>(f[8 * j + 4], f[8 * j + 5]), pack2<T>(f[8 * j + 6], f[8 * j + 7])};
}

// 16 fp32 -> one 16-byte chunk of e4m3(clamp(f * inv)): one rounding from fp32; a NaN stays NaN (as kv8_quant16)
__device__ __forceinline__ void rope_st8(uint8_t* p, float* f, float inv) {
#pragma unroll
  for (int i = 0; i < 16; ++i) f[i] = __builtin_isnan(f[i]) ? f[i] : kv8_clamp(f[i] * inv);
  *(u32x4_t*)p = (u32x4_t){kv8_pack4(f), kv8_pack4(f + 4), kv8_pack4(f + 8), kv8_pack4(f + 12)};
}

// E 16-bit elements copied as they are
template <typename T, int E>
__device__ __forceinline__ void rope_copy(T* dst, const T* src) {
  u32x4_t r[E / 8];
#pragma unroll
  for (int j = 0; j < E / 8; ++j) r[j] = *(const u32x4_t*)(src + 8 * j);
#pragma unroll
  for (int j = 0; j < E / 8; ++j) *(u32x4_t*)(dst + 8 * j) = r[j];
}

template <typename T, int E>
__device__ __forceinline__ void rope_zero(T* dst) {
#pragma unroll
  for (int j = 0; j < E / 8; ++j) *(u32x4_t*)(dst + 8 * j) = (u32x4_t){0u, 0u, 0u, 0u};
}

// N consecutive fp32 table entries (16-byte loads)
template <int N>
__device__ __forceinline__ void rope_tab(const float* p, float* f) {
#pragma unroll
  for (int j = 0; j < N / 4; ++j) {
    const f32x4_t x = *(const f32x4_t*)(p + 4 * j);
    f[4 * j] = x[0];
    f[4 * j + 1] = x[1];
    f[4 * j + 2] = x[2];
    f[4 * j + 3] = x[3];
  }
}

// The rotated unit at element e0 of the head row src at table row (cos, sin: the position's rot / 2 entries): a (and, neox, its
// partner b) in fp32.  neox: a = elements e0 .. e0 + E, b = those half further on, pair i uses entry e0 + i.  Interleaved:
// a = elements e0 .. e0 + E, pair i = (a[2 i], a[2 i + 1]) uses entry e0 / 2 + i.
template <typename T, int E, bool IL>
__device__ __forceinline__ void rope_unit(const T* src, const float* cos, const float* sin, int e0, int half, float* a, float* b) {
  rope_ld<T, E>(src + e0, a);
  if constexpr (IL) {
    float c[E / 2], s[E / 2];
    rope_tab<E / 2>(cos + e0 / 2, c);
    rope_tab<E / 2>(sin + e0 / 2, s);
#pragma unroll
    for (int i = 0; i < E / 2; ++i) {
      const float x1 = a[2 * i], x2 = a[2 * i + 1];
      a[2 * i] = x1 * c[i] - x2 * s[i];
      a[2 * i + 1] = x2 * c[i] + x1 * s[i];
    }
  } else {
    rope_ld<T, E>(src + e0 + half, b);
    float c[E], s[E];
    rope_tab<E>(cos + e0, c);
    rope_tab<E>(sin + e0, s);
#pragma unroll
    for (int i = 0; i < E; ++i) {
      const float x1 = a[i], x2 = b[i];
      a[i] = x1 * c[i] - x2 * s[i];
      b[i] = x2 * c[i] + x1 * s[i];
    }
  }
}

// units of a head row: nrot rotated ones, then the copied ones; e0: the unit's first element
template <int E, bool IL>
__device__ __forceinline__ void rope_units(int D, int rot, int& nrot, int& upr) {
  nrot = IL ? rot / E : rot / (2 * E);
  upr = nrot + (D - rot) / E;
}

// One rotated / copied / zeroed unit of a 16-bit row into dst (the Q rows of the fused write, every row of rope_rows).
// live false: the row is written as zeros.
template <typename T, int E, bool IL>
__device__ __forceinline__ void rope_row16(const T* src, T* dst, const float* cos, const float* sin, int64_t tab, int u,
                                           int nrot, int rot, bool live) {
  const int half = rot >> 1;
  const bool rotu = u < nrot;
  const int e0 = rotu ? u * E : rot + (u - nrot) * E;
  if (!live) {
    rope_zero<T, E>(dst + e0);
    if (!IL && rotu) rope_zero<T, E>(dst + e0 + half);
    return;
  }
  if (!rotu) {
    rope_copy<T, E>(dst + e0, src + e0);
    return;
  }
  float a[E], b[E];
  rope_unit<T, E, IL>(src, cos + tab, sin + tab, e0, half, a, b);  // both chunks are read before either is written: dst may be src
  rope_st<T, E>(dst + e0, a);
  if constexpr (!IL) rope_st<T, E>(dst + e0 + half, b);
}

// E fp32 of a rotated unit -> its chunk of the cache: E = 8 16-bit elements, or (KV8) E = 16 e4m3
template <typename T, bool KV8>
__device__ __forceinline__ void rope_st_cache(uint8_t* p, float* f, float inv) {
  if constexpr (KV8) rope_st8(p, f, inv);
  else rope_st<T, 8>((T*)p, f);
}

// ---- rope_and_cache_varlen: a packed token is H uq + Hkv uk threads, uq units of 8 elements per Q head row first (rotated
// into qo), then uk units per K head row (8 elements, or 16 for an fp8 cache; rotated into the cache) together with the same
// chunks of the V head of the same index.  V and the units of K past rot go through cw_store, exactly as
// cache_write_varlen_kernel writes them; the token's sequence, cache position and row are cw_tok / cw_row_at's (= cw_row's).
template <typename T, bool KV8, bool IL>
__global__ __launch_bounds__(256) void rope_and_cache_varlen_kernel(const CwDev p) {
  constexpr int E = KV8 ? 16 : 8, ESZ = KV8 ? 1 : 2;
  int nrot_q, uq, nrot, uk;
  rope_units<8, IL>(p.D, p.rot, nrot_q, uq);
  rope_units<E, IL>(p.D, p.rot, nrot, uk);
  const int q_n = p.H * uq, upt = q_n + p.Hkv * uk;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)p.total * upt) return;
  const int t = (int)(i / upt), r = (int)(i % upt);
  const float kinv = cw_inv<KV8>(p.ksc), vinv = cw_inv<KV8>(p.vsc);  // read ahead of the token lookup's dependent loads
  int b, pos = 0;
  const bool in_seq = cw_tok(t, p.cu, p.cl, p.B, p.total, b, pos);
  const int rpos = p.positions ? p.positions[t] : pos;  // the rotation's position; the cache row stays pos's
  const bool live = in_seq && rpos >= 0 && rpos < p.maxpos;
  const int half = p.rot >> 1;
  const int64_t tab = live ? (int64_t)rpos * half : 0;
  if (r < q_n) {
    const int hs = r / uq, u = r % uq;
    rope_row16<T, 8, IL>((const T*)p.q + t * p.qs_t + hs * p.qs_h, (T*)p.qo + t * p.os_t + hs * p.os_h, p.cos, p.sin, tab, u,
                         nrot_q, p.rot, live);
    return;
  }
  if (!live) return;
  const int hh = (r - q_n) / uk, u = (r - q_n) % uk;
  cw_row_at(b, pos, p.bt, p.num_blocks, p.L, p.layer, p.bs, p.max_blocks, [&](int64_t row) __attribute__((always_inline)) {
    const bool rotu = u < nrot;
    const int e0 = rotu ? u * E : p.rot + (u - nrot) * E;
    const int64_t dst = (row * ((int64_t)p.Hkv * p.D) + (int64_t)hh * p.D + e0) * ESZ;
    uint8_t* kc = (uint8_t*)p.kc + dst;
    uint8_t* vc = (uint8_t*)p.vc + dst;
    const T* kp = (const T*)p.k + t * p.ks_t + hh * p.ks_h;
    const T* vp = (const T*)p.v + t * p.vs_t + hh * p.vs_h + e0;
    cw_store<T, KV8>(vc, vp, vinv);
    if (!IL && rotu) cw_store<T, KV8>(vc + half * ESZ, vp + half, vinv);  // the partner chunk as well
    if (!rotu) {
      cw_store<T, KV8>(kc, kp + e0, kinv);
      return;
    }
    float a[E], bb[E];
    rope_unit<T, E, IL>(kp, p.cos + tab, p.sin + tab, e0, half, a, bb);
    rope_st_cache<T, KV8>(kc, a, kinv);
    if constexpr (!IL) rope_st_cache<T, KV8>(kc + half * ESZ, bb, kinv);
  });
}

// ---- rope_rows: x [tokens, heads, D] by (token, head) strides rotated into out (which may be x) at positions[token]; a
// position outside [0, maxpos) writes the row as zeros.  Thread i owns unit i % upr of head (i / upr) % heads.
template <typename T, bool IL>
__global__ __launch_bounds__(256) void rope_rows_kernel(const T* x, T* out, const int32_t* __restrict__ positions,
                                                        const float* __restrict__ cos, const float* __restrict__ sin,
                                                        int64_t xs_t, int64_t xs_h, int64_t os_t, int64_t os_h, int tokens,
                                                        int heads, int D, int rot, int maxpos) {
  int nrot, upr;
  rope_units<8, IL>(D, rot, nrot, upr);
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)tokens * heads * upr) return;
  const int t = (int)(i / ((int64_t)heads * upr)), r = (int)(i % ((int64_t)heads * upr)), h = r / upr, u = r % upr;
  const int rpos = positions[t];
  const bool live = rpos >= 0 && rpos < maxpos;
  rope_row16<T, 8, IL>(x + t * xs_t + h * xs_h, out + t * os_t + h * os_h, cos, sin, live ? (int64_t)rpos * (rot >> 1) : 0, u,
                       nrot, rot, live);
}

// ---- host ----------------------------------------------------------------------------------------------------------------
static bool rope_strides_ok(const int64_t* s) { return s[0] >= 0 && s[1] >= 0 && s[0] % 8 == 0 && s[1] % 8 == 0; }

// the checks of the rotation itself, shared by the rotating writes (through cw_plan) and mio_rope_rows
static int rope_check_rot(const std::string& fn, bool kv8, const float* cos, const float* sin, int32_t D, int32_t rot_dim,
                          int32_t max_position, int32_t interleaved, int32_t dtype) {
  if (kv8) MIO_CHECK(D >= 16 && D <= 128 && D % 16 == 0, fn + ": head_dim must be a multiple of 16 in [16,128] for an fp8 cache");
  else MIO_CHECK(D >= 8 && D <= 128 && D % 8 == 0, fn + ": head_dim must be a multiple of 8 in [8,128]");
  MIO_CHECK(rot_dim > 0 && rot_dim % 16 == 0 && rot_dim <= D, fn + ": rot_dim must be a multiple of 16 in [16, head_dim]");
  MIO_CHECK(interleaved == 0 || interleaved == 1, fn + ": interleaved must be 0 (neox pairing) or 1");
  MIO_CHECK(!kv8 || interleaved || rot_dim % 32 == 0,
            fn + ": rot_dim must be a multiple of 32 for an fp8 cache with the neox pairing");
  MIO_CHECK(max_position > 0, fn + ": max_position must be positive");
  MIO_CHECK(dtype == MIO_BF16 || dtype == MIO_FP16, fn + ": dtype must be bf16 or fp16");
  MIO_CHECK(cos && sin, fn + ": null cos / sin table");
  MIO_CHECK(mio_aligned16(cos) && mio_aligned16(sin), fn + ": 16-byte alignment (cos / sin tables)");
  return 0;
}

// What distinguishes a write's entry point.  name prefixes its refusals, launch its launch failure.
struct CwForm {
  const char *name, *launch;
  bool varlen;  // packed new tokens by cu_seqlens_new (and a num_blocks to check block ids against); else one token per sequence
  bool kv8;     // fp8 (e4m3fn) cache with k_scale / v_scale; else a 16-bit cache of the source's dtype
  bool rope;    // rotates q and k (varlen only)
};

// An entry point's arguments under the names of include/mio_hip.h; what a form does not take stays zero.
struct CwCall {
  const void *q = nullptr, *key = nullptr, *value = nullptr;
  void *q_out = nullptr, *k_cache = nullptr, *v_cache = nullptr;
  const float *k_scale = nullptr, *v_scale = nullptr, *cos = nullptr, *sin = nullptr;
  const int32_t *block_tables = nullptr, *cu_seqlens_new = nullptr, *context_lengths = nullptr, *positions = nullptr;
  const int64_t *q_stride = nullptr, *q_out_stride = nullptr, *k_stride = nullptr, *v_stride = nullptr;
  int32_t B = 0, total_new = 0, H = 0, Hkv = 0, D = 0, rot_dim = 0, max_position = 0, interleaved = 0, num_blocks = 0,
          num_layers = 0, layer_idx = 0, block_size = 0, max_blocks_per_seq = 0, dtype = 0;
};

// the arguments every form takes (mio_reshape_and_cache's), then those of the varlen forms
static CwCall cw_call(const void* key, const void* value, void* k_cache, void* v_cache, const int32_t* block_tables,
                      const int32_t* context_lengths, const int64_t* k_stride, const int64_t* v_stride, int32_t B, int32_t Hkv,
                      int32_t D, int32_t num_layers, int32_t layer_idx, int32_t block_size, int32_t max_blocks_per_seq,
                      int32_t dtype, const int32_t* cu_seqlens_new = nullptr, int32_t total_new = 0, int32_t num_blocks = 0) {
  CwCall c;
  c.cu_seqlens_new = cu_seqlens_new, c.total_new = total_new, c.num_blocks = num_blocks;
  c.key = key, c.value = value, c.k_cache = k_cache, c.v_cache = v_cache;
  c.block_tables = block_tables, c.context_lengths = context_lengths, c.k_stride = k_stride, c.v_stride = v_stride;
  c.B = B, c.Hkv = Hkv, c.D = D, c.num_layers = num_layers, c.layer_idx = layer_idx, c.block_size = block_size;
  c.max_blocks_per_seq = max_blocks_per_seq, c.dtype = dtype;
  return c;
}

// The plan of a write: every check of the form, once, then the device arguments and the grid (blocks; 0: nothing to launch,
// which only a varlen form without sequences or tokens returns).  The forms' accept sets differ where they did before they
// shared this plan; each difference is a condition on the form here, not a second copy of a check:
//   a single-token form needs B > 0 and looks at every pointer first; a varlen form with no work returns before it looks at
//   its data pointers, strides' values, alignment or grid, and refuses negative strides, which a single-token form takes;
//   the plain 16-bit forms fold head_dim into "bad sizes" and, like the plain fp8 forms, do not bound it from above;
//   mio_reshape_and_cache takes any max_blocks_per_seq (its kernel writes nothing when it is <= 0).
static int cw_plan(const CwForm& f, const CwCall& c, CwDev& p, int64_t& blocks) {
  const std::string fn = f.name;
  blocks = 0;
  const bool data = c.key && c.value && c.k_cache && c.v_cache && c.block_tables && c.context_lengths &&
                    (!f.varlen || c.cu_seqlens_new) && (!f.rope || (c.q && c.q_out));
  const bool strides = c.k_stride && c.v_stride && (!f.rope || (c.q_stride && c.q_out_stride));
  if (f.varlen) MIO_CHECK(strides, fn + ": null strides");
  else MIO_CHECK(data && strides, fn + ": null pointer");
  if (f.kv8)
    MIO_CHECK(c.k_scale && c.v_scale && ((uintptr_t)c.k_scale & 3) == 0 && ((uintptr_t)c.v_scale & 3) == 0,
              fn + ": k_scale and v_scale are required with an fp8 cache (null scale pointer or not 4-byte aligned)");
  MIO_CHECK((f.varlen ? c.B >= 0 && c.total_new >= 0 : c.B > 0) && c.Hkv > 0 && (!f.rope || (c.H > 0 && c.H % c.Hkv == 0)) &&
                (f.kv8 || f.rope || (c.D >= 8 && c.D % 8 == 0)),
            fn + ": bad sizes");
  if (f.kv8 && !f.rope) MIO_CHECK(c.D >= 16 && c.D % 16 == 0, fn + ": head_dim must be a multiple of 16 for an fp8 cache");
  MIO_CHECK(c.layer_idx >= 0 && c.layer_idx < c.num_layers && c.block_size > 0 && (!f.varlen || c.num_blocks > 0) &&
                (c.max_blocks_per_seq > 0 || !(f.varlen || f.kv8)),
            fn + ": bad cache geometry");
  if (f.rope) {
    if (rope_check_rot(fn, f.kv8, c.cos, c.sin, c.D, c.rot_dim, c.max_position, c.interleaved, c.dtype) != 0) return -1;
  } else {
    MIO_CHECK(c.dtype == MIO_BF16 || c.dtype == MIO_FP16,
              fn + (f.kv8 ? ": dtype (of key and value) must be bf16 or fp16" : ": dtype must be bf16 or fp16"));
  }
  if (f.varlen) {
    if (c.B == 0 || c.total_new == 0) return 0;
    MIO_CHECK(data, fn + ": null pointer");
  }
  const auto rows16 = [&](const int64_t* s) { return f.varlen ? rope_strides_ok(s) : s[0] % 8 == 0 && s[1] % 8 == 0; };
  MIO_CHECK(rows16(c.k_stride) && rows16(c.v_stride) && mio_aligned16(c.key) && mio_aligned16(c.value) &&
                mio_aligned16(c.k_cache) && mio_aligned16(c.v_cache) &&
                (!f.rope || (rows16(c.q_stride) && rows16(c.q_out_stride) && mio_aligned16(c.q) && mio_aligned16(c.q_out) &&
                             ((uintptr_t)c.positions & 3) == 0)),
            fn + ": 16-byte alignment");
  p = {c.q, c.q_out, c.key, c.value, c.k_cache, c.v_cache, c.k_scale, c.v_scale, c.cos, c.sin, c.block_tables, c.cu_seqlens_new,
       c.context_lengths, c.positions, 0, 0, 0, 0, c.k_stride[0], c.k_stride[1], c.v_stride[0], c.v_stride[1], c.B, c.total_new,
       c.H, c.Hkv, c.D, c.rot_dim, c.max_position, c.num_blocks, c.num_layers, c.layer_idx, c.block_size, c.max_blocks_per_seq};
  if (f.rope) {
    p.qs_t = c.q_stride[0], p.qs_h = c.q_stride[1];
    p.os_t = c.q_out_stride[0], p.os_h = c.q_out_stride[1];
  }
  if (!f.varlen) {
    blocks = c.B;  // one workgroup per sequence
    return 0;
  }
  // one thread per unit: uq of 8 elements per Q head row, uk of E per K / V head row (a plain write: H = 0, rot_dim = 0)
  const int E = f.kv8 ? 16 : 8;
  const int uq = (c.interleaved ? c.rot_dim / 8 : c.rot_dim / 16) + (c.D - c.rot_dim) / 8;
  const int uk = (c.interleaved ? c.rot_dim / E : c.rot_dim / (2 * E)) + (c.D - c.rot_dim) / E;
  blocks = ((int64_t)c.total_new * ((int64_t)c.H * uq + (int64_t)c.Hkv * uk) + 255) / 256;
  MIO_CHECK(blocks <= 0x7fffffff, fn + ": too many tokens");
  return 0;
}

// the launch of a planned write: the kernel of the form, of the source dtype and (rotating) of the pairing
static int cw_launch(const CwForm& f, const CwDev& p, int64_t blocks, int32_t dtype, int32_t interleaved, void* stream) {
  const dim3 grid((unsigned)blocks), wg(256);
  hipStream_t st = (hipStream_t)stream;
#define CW_ONE(T, KV8)                                                                                                        \
  hipLaunchKernelGGL((cache_write_kernel<T, KV8>), grid, wg, 0, st, (const T*)p.k, (const T*)p.v, (uint8_t*)p.kc,            \
                     (uint8_t*)p.vc, p.ksc, p.vsc, p.bt, p.cl, p.ks_t, p.ks_h, p.vs_t, p.vs_h, p.Hkv, p.D, p.L, p.layer, p.bs, \
                     p.max_blocks)
#define CW_VARLEN(T, KV8)                                                                                                      \
  hipLaunchKernelGGL((cache_write_varlen_kernel<T, KV8>), grid, wg, 0, st, (const T*)p.k, (const T*)p.v, (uint8_t*)p.kc,      \
                     (uint8_t*)p.vc, p.ksc, p.vsc, p.bt, p.cu, p.cl, p.ks_t, p.ks_h, p.vs_t, p.vs_h, p.B, p.total, p.Hkv, p.D, \
                     p.num_blocks, p.L, p.layer, p.bs, p.max_blocks)
#define CW_ROPE(T, KV8)                                                                                \
  do {                                                                                                 \
    if (interleaved) hipLaunchKernelGGL((rope_and_cache_varlen_kernel<T, KV8, true>), grid, wg, 0, st, p); \
    else hipLaunchKernelGGL((rope_and_cache_varlen_kernel<T, KV8, false>), grid, wg, 0, st, p);        \
  } while (0)
#define CW_DTYPE(KERN, KV8)                      \
  do {                                           \
    if (dtype == MIO_BF16) KERN(__bf16, KV8);    \
    else KERN(_Float16, KV8);                    \
  } while (0)
  if (f.rope) {
    if (f.kv8) CW_DTYPE(CW_ROPE, true);
    else CW_DTYPE(CW_ROPE, false);
  } else if (f.varlen) {
    if (f.kv8) CW_DTYPE(CW_VARLEN, true);
    else CW_VARLEN(uint16_t, false);  // a 16-bit cache copies bits: one instantiation for both dtypes
  } else {
    if (f.kv8) CW_DTYPE(CW_ONE, true);
    else CW_ONE(uint16_t, false);
  }
#undef CW_DTYPE
#undef CW_ROPE
#undef CW_VARLEN
#undef CW_ONE
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mio_fail(std::string(f.launch) + " launch: " + hipGetErrorString(e));
  return 0;
}

static int cw_run(const CwForm& f, const CwCall& c, void* stream) {
  CwDev p;
  int64_t blocks;
  const int rc = cw_plan(f, c, p, blocks);
  if (rc != 0 || blocks == 0) return rc;
  return cw_launch(f, p, blocks, c.dtype, c.interleaved, stream);
}

// name, launch-failure prefix, varlen, fp8 cache, rotating
static const CwForm CW_ONE_16 = {"mio_reshape_and_cache", "reshape_and_cache", false, false, false};
static const CwForm CW_ONE_KV8 = {"mio_reshape_and_cache_kv8", "reshape_and_cache_kv8", false, true, false};
static const CwForm CW_VARLEN_16 = {"mio_reshape_and_cache_varlen", "reshape_and_cache_varlen", true, false, false};
static const CwForm CW_VARLEN_KV8 = {"mio_reshape_and_cache_varlen_kv8", "reshape_and_cache_varlen_kv8", true, true, false};
static const CwForm CW_ROPE_16 = {"mio_rope_and_cache_varlen", "mio_rope_and_cache_varlen", true, false, true};
static const CwForm CW_ROPE_KV8 = {"mio_rope_and_cache_varlen_kv8", "mio_rope_and_cache_varlen_kv8", true, true, true};

extern "C" int mio_reshape_and_cache(const void* key, const void* value, void* k_cache, void* v_cache,
                                     const int32_t* block_tables, const int32_t* context_lengths,
                                     const int64_t k_stride[2], const int64_t v_stride[2], int32_t B, int32_t Hkv,
                                     int32_t D, int32_t num_layers, int32_t layer_idx, int32_t block_size,
                                     int32_t max_blocks_per_seq, int32_t dtype, void* stream) {
  return cw_run(CW_ONE_16, cw_call(key, value, k_cache, v_cache, block_tables, context_lengths, k_stride, v_stride, B, Hkv, D,
                                   num_layers, layer_idx, block_size, max_blocks_per_seq, dtype), stream);
}

extern "C" int mio_reshape_and_cache_kv8(const void* key, const void* value, void* k_cache, void* v_cache,
                                         const float* k_scale, const float* v_scale, const int32_t* block_tables,
                                         const int32_t* context_lengths, const int64_t k_stride[2],
                                         const int64_t v_stride[2], int32_t B, int32_t Hkv, int32_t D,
                                         int32_t num_layers, int32_t layer_idx, int32_t block_size,
                                         int32_t max_blocks_per_seq, int32_t dtype, void* stream) {
  CwCall c = cw_call(key, value, k_cache, v_cache, block_tables, context_lengths, k_stride, v_stride, B, Hkv, D, num_layers,
                     layer_idx, block_size, max_blocks_per_seq, dtype);
  c.k_scale = k_scale, c.v_scale = v_scale;
  return cw_run(CW_ONE_KV8, c, stream);
}

extern "C" int mio_reshape_and_cache_varlen(const void* key, const void* value, void* k_cache, void* v_cache,
                                            const int32_t* block_tables, const int32_t* cu_seqlens_new,
                                            const int32_t* context_lengths, const int64_t k_stride[2],
                                            const int64_t v_stride[2], int32_t B, int32_t total_new, int32_t Hkv,
                                            int32_t D, int32_t num_blocks, int32_t num_layers, int32_t layer_idx,
                                            int32_t block_size, int32_t max_blocks_per_seq, int32_t dtype,
                                            void* stream) {
  return cw_run(CW_VARLEN_16, cw_call(key, value, k_cache, v_cache, block_tables, context_lengths, k_stride, v_stride, B, Hkv, D,
                                      num_layers, layer_idx, block_size, max_blocks_per_seq, dtype, cu_seqlens_new, total_new,
                                      num_blocks), stream);
}

extern "C" int mio_reshape_and_cache_varlen_kv8(const void* key, const void* value, void* k_cache, void* v_cache,
                                                const float* k_scale, const float* v_scale,
                                                const int32_t* block_tables, const int32_t* cu_seqlens_new,
                                                const int32_t* context_lengths, const int64_t k_stride[2],
                                                const int64_t v_stride[2], int32_t B, int32_t total_new, int32_t Hkv,
                                                int32_t D, int32_t num_blocks, int32_t num_layers, int32_t layer_idx,
                                                int32_t block_size, int32_t max_blocks_per_seq, int32_t dtype,
                                                void* stream) {
  CwCall c = cw_call(key, value, k_cache, v_cache, block_tables, context_lengths, k_stride, v_stride, B, Hkv, D, num_layers,
                     layer_idx, block_size, max_blocks_per_seq, dtype, cu_seqlens_new, total_new, num_blocks);
  c.k_scale = k_scale, c.v_scale = v_scale;
  return cw_run(CW_VARLEN_KV8, c, stream);
}

// both rotating forms: the varlen arguments with q, the tables and the rotation's sizes (the scales null for a 16-bit cache)
static int rope_cache_run(const CwForm& f, const void* q, void* q_out, const void* key, const void* value, void* k_cache,
                          void* v_cache, const float* k_scale, const float* v_scale, const int32_t* block_tables,
                          const int32_t* cu_seqlens_new, const int32_t* context_lengths, const int32_t* positions,
                          const float* cos, const float* sin, const int64_t* q_stride, const int64_t* q_out_stride,
                          const int64_t* k_stride, const int64_t* v_stride, int32_t B, int32_t total_new, int32_t H,
                          int32_t Hkv, int32_t D, int32_t rot_dim, int32_t max_position, int32_t interleaved,
                          int32_t num_blocks, int32_t num_layers, int32_t layer_idx, int32_t block_size,
                          int32_t max_blocks_per_seq, int32_t dtype, void* stream) {
  CwCall c = cw_call(key, value, k_cache, v_cache, block_tables, context_lengths, k_stride, v_stride, B, Hkv, D, num_layers,
                     layer_idx, block_size, max_blocks_per_seq, dtype, cu_seqlens_new, total_new, num_blocks);
  c.q = q, c.q_out = q_out, c.k_scale = k_scale, c.v_scale = v_scale, c.positions = positions, c.cos = cos, c.sin = sin;
  c.q_stride = q_stride, c.q_out_stride = q_out_stride;
  c.H = H, c.rot_dim = rot_dim, c.max_position = max_position, c.interleaved = interleaved;
  return cw_run(f, c, stream);
}

extern "C" int mio_rope_and_cache_varlen(const void* q, void* q_out, const void* key, const void* value, void* k_cache,
                                         void* v_cache, const int32_t* block_tables, const int32_t* cu_seqlens_new,
                                         const int32_t* context_lengths, const int32_t* positions, const float* cos,
                                         const float* sin, const int64_t q_stride[2], const int64_t q_out_stride[2],
                                         const int64_t k_stride[2], const int64_t v_stride[2], int32_t B,
                                         int32_t total_new, int32_t H, int32_t Hkv, int32_t D, int32_t rot_dim,
                                         int32_t max_position, int32_t interleaved, int32_t num_blocks,
                                         int32_t num_layers, int32_t layer_idx, int32_t block_size,
                                         int32_t max_blocks_per_seq, int32_t dtype, void* stream) {
  return rope_cache_run(CW_ROPE_16, q, q_out, key, value, k_cache, v_cache, nullptr, nullptr, block_tables, cu_seqlens_new,
                        context_lengths, positions, cos, sin, q_stride, q_out_stride, k_stride, v_stride, B, total_new, H, Hkv,
                        D, rot_dim, max_position, interleaved, num_blocks, num_layers, layer_idx, block_size,
                        max_blocks_per_seq, dtype, stream);
}

extern "C" int mio_rope_and_cache_varlen_kv8(const void* q, void* q_out, const void* key, const void* value, void* k_cache,
                                             void* v_cache, const float* k_scale, const float* v_scale,
                                             const int32_t* block_tables, const int32_t* cu_seqlens_new,
                                             const int32_t* context_lengths, const int32_t* positions, const float* cos,
                                             const float* sin, const int64_t q_stride[2], const int64_t q_out_stride[2],
                                             const int64_t k_stride[2], const int64_t v_stride[2], int32_t B,
                                             int32_t total_new, int32_t H, int32_t Hkv, int32_t D, int32_t rot_dim,
                                             int32_t max_position, int32_t interleaved, int32_t num_blocks,
                                             int32_t num_layers, int32_t layer_idx, int32_t block_size,
                                             int32_t max_blocks_per_seq, int32_t dtype, void* stream) {
  return rope_cache_run(CW_ROPE_KV8, q, q_out, key, value, k_cache, v_cache, k_scale, v_scale, block_tables, cu_seqlens_new,
                        context_lengths, positions, cos, sin, q_stride, q_out_stride, k_stride, v_stride, B, total_new, H, Hkv,
                        D, rot_dim, max_position, interleaved, num_blocks, num_layers, layer_idx, block_size,
                        max_blocks_per_seq, dtype, stream);
}

extern "C" int mio_rope_rows(const void* x, void* out, const int32_t* positions, const float* cos, const float* sin,
                             const int64_t x_stride[2], const int64_t out_stride[2], int32_t tokens, int32_t heads,
                             int32_t D, int32_t rot_dim, int32_t max_position, int32_t interleaved, int32_t dtype,
                             void* stream) {
  const std::string fn = "mio_rope_rows";
  MIO_CHECK(x_stride && out_stride, fn + ": null strides");
  MIO_CHECK(tokens >= 0 && heads > 0, fn + ": bad sizes");
  if (rope_check_rot(fn, false, cos, sin, D, rot_dim, max_position, interleaved, dtype) != 0) return -1;
  if (tokens == 0) return 0;
  MIO_CHECK(x && out && positions, fn + ": null pointer");
  MIO_CHECK(rope_strides_ok(x_stride) && rope_strides_ok(out_stride) && mio_aligned16(x) && mio_aligned16(out) &&
                ((uintptr_t)positions & 3) == 0,
            fn + ": 16-byte alignment");
  const int upr = (interleaved ? rot_dim / 8 : rot_dim / 16) + (D - rot_dim) / 8;
  const int64_t blocks = ((int64_t)tokens * heads * upr + 255) / 256;
  MIO_CHECK(blocks <= 0x7fffffff, fn + ": too many tokens");
  const dim3 grid((unsigned)blocks), wg(256);
  hipStream_t st = (hipStream_t)stream;
#define ROPE_ROWS(T, IL)                                                                                                   \
  hipLaunchKernelGGL((rope_rows_kernel<T, IL>), grid, wg, 0, st, (const T*)x, (T*)out, positions, cos, sin, x_stride[0], \
                     x_stride[1], out_stride[0], out_stride[1], tokens, heads, D, rot_dim, max_position)
  if (dtype == MIO_BF16) {
    if (interleaved) ROPE_ROWS(__bf16, true);
    else ROPE_ROWS(__bf16, false);
  } else {
    if (interleaved) ROPE_ROWS(_Float16, true);
    else ROPE_ROWS(_Float16, false);
  }
#undef ROPE_ROWS
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mio_fail(fn + " launch: " + hipGetErrorString(e));
  return 0;
}

// Rotary position embedding for CDNA4 (gfx950): the rotation fused into the paged KV-cache write (rope_and_cache_varlen,
// 16-bit and fp8 caches) and the standalone form of the dense path (rope_rows).  Bandwidth-bound: 16-byte global loads and
// stores only, registers only (no LDS, no scratch).
//
// The first rot elements of a head are rotated by the angle of (position, pair): y1 = x1 c - x2 s, y2 = x2 c + x1 s in fp32,
// c / s read from the caller's fp32 tables [max_position, rot / 2] (never computed here), rounded once to the stored format.
// Pairing: neox (IL false) pairs element i with i + rot / 2, interleaved (IL true, GPT-J) pairs 2 i with 2 i + 1.
//
// Thread mapping: a head row is cut into units of E elements -- E = 8 (one 16-byte chunk of 16 bits) or, for the K / V rows of
// an fp8 cache, E = 16 (one 16-byte chunk of e4m3; two chunks of the 16-bit source).  A rotated unit of the neox pairing is a
// chunk AND its partner chunk rot / 2 further on, so a thread holds both halves of every pair it writes; of the interleaved
// pairing it is one chunk (pairs are neighbours).  Units past rot copy.  Consecutive threads take consecutive units, heads and
// tokens, so a wave reads and writes whole rows of a token at 16 bytes per lane.
#include "mio_common.h"

#include "decode_plan.h"

struct RopeDev {
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

// ---- rope_and_cache_varlen: a packed token is H uq + Hkv uk threads, uq units of 8 elements per Q head row first (rotated
// into qo), then uk units per K head row (8 elements, or 16 for an fp8 cache; rotated into the cache) together with the same
// chunks of the V head of the same index (copied / quantised as reshape_and_cache_varlen(_kv8) does).  The token's sequence,
// cache position and row are dec_varlen_tok / dec_varlen_row_at's (= dec_varlen_row's: decode_plan.h).
template <typename T, bool KV8, bool IL>
__global__ __launch_bounds__(256) void rope_and_cache_varlen_kernel(const RopeDev p) {
  constexpr int E = KV8 ? 16 : 8;
  int nrot_q, uq, nrot, uk;
  rope_units<8, IL>(p.D, p.rot, nrot_q, uq);
  rope_units<E, IL>(p.D, p.rot, nrot, uk);
  const int q_n = p.H * uq, upt = q_n + p.Hkv * uk;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)p.total * upt) return;
  const int t = (int)(i / upt), r = (int)(i % upt);
  [[maybe_unused]] float kinv = 1.f, vinv = 1.f;
  if constexpr (KV8) {  // read ahead of the token lookup's dependent loads
    kinv = 1.0f / p.ksc[0];
    vinv = 1.0f / p.vsc[0];
  }
  int b, pos = 0;
  const bool in_seq = dec_varlen_tok(t, p.cu, p.cl, p.B, p.total, b, pos);
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
  dec_varlen_row_at(b, pos, p.bt, p.num_blocks, p.L, p.layer, p.bs, p.max_blocks, [&](int64_t row) __attribute__((always_inline)) {
    const bool rotu = u < nrot;
    const int e0 = rotu ? u * E : p.rot + (u - nrot) * E;
    const bool two = !IL && rotu;  // the partner chunk as well
    const int64_t dst = row * ((int64_t)p.Hkv * p.D) + (int64_t)hh * p.D + e0;
    const T* kp = (const T*)p.k + t * p.ks_t + hh * p.ks_h;
    const T* vp = (const T*)p.v + t * p.vs_t + hh * p.vs_h + e0;
    if constexpr (KV8) {
      uint8_t* kc = (uint8_t*)p.kc + dst;
      uint8_t* vc = (uint8_t*)p.vc + dst;
      *(u32x4_t*)vc = kv8_quant16<T>(*(const u32x4_t*)vp, *(const u32x4_t*)(vp + 8), vinv);
      if (two) *(u32x4_t*)(vc + half) = kv8_quant16<T>(*(const u32x4_t*)(vp + half), *(const u32x4_t*)(vp + half + 8), vinv);
      if (!rotu) {
        *(u32x4_t*)kc = kv8_quant16<T>(*(const u32x4_t*)(kp + e0), *(const u32x4_t*)(kp + e0 + 8), kinv);
        return;
      }
      float a[E], bb[E];
      rope_unit<T, E, IL>(kp, p.cos + tab, p.sin + tab, e0, half, a, bb);
      rope_st8(kc, a, kinv);
      if constexpr (!IL) rope_st8(kc + half, bb, kinv);
    } else {
      T* kc = (T*)p.kc + dst;
      T* vc = (T*)p.vc + dst;
      rope_copy<T, E>(vc, vp);
      if (two) rope_copy<T, E>(vc + half, vp + half);
      if (!rotu) {
        rope_copy<T, E>(kc, kp + e0);
        return;
      }
      float a[E], bb[E];
      rope_unit<T, E, IL>(kp, p.cos + tab, p.sin + tab, e0, half, a, bb);
      rope_st<T, E>(kc, a);
      if constexpr (!IL) rope_st<T, E>(kc + half, bb);
    }
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

// the checks of the rotation itself, shared by the three entry points
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

template <bool KV8>
static int rope_cache_run(const char* name, const void* q, void* q_out, const void* key, const void* value, void* k_cache,
                          void* v_cache, const float* k_scale, const float* v_scale, const int32_t* block_tables,
                          const int32_t* cu_seqlens_new, const int32_t* context_lengths, const int32_t* positions,
                          const float* cos, const float* sin, const int64_t* q_stride, const int64_t* qo_stride,
                          const int64_t* k_stride, const int64_t* v_stride, int32_t B, int32_t total_new, int32_t H,
                          int32_t Hkv, int32_t D, int32_t rot_dim, int32_t max_position, int32_t interleaved,
                          int32_t num_blocks, int32_t num_layers, int32_t layer_idx, int32_t block_size,
                          int32_t max_blocks_per_seq, int32_t dtype, void* stream) {
  const std::string fn = name;
  MIO_CHECK(q_stride && qo_stride && k_stride && v_stride, fn + ": null strides");
  if (KV8)
    MIO_CHECK(k_scale && v_scale && ((uintptr_t)k_scale & 3) == 0 && ((uintptr_t)v_scale & 3) == 0,
              fn + ": k_scale and v_scale are required with an fp8 cache (null scale pointer or not 4-byte aligned)");
  MIO_CHECK(B >= 0 && total_new >= 0 && H > 0 && Hkv > 0 && H % Hkv == 0, fn + ": bad sizes");
  MIO_CHECK(num_blocks > 0 && num_layers > 0 && layer_idx >= 0 && layer_idx < num_layers && block_size > 0 &&
                max_blocks_per_seq > 0,
            fn + ": bad cache geometry");
  if (rope_check_rot(fn, KV8, cos, sin, D, rot_dim, max_position, interleaved, dtype) != 0) return -1;
  if (B == 0 || total_new == 0) return 0;
  MIO_CHECK(q && q_out && key && value && k_cache && v_cache && block_tables && cu_seqlens_new && context_lengths,
            fn + ": null pointer");
  MIO_CHECK(rope_strides_ok(q_stride) && rope_strides_ok(qo_stride) && rope_strides_ok(k_stride) && rope_strides_ok(v_stride) &&
                mio_aligned16(q) && mio_aligned16(q_out) && mio_aligned16(key) && mio_aligned16(value) &&
                mio_aligned16(k_cache) && mio_aligned16(v_cache) && ((uintptr_t)positions & 3) == 0,
            fn + ": 16-byte alignment");
  constexpr int E = KV8 ? 16 : 8;  // elements per unit of a K / V row; a Q row's units are 8 elements
  const int uq = (interleaved ? rot_dim / 8 : rot_dim / 16) + (D - rot_dim) / 8;
  const int uk = (interleaved ? rot_dim / E : rot_dim / (2 * E)) + (D - rot_dim) / E;
  const int64_t blocks = ((int64_t)total_new * ((int64_t)H * uq + (int64_t)Hkv * uk) + 255) / 256;
  MIO_CHECK(blocks <= 0x7fffffff, fn + ": too many tokens");
  const RopeDev p = {q, q_out, key, value, k_cache, v_cache, k_scale, v_scale, cos, sin, block_tables, cu_seqlens_new,
                     context_lengths, positions, q_stride[0], q_stride[1], qo_stride[0], qo_stride[1], k_stride[0],
                     k_stride[1], v_stride[0], v_stride[1], B, total_new, H, Hkv, D, rot_dim, max_position, num_blocks,
                     num_layers, layer_idx, block_size, max_blocks_per_seq};
  const dim3 grid((unsigned)blocks), wg(256);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == MIO_BF16) {
    if (interleaved) hipLaunchKernelGGL((rope_and_cache_varlen_kernel<__bf16, KV8, true>), grid, wg, 0, st, p);
    else hipLaunchKernelGGL((rope_and_cache_varlen_kernel<__bf16, KV8, false>), grid, wg, 0, st, p);
  } else {
    if (interleaved) hipLaunchKernelGGL((rope_and_cache_varlen_kernel<_Float16, KV8, true>), grid, wg, 0, st, p);
    else hipLaunchKernelGGL((rope_and_cache_varlen_kernel<_Float16, KV8, false>), grid, wg, 0, st, p);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mio_fail(fn + " launch: " + hipGetErrorString(e));
  return 0;
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
  return rope_cache_run<false>("mio_rope_and_cache_varlen", q, q_out, key, value, k_cache, v_cache, nullptr, nullptr,
                               block_tables, cu_seqlens_new, context_lengths, positions, cos, sin, q_stride, q_out_stride,
                               k_stride, v_stride, B, total_new, H, Hkv, D, rot_dim, max_position, interleaved, num_blocks,
                               num_layers, layer_idx, block_size, max_blocks_per_seq, dtype, stream);
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
  return rope_cache_run<true>("mio_rope_and_cache_varlen_kv8", q, q_out, key, value, k_cache, v_cache, k_scale, v_scale,
                              block_tables, cu_seqlens_new, context_lengths, positions, cos, sin, q_stride, q_out_stride,
                              k_stride, v_stride, B, total_new, H, Hkv, D, rot_dim, max_position, interleaved, num_blocks,
                              num_layers, layer_idx, block_size, max_blocks_per_seq, dtype, stream);
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

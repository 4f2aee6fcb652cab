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
//
// The device arguments (CwDev), the cache row of a packed token (cw_tok / cw_row_at / cw_row), the chunk store (cw_store), the
// rotation of a unit (rope_unit and its loads and stores) and the host plan (CwForm, CwCall, cw_plan, rope_check_rot) live in
// cache_write_common.h, which qknorm_rope.hip shares.
#include "cache_write_common.h"

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
// E 16-bit elements copied as they are
template <typename T, int E>
__device__ __forceinline__ void rope_copy(T* dst, const T* src) {
  u32x4_t r[E / 8];
#pragma unroll
  for (int j = 0; j < E / 8; ++j) r[j] = *(const u32x4_t*)(src + 8 * j);
#pragma unroll
  for (int j = 0; j < E / 8; ++j) *(u32x4_t*)(dst + 8 * j) = r[j];
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
  cw_call_rope(c, q, q_out, k_scale, v_scale, positions, cos, sin, q_stride, q_out_stride, H, rot_dim, max_position, interleaved);
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

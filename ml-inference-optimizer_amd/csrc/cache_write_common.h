// What the units that write into the paged KV cache share (cache_write.hip: the plain and the rotating writes; qknorm_rope.hip:
// the rotating writes with the per-head RMSNorm of q and k in front of the rotation): the device arguments, the cache row of a
// packed token, the one chunk store, the rotation of a unit, and the host plan with every check of a write's arguments.
#pragma once
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

// The rotation of a unit held in fp32: a = elements e0 .. e0 + E of a head row and (neox) b = those half a rotation further on,
// at table row (cos, sin: the position's rot / 2 entries).  neox: pair i = (a[i], b[i]) uses entry e0 + i.  Interleaved:
// pair i = (a[2 i], a[2 i + 1]) uses entry e0 / 2 + i, b is not touched.
template <int E, bool IL>
__device__ __forceinline__ void rope_rot(const float* cos, const float* sin, int e0, float* a, float* b) {
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

// The rotated unit at element e0 of the head row src: loaded (a and, neox, its partner b at e0 + half) and rotated by rope_rot.
template <typename T, int E, bool IL>
__device__ __forceinline__ void rope_unit(const T* src, const float* cos, const float* sin, int e0, int half, float* a, float* b) {
  rope_ld<T, E>(src + e0, a);
  if constexpr (!IL) rope_ld<T, E>(src + e0 + half, b);
  rope_rot<E, IL>(cos, sin, e0, a, b);
}

// units of a head row: nrot rotated ones, then the copied ones; e0: the unit's first element
template <int E, bool IL>
__device__ __forceinline__ void rope_units(int D, int rot, int& nrot, int& upr) {
  nrot = IL ? rot / E : rot / (2 * E);
  upr = nrot + (D - rot) / E;
}

// E fp32 of a rotated unit -> its chunk of the cache: E = 8 16-bit elements, or (KV8) E = 16 e4m3
template <typename T, bool KV8>
__device__ __forceinline__ void rope_st_cache(uint8_t* p, float* f, float inv) {
  if constexpr (KV8) rope_st8(p, f, inv);
  else rope_st<T, 8>((T*)p, f);
}

// ---- host ----------------------------------------------------------------------------------------------------------------
static inline bool rope_strides_ok(const int64_t* s) { return s[0] >= 0 && s[1] >= 0 && s[0] % 8 == 0 && s[1] % 8 == 0; }

// the checks of the rotation itself, shared by the rotating writes (through cw_plan) and the standalone forms
static inline int rope_check_rot(const std::string& fn, bool kv8, const float* cos, const float* sin, int32_t D, int32_t rot_dim,
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
static inline CwCall cw_call(const void* key, const void* value, void* k_cache, void* v_cache, const int32_t* block_tables,
                             const int32_t* context_lengths, const int64_t* k_stride, const int64_t* v_stride, int32_t B,
                             int32_t Hkv, int32_t D, int32_t num_layers, int32_t layer_idx, int32_t block_size,
                             int32_t max_blocks_per_seq, int32_t dtype, const int32_t* cu_seqlens_new = nullptr,
                             int32_t total_new = 0, int32_t num_blocks = 0) {
  CwCall c;
  c.cu_seqlens_new = cu_seqlens_new, c.total_new = total_new, c.num_blocks = num_blocks;
  c.key = key, c.value = value, c.k_cache = k_cache, c.v_cache = v_cache;
  c.block_tables = block_tables, c.context_lengths = context_lengths, c.k_stride = k_stride, c.v_stride = v_stride;
  c.B = B, c.Hkv = Hkv, c.D = D, c.num_layers = num_layers, c.layer_idx = layer_idx, c.block_size = block_size;
  c.max_blocks_per_seq = max_blocks_per_seq, c.dtype = dtype;
  return c;
}

// the rotating forms' further arguments on top of cw_call's: q, the tables and the rotation's sizes (scales null: 16-bit cache)
static inline void cw_call_rope(CwCall& c, const void* q, void* q_out, const float* k_scale, const float* v_scale,
                                const int32_t* positions, const float* cos, const float* sin, const int64_t* q_stride,
                                const int64_t* q_out_stride, int32_t H, int32_t rot_dim, int32_t max_position,
                                int32_t interleaved) {
  c.q = q, c.q_out = q_out, c.k_scale = k_scale, c.v_scale = v_scale, c.positions = positions, c.cos = cos, c.sin = sin;
  c.q_stride = q_stride, c.q_out_stride = q_out_stride;
  c.H = H, c.rot_dim = rot_dim, c.max_position = max_position, c.interleaved = interleaved;
}

// The plan of a write: every check of the form, once, then the device arguments and the grid (blocks; 0: nothing to launch,
// which only a varlen form without sequences or tokens returns).  The forms' accept sets differ where they did before they
// shared this plan; each difference is a condition on the form here, not a second copy of a check:
//   a single-token form needs B > 0 and looks at every pointer first; a varlen form with no work returns before it looks at
//   its data pointers, strides' values, alignment or grid, and refuses negative strides, which a single-token form takes;
//   the plain 16-bit forms fold head_dim into "bad sizes" and, like the plain fp8 forms, do not bound it from above;
//   mio_reshape_and_cache takes any max_blocks_per_seq (its kernel writes nothing when it is <= 0).
// The grid is that of cache_write.hip's kernels (one thread per unit); a unit with another thread mapping (qknorm_rope.hip)
// takes blocks > 0 as "there is work" and sizes its own.
static inline int cw_plan(const CwForm& f, const CwCall& c, CwDev& p, int64_t& blocks) {
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

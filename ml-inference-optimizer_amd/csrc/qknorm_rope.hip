// QK-norm for CDNA4 (gfx950): the per-head RMSNorm of q and k (Qwen3, Gemma 3) fused in front of the rotary position embedding,
// on the way into q_out and the paged KV cache.  The unit holds
//   qknorm_rope_and_cache_varlen_kernel  mio_qknorm_rope_and_cache_varlen(_kv8): rope_and_cache_varlen_kernel's write with the norm
//   qknorm_rope_rows_kernel              mio_qknorm_rope_rows: norm and rotation alone (the dense path)
// and shares the device helpers and the host plan of the write unit (cache_write_common.h).
//
// A head row x[0 .. D) becomes n[d] = x[d] * r * w[d], r = rsqrt(sum(x^2) / D + eps), in fp32 and in layernorm_kernel<.., RMS>'s
// order; the first rot elements of n are rotated as rope_rot rotates (neox or interleaved pairing, the caller's fp32 tables),
// the others are n itself; the result is rounded once, to 16 bits or (K into an fp8 cache) to e4m3(clamp(y * (1 / k_scale))).
// Nothing is rounded between the norm and the rotation.  V goes through cw_store untouched.
//
// Thread mapping.  The norm needs one statistic per head row, the same bits for every element of the row.  cache_write.hip's
// rotating kernels lay a row's units on consecutive threads of a flat grid with any number of units per token, so a row may
// straddle a wave; a cross-lane sum over that mapping would be wrong for some shapes.  Here a head row owns a GROUP of
// G = 2^k consecutive lanes, G the smallest power of two that holds the row's units of 8 elements (at most 16: D <= 128); 64 / G
// rows share a wave, a group never crosses a wave, and the lanes past the row's unit count idle (they add 0 to the sum).  A lane
// loads its unit -- one 16-byte chunk and, in the neox pairing, the partner chunk rot / 2 further on; two chunks each for the K
// rows of an fp8 cache (E = 16), which then fill half the group -- sums its squares (exact products: 8- and 11-bit significands),
// and a butterfly of DPP moves inside the group leaves the one sum in every lane: each step adds two partial sums that are equal
// across the lanes they came from, and a + b = b + a bit for bit.  Then the lane normalises, rotates and stores its own unit.
// Registers and DPP only: no LDS, no scratch; every global load of rows, weights and tables and every store is 16 bytes wide.
#include <cmath>

#include "cache_write_common.h"

// the rotating write's device arguments, the two norm weights [D] (16-bit, the rows' dtype), eps and log2 of the group size
struct QknDev {
  CwDev c;
  const void* qw;
  const void* kw;
  float eps;
  int lg;
};

// v + the v of the lane a DPP control names, inside the row of 16 lanes
template <int CTRL>
__device__ __forceinline__ float qkn_xadd(float v) {
  return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}

// The sum of v over the G = 2^lg (<= 16) lanes of a group, the same bits in each of them.  Lane ^ 1 and lane ^ 2 are quad
// permutations; after them a quad holds one value, so the mirror of 8 lanes (lane i <- 7 - i: the other quad) and then of 16
// (the other half) stand for lane ^ 4 and lane ^ 8.  Every lane of the group must be here (an idle lane with v = 0).
__device__ __forceinline__ float qkn_group_sum(float v, int lg) {
  if (lg > 0) v = qkn_xadd<0xB1>(v);   // quad_perm [1,0,3,2]
  if (lg > 1) v = qkn_xadd<0x4E>(v);   // quad_perm [2,3,0,1]
  if (lg > 2) v = qkn_xadd<0x141>(v);  // row_half_mirror
  if (lg > 3) v = qkn_xadd<0x140>(v);  // row_mirror
  return v;
}

// where unit u of a head row sits: e0 its first element, rotu whether it is rotated; false for a lane past the row's units
template <int E, bool IL>
__device__ __forceinline__ bool qkn_place(int u, int D, int rot, int& e0, bool& rotu) {
  int nrot, upr;
  rope_units<E, IL>(D, rot, nrot, upr);
  rotu = u < nrot;
  e0 = rotu ? u * E : rot + (u - nrot) * E;
  return u < upr;
}

// Unit u of the head row src, normalised with the weight w and rotated at table row (cos, sin), left in fp32: a = elements
// e0 .. e0 + E and (a rotated unit of the neox pairing) b = those rot / 2 further on.  The one place a row is computed: the Q
// rows of the fused write, its K rows and the rows of the standalone form all come through here.  Called by every lane of the
// row's group; false for an idle lane, which has nothing to store.
template <typename T, int E, bool IL>
__device__ __forceinline__ bool qkn_unit(const T* src, const T* w, const float* cos, const float* sin, int u, int D, int rot,
                                         float eps, int lg, int& e0, bool& rotu, float* a, float* b) {
  const bool act = qkn_place<E, IL>(u, D, rot, e0, rotu);
  const bool two = !IL && rotu;
  const int half = rot >> 1;
  float ss = 0.f;
  if (act) {
    rope_ld<T, E>(src + e0, a);
#pragma unroll
    for (int i = 0; i < E; ++i) ss += a[i] * a[i];
    if (two) {
      rope_ld<T, E>(src + e0 + half, b);
#pragma unroll
      for (int i = 0; i < E; ++i) ss += b[i] * b[i];
    }
  }
  ss = qkn_group_sum(ss, lg);
  if (!act) return false;
  const float r = rsqrtf(ss / (float)D + eps);
  float wv[E];
  rope_ld<T, E>(w + e0, wv);
#pragma unroll
  for (int i = 0; i < E; ++i) a[i] = a[i] * r * wv[i];
  if (two) {
    rope_ld<T, E>(w + e0 + half, wv);
#pragma unroll
    for (int i = 0; i < E; ++i) b[i] = b[i] * r * wv[i];
  }
  if (rotu) rope_rot<E, IL>(cos, sin, e0, a, b);
  return true;
}

// One unit of a 16-bit row, normalised and rotated into dst (the Q rows of the fused write, every row of qknorm_rope_rows); both
// chunks of a unit are read before either is written and no other lane reads them, so dst may be src.  live false (the whole
// group's): the row is written as zeros.
template <typename T, bool IL>
__device__ __forceinline__ void qkn_row16(const T* src, T* dst, const T* w, const float* cos, const float* sin, int64_t tab,
                                          int u, int D, int rot, float eps, int lg, bool live) {
  const int half = rot >> 1;
  int e0;
  bool rotu;
  if (!live) {
    if (!qkn_place<8, IL>(u, D, rot, e0, rotu)) return;
    rope_zero<T, 8>(dst + e0);
    if (!IL && rotu) rope_zero<T, 8>(dst + e0 + half);
    return;
  }
  float a[8], b[8];
  if (!qkn_unit<T, 8, IL>(src, w, cos + tab, sin + tab, u, D, rot, eps, lg, e0, rotu, a, b)) return;
  rope_st<T, 8>(dst + e0, a);
  if (!IL && rotu) rope_st<T, 8>(dst + e0 + half, b);
}

// ---- qknorm_rope_and_cache_varlen: a packed token is H + Hkv head rows of G lanes each, its Q rows first (into qo), then its K
// rows (units of 8 elements, or 16 for an fp8 cache; into the cache) together with the same chunks of the V head of the same
// index, which go through cw_store exactly as cache_write_varlen_kernel writes them.  The token's sequence, cache position and
// row are cw_tok / cw_row_at's, its liveness rope_and_cache_varlen_kernel's; every condition up to qkn_unit is one per token or
// per row, so a group reaches the butterfly whole.
template <typename T, bool KV8, bool IL>
__global__ __launch_bounds__(256) void qknorm_rope_and_cache_varlen_kernel(const QknDev d) {
  constexpr int E = KV8 ? 16 : 8, ESZ = KV8 ? 1 : 2;
  const CwDev& p = d.c;
  const int rpt = p.H + p.Hkv;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, row = i >> d.lg;
  const int u = (int)(i & ((1 << d.lg) - 1));
  if (row >= (int64_t)p.total * rpt) return;
  const int t = (int)(row / rpt), r = (int)(row % rpt);
  const float kinv = cw_inv<KV8>(p.ksc), vinv = cw_inv<KV8>(p.vsc);  // read ahead of the token lookup's dependent loads
  int b, pos = 0;
  const bool in_seq = cw_tok(t, p.cu, p.cl, p.B, p.total, b, pos);
  const int rpos = p.positions ? p.positions[t] : pos;  // the rotation's position; the cache row stays pos's
  const bool live = in_seq && rpos >= 0 && rpos < p.maxpos;
  const int half = p.rot >> 1;
  const int64_t tab = live ? (int64_t)rpos * half : 0;
  if (r < p.H) {
    qkn_row16<T, IL>((const T*)p.q + t * p.qs_t + r * p.qs_h, (T*)p.qo + t * p.os_t + r * p.os_h, (const T*)d.qw, p.cos, p.sin,
                     tab, u, p.D, p.rot, d.eps, d.lg, live);
    return;
  }
  if (!live) return;
  const int hh = r - p.H;
  int64_t crow = -1;
  cw_row_at(b, pos, p.bt, p.num_blocks, p.L, p.layer, p.bs, p.max_blocks,
            [&](int64_t x) __attribute__((always_inline)) { crow = x; });
  if (crow < 0) return;
  float a[E], bb[E];
  int e0;
  bool rotu;
  if (!qkn_unit<T, E, IL>((const T*)p.k + t * p.ks_t + hh * p.ks_h, (const T*)d.kw, p.cos + tab, p.sin + tab, u, p.D, p.rot,
                          d.eps, d.lg, e0, rotu, a, bb))
    return;
  const int64_t dst = (crow * ((int64_t)p.Hkv * p.D) + (int64_t)hh * p.D + e0) * ESZ;
  uint8_t* kc = (uint8_t*)p.kc + dst;
  uint8_t* vc = (uint8_t*)p.vc + dst;
  const T* vp = (const T*)p.v + t * p.vs_t + hh * p.vs_h + e0;
  cw_store<T, KV8>(vc, vp, vinv);
  if (!IL && rotu) cw_store<T, KV8>(vc + half * ESZ, vp + half, vinv);  // the partner chunk as well
  rope_st_cache<T, KV8>(kc, a, kinv);
  if (!IL && rotu) rope_st_cache<T, KV8>(kc + half * ESZ, bb, kinv);
}

// ---- qknorm_rope_rows: x [tokens, heads, D] by (token, head) strides normalised with w and rotated into out (which may be x) at
// positions[token]; a position outside [0, maxpos) writes the row as zeros.  Group i >> lg owns head (i >> lg) % heads.
template <typename T, bool IL>
__global__ __launch_bounds__(256) void qknorm_rope_rows_kernel(const T* x, T* out, const T* __restrict__ w,
                                                               const int32_t* __restrict__ positions,
                                                               const float* __restrict__ cos, const float* __restrict__ sin,
                                                               int64_t xs_t, int64_t xs_h, int64_t os_t, int64_t os_h,
                                                               int tokens, int heads, int D, int rot, int maxpos, float eps,
                                                               int lg) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, row = i >> lg;
  const int u = (int)(i & ((1 << lg) - 1));
  if (row >= (int64_t)tokens * heads) return;
  const int t = (int)(row / heads), h = (int)(row % heads);
  const int rpos = positions[t];
  const bool live = rpos >= 0 && rpos < maxpos;
  qkn_row16<T, IL>(x + t * xs_t + h * xs_h, out + t * os_t + h * os_h, w, cos, sin, live ? (int64_t)rpos * (rot >> 1) : 0, u, D,
                   rot, eps, lg, live);
}

// ---- host ----------------------------------------------------------------------------------------------------------------
// log2 of the group size: the smallest power of two that holds a 16-bit row's units of 8 elements (1 .. 16 of them)
static int qkn_lg(int32_t D, int32_t rot_dim, int32_t interleaved) {
  const int upr = (interleaved ? rot_dim / 8 : rot_dim / 16) + (D - rot_dim) / 8;
  int lg = 0;
  while ((1 << lg) < upr) ++lg;
  return lg;
}

static int qkn_check_eps(const std::string& fn, float eps) {
  MIO_CHECK(std::isfinite(eps) && eps >= 0.f, fn + ": eps must be finite and not negative");
  return 0;
}

static int qkn_check_weight(const std::string& fn, const void* w, const char* what) {
  MIO_CHECK(w, fn + ": null norm weight (" + what + ")");
  MIO_CHECK(mio_aligned16(w), fn + ": 16-byte alignment (norm weight " + what + ")");
  return 0;
}

// both fused forms: the rotating write's plan (every check of mio_rope_and_cache_varlen(_kv8) under this form's name), then the
// norm's own arguments, then the grid of groups
static int qkn_cache_run(const CwForm& f, const void* q, void* q_out, const void* key, const void* value, void* k_cache,
                         void* v_cache, const float* k_scale, const float* v_scale, const int32_t* block_tables,
                         const int32_t* cu_seqlens_new, const int32_t* context_lengths, const int32_t* positions,
                         const float* cos, const float* sin, const void* q_weight, const void* k_weight,
                         const int64_t* q_stride, const int64_t* q_out_stride, const int64_t* k_stride, const int64_t* v_stride,
                         int32_t B, int32_t total_new, int32_t H, int32_t Hkv, int32_t D, int32_t rot_dim, int32_t max_position,
                         int32_t interleaved, int32_t num_blocks, int32_t num_layers, int32_t layer_idx, int32_t block_size,
                         int32_t max_blocks_per_seq, int32_t dtype, float eps, void* stream) {
  const std::string fn = f.name;
  CwCall c = cw_call(key, value, k_cache, v_cache, block_tables, context_lengths, k_stride, v_stride, B, Hkv, D, num_layers,
                     layer_idx, block_size, max_blocks_per_seq, dtype, cu_seqlens_new, total_new, num_blocks);
  cw_call_rope(c, q, q_out, k_scale, v_scale, positions, cos, sin, q_stride, q_out_stride, H, rot_dim, max_position, interleaved);
  QknDev d;
  int64_t work;
  if (cw_plan(f, c, d.c, work) != 0 || qkn_check_eps(fn, eps) != 0) return -1;
  if (work == 0) return 0;
  if (qkn_check_weight(fn, q_weight, "q_weight") != 0 || qkn_check_weight(fn, k_weight, "k_weight") != 0) return -1;
  d.qw = q_weight, d.kw = k_weight, d.eps = eps, d.lg = qkn_lg(D, rot_dim, interleaved);
  const int64_t blocks = ((((int64_t)total_new * ((int64_t)H + Hkv)) << d.lg) + 255) / 256;
  MIO_CHECK(blocks <= 0x7fffffff, fn + ": too many tokens");
  const dim3 grid((unsigned)blocks), wg(256);
  hipStream_t st = (hipStream_t)stream;
#define QKN_IL(T, KV8)                                                                                              \
  do {                                                                                                              \
    if (interleaved) hipLaunchKernelGGL((qknorm_rope_and_cache_varlen_kernel<T, KV8, true>), grid, wg, 0, st, d);   \
    else hipLaunchKernelGGL((qknorm_rope_and_cache_varlen_kernel<T, KV8, false>), grid, wg, 0, st, d);              \
  } while (0)
#define QKN_DTYPE(KV8)                       \
  do {                                       \
    if (dtype == MIO_BF16) QKN_IL(__bf16, KV8); \
    else QKN_IL(_Float16, KV8);              \
  } while (0)
  if (f.kv8) QKN_DTYPE(true);
  else QKN_DTYPE(false);
#undef QKN_DTYPE
#undef QKN_IL
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mio_fail(std::string(f.launch) + " launch: " + hipGetErrorString(e));
  return 0;
}

// name, launch-failure prefix, varlen, fp8 cache, rotating
static const CwForm QKN_16 = {"mio_qknorm_rope_and_cache_varlen", "mio_qknorm_rope_and_cache_varlen", true, false, true};
static const CwForm QKN_KV8 = {"mio_qknorm_rope_and_cache_varlen_kv8", "mio_qknorm_rope_and_cache_varlen_kv8", true, true, true};

extern "C" int mio_qknorm_rope_and_cache_varlen(const void* q, void* q_out, const void* key, const void* value, void* k_cache,
                                                void* v_cache, const int32_t* block_tables, const int32_t* cu_seqlens_new,
                                                const int32_t* context_lengths, const int32_t* positions, const float* cos,
                                                const float* sin, const void* q_weight, const void* k_weight,
                                                const int64_t q_stride[2], const int64_t q_out_stride[2],
                                                const int64_t k_stride[2], const int64_t v_stride[2], int32_t B,
                                                int32_t total_new, int32_t H, int32_t Hkv, int32_t D, int32_t rot_dim,
                                                int32_t max_position, int32_t interleaved, int32_t num_blocks,
                                                int32_t num_layers, int32_t layer_idx, int32_t block_size,
                                                int32_t max_blocks_per_seq, int32_t dtype, float eps, void* stream) {
  return qkn_cache_run(QKN_16, q, q_out, key, value, k_cache, v_cache, nullptr, nullptr, block_tables, cu_seqlens_new,
                       context_lengths, positions, cos, sin, q_weight, k_weight, q_stride, q_out_stride, k_stride, v_stride, B,
                       total_new, H, Hkv, D, rot_dim, max_position, interleaved, num_blocks, num_layers, layer_idx, block_size,
                       max_blocks_per_seq, dtype, eps, stream);
}

extern "C" int mio_qknorm_rope_and_cache_varlen_kv8(const void* q, void* q_out, const void* key, const void* value,
                                                    void* k_cache, void* v_cache, const float* k_scale, const float* v_scale,
                                                    const int32_t* block_tables, const int32_t* cu_seqlens_new,
                                                    const int32_t* context_lengths, const int32_t* positions,
                                                    const float* cos, const float* sin, const void* q_weight,
                                                    const void* k_weight, const int64_t q_stride[2],
                                                    const int64_t q_out_stride[2], const int64_t k_stride[2],
                                                    const int64_t v_stride[2], int32_t B, int32_t total_new, int32_t H,
                                                    int32_t Hkv, int32_t D, int32_t rot_dim, int32_t max_position,
                                                    int32_t interleaved, int32_t num_blocks, int32_t num_layers,
                                                    int32_t layer_idx, int32_t block_size, int32_t max_blocks_per_seq,
                                                    int32_t dtype, float eps, void* stream) {
  return qkn_cache_run(QKN_KV8, q, q_out, key, value, k_cache, v_cache, k_scale, v_scale, block_tables, cu_seqlens_new,
                       context_lengths, positions, cos, sin, q_weight, k_weight, q_stride, q_out_stride, k_stride, v_stride, B,
                       total_new, H, Hkv, D, rot_dim, max_position, interleaved, num_blocks, num_layers, layer_idx, block_size,
                       max_blocks_per_seq, dtype, eps, stream);
}

extern "C" int mio_qknorm_rope_rows(const void* x, void* out, const int32_t* positions, const float* cos, const float* sin,
                                    const void* weight, const int64_t x_stride[2], const int64_t out_stride[2], int32_t tokens,
                                    int32_t heads, int32_t D, int32_t rot_dim, int32_t max_position, int32_t interleaved,
                                    int32_t dtype, float eps, void* stream) {
  const std::string fn = "mio_qknorm_rope_rows";
  MIO_CHECK(x_stride && out_stride, fn + ": null strides");
  MIO_CHECK(tokens >= 0 && heads > 0, fn + ": bad sizes");
  if (rope_check_rot(fn, false, cos, sin, D, rot_dim, max_position, interleaved, dtype) != 0 || qkn_check_eps(fn, eps) != 0)
    return -1;
  if (tokens == 0) return 0;
  MIO_CHECK(x && out && positions, fn + ": null pointer");
  MIO_CHECK(rope_strides_ok(x_stride) && rope_strides_ok(out_stride) && mio_aligned16(x) && mio_aligned16(out) &&
                ((uintptr_t)positions & 3) == 0,
            fn + ": 16-byte alignment");
  if (qkn_check_weight(fn, weight, "weight") != 0) return -1;
  const int lg = qkn_lg(D, rot_dim, interleaved);
  const int64_t blocks = ((((int64_t)tokens * heads) << lg) + 255) / 256;
  MIO_CHECK(blocks <= 0x7fffffff, fn + ": too many tokens");
  const dim3 grid((unsigned)blocks), wg(256);
  hipStream_t st = (hipStream_t)stream;
#define QKN_ROWS(T, IL)                                                                                                        \
  hipLaunchKernelGGL((qknorm_rope_rows_kernel<T, IL>), grid, wg, 0, st, (const T*)x, (T*)out, (const T*)weight, positions, cos, \
                     sin, x_stride[0], x_stride[1], out_stride[0], out_stride[1], tokens, heads, D, rot_dim, max_position, eps, lg)
  if (dtype == MIO_BF16) {
    if (interleaved) QKN_ROWS(__bf16, true);
    else QKN_ROWS(__bf16, false);
  } else {
    if (interleaved) QKN_ROWS(_Float16, true);
    else QKN_ROWS(_Float16, false);
  }
#undef QKN_ROWS
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mio_fail(fn + " launch: " + hipGetErrorString(e));
  return 0;
}

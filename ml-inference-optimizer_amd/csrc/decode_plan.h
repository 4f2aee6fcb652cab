// Decode launch state, the plan of a launch (argument checks, kernel choice, split geometry) and its rules, shared by the
// 16-bit decode (decode_paged.hip) and the fp8-cache decode (decode_kv8.hip), with the split-merge kernel both launch.
// The kernel bodies (decode_paged_body.inc, decode_rows_body.inc, decode_gqa_body.inc) serve both caches: each unit's
// kernels include them with KV8 false (16-bit elements) or true (one e4m3fn byte per element, kv8_cvt.h).
#pragma once
#include <algorithm>
#include <cstdlib>
#include <string>

#include "mio_common.h"
#include "kv8_cvt.h"

struct DecDev {
  const void* q;
  void* o;
  const void* kc;
  const void* vc;
  const int32_t* bt;
  const int32_t* cl;
  float* ws_o;    // [rows, nsplit, D]
  float* ws_lse;  // [rows, nsplit]
  int64_t qs_b, qs_h, qs_s, os_b, os_h, os_s;
  int B, H, Hkv, q_len, D, L, layer, bs, max_blocks, nsplit, split_len;
  float scale;
};

// each element of one 16-byte chunk of the cache as fp32, in order: f(i, x) for the 8 16-bit elements, or (KV8) the 16
// e4m3fn bytes
template <typename T, bool KV8, typename F>
__device__ __forceinline__ void dec_chunk_each(u32x4_t raw, F&& f) {
  if constexpr (KV8) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      float x[4];
      kv8_to_f32x4(raw[w], x);
#pragma unroll
      for (int i = 0; i < 4; ++i) f(4 * w + i, x[i]);
    }
  } else {
    const typename DT<T>::x8 v = __builtin_bit_cast(typename DT<T>::x8, raw);
#pragma unroll
    for (int i = 0; i < 8; ++i) f(i, (float)v[i]);
  }
}

#include "decode_gqa_kernel.h"

// decode_gqa_kernel (matrix-core form): one workgroup per (sequence, kv head, split); the split count aims at one
// (D 128: 136 KiB of LDS) or two (D 64, or the fp8 cache's image of one byte per element) workgroups per CU, 128-key
// granularity (4 waves x 32-key chunks); esz: bytes per cached element
static inline int dec_nsplit_gqa(int64_t units, int max_ctx, int bs, int D = 128, int esz = 2) {
  // workgroups aimed for = what is resident at once (D 128: 136 KiB of LDS, one per CU; D 64: two per CU); a second round of
  // workgroups costs its tail (tools/dbg/dec_gqa_ab.py, B 64 H 32 Hkv 4 D 128: 256 -> 5.68 TB/s, 512 -> 5.37, 2048 -> 4.50)
  int target = D * esz > 128 ? 256 : 512;
#ifdef MIO_DIAG
  if (mio_dbg_get(2) > 0) target = mio_dbg_get(2);
#endif
  int want = (int)((target + units - 1) / units);
  int cap = (max_ctx + 255) / 256;  // >= 256 keys per split
  if (cap < 1) cap = 1;
  if (want > cap) want = cap;
  if (want < 1) want = 1;
  // a split's block-table slice must fit its LDS image
  while (((int64_t)(max_ctx + want - 1) / want + 127) / bs + 2 > DG_BT_MAX) ++want;
  return want;
}
// Picked when 2 .. 16 query vectors share a cached key ((H / Hkv) * q_len): the vector-ALU kernels are HBM-bound with one
// (5.7-5.9 TB/s at MHA) and fall off from there -- tools/dbg/dec_gqa_small_qn.py, shipped-before vs this kernel: 2 vectors
// 5.52 -> 6.16 TB/s (D 128, B 64), 2.31 -> 3.25 (D 64, B 8), 5.46 -> 5.25 (D 64, two query positions: the one loss); 3 vectors
// 2.36 -> 5.75; 4 vectors 3.32 -> 5.48 and 1.67 -> 4.89 at B 1 x ctx 131072; 8 vectors 1.04 -> 5.4-5.7.  With one vector it
// is 8 % slower at D 64 (5.20 vs 5.68: left to the row kernels) and 2 % faster at D 128 (taken).
static inline bool dec_gqa_ok(int B, int H, int Hkv, int q_len, int D, int max_ctx, int bs, const int64_t* os, const void* o) {
  const int qn = (H / Hkv) * q_len;
  if (qn > 16 || (qn < 2 && D != 128)) return false;  // one query vector per key: only at D 128 (5.90 -> 6.05, 5.49 -> 5.62 TB/s)
  if (D != 64 && D != 128) return false;
  if (max_ctx < 1) return false;
  if (os[0] % 8 != 0 || os[1] % 8 != 0 || os[2] % 8 != 0 || !mio_aligned16(o)) return false;  // 16-byte output stores
  return true;
}

static inline int dec_nsplit(int B, int H, int q_len, int max_ctx) {
  const int64_t rows = (int64_t)B * H * q_len;
#ifdef MIO_DIAG
  static const int wgs = [] {  // MIO_DEC_WGS: workgroups the split aims for (tuning aid)
    const char* e = std::getenv("MIO_DEC_WGS");
    const int v = e ? std::atoi(e) : 0;
    return v > 0 ? v : 512;
  }();
#else
  constexpr int wgs = 512;  // workgroups the split aims for: 2 per CU
#endif
  int want = (int)((wgs + rows - 1) / rows);
  int cap = (max_ctx + 255) / 256;
  if (cap < 1) cap = 1;
  if (want > cap) want = cap;
  if (want < 1) want = 1;
  return want;
}

// whole-token-row kernel (decode_rows_kernel): one workgroup per (sequence, split) -> the split count aims at the same
// number of workgroups with B sequences instead of B * H * q_len rows
static inline int dec_nsplit_rows(int B, int max_ctx) {
  int target = 512;  // workgroups aimed for: 2 per CU (sweep 256 .. 4096 at B 8 / 32 / 64 / 256: tools/dbg/dec_rows_sweep.py)
#ifdef MIO_DIAG
  if (mio_dbg_get(2) > 0) target = mio_dbg_get(2);  // tuning sweep (tools/dbg/dec_rows_sweep.py)
#endif
  int want = (target + B - 1) / B;
  int cap = (max_ctx + 63) / 64;
  if (cap < 1) cap = 1;
  if (want > cap) want = cap;
  if (want < 1) want = 1;
  return want;
}
// Picked for B >= 16: at B 8 (128 MiB of cache, Infinity-Cache resident between launches) the per-head kernel's 512
// small workgroups run 28 us against 40-46 us here; from B 32 on (streams from HBM) the whole-row reads win:
// B 64 H 16 D 64 187 -> 183 us (5.87 TB/s), B 256 6.06 TB/s (tools/dbg/dec_rows_sweep.py).
// esz: bytes per cached element (2, or 1 for the fp8 cache: the byte estimate and the 16-byte chunks per row follow it)
static inline bool dec_rows_ok(int B, int H, int Hkv, int q_len, int D, int max_ctx, int esz = 2) {
  // a cache that fits the 256 MiB Infinity Cache between steps (B 8 at ctx 4096: 128 MiB) is read faster by the per-head
  // kernel's many small workgroups (28 vs 40-46 us); one that streams from HBM goes through whole token rows from B 8 on
  // (round 3, B 8 x ctx 32768: 5.49 vs 5.42 TB/s; B 4 x ctx 65536: 5.02 vs 5.41 -- too few sequences per split column)
  const double kv_bytes = 2.0 * esz * B * (double)max_ctx * Hkv * D;
  if (B < 16 && (B < 8 || kv_bytes <= 200.0 * 1048576.0)) return false;
  if (D != 64 && D != 128) return false;
  const int cpt = Hkv * (D * esz / 16), qn = (H / Hkv) * q_len;
  return cpt >= 16 && cpt <= 256 && (cpt & (cpt - 1)) == 0 && qn == 1;  // 2 .. 16 query vectors per key: decode_gqa_kernel
}

template <typename T>
__global__ __launch_bounds__(128) void decode_reduce_kernel(const DecDev p) {
  const int row = blockIdx.x, d = threadIdx.x;
  if (d >= p.D) return;
  const int qi = row % p.q_len;
  const int h = (row / p.q_len) % p.H;
  const int b = row / (p.q_len * p.H);
  float M = -INFINITY;
  for (int s = 0; s < p.nsplit; ++s) M = fmaxf(M, p.ws_lse[(int64_t)row * p.nsplit + s]);
  float W = 0.f, acc = 0.f;
  if (M != -INFINITY) {
    for (int s = 0; s < p.nsplit; ++s) {
      const float w = __expf(p.ws_lse[(int64_t)row * p.nsplit + s] - M);
      W += w;
      acc += w * p.ws_o[((int64_t)row * p.nsplit + s) * p.D + d];
    }
  }
  ((T*)p.o)[b * p.os_b + h * p.os_h + (int64_t)qi * p.os_s + d] = (T)((W > 0.f) ? acc / W : 0.f);
}

// a window no shorter than max_ctx + q_len is the unbounded one: clamped, so the kernels' bounds stay in int
static inline int32_t dec_window(int32_t window_left, int32_t max_ctx, int32_t q_len) {
  if (window_left < 0) return window_left;
  return (int32_t)std::min<int64_t>(std::min<int64_t>(window_left, (int64_t)max_ctx + q_len), 1 << 29);
}

// The checks, kernel choice and split geometry of a decode launch, shared by both caches' launches (wleft = -1: no window)
// and their host-only route queries; fn prefixes the messages.  route: a mio_decode_route_t.  esz: bytes per cached element,
// 2, or 1 for the fp8 cache, which needs k_scale / v_scale (the 16-bit one ignores them).  With a window the kernel
// heuristics and the split count see the span min(max_ctx, wleft + q_len) as the context length: no split lies past the
// window, and the split count is at most the one of max_ctx (every dec_nsplit* grows with the context length), so
// mio_fa3_decode_workspace_bytes(max_ctx) covers it.
static inline int dec_plan(DecDev& p, int& route, const std::string& fn, int esz, const void* q, void* o,
                           const void* k_cache, const void* v_cache, const float* k_scale, const float* v_scale,
                           const int32_t* block_tables, const int32_t* context_lengths, const int64_t q_stride[3],
                           const int64_t o_stride[3], int32_t B, int32_t H, int32_t Hkv, int32_t q_len, int32_t D,
                           int32_t num_layers, int32_t layer_idx, int32_t block_size, int32_t max_blocks_per_seq,
                           int32_t max_ctx, float scale, int32_t dtype, int32_t wleft) {
  const bool kv8 = esz == 1;
  MIO_CHECK(q && o && k_cache && v_cache && block_tables && context_lengths && q_stride && o_stride, fn + ": null pointer");
  if (kv8) {
    MIO_CHECK(k_scale && v_scale, fn + ": k_scale and v_scale are required with an fp8 cache (null scale pointer)");
    MIO_CHECK(((uintptr_t)k_scale & 3) == 0 && ((uintptr_t)v_scale & 3) == 0, fn + ": scales must be 4-byte aligned fp32");
  }
  MIO_CHECK(B > 0 && H > 0 && Hkv > 0 && H % Hkv == 0 && q_len > 0, fn + ": bad sizes");
  if (kv8) MIO_CHECK(D >= 16 && D <= 128 && D % 16 == 0, fn + ": head_dim must be a multiple of 16 in [16,128] for an fp8 cache");
  else MIO_CHECK(D >= 8 && D <= 128 && D % 8 == 0, fn + ": head_dim must be a multiple of 8 in [8,128]");
  MIO_CHECK(layer_idx >= 0 && layer_idx < num_layers, fn + ": layer_idx out of range");
  MIO_CHECK(block_size > 0 && max_blocks_per_seq > 0 && max_ctx >= 0, fn + ": bad cache geometry");
  MIO_CHECK(dtype == MIO_BF16 || dtype == MIO_FP16, fn + (kv8 ? ": dtype (of q and o) must be bf16 or fp16" : ": dtype must be bf16 or fp16"));
  MIO_CHECK(wleft >= -1, fn + ": window_left must be -1 (unbounded) or >= 0");
  MIO_CHECK(wleft < 0 || q_len < (1 << 29), fn + ": q_len must be below 2^29 under a window");
  MIO_CHECK(q_stride[0] % 8 == 0 && q_stride[1] % 8 == 0 && q_stride[2] % 8 == 0 && mio_aligned16(q) &&
                mio_aligned16(k_cache) && mio_aligned16(v_cache),
            fn + ": q/cache rows must be 16-byte aligned");
  p.q = q; p.o = o; p.kc = k_cache; p.vc = v_cache; p.bt = block_tables; p.cl = context_lengths;
  p.qs_b = q_stride[0]; p.qs_h = q_stride[1]; p.qs_s = q_stride[2];
  p.os_b = o_stride[0]; p.os_h = o_stride[1]; p.os_s = o_stride[2];
  p.B = B; p.H = H; p.Hkv = Hkv; p.q_len = q_len; p.D = D; p.L = num_layers; p.layer = layer_idx;
  p.bs = block_size; p.max_blocks = max_blocks_per_seq; p.scale = scale;
  // the keys a sequence's splits cover: all of max_ctx, or the window span
  const int span = (wleft >= 0 && (int64_t)wleft + q_len < max_ctx) ? wleft + q_len : max_ctx;
  bool rows_kernel = dec_rows_ok(B, H, Hkv, q_len, D, span, esz);
  bool gqa_kernel = dec_gqa_ok(B, H, Hkv, q_len, D, span, block_size, o_stride, o);
#ifdef MIO_DIAG
  if (!kv8 && mio_dbg_get(6) == 1) rows_kernel = gqa_kernel = false;  // A/B: the per-head kernel (tools/dbg/dec_rows_ab.py)
  if (!kv8 && mio_dbg_get(6) == 2) gqa_kernel = false;                // A/B: rows kernel where it applies
  if (!kv8 && mio_dbg_get(6) == 3)                                    // A/B: the matrix-core kernel for 1 .. 4 query vectors too
    gqa_kernel = (H / Hkv) * q_len <= 16 && (D == 64 || D == 128) && o_stride[0] % 8 == 0 && o_stride[1] % 8 == 0 &&
                 o_stride[2] % 8 == 0 && mio_aligned16(o);
#endif
  if (gqa_kernel) rows_kernel = false;
  route = gqa_kernel ? MIO_DEC_ROUTE_GQA : rows_kernel ? MIO_DEC_ROUTE_ROWS : MIO_DEC_ROUTE_HEAD;
  p.nsplit = gqa_kernel ? dec_nsplit_gqa((int64_t)B * Hkv, span, block_size, D, esz)
                        : rows_kernel ? dec_nsplit_rows(B, span) : dec_nsplit(B, H, q_len, span);
  int sl = (span + p.nsplit - 1) / p.nsplit;
  const int gran = gqa_kernel ? 128 : 32;
  sl = (sl + gran - 1) / gran * gran;
  if (sl < gran) sl = gran;
  p.split_len = sl;
  return 0;
}

// the split states' workspace [rows, nsplit, D] fp32 then [rows, nsplit] lse, required with more than one split
static inline int dec_workspace(DecDev& p, const std::string& fn, void* workspace) {
  MIO_CHECK(p.nsplit == 1 || workspace != nullptr, fn + ": workspace required");
  p.ws_o = (float*)workspace;
  p.ws_lse = p.ws_o ? p.ws_o + (int64_t)p.B * p.H * p.q_len * p.nsplit * p.D : nullptr;
  return 0;
}

// a gqa kernel's launch: its dynamic LDS (above the default limit) is raised once per kernel, on its first launch
template <auto KERN, int SMEM, typename... A>
static int dec_launch_gqa(const char* name, const DecDev& p, hipStream_t st, const A&... args) {
  static const hipError_t ea = hipFuncSetAttribute((const void*)KERN, hipFuncAttributeMaxDynamicSharedMemorySize, SMEM);
  if (ea != hipSuccess) return mio_fail(std::string(name) + ": hipFuncSetAttribute: " + hipGetErrorString(ea));
  hipLaunchKernelGGL(KERN, dim3((unsigned)(p.B * p.Hkv), (unsigned)p.nsplit), dim3(256), SMEM, st, p, args...);
  return 0;
}

// the merge of the splits' partial states, when there are several
template <typename T>
static void dec_merge(const DecDev& p, hipStream_t st) {
  if (p.nsplit > 1) hipLaunchKernelGGL(decode_reduce_kernel<T>, dim3((unsigned)((int64_t)p.B * p.H * p.q_len)), dim3(128), 0, st, p);
}

// Decode launch state, split planning and kernel-choice rules shared by the 16-bit decode (decode_paged.hip) and the
// fp8-cache decode (decode_kv8.hip), and the split-merge kernel both launch.
#pragma once
#include <cstdlib>

#include "mio_common.h"

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

#include "decode_gqa_kernel.h"

// decode_gqa_kernel (matrix-core form): one workgroup per (sequence, kv head, split); the split count aims at one
// (D 128: 136 KiB of LDS) or two (D 64) workgroups per CU, 128-key granularity (4 waves x 32-key chunks); target > 0 sets
// the workgroups aimed for (the fp8-cache kernel's smaller LDS image)
static inline int dec_nsplit_gqa(int64_t units, int max_ctx, int bs, int D = 128, int target = 0) {
  // workgroups aimed for = what is resident at once (D 128: 136 KiB of LDS, one per CU; D 64: two per CU); a second round of
  // workgroups costs its tail (tools/dbg/dec_gqa_ab.py, B 64 H 32 Hkv 4 D 128: 256 -> 5.68 TB/s, 512 -> 5.37, 2048 -> 4.50)
  if (target <= 0) target = D > 64 ? 256 : 512;
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

// FP8 paged KV cache (OCP e4m3fn, torch.float8_e4m3fn) for CDNA4 (gfx950): the three decode kernels of decode_paged.hip
// over one byte per cached element; decode only: the quantising writes into the cache are cache_write.hip's.
//
// Same cache layout, one byte per element: [num_blocks, num_layers, block_size, Hkv, D].  A cached element x8 stands for
// x8 * scale with one fp32 scale per (K or V, layer), read by the kernels from device memory (no host sync: a scale may change
// between replays of a captured graph).  The host passes the address of the scale of layer_idx.
//   write:  q = e4m3(clamp(float(x) * (1 / scale), -448, 448)), round to nearest even; NaN stays NaN (cache_write.hip)
//   decode: every e4m3 value is exact in bf16 / fp16 / fp32, so K and V enter the products unrounded; k_scale is folded into
//           the score scale, v_scale into the output of each split before its partial state is stored (the split merge,
//           decode_reduce_kernel, is linear in o and is the 16-bit one).  Q and the softmax weights stay 16-bit / fp32.
// The decode kernels include the 16-bit kernels' bodies with KV8 = true (16 elements per 16-byte chunk, the conversions of
// kv8_cvt.h); the plan (checks, route, splits) is decode_plan.h's dec_plan with one byte per element:
//   decode_paged_kv8_kernel  (route head)  one workgroup per (query row, split), a lane owns one 16-element chunk of a head row
//   decode_rows_kv8_kernel   (route rows)  one workgroup per (sequence, split) over whole token rows of Hkv * D bytes
//   decode_gqa_kv8_kernel    (route gqa)   matrix core: K / V by DMA into a 32 * D-byte LDS image per 32-key half; the K
//                                          fragment is one ds_read_b64 + 4 v_cvt_scalef32_pk_{bf16,f16}_fp8, the V^T fragment
//                                          one ds_read_b64_tr_b8 + 4 conversions; the MFMAs stay 16x16x32 bf16 / fp16
// and their *_win_kernel forms take a sliding window as decode_paged.hip's do.
#include "mio_common.h"

#include "decode_plan.h"

// ---- route head: CPRP = 16-byte chunks per head row padded to a power of two (4 for D <= 64, 8 for D <= 128)
template <typename T, int CPRP>
__global__ __launch_bounds__(256) void decode_paged_kv8_kernel(const DecDev p, const float* ksc, const float* vsc) {
  constexpr int U = 2;
  constexpr bool WIN = false, KV8 = true;
  [[maybe_unused]] constexpr int wleft = 0;
#include "decode_paged_body.inc"
}

template <typename T, int CPRP>
__global__ __launch_bounds__(256) void decode_paged_kv8_win_kernel(const DecDev p, const float* ksc, const float* vsc,
                                                                   int wleft) {
  constexpr int U = 2;
  constexpr bool WIN = true, KV8 = true;
#include "decode_paged_body.inc"
}

// ---- route rows: CPR = D / 16 chunks per head row, CPT = Hkv * CPR per token row (16 .. 256, a power of two: dec_rows_ok
// with one byte per element); one query vector per key
template <typename T, int CPR>
__global__ __launch_bounds__(256) void decode_rows_kv8_kernel(const DecDev p, const float* ksc, const float* vsc) {
  constexpr int QN = 1;
  constexpr bool WIN = false, KV8 = true;
  [[maybe_unused]] constexpr int wleft = 0;
#include "decode_rows_body.inc"
}

template <typename T, int CPR>
__global__ __launch_bounds__(256) void decode_rows_kv8_win_kernel(const DecDev p, const float* ksc, const float* vsc,
                                                                  int wleft) {
  constexpr int QN = 1;
  constexpr bool WIN = true, KV8 = true;
#include "decode_rows_body.inc"
}

// ---- route gqa: matrix core over the one-byte LDS image (dg_kv8_sw, decode_gqa_kernel.h)
template <typename T, int D>
__global__ __launch_bounds__(256) void decode_gqa_kv8_kernel(const DecDev p, const float* ksc, const float* vsc) {
  constexpr bool WIN = false, KV8 = true;
  [[maybe_unused]] constexpr int wleft = 0;
#include "decode_gqa_body.inc"
}

template <typename T, int D>
__global__ __launch_bounds__(256) void decode_gqa_kv8_win_kernel(const DecDev p, const float* ksc, const float* vsc,
                                                                 int wleft) {
  constexpr bool WIN = true, KV8 = true;
#include "decode_gqa_body.inc"
}

// ---- host: launches
template <typename T>
static int kv8_run(const DecDev& p, int route, int wleft, const float* ks, const float* vs, hipStream_t st) {
  const bool win = wleft >= 0;
  if (route == MIO_DEC_ROUTE_GQA) {
    constexpr int S128 = dg_smem_bytes<128, 1>(), S64 = dg_smem_bytes<64, 1>();
    int rc;
    if (p.D == 128) {
      rc = win ? dec_launch_gqa<decode_gqa_kv8_win_kernel<T, 128>, S128>("decode_gqa_kv8", p, st, ks, vs, wleft)
               : dec_launch_gqa<decode_gqa_kv8_kernel<T, 128>, S128>("decode_gqa_kv8", p, st, ks, vs);
    } else {
      rc = win ? dec_launch_gqa<decode_gqa_kv8_win_kernel<T, 64>, S64>("decode_gqa_kv8", p, st, ks, vs, wleft)
               : dec_launch_gqa<decode_gqa_kv8_kernel<T, 64>, S64>("decode_gqa_kv8", p, st, ks, vs);
    }
    if (rc != 0) return rc;
  } else if (route == MIO_DEC_ROUTE_ROWS) {  // one query vector per key (dec_rows_ok)
    const dim3 grid((unsigned)p.B, (unsigned)p.nsplit);
    if (p.D == 64) {
      if (win) hipLaunchKernelGGL((decode_rows_kv8_win_kernel<T, 4>), grid, dim3(256), 0, st, p, ks, vs, wleft);
      else hipLaunchKernelGGL((decode_rows_kv8_kernel<T, 4>), grid, dim3(256), 0, st, p, ks, vs);
    } else {
      if (win) hipLaunchKernelGGL((decode_rows_kv8_win_kernel<T, 8>), grid, dim3(256), 0, st, p, ks, vs, wleft);
      else hipLaunchKernelGGL((decode_rows_kv8_kernel<T, 8>), grid, dim3(256), 0, st, p, ks, vs);
    }
  } else {
    const dim3 grid((unsigned)((int64_t)p.B * p.H * p.q_len), (unsigned)p.nsplit);
    if (p.D <= 64) {
      if (win) hipLaunchKernelGGL((decode_paged_kv8_win_kernel<T, 4>), grid, dim3(256), 0, st, p, ks, vs, wleft);
      else hipLaunchKernelGGL((decode_paged_kv8_kernel<T, 4>), grid, dim3(256), 0, st, p, ks, vs);
    } else {
      if (win) hipLaunchKernelGGL((decode_paged_kv8_win_kernel<T, 8>), grid, dim3(256), 0, st, p, ks, vs, wleft);
      else hipLaunchKernelGGL((decode_paged_kv8_kernel<T, 8>), grid, dim3(256), 0, st, p, ks, vs);
    }
  }
  dec_merge<T>(p, st);
  return 0;
}

extern "C" int mio_fa3_decode_paged_kv8(const void* q, void* o, const void* k_cache, const void* v_cache,
                                        const float* k_scale, const float* v_scale, const int32_t* block_tables,
                                        const int32_t* context_lengths, const int64_t q_stride[3],
                                        const int64_t o_stride[3], int32_t B, int32_t H, int32_t Hkv, int32_t q_len,
                                        int32_t D, int32_t num_layers, int32_t layer_idx, int32_t block_size,
                                        int32_t max_blocks_per_seq, int32_t max_ctx, float scale, int32_t window_left,
                                        int32_t dtype, void* workspace, void* stream) {
  const std::string fn = "mio_fa3_decode_paged_kv8";
  DecDev p;
  int route = 0;
  const int rc = dec_plan(p, route, fn, 1, q, o, k_cache, v_cache, k_scale, v_scale, block_tables, context_lengths, q_stride,
                          o_stride, B, H, Hkv, q_len, D, num_layers, layer_idx, block_size, max_blocks_per_seq, max_ctx,
                          scale, dtype, window_left);
  if (rc != 0) return rc;
  if (dec_workspace(p, fn, workspace) != 0) return -1;
  const int32_t wleft = dec_window(window_left, max_ctx, q_len);
  hipStream_t st = (hipStream_t)stream;
  const int rl = (dtype == MIO_BF16) ? kv8_run<__bf16>(p, route, wleft, k_scale, v_scale, st)
                                     : kv8_run<_Float16>(p, route, wleft, k_scale, v_scale, st);
  if (rl != 0) return rl;
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mio_fail(std::string("decode_paged_kv8 launch: ") + hipGetErrorString(e));
  return 0;
}

extern "C" int mio_fa3_decode_kv8_route(const void* q, void* o, const void* k_cache, const void* v_cache,
                                        const float* k_scale, const float* v_scale, const int32_t* block_tables,
                                        const int32_t* context_lengths, const int64_t q_stride[3],
                                        const int64_t o_stride[3], int32_t B, int32_t H, int32_t Hkv, int32_t q_len,
                                        int32_t D, int32_t num_layers, int32_t layer_idx, int32_t block_size,
                                        int32_t max_blocks_per_seq, int32_t max_ctx, float scale, int32_t window_left,
                                        int32_t dtype, void* workspace, void* stream) {
  (void)workspace;
  (void)stream;
  DecDev p;
  int route = 0;
  const int rc = dec_plan(p, route, "mio_fa3_decode_kv8_route", 1, q, o, k_cache, v_cache, k_scale, v_scale, block_tables,
                          context_lengths, q_stride, o_stride, B, H, Hkv, q_len, D, num_layers, layer_idx, block_size,
                          max_blocks_per_seq, max_ctx, scale, dtype, dec_window(window_left, max_ctx, q_len));
  return rc != 0 ? rc : route;
}

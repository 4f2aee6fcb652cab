// Paged-KV decode attention for CDNA4 (gfx950); decode only: the writes into the cache are cache_write.hip's.
// HBM-bandwidth-bound: K/V rows go straight from global memory to VGPRs (16 B per lane), no LDS staging, split over the
// context so a small batch still fills 256 CUs; partial (o, lse) states are merged by a second tiny kernel.
//
// Replaces _paged_attention_fwd_kernel (reference kernels/triton/attention_kernels.py:628-808, wrapper :1206-1311).
// Cache layout [num_blocks, num_layers, block_size, Hkv, D]; token t of sequence b lives in physical
// block block_tables[b, t / block_size] at slot t % block_size (:728-751).
#include <cstdlib>

#include "mio_common.h"

#include "decode_plan.h"

// CPRP = chunks-per-row padded to a power of two (8 for D <= 64, 16 for D <= 128).  The body (decode_paged_body.inc) is shared
// with the sliding-window form decode_paged_win_kernel (WIN, `wleft` keys to the left): row qi of sequence b sees keys
// max(0, ctx - q_len + qi - wleft) .. ctx - 1, the splits cover [max(0, ctx - q_len - wleft), ctx) and each row (one per
// workgroup here) starts its walk at its own first key.  WIN = false compiles to the kernel as it was before the window.
template <typename T, int CPRP, int U>
__global__ __launch_bounds__(256) void decode_paged_kernel(const DecDev p) {
  constexpr bool WIN = false, KV8 = false;
  [[maybe_unused]] constexpr int wleft = 0;
  [[maybe_unused]] constexpr const float *ksc = nullptr, *vsc = nullptr;
#include "decode_paged_body.inc"
}

template <typename T, int CPRP, int U>
__global__ __launch_bounds__(256) void decode_paged_win_kernel(const DecDev p, int wleft) {
  constexpr bool WIN = true, KV8 = false;
  [[maybe_unused]] constexpr const float *ksc = nullptr, *vsc = nullptr;
#include "decode_paged_body.inc"
}

// ---- whole-token-row variant -------------------------------------------------------------------------------------------
// decode_paged_kernel reads 128- / 256-byte pieces (one head of one token) at the token stride Hkv * D * 2 bytes: every
// piece is a separate HBM burst in a random physical block, and the other heads' workgroups fetch the neighbouring pieces
// at other times (5.1-5.4 TB/s at B 64, H 16, D 64).  Here ONE workgroup owns a (sequence, context split) for ALL heads:
// a wave-load is 64 lanes x 16 B = 1 KiB of ONE token row (contiguous: the cache stores [token][Hkv][D]), a lane keeps the
// running softmax state of its own (kv head, 16-byte chunk) for the QN = (H / Hkv) * q_len query vectors that attend
// through that kv head, and consecutive tokens of a block are consecutive 2-KiB rows -- 32 KiB contiguous per block.
//   CPR  = chunks per head row (D / 8: 8 or 16)          CPT = Hkv * CPR chunks per token row (16 .. 256, power of two)
//   CPT >= 64: the row is NPART = CPT / 64 wave-loads; wave w takes part w % NPART of tokens (w / NPART) + k * (4 / NPART)
//   CPT <  64: one wave-load holds TPL = 64 / CPT tokens; wave w takes token slots 4 k + w
// Same clamped-address / masked-score loop as decode_paged_kernel, batches of U token slots, double-buffered.
// The body (decode_rows_body.inc) is shared with the sliding-window form decode_rows_win_kernel: splits as in
// decode_paged_win_kernel, and query q's keys below its own first key are masked per score.
template <typename T, int CPR, int QN>
__global__ __launch_bounds__(256) void decode_rows_kernel(const DecDev p) {
  constexpr bool WIN = false, KV8 = false;
  [[maybe_unused]] constexpr int wleft = 0;
  [[maybe_unused]] constexpr const float *ksc = nullptr, *vsc = nullptr;
#include "decode_rows_body.inc"
}

template <typename T, int CPR, int QN>
__global__ __launch_bounds__(256) void decode_rows_win_kernel(const DecDev p, int wleft) {
  constexpr bool WIN = true, KV8 = false;
  [[maybe_unused]] constexpr const float *ksc = nullptr, *vsc = nullptr;
#include "decode_rows_body.inc"
}

// wave-iterations per double-buffered batch: 2 (a sweep of 1 / 2 / 4 / 8 moved the kernel by <= 3 %, 8 slower; the
// diagnostic build keeps the sweep behind MIO_DEC_U, read once)
template <typename T, int CPRP>
static void dec_launch_u(const DecDev& p, dim3 grid, hipStream_t st) {
#ifdef MIO_DIAG
  static const int u = [] { const char* e = std::getenv("MIO_DEC_U"); return e ? std::atoi(e) : 2; }();
  switch (u) {
    case 1: hipLaunchKernelGGL((decode_paged_kernel<T, CPRP, 1>), grid, dim3(256), 0, st, p); return;
    case 4: hipLaunchKernelGGL((decode_paged_kernel<T, CPRP, 4>), grid, dim3(256), 0, st, p); return;
    case 8: hipLaunchKernelGGL((decode_paged_kernel<T, CPRP, 8>), grid, dim3(256), 0, st, p); return;
    default: break;
  }
#endif
  hipLaunchKernelGGL((decode_paged_kernel<T, CPRP, 2>), grid, dim3(256), 0, st, p);
}

extern "C" size_t mio_fa3_decode_workspace_bytes(int32_t B, int32_t H, int32_t q_len, int32_t D, int32_t max_ctx) {
  const int ns_a = dec_nsplit(B, H, q_len, max_ctx), ns_b = dec_nsplit_rows(B, max_ctx);
  const int ns_c = dec_nsplit_gqa(B, max_ctx, 1, 64);  // fewest units (Hkv 1), smallest block size, larger target: the largest split count
  int ns = ns_a > ns_b ? ns_a : ns_b;  // covers whichever kernel the launch picks (it does not know Hkv here)
  if (ns_c > ns) ns = ns_c;
  return (size_t)B * H * q_len * ns * (size_t)(D + 1) * sizeof(float) + 256;
}

// the launches of one route; wleft >= 0 takes the windowed form of its kernel
template <typename T>
static int dec_run(const DecDev& p, int route, int wleft, hipStream_t st) {
  const bool win = wleft >= 0;
  if (route == MIO_DEC_ROUTE_GQA) {
    int rc;
    if (p.D == 128) {
      rc = win ? dec_launch_gqa<decode_gqa_win_kernel<T, 128>, dg_smem_bytes<128>()>("decode_gqa_win", p, st, wleft)
               : dec_launch_gqa<decode_gqa_kernel<T, 128>, dg_smem_bytes<128>()>("decode_gqa", p, st);
    } else {
      rc = win ? dec_launch_gqa<decode_gqa_win_kernel<T, 64>, dg_smem_bytes<64>()>("decode_gqa_win", p, st, wleft)
               : dec_launch_gqa<decode_gqa_kernel<T, 64>, dg_smem_bytes<64>()>("decode_gqa", p, st);
    }
    if (rc != 0) return rc;
  } else if (route == MIO_DEC_ROUTE_ROWS) {  // one query vector per key (dec_rows_ok); QN stays a template parameter for sweeps
    const dim3 grid((unsigned)p.B, (unsigned)p.nsplit);
    if (p.D == 64) {
      if (win) hipLaunchKernelGGL((decode_rows_win_kernel<T, 8, 1>), grid, dim3(256), 0, st, p, wleft);
      else hipLaunchKernelGGL((decode_rows_kernel<T, 8, 1>), grid, dim3(256), 0, st, p);
    } else {
      if (win) hipLaunchKernelGGL((decode_rows_win_kernel<T, 16, 1>), grid, dim3(256), 0, st, p, wleft);
      else hipLaunchKernelGGL((decode_rows_kernel<T, 16, 1>), grid, dim3(256), 0, st, p);
    }
  } else {
    const dim3 grid((unsigned)((int64_t)p.B * p.H * p.q_len), (unsigned)p.nsplit);
    if (win) {
      if (p.D <= 64) hipLaunchKernelGGL((decode_paged_win_kernel<T, 8, 2>), grid, dim3(256), 0, st, p, wleft);
      else hipLaunchKernelGGL((decode_paged_win_kernel<T, 16, 2>), grid, dim3(256), 0, st, p, wleft);
    } else {
      if (p.D <= 64) dec_launch_u<T, 8>(p, grid, st);
      else dec_launch_u<T, 16>(p, grid, st);
    }
  }
  dec_merge<T>(p, st);
  return 0;
}

static int dec_forward(const std::string& fn, const void* q, void* o, const void* k_cache, const void* v_cache,
                       const int32_t* block_tables, const int32_t* context_lengths, const int64_t q_stride[3],
                       const int64_t o_stride[3], int32_t B, int32_t H, int32_t Hkv, int32_t q_len, int32_t D,
                       int32_t num_layers, int32_t layer_idx, int32_t block_size, int32_t max_blocks_per_seq,
                       int32_t max_ctx, float scale, int32_t dtype, int32_t wleft, void* workspace, void* stream) {
  DecDev p;
  int route = 0;
  const int rc = dec_plan(p, route, fn, 2, q, o, k_cache, v_cache, nullptr, nullptr, block_tables, context_lengths, q_stride,
                          o_stride, B, H, Hkv, q_len, D, num_layers, layer_idx, block_size, max_blocks_per_seq, max_ctx,
                          scale, dtype, wleft);
  if (rc != 0) return rc;
  if (dec_workspace(p, fn, workspace) != 0) return -1;
  hipStream_t st = (hipStream_t)stream;
  const int rl = (dtype == MIO_BF16) ? dec_run<__bf16>(p, route, wleft, st) : dec_run<_Float16>(p, route, wleft, st);
  if (rl != 0) return rl;
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mio_fail(std::string("decode_paged launch: ") + hipGetErrorString(e));
  return 0;
}

extern "C" int mio_fa3_decode_paged(const void* q, void* o, const void* k_cache, const void* v_cache,
                                    const int32_t* block_tables, const int32_t* context_lengths,
                                    const int64_t q_stride[3], const int64_t o_stride[3], int32_t B, int32_t H,
                                    int32_t Hkv, int32_t q_len, int32_t D, int32_t num_layers, int32_t layer_idx,
                                    int32_t block_size, int32_t max_blocks_per_seq, int32_t max_ctx, float scale,
                                    int32_t dtype, void* workspace, void* stream) {
  return dec_forward("mio_fa3_decode_paged", q, o, k_cache, v_cache, block_tables, context_lengths, q_stride, o_stride, B,
                     H, Hkv, q_len, D, num_layers, layer_idx, block_size, max_blocks_per_seq, max_ctx, scale, dtype, -1,
                     workspace, stream);
}

static int dec_window_check(const char* fn, int32_t window_left, int32_t window_right, int32_t q_len) {
  MIO_CHECK(window_left >= -1 && window_right >= -1, std::string(fn) + ": window values must be -1 (unbounded) or >= 0");
  MIO_CHECK(window_right == -1, std::string(fn) + ": decode takes no right window (window_right must be -1)");
  MIO_CHECK(window_left < 0 || q_len < (1 << 29), std::string(fn) + ": q_len must be below 2^29 under a window");
  return 0;
}

extern "C" int mio_fa3_decode_paged_window(const void* q, void* o, const void* k_cache, const void* v_cache,
                                           const int32_t* block_tables, const int32_t* context_lengths,
                                           const int64_t q_stride[3], const int64_t o_stride[3], int32_t B, int32_t H,
                                           int32_t Hkv, int32_t q_len, int32_t D, int32_t num_layers, int32_t layer_idx,
                                           int32_t block_size, int32_t max_blocks_per_seq, int32_t max_ctx, float scale,
                                           int32_t window_left, int32_t window_right, int32_t dtype, void* workspace,
                                           void* stream) {
  const char* fn = "mio_fa3_decode_paged_window";
  if (dec_window_check(fn, window_left, window_right, q_len) != 0) return -1;
  window_left = dec_window(window_left, max_ctx, q_len);
  if (window_left < 0)  // no window: exactly mio_fa3_decode_paged
    return mio_fa3_decode_paged(q, o, k_cache, v_cache, block_tables, context_lengths, q_stride, o_stride, B, H, Hkv,
                                q_len, D, num_layers, layer_idx, block_size, max_blocks_per_seq, max_ctx, scale, dtype,
                                workspace, stream);
  return dec_forward(fn, q, o, k_cache, v_cache, block_tables, context_lengths, q_stride, o_stride, B, H, Hkv, q_len, D,
                     num_layers, layer_idx, block_size, max_blocks_per_seq, max_ctx, scale, dtype, window_left, workspace,
                     stream);
}

extern "C" int mio_fa3_decode_window_route(const void* q, void* o, const void* k_cache, const void* v_cache,
                                           const int32_t* block_tables, const int32_t* context_lengths,
                                           const int64_t q_stride[3], const int64_t o_stride[3], int32_t B, int32_t H,
                                           int32_t Hkv, int32_t q_len, int32_t D, int32_t num_layers, int32_t layer_idx,
                                           int32_t block_size, int32_t max_blocks_per_seq, int32_t max_ctx, float scale,
                                           int32_t window_left, int32_t window_right, int32_t dtype, void* workspace,
                                           void* stream) {
  (void)workspace;
  (void)stream;
  const char* fn = "mio_fa3_decode_window_route";
  if (dec_window_check(fn, window_left, window_right, q_len) != 0) return -1;
  DecDev p;
  int route = 0;
  const int rc = dec_plan(p, route, fn, 2, q, o, k_cache, v_cache, nullptr, nullptr, block_tables, context_lengths, q_stride,
                          o_stride, B, H, Hkv, q_len, D, num_layers, layer_idx, block_size, max_blocks_per_seq, max_ctx,
                          scale, dtype, dec_window(window_left, max_ctx, q_len));
  return rc != 0 ? rc : route;
}

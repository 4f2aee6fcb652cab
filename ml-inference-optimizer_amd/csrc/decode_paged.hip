// Paged-KV decode attention + cache scatter for CDNA4 (gfx950).  HBM-bandwidth-bound: K/V rows go
// straight from global memory to VGPRs (16 B per lane), no LDS staging, split over the context so
// a small batch still fills 256 CUs; partial (o, lse) states are merged by a second tiny kernel.
//
// Replaces _paged_attention_fwd_kernel (reference kernels/triton/attention_kernels.py:628-808, wrapper
// :1206-1311) and _reshape_and_cache_kernel (:811-905, wrapper :1314-1407).
// Cache layout [num_blocks, num_layers, block_size, Hkv, D]; token t of sequence b lives in physical
// block block_tables[b, t / block_size] at slot t % block_size (:728-751).
#include <algorithm>
#include <cstdlib>
#include <mutex>

#include "mio_common.h"

#include "decode_plan.h"

// CPRP = chunks-per-row padded to a power of two (8 for D <= 64, 16 for D <= 128).  The body (decode_paged_body.inc) is shared
// with the sliding-window form decode_paged_win_kernel (WIN, `wleft` keys to the left): row qi of sequence b sees keys
// max(0, ctx - q_len + qi - wleft) .. ctx - 1, the splits cover [max(0, ctx - q_len - wleft), ctx) and each row (one per
// workgroup here) starts its walk at its own first key.  WIN = false compiles to the kernel as it was before the window.
template <typename T, int CPRP, int U>
__global__ __launch_bounds__(256) void decode_paged_kernel(const DecDev p) {
  constexpr bool WIN = false;
  [[maybe_unused]] constexpr int wleft = 0;
#include "decode_paged_body.inc"
}

template <typename T, int CPRP, int U>
__global__ __launch_bounds__(256) void decode_paged_win_kernel(const DecDev p, int wleft) {
  constexpr bool WIN = true;
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
  constexpr bool WIN = false;
  [[maybe_unused]] constexpr int wleft = 0;
#include "decode_rows_body.inc"
}

template <typename T, int CPR, int QN>
__global__ __launch_bounds__(256) void decode_rows_win_kernel(const DecDev p, int wleft) {
  constexpr bool WIN = true;
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

template <typename T>
static void dec_launch(const DecDev& p, dim3 grid, hipStream_t st) {
  if (p.D <= 64) dec_launch_u<T, 8>(p, grid, st);
  else dec_launch_u<T, 16>(p, grid, st);
  if (p.nsplit > 1) hipLaunchKernelGGL(decode_reduce_kernel<T>, dim3(grid.x), dim3(128), 0, st, p);
}

template <typename T>
static void dec_launch_rows(const DecDev& p, int qn, unsigned rows, hipStream_t st) {
  const dim3 grid((unsigned)p.B, (unsigned)p.nsplit);
#define MIO_DEC_ROWS(CPR_, QN_) hipLaunchKernelGGL((decode_rows_kernel<T, CPR_, QN_>), grid, dim3(256), 0, st, p)
  (void)qn;  // always 1 (dec_rows_ok); the kernel template keeps QN for the diagnostic sweeps
  if (p.D == 64) MIO_DEC_ROWS(8, 1);
  else MIO_DEC_ROWS(16, 1);
#undef MIO_DEC_ROWS
  if (p.nsplit > 1) hipLaunchKernelGGL(decode_reduce_kernel<T>, dim3(rows), dim3(128), 0, st, p);
}

template <typename T>
static int dec_launch_gqa(const DecDev& p, unsigned rows, hipStream_t st) {
  const dim3 grid((unsigned)(p.B * p.Hkv), (unsigned)p.nsplit);
  static std::once_flag once;
  static hipError_t ea = hipSuccess;
  std::call_once(once, [&] {
    ea = hipFuncSetAttribute((const void*)decode_gqa_kernel<T, 128>, hipFuncAttributeMaxDynamicSharedMemorySize, dg_smem_bytes<128>());
    if (ea == hipSuccess)
      ea = hipFuncSetAttribute((const void*)decode_gqa_kernel<T, 64>, hipFuncAttributeMaxDynamicSharedMemorySize, dg_smem_bytes<64>());
  });
  if (ea != hipSuccess) return mio_fail(std::string("decode_gqa: hipFuncSetAttribute: ") + hipGetErrorString(ea));
  if (p.D == 128) hipLaunchKernelGGL((decode_gqa_kernel<T, 128>), grid, dim3(256), dg_smem_bytes<128>(), st, p);
  else hipLaunchKernelGGL((decode_gqa_kernel<T, 64>), grid, dim3(256), dg_smem_bytes<64>(), st, p);
  if (p.nsplit > 1) hipLaunchKernelGGL(decode_reduce_kernel<T>, dim3(rows), dim3(128), 0, st, p);
  return 0;
}

extern "C" size_t mio_fa3_decode_workspace_bytes(int32_t B, int32_t H, int32_t q_len, int32_t D, int32_t max_ctx) {
  const int ns_a = dec_nsplit(B, H, q_len, max_ctx), ns_b = dec_nsplit_rows(B, max_ctx);
  const int ns_c = dec_nsplit_gqa(B, max_ctx, 1, 64);  // fewest units (Hkv 1), smallest block size, larger target: the largest split count
  int ns = ns_a > ns_b ? ns_a : ns_b;  // covers whichever kernel the launch picks (it does not know Hkv here)
  if (ns_c > ns) ns = ns_c;
  return (size_t)B * H * q_len * ns * (size_t)(D + 1) * sizeof(float) + 256;
}

// The checks, kernel choice and split geometry of a decode launch, shared by mio_fa3_decode_paged (wleft = -1), its windowed
// form and the host-only route query; fn prefixes the messages.  route: a mio_decode_route_t.  With a window the kernel
// heuristics and the split count see the span min(max_ctx, wleft + q_len) as the context length: no split lies past the
// window, and the split count is at most the one of max_ctx (every dec_nsplit* grows with the context length), so
// mio_fa3_decode_workspace_bytes(max_ctx) covers it.
static int dec_plan(DecDev& p, int& route, const std::string& fn, const void* q, void* o, const void* k_cache,
                    const void* v_cache, const int32_t* block_tables, const int32_t* context_lengths,
                    const int64_t q_stride[3], const int64_t o_stride[3], int32_t B, int32_t H, int32_t Hkv,
                    int32_t q_len, int32_t D, int32_t num_layers, int32_t layer_idx, int32_t block_size,
                    int32_t max_blocks_per_seq, int32_t max_ctx, float scale, int32_t dtype, int32_t wleft) {
  MIO_CHECK(q && o && k_cache && v_cache && block_tables && context_lengths, fn + ": null pointer");
  MIO_CHECK(B > 0 && H > 0 && Hkv > 0 && H % Hkv == 0 && q_len > 0, fn + ": bad sizes");
  MIO_CHECK(D >= 8 && D <= 128 && D % 8 == 0, fn + ": head_dim must be a multiple of 8 in [8,128]");
  MIO_CHECK(layer_idx >= 0 && layer_idx < num_layers, fn + ": layer_idx out of range");
  MIO_CHECK(block_size > 0 && max_blocks_per_seq > 0 && max_ctx >= 0, fn + ": bad cache geometry");
  MIO_CHECK(dtype == MIO_BF16 || dtype == MIO_FP16, fn + ": dtype must be bf16 or fp16");
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
  bool rows_kernel = dec_rows_ok(B, H, Hkv, q_len, D, span);
  bool gqa_kernel = dec_gqa_ok(B, H, Hkv, q_len, D, span, block_size, o_stride, o);
#ifdef MIO_DIAG
  if (mio_dbg_get(6) == 1) rows_kernel = gqa_kernel = false;  // A/B: the per-head kernel (tools/dbg/dec_rows_ab.py)
  if (mio_dbg_get(6) == 2) gqa_kernel = false;                // A/B: rows kernel where it applies
  if (mio_dbg_get(6) == 3)                                    // A/B: the matrix-core kernel for 1 .. 4 query vectors too
    gqa_kernel = (H / Hkv) * q_len <= 16 && (D == 64 || D == 128) && o_stride[0] % 8 == 0 && o_stride[1] % 8 == 0 &&
                 o_stride[2] % 8 == 0 && mio_aligned16(o);
#endif
  if (gqa_kernel) rows_kernel = false;
  route = gqa_kernel ? MIO_DEC_ROUTE_GQA : rows_kernel ? MIO_DEC_ROUTE_ROWS : MIO_DEC_ROUTE_HEAD;
  p.nsplit = gqa_kernel ? dec_nsplit_gqa((int64_t)B * Hkv, span, block_size, D)
                        : rows_kernel ? dec_nsplit_rows(B, span) : dec_nsplit(B, H, q_len, span);
  int sl = (span + p.nsplit - 1) / p.nsplit;
  const int gran = gqa_kernel ? 128 : 32;
  sl = (sl + gran - 1) / gran * gran;
  if (sl < gran) sl = gran;
  p.split_len = sl;
  return 0;
}

// the launches of one route; wleft >= 0 takes the windowed form of its kernel
template <typename T>
static int dec_run(const DecDev& p, int route, int wleft, hipStream_t st) {
  const int64_t rows = (int64_t)p.B * p.H * p.q_len;
  if (wleft < 0) {
    if (route == MIO_DEC_ROUTE_GQA) return dec_launch_gqa<T>(p, (unsigned)rows, st);
    if (route == MIO_DEC_ROUTE_ROWS) dec_launch_rows<T>(p, (p.H / p.Hkv) * p.q_len, (unsigned)rows, st);
    else dec_launch<T>(p, dim3((unsigned)rows, (unsigned)p.nsplit), st);
    return 0;
  }
  if (route == MIO_DEC_ROUTE_GQA) {
    static std::once_flag once;
    static hipError_t ea = hipSuccess;
    std::call_once(once, [&] {
      ea = hipFuncSetAttribute((const void*)decode_gqa_win_kernel<T, 128>, hipFuncAttributeMaxDynamicSharedMemorySize,
                               dg_smem_bytes<128>());
      if (ea == hipSuccess)
        ea = hipFuncSetAttribute((const void*)decode_gqa_win_kernel<T, 64>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                 dg_smem_bytes<64>());
    });
    if (ea != hipSuccess) return mio_fail(std::string("decode_gqa_win: hipFuncSetAttribute: ") + hipGetErrorString(ea));
    const dim3 grid((unsigned)(p.B * p.Hkv), (unsigned)p.nsplit);
    if (p.D == 128) hipLaunchKernelGGL((decode_gqa_win_kernel<T, 128>), grid, dim3(256), dg_smem_bytes<128>(), st, p, wleft);
    else hipLaunchKernelGGL((decode_gqa_win_kernel<T, 64>), grid, dim3(256), dg_smem_bytes<64>(), st, p, wleft);
  } else if (route == MIO_DEC_ROUTE_ROWS) {  // one query vector per key (dec_rows_ok)
    const dim3 grid((unsigned)p.B, (unsigned)p.nsplit);
    if (p.D == 64) hipLaunchKernelGGL((decode_rows_win_kernel<T, 8, 1>), grid, dim3(256), 0, st, p, wleft);
    else hipLaunchKernelGGL((decode_rows_win_kernel<T, 16, 1>), grid, dim3(256), 0, st, p, wleft);
  } else {
    const dim3 grid((unsigned)rows, (unsigned)p.nsplit);
    if (p.D <= 64) hipLaunchKernelGGL((decode_paged_win_kernel<T, 8, 2>), grid, dim3(256), 0, st, p, wleft);
    else hipLaunchKernelGGL((decode_paged_win_kernel<T, 16, 2>), grid, dim3(256), 0, st, p, wleft);
  }
  if (p.nsplit > 1) hipLaunchKernelGGL(decode_reduce_kernel<T>, dim3((unsigned)rows), dim3(128), 0, st, p);
  return 0;
}

static int dec_forward(const std::string& fn, const void* q, void* o, const void* k_cache, const void* v_cache,
                       const int32_t* block_tables, const int32_t* context_lengths, const int64_t q_stride[3],
                       const int64_t o_stride[3], int32_t B, int32_t H, int32_t Hkv, int32_t q_len, int32_t D,
                       int32_t num_layers, int32_t layer_idx, int32_t block_size, int32_t max_blocks_per_seq,
                       int32_t max_ctx, float scale, int32_t dtype, int32_t wleft, void* workspace, void* stream) {
  DecDev p;
  int route = 0;
  const int rc = dec_plan(p, route, fn, q, o, k_cache, v_cache, block_tables, context_lengths, q_stride, o_stride, B, H,
                          Hkv, q_len, D, num_layers, layer_idx, block_size, max_blocks_per_seq, max_ctx, scale, dtype, wleft);
  if (rc != 0) return rc;
  MIO_CHECK(p.nsplit == 1 || workspace != nullptr, fn + ": workspace required");
  const int64_t rows = (int64_t)B * H * q_len;
  p.ws_o = (float*)workspace;
  p.ws_lse = p.ws_o ? p.ws_o + rows * p.nsplit * D : nullptr;
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

static int dec_window_check(const char* fn, int32_t window_left, int32_t window_right) {
  MIO_CHECK(window_left >= -1 && window_right >= -1, std::string(fn) + ": window values must be -1 (unbounded) or >= 0");
  MIO_CHECK(window_right == -1, std::string(fn) + ": decode takes no right window (window_right must be -1)");
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
  if (dec_window_check(fn, window_left, window_right) != 0) return -1;
  MIO_CHECK(window_left < 0 || q_len < (1 << 29), std::string(fn) + ": q_len must be below 2^29 under a window");
  // a window no shorter than max_ctx + q_len is the unbounded one: clamped, so the kernels' bounds stay in int
  if (window_left >= 0) window_left = (int32_t)std::min<int64_t>(std::min<int64_t>(window_left, (int64_t)max_ctx + q_len), 1 << 29);
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
  if (dec_window_check(fn, window_left, window_right) != 0) return -1;
  MIO_CHECK(window_left < 0 || q_len < (1 << 29), std::string(fn) + ": q_len must be below 2^29 under a window");
  if (window_left >= 0) window_left = (int32_t)std::min<int64_t>(std::min<int64_t>(window_left, (int64_t)max_ctx + q_len), 1 << 29);
  DecDev p;
  int route = 0;
  const int rc = dec_plan(p, route, fn, q, o, k_cache, v_cache, block_tables, context_lengths, q_stride, o_stride, B, H,
                          Hkv, q_len, D, num_layers, layer_idx, block_size, max_blocks_per_seq, max_ctx, scale, dtype,
                          window_left);
  return rc != 0 ? rc : route;
}

// ---- reshape_and_cache: one workgroup per sequence, 16-byte chunks over (Hkv, D) --------------------
__global__ __launch_bounds__(256) void reshape_and_cache_kernel(const uint16_t* __restrict__ key,
                                                                const uint16_t* __restrict__ value,
                                                                uint16_t* __restrict__ kc, uint16_t* __restrict__ vc,
                                                                const int32_t* __restrict__ bt,
                                                                const int32_t* __restrict__ cl, int64_t ks_b,
                                                                int64_t ks_h, int64_t vs_b, int64_t vs_h, int Hkv,
                                                                int D, int L, int layer, int bs, int max_blocks) {
  const int b = blockIdx.x;
  const int pos = cl[b] - 1;  // write position (attention_kernels.py:858)
  if (pos < 0 || pos / bs >= max_blocks) return;  // empty sequence / context longer than the block table row: nothing written
  const int pb = bt[(int64_t)b * max_blocks + pos / bs];
  const int64_t tok_stride = (int64_t)Hkv * D;
  const int64_t dst = ((int64_t)pb * L + layer) * bs * tok_stride + (int64_t)(pos % bs) * tok_stride;
  const int cpr = D >> 3;
  for (int i = threadIdx.x; i < Hkv * cpr; i += 256) {
    const int hh = i / cpr, c = i % cpr;
    const u32x4_t kk = *(const u32x4_t*)(key + b * ks_b + hh * ks_h + 8 * c);
    const u32x4_t vv = *(const u32x4_t*)(value + b * vs_b + hh * vs_h + 8 * c);
    *(u32x4_t*)(kc + dst + (int64_t)hh * D + 8 * c) = kk;
    *(u32x4_t*)(vc + dst + (int64_t)hh * D + 8 * c) = vv;
  }
}

extern "C" int mio_reshape_and_cache(const void* key, const void* value, void* k_cache, void* v_cache,
                                     const int32_t* block_tables, const int32_t* context_lengths,
                                     const int64_t k_stride[2], const int64_t v_stride[2], int32_t B, int32_t Hkv,
                                     int32_t D, int32_t num_layers, int32_t layer_idx, int32_t block_size,
                                     int32_t max_blocks_per_seq, int32_t dtype, void* stream) {
  MIO_CHECK(key && value && k_cache && v_cache && block_tables && context_lengths, "mio_reshape_and_cache: null pointer");
  MIO_CHECK(B > 0 && Hkv > 0 && D >= 8 && D % 8 == 0, "mio_reshape_and_cache: bad sizes");
  MIO_CHECK(layer_idx >= 0 && layer_idx < num_layers && block_size > 0, "mio_reshape_and_cache: bad cache geometry");
  MIO_CHECK(dtype == MIO_BF16 || dtype == MIO_FP16, "mio_reshape_and_cache: dtype must be bf16 or fp16");
  MIO_CHECK(k_stride[0] % 8 == 0 && k_stride[1] % 8 == 0 && v_stride[0] % 8 == 0 && v_stride[1] % 8 == 0 &&
                mio_aligned16(key) && mio_aligned16(value) && mio_aligned16(k_cache) && mio_aligned16(v_cache),
            "mio_reshape_and_cache: 16-byte alignment");
  hipLaunchKernelGGL(reshape_and_cache_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream,
                     (const uint16_t*)key, (const uint16_t*)value, (uint16_t*)k_cache, (uint16_t*)v_cache,
                     block_tables, context_lengths, k_stride[0], k_stride[1], v_stride[0], v_stride[1], Hkv, D,
                     num_layers, layer_idx, block_size, max_blocks_per_seq);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mio_fail(std::string("reshape_and_cache launch: ") + hipGetErrorString(e));
  return 0;
}

// ---- reshape_and_cache_varlen: many new tokens per sequence; one thread per 16-byte chunk of K and of V ------------------
// Thread i of the grid owns chunk i % (Hkv * D / 8) of packed token i / (Hkv * D / 8).  The token's sequence is the last b
// with cu[b] <= token (binary search over the clamped offsets, then checked: a token outside its sequence's clamped range is
// skipped, so offsets that disagree with total_new write nothing out of place).
__global__ __launch_bounds__(256) void reshape_and_cache_varlen_kernel(
    const uint16_t* __restrict__ key, const uint16_t* __restrict__ value, uint16_t* __restrict__ kc,
    uint16_t* __restrict__ vc, const int32_t* __restrict__ bt, const int32_t* __restrict__ cu,
    const int32_t* __restrict__ cl, int64_t ks_t, int64_t ks_h, int64_t vs_t, int64_t vs_h, int B, int total, int Hkv, int D,
    int num_blocks, int L, int layer, int bs, int max_blocks) {
  const int cpr = D >> 3, cpt = Hkv * cpr;  // 16-byte chunks per head row / per token
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)total * cpt) return;
  const int t = (int)(i / cpt), c = (int)(i % cpt), hh = c / cpr, cc = c % cpr;
  auto cu_at = [&](int b) { const int x = cu[b]; return x < 0 ? 0 : (x > total ? total : x); };
  int lo = 0, hi = B;  // the sequence: last b in [0, B) with cu[b] <= t
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (cu_at(mid) <= t) lo = mid; else hi = mid;
  }
  const int b = lo, s0 = cu_at(b), s1e = cu_at(b + 1), s1 = s1e > s0 ? s1e : s0;
  if (t < s0 || t >= s1) return;
  const int pos = cl[b] - (s1 - s0) + (t - s0);
  if (pos < 0 || pos / bs >= max_blocks) return;  // before the sequence / past its block-table row
  const int pb = bt[(int64_t)b * max_blocks + pos / bs];
  if (pb < 0 || pb >= num_blocks) return;
  const int64_t tok_stride = (int64_t)Hkv * D;
  const int64_t dst = (((int64_t)pb * L + layer) * bs + pos % bs) * tok_stride + (int64_t)hh * D + 8 * cc;
  *(u32x4_t*)(kc + dst) = *(const u32x4_t*)(key + t * ks_t + hh * ks_h + 8 * cc);
  *(u32x4_t*)(vc + dst) = *(const u32x4_t*)(value + t * vs_t + hh * vs_h + 8 * cc);
}

extern "C" int mio_reshape_and_cache_varlen(const void* key, const void* value, void* k_cache, void* v_cache,
                                            const int32_t* block_tables, const int32_t* cu_seqlens_new,
                                            const int32_t* context_lengths, const int64_t k_stride[2],
                                            const int64_t v_stride[2], int32_t B, int32_t total_new, int32_t Hkv,
                                            int32_t D, int32_t num_blocks, int32_t num_layers, int32_t layer_idx,
                                            int32_t block_size, int32_t max_blocks_per_seq, int32_t dtype,
                                            void* stream) {
  MIO_CHECK(k_stride != nullptr && v_stride != nullptr, "mio_reshape_and_cache_varlen: null strides");
  MIO_CHECK(B >= 0 && total_new >= 0 && Hkv > 0 && D >= 8 && D % 8 == 0, "mio_reshape_and_cache_varlen: bad sizes");
  MIO_CHECK(num_blocks > 0 && num_layers > 0 && layer_idx >= 0 && layer_idx < num_layers && block_size > 0 &&
                max_blocks_per_seq > 0,
            "mio_reshape_and_cache_varlen: bad cache geometry");
  MIO_CHECK(dtype == MIO_BF16 || dtype == MIO_FP16, "mio_reshape_and_cache_varlen: dtype must be bf16 or fp16");
  if (B == 0 || total_new == 0) return 0;
  MIO_CHECK(key && value && k_cache && v_cache && block_tables && cu_seqlens_new && context_lengths,
            "mio_reshape_and_cache_varlen: null pointer");
  MIO_CHECK(k_stride[0] >= 0 && k_stride[1] >= 0 && v_stride[0] >= 0 && v_stride[1] >= 0 && k_stride[0] % 8 == 0 &&
                k_stride[1] % 8 == 0 && v_stride[0] % 8 == 0 && v_stride[1] % 8 == 0 && mio_aligned16(key) &&
                mio_aligned16(value) && mio_aligned16(k_cache) && mio_aligned16(v_cache),
            "mio_reshape_and_cache_varlen: 16-byte alignment");
  const int64_t blocks = ((int64_t)total_new * Hkv * (D / 8) + 255) / 256;
  MIO_CHECK(blocks <= 0x7fffffff, "mio_reshape_and_cache_varlen: too many tokens");
  hipLaunchKernelGGL(reshape_and_cache_varlen_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                     (const uint16_t*)key, (const uint16_t*)value, (uint16_t*)k_cache, (uint16_t*)v_cache, block_tables,
                     cu_seqlens_new, context_lengths, k_stride[0], k_stride[1], v_stride[0], v_stride[1], B, total_new,
                     Hkv, D, num_blocks, num_layers, layer_idx, block_size, max_blocks_per_seq);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mio_fail(std::string("reshape_and_cache_varlen launch: ") + hipGetErrorString(e));
  return 0;
}

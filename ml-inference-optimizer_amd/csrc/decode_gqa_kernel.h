// Paged decode for grouped-query attention on the matrix core (gfx950): the (H / Hkv) * q_len <= 16 query vectors that
// attend through one kv head are the 16 columns of v_mfma_f32_16x16x32 tiles, so a cached key / value element is fetched
// once and used by all of them in ONE instruction.  decode_rows_kernel / decode_paged_kernel spend ~240 vector instructions
// per 16-byte cache chunk at 8 queries per key (1.04 TB/s at H 32 / Hkv 4 / D 128); here the per-chunk work is 16 MFMAs and
// ~60 vector instructions per 32 keys, and the kernel is bound by HBM again.
//
// Same paged layout and semantics as decode_paged_kernel (reference attention_kernels.py:628-808): cache
// [num_blocks, num_layers, block_size, Hkv, D], token t of sequence b in block block_tables[b, t / block_size].
//
//   workgroup = (sequence b, kv head, context split), 4 waves; wave w owns the 32-key chunks w, w + 4, ... of the split and its
//   own online-softmax state; the four states are merged through LDS at the end, the splits by decode_reduce_kernel.
//   K and V of a chunk go global -> LDS by DMA (global_load_lds_dwordx4: no VGPRs, no compiler-visible vector loads, so
//   every s_waitcnt vmcnt in the loop is ours), two stages per wave: ~1.5 chunks (K + V: 16 KiB at D 128) in flight per wave.
//   The products are fa3_fwd5_kernel's swapped forms:
//     S^T tile (16 keys x 16 queries) = K (A: lane (r, g) = K[key r][32 ds + 8 g .. +7]) . Q^T (B: lane (c, g) = Q[c][same d]);
//       accumulator: query c on the lane, keys 4 g + i in registers i;
//     O^T (16 d x 16 queries) += V^T (A: two ds_read_b64_tr_b16 of 4 keys x 16 d from the row-major V image) . P^T (B: the
//       lane's own exp'd registers of key tiles 0 / 1: k = 8 g + j <-> key 4 g + j (j < 4), 16 + 4 g + j - 4 (j >= 4)).
//   LDS images carry an XOR swizzle applied on the DMA's per-lane SOURCE address (K: 16-byte chunk ^ row, V: 32-byte block
//   ^ row) so the fragment reads are bank-conflict free.
//   The block-table slice of the split is staged in LDS once (ds_read lookups: no vector-memory traffic beside the DMA).
#pragma once
#include "mio_common.h"

// the first key a windowed decode launch walks in sequence b: row 0's window start (ctx: the sequence's length)
__device__ __forceinline__ int dec_win_begin(int ctx, int q_len, int wleft) {
  const int lo = ctx - q_len - wleft;
  return lo > 0 ? lo : 0;
}

constexpr int DG_BT_MAX = 2048;  // block-table entries a split may span (8 KiB of LDS)
constexpr int DG_NST = 2;        // (K, V) stages per wave

// ESZ: bytes per cached element (2, or 1 for the fp8 cache: 72 KiB at D 128)
template <int D, int ESZ = 2>
constexpr int dg_smem_bytes() {
  return 4 * DG_NST * (2 * 32 * D * ESZ) + DG_BT_MAX * 4;
}

// The fp8 cache's LDS image (KV8): 32 rows x D bytes per 32-key half, 16-byte chunk `ch` of row r stored at chunk
// ch ^ dg_kv8_sw(r) (applied on the DMA's source address).  The swizzle makes both fragment reads conflict-free within each
// 32-lane half: the K read takes one chunk of 16 consecutive rows (keys 0-15 or 16-31), the V^T read one chunk of the 16
// rows 4g .. 4g+3, 16+4g .. 16+4g+3 for g in {0, 1} (or {2, 3}); with b the row's bits, sw = [b3^b4, b2, b1] (D 128, 8
// chunks, rows 2 apart share a 256-byte bank row) and [b3^b4, b2] (D 64, 4 chunks, rows 4 apart share it).
//   K fragment (A of S^T = K . Q^T): lane (c16, g) = K[key 16 kt + c16][32 ds + 8 g .. +7]: one ds_read_b64 + 4 conversions.
//   V^T fragment (A of O^T += V^T . P^T): lane (c16, g) = V[key(k)][16 dt + c16] for k = 8 g .. 8 g + 7, key(8 g + j) =
//   4 g + j (j < 4), 16 + 4 g + j - 4 (j >= 4): one ds_read_b64_tr_b8 (lane 2 q + p of a 16-lane group addresses row q's
//   bytes 8 p .. 8 p + 7; lane i receives byte i of the 8 rows) + 4 conversions.
template <int D>
__device__ __forceinline__ int dg_kv8_sw(int r) {
  const int x = ((r >> 3) ^ (r >> 4)) & 1;
  if constexpr (D == 128) return (x << 2) | ((r >> 1) & 3);
  else return (x << 1) | ((r >> 2) & 1);
}

// The body (decode_gqa_body.inc) is shared with the sliding-window form decode_gqa_win_kernel (WIN, `wleft` keys to the left):
// the splits cover [max(0, ctx - q_len - wleft), ctx) (the staged block-table slice starts with them), and query j's keys
// below ctx - q_len + j % q_len - wleft are masked like the split's tail.
template <typename T, int D>
__global__ __launch_bounds__(256) void decode_gqa_kernel(const DecDev p) {
  constexpr bool WIN = false, KV8 = false;
  [[maybe_unused]] constexpr int wleft = 0;
  [[maybe_unused]] constexpr const float *ksc = nullptr, *vsc = nullptr;
#include "decode_gqa_body.inc"
}

template <typename T, int D>
__global__ __launch_bounds__(256) void decode_gqa_win_kernel(const DecDev p, int wleft) {
  constexpr bool WIN = true, KV8 = false;
  [[maybe_unused]] constexpr const float *ksc = nullptr, *vsc = nullptr;
#include "decode_gqa_body.inc"
}

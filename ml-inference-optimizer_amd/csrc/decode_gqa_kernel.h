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

template <int D>
constexpr int dg_smem_bytes() {
  return 4 * DG_NST * (2 * 32 * D * 2) + DG_BT_MAX * 4;
}

// The body (decode_gqa_body.inc) is shared with the sliding-window form decode_gqa_win_kernel (WIN, `wleft` keys to the left):
// the splits cover [max(0, ctx - q_len - wleft), ctx) (the staged block-table slice starts with them), and query j's keys
// below ctx - q_len + j % q_len - wleft are masked like the split's tail.
template <typename T, int D>
__global__ __launch_bounds__(256) void decode_gqa_kernel(const DecDev p) {
  constexpr bool WIN = false;
  [[maybe_unused]] constexpr int wleft = 0;
#include "decode_gqa_body.inc"
}

template <typename T, int D>
__global__ __launch_bounds__(256) void decode_gqa_win_kernel(const DecDev p, int wleft) {
  constexpr bool WIN = true;
#include "decode_gqa_body.inc"
}

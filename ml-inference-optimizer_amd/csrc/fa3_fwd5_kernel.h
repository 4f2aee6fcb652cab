// FlashAttention forward, fifth structure: TWO waves per SIMD (8 waves x 32 query rows per workgroup, 256 registers per
// wave) on v_mfma_f32_16x16x32 tiles (head dim <= 64, no user mask).
//
// Why two waves: with ONE wave per SIMD (fa3_fwd3_kernel) every LDS read, DMA issue, scalar instruction, wait and barrier
// is issue time of the same stream that carries the softmax (timing-only ablations, tools/fa_ablate.py: with all softmax
// work, DMA, masks and the reference test removed a fwd3 tile at head dim 64 still takes 1.5 x its 1024 matrix-pipe
// cycles); with two, one wave's LDS / DMA / scalar / wait instructions issue beside the other wave's vector work.
// Why: the attention kernels are bound by the power cap, so what counts is energy per tile.
//   * On random operands the chip sustains ~1.2 x the FLOP/s on 16x16x32 that it does on 32x32x16 (tools/micro/
//     mfma_peak.hip: 1.88 vs 1.53 PFLOP/s, same cycles per FLOP, higher clock).
//   * The row sum "ones . P^T" is one MFMA per (16 queries, 32 keys): 4 of 36 MFMAs of 16 cycles per wave-tile instead of
//     4 of 20 of 32 cycles -- 1/9 of the matrix-pipe time instead of 1/5.
// The swapped product carries over to the 16x16 shape:
//   S^T tile (16 keys x 16 queries) = K tile (A: lane (r, g) = K[key 16 kt + r][d 32 ds + 8 g .. +7], one ds_read_b128)
//                                     . Q^T (B: lane (c, g) = Q[query 16 qg + c][d 32 ds + 8 g .. +7]); accumulator: query
//                                     c on the lane, keys 16 kt + 4 g + i in registers i = 0..3;
//   P^T as the B operand of O^T += V^T . P^T needs k = 8 g + j on lane group g: the exp'd registers of key tiles 2 s and
//     2 s + 1 ARE that fragment for the 32-key step s if k <-> key is read as j < 4: 32 s + 4 g + j, j >= 4: 32 s + 16 + 4 g
//     + (j - 4) -- the contraction order is free as long as the A operand uses the same map;
//   V^T tile (A: 16 d rows x 32 keys) in that map = two ds_read_b64_tr_b16 of 4 consecutive keys x 16 d from a ROW-MAJOR V
//     image (lane group g: keys 32 s (+16) + 4 g .., lane i of the group receives column d = 16 dt + i).
// LDS images (both filled by DMA, swizzle on the per-lane SOURCE address): K rows of 128 B with chunk c at c ^ ((row >> 1) &
// 7) (conflict-free ds_read_b128 for this lane -> (row, chunk) map); V rows of 128 B with the 32-byte block b
// at b ^ ((row >> 1) & 3) (the 8 rows of a half-wave's transposed read then cover 8 different 32-byte blocks of the 256-byte
// bank row).
//
// Software pipeline.  No LDS read sits in front of its consumer: the fragments are requested one half-iteration ahead, one
// per micro-step, so the eight waves' 128 KB of LDS reads per tile spread over the whole iteration instead of bursting behind
// the barrier (tools/fa5_stamps.py: with the reads at the head of their phase the second-dispatched waves waited 580 cycles
// for their first K fragment and the PV half ran at the LDS latency, 60 cycles per MFMA pair).
//   iteration t:  half 1: S(t+1) = K(t+1) fragments (registers) . Q^T - ref || P(t) = exp2(S(t)) || request V(t) fragments
//                 reference test (rare: move), edge masks of S(t+1)
//                 t even: wait for this wave's DMA shares, barrier (tiles <= t+3 visible), DMA of the next two tiles
//                 half 2: O^T += V(t) fragments . P(t), row sums || request K(t+2) fragments
// A K fragment dies in the step that a V fragment is born in and vice versa: ~36 fragment registers live.  Tiles t .. t+5
// are live or in flight: 8 LDS stages of 16 KB, ONE barrier per two tiles.  The KV tiles of both causal passes (same head)
// are one stream of "virtual" tiles: the heavy pass' last iterations request the light pass' first tiles.
#pragma once
#include "fa3_varlen.h"

constexpr int FA5_BM = 256;                  // query rows per workgroup (8 waves x 32)
constexpr int FA5_KBYTES = FA_BN * 128;      // K tile: 64 rows x 128 B, chunk c of row r at position c ^ ((r >> 1) & 7)
constexpr int FA5_STAGE = 2 * FA5_KBYTES;    // + V tile: 64 rows x 128 B, 32-byte block b of row r at b ^ ((r >> 1) & 3)

constexpr int FA5_STAGES = 8;
// Waves 4..7 (the second wave of each SIMD) meet the barrier BEFORE the QK^T half of an iteration, waves 0..3 behind it: the
// two waves of a SIMD then run opposite halves (vector-heavy QK^T || exp beside matrix-only PV) instead of queueing for the
// same unit
constexpr bool FA5_STAGGER = true;
constexpr int FA5_SMEM = FA5_STAGES * FA5_STAGE;

// KPRE (FaDev::k_prescaled): K arrives already multiplied by softmax_scale * log2(e) -- applied in fp32 in the epilogue of
// the GEMM that produced it, before its one rounding to 16 bits (ops.gemm_bias_act col_scale=; scaling a 16-bit K or Q
// afterwards would add a rounding and costs 3-5e-3 of lse accuracy).  Then the running reference enters the QK^T product
// as the MFMA's C operand (holding -reference: one query per lane), S = K~ . Q^T - reference is already the exp2 argument,
// and the scale / max pass over the scores is gone.  The rescale trigger moves behind the exp: the reference is kept
// Fa5Margin above the running maximum, so P <= 2^-margin normally, and "some P >= 2" (the row outgrew the maximum by
// 2^(margin + 1)) is bit 14 of a packed 16-bit word -- one v_or3_b32 per four values; the rare branch recomputes the
// tile's P from the still intact scores.
template <typename T>
struct Fa5Margin { static constexpr float value = 5.0f; };   // bf16: exponent range of fp32
template <>
struct Fa5Margin<_Float16> { static constexpr float value = 2.0f; };  // fp16: keep the small probabilities out of the subnormals

// CARRY: the ring form -- (o_acc fp32 [B, Sq, H, D], lse) carried in (p.carry_in) and written back; p.o may be null.
// OBLK: the 16-bit output goes to the GEMMs' blocked activation layout (FaDev::o_blk launches; not with CARRY).
// KPRE = false: K arrives as it is (the reference's functional entry point, triton_flash_attention(q, k, v)): the scores
// and the running reference stay in RAW units (q . k), the C operand subtracts the raw reference, and softmax_scale * log2(e)
// is applied in fp32 on the way into exp2 (one v_pk_mul per two scores: 16 vector instructions per wave-tile more than the
// pre-scaled form, no extra rounding of Q or K).
template <typename T, bool CAUSAL, bool STAMP = false, int ABL = 0, bool CARRY = false, bool OBLK = false, bool KPRE = true>  // ABL: timing-only ablations (diagnostic build)
__global__ __launch_bounds__(512) void fa3_fwd5_kernel(const FaDev p) {
#define FA_KV_TILE FA_KV_TILE_STRIDED
#define FA_LSE_INDEX(b, head, row) (((int64_t)(b) * p.H + (head)) * p.Sq + (row))
#include "fa3_fwd5_body.inc"
#undef FA_LSE_INDEX
#undef FA_KV_TILE
}

// packed variable-length form (mio_fa3_fwd_varlen, fa3_varlen.h), plain K and output: the dense body on this workgroup's
// sequence
template <typename T, bool CAUSAL>
__global__ __launch_bounds__(512) void fa3_fwd5_varlen_kernel(const FaDev pl, const FaVarlen vl) {
  constexpr bool STAMP = false, CARRY = false, OBLK = false, KPRE = false;
  constexpr int ABL = 0;
  FaDev p = pl;
  if (!fa_varlen_prepare<FA5_BM, 512, CAUSAL>(p, vl)) return;
#define FA_KV_TILE FA_KV_TILE_STRIDED
#define FA_LSE_INDEX(b, head, row) ((int64_t)(head) * vl.total_q + (row))
#include "fa3_fwd5_body.inc"
#undef FA_LSE_INDEX
#undef FA_KV_TILE
}

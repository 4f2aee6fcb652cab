// Variable-length (packed, cu_seqlens) form of the pipelined attention kernels (mio_fa3_fwd_varlen).
//
// q [total_q, H, D], k / v [total_k, Hkv, D], o [total_q, H, D]; sequence b owns rows cu_seqlens_q[b] .. cu_seqlens_q[b+1]-1
// of q / o and rows cu_seqlens_k[b] .. cu_seqlens_k[b+1]-1 of k / v.  The grid is the dense one of a [B, max_seqlen_q] batch
// (FaDev::qgrid / nqblk of max_seqlen_q, the same XCD remap); each workgroup reads its sequence's bounds and then runs the
// dense body with per-workgroup Sq = Lq, Sk = Lk, q_offset = Lk - Lq, k_offset = 0 (causal = bottom-right aligned, exactly a
// dense launch on that one sequence), its own block count for the causal heavy / light pairing, and row bases moved by
// q0 * q_stride_token in 64 bits.  lse is fp32 [H, total_q].
// The varlen kernels are the dense kernel bodies (fa3_fwd5_body.inc, fa3_fwd3_body.inc) run on a per-workgroup copy of FaDev
// that fa_varlen_prepare fills in: batch strides zero, the q / k / v / o / lse pointers at the sequence's first row.  The
// dense kernels compile exactly as before (their bodies are the same text, the varlen-only lines are discarded at compile
// time).
#pragma once
#include "fa3_fwd_kernel.h"

struct FaVarlen {
  const int32_t* cu_q;  // [B + 1] device
  const int32_t* cu_k;
  int total_q, total_k;
  int max_q, max_k;
};

template <typename P>
__device__ __forceinline__ P fa_sgpr(P x) {  // a wave-uniform pointer, made visibly so
  const uint64_t u = (uint64_t)x;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)u), hi = __builtin_amdgcn_readfirstlane((uint32_t)(u >> 32));
  return (P)(((uint64_t)hi << 32) | lo);
}

struct FaSeq {
  int q0, k0;  // first packed row of the sequence
  int Lq, Lk;  // its lengths
};

// The sequence of batch entry b, clamped so that nothing outside [0, total_q) / [0, total_k) is addressed and Lq <= max_q,
// Lk <= max_k whatever cu_seqlens holds (inconsistent offsets give wrong numbers, never an out-of-bounds access).  The
// values are wave-uniform (scalar registers): every wave of the workgroup takes the same exits.
__device__ __forceinline__ FaSeq fa_varlen_seq(const FaVarlen& v, int b) {
  auto clamp = [](int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); };
  FaSeq s;
  s.q0 = clamp(__builtin_amdgcn_readfirstlane(v.cu_q[b]), 0, v.total_q);
  const int q1 = clamp(__builtin_amdgcn_readfirstlane(v.cu_q[b + 1]), s.q0, v.total_q);
  s.k0 = clamp(__builtin_amdgcn_readfirstlane(v.cu_k[b]), 0, v.total_k);
  const int k1 = clamp(__builtin_amdgcn_readfirstlane(v.cu_k[b + 1]), s.k0, v.total_k);
  s.Lq = q1 - s.q0 < v.max_q ? q1 - s.q0 : v.max_q;
  s.Lk = k1 - s.k0 < v.max_k ? k1 - s.k0 : v.max_k;
  return s;
}

__device__ __forceinline__ FaSeq fa_seq_of(const FaVarlen& v, int b) { return fa_varlen_seq(v, b); }

// A sequence with no keys: o = 0 and lse = -inf for the rows of query blocks blk0 and blk1 (blk1 < 0: none) that lie below
// Lq.  No K / V load, no barrier -- the pipelined prologue fetches its
// first tile before it looks at the tile count.
template <int BM, int NT, typename V>
__device__ __forceinline__ void fa_varlen_write_empty(const FaDev& p, const V& v, const FaSeq& s, int head, int blk0,
                                                      int blk1) {
  // No lane-dependent branch: lanes past the rows store the same value to the sequence's last row (Lq >= 1 here).  A branch
  // on the lane makes the compiler treat what follows the join as divergent, and the pipelined body behind this needs its
  // tile addresses in scalar registers.
  const int dch = p.D >> 3;  // 16-byte chunks per row
  for (int k = 0; k < 2; ++k) {
    const int blk = k == 0 ? blk0 : blk1;
    if (blk < 0) continue;
    const int rows = s.Lq - blk * BM < BM ? s.Lq - blk * BM : BM;  // >= 1
    for (int i0 = 0; i0 < rows * dch; i0 += NT) {
      const int i = i0 + (int)threadIdx.x < rows * dch ? i0 + (int)threadIdx.x : rows * dch - 1;
      const int64_t row = s.q0 + blk * BM + i / dch;
      *(u32x4_t*)((char*)p.o + 2 * (row * p.os_s + head * p.os_h + 8 * (i % dch))) = (u32x4_t){0u, 0u, 0u, 0u};
    }
    if (p.lse != nullptr) {
      for (int i0 = 0; i0 < rows; i0 += NT) {
        const int i = i0 + (int)threadIdx.x < rows ? i0 + (int)threadIdx.x : rows - 1;
        p.lse[(int64_t)head * v.total_q + s.q0 + blk * BM + i] = -INFINITY;
      }
    }
  }
}

// Turns the launch's FaDev into this workgroup's dense problem (one sequence, p.B and the grid fields unchanged).  V is the
// launch's sequence description (FaVarlen, FaPaged in fa3_paged.h): fa_seq_of(v, b) gives batch entry b's FaSeq (clamped),
// v.total_q is the packed row count (the lse row stride); b_out receives the workgroup's batch entry.  Returns false when
// the workgroup has nothing (more) to do: no query block of its sequence, or a sequence without keys (its rows are written
// here).  Every wave of the workgroup takes the same exit.
template <int BM, int NT, bool CAUSAL, typename V>
__device__ __forceinline__ bool fa_seq_prepare(FaDev& p, const V& v, int& b_out) {
  int bh, qi;
  {  // the dense kernels' workgroup -> (batch, head, query block) map
    const int id = blockIdx.x;
    if (p.xcd_remap & 1) {
      const int xcd = id & 7, slot = id >> 3;
      bh = (slot / p.qgrid) * 8 + xcd;
      qi = slot % p.qgrid;
    } else {
      bh = id / p.qgrid;
      qi = id % p.qgrid;
    }
  }
  const int b = bh / p.H, head = bh % p.H;
  b_out = b;
  const FaSeq s = fa_seq_of(v, b);
  const int nqblk = (s.Lq + BM - 1) / BM;
  if (qi >= (CAUSAL ? (nqblk + 1) / 2 : nqblk)) return false;
  if (s.Lk == 0) {
    const int heavy = CAUSAL ? nqblk - 1 - qi : qi;
    fa_varlen_write_empty<BM, NT>(p, v, s, head, heavy, (CAUSAL && heavy != qi) ? qi : -1);
    return false;
  }
  // (the row bases go through readfirstlane: the body hands them to its DMA asm as scalar operands)
  p.q = fa_sgpr((const char*)p.q + 2 * (int64_t)s.q0 * p.qs_s);
  p.o = fa_sgpr((char*)p.o + 2 * (int64_t)s.q0 * p.os_s);
  p.k = fa_sgpr((const char*)p.k + 2 * (int64_t)s.k0 * p.ks_s);
  p.v = fa_sgpr((const char*)p.v + 2 * (int64_t)s.k0 * p.vs_s);
  if (p.lse != nullptr) p.lse = fa_sgpr(p.lse + s.q0);
  p.qs_b = p.ks_b = p.vs_b = p.os_b = 0;
  p.Sq = s.Lq;
  p.Sk = s.Lk;
  p.q_offset = s.Lk - s.Lq;  // bottom-right aligned causal mask
  p.k_offset = 0;
  p.nqblk = nqblk;
  return true;
}

template <int BM, int NT, bool CAUSAL>
__device__ __forceinline__ bool fa_varlen_prepare(FaDev& p, const FaVarlen& v) {
  int b;
  return fa_seq_prepare<BM, NT, CAUSAL>(p, v, b);
}

// Host launcher of the per-sequence forms for one (dtype, padded D) and sequence description V (FaVarlen, FaPaged in
// fa3_paged.h); defined per translation unit (fa3_seq_inst.hip).  p carries the launch's sizes, strides (batch strides
// unused) and pointers (paged: k / v are the caches, ks_s = vs_s = Hkv * D, ks_h = vs_h = D); the grid fields are set by
// the launcher.
template <typename T, int D, typename V>
int fa3_seq_launch(const FaDev& p, const V& seq, int causal, hipStream_t stream);

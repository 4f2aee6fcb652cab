// What the attention units fa3_{fwd,seq,win,kv8}_inst.hip share.  Each is one translation unit per (dtype, padded head dim),
// compiled with -DFA_TYPE_ID={0,1} -DFA_D={64,96,128}: the element type, the pipelined kernel's launch constants for this
// head dim (64: the fwd5 body, 96 / 128: the fwd3 body) and the one grid launcher.
#pragma once
#include "fa3_fwd3_kernel.h"
#if FA_D == 64
#include "fa3_fwd5_kernel.h"
#endif

#if FA_TYPE_ID == 0
using FaT = __bf16;
#else
using FaT = _Float16;
#endif

#if FA_D == 64
constexpr int FA_PIPE_BM = FA5_BM, FA_PIPE_NT = 512;
constexpr size_t FA_PIPE_SMEM = FA5_SMEM;
#else
constexpr int FA_PIPE_BM = FA3_BM, FA_PIPE_NT = 256;
constexpr size_t FA_PIPE_SMEM = FA3_STAGES * FaSmem<FA_D>::STAGE;
#endif
static_assert(FA_PIPE_SMEM <= 160 * 1024, "pipelined attention: LDS above 160 KiB per workgroup");

// The grid fields of a pipelined launch with max_q query rows per (batch, head) in blocks of BM; returns the workgroup
// count.  Causal: heavy / light pairing of the query blocks.  Per-sequence forms: the grid of a dense [B, max_seqlen_q]
// launch; workgroups past their own sequence's blocks leave at once.
template <bool CAUSAL>
static int64_t fa_grid(FaDev& p, int max_q, int BM) {
  p.nqblk = (max_q + BM - 1) / BM;
  p.qgrid = CAUSAL ? (p.nqblk + 1) / 2 : p.nqblk;
  return (int64_t)p.qgrid * p.B * p.H;
}

// One launch of this unit's pipelined kernel KERN(args...); p is the FaDev inside args, whose grid fields are set here.
template <auto KERN, bool CAUSAL, typename... A>
static int fa_grid_launch(const char* family, FaDev& p, int max_q, hipStream_t stream, const A&... args) {
  const int64_t grid = fa_grid<CAUSAL>(p, max_q, FA_PIPE_BM);
  if (grid > 0x7fffffff) return mio_fail(std::string(family) + ": grid too large");
  return fa_launch<KERN>(family, (unsigned)grid, FA_PIPE_NT, FA_PIPE_SMEM, stream, args...);
}

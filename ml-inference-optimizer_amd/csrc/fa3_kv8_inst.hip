// The paged attention forward over an fp8 (OCP e4m3fn) KV cache (mio_fa3_fwd_paged_kv8): the paged kernels of
// fa3_seq_inst.hip and their windowed forms of fa3_win_inst.hip with FA_KV8 defined.  One translation unit per (dtype,
// padded head dim), see fa3_inst.h.  Padded head dim 64: the fwd5 body; 96 / 128: the fwd3 body.
//
// K = x8 * k_scale, V = x8 * v_scale with the fp32 scales of the layer read here from device memory (no host sync: a scale
// may change between replays of a captured graph).  The bytes are widened exactly to 16 bits in LDS (fa3_fwd5_body.inc,
// fa3_fwd3_body.inc: FA_KV8, with kv8_cvt2 of kv8_cvt.h) and the MFMAs see x8 itself; k_scale joins softmax_scale *
// log2(e) in the fp32 score scale, v_scale the epilogue's 1 / l.  The per-lane strides of the bodies count 16-bit units
// (ks2 = 2 * ks_s bytes), so the paged plan (fa3_api.hip) gives the one-byte cache's strides halved.  No extra LDS: a
// wave's fp8 rows land inside the 16-bit image of the same rows, which that wave alone widens, so the stage sizes are
// those of the 16-bit kernels.
#include "fa3_inst.h"
#include "fa3_paged.h"
#include "kv8_cvt.h"

struct FaKv8Args {
  FaDev p;
  const float* k_scale;  // device: the layer's fp32 scales
  const float* v_scale;
  int left, right;       // window; -1 = unbounded (the plan clamps both to 2^29: fa3_api.hip, fa_plan_window)
};

#define FA_KV8 1
#define FA_LSE_INDEX(b, head, row) ((int64_t)(head) * pg.total_q + (row))

// ---- head dim <= 64: the fwd5 body
template <typename T, bool CAUSAL>
__global__ __launch_bounds__(512) void fa3_fwd5_paged_kv8_kernel(const FaKv8Args a, const FaPaged pg) {
  constexpr bool STAMP = false, CARRY = false, OBLK = false, KPRE = false;
  constexpr int ABL = 0;
  FaDev p = a.p;
  FaPageWalk walk;
  if (!fa_paged_prepare<FA5_BM, 512, CAUSAL>(p, pg, walk)) return;
  const float kv8_vs = fa_kv8_scales(p, a.k_scale, a.v_scale);
#define FA_KV_TILE FA_KV_TILE_PAGED
#include "fa3_fwd5_body.inc"
#undef FA_KV_TILE
}

#define FA_WINDOW 1
template <typename T, bool CAUSAL>
__global__ __launch_bounds__(512) void fa3_fwd5_paged_kv8_win_kernel(const FaKv8Args a, const FaPaged pg) {
  constexpr bool STAMP = false, CARRY = false, OBLK = false, KPRE = false;
  constexpr int ABL = 0;
  FaDev p = a.p;
  const int wl = a.left, wr = a.right;
  FaPageWalkWin walk;
  int bseq;
  if (!fa_seq_prepare<FA5_BM, 512, CAUSAL>(p, pg, bseq)) return;
  walk.row = (fa_cint32*)(pg.block_tables + (int64_t)bseq * pg.max_blocks);
  const float kv8_vs = fa_kv8_scales(p, a.k_scale, a.v_scale);
#define FA_KV_TILE FA_KV_TILE_PAGED_WIN
#define FA_WIN_PASS FA_WIN_PASS_PAGED
#include "fa3_fwd5_body.inc"
#undef FA_WIN_PASS
#undef FA_KV_TILE
}
#undef FA_WINDOW

// ---- head dims 96 / 128: the fwd3 body
template <typename T, int D, bool CAUSAL>
__global__ __launch_bounds__(256) void fa3_fwd3_paged_kv8_kernel(const FaKv8Args a, const FaPaged pg) {
  constexpr bool STAMP = false, KPRE = false;
  constexpr int ABL = 0;
  FaDev p = a.p;
  FaPageWalk walk;
  if (!fa_paged_prepare<FA3_BM, 256, CAUSAL>(p, pg, walk)) return;
  const float kv8_vs = fa_kv8_scales(p, a.k_scale, a.v_scale);
#define FA_KV_TILE FA_KV_TILE_PAGED
#include "fa3_fwd3_body.inc"
#undef FA_KV_TILE
}

#define FA_WINDOW 1
template <typename T, int D, bool CAUSAL>
__global__ __launch_bounds__(256) void fa3_fwd3_paged_kv8_win_kernel(const FaKv8Args a, const FaPaged pg) {
  constexpr bool STAMP = false, KPRE = false;
  constexpr int ABL = 0;
  FaDev p = a.p;
  const int wl = a.left, wr = a.right;
  FaPageWalkWin walk;
  int bseq;
  if (!fa_seq_prepare<FA3_BM, 256, CAUSAL>(p, pg, bseq)) return;
  walk.row = (fa_cint32*)(pg.block_tables + (int64_t)bseq * pg.max_blocks);
  const float kv8_vs = fa_kv8_scales(p, a.k_scale, a.v_scale);
#define FA_KV_TILE FA_KV_TILE_PAGED_WIN
#define FA_WIN_PASS FA_WIN_PASS_PAGED
#include "fa3_fwd3_body.inc"
#undef FA_WIN_PASS
#undef FA_KV_TILE
}
#undef FA_WINDOW
#undef FA_LSE_INDEX
#undef FA_KV8

// ---- launcher

template <bool WIN, bool CAUSAL>
constexpr auto kv8_kernel() {
#if FA_D == 64
  if constexpr (WIN) return fa3_fwd5_paged_kv8_win_kernel<FaT, CAUSAL>;
  else return fa3_fwd5_paged_kv8_kernel<FaT, CAUSAL>;
#else
  if constexpr (WIN) return fa3_fwd3_paged_kv8_win_kernel<FaT, FA_D, CAUSAL>;
  else return fa3_fwd3_paged_kv8_kernel<FaT, FA_D, CAUSAL>;
#endif
}

template <bool WIN, bool CAUSAL>
static int kv8_launch(FaKv8Args a, const FaPaged& pg, hipStream_t stream) {
  return fa_grid_launch<kv8_kernel<WIN, CAUSAL>(), CAUSAL>("fa3_fwd_paged_kv8", a.p, pg.max_q, stream, a, pg);
}

template <>
int fa3_kv8_launch<FaT, FA_D>(const FaDev& p, const FaPaged& pg, const float* k_scale, const float* v_scale, int causal,
                              int left, int right, hipStream_t stream) {
  const FaKv8Args a = {p, k_scale, v_scale, left, right};
  if (left == -1 && right == -1) return causal ? kv8_launch<false, true>(a, pg, stream) : kv8_launch<false, false>(a, pg, stream);
  return causal ? kv8_launch<true, true>(a, pg, stream) : kv8_launch<true, false>(a, pg, stream);
}

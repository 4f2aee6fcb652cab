// Sliding-window forms of the pipelined attention kernels (mio_fa3_fwd_window, mio_fa3_fwd_varlen_window,
// mio_fa3_fwd_paged_window).  One translation unit per (dtype, padded head dim), see fa3_inst.h.  Padded head dim 64:
// the fwd5 body; 96 / 128: the fwd3 body -- both with FA_WINDOW defined, so that each pass walks only the KV tiles of its
// rows' windows (fa3_fwd5_body.inc).  Plain K, plain output, no mask, no carry.  The window bounds travel beside FaDev
// (FaWinArgs), whose layout is unchanged.
#include <type_traits>

#include "fa3_inst.h"
#include "fa3_paged.h"

struct FaWinArgs {
  FaDev p;
  int left, right;  // -1 = unbounded; the plan (fa3_api.hip, fa_plan_window) clamps both to 2^29
};

#define FA_WINDOW 1
#define FA_WIN_PASS_NONE(t_lo, t_end, t_next, first) ((void)0)  // the dense and varlen kernels keep no page walk

// ---- head dim <= 64: the fwd5 body
template <typename T, bool CAUSAL>
__global__ __launch_bounds__(512) void fa3_fwd5_win_kernel(const FaWinArgs a) {
  constexpr bool STAMP = false, CARRY = false, OBLK = false, KPRE = false;
  constexpr int ABL = 0;
  const FaDev p = a.p;
  const int wl = a.left, wr = a.right;
#define FA_KV_TILE FA_KV_TILE_STRIDED
#define FA_WIN_PASS FA_WIN_PASS_NONE
#define FA_LSE_INDEX(b, head, row) (((int64_t)(b) * p.H + (head)) * p.Sq + (row))
#include "fa3_fwd5_body.inc"
#undef FA_LSE_INDEX
#undef FA_WIN_PASS
#undef FA_KV_TILE
}

template <typename T, bool CAUSAL>
__global__ __launch_bounds__(512) void fa3_fwd5_win_varlen_kernel(const FaWinArgs a, const FaVarlen vl) {
  constexpr bool STAMP = false, CARRY = false, OBLK = false, KPRE = false;
  constexpr int ABL = 0;
  FaDev p = a.p;
  const int wl = a.left, wr = a.right;
  if (!fa_varlen_prepare<FA5_BM, 512, CAUSAL>(p, vl)) return;
#define FA_KV_TILE FA_KV_TILE_STRIDED
#define FA_WIN_PASS FA_WIN_PASS_NONE
#define FA_LSE_INDEX(b, head, row) ((int64_t)(head) * vl.total_q + (row))
#include "fa3_fwd5_body.inc"
#undef FA_LSE_INDEX
#undef FA_WIN_PASS
#undef FA_KV_TILE
}

template <typename T, bool CAUSAL>
__global__ __launch_bounds__(512) void fa3_fwd5_win_paged_kernel(const FaWinArgs a, const FaPaged pg) {
  constexpr bool STAMP = false, CARRY = false, OBLK = false, KPRE = false;
  constexpr int ABL = 0;
  FaDev p = a.p;
  const int wl = a.left, wr = a.right;
  FaPageWalkWin walk;
  int bseq;
  if (!fa_seq_prepare<FA5_BM, 512, CAUSAL>(p, pg, bseq)) return;
  walk.row = (fa_cint32*)(pg.block_tables + (int64_t)bseq * pg.max_blocks);
#define FA_KV_TILE FA_KV_TILE_PAGED_WIN
#define FA_WIN_PASS FA_WIN_PASS_PAGED
#define FA_LSE_INDEX(b, head, row) ((int64_t)(head) * pg.total_q + (row))
#include "fa3_fwd5_body.inc"
#undef FA_LSE_INDEX
#undef FA_WIN_PASS
#undef FA_KV_TILE
}

// ---- head dims 96 / 128: the fwd3 body
template <typename T, int D, bool CAUSAL>
__global__ __launch_bounds__(256) void fa3_fwd3_win_kernel(const FaWinArgs a) {
  constexpr bool STAMP = false, KPRE = false;
  constexpr int ABL = 0;
  const FaDev p = a.p;
  const int wl = a.left, wr = a.right;
#define FA_KV_TILE FA_KV_TILE_STRIDED
#define FA_WIN_PASS FA_WIN_PASS_NONE
#define FA_LSE_INDEX(b, head, row) (((int64_t)(b) * p.H + (head)) * p.Sq + (row))
#include "fa3_fwd3_body.inc"
#undef FA_LSE_INDEX
#undef FA_WIN_PASS
#undef FA_KV_TILE
}

template <typename T, int D, bool CAUSAL>
__global__ __launch_bounds__(256) void fa3_fwd3_win_varlen_kernel(const FaWinArgs a, const FaVarlen vl) {
  constexpr bool STAMP = false, KPRE = false;
  constexpr int ABL = 0;
  FaDev p = a.p;
  const int wl = a.left, wr = a.right;
  if (!fa_varlen_prepare<FA3_BM, 256, CAUSAL>(p, vl)) return;
#define FA_KV_TILE FA_KV_TILE_STRIDED
#define FA_WIN_PASS FA_WIN_PASS_NONE
#define FA_LSE_INDEX(b, head, row) ((int64_t)(head) * vl.total_q + (row))
#include "fa3_fwd3_body.inc"
#undef FA_LSE_INDEX
#undef FA_WIN_PASS
#undef FA_KV_TILE
}

template <typename T, int D, bool CAUSAL>
__global__ __launch_bounds__(256) void fa3_fwd3_win_paged_kernel(const FaWinArgs a, const FaPaged pg) {
  constexpr bool STAMP = false, KPRE = false;
  constexpr int ABL = 0;
  FaDev p = a.p;
  const int wl = a.left, wr = a.right;
  FaPageWalkWin walk;
  int bseq;
  if (!fa_seq_prepare<FA3_BM, 256, CAUSAL>(p, pg, bseq)) return;
  walk.row = (fa_cint32*)(pg.block_tables + (int64_t)bseq * pg.max_blocks);
#define FA_KV_TILE FA_KV_TILE_PAGED_WIN
#define FA_WIN_PASS FA_WIN_PASS_PAGED
#define FA_LSE_INDEX(b, head, row) ((int64_t)(head) * pg.total_q + (row))
#include "fa3_fwd3_body.inc"
#undef FA_LSE_INDEX
#undef FA_WIN_PASS
#undef FA_KV_TILE
}

// ---- launchers

// the windowed kernel of this unit for (launch kind V: void = dense, FaVarlen, FaPaged; CAUSAL)
template <typename V, bool CAUSAL>
constexpr auto win_kernel() {
#if FA_D == 64
  if constexpr (std::is_same_v<V, void>) return fa3_fwd5_win_kernel<FaT, CAUSAL>;
  else if constexpr (std::is_same_v<V, FaVarlen>) return fa3_fwd5_win_varlen_kernel<FaT, CAUSAL>;
  else return fa3_fwd5_win_paged_kernel<FaT, CAUSAL>;
#else
  if constexpr (std::is_same_v<V, void>) return fa3_fwd3_win_kernel<FaT, FA_D, CAUSAL>;
  else if constexpr (std::is_same_v<V, FaVarlen>) return fa3_fwd3_win_varlen_kernel<FaT, FA_D, CAUSAL>;
  else return fa3_fwd3_win_paged_kernel<FaT, FA_D, CAUSAL>;
#endif
}

template <typename V, bool CAUSAL, typename... S>
static int win_launch(FaWinArgs a, int max_q, hipStream_t stream, const S&... seq) {
  const char* family = std::is_same_v<V, void> ? "fa3_fwd_window" : std::is_same_v<V, FaVarlen> ? "fa3_fwd_varlen_window"
                                                                                                  : "fa3_fwd_paged_window";
  return fa_grid_launch<win_kernel<V, CAUSAL>(), CAUSAL>(family, a.p, max_q, stream, a, seq...);
}

template <>
int fa3_win_launch<FaT, FA_D>(const FaDev& p, int causal, int left, int right, hipStream_t stream) {
  const FaWinArgs a = {p, left, right};
  return causal ? win_launch<void, true>(a, p.Sq, stream) : win_launch<void, false>(a, p.Sq, stream);
}

template <>
int fa3_win_seq_launch<FaT, FA_D>(const FaDev& p, const FaVarlen& s, int causal, int left, int right, hipStream_t stream) {
  const FaWinArgs a = {p, left, right};
  return causal ? win_launch<FaVarlen, true>(a, s.max_q, stream, s)
                : win_launch<FaVarlen, false>(a, s.max_q, stream, s);
}

template <>
int fa3_win_seq_launch<FaT, FA_D>(const FaDev& p, const FaPaged& s, int causal, int left, int right, hipStream_t stream) {
  const FaWinArgs a = {p, left, right};
  return causal ? win_launch<FaPaged, true>(a, s.max_q, stream, s) : win_launch<FaPaged, false>(a, s.max_q, stream, s);
}

// The one rule that picks the GEMM kernel for a launch, and the one tile predicate under it.  Host-only, no HIP.
// gemm_plan (gemm_api.hip) validates the arguments and asks the rule once, for the launches and for mio_gemm_route alike.  The diagnostic build's A/B overrides
// (MIO_GEMM_IMPL, mio_dbg_set) are applied by the launcher on top of this result, as variants of the route they replace.
#pragma once
#include <stdint.h>

#include "mio_hip.h"

struct GemmRouteArgs {
  int64_t M, ldx, ldw, ldy, ldr;  // row strides in elements (blocked operands: their row length)
  int32_t N, K, act;
  bool res;         // a residual is added in the epilogue
  int w_blk;        // weight layout: 0 row-major, 1 blocked (mio_weight_block), 2 gate / up interleaved (mio_weight_block_glu)
  bool ln_stats;    // LayerNorm consumer: the read-out applies the folded LayerNorm
  bool stats_out;   // LayerNorm producer: the read-out also writes the output rows' statistics
};

// The one tile predicate of the 16x16x32 kernels: the launch fills the chip with 256-row x BN-column tiles (>= 256 workgroups),
// K is whole K-tiles of 32 with at least four of them, and a row of K or N elements stays inside the 32-bit per-tile byte offsets
// (gemm_off32, which every row stride has to pass too).
static inline bool gemm_off32(int64_t ld) { return ld * 512 < (int64_t)0x7fffffff; }
static inline bool gemm_fills_chip(int64_t M, int32_t N, int BN) { return ((M + 255) / 256) * (int64_t)((N + BN - 1) / BN) >= 256; }
static inline bool gemm_tiles_ok(int64_t M, int32_t N, int32_t K, int BN) {
  return gemm_fills_chip(M, N, BN) && K % 32 == 0 && K >= 128 && gemm_off32(K) && gemm_off32(N);
}

static inline int gemm_pick_route(const GemmRouteArgs& a) {
  if (a.M == 0) return MIO_GEMM_ROUTE_EMPTY;
  if (a.act == MIO_ACT_SWIGLU) {
    if (a.w_blk == 2) return a.ln_stats ? MIO_GEMM_ROUTE_P8W_GLU_FOLD : MIO_GEMM_ROUTE_P8W_GLU;
    // big tiles (256 x 128) when they still fill the chip
    return gemm_fills_chip(a.M, a.N, 128) ? MIO_GEMM_ROUTE_GLU_T256X128 : MIO_GEMM_ROUTE_GLU_T128X64;
  }
  if (!gemm_fills_chip(a.M, a.N, 256)) return MIO_GEMM_ROUTE_T128;
  if (!(gemm_tiles_ok(a.M, a.N, a.K, 256) && gemm_off32(a.ldx) && gemm_off32(a.ldw) && gemm_off32(a.ldy) &&
        (!a.res || gemm_off32(a.ldr))))
    return MIO_GEMM_ROUTE_T256;
  // LayerNorm fold (mio_gemm_ln_bw checked the shape): consumer = projection behind the LayerNorm, producer = residual GEMM
  if (a.ln_stats && (a.act == MIO_ACT_NONE || a.act == MIO_ACT_GELU_TANH)) return MIO_GEMM_ROUTE_P8W_FOLD;
  if (a.stats_out && a.act == MIO_ACT_NONE) return MIO_GEMM_ROUTE_P8W_STATS;
  return a.res ? MIO_GEMM_ROUTE_P8W_RES : MIO_GEMM_ROUTE_P8W;
}

// The one rule that picks the GEMM kernel for a launch (mio_gemm_route / gemm_inst.hip launch_act).  Host-only, no HIP.
// The entry points of gemm_api.hip have validated the arguments before this runs.  The diagnostic build's A/B overrides
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

static inline int gemm_pick_route(const GemmRouteArgs& a) {
  if (a.M == 0) return MIO_GEMM_ROUTE_EMPTY;
  if (a.act == MIO_ACT_SWIGLU) {
    if (a.w_blk == 2) return a.ln_stats ? MIO_GEMM_ROUTE_P8W_GLU_FOLD : MIO_GEMM_ROUTE_P8W_GLU;
    // big tiles (256 x 128) when they still fill the chip (>= 256 workgroups)
    const int64_t big = ((a.M + 255) / 256) * ((a.N + 127) / 128);
    return big >= 256 ? MIO_GEMM_ROUTE_GLU_T256X128 : MIO_GEMM_ROUTE_GLU_T128X64;
  }
  const int64_t big = ((a.M + 255) / 256) * ((a.N + 255) / 256);
  if (big < 256) return MIO_GEMM_ROUTE_T128;
  // the 16x16x32 kernels address operands with 32-bit per-tile byte offsets and need whole K-tiles (>= 4 of them)
  const bool fits = (a.K % 32 == 0) && a.K >= 128 && (a.ldx * 512 < (int64_t)0x7fffffff) &&
                    (a.ldw * 512 < (int64_t)0x7fffffff) && (a.ldy * 512 < (int64_t)0x7fffffff) &&
                    (!a.res || a.ldr * 512 < (int64_t)0x7fffffff);
  if (!fits) return MIO_GEMM_ROUTE_T256;
  // LayerNorm fold (mio_gemm_ln_bw checked the shape): consumer = projection behind the LayerNorm, producer = residual GEMM
  if (a.ln_stats && (a.act == MIO_ACT_NONE || a.act == MIO_ACT_GELU_TANH)) return MIO_GEMM_ROUTE_P8W_FOLD;
  if (a.stats_out && a.act == MIO_ACT_NONE) return MIO_GEMM_ROUTE_P8W_STATS;
  return a.res ? MIO_GEMM_ROUTE_P8W_RES : MIO_GEMM_ROUTE_P8W;
}

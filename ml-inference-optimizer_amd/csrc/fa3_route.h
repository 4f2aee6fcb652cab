// The one rule that picks the attention-forward kernel for a launch (mio_fa3_route / fa3_launch).  Host-only, no HIP.
// mio_fa3_fwd has validated the arguments (and checked mio_fa3_k_prescaled_ok / mio_fa3_o_blocked_ok) before this runs.
// The diagnostic build's A/B overrides (MIO_FA_IMPL, mio_dbg_set) are applied by the launcher on top of this result.
#pragma once
#include <stdint.h>

#include "mio_hip.h"

struct Fa3RouteArgs {
  int dpad;            // padded head dim: 64 / 96 / 128
  int mask_kind;       // mio_mask_kind_t
  int Sq, Sk;
  int64_t ks_s, vs_s;  // K / V row strides in elements
  bool o, o_acc, carry_in, k_prescaled, o_blocked;
};

static inline int fa3_pick_route(const Fa3RouteArgs& a) {
  // K / V rows within 4 GiB of their (batch, head) base: the pipelined kernels address tiles with 32-bit byte offsets
  const bool span32 = (int64_t)a.Sk * a.ks_s * 2 < (1ll << 32) && (int64_t)a.Sk * a.vs_s * 2 < (1ll << 32);
  // Sk > 0: the pipelined kernels fetch their first K / V tile before they look at the tile count; fa3_fwd_kernel with
  // no key tiles issues no load and writes the empty (or carried) state
  const bool pipe = a.mask_kind == MIO_MASK_NONE && a.Sq > 128 && a.Sk > 0 && span32;
  const bool plain = pipe && a.o && !a.o_acc && !a.carry_in;
  if (a.dpad == 64) {
    if (a.k_prescaled && !plain && pipe && a.o_acc) return MIO_FA3_ROUTE_FWD5_KPRE_CARRY;
    if (a.k_prescaled && plain) return a.o_blocked ? MIO_FA3_ROUTE_FWD5_KPRE_OBLK : MIO_FA3_ROUTE_FWD5_KPRE;
    if (!a.k_prescaled && plain) return MIO_FA3_ROUTE_FWD5;
  }
  if (a.k_prescaled) {
    // not at 128: the two reference tuples of the KPRE form do not fit beside the score / P / fragment registers there
    if (a.dpad < 128 && plain) return MIO_FA3_ROUTE_FWD3_KPRE;
    return MIO_FA3_ROUTE_INVALID;
  }
  if (pipe) return MIO_FA3_ROUTE_FWD3;
  if (a.mask_kind == MIO_MASK_KEEP_U8) return MIO_FA3_ROUTE_FWD1_KEEP;
  if (a.mask_kind == MIO_MASK_ADD_F32) return MIO_FA3_ROUTE_FWD1_ADD;
  return MIO_FA3_ROUTE_FWD1;
}

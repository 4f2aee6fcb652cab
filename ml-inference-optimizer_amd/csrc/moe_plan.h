// The plan of the mixture-of-experts decode-step launches (moe.hip: mio_moe_route, mio_moe_up, mio_moe_down): shape checks, the
// split of K, the workspaces.  Host-only, no HIP, in the manner of gemm_skinny_plan.h, whose constants it shares: the launches and
// the host queries (mio_moe_up_splits, mio_moe_up_workspace_bytes, mio_moe_down_splits, mio_moe_down_workspace_bytes) all ask
// here.  A plan is a pure function of (T, k, E, N, K, act): the routing is device data and is never consulted, so a captured
// graph replays under any routing.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <string>

#include "gemm_skinny_plan.h"
#include "mio_hip.h"

constexpr int MOE_T_MAX = SKINNY_M_MAX;  // tokens of one launch: a token picks an expert at most once, so an expert has <= T rows
constexpr int MOE_E_MAX = 256;           // experts: the router's wave holds 4 logits per lane
constexpr int MOE_TOPK_MAX = 8;
constexpr SkinnyForm MOE_FORM = SKINNY_W16;  // the grouped GEMM runs the 16-bit decode-step GEMM's K loop: its step and chunks

// The 16-bit decode-step GEMM's plan at M = T: mf = ceil(T / 16) row fragments, the host's bound on an expert's rows, for which
// the kernel is built; tiles_n; steps; glu.  nsplit is this unit's own (moe_nsplit), and the slices are skinny_slice's.
struct MoePlan : SkinnyPlan {
  int rows;  // routed rows: T * k
};

// the experts the split aims at: how many are active is device data, so the most that can be
static inline int moe_experts_aimed(int64_t T, int32_t k, int32_t E) { return (int)std::max<int64_t>(1, std::min<int64_t>(E, T * k)); }

// Split rule.  Slices so that experts_aimed x tiles_n x nsplit reaches SKINNY_WGS workgroups, each slice at least
// 8 * rbar k long (whole steps), rbar = ceil(T k / experts_aimed) the rows per expert when the aimed experts share the routed rows
// evenly.  Reason: every routed row gets one fp32 partial row per slice whatever the routing, 4 T k N nsplit bytes in all,
// against 2 N K bytes of weight per active expert; at experts_aimed active experts the ratio is 2 rbar nsplit / K <= 2 rbar /
// min_len = 1/4, the bound the decode-step GEMM keeps with its 8 M.  A routing that leaves experts idle reads less weight for the
// same partials; the host cannot know, and the plan does not try to.  Slices are cut in steps, so with nsplit <= steps none is
// empty and two differ by one step at most; K / min_len grows with K at fixed (T, k, E, N), so the count never falls as K grows.
static inline int moe_min_slice(int64_t T, int32_t k, int32_t E) {
  const int aimed = moe_experts_aimed(T, k, E);
  const int64_t rbar = std::max<int64_t>(1, (T * k + aimed - 1) / aimed);
  const int kstep = MOE_FORM.kstep;
  return (int)std::max<int64_t>(kstep, (MOE_FORM.min_k_per_row * rbar + kstep - 1) / kstep * kstep);
}

static inline int moe_nsplit(int64_t T, int32_t k, int32_t E, int32_t N, int32_t K) {
  const int64_t wgs = (int64_t)moe_experts_aimed(T, k, E) * ((N + SKINNY_BN - 1) / SKINNY_BN);
  const int want = wgs > 0 ? (int)((SKINNY_WGS + wgs - 1) / wgs) : 1;
  return std::max(1, std::min(want, K / moe_min_slice(T, k, E)));
}

// the routing part of every entry point's checks; who prefixes the message
static inline bool moe_route_shape_ok(const char* who, int64_t T, int32_t k, int32_t E, std::string& err) {
  if (T < 0) err = ": T must not be negative";
  else if (T > MOE_T_MAX) err = ": T must be at most 64 (decode steps only; run taller batches in row chunks of 64)";
  else if (E < 1 || E > MOE_E_MAX) err = ": E must be in [1, 256]";
  else if (k < 1 || k > MOE_TOPK_MAX || k > E) err = ": top_k must be in [1, min(E, 8)]";
  else return true;
  err = who + err;
  return false;
}

// the shape part of a grouped GEMM's checks (N output columns, K the reduction), shared with the host queries
static inline bool moe_shape_ok(const char* who, int64_t T, int32_t k, int32_t E, int32_t N, int32_t K, int32_t act, std::string& err) {
  if (!moe_route_shape_ok(who, T, k, E, err)) return false;
  if (N < 0 || K < 0) err = ": sizes must not be negative";
  else if (K % 8 != 0) err = ": K must be a multiple of 8";
  else if (act < MIO_ACT_NONE || act > MIO_ACT_SWIGLU) err = ": unknown activation";
  else return true;
  err = who + err;
  return false;
}

static inline MoePlan moe_plan(int64_t T, int32_t k, int32_t E, int32_t N, int32_t K, int32_t act) {
  MoePlan pl;
  static_cast<SkinnyPlan&>(pl) = skinny_plan(MOE_FORM, T, N, K, act);
  pl.nsplit = moe_nsplit(T, k, E, N, K);
  pl.rows = (int)(T * k);
  return pl;
}

// up: fp32 partials [nsplit][T k][N] by sorted position (SwiGLU: the up half, then the gate half); none with one slice
static inline size_t moe_up_workspace_bytes(const MoePlan& pl, int32_t N) {
  return pl.nsplit == 1 ? 0 : (size_t)pl.nsplit * (size_t)pl.rows * (size_t)N * sizeof(float) * (pl.glu ? 2 : 1);
}

// down: always through fp32 partials [nsplit][T k][N]: the finishing launch is where the slots of a token meet
static inline size_t moe_down_workspace_bytes(const MoePlan& pl, int32_t N) {
  return (size_t)pl.nsplit * (size_t)pl.rows * (size_t)N * sizeof(float);
}

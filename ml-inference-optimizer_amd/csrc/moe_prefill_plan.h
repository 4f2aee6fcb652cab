// The plan of the mixture-of-experts launches for tall inputs (moe_prefill.hip: mio_moe_prefill_route, mio_moe_prefill_up,
// mio_moe_prefill_down): the tile, the bound on the tile map, the shape checks, the workspace.  Host-only, no HIP, in the manner
// of moe_plan.h, whose ranges of E and top_k it shares.  Everything here is a pure function of the sizes: the routing is device
// data and is never consulted, so a captured graph replays under any routing.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <string>

#include "moe_plan.h"

constexpr int MOE_PREFILL_T_MAX = 8192;  // tokens of one launch: routed rows <= 65536, int32 everywhere
constexpr int MOE_PF_BM = 128;           // sorted positions of one expert per tile
constexpr int MOE_PF_BN = 128;           // output columns per tile; SwiGLU: MOE_PF_BN_GLU up columns and their gate columns
constexpr int MOE_PF_BN_GLU = 64;
constexpr int MOE_PF_BK = 64;            // k per chunk: a tile row in LDS is 128 bytes, 8 pieces of 16
constexpr int MOE_PF_NT = 256;           // threads: four waves, 2 (rows) x 2 (columns), 64 x 64 of the tile each
// LDS: two buffers of an x tile and a weight tile, BM x BK and BN x BK 16-bit elements each: 64 KiB, two workgroups on a CU's 160
constexpr int MOE_PF_TILE_BYTES = MOE_PF_BM * MOE_PF_BK * 2;
constexpr int MOE_PF_LDS_BYTES = 2 * 2 * MOE_PF_TILE_BYTES;
static_assert(MOE_PF_BM == MOE_PF_BN && 2 * MOE_PF_BN_GLU == MOE_PF_BN, "one staging pattern for both operands; up and gate rows fill one weight tile");
static_assert(MOE_PF_LDS_BYTES <= 64 * 1024, "static LDS of one workgroup");

static inline int moe_prefill_bn(bool glu) { return glu ? MOE_PF_BN_GLU : MOE_PF_BN; }

// The bound on the tile map.  Expert e with c_e rows has ceil(c_e / BM) <= floor(c_e / BM) + 1 tiles, the + 1 only where c_e > 0;
// summed over the at most min(E, T k) experts with rows, and sum floor(c_e / BM) <= floor(T k / BM).
static inline int64_t moe_prefill_max_tiles(int64_t T, int32_t k, int32_t E) {
  return T * k / MOE_PF_BM + std::min<int64_t>(E, T * k);
}

// the routing part of every entry point's checks; who prefixes the message
static inline bool moe_prefill_route_shape_ok(const char* who, int64_t T, int32_t k, int32_t E, std::string& err) {
  if (T < 0) err = ": T must not be negative";
  else if (T > MOE_PREFILL_T_MAX) err = ": T must be at most 8192 (run taller inputs in row chunks of 8192)";
  else if (E < 1 || E > MOE_E_MAX) err = ": E must be in [1, 256]";
  else if (k < 1 || k > MOE_TOPK_MAX || k > E) err = ": top_k must be in [1, min(E, 8)]";
  else return true;
  err = who + err;
  return false;
}

// the shape part of a grouped GEMM's checks (N output columns, K the reduction), shared with the host query
static inline bool moe_prefill_shape_ok(const char* who, int64_t T, int32_t k, int32_t E, int32_t N, int32_t K, int32_t act,
                                        std::string& err) {
  if (!moe_prefill_route_shape_ok(who, T, k, E, err)) return false;
  if (N < 0 || K < 0) err = ": sizes must not be negative";
  else if (K % 8 != 0) err = ": K must be a multiple of 8";
  else if (act < MIO_ACT_NONE || act > MIO_ACT_SWIGLU) err = ": unknown activation";
  else return true;
  err = who + err;
  return false;
}

// The MXFP4 unit (moe_prefill_w4.hip): the same tile over e2m1 nibbles [E][N, K / 2] with one e8m0 scale byte per row and 32 k.  A
// chunk of a weight tile row is MOE_PF_W4_BLOCKS MX blocks, each 16 bytes of nibbles and one scale byte, and the tile's (row,
// block) pairs are one per thread.  The shape rule is the 16-bit one with whole MX blocks, under the decode form's words.
constexpr int MOE_PF_W4_BLOCKS = MOE_PF_BK / 32;
static_assert(MOE_PF_BN * MOE_PF_W4_BLOCKS == MOE_PF_NT, "MXFP4 weight staging: one (row, block) per thread");

static inline bool moe_prefill_w4_shape_ok(const char* who, int64_t T, int32_t k, int32_t E, int32_t N, int32_t K, int32_t act,
                                           std::string& err) {
  // (K rounded to 8: the 16-bit rule on K has nothing to say, the one below says it in the half-byte form's words)
  if (!moe_prefill_shape_ok(who, T, k, E, N, K - K % 8, act, err)) return false;
  if (K % SKINNY_W4.k_multiple == 0) return true;
  err = std::string(who) + SKINNY_W4.k_multiple_text;
  return false;
}

// down: fp32 rows [T k][N] by sorted position, the decode path's partials layout with one slice
static inline size_t moe_prefill_down_workspace_bytes(int64_t T, int32_t k, int32_t N) {
  return (size_t)(T * k) * (size_t)N * sizeof(float);
}

// The plan of the FP8 x FP8 GEMM for tall inputs (gemm_f8.hip: mio_gemm_f8, mio_gemm_f8_ok, mio_gemm_f8_route): the tile, the
// LDS budget, the shape checks, the tile count, the route names and the advice table.  Host-only, no HIP, in the manner of
// gemm_skinny_plan.h and moe_prefill_plan.h: the launch and the host queries read the same statements.
#pragma once
#include <stdint.h>

#include <string>

#include "mio_hip.h"

constexpr int F8_BM = 256;      // rows of x per workgroup
constexpr int F8_BN = 256;      // weight rows per workgroup: 256 output columns, SwiGLU 128 gate + 128 up rows of 128 columns
constexpr int F8_BN_GLU = 128;  // output columns of a SwiGLU tile
constexpr int F8_BK = 128;      // bytes of K per step: one v_mfma_f32_16x16x128_f8f6f4 deep
constexpr int F8_NT = 512;      // eight waves, 2 (rows) x 4 (weight rows): 128 x 64 of the tile each, 8 x 4 fragments of 16 x 16
// LDS: two stages of an x tile and a weight tile of F8_BK bytes a row; the third step is in flight in registers
constexpr int F8_TILE_BYTES = F8_BM * F8_BK;
constexpr int F8_STAGE_BYTES = 2 * F8_TILE_BYTES;
constexpr int F8_LDS_BYTES = 2 * F8_STAGE_BYTES;
static_assert(F8_BM == F8_BN && 2 * F8_BN_GLU == F8_BN, "one staging pattern for both operands; gate and up rows fill one weight tile");
static_assert(F8_TILE_BYTES / 16 % F8_NT == 0, "whole 16-byte chunks per thread");
static_assert(F8_LDS_BYTES <= 160 * 1024, "the CU's LDS");

static inline int f8_bn(bool glu) { return glu ? F8_BN_GLU : F8_BN; }

struct F8Plan {
  int64_t tiles_m;
  int tiles_n;
  int steps;  // K steps of F8_BK bytes, the last one possibly short (zero-filled in LDS, never read from memory)
  bool glu;
};

// The shape part of the launch's checks, shared with the host queries; who prefixes the message.
static inline bool f8_shape_ok(const char* who, int64_t M, int32_t N, int32_t K, int32_t act, std::string& err) {
  if (M < 0 || N < 0 || K < 0) err = ": M, N, K must not be negative";
  else if (K % 16 != 0) err = ": K must be a multiple of 16";
  else if (act < MIO_ACT_NONE || act > MIO_ACT_SWIGLU) err = ": unknown activation";
  else if (((M + F8_BM - 1) / F8_BM) * (int64_t)((N + f8_bn(act == MIO_ACT_SWIGLU) - 1) / f8_bn(act == MIO_ACT_SWIGLU)) > INT32_MAX)
    err = ": more than 2^31 - 1 output tiles";
  else return true;
  err = who + err;
  return false;
}

static inline F8Plan f8_plan(int64_t M, int32_t N, int32_t K, int32_t act) {
  F8Plan pl;
  pl.glu = act == MIO_ACT_SWIGLU;
  pl.tiles_m = (M + F8_BM - 1) / F8_BM;
  pl.tiles_n = (N + f8_bn(pl.glu) - 1) / f8_bn(pl.glu);
  pl.steps = (K + F8_BK - 1) / F8_BK;
  return pl;
}

// One workgroup per tile; the order of the tiles over the grid is gemm_tile_coords (gemm_kernel.h), as the 16-bit tiled kernel's.
static inline const char* f8_route_name(int64_t M, int32_t N, const F8Plan& pl) {
  if (M == 0 || N == 0) return "empty";
  return pl.glu ? "f8_glu_t256x128" : "f8_t256x256";
}

// The advice of mio_gemm_f8_ok: the shapes profiles/gemm_f8.md measured at most 0.9 x the time of ops.gemm_bias_act's route on the
// 16-bit weight WITH the activation quantiser's time included.  A shape that was not measured is not admitted.
struct F8Advised {
  int64_t M;
  int32_t N, K;
  bool glu;
};
constexpr F8Advised F8_ADVISED[] = {
    // quantiser + gemm_f8 over the 16-bit route (glu_t256x128); the four plain shapes measured lose (1.55 .. 2.06) and are not here
    {32768, 4096, 1024, true},  // 0.691
    {8192, 14336, 4096, true},  // 0.561
};

static inline bool f8_advised(int64_t M, int32_t N, int32_t K, int32_t act) {
  if (M <= 0 || N <= 0) return false;
  for (const F8Advised& a : F8_ADVISED)
    if (a.M == M && a.N == N && a.K == K && a.glu == (act == MIO_ACT_SWIGLU)) return true;
  return false;
}

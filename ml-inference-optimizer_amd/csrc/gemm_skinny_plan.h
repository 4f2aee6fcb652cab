// The plan of a decode-step GEMM launch (gemm_skinny.hip): shape checks, the split of K and the workspace, and the advice
// mio_gemm_skinny_ok gives the module layer.  Host-only, no HIP: the launch and the host queries (mio_gemm_skinny_splits,
// _workspace_bytes, _slice, _ok) all ask here, as the decode launches ask decode_plan.h.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <string>

#include "mio_hip.h"

constexpr int SKINNY_M_MAX = 64;   // 1 .. 4 row fragments of 16
constexpr int SKINNY_BN = 64;      // output columns per workgroup: 4 waves x one 16-row weight fragment
constexpr int SKINNY_KSTEP = 32;   // k per MFMA: every slice is whole steps (the last one ends at K)
// k per chunk of the kernel's double-buffered loop over a slice (mio_gemm_skinny_chunk_k): the weight registers of two chunks
// (this one, the next) are 64 VGPRs, so SwiGLU, with two weights, takes half the k
constexpr int SKINNY_CHUNK_K = 256;
constexpr int SKINNY_CHUNK_K_GLU = 128;
// workgroups the split aims for: two per CU.  tools/skinny_gemm_bench.py, profiles/skinny_gemm.md: the sweep ran with this value.
constexpr int SKINNY_WGS = 512;

struct SkinnyPlan {
  int mf;        // row fragments: ceil(M / 16)
  int tiles_n;   // ceil(N / SKINNY_BN)
  int steps;     // ceil(K / 32)
  int nsplit;    // slices of K; slice s covers steps [s * steps / nsplit, (s + 1) * steps / nsplit)
  bool glu;
};

// k range of slice s: whole 32-k steps, at most one step apart in length, the last one cut at K
static inline void skinny_slice(const SkinnyPlan& pl, int32_t K, int s, int32_t& kb, int32_t& ke) {
  kb = (int32_t)((int64_t)s * pl.steps / pl.nsplit) * SKINNY_KSTEP;
  ke = (int32_t)std::min<int64_t>(K, ((int64_t)(s + 1) * pl.steps / pl.nsplit) * SKINNY_KSTEP);
}

// Split rule.  Slices for SKINNY_WGS workgroups, each at least 8 * M elements (rounded up to whole steps): a slice's fp32
// partials are 4 M bytes per column against 2 * K_slice weight bytes, so the partials written stay at or under 1/4 of the weight
// bytes read (16 * M, 1/8, would leave M 64 at K 1024 in one slice: 48 workgroups for N 3072).  Both terms grow with K at fixed
// M, N, so the count never falls as K grows.
constexpr int SKINNY_MIN_K_PER_ROW = 8;
static inline int skinny_nsplit(int64_t M, int32_t N, int32_t K) {
  const int tiles_n = (N + SKINNY_BN - 1) / SKINNY_BN;
  const int min_len = std::max<int>(SKINNY_KSTEP, (int)((SKINNY_MIN_K_PER_ROW * M + SKINNY_KSTEP - 1) / SKINNY_KSTEP) * SKINNY_KSTEP);
  const int want = tiles_n > 0 ? (SKINNY_WGS + tiles_n - 1) / tiles_n : 1;
  return std::max(1, std::min(want, K / min_len));
}

// the shape part of a launch's checks, shared with the host queries; who prefixes the message
static inline bool skinny_shape_ok(const char* who, int64_t M, int32_t N, int32_t K, int32_t act, std::string& err) {
  if (M < 0 || N < 0 || K < 0) err = ": M, N, K must not be negative";
  else if (M > SKINNY_M_MAX) err = ": M must be at most 64 (mio_gemm_bias_act runs taller calls)";
  else if (K % 8 != 0) err = ": K must be a multiple of 8";
  else if (act < MIO_ACT_NONE || act > MIO_ACT_SWIGLU) err = ": unknown activation";
  else return true;
  err = who + err;
  return false;
}

static inline SkinnyPlan skinny_plan(int64_t M, int32_t N, int32_t K, int32_t act) {
  SkinnyPlan pl;
  pl.mf = (int)std::max<int64_t>(1, (M + 15) / 16);
  pl.tiles_n = (N + SKINNY_BN - 1) / SKINNY_BN;
  pl.steps = (K + SKINNY_KSTEP - 1) / SKINNY_KSTEP;
  pl.nsplit = skinny_nsplit(M, N, K);
  pl.glu = act == MIO_ACT_SWIGLU;
  return pl;
}

// fp32 partials [nsplit][M][N] (SwiGLU: the up half, then the gate half); none with one slice
static inline size_t skinny_workspace_bytes(const SkinnyPlan& pl, int64_t M, int32_t N) {
  return pl.nsplit == 1 ? 0 : (size_t)pl.nsplit * (size_t)M * (size_t)N * sizeof(float) * (pl.glu ? 2 : 1);
}

// Where the module layer should take this kernel: the regions of tools/skinny_gemm_bench.py's sweep in which both launches
// together ran in at most 0.9 x the time of mio_gemm_bias_act's route for the same call (profiles/skinny_gemm.md: bf16, weights
// streamed from HBM).  Plain activations: every M 1 .. 64 from the smallest weight measured up (N K >= 2^20: 0.45 - 0.86 x at
// 1024 x 1024, 0.14 - 0.18 x at 4096 x 14336).  SwiGLU (two weights, 128-k chunks): 0.78 - 0.82 x for M <= 16 at 14336 x 4096,
// the one shape measured, and 1.12 - 1.15 x at M 32 / 64 (three and four row fragments: 216 - 252 VGPRs, one wave per SIMD),
// so M <= 16 from that weight up.  Smaller weights than the sweep's were not measured and are not admitted.
static inline bool skinny_advised(int64_t M, int32_t N, int32_t K, int32_t act) {
  if (M < 1 || M > SKINNY_M_MAX || N < 1 || K < 8) return false;
  const int64_t nk = (int64_t)N * K;
  if (act == MIO_ACT_SWIGLU) return M <= 16 && nk >= (int64_t)14336 * 4096;
  return nk >= (int64_t)1 << 20;
}

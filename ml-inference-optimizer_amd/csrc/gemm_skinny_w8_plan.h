// The plan of a decode-step GEMM launch on e4m3fn weights (gemm_skinny_w8.hip): shape checks, the split of K, the workspace, the
// tuning values of the kernel's K loop and the advice mio_gemm_skinny_w8_ok gives the module layer.  Host-only, no HIP: the launch
// and the host queries (mio_gemm_skinny_w8_splits, _workspace_bytes, _slice, _chunk_k, _depth, _ok) all ask here, as the 16-bit
// unit asks gemm_skinny_plan.h, whose row fragments, column tiles and workgroup target it keeps.
#pragma once
#include "gemm_skinny_plan.h"

constexpr int SKW8_KSTEP = 64;  // k per 16-byte weight piece pair: one load feeds two MFMAs; every slice is whole steps
// k per chunk of the kernel's loop over a slice and the number of register sets in its ring (mio_gemm_skinny_w8_chunk_k /
// _depth).  A set holds one chunk of weight bytes per lane, 4 loads of 16 bytes at 256 k (SwiGLU: 2 weights x 2 loads at 128 k),
// and the x pieces of that chunk (up to 8 x 16 bytes at four row fragments), so depth - 1 chunks are in flight while one is
// multiplied: at depth 3 the 8 x 16 bytes of weight per lane the 16-bit kernel keeps outstanding.  The x chunk in LDS stays
// 2 x 64 rows x 512 B = 64 KiB at four row fragments, the static limit, so the chunk does not grow.  Tried on the sweep of
// tools/skinny_w8_bench.py (profiles/skinny_gemm_w8.md): plain depth 4 is within 1 % of depth 3 up to M 16 and slower at M 32 / 64
// (268 VGPRs at four row fragments: past 256, one wave per SIMD); SwiGLU depth 3 is within 2 % of depth 4.
constexpr int SKW8_CHUNK_K = 256;
constexpr int SKW8_CHUNK_K_GLU = 128;
constexpr int SKW8_DEPTH = 3;
constexpr int SKW8_DEPTH_GLU = 4;

struct SkinnyW8Plan {
  int mf;       // row fragments: ceil(M / 16)
  int tiles_n;  // ceil(N / SKINNY_BN)
  int steps;    // ceil(K / 64)
  int nsplit;   // slices of K; slice s covers steps [s * steps / nsplit, (s + 1) * steps / nsplit)
  bool glu;
};

// k range of slice s: whole 64-k steps, at most one step apart in length, the last one cut at K
static inline void skinny_w8_slice(const SkinnyW8Plan& pl, int32_t K, int s, int32_t& kb, int32_t& ke) {
  kb = (int32_t)((int64_t)s * pl.steps / pl.nsplit) * SKW8_KSTEP;
  ke = (int32_t)std::min<int64_t>(K, ((int64_t)(s + 1) * pl.steps / pl.nsplit) * SKW8_KSTEP);
}

// Split rule: skinny_nsplit's, for one-byte weights.  A slice's fp32 partials are 4 M bytes per column against K_slice weight
// bytes, so "partials at or under 1/4 of the weight bytes read" asks for slices of at least 16 M k, rounded up to whole steps.
// Slices are cut in steps, so with nsplit <= steps none is empty and two differ by one step at most; both terms of the minimum
// grow with K at fixed M, N, so the count never falls as K grows.
constexpr int SKW8_MIN_K_PER_ROW = 16;
static inline int skinny_w8_nsplit(int64_t M, int32_t N, int32_t K) {
  const int tiles_n = (N + SKINNY_BN - 1) / SKINNY_BN;
  const int min_len = std::max<int>(SKW8_KSTEP, (int)((SKW8_MIN_K_PER_ROW * M + SKW8_KSTEP - 1) / SKW8_KSTEP) * SKW8_KSTEP);
  const int want = tiles_n > 0 ? (SKINNY_WGS + tiles_n - 1) / tiles_n : 1;
  return std::max(1, std::min(want, K / min_len));
}

// the shape part of a launch's checks, shared with the host queries; who prefixes the message
static inline bool skinny_w8_shape_ok(const char* who, int64_t M, int32_t N, int32_t K, int32_t act, std::string& err) {
  if (M < 0 || N < 0 || K < 0) err = ": M, N, K must not be negative";
  else if (M > SKINNY_M_MAX) err = ": M must be at most 64 (fp8 weights are read by the decode-step kernel only)";
  else if (K % 16 != 0) err = ": K must be a multiple of 16";
  else if (act < MIO_ACT_NONE || act > MIO_ACT_SWIGLU) err = ": unknown activation";
  else return true;
  err = who + err;
  return false;
}

static inline SkinnyW8Plan skinny_w8_plan(int64_t M, int32_t N, int32_t K, int32_t act) {
  SkinnyW8Plan pl;
  pl.mf = (int)std::max<int64_t>(1, (M + 15) / 16);
  pl.tiles_n = (N + SKINNY_BN - 1) / SKINNY_BN;
  pl.steps = (K + SKW8_KSTEP - 1) / SKW8_KSTEP;
  pl.nsplit = skinny_w8_nsplit(M, N, K);
  pl.glu = act == MIO_ACT_SWIGLU;
  return pl;
}

// fp32 partials [nsplit][M][N] (SwiGLU: the up half, then the gate half); none with one slice
static inline size_t skinny_w8_workspace_bytes(const SkinnyW8Plan& pl, int64_t M, int32_t N) {
  return pl.nsplit == 1 ? 0 : (size_t)pl.nsplit * (size_t)M * (size_t)N * sizeof(float) * (pl.glu ? 2 : 1);
}

// Where the module layer should take this kernel: the regions of tools/skinny_w8_bench.py's sweep in which it ran in at most
// 0.9 x the time of the faster of mio_gemm_skinny and mio_gemm_bias_act on the 16-bit weight (profiles/skinny_gemm_w8.md: bf16,
// weights streamed from HBM).  Plain activations: every M 1 .. 64 from 6144 x 4096 weights up (0.78 - 0.85 x there, 0.66 - 0.80 x
// at 4096 x 14336), and M <= 16 from 4096 x 4096 up (0.82 - 0.86 x; M 32 / 64 ran 0.93 - 0.94 x there).  SwiGLU: every M from
// 14336 x 4096, the one shape measured, up (0.58 - 0.69 x).  Below 4096 x 4096 both kernels are two launches of about 10 us and
// the ratio (0.70 - 1.38 x) follows the two plans' split counts, not the weight's size: single (M, N, K) cells qualify, no region
// does, and none is admitted.  Nothing outside the shapes measured is admitted either.
static inline bool skinny_w8_advised(int64_t M, int32_t N, int32_t K, int32_t act) {
  if (M < 1 || M > SKINNY_M_MAX || N < 1 || K < 16) return false;
  const int64_t nk = (int64_t)N * K;
  if (act == MIO_ACT_SWIGLU) return nk >= (int64_t)14336 * 4096;
  if (nk >= (int64_t)6144 * 4096) return true;
  return M <= 16 && nk >= (int64_t)4096 * 4096;
}

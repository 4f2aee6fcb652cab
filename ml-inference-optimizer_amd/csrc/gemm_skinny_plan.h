// The plan of a decode-step GEMM launch, for both weight forms (gemm_skinny.hip: 16-bit weights; gemm_skinny_w8.hip: e4m3fn weights):
// shape checks, the split of K, the workspace, the tuning values of the kernels' K loops and the advice mio_gemm_skinny*_ok gives
// the module layer.  What differs between the forms is a SkinnyForm; everything else is written once and takes one.  Host-only,
// no HIP: the launches and the host queries (mio_gemm_skinny*_splits, _workspace_bytes, _slice, _chunk_k, _depth, _ok) all ask
// here, as the decode launches ask decode_plan.h.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <string>

#include "mio_hip.h"

// what a kernel calls as well: __host__ __device__ under a HIP compiler, nothing under a plain host compiler
#if defined(__HIP__) || defined(__HIPCC__)
#define SKINNY_HD __host__ __device__
#else
#define SKINNY_HD
#endif

constexpr int SKINNY_M_MAX = 64;   // 1 .. 4 row fragments of 16
constexpr int SKINNY_BN = 64;      // output columns per workgroup: 4 waves x one 16-row weight fragment
// workgroups the split aims for: two per CU.  tools/skinny_gemm_bench.py, profiles/skinny_gemm.md: the sweep ran with this value.
constexpr int SKINNY_WGS = 512;

// Where the module layer should take the 16-bit kernel: the regions of tools/skinny_gemm_bench.py's sweep in which both launches
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

// Where the module layer should take the fp8-weight kernel: the regions of tools/skinny_w8_bench.py's sweep in which it ran in at
// most 0.9 x the time of the faster of mio_gemm_skinny and mio_gemm_bias_act on the 16-bit weight (profiles/skinny_gemm_w8.md:
// bf16, weights streamed from HBM).  Plain activations: every M 1 .. 64 from 6144 x 4096 weights up (0.78 - 0.85 x there, 0.66 -
// 0.80 x at 4096 x 14336), and M <= 16 from 4096 x 4096 up (0.82 - 0.86 x; M 32 / 64 ran 0.93 - 0.94 x there).  SwiGLU: every M
// from 14336 x 4096, the one shape measured, up (0.58 - 0.69 x).  Below 4096 x 4096 both kernels are two launches of about 10 us
// and the ratio (0.70 - 1.38 x) follows the two plans' split counts, not the weight's size: single (M, N, K) cells qualify, no
// region does, and none is admitted.  Nothing outside the shapes measured is admitted either.
static inline bool skinny_w8_advised(int64_t M, int32_t N, int32_t K, int32_t act) {
  if (M < 1 || M > SKINNY_M_MAX || N < 1 || K < 16) return false;
  const int64_t nk = (int64_t)N * K;
  if (act == MIO_ACT_SWIGLU) return nk >= (int64_t)14336 * 4096;
  if (nk >= (int64_t)6144 * 4096) return true;
  return M <= 16 && nk >= (int64_t)4096 * 4096;
}

// A weight form: what the plan, the checks and the kernel's K loop of one unit read.
struct SkinnyForm {
  const char* name;   // the launch entry point; the queries are name_splits, name_workspace_bytes, ...
  bool scaled;        // the weights carry fp32 per-column scales (two more pointers in the call)
  int kstep;          // k per step of the kernel: every slice is whole steps (the last one ends at K)
  int k_multiple;     // K must be a multiple of this: the k of one 16-byte weight load
  int min_k_per_row;  // a slice is at least this many k per row of x (the split rule below)
  int ldw_multiple;   // ldw must be a multiple of this, in the unit ldw counts in: 16 bytes
  // k per chunk of the kernel's loop over a slice and the register sets the loop keeps (name_chunk_k / name_depth), plain and SwiGLU
  int chunk_k, chunk_k_glu;
  int depth, depth_glu;
  bool (*advised)(int64_t M, int32_t N, int32_t K, int32_t act);
  // the refusals that read differently for the two forms (the entry point's name goes in front)
  const char *m_max_text, *k_multiple_text, *dtype_text, *gate_text, *ldw_multiple_text, *ldw_short_text, *ld_multiple_text,
      *null_text;
  constexpr int chunk(bool glu) const { return glu ? chunk_k_glu : chunk_k; }
  constexpr int sets(bool glu) const { return glu ? depth_glu : depth; }
};

// 16-bit weights.  A step is one MFMA's 32 k.  The loop is double-buffered: the weight registers of two chunks (this one, the
// next) are 64 VGPRs, so SwiGLU, with two weights, takes half the k.
constexpr SkinnyForm SKINNY_W16 = {
    "mio_gemm_skinny", /*scaled*/ false, /*kstep*/ 32, /*k_multiple*/ 8, /*min_k_per_row*/ 8, /*ldw_multiple*/ 8,
    /*chunk_k*/ 256, 128, /*depth*/ 2, 2, skinny_advised,
    ": M must be at most 64 (mio_gemm_bias_act runs taller calls)", ": K must be a multiple of 8", ": dtype must be bf16 or fp16",
    ": w_gate is required iff act == SWIGLU", ": row strides must be multiples of 8 elements",
    ": row stride smaller than row length", ": row strides must be multiples of 8 elements", ": x, w, y must be non-null"};

// e4m3fn weights.  A step is the 64 k of a 16-byte weight piece per lane group: one load feeds two MFMAs.  A register set holds
// one chunk of weight bytes per lane, 4 loads of 16 bytes at 256 k (SwiGLU: 2 weights x 2 loads at 128 k), and the x pieces of
// that chunk (up to 8 x 16 bytes at four row fragments), so depth - 1 chunks are in flight while one is multiplied: at depth 3 the
// 8 x 16 bytes of weight per lane the 16-bit kernel keeps outstanding.  The x chunk in LDS stays 2 x 64 rows x 512 B = 64 KiB at
// four row fragments, the static limit, so the chunk does not grow.  Tried on the sweep of tools/skinny_w8_bench.py
// (profiles/skinny_gemm_w8.md): plain depth 4 is within 1 % of depth 3 up to M 16 and slower at M 32 / 64 (268 VGPRs at four row
// fragments: past 256, one wave per SIMD); SwiGLU depth 3 is within 2 % of depth 4.
constexpr SkinnyForm SKINNY_W8 = {
    "mio_gemm_skinny_w8", /*scaled*/ true, /*kstep*/ 64, /*k_multiple*/ 16, /*min_k_per_row*/ 16, /*ldw_multiple*/ 16,
    /*chunk_k*/ 256, 128, /*depth*/ 3, 4, skinny_w8_advised,
    ": M must be at most 64 (fp8 weights are read by the decode-step kernel only)", ": K must be a multiple of 16",
    ": dtype must be bf16 or fp16 (the activations'; the weights are e4m3fn bytes)",
    ": w8_gate and w_scale_gate are required together iff act == SWIGLU", ": ldw must be a multiple of 16 bytes",
    ": ldw smaller than K", ": ldx, ldy, ldr must be multiples of 8 elements", ": x, w8, w_scale, y must be non-null"};

struct SkinnyPlan {
  int mf;        // row fragments: ceil(M / 16)
  int tiles_n;   // ceil(N / SKINNY_BN)
  int steps;     // ceil(K / kstep)
  int nsplit;    // slices of K; slice s covers steps [s * steps / nsplit, (s + 1) * steps / nsplit)
  bool glu;
};

// k range of slice s of nsplit over `steps` steps of kstep: whole steps, at most one step apart in length, the last one cut at K.
// The one statement of it: the kernels of both forms and of the mixture-of-experts unit (moe.hip) call it, as do the hosts' slice
// queries.  (32-bit like steps itself: steps * kstep <= K + kstep - 1, which skinny_plan has formed as an int to get steps.)
SKINNY_HD inline void skinny_slice_range(int steps, int nsplit, int kstep, int32_t K, int s, int32_t& kb, int32_t& ke) {
  kb = (int32_t)((int64_t)s * steps / nsplit) * kstep;
  const int32_t end = (int32_t)((int64_t)(s + 1) * steps / nsplit) * kstep;
  ke = K < end ? K : end;
}
static inline void skinny_slice(const SkinnyForm& f, const SkinnyPlan& pl, int32_t K, int s, int32_t& kb, int32_t& ke) {
  skinny_slice_range(pl.steps, pl.nsplit, f.kstep, K, s, kb, ke);
}

// Split rule.  Slices for SKINNY_WGS workgroups, each at least min_k_per_row * M elements (rounded up to whole steps): a slice's
// fp32 partials are 4 M bytes per column against K_slice weight elements, so the partials written stay at or under 1/4 of the
// weight bytes read with 8 * M k of two-byte weights and with 16 * M k of one-byte weights (for two-byte weights 16 * M, 1/8,
// would leave M 64 at K 1024 in one slice: 48 workgroups for N 3072; profiles/skinny_gemm.md, profiles/skinny_gemm_w8.md).
// Slices are cut in steps, so with nsplit <= steps none is empty and two differ by one step at most; both terms of the minimum
// grow with K at fixed M, N, so the count never falls as K grows.
static inline int skinny_nsplit(const SkinnyForm& f, int64_t M, int32_t N, int32_t K) {
  const int tiles_n = (N + SKINNY_BN - 1) / SKINNY_BN;
  const int min_len = std::max<int>(f.kstep, (int)((f.min_k_per_row * M + f.kstep - 1) / f.kstep) * f.kstep);
  const int want = tiles_n > 0 ? (SKINNY_WGS + tiles_n - 1) / tiles_n : 1;
  return std::max(1, std::min(want, K / min_len));
}

// the shape part of a launch's checks, shared with the host queries; who prefixes the message
static inline bool skinny_shape_ok(const SkinnyForm& f, const char* who, int64_t M, int32_t N, int32_t K, int32_t act,
                                   std::string& err) {
  if (M < 0 || N < 0 || K < 0) err = ": M, N, K must not be negative";
  else if (M > SKINNY_M_MAX) err = f.m_max_text;
  else if (K % f.k_multiple != 0) err = f.k_multiple_text;
  else if (act < MIO_ACT_NONE || act > MIO_ACT_SWIGLU) err = ": unknown activation";
  else return true;
  err = who + err;
  return false;
}

static inline SkinnyPlan skinny_plan(const SkinnyForm& f, int64_t M, int32_t N, int32_t K, int32_t act) {
  SkinnyPlan pl;
  pl.mf = (int)std::max<int64_t>(1, (M + 15) / 16);
  pl.tiles_n = (N + SKINNY_BN - 1) / SKINNY_BN;
  pl.steps = (K + f.kstep - 1) / f.kstep;
  pl.nsplit = skinny_nsplit(f, M, N, K);
  pl.glu = act == MIO_ACT_SWIGLU;
  return pl;
}

// fp32 partials [nsplit][M][N] (SwiGLU: the up half, then the gate half); none with one slice
static inline size_t skinny_workspace_bytes(const SkinnyPlan& pl, int64_t M, int32_t N) {
  return pl.nsplit == 1 ? 0 : (size_t)pl.nsplit * (size_t)M * (size_t)N * sizeof(float) * (pl.glu ? 2 : 1);
}

// The plan of a decode-step GEMM launch, for the weight forms (gemm_skinny.hip: 16-bit weights; gemm_skinny_w8.hip: e4m3fn weights;
// gemm_skinny_w4.hip: MXFP4 weights):
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

// The refusals of the mixture-of-experts decode launches over stacked weights of a form (moe_gemm_common.h) that read differently
// for the two forms; the entry point's name goes in front.  The scale texts of a form without scales are never shown.
struct SkinnyMoeTexts {
  const char *ldw_multiple, *ld_multiple, *gate, *up_scale, *down_scale, *up_null, *down_null, *aligned;
};

// A weight form: what the plan, the checks and the kernel's K loop of one unit read.
struct SkinnyForm {
  const char* name;   // the launch entry point; the queries are name_splits, name_workspace_bytes, ...
  bool scaled;        // the weights carry fp32 per-column scales (two more pointers in the call)
  bool block_scaled;  // the weights carry e8m0 block-scale bytes [N, K / 32] (the same two pointers and a row stride), applied
                      // inside the K loop: nothing is left for the epilogue, which runs with scaled = false
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
  SkinnyMoeTexts moe;
  constexpr int chunk(bool glu) const { return glu ? chunk_k_glu : chunk_k; }
  constexpr int sets(bool glu) const { return glu ? depth_glu : depth; }
};

// 16-bit weights.  A step is one MFMA's 32 k.  The loop is double-buffered: the weight registers of two chunks (this one, the
// next) are 64 VGPRs, so SwiGLU, with two weights, takes half the k.
constexpr SkinnyForm SKINNY_W16 = {
    "mio_gemm_skinny", /*scaled*/ false, /*block_scaled*/ false, /*kstep*/ 32, /*k_multiple*/ 8, /*min_k_per_row*/ 8, /*ldw_multiple*/ 8,
    /*chunk_k*/ 256, 128, /*depth*/ 2, 2, skinny_advised,
    ": M must be at most 64 (mio_gemm_bias_act runs taller calls)", ": K must be a multiple of 8", ": dtype must be bf16 or fp16",
    ": w_gate is required iff act == SWIGLU", ": row strides must be multiples of 8 elements",
    ": row stride smaller than row length", ": row strides must be multiples of 8 elements", ": x, w, y must be non-null",
    {": row and expert strides must be multiples of 8 elements", ": row and expert strides must be multiples of 8 elements",
     ": w_gate is required iff act == SWIGLU", "", "", ": x, w_up, h, expert_offsets, sorted_rows must be non-null",
     ": h, w_down, y, ids, weights, expert_offsets, row_pos must be non-null",
     ": pointers must be 16-byte aligned (the route's arrays: 4-byte)"}};

// e4m3fn weights.  A step is the 64 k of a 16-byte weight piece per lane group: one load feeds two MFMAs.  A register set holds
// one chunk of weight bytes per lane, 4 loads of 16 bytes at 256 k (SwiGLU: 2 weights x 2 loads at 128 k), and the x pieces of
// that chunk (up to 8 x 16 bytes at four row fragments), so depth - 1 chunks are in flight while one is multiplied: at depth 3 the
// 8 x 16 bytes of weight per lane the 16-bit kernel keeps outstanding.  The x chunk in LDS stays 2 x 64 rows x 512 B = 64 KiB at
// four row fragments, the static limit, so the chunk does not grow.  Tried on the sweep of tools/skinny_w8_bench.py
// (profiles/skinny_gemm_w8.md): plain depth 4 is within 1 % of depth 3 up to M 16 and slower at M 32 / 64 (268 VGPRs at four row
// fragments: past 256, one wave per SIMD); SwiGLU depth 3 is within 2 % of depth 4.
constexpr SkinnyForm SKINNY_W8 = {
    "mio_gemm_skinny_w8", /*scaled*/ true, /*block_scaled*/ false, /*kstep*/ 64, /*k_multiple*/ 16, /*min_k_per_row*/ 16, /*ldw_multiple*/ 16,
    /*chunk_k*/ 256, 128, /*depth*/ 3, 4, skinny_w8_advised,
    ": M must be at most 64 (fp8 weights are read by the decode-step kernel only)", ": K must be a multiple of 16",
    ": dtype must be bf16 or fp16 (the activations'; the weights are e4m3fn bytes)",
    ": w8_gate and w_scale_gate are required together iff act == SWIGLU", ": ldw must be a multiple of 16 bytes",
    ": ldw smaller than K", ": ldx, ldy, ldr must be multiples of 8 elements", ": x, w8, w_scale, y must be non-null",
    {": ldw and expert_stride must be multiples of 16 bytes", ": activation row strides must be multiples of 8 elements",
     ": w8_gate and s_gate are required together iff act == SWIGLU", ": s_up (the fp32 scales [E, I]) must be non-null",
     ": s_down (the fp32 scales [E, d]) must be non-null", ": x, w8_up, h, expert_offsets, sorted_rows must be non-null",
     ": h, w8_down, y, ids, weights, expert_offsets, row_pos must be non-null",
     ": pointers must be 16-byte aligned (the scales and the route's arrays: 4-byte)"}};

// Where the module layer should take the MXFP4-weight kernel: the regions of tools/skinny_w4_bench.py's sweep in which it ran in at
// most 0.9 x the time of the faster of mio_gemm_skinny_w8 and mio_gemm_skinny on the same weight (profiles/skinny_gemm_w4.md: bf16,
// weights streamed from HBM).  SwiGLU: M <= 16 from 14336 x 4096, the one shape measured, up (0.80 x; M 64 ran 0.91 x).  Plain
// activations: 0.91 - 0.95 x for M <= 16 at 4096 x 4096, 6144 x 4096 and 4096 x 14336, and 1.00 - 1.36 x at M 64: no region
// qualifies, and none is admitted.  The SwiGLU region is open upwards from that size, any aspect ratio and every M 1 .. 16, as
// skinny_w8_advised's regions are; nothing below the sizes measured is admitted.
static inline bool skinny_w4_advised(int64_t M, int32_t N, int32_t K, int32_t act) {
  if (M < 1 || M > 16 || N < 1 || K < 32) return false;
  return act == MIO_ACT_SWIGLU && (int64_t)N * K >= (int64_t)14336 * 4096;
}

// MXFP4 weights: e2m1 nibbles, two per byte, with one e8m0 scale byte per 32 consecutive k.  A 16-byte weight load is one block of
// 32 k.  Slices are cut in steps of 128 k, four blocks, so that a slice's first scale byte sits on a dword of its row; a chunk is
// 256 k, in which lane group q owns the two consecutive blocks at 64 q: two weight loads and one 2-byte scale load per lane
// and chunk.  A register set holds 32 bytes of weight per lane (SwiGLU: 64), a quarter of the one-byte form's per k, so the ring is
// one set deeper than that form's plain ring at fewer registers; what fills a set is the x pieces (8 x 16 bytes at four row
// fragments).  The x chunk in LDS is 2 x 64 rows x 512 B = 64 KiB at four row fragments, the static limit, so the chunk does not
// grow to the 512 k at which a scale dword would ride with four weight loads.  Tried on the sweeps of tools/skinny_w4_bench.py and
// tools/moe_w4_bench.py (profiles/skinny_gemm_w4.md, profiles/moe_w4.md) at depth 3 / 4 / 5 plain and 4 / 3 / 2 SwiGLU: plain depth 5
// is 2 - 13 % faster for M <= 16 and 1.2 - 1.6 x slower at M 64 (past 256 VGPRs at four row fragments), depth 3 is within 3 % of
// depth 4; SwiGLU depth 4 is slower, depth 2 equal up to M 16 and faster at M 64, but measured only next to plain depth 5, a pair
// that loses on the MoE step at T 64.  At depth 4 / 3 the dense kernel reaches 0.8 - 2.4 TB/s of half-byte weight (the grouped
// one 0.5 - 3.3 TB/s, profiles/moe_w4.md), so the conversions and the x traffic bound it, not HBM.
constexpr SkinnyForm SKINNY_W4 = {
    "mio_gemm_skinny_w4", /*scaled*/ false, /*block_scaled*/ true, /*kstep*/ 128, /*k_multiple*/ 32, /*min_k_per_row*/ 32,
    /*ldw_multiple*/ 16, /*chunk_k*/ 256, 256, /*depth*/ 4, 3, skinny_w4_advised,
    ": M must be at most 64 (MXFP4 weights are read by the decode-step kernel only)",
    ": K must be a multiple of 32 (whole MX blocks)",
    ": dtype must be bf16 (e2m1 x 2^e is exact in bf16; in fp16 only inside a narrow exponent range)",
    ": w4_gate and w_scale_gate are required together iff act == SWIGLU", ": ldw must be a multiple of 16 bytes",
    ": ldw smaller than K / 2 bytes", ": ldx, ldy, ldr must be multiples of 8 elements", ": x, w4, w_scale, y must be non-null",
    {": ldw and expert_stride must be multiples of 16 bytes", ": activation row strides must be multiples of 8 elements",
     ": w4_gate and s_gate are required together iff act == SWIGLU", ": s_up (the e8m0 block scales [E, I, d / 32]) must be non-null",
     ": s_down (the e8m0 block scales [E, d, I / 32]) must be non-null", ": x, w4_up, h, expert_offsets, sorted_rows must be non-null",
     ": h, w4_down, y, ids, weights, expert_offsets, row_pos must be non-null",
     ": pointers must be 16-byte aligned (the block scales and the route's arrays: 4-byte)"}};

// bytes of a weight row's K elements in the form's storage, in the unit ldw counts in
static inline int64_t skinny_row_units(const SkinnyForm& f, int32_t K) { return f.block_scaled ? K / 2 : K; }
// the block-scale operands of a block-scaled form: row (and expert) strides in bytes, multiples of 4, a row at least K / 32
static inline bool skinny_lds_ok(int64_t lds, int32_t K) { return lds % 4 == 0 && lds >= K / 32; }

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

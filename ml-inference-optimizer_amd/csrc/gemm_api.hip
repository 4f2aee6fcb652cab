// C-ABI entry points mio_gemm_bias_act / mio_fused_mlp_fwd (see include/mio_hip.h).
#include <cstdlib>
#include <string>

#include "gemm_kernel.h"
#include "gemm_route.h"

extern template int gemm_launch<__bf16>(GemmDev, int, int, hipStream_t);
extern template int gemm_launch<_Float16>(GemmDev, int, int, hipStream_t);

// Diagnostic build only: MIO_GEMM_IMPL=v1|8w1 forces one pipeline for A/B comparisons (read once).  The product
// library always takes the default dispatch (0) and reads no environment variable.
int mio_gemm_impl() {
#ifdef MIO_DIAG
  if (mio_dbg_get(4) != 0) return mio_dbg_get(4);  // run-time override for same-process A/B (tools/gemm8_ab.py)
  static const int v = [] {
    const char* e = std::getenv("MIO_GEMM_IMPL");
    if (e == nullptr) return 0;
    const std::string s(e);
    if (s == "v1") return 1;
    if (s == "8w1") return 9;   // gemm8w_kernel, one workgroup per tile
    return 0;
  }();
  return v;
#else
  return 0;
#endif
}

// ---- shape queries: which launches take the 256-tile kernels (gemm_route.h gemm_tiles_ok) ---------------------------------------
static bool gemm_blocked_w_ok(int64_t M, int32_t N, int32_t K, int32_t act) {
  return act != MIO_ACT_SWIGLU && mio_gemm_impl() != 1 && gemm_tiles_ok(M, N, K, 256);
}

extern "C" int32_t mio_gemm_blocked_weight_ok(int64_t M, int32_t N, int32_t K, int32_t act) {
  return gemm_blocked_w_ok(M, N, K, act) ? 1 : 0;
}

// column scale: the launch must end in the persistent kernel (gemm_inst.hip launch_act): blocked weight shape, no residual,
// K >= 256, K % 64 == 0
extern "C" int32_t mio_gemm_col_scale_ok(int64_t M, int32_t N, int32_t K, int32_t act) {
  return (gemm_blocked_w_ok(M, N, K, act) && K >= 256 && K % 64 == 0 && N % 8 == 0) ? 1 : 0;
}

// Both GEMMs of the MLP take a 256x256-tile 16x16x32 kernel (gemm_inst.hip launch_act) and stage 1 the persistent one:
// then the intermediate can use the blocked layout (GemmDev::x_blk / y_blk).
// (SwiGLU: stage 1 computes 256 x 128 output tiles from 256 interleaved gate / up weight rows, gemm8w_kernel.h)
static bool mlp_blocked_ok(int64_t M, int32_t d, int32_t I) {
  return mio_gemm_impl() != 1 && gemm_tiles_ok(M, I, d, 256) && gemm_tiles_ok(M, d, I, 256) && d % 64 == 0 && d >= 256 &&
         I % 256 == 0;
}

extern "C" int32_t mio_fused_mlp_blocked_weight_ok(int64_t M, int32_t d, int32_t I, int32_t act) {
  (void)act;
  return (M > 0 && mlp_blocked_ok(M, d, I)) ? 1 : 0;
}

// the longest weight rows mio_ln_fold_weight prepares (ln_fold_weight_kernel: 256 threads x 32 elements), so the widest stream a
// consumer (fold_in) takes
constexpr int32_t GEMM_LN_FOLD_K_MAX = 8192;

extern "C" int32_t mio_gemm_ln_ok(int64_t M, int32_t N, int32_t K, int32_t act, int32_t fold_in, int32_t stats_out) {
  if (mio_gemm_impl() != 0) return 0;
  if (fold_in && K > GEMM_LN_FOLD_K_MAX) return 0;
  if (act == MIO_ACT_SWIGLU)  // the gated stage (interleaved gate / up blocked weight, 256 x 128 output tiles): consumer form only
    return (gemm_tiles_ok(M, N, K, 128) && !stats_out && N % 128 == 0 && (!fold_in || K % 256 == 0)) ? 1 : 0;
  if (!gemm_blocked_w_ok(M, N, K, act) || N % 32 != 0) return 0;
  if (fold_in && (K % 256 != 0 || (act != MIO_ACT_NONE && act != MIO_ACT_GELU_TANH))) return 0;
  if (stats_out && (N % 256 != 0 || act != MIO_ACT_NONE || fold_in)) return 0;
  return 1;
}

// ---- the host plan: every launch form and mio_gemm_route validate, fill the device struct and pick the kernel here ----------------
// A form is an entry point's set of checks and the words of its refusals (tests/test_gemm_refusals_host.py pins both; the order
// of the checks is not part of the contract):
enum GemmForm {
  GEMM_PLAIN,  // mio_gemm_bias_act: row-major weight, every shape
  GEMM_BW,     // mio_gemm_bias_act_bw: blocked weight, gated by mio_gemm_blocked_weight_ok
  GEMM_CS,     // mio_gemm_bias_act_bw_cs: GEMM_BW with a column range and no residual, gated by mio_gemm_col_scale_ok
  GEMM_LN,     // mio_gemm_ln_bw: blocked / interleaved weight, LayerNorm consumer or producer, gated by mio_gemm_ln_ok
  GEMM_STAGE,  // a stage of the blocked fused MLP on a blocked weight: mlp_blocked_ok has judged both stages
};

// A call as its entry point received it (the operands, sizes, strides and layouts sit in `dev`, everything not named at its
// default); gemm_plan makes `dev` what the kernel reads and names the kernel in `route`.
struct GemmCall {
  GemmForm form;
  int act, dtype, route;
  GemmDev dev;
};

static GemmCall gemm_call(GemmForm form, const void* x, const void* w, const void* bias, const void* residual, void* y, int64_t M,
                          int32_t N, int32_t K, int64_t ldx, int64_t ldy, int64_t ldr, int32_t act, int32_t dtype) {
  GemmCall c = {form, act, dtype, MIO_GEMM_ROUTE_EMPTY, {}};
  GemmDev& p = c.dev;
  gemm_dev_defaults(p);
  p.x = x; p.w = w; p.bias = bias; p.res = residual; p.y = y;
  p.M = M; p.N = N; p.K = K; p.ldx = ldx; p.ldw = K; p.ldy = ldy; p.ldr = ldr;
  p.w_blk = form == GEMM_PLAIN ? 0 : act == MIO_ACT_SWIGLU ? 2 : 1;  // (2: gate / up rows interleaved per wave)
  return c;
}

// route_only (mio_gemm_route): no pointer or dtype checks; a non-null res / ln_stats / stats_out only says that the operand is
// given.  M == 0 is answered as each entry point always has: mio_gemm_bias_act after all its checks, mio_gemm_ln_bw right after
// the null and size checks, mio_gemm_route before the blocked forms' shape checks (all three: MIO_GEMM_ROUTE_EMPTY);
// mio_gemm_bias_act_bw / _bw_cs refuse it through their shape query.
static int gemm_plan(const char* who, GemmCall& c, bool route_only) {
#define GEMM_CHECK(cond, text) MIO_CHECK(cond, std::string(who) + (text))
  GemmDev& p = c.dev;
  const bool launch = !route_only, plain = c.form == GEMM_PLAIN, bw = c.form == GEMM_BW, cs = c.form == GEMM_CS, ln = c.form == GEMM_LN;
  const bool res = p.res != nullptr, fold = p.ln_stats != nullptr, stats = p.stats_out != nullptr, glu = c.act == MIO_ACT_SWIGLU;
  const int64_t M = p.M;
  const int N = p.N, K = p.K;
  // (M == 0: x and y hold no element, and an empty allocation may be a null pointer)
  if (launch && plain) GEMM_CHECK(p.w && (M == 0 || (p.x && p.y)), ": x, w, y must be non-null");
  if (launch && !plain) GEMM_CHECK(p.x && p.w && p.y, ": x, wb, y must be non-null");
  GEMM_CHECK(M >= 0 && N > 0 && K > 0, ": bad sizes");
  if (launch && ln && M == 0) return 0;
  GEMM_CHECK(route_only || c.dtype == MIO_BF16 || c.dtype == MIO_FP16, ": dtype must be bf16 or fp16");
  if (launch && (bw || cs)) GEMM_CHECK(c.act >= MIO_ACT_NONE && c.act < MIO_ACT_SWIGLU, ": unknown / unsupported activation");
  GEMM_CHECK(c.act >= MIO_ACT_NONE && c.act <= MIO_ACT_SWIGLU, ": unknown activation");
  if (launch && plain) GEMM_CHECK(glu == (p.wg != nullptr), ": w_gate is required iff act == SWIGLU");
  GEMM_CHECK(!plain || (!fold && !stats), ": the LayerNorm forms take a blocked weight");
  // row strides: a blocked operand has none, its row length stands in (the weight's, once checked as given)
  if (p.x_blk) p.ldx = K;
  if (p.y_blk) p.ldy = N;
  if (p.res_blk) p.ldr = N;
  const bool ld8 = p.ldx % 8 == 0 && p.ldw % 8 == 0 && p.ldy % 8 == 0 && (!res || p.ldr % 8 == 0);
  const bool ldlen = p.ldx >= K && p.ldw >= K && p.ldy >= N;
  if (plain || route_only) GEMM_CHECK(K % 8 == 0 && N % 8 == 0, ": N and K must be multiples of 8");
  if (launch && plain) {
    GEMM_CHECK(ld8, ": row strides must be multiples of 8 elements");
    GEMM_CHECK(ldlen, ": row stride smaller than row length");
  }  // (only mio_gemm_ln_bw asks ldr >= N, and only mio_gemm_bias_act_bw N % 8: the other shape queries ask more of N)
  GEMM_CHECK(ld8 && ldlen && (!bw || N % 8 == 0) && (!ln || route_only || !res || p.ldr >= N), ": bad strides");
  if (!plain) p.ldw = K;
  if (launch)
    GEMM_CHECK(mio_aligned16(p.x) && mio_aligned16(p.w) && mio_aligned16(p.y) && mio_aligned16(p.wg) && mio_aligned16(p.res) &&
                   mio_aligned16(p.bias) && mio_aligned16(p.bias_g) && mio_aligned16(p.ln_stats) && mio_aligned16(p.stats_out),
               ": pointers must be 16-byte aligned");
  if (route_only && M == 0) return 0;
  if (!plain)
    GEMM_CHECK(gemm_off32(p.ldx) && gemm_off32(p.ldy) && (!res || gemm_off32(p.ldr)),
               bw || route_only ? ": row stride too large for the blocked-weight kernels" : ": row stride too large");
  if (bw)
    GEMM_CHECK(gemm_blocked_w_ok(M, N, K, c.act),
               route_only ? ": this shape does not take the blocked-weight kernels (mio_gemm_blocked_weight_ok == 0)"
                          : ": this shape does not take the blocked-weight kernels (mio_gemm_blocked_weight_ok == 0); use "
                            "mio_gemm_bias_act with the plain weight");
  if (cs) {
    GEMM_CHECK(mio_gemm_col_scale_ok(M, N, K, c.act), ": this shape does not run the persistent kernel (mio_gemm_col_scale_ok == 0)");
    GEMM_CHECK(p.cs_lo >= 0 && p.cs_hi <= N && p.cs_lo % 128 == 0 && p.cs_hi % 128 == 0 && p.cs_lo <= p.cs_hi,
               ": [cs_lo, cs_hi) must be multiples of 128 inside [0, N]");
  }
  if (ln) {
    GEMM_CHECK(glu || p.bias_g == nullptr, ": bias_gate belongs to the gated stage (act == SWIGLU)");
    GEMM_CHECK(mio_gemm_ln_ok(M, N, K, c.act, fold, stats), ": this shape / activation does not take the folded kernels (mio_gemm_ln_ok == 0)");
    if (route_only) GEMM_CHECK(!((fold || glu) && res), ": the consumer and gated forms take no residual");
    GEMM_CHECK(!(glu && res), ": the gated stage takes no residual");
    GEMM_CHECK(!(fold && res), ": the consumer form takes no residual");
    p.ln_slots = !fold ? 0 : p.ln_slots == 0 ? K / 256 : p.ln_slots;
    GEMM_CHECK(!fold || route_only || (p.ln_slots >= 1 && p.ln_slots <= GEMM_LN_SLOTS_MAX),
               ": at most 8 statistic slots (rows wider than 2048 columns: mio_ln_stats_reduce first)");
    GEMM_CHECK(!stats || res, ": the producer form is the residual epilogue");
    GEMM_CHECK(!p.res_blk || res, ": RES_BLOCKED without a residual");
    GEMM_CHECK(p.cs_lo >= p.cs_hi || (!res && p.cs_lo >= 0 && p.cs_hi <= N && p.cs_lo % 128 == 0 && p.cs_hi % 128 == 0),
               ": [cs_lo, cs_hi) must be multiples of 128 inside [0, N], without a residual");
  }
#undef GEMM_CHECK
  GemmRouteArgs ra;
  ra.M = M; ra.ldx = p.ldx; ra.ldw = p.ldw; ra.ldy = p.ldy; ra.ldr = p.ldr; ra.N = N; ra.K = K; ra.act = c.act;
  ra.res = res; ra.w_blk = p.w_blk; ra.ln_stats = fold; ra.stats_out = stats;
  c.route = gemm_pick_route(ra);
  return 0;
}

static int gemm_dispatch(const GemmCall& c, void* stream) {
  if (c.route == MIO_GEMM_ROUTE_EMPTY) return 0;
  return c.dtype == MIO_BF16 ? gemm_launch<__bf16>(c.dev, c.act, c.route, (hipStream_t)stream)
                             : gemm_launch<_Float16>(c.dev, c.act, c.route, (hipStream_t)stream);
}

static int gemm_run(const char* who, GemmCall& c, void* stream) {
  const int rc = gemm_plan(who, c, false);
  return rc != 0 ? rc : gemm_dispatch(c, stream);
}

extern "C" int mio_gemm_bias_act(const void* x, const void* w, const void* bias, const void* w_gate,
                                 const void* bias_gate, const void* residual, void* y, int64_t M, int32_t N,
                                 int32_t K, int64_t ldx, int64_t ldw, int64_t ldy, int64_t ldr, int32_t act,
                                 int32_t dtype, void* stream) {
  GemmCall c = gemm_call(GEMM_PLAIN, x, w, bias, residual, y, M, N, K, ldx, ldy, ldr, act, dtype);
  c.dev.wg = w_gate; c.dev.bias_g = bias_gate; c.dev.ldw = ldw;
  return gemm_run("mio_gemm_bias_act", c, stream);
}

extern "C" int mio_gemm_bias_act_bw(const void* x, const void* wb, const void* bias, const void* residual, void* y,
                                    int64_t M, int32_t N, int32_t K, int64_t ldx, int64_t ldy, int64_t ldr, int32_t act,
                                    int32_t dtype, int32_t x_blocked, void* stream) {
  GemmCall c = gemm_call(GEMM_BW, x, wb, bias, residual, y, M, N, K, ldx, ldy, ldr, act, dtype);
  c.dev.x_blk = x_blocked ? 1 : 0;  // blocked x: ceil(M / 256) * 256 x K elements, no row stride
  return gemm_run("mio_gemm_bias_act_bw", c, stream);
}

extern "C" int mio_gemm_bias_act_bw_cs(const void* x, const void* wb, const void* bias, void* y, int64_t M, int32_t N,
                                       int32_t K, int64_t ldx, int64_t ldy, int32_t act, int32_t dtype, int32_t x_blocked,
                                       int32_t cs_lo, int32_t cs_hi, float cs_val, void* stream) {
  GemmCall c = gemm_call(GEMM_CS, x, wb, bias, nullptr, y, M, N, K, ldx, ldy, 0, act, dtype);
  c.dev.x_blk = x_blocked ? 1 : 0;
  c.dev.cs_lo = cs_lo; c.dev.cs_hi = cs_hi; c.dev.cs_val = cs_val;
  return gemm_run("mio_gemm_bias_act_bw_cs", c, stream);
}

extern "C" int mio_gemm_ln_bw(const void* x, const void* wb, const void* bias, const void* bias_gate, const void* residual, void* y, int64_t M, int32_t N,
                              int32_t K, int64_t ldx, int64_t ldy, int64_t ldr, int32_t act, int32_t dtype, int32_t flags,
                              const float* ln_stats, int32_t ln_slots, float ln_eps, float* stats_out, int32_t cs_lo, int32_t cs_hi,
                              float cs_val, void* stream) {
  MIO_CHECK(M == 0 || (flags & ~7) == 0, "mio_gemm_ln_bw: unknown flag");
  GemmCall c = gemm_call(GEMM_LN, x, wb, bias, residual, y, M, N, K, ldx, ldy, ldr, act, dtype);
  GemmDev& p = c.dev;
  p.bias_g = bias_gate;
  p.x_blk = (flags & MIO_GEMM_X_BLOCKED) != 0; p.y_blk = (flags & MIO_GEMM_Y_BLOCKED) != 0; p.res_blk = (flags & MIO_GEMM_RES_BLOCKED) != 0;
  p.cs_lo = cs_lo; p.cs_hi = cs_hi; p.cs_val = cs_val;
  p.ln_stats = ln_stats; p.ln_slots = ln_slots; p.ln_eps = ln_eps; p.stats_out = stats_out;
  return gemm_run("mio_gemm_ln_bw", c, stream);
}

// The consumer form of mio_gemm_ln_bw behind an RMSNorm: same kernels, routes and checks (form GEMM_LN), rstd without the mean.
extern "C" int mio_gemm_rms_bw(const void* x, const void* wb, const void* bias, const void* bias_gate, const void* residual, void* y, int64_t M, int32_t N,
                               int32_t K, int64_t ldx, int64_t ldy, int64_t ldr, int32_t act, int32_t dtype, int32_t flags,
                               const float* ln_stats, int32_t ln_slots, float ln_eps, float* stats_out, int32_t cs_lo, int32_t cs_hi,
                               float cs_val, void* stream) {
  MIO_CHECK(M == 0 || (flags & ~7) == 0, "mio_gemm_rms_bw: unknown flag");
  MIO_CHECK(ln_stats != nullptr, "mio_gemm_rms_bw: ln_stats must be non-null (the consumer form only)");
  MIO_CHECK(residual == nullptr, "mio_gemm_rms_bw: the consumer form takes no residual");
  MIO_CHECK(stats_out == nullptr, "mio_gemm_rms_bw: the consumer form writes no statistics (stats_out)");
  GemmCall c = gemm_call(GEMM_LN, x, wb, bias, nullptr, y, M, N, K, ldx, ldy, ldr, act, dtype);
  GemmDev& p = c.dev;
  p.bias_g = bias_gate;
  p.x_blk = (flags & MIO_GEMM_X_BLOCKED) != 0; p.y_blk = (flags & MIO_GEMM_Y_BLOCKED) != 0;
  p.cs_lo = cs_lo; p.cs_hi = cs_hi; p.cs_val = cs_val;
  p.ln_stats = ln_stats; p.ln_slots = ln_slots; p.ln_eps = ln_eps; p.ln_rms = 1;
  return gemm_run("mio_gemm_rms_bw", c, stream);
}

// ---- route query ------------------------------------------------------------------------------------------------------
extern "C" int32_t mio_gemm_route(int64_t M, int32_t N, int32_t K, int64_t ldx, int64_t ldw, int64_t ldy, int64_t ldr, int32_t act,
                                  int32_t has_residual, int32_t w_layout, int32_t fold_in, int32_t stats_out) {
  MIO_CHECK(w_layout >= 0 && w_layout <= 2, "mio_gemm_route: w_layout must be 0 (row-major), 1 (blocked) or 2 (gate / up interleaved)");
  MIO_CHECK((w_layout == 2) == (act == MIO_ACT_SWIGLU) || w_layout == 0,
            "mio_gemm_route: the interleaved weight belongs to act == SWIGLU, and SWIGLU has no plain blocked weight");
  static float given[1];  // marks an operand as given: the plan reads no pointer of a route query
  const GemmForm form = w_layout == 0 ? GEMM_PLAIN : (fold_in || stats_out || act == MIO_ACT_SWIGLU) ? GEMM_LN : GEMM_BW;
  GemmCall c = gemm_call(form, nullptr, nullptr, nullptr, has_residual ? given : nullptr, nullptr, M, N, K, ldx, ldy, ldr, act, MIO_BF16);
  c.dev.ldw = ldw;  // (checked as given, also where a blocked weight then counts with its row length K)
  c.dev.w_blk = w_layout;
  c.dev.ln_stats = fold_in ? given : nullptr;
  c.dev.stats_out = stats_out ? given : nullptr;
  const int rc = gemm_plan("mio_gemm_route", c, true);
  return rc != 0 ? rc : c.route;
}

// ---- fused MLP ------------------------------------------------------------------------------------------------------------
extern "C" size_t mio_fused_mlp_workspace_bytes(int64_t M, int32_t d, int32_t I, int32_t act) {
  (void)d; (void)act;
  const int64_t mp = (M + 255) / 256 * 256;  // whole 256-row blocks (blocked intermediate layout)
  return (size_t)mp * (size_t)I * 2;
}

// Two GEMMs.  Where mlp_blocked_ok, both run on the 256-tile kernels with the intermediate in the blocked layout (SwiGLU: only
// with its interleaved blocked weight) and refusals come as mio_fused_mlp_fwd; elsewhere they are what two mio_gemm_bias_act
// calls are, refusals under that name included.
static int fused_mlp_impl(const void* x, const void* w1, const void* b1, const void* wg, const void* bg, const void* w2,
                          const void* b2, const void* residual, void* y, void* workspace, int64_t M, int32_t d, int32_t I,
                          int32_t act, int32_t dtype, void* stream, int wblk, int xblk = 0) {
  MIO_CHECK(workspace != nullptr || M == 0, "mio_fused_mlp_fwd: workspace must be non-null");
  MIO_CHECK(act != MIO_ACT_NONE, "mio_fused_mlp_fwd: an activation is required");
  const bool glu = act == MIO_ACT_SWIGLU;
  const bool blocked = M > 0 && mlp_blocked_ok(M, d, I) && (!glu || wblk);
  if (blocked) MIO_CHECK(x && w1 && w2 && y, "mio_fused_mlp_fwd: x, w1, w2, y must be non-null");
  else MIO_CHECK(!wblk && !xblk, "mio_fused_mlp_fwd_bw: this shape does not take the blocked-weight kernels "
                                 "(mio_fused_mlp_blocked_weight_ok == 0); pass the plain weights to mio_fused_mlp_fwd");
  const char* who = blocked ? "mio_fused_mlp_fwd" : "mio_gemm_bias_act";
  const GemmForm form = wblk ? GEMM_STAGE : GEMM_PLAIN;
  // stage 1: h = act(x w1^T + b1) [* silu-gate], written once in the storage dtype
  GemmCall s1 = gemm_call(form, x, w1, b1, nullptr, workspace, M, I, d, d, I, 0, act, dtype);
  s1.dev.x_blk = xblk; s1.dev.y_blk = blocked;
  if (!blocked) s1.dev.wg = wg;
  if (!blocked || glu) s1.dev.bias_g = bg;
  // stage 2: y = h w2^T + b2 (+ residual)
  GemmCall s2 = gemm_call(form, workspace, w2, b2, residual, y, M, d, I, I, d, d, MIO_ACT_NONE, dtype);
  s2.dev.x_blk = blocked;
  int rc = gemm_plan(who, s1, false);
  if (rc == 0) rc = gemm_plan(who, s2, false);
  if (rc == 0) rc = gemm_dispatch(s1, stream);
  return rc != 0 ? rc : gemm_dispatch(s2, stream);
}

extern "C" int mio_fused_mlp_fwd(const void* x, const void* w1, const void* b1, const void* wg, const void* bg,
                                 const void* w2, const void* b2, const void* residual, void* y, void* workspace,
                                 int64_t M, int32_t d, int32_t I, int32_t act, int32_t dtype, void* stream) {
  return fused_mlp_impl(x, w1, b1, wg, bg, w2, b2, residual, y, workspace, M, d, I, act, dtype, stream, 0);
}

extern "C" int mio_fused_mlp_fwd_bw(const void* x, const void* w1b, const void* b1, const void* w2b, const void* b2,
                                    const void* residual, void* y, void* workspace, int64_t M, int32_t d, int32_t I,
                                    int32_t act, int32_t dtype, int32_t x_blocked, void* stream) {
  return fused_mlp_impl(x, w1b, b1, nullptr, nullptr, w2b, b2, residual, y, workspace, M, d, I, act, dtype, stream, 1,
                        x_blocked ? 1 : 0);
}

extern "C" int mio_fused_mlp_glu_fwd_bw(const void* x, const void* wgu_b, const void* b_up, const void* b_gate, const void* w2b,
                                        const void* b2, const void* residual, void* y, void* workspace, int64_t M, int32_t d,
                                        int32_t I, int32_t dtype, int32_t x_blocked, void* stream) {
  MIO_CHECK(mio_aligned16(b_gate), "mio_fused_mlp_glu_fwd_bw: pointers must be 16-byte aligned");
  MIO_CHECK(M == 0 || mlp_blocked_ok(M, d, I),
            "mio_fused_mlp_glu_fwd_bw: this shape does not take the 256-tile kernels (mio_fused_mlp_blocked_weight_ok(.., SWIGLU) == 0); "
            "pass the plain weights to mio_fused_mlp_fwd");
  return fused_mlp_impl(x, wgu_b, b_up, nullptr, b_gate, w2b, b2, residual, y, workspace, M, d, I, MIO_ACT_SWIGLU, dtype, stream, 1,
                        x_blocked ? 1 : 0);
}

// ---- blocked weights -----------------------------------------------------------------------------------------------
extern "C" size_t mio_weight_blocked_bytes(int32_t N, int32_t K) {
  return (size_t)((N + 255) / 256 * 256) * (size_t)K * 2;
}

// one 16-byte chunk per thread: destination unit u = ((tn * nk + kt) * 256 + row) * 4 + chunk
__global__ void weight_block_kernel(const uint16_t* __restrict__ w, int64_t ldw, uint16_t* __restrict__ wb, int N, int K,
                                    int64_t units) {
  const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= units) return;
  const int nk = K / 32;
  const int chunk = (int)(u & 3), row = (int)((u >> 2) & 255);
  const int64_t blk = u >> 10;
  const int kt = (int)(blk % nk), tn = (int)(blk / nk);
  const int n = tn * 256 + row;
  u32x4_t v = {0u, 0u, 0u, 0u};
  if (n < N) v = *(const u32x4_t*)(w + (int64_t)n * ldw + kt * 32 + chunk * 8);
  *(u32x4_t*)(wb + u * 8) = v;
}

extern "C" int mio_weight_block(const void* w, int64_t ldw, void* wb, int32_t N, int32_t K, int32_t dtype, void* stream) {
  MIO_CHECK(w && wb, "mio_weight_block: w and wb must be non-null");
  MIO_CHECK(dtype == MIO_BF16 || dtype == MIO_FP16, "mio_weight_block: dtype must be bf16 or fp16");
  MIO_CHECK(N > 0 && K > 0 && K % 32 == 0 && ldw >= K && ldw % 8 == 0, "mio_weight_block: need K % 32 == 0, ldw % 8 == 0");
  MIO_CHECK(mio_aligned16(w) && mio_aligned16(wb), "mio_weight_block: pointers must be 16-byte aligned");
  const int64_t units = (int64_t)((N + 255) / 256) * (K / 32) * 1024;
  hipLaunchKernelGGL(weight_block_kernel, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const uint16_t*)w, ldw, (uint16_t*)wb, N, K, units);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mio_fail(std::string("mio_weight_block launch: ") + hipGetErrorString(e));
  return 0;
}

// ---- SwiGLU on the 256-tile kernel: gate / up weights interleaved per wave in one blocked weight ----------------------
extern "C" size_t mio_weight_blocked_glu_bytes(int32_t I, int32_t K) {
  return (size_t)((I + 127) / 128 * 256) * (size_t)K * 2;
}

// one 16-byte chunk per thread: destination unit u = ((tn * nk + kt) * 256 + row) * 4 + chunk, row = wn * 64 + h * 32 + j
// <- row tn * 128 + wn * 32 + j of the gate (h = 0) or up (h = 1) weight
__global__ void weight_block_glu_kernel(const uint16_t* __restrict__ wg, const uint16_t* __restrict__ wu, int64_t ldw,
                                        uint16_t* __restrict__ wb, int I, int K, int64_t units) {
  const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= units) return;
  const int nk = K / 32;
  const int chunk = (int)(u & 3), row = (int)((u >> 2) & 255);
  const int64_t blk = u >> 10;
  const int kt = (int)(blk % nk), tn = (int)(blk / nk);
  const int n = tn * 128 + (row >> 6) * 32 + (row & 31);
  const uint16_t* src = ((row >> 5) & 1) ? wu : wg;
  u32x4_t v = {0u, 0u, 0u, 0u};
  if (n < I) v = *(const u32x4_t*)(src + (int64_t)n * ldw + kt * 32 + chunk * 8);
  *(u32x4_t*)(wb + u * 8) = v;
}

extern "C" int mio_weight_block_glu(const void* w_gate, const void* w_up, int64_t ldw, void* wb, int32_t I, int32_t K,
                                    int32_t dtype, void* stream) {
  MIO_CHECK(w_gate && w_up && wb, "mio_weight_block_glu: w_gate, w_up and wb must be non-null");
  MIO_CHECK(dtype == MIO_BF16 || dtype == MIO_FP16, "mio_weight_block_glu: dtype must be bf16 or fp16");
  MIO_CHECK(I > 0 && K > 0 && K % 32 == 0 && ldw >= K && ldw % 8 == 0, "mio_weight_block_glu: need K % 32 == 0, ldw % 8 == 0");
  MIO_CHECK(mio_aligned16(w_gate) && mio_aligned16(w_up) && mio_aligned16(wb), "mio_weight_block_glu: pointers must be 16-byte aligned");
  const int64_t units = (int64_t)((I + 127) / 128) * (K / 32) * 1024;
  hipLaunchKernelGGL(weight_block_glu_kernel, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const uint16_t*)w_gate, (const uint16_t*)w_up, ldw, (uint16_t*)wb, I, K, units);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mio_fail(std::string("mio_weight_block_glu launch: ") + hipGetErrorString(e));
  return 0;
}

// ---- LayerNorm folded into the GEMMs on either side of it ------------------------------------------------
// Reference: kernels/triton/fused_layernorm_qkv.py:37-420 (LayerNorm as the prologue of the QKV projection) and
// layernorm_kernels.py:35-188 (residual add + LayerNorm in one pass).  Here neither a prologue nor a pass: the GEMM that
// WRITES the residual stream (out-proj / fc2, residual epilogue) also writes each output row's (sum, sum of squares) per
// 256-column tile, and the projection BEHIND the LayerNorm multiplies the raw stream with gamma-scaled weights and applies
// rstd in its read-out:  LN(x) W^T + b = rstd * (x - mean 1) (gamma o W)^T + b' = rstd * x W'^T + b',  W' = gamma o W with every
// row's mean over k subtracted (the centring moves from the activations to the weights), b' = b + W beta.
extern "C" size_t mio_ln_stats_bytes(int64_t M, int32_t width) {
  return (size_t)((width + 255) / 256) * (size_t)((M + 255) / 256 * 256) * 2 * sizeof(float);
}


// one workgroup per weight row: w_scaled[n][k] = T(w[n][k] * gamma[k] - mean_k(w[n][.] * gamma[.])) (the row mean is taken over
// the unrounded products), bias_out[n] = T(bias[n] + sum_k w[n][k] * beta[k]).
// The consumer's read-out relies on sum_k w_scaled[n][k] = 0 (that is what removes the activations' mean); after rounding to 16
// bits the sum is off by ~sqrt(K / 12) ulp, and the product picks up mean(x) times that.  So the rounding DIRECTION of a few
// elements is flipped (those whose exact value sits closest to the midpoint of its two neighbours: the flip leaves their own
// error almost unchanged, weighed against how much of the sum it removes) until no flip brings the row sum closer to zero.
// One-time weight preparation.  Every step strictly lowers |sum| and the loop leaves as soon as no flip does, so the step
// count only has to be large enough: a row starts about sqrt(K / 12) ulp off and a flip takes off at most one ulp of its own
// element, less where a gamma spread over many binades leaves the residue to the K / 13 or so elements of the top binade.
// A fixed budget of 64 ran out there (K 8192, gamma = +-2^-6 .. 2^6: 32 ulp of the row's largest element were left), so the
// budget is max(64, K).  Rows that 64 steps had cut short (wide rows may be among them under any gamma) now come out closer to a
// zero sum than before; rows that were done within 64 steps are prepared bit for bit as before.
template <typename T, int EPT>  // EPT: elements per thread (K <= 256 * EPT)
__global__ __launch_bounds__(256) void ln_fold_weight_kernel(const T* __restrict__ w, int64_t ldw, const T* __restrict__ gamma,
                                                             const T* __restrict__ beta, const T* __restrict__ bias,
                                                             T* __restrict__ ws, T* __restrict__ bias_out, int K) {
  __shared__ float s_c[256], s_b[256];
  __shared__ int s_i[256];
  const int n = blockIdx.x, t = threadIdx.x;
  float c = 0.f, bb = 0.f;
  for (int k = t; k < K; k += 256) {
    const float wv = (float)w[(int64_t)n * ldw + k];
    c += wv * (float)gamma[k];
    if (beta != nullptr) bb += wv * (float)beta[k];
  }
  s_c[t] = c;
  s_b[t] = bb;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) {
      s_c[t] += s_c[t + s];
      s_b[t] += s_b[t + s];
    }
    __syncthreads();
  }
  const float mean = s_c[0] / (float)K;
  if (t == 0) bias_out[n] = (T)((bias != nullptr ? (float)bias[n] : 0.f) + s_b[0]);
  __syncthreads();
  // rounded values (as 16-bit patterns) and their exact counterparts
  uint16_t bits[EPT];
  float exact[EPT];
  float sum = 0.f;
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const int k = t + 256 * e;
    bits[e] = 0;
    exact[e] = 0.f;
    if (k < K) {
      exact[e] = (float)w[(int64_t)n * ldw + k] * (float)gamma[k] - mean;
      const T r = (T)exact[e];
      bits[e] = __builtin_bit_cast(uint16_t, r);
      sum += (float)r;
    }
  }
  auto val = [](uint16_t b) { return (float)__builtin_bit_cast(T, b); };
  const int budget = K > 64 ? K : 64;
  for (int it = 0; it < budget; ++it) {
    s_c[t] = sum;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (t < s) s_c[t] += s_c[t + s];
      __syncthreads();
    }
    const float eps = s_c[0];  // sum of the rounded row (the exact row sums to zero)
    __syncthreads();
    // this thread's best flip: moves the sum towards zero without overshooting past -eps, smallest growth of its own error
    float best = 3.0e38f;
    int best_e = -1;
    uint16_t best_bits = 0;
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      const int k = t + 256 * e;
      if (k >= K || (bits[e] & 0x7fff) == 0) continue;
      const float cur = val(bits[e]);
      // the neighbour on the other side of the exact value
      const bool up = cur < exact[e];  // rounded down -> candidate is the next value up
      const bool neg = (bits[e] & 0x8000) != 0;
      const uint16_t nb = (uint16_t)((up != neg) ? bits[e] + 1 : bits[e] - 1);
      const float nv = val(nb);
      const float delta = nv - cur;
      if (!(delta * eps < 0.f) || fabsf(eps + delta) >= fabsf(eps)) continue;
      // what the flip takes off |sum| minus what it adds to the element's own error (lower = better; the reduction of s_b is a min)
      const float cost = fmaxf(fabsf(nv - exact[e]) - fabsf(cur - exact[e]), 0.f) - (fabsf(eps) - fabsf(eps + delta));
      if (cost < best) {
        best = cost;
        best_e = e;
        best_bits = nb;
      }
    }
    s_b[t] = best;
    s_i[t] = t;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (t < s && s_b[t + s] < s_b[t]) {
        s_b[t] = s_b[t + s];
        s_i[t] = s_i[t + s];
      }
      __syncthreads();
    }
    const bool any = s_b[0] < 3.0e38f;
    const int winner = s_i[0];
    __syncthreads();
    if (!any) break;
    if (t == winner) {
#pragma unroll
      for (int e = 0; e < EPT; ++e)
        if (e == best_e) {
          sum += val(best_bits) - val(bits[e]);
          bits[e] = best_bits;
        }
    }
  }
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const int k = t + 256 * e;
    if (k < K) ws[(int64_t)n * K + k] = __builtin_bit_cast(T, bits[e]);
  }
}

extern "C" int mio_ln_fold_weight(const void* w, int64_t ldw, const void* gamma, const void* beta, const void* bias,
                                  void* w_scaled, void* bias_out, int32_t N, int32_t K, int32_t dtype, void* stream) {
  MIO_CHECK(w && gamma && w_scaled && bias_out, "mio_ln_fold_weight: w, gamma, w_scaled, bias_out must be non-null");
  MIO_CHECK(dtype == MIO_BF16 || dtype == MIO_FP16, "mio_ln_fold_weight: dtype must be bf16 or fp16");
  MIO_CHECK(N > 0 && K > 0 && K <= GEMM_LN_FOLD_K_MAX && ldw >= K, "mio_ln_fold_weight: bad sizes (K <= 8192)");
#define MIO_LNFW(T_, E_)                                                                                                       \
  hipLaunchKernelGGL((ln_fold_weight_kernel<T_, E_>), dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, (const T_*)w, ldw, \
                     (const T_*)gamma, (const T_*)beta, (const T_*)bias, (T_*)w_scaled, (T_*)bias_out, K)
  if (dtype == MIO_BF16) {
    if (K <= 2048) MIO_LNFW(__bf16, 8); else MIO_LNFW(__bf16, 32);
  } else {
    if (K <= 2048) MIO_LNFW(_Float16, 8); else MIO_LNFW(_Float16, 32);
  }
#undef MIO_LNFW
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mio_fail(std::string("mio_ln_fold_weight launch: ") + hipGetErrorString(e));
  return 0;
}

// rows wider than 2048 columns leave more than GEMM_LN_SLOTS_MAX statistic slots: summed in groups (fixed order) down to a count
// the consumer's LDS region holds -- one small launch per LayerNorm, against a LayerNorm pass over the whole stream
__global__ void ln_stats_reduce_kernel(const float* __restrict__ in, float* __restrict__ out, int per, int64_t n2, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // over slots_out * rows * 2 floats
  if (i >= total) return;
  const int64_t so = i / n2, r = i % n2;
  float a = 0.f;
  for (int j = 0; j < per; ++j) a += in[(so * per + j) * n2 + r];
  out[i] = a;
}

extern "C" int mio_ln_stats_reduce(const float* stats_in, int32_t slots_in, float* stats_out, int32_t slots_out, int64_t M, void* stream) {
  MIO_CHECK(stats_in && stats_out, "mio_ln_stats_reduce: null pointer");
  MIO_CHECK(slots_in > 0 && slots_out > 0 && slots_in % slots_out == 0 && M >= 0, "mio_ln_stats_reduce: slots_in must be a multiple of slots_out");
  const int64_t n2 = (M + 255) / 256 * 256 * 2, total = n2 * slots_out;
  if (total == 0) return 0;
  hipLaunchKernelGGL(ln_stats_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, stats_in, stats_out,
                     slots_in / slots_out, n2, total);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mio_fail(std::string("mio_ln_stats_reduce launch: ") + hipGetErrorString(e));
  return 0;
}

// C-ABI entry points of the attention forward, dense (mio_fa3_fwd), packed varlen (mio_fa3_fwd_varlen) and paged
// (mio_fa3_fwd_paged): argument validation + dispatch (see include/mio_hip.h).
#include <algorithm>
#include <cmath>
#include <initializer_list>

#include "fa3_fwd_kernel.h"
#include "fa3_route.h"
#include "fa3_paged.h"
#include "fa3_varlen.h"

static bool strides_ok(const int64_t s[3]) { return (s[0] % 8 == 0) && (s[1] % 8 == 0) && (s[2] % 8 == 0); }

static bool aligned16(std::initializer_list<const void*> ptrs) {
  for (const void* p : ptrs)
    if (!mio_aligned16(p)) return false;
  return true;
}

// The checks all three entry points make alike, in this order; fn (the entry point's name) prefixes the messages.
static int fa_check_common(const char* fn, int H, int Hkv, int D, int dtype, float softmax_scale) {
  MIO_CHECK(H % Hkv == 0, std::string(fn) + ": H must be a multiple of Hkv");
  MIO_CHECK(D >= 8 && D <= 128 && D % 8 == 0, std::string(fn) + ": head_dim must be a multiple of 8 in [8,128]");
  MIO_CHECK(dtype == MIO_BF16 || dtype == MIO_FP16, std::string(fn) + ": dtype must be bf16 or fp16");
  MIO_CHECK(softmax_scale > 0.f && std::isfinite(softmax_scale), std::string(fn) + ": softmax_scale must be > 0");
  return 0;
}

// The packed-row checks of the per-sequence forms (varlen, paged): [token, head] strides, pointers, max_seqlen_q.
static int fa_check_packed(const char* fn, std::initializer_list<const int64_t*> strides,
                           std::initializer_list<const void*> ptrs, int total_q, int max_seqlen_q) {
  for (const int64_t* s : strides)
    MIO_CHECK(s[0] >= 0 && s[1] >= 0 && s[0] % 8 == 0 && s[1] % 8 == 0,
              std::string(fn) + ": strides must be non-negative multiples of 8 elements (16-byte rows)");
  MIO_CHECK(aligned16(ptrs), std::string(fn) + ": pointers must be 16-byte aligned");
  MIO_CHECK(total_q == 0 || max_seqlen_q >= 1, std::string(fn) + ": max_seqlen_q must be >= 1 when total_q > 0");
  return 0;
}

// The FaDev fields all three entry points fill alike; each adds its strides and its own fields.
static FaDev fa_dev(const void* q, const void* k, const void* v, void* o, float* lse, int B, int H, int Hkv, int D,
                    float softmax_scale) {
  FaDev p = {};
  p.q = q; p.k = k; p.v = v; p.o = o; p.lse = lse;
  p.B = B; p.H = H; p.Hkv = Hkv; p.D = D;
  p.xcd_remap = ((B * H) % 8 == 0) ? 1 : 0;
  p.scale_log2e = softmax_scale * FA_LOG2E;
  return p;
}

static int dpad_of(int D) { return D <= 64 ? 64 : (D <= 96 ? 96 : 128); }

template <typename T_, int D_>
struct FaInst {  // one (dtype, padded head dim) instantiation of the launchers
  using T = T_;
  static constexpr int D = D_;
};

// f(FaInst<T, D>{}) for the launch's dtype and padded head dim: the one list of the instantiations the library holds
template <typename F>
static int fa_dispatch(int dtype, int D, F&& f) {
  const int dpad = dpad_of(D);
  if (dtype == MIO_BF16) {
    if (dpad == 64) return f(FaInst<__bf16, 64>{});
    if (dpad == 96) return f(FaInst<__bf16, 96>{});
    return f(FaInst<__bf16, 128>{});
  }
  if (dpad == 64) return f(FaInst<_Float16, 64>{});
  if (dpad == 96) return f(FaInst<_Float16, 96>{});
  return f(FaInst<_Float16, 128>{});
}

extern "C" int32_t mio_fa3_k_prescaled_ok(const mio_fa3_fwd_params_t* a) {
  if (a == nullptr) return 0;
  const bool span32 = (int64_t)a->Sk * a->k_stride[1] * 2 < (1ll << 32) && (int64_t)a->Sk * a->v_stride[1] * 2 < (1ll << 32);
  if (!(a->D <= 96 && a->mask_kind == MIO_MASK_NONE && a->Sq > 128 && a->Sk > 0 && span32)) return 0;
  const bool plain = a->o != nullptr && a->o_acc == nullptr && !a->carry_in;
  // the (o_acc, lse) ring carry: fa3_fwd5_kernel only (head dim <= 64)
  return (plain || (a->D <= 64 && a->o_acc != nullptr && a->lse != nullptr)) ? 1 : 0;
}

extern "C" int32_t mio_fa3_o_blocked_ok(const mio_fa3_fwd_params_t* a) {
  if (a == nullptr || !mio_fa3_k_prescaled_ok(a)) return 0;
  const bool plain = a->o != nullptr && a->o_acc == nullptr && !a->carry_in;
  return (plain && a->D <= 64 && ((int64_t)a->H * a->D) % 32 == 0) ? 1 : 0;
}

// every argument check of mio_fa3_fwd (0 or -1 with the message set)
static int fa3_validate(const mio_fa3_fwd_params_t* a) {
  MIO_CHECK(a != nullptr, "mio_fa3_fwd: null params");
  MIO_CHECK(a->q && a->k && a->v, "mio_fa3_fwd: q/k/v must be non-null");
  MIO_CHECK(a->o != nullptr || a->o_acc != nullptr, "mio_fa3_fwd: o or o_acc must be given");
  MIO_CHECK(a->B > 0 && a->H > 0 && a->Hkv > 0 && a->Sq >= 0 && a->Sk >= 0, "mio_fa3_fwd: bad sizes");
  if (fa_check_common("mio_fa3_fwd", a->H, a->Hkv, a->D, a->dtype, a->softmax_scale) != 0) return -1;
  MIO_CHECK(a->mask_kind >= 0 && a->mask_kind <= 2, "mio_fa3_fwd: bad mask_kind");
  MIO_CHECK((a->mask_kind == MIO_MASK_NONE) == (a->mask == nullptr), "mio_fa3_fwd: mask pointer / mask_kind mismatch");
  MIO_CHECK(strides_ok(a->q_stride) && strides_ok(a->k_stride) && strides_ok(a->v_stride) &&
                (a->o == nullptr || a->o_blocked || strides_ok(a->o_stride)),
            "mio_fa3_fwd: strides must be multiples of 8 elements (16-byte rows)");
  MIO_CHECK(aligned16({a->q, a->k, a->v, a->o, a->o_acc}), "mio_fa3_fwd: pointers must be 16-byte aligned");
  MIO_CHECK(!a->carry_in || (a->o_acc && a->lse), "mio_fa3_fwd: carry_in needs o_acc and lse");
  MIO_CHECK(a->o_acc == nullptr || a->lse != nullptr, "mio_fa3_fwd: o_acc needs lse");
  if (a->Sq == 0) return 0;  // nothing is launched
  MIO_CHECK(!a->o_blocked || (a->k_prescaled && mio_fa3_o_blocked_ok(a)), "mio_fa3_fwd: o_blocked is not supported for this launch "
                                                                          "(needs k_prescaled and mio_fa3_o_blocked_ok != 0)");
  MIO_CHECK(!a->k_prescaled || mio_fa3_k_prescaled_ok(a), "mio_fa3_fwd: k_prescaled is not supported for this launch "
                                                          "(mio_fa3_k_prescaled_ok == 0)");
  return 0;
}

static int route_of(const mio_fa3_fwd_params_t* a) {
  Fa3RouteArgs r;
  r.dpad = dpad_of(a->D);
  r.mask_kind = a->mask_kind;
  r.Sq = a->Sq;
  r.Sk = a->Sk;
  r.ks_s = a->k_stride[1];
  r.vs_s = a->v_stride[1];
  r.o = a->o != nullptr;
  r.o_acc = a->o_acc != nullptr;
  r.carry_in = a->carry_in != 0;
  r.k_prescaled = a->k_prescaled != 0;
  r.o_blocked = a->o_blocked != 0;
  return fa3_pick_route(r);
}

// ---- sliding windows (flash-attn's window_size = (left, right)): the mio_fa3_*_window entry points.  (-1, -1) is the
// entry point without a window exactly; any other window takes the windowed fwd5 / fwd3 kernels (fa3_win_inst.hip, and
// fa3_kv8_inst.hip over the fp8 cache) for every launch with keys.

constexpr int64_t FA_WIN_LEN_MAX = 1 << 28;  // lengths and offsets of a windowed launch (the kernels' bounds stay in int)
constexpr int32_t FA_WIN_CLAMP = 1 << 29;    // a window wider than every length is the unbounded one: clamped to this

static bool fa_windowed(int32_t left, int32_t right) { return left != -1 || right != -1; }

static int fa_window_check(const char* fn, int32_t left, int32_t right, int causal) {
  MIO_CHECK(left >= -1 && right >= -1, std::string(fn) + ": window values must be -1 (unbounded) or >= 0");
  MIO_CHECK(!causal || right <= 0, std::string(fn) + ": causal means window_right = 0 (give -1 or 0)");
  return 0;
}

// the checks a window adds to those of a per-sequence form (varlen, paged)
static int fa_window_check_packed(const char* fn, int32_t left, int32_t right, int causal, int max_seqlen_q, int max_seqlen_k) {
  if (fa_window_check(fn, left, right, causal) != 0) return -1;
  MIO_CHECK(max_seqlen_q < FA_WIN_LEN_MAX && max_seqlen_k < FA_WIN_LEN_MAX,
            std::string(fn) + ": max_seqlen_q / max_seqlen_k must be below 2^28 under a window");
  return 0;
}

// A launch as its form's plan function (fa3_plan, fa3_varlen_plan, fa3_paged_plan) describes it.  Each plan makes every
// argument check of its form's entry points in one order and returns the form's route: INVALID (-1: refused, the message
// is set), EMPTY (0: nothing to launch) or the kernel, with the plan filled.  The launch entry point and its route query
// both go through it; nothing here reads device memory (the kernels clamp sequence bounds, block indices and pages).
struct FaPlan {
  FaDev p;      // the grid fields of the pipelined kernels are set by their launchers
  FaVarlen vl;  // fa3_varlen_plan
  FaPaged pg;   // fa3_paged_plan
  int wl, wr;   // the window, clamped; (-1, -1): the kernels without a window
};
static_assert(MIO_FA3_ROUTE_INVALID == -1 && MIO_FA3_ROUTE_EMPTY == 0 && MIO_FA3_VARLEN_ROUTE_INVALID == -1 &&
              MIO_FA3_VARLEN_ROUTE_EMPTY == 0 && MIO_FA3_PAGED_ROUTE_INVALID == -1 && MIO_FA3_PAGED_ROUTE_EMPTY == 0,
              "a route <= EMPTY is the launch entry point's return value");

// the pipelined kernel of a head dim: fwd5 at padded head dim 64, fwd3 at 96 / 128
static int fa_pipelined(int D, int fwd5, int fwd3) { return dpad_of(D) == 64 ? fwd5 : fwd3; }

static void fa_plan_window(FaPlan& pl, int32_t left, int32_t right) {
  pl.wl = left > FA_WIN_CLAMP ? FA_WIN_CLAMP : left;
  pl.wr = right > FA_WIN_CLAMP ? FA_WIN_CLAMP : right;
}

// dense (mio_fa3_fwd, mio_fa3_fwd_window): a mio_fa3_route_t
static int fa3_plan(FaPlan& pl, const mio_fa3_fwd_params_t* a, int32_t left, int32_t right) {
  if (fa3_validate(a) != 0) return -1;
  const bool win = fa_windowed(left, right);
  if (win) {
    const char* fn = "mio_fa3_fwd_window";
    if (fa_window_check(fn, left, right, a->causal) != 0) return -1;
    MIO_CHECK(a->mask_kind == MIO_MASK_NONE, std::string(fn) + ": a window cannot be combined with a mask");
    MIO_CHECK(a->o_acc == nullptr && !a->carry_in, std::string(fn) + ": a window cannot be combined with the ring carry");
    MIO_CHECK(!a->k_prescaled, std::string(fn) + ": a window cannot be combined with k_prescaled");
    MIO_CHECK(!a->o_blocked, std::string(fn) + ": a window cannot be combined with o_blocked");
    MIO_CHECK((int64_t)a->Sk * a->k_stride[1] * 2 < (1ll << 32) && (int64_t)a->Sk * a->v_stride[1] * 2 < (1ll << 32),
              std::string(fn) + ": K / V rows of one (batch, head) must span less than 4 GiB under a window");
    MIO_CHECK(a->Sq < FA_WIN_LEN_MAX && a->Sk < FA_WIN_LEN_MAX && std::abs((int64_t)a->q_offset - a->k_offset) < FA_WIN_LEN_MAX,
              std::string(fn) + ": Sq, Sk and |q_offset - k_offset| must be below 2^28 under a window");
  }
  if (a->Sq == 0) return MIO_FA3_ROUTE_EMPTY;
  if (win && a->Sk > 0) fa_plan_window(pl, left, right);
  else fa_plan_window(pl, -1, -1);  // no key to window: the launch without one writes the empty rows

  FaDev& p = pl.p = fa_dev(a->q, a->k, a->v, a->o, a->lse, a->B, a->H, a->Hkv, a->D, a->softmax_scale);
  p.o_acc = a->o_acc; p.mask = a->mask;
  p.qs_b = a->q_stride[0]; p.qs_s = a->q_stride[1]; p.qs_h = a->q_stride[2];
  p.ks_b = a->k_stride[0]; p.ks_s = a->k_stride[1]; p.ks_h = a->k_stride[2];
  p.vs_b = a->v_stride[0]; p.vs_s = a->v_stride[1]; p.vs_h = a->v_stride[2];
  p.os_b = a->o_stride[0]; p.os_s = a->o_stride[1]; p.os_h = a->o_stride[2];
  p.ms_b = a->mask_stride[0]; p.ms_h = a->mask_stride[1]; p.ms_q = a->mask_stride[2]; p.ms_k = a->mask_stride[3];
  p.Sq = a->Sq; p.Sk = a->Sk;
  p.carry_in = a->carry_in; p.q_offset = a->q_offset; p.k_offset = a->k_offset;
  p.nqblk = (a->Sq + FA_BM - 1) / FA_BM;  // fa3_fwd_kernel's grid
  p.qgrid = p.nqblk;
  p.k_prescaled = a->k_prescaled ? 1 : 0;
  p.o_blk = a->o_blocked ? 1 : 0;

  if (fa_windowed(pl.wl, pl.wr)) return fa_pipelined(a->D, MIO_FA3_ROUTE_FWD5, MIO_FA3_ROUTE_FWD3);
  const int r = route_of(a);
  if (r == MIO_FA3_ROUTE_INVALID) return mio_fail("fa3_fwd: k_prescaled launch outside the kernels that support it");
  return r;
}

extern "C" int32_t mio_fa3_route_window(const mio_fa3_fwd_params_t* a, int32_t window_left, int32_t window_right) {
  FaPlan pl;
  return fa3_plan(pl, a, window_left, window_right);
}

extern "C" int32_t mio_fa3_route(const mio_fa3_fwd_params_t* a) { return mio_fa3_route_window(a, -1, -1); }

extern "C" int mio_fa3_fwd_window(const mio_fa3_fwd_params_t* a, int32_t window_left, int32_t window_right, void* stream) {
  FaPlan pl;
  const int route = fa3_plan(pl, a, window_left, window_right);
  if (route <= MIO_FA3_ROUTE_EMPTY) return route;
  return fa_dispatch(a->dtype, a->D, [&](auto i) {
    using T = typename decltype(i)::T;
    constexpr int D = decltype(i)::D;
    if (fa_windowed(pl.wl, pl.wr)) return fa3_win_launch<T, D>(pl.p, a->causal, pl.wl, pl.wr, (hipStream_t)stream);
    return fa3_launch<T, D>(pl.p, a->causal, route, (hipStream_t)stream);
  });
}

extern "C" int mio_fa3_fwd(const mio_fa3_fwd_params_t* a, void* stream) { return mio_fa3_fwd_window(a, -1, -1, stream); }

// ---- the per-sequence forms: packed variable-length (mio_fa3_fwd_varlen) and over the paged KV cache (mio_fa3_fwd_paged);
// the same kernels for the same head dims (the two route enums have equal values)
static_assert((int)MIO_FA3_PAGED_ROUTE_FWD5 == MIO_FA3_VARLEN_ROUTE_FWD5 && (int)MIO_FA3_PAGED_ROUTE_FWD3 == MIO_FA3_VARLEN_ROUTE_FWD3);

// The per-sequence launch of plan pl (seq: pl.vl or pl.pg) on the kernels with or without a window
template <typename V>
static int fa_seq_launch(const FaPlan& pl, const V& seq, int dtype, int D, int causal, void* stream) {
  return fa_dispatch(dtype, D, [&](auto i) {
    using T = typename decltype(i)::T;
    constexpr int DP = decltype(i)::D;
    if (fa_windowed(pl.wl, pl.wr)) return fa3_win_seq_launch<T, DP>(pl.p, seq, causal, pl.wl, pl.wr, (hipStream_t)stream);
    return fa3_seq_launch<T, DP>(pl.p, seq, causal, (hipStream_t)stream);
  });
}

// packed varlen (mio_fa3_fwd_varlen, mio_fa3_fwd_varlen_window): a mio_fa3_varlen_route_t
static int fa3_varlen_plan(FaPlan& pl, const mio_fa3_varlen_params_t* a, int32_t left, int32_t right) {
  MIO_CHECK(a != nullptr, "mio_fa3_fwd_varlen: null params");
  MIO_CHECK(a->B >= 0 && a->total_q >= 0 && a->total_k >= 0 && a->max_seqlen_q >= 0 && a->max_seqlen_k >= 0 && a->H > 0 &&
                a->Hkv > 0,
            "mio_fa3_fwd_varlen: bad sizes");
  if (fa_check_common("mio_fa3_fwd_varlen", a->H, a->Hkv, a->D, a->dtype, a->softmax_scale) != 0) return -1;
  MIO_CHECK(a->q && a->k && a->v && a->o, "mio_fa3_fwd_varlen: q/k/v/o must be non-null");
  MIO_CHECK(a->B == 0 || (a->cu_seqlens_q != nullptr && a->cu_seqlens_k != nullptr),
            "mio_fa3_fwd_varlen: cu_seqlens_q / cu_seqlens_k must be non-null");
  if (fa_check_packed("mio_fa3_fwd_varlen", {a->q_stride, a->k_stride, a->v_stride, a->o_stride}, {a->q, a->k, a->v, a->o},
                      a->total_q, a->max_seqlen_q) != 0)
    return -1;
  MIO_CHECK(a->total_k == 0 || a->max_seqlen_k >= 1, "mio_fa3_fwd_varlen: max_seqlen_k must be >= 1 when total_k > 0");
  // the pipelined kernels address K / V tiles with 32-bit byte offsets from the sequence's first row
  MIO_CHECK((int64_t)a->max_seqlen_k * a->k_stride[0] * 2 < (1ll << 32) &&
                (int64_t)a->max_seqlen_k * a->v_stride[0] * 2 < (1ll << 32),
            "mio_fa3_fwd_varlen: K / V rows of one sequence must span less than 4 GiB (max_seqlen_k * token stride * 2)");
  if (fa_windowed(left, right) &&
      fa_window_check_packed("mio_fa3_fwd_varlen_window", left, right, a->causal, a->max_seqlen_q, a->max_seqlen_k) != 0)
    return -1;
  if (a->B == 0 || a->total_q == 0) return MIO_FA3_VARLEN_ROUTE_EMPTY;
  fa_plan_window(pl, left, right);

  FaDev& p = pl.p = fa_dev(a->q, a->k, a->v, a->o, a->lse, a->B, a->H, a->Hkv, a->D, a->softmax_scale);
  p.qs_s = a->q_stride[0]; p.qs_h = a->q_stride[1];
  p.ks_s = a->k_stride[0]; p.ks_h = a->k_stride[1];
  p.vs_s = a->v_stride[0]; p.vs_h = a->v_stride[1];
  p.os_s = a->o_stride[0]; p.os_h = a->o_stride[1];
  FaVarlen& vl = pl.vl;
  vl.cu_q = a->cu_seqlens_q; vl.cu_k = a->cu_seqlens_k;
  vl.total_q = a->total_q; vl.total_k = a->total_k;
  vl.max_q = a->max_seqlen_q; vl.max_k = a->max_seqlen_k;
  return fa_pipelined(a->D, MIO_FA3_VARLEN_ROUTE_FWD5, MIO_FA3_VARLEN_ROUTE_FWD3);
}

extern "C" int32_t mio_fa3_varlen_route_window(const mio_fa3_varlen_params_t* a, int32_t window_left, int32_t window_right) {
  FaPlan pl;
  return fa3_varlen_plan(pl, a, window_left, window_right);
}

extern "C" int32_t mio_fa3_varlen_route(const mio_fa3_varlen_params_t* a) { return mio_fa3_varlen_route_window(a, -1, -1); }

extern "C" int mio_fa3_fwd_varlen_window(const mio_fa3_varlen_params_t* a, int32_t window_left, int32_t window_right,
                                         void* stream) {
  FaPlan pl;
  const int route = fa3_varlen_plan(pl, a, window_left, window_right);
  if (route <= MIO_FA3_VARLEN_ROUTE_EMPTY) return route;
  return fa_seq_launch(pl, pl.vl, a->dtype, a->D, a->causal, stream);
}

extern "C" int mio_fa3_fwd_varlen(const mio_fa3_varlen_params_t* a, void* stream) {
  return mio_fa3_fwd_varlen_window(a, -1, -1, stream);
}

// Paged (mio_fa3_fwd_paged, mio_fa3_fwd_paged_window; kv8: mio_fa3_fwd_paged_kv8 over the fp8 (e4m3fn) cache, whose checks
// are these, then the scales and head_dim % 16): a mio_fa3_paged_route_t.  kv8: the cache pointers address bytes.
static int fa3_paged_plan(FaPlan& pl, const mio_fa3_paged_params_t* a, int32_t left, int32_t right, bool kv8 = false,
                          const float* k_scale = nullptr, const float* v_scale = nullptr) {
  MIO_CHECK(a != nullptr, "mio_fa3_fwd_paged: null params");
  MIO_CHECK(a->B >= 0 && a->total_q >= 0 && a->max_seqlen_q >= 0 && a->max_seqlen_k >= 0 && a->H > 0 && a->Hkv > 0,
            "mio_fa3_fwd_paged: bad sizes");
  if (fa_check_common("mio_fa3_fwd_paged", a->H, a->Hkv, a->D, a->dtype, a->softmax_scale) != 0) return -1;
  MIO_CHECK(a->q && a->k_cache && a->v_cache && a->o, "mio_fa3_fwd_paged: q/k_cache/v_cache/o must be non-null");
  MIO_CHECK(a->B == 0 || (a->cu_seqlens_q != nullptr && a->seqused_k != nullptr && a->block_tables != nullptr),
            "mio_fa3_fwd_paged: cu_seqlens_q / seqused_k / block_tables must be non-null");
  MIO_CHECK(a->num_blocks > 0 && a->num_layers > 0 && a->max_blocks_per_seq > 0, "mio_fa3_fwd_paged: bad cache geometry");
  MIO_CHECK(a->layer_idx >= 0 && a->layer_idx < a->num_layers, "mio_fa3_fwd_paged: layer_idx must be in [0, num_layers)");
  MIO_CHECK(a->block_size > 0 && a->block_size % 64 == 0,
            "mio_fa3_fwd_paged: block_size must be a multiple of 64 (a 64-key tile may not span two pages)");
  if (fa_check_packed("mio_fa3_fwd_paged", {a->q_stride, a->o_stride}, {a->q, a->k_cache, a->v_cache, a->o}, a->total_q,
                      a->max_seqlen_q) != 0)
    return -1;
  // the kernels index the cache by a 32-bit row (page, layer, slot) and divide tile indices by a 31-bit reciprocal
  MIO_CHECK((int64_t)a->num_blocks * a->num_layers * a->block_size < (1ll << 32),
            "mio_fa3_fwd_paged: the cache must hold fewer than 2^32 token rows (num_blocks * num_layers * block_size)");
  const int tpb = a->block_size / 64;
  MIO_CHECK((int64_t)a->max_blocks_per_seq * tpb * tpb < (1ll << 31),
            "mio_fa3_fwd_paged: max_blocks_per_seq * (block_size / 64)^2 must be below 2^31");
  if (fa_windowed(left, right) &&
      fa_window_check_packed("mio_fa3_fwd_paged_window", left, right, a->causal, a->max_seqlen_q, a->max_seqlen_k) != 0)
    return -1;
  if (kv8) {
    const char* fn = "mio_fa3_fwd_paged_kv8";
    MIO_CHECK(k_scale != nullptr && v_scale != nullptr,
              std::string(fn) + ": k_scale and v_scale are required with an fp8 cache (null scale pointer)");
    MIO_CHECK(((uintptr_t)k_scale & 3) == 0 && ((uintptr_t)v_scale & 3) == 0, std::string(fn) + ": scales must be 4-byte aligned fp32");
    MIO_CHECK(a->D % 16 == 0, std::string(fn) + ": head_dim must be a multiple of 16 in [16,128] for an fp8 cache");
  }
  if (a->B == 0 || a->total_q == 0) return MIO_FA3_PAGED_ROUTE_EMPTY;
  fa_plan_window(pl, left, right);

  FaDev& p = pl.p = fa_dev(a->q, a->k_cache, a->v_cache, a->o, a->lse, a->B, a->H, a->Hkv, a->D, a->softmax_scale);
  p.qs_s = a->q_stride[0]; p.qs_h = a->q_stride[1];
  // the cache's token and head strides (pages and layers come from the walk); the bodies count 16-bit units, which is half
  // the one-byte row of the fp8 cache
  p.ks_h = p.vs_h = kv8 ? a->D / 2 : a->D;
  p.ks_s = p.vs_s = (int64_t)a->Hkv * p.ks_h;
  p.os_s = a->o_stride[0]; p.os_h = a->o_stride[1];
  FaPaged& pg = pl.pg;
  pg.cu_q = a->cu_seqlens_q; pg.seqused_k = a->seqused_k; pg.block_tables = a->block_tables;
  pg.total_q = a->total_q; pg.max_q = a->max_seqlen_q;
  pg.max_k = (int)std::min<int64_t>(a->max_seqlen_k, (int64_t)a->max_blocks_per_seq * a->block_size);
  pg.num_blocks = a->num_blocks; pg.num_layers = a->num_layers; pg.layer = a->layer_idx;
  pg.block_size = a->block_size; pg.max_blocks = a->max_blocks_per_seq;
  pg.tpb = tpb;
  pg.tpb_magic = (uint32_t)(((1ull << 31) + pg.tpb - 1) / pg.tpb);
  return fa_pipelined(a->D, MIO_FA3_PAGED_ROUTE_FWD5, MIO_FA3_PAGED_ROUTE_FWD3);
}

extern "C" int32_t mio_fa3_paged_route_window(const mio_fa3_paged_params_t* a, int32_t window_left, int32_t window_right) {
  FaPlan pl;
  return fa3_paged_plan(pl, a, window_left, window_right);
}

extern "C" int32_t mio_fa3_paged_route(const mio_fa3_paged_params_t* a) { return mio_fa3_paged_route_window(a, -1, -1); }

extern "C" int mio_fa3_fwd_paged_window(const mio_fa3_paged_params_t* a, int32_t window_left, int32_t window_right,
                                        void* stream) {
  FaPlan pl;
  const int route = fa3_paged_plan(pl, a, window_left, window_right);
  if (route <= MIO_FA3_PAGED_ROUTE_EMPTY) return route;
  return fa_seq_launch(pl, pl.pg, a->dtype, a->D, a->causal, stream);
}

extern "C" int mio_fa3_fwd_paged(const mio_fa3_paged_params_t* a, void* stream) {
  return mio_fa3_fwd_paged_window(a, -1, -1, stream);
}

extern "C" int32_t mio_fa3_paged_kv8_route(const mio_fa3_paged_params_t* a, const float* k_scale, const float* v_scale,
                                           int32_t window_left, int32_t window_right) {
  FaPlan pl;
  return fa3_paged_plan(pl, a, window_left, window_right, true, k_scale, v_scale);
}

// K = x8 * k_scale, V = x8 * v_scale with the layer's fp32 scales, read on the device (fa3_kv8_inst.hip)
extern "C" int mio_fa3_fwd_paged_kv8(const mio_fa3_paged_params_t* a, const float* k_scale, const float* v_scale,
                                     int32_t window_left, int32_t window_right, void* stream) {
  FaPlan pl;
  const int route = fa3_paged_plan(pl, a, window_left, window_right, true, k_scale, v_scale);
  if (route <= MIO_FA3_PAGED_ROUTE_EMPTY) return route;
  return fa_dispatch(a->dtype, a->D, [&](auto i) {
    return fa3_kv8_launch<typename decltype(i)::T, decltype(i)::D>(pl.p, pl.pg, k_scale, v_scale, a->causal, pl.wl, pl.wr,
                                                                    (hipStream_t)stream);
  });
}

"""CPU-only: the refusals of the GEMM / fused-MLP entry points, pinned as literal strings.

Every case is a call that is wrong in exactly one way: `base` with `common` applied is the valid neighbour, `fault` on top of
it is refused with a non-zero return and mio_last_error() equal to the literal, entry-point prefix included.  The neighbour is
judged by the host-only queries (mio_gemm_route, mio_gemm_blocked_weight_ok, mio_gemm_col_scale_ok,
mio_fused_mlp_blocked_weight_ok, mio_gemm_ln_ok); a launch entry point is only called where it launches nothing (a refusal,
or M == 0).  What no host-only query judges runs on the GPU:
  the column range of mio_gemm_bias_act_bw_cs      tests/test_gpu_kernels.py::test_gemm_col_scale
  the column range, flags word and ln_slots of
  mio_gemm_ln_bw                                   tests/test_gpu_kernels.py::test_gemm_ln_fold, ::test_gemm_ln_fold_wide_stream
  mio_weight_block / mio_weight_block_glu          tests/test_gpu_kernels.py::test_fused_mlp_blocked_intermediate,
                                                   ::test_fused_mlp_swiglu_blocked_glu_weight
  mio_ln_fold_weight / mio_ln_stats_reduce         tests/test_gpu_kernels.py::test_gemm_ln_fold, ::test_gemm_ln_fold_wide_stream
The order of the checks is not part of the contract: a doubly-wrong call (PAIRS) is refused with either of its two messages.
Addresses are fake and 16-byte aligned; nothing is dereferenced."""
import pytest
import torch

from test_gemm_route_host import BENCH, STRIDE_MAX

A = 1 << 20        # a fake 16-byte aligned device address
BIG = STRIDE_MAX + 8  # the first row stride the 32-bit per-tile offsets do not take
NONE, GELU, RELU, SWIGLU = 0, 1, 3, 5

# argument order of every entry point (include/mio_hip.h); `stream` is always null
SIG = {
    "mio_gemm_bias_act": "x w bias w_gate bias_gate residual y M N K ldx ldw ldy ldr act dtype",
    "mio_gemm_bias_act_bw": "x wb bias residual y M N K ldx ldy ldr act dtype x_blocked",
    "mio_gemm_bias_act_bw_cs": "x wb bias y M N K ldx ldy act dtype x_blocked cs_lo cs_hi cs_val",
    "mio_gemm_ln_bw": "x wb bias bias_gate residual y M N K ldx ldy ldr act dtype flags ln_stats ln_slots ln_eps stats_out "
                      "cs_lo cs_hi cs_val",
    "mio_fused_mlp_fwd": "x w1 b1 wg bg w2 b2 residual y workspace M d I act dtype",
    "mio_fused_mlp_fwd_bw": "x w1 b1 w2 b2 residual y workspace M d I act dtype x_blocked",
    "mio_fused_mlp_glu_fwd_bw": "x w1 b1 bg w2 b2 residual y workspace M d I dtype x_blocked",
    "mio_weight_block": "w ldw wb N K dtype",
    "mio_weight_block_glu": "w_gate w_up ldw wb N K dtype",
    "mio_ln_fold_weight": "w ldw gamma beta bias w_scaled bias_out N K dtype",
    "mio_ln_stats_reduce": "stats_in slots_in stats_out slots_out M",
    "mio_gemm_route": "M N K ldx ldw ldy ldr act has_residual w_layout fold_in stats_out",
}
LAUNCHES = tuple(n for n in SIG if n != "mio_gemm_route")

_G = dict(M=4096, N=4096, K=1024, act=NONE, dtype=0)  # 16 x 16 tiles of 256 x 256: every blocked-weight form takes it
_MLP = dict(x=A, w1=A, b1=None, w2=A, b2=None, residual=None, y=A, workspace=A, dtype=0)
BASES = {
    "plain": ("mio_gemm_bias_act", dict(x=A, w=A, bias=None, w_gate=None, bias_gate=None, residual=None, y=A, M=37, N=128, K=64,
                                        ldx=64, ldw=64, ldy=128, ldr=0, act=NONE, dtype=0)),
    "bw": ("mio_gemm_bias_act_bw", dict(_G, x=A, wb=A, bias=None, residual=None, y=A, ldx=1024, ldy=4096, ldr=0, x_blocked=0)),
    "cs": ("mio_gemm_bias_act_bw_cs", dict(_G, x=A, wb=A, bias=None, y=A, ldx=1024, ldy=4096, x_blocked=0, cs_lo=0, cs_hi=128,
                                           cs_val=0.5)),
    "ln": ("mio_gemm_ln_bw", dict(_G, x=A, wb=A, bias=None, bias_gate=None, residual=None, y=A, ldx=1024, ldy=4096, ldr=0, flags=0,
                                  ln_stats=None, ln_slots=0, ln_eps=1e-5, stats_out=None, cs_lo=0, cs_hi=0, cs_val=1.0)),
    # both stages on the 256-tile kernels (mio_fused_mlp_blocked_weight_ok == 1)
    "mlp": ("mio_fused_mlp_fwd", dict(_MLP, wg=None, bg=None, M=16384, d=1024, I=4096, act=GELU)),
    "mlp_bw": ("mio_fused_mlp_fwd_bw", dict(_MLP, M=16384, d=1024, I=4096, act=GELU, x_blocked=0)),
    "mlp_glu": ("mio_fused_mlp_glu_fwd_bw", dict(_MLP, bg=None, M=16384, d=1024, I=4096, x_blocked=0)),
    # a shape that takes two mio_gemm_bias_act launches
    "mlp2": ("mio_fused_mlp_fwd", dict(_MLP, wg=None, bg=None, M=300, d=256, I=1024, act=RELU)),
    "wblock": ("mio_weight_block", dict(w=A, ldw=1024, wb=A, N=4096, K=1024, dtype=0)),
    "wglu": ("mio_weight_block_glu", dict(w_gate=A, w_up=A, ldw=1024, wb=A, N=4096, K=1024, dtype=0)),
    "fold": ("mio_ln_fold_weight", dict(w=A, ldw=16384, gamma=A, beta=None, bias=None, w_scaled=A, bias_out=A, N=4096, K=1024,
                                        dtype=0)),
    "reduce": ("mio_ln_stats_reduce", dict(stats_in=A, slots_in=16, stats_out=A, slots_out=8, M=0)),
    "route": ("mio_gemm_route", dict(M=4096, N=4096, K=1024, ldx=1024, ldw=1024, ldy=4096, ldr=0, act=NONE, has_residual=0,
                                     w_layout=0, fold_in=0, stats_out=0)),
}

P, BW, CS, LN = "mio_gemm_bias_act", "mio_gemm_bias_act_bw", "mio_gemm_bias_act_bw_cs", "mio_gemm_ln_bw"
MLP, MLPBW, MLPGLU = "mio_fused_mlp_fwd", "mio_fused_mlp_fwd_bw", "mio_fused_mlp_glu_fwd_bw"
WB, WG, FW, SR, RT = "mio_weight_block", "mio_weight_block_glu", "mio_ln_fold_weight", "mio_ln_stats_reduce", "mio_gemm_route"
_SIZES, _DTYPE, _ALIGN = ": bad sizes", ": dtype must be bf16 or fp16", ": pointers must be 16-byte aligned"
_ACT, _ACTBW, _STRIDES = ": unknown activation", ": unknown / unsupported activation", ": bad strides"
_GATE = P + ": w_gate is required iff act == SWIGLU"
_N8 = ": N and K must be multiples of 8"
_ROW8 = P + ": row strides must be multiples of 8 elements"
_ROWLEN = P + ": row stride smaller than row length"
_BW_LARGE = ": row stride too large for the blocked-weight kernels"
_BW_SHAPE = BW + ": this shape does not take the blocked-weight kernels (mio_gemm_blocked_weight_ok == 0); use " \
    "mio_gemm_bias_act with the plain weight"
_CS_SHAPE = CS + ": this shape does not run the persistent kernel (mio_gemm_col_scale_ok == 0)"
_CS_RANGE = CS + ": [cs_lo, cs_hi) must be multiples of 128 inside [0, N]"
_LN_SHAPE = ": this shape / activation does not take the folded kernels (mio_gemm_ln_ok == 0)"
_LN_SLOTS = LN + ": at most 8 statistic slots (rows wider than 2048 columns: mio_ln_stats_reduce first)"
_LN_RANGE = LN + ": [cs_lo, cs_hi) must be multiples of 128 inside [0, N], without a residual"
_LN_PRODUCER = ": the producer form is the residual epilogue"
_MLP_SHAPE = MLPBW + ": this shape does not take the blocked-weight kernels (mio_fused_mlp_blocked_weight_ok == 0); pass the " \
    "plain weights to mio_fused_mlp_fwd"
_GLU_SHAPE = MLPGLU + ": this shape does not take the 256-tile kernels (mio_fused_mlp_blocked_weight_ok(.., SWIGLU) == 0); " \
    "pass the plain weights to mio_fused_mlp_fwd"
_WB_SIZES = ": need K % 32 == 0, ldw % 8 == 0"
_RT_PAIR = RT + ": the interleaved weight belongs to act == SWIGLU, and SWIGLU has no plain blocked weight"
_RT_SHAPE = RT + ": this shape does not take the blocked-weight kernels (mio_gemm_blocked_weight_ok == 0)"

RES = dict(residual=A, ldr=4096)         # a residual for the 4096-column bases
FOLD = dict(ln_stats=A, ln_slots=4)      # the LayerNorm consumer at K = 1024
STATS = dict(RES, stats_out=A)           # the LayerNorm producer
BADY = dict(y=A + 8)

# (base, common, fault, message): BASES[base] + common is accepted, + fault refused with the message
CASES = [
    # ---- mio_gemm_bias_act
    ("plain", {}, dict(w=None), P + ": x, w, y must be non-null"),
    ("plain", {}, dict(x=None), P + ": x, w, y must be non-null"),
    ("plain", {}, dict(y=None), P + ": x, w, y must be non-null"),
    ("plain", dict(M=0, x=None, y=None), dict(w=None), P + ": x, w, y must be non-null"),
    ("plain", {}, dict(M=-1), P + _SIZES),
    ("plain", {}, dict(N=0), P + _SIZES),
    ("plain", {}, dict(K=0), P + _SIZES),
    ("plain", {}, dict(dtype=2), P + _DTYPE),
    ("plain", dict(M=0), dict(dtype=-1), P + _DTYPE),  # M == 0 returns 0 only after all the checks
    ("plain", {}, dict(act=6), P + _ACT),
    ("plain", {}, dict(act=-1), P + _ACT),
    ("plain", dict(act=SWIGLU, w_gate=A), dict(w_gate=None), _GATE),
    ("plain", {}, dict(w_gate=A), _GATE),
    ("plain", {}, dict(K=60), P + _N8),
    ("plain", {}, dict(N=124), P + _N8),
    ("plain", {}, dict(ldx=68), _ROW8),
    ("plain", {}, dict(ldw=68), _ROW8),
    ("plain", {}, dict(ldy=132), _ROW8),
    ("plain", dict(residual=A, ldr=128), dict(ldr=132), _ROW8),
    ("plain", dict(ldr=132), dict(x=A + 8), P + _ALIGN),             # no residual: its stride is not read
    ("plain", {}, dict(ldx=56), _ROWLEN),
    ("plain", {}, dict(ldw=56), _ROWLEN),
    ("plain", {}, dict(ldy=120), _ROWLEN),
    ("plain", dict(residual=A, ldr=8), dict(w=A + 8), P + _ALIGN),    # the residual's stride may be below N
    ("plain", {}, dict(y=A + 8), P + _ALIGN),
    ("plain", dict(act=SWIGLU, w_gate=A), dict(w_gate=A + 8), P + _ALIGN),
    ("plain", dict(residual=A, ldr=128), dict(residual=A + 8), P + _ALIGN),
    ("plain", dict(bias=A), dict(bias=A + 8), P + _ALIGN),
    ("plain", dict(bias_gate=A), dict(bias_gate=A + 8), P + _ALIGN),
    # ---- mio_gemm_bias_act_bw
    ("bw", {}, dict(x=None), BW + ": x, wb, y must be non-null"),
    ("bw", {}, dict(wb=None), BW + ": x, wb, y must be non-null"),
    ("bw", {}, dict(y=None), BW + ": x, wb, y must be non-null"),
    ("bw", {}, dict(M=-1), BW + _SIZES),
    ("bw", {}, dict(N=0), BW + _SIZES),
    ("bw", {}, dict(K=0), BW + _SIZES),
    ("bw", {}, dict(dtype=2), BW + _DTYPE),
    ("bw", {}, dict(act=SWIGLU), BW + _ACTBW),
    ("bw", {}, dict(act=-1), BW + _ACTBW),
    ("bw", dict(ldy=4104), dict(N=4100), BW + _STRIDES),
    ("bw", {}, dict(ldx=1028), BW + _STRIDES),
    ("bw", {}, dict(ldy=4100), BW + _STRIDES),
    ("bw", RES, dict(ldr=4100), BW + _STRIDES),
    ("bw", {}, dict(ldx=1016), BW + _STRIDES),
    ("bw", {}, dict(ldy=4088), BW + _STRIDES),
    ("bw", dict(residual=A, ldr=8), BADY, BW + _ALIGN),               # the residual's stride may be below N
    ("bw", dict(x_blocked=1, ldx=4), BADY, BW + _ALIGN),              # x_blocked replaces ldx by K before the stride checks
    ("bw", dict(x_blocked=1, ldx=BIG), BADY, BW + _ALIGN),
    ("bw", dict(ldr=BIG + 4), BADY, BW + _ALIGN),                     # no residual: its stride is not read
    ("bw", {}, dict(x=A + 8), BW + _ALIGN),
    ("bw", {}, dict(wb=A + 8), BW + _ALIGN),
    ("bw", RES, dict(residual=A + 8), BW + _ALIGN),
    ("bw", dict(bias=A), dict(bias=A + 8), BW + _ALIGN),
    ("bw", {}, dict(ldx=BIG), BW + _BW_LARGE),
    ("bw", {}, dict(ldy=BIG), BW + _BW_LARGE),
    ("bw", RES, dict(ldr=BIG), BW + _BW_LARGE),
    ("bw", {}, dict(M=1024), _BW_SHAPE),   # 64 tiles
    ("bw", {}, dict(M=0), _BW_SHAPE),      # M == 0 is refused, through the tile predicate
    ("bw", {}, dict(K=96), _BW_SHAPE),     # three K-tiles
    ("bw", dict(ldx=2048), dict(K=1032), _BW_SHAPE),
    # ---- mio_gemm_bias_act_bw_cs
    ("cs", {}, dict(x=None), CS + ": x, wb, y must be non-null"),
    ("cs", {}, dict(wb=None), CS + ": x, wb, y must be non-null"),
    ("cs", {}, dict(y=None), CS + ": x, wb, y must be non-null"),
    ("cs", {}, dict(M=-1), CS + _SIZES),
    ("cs", {}, dict(N=0), CS + _SIZES),
    ("cs", {}, dict(K=0), CS + _SIZES),
    ("cs", {}, dict(dtype=2), CS + _DTYPE),
    ("cs", {}, dict(act=SWIGLU), CS + _ACTBW),
    ("cs", {}, dict(act=6), CS + _ACTBW),
    ("cs", {}, dict(ldx=1028), CS + _STRIDES),
    ("cs", {}, dict(ldy=4100), CS + _STRIDES),
    ("cs", {}, dict(ldx=1016), CS + _STRIDES),
    ("cs", {}, dict(ldy=4088), CS + _STRIDES),
    ("cs", dict(x_blocked=1, ldx=4), BADY, CS + _ALIGN),
    ("cs", {}, dict(x=A + 8), CS + _ALIGN),
    ("cs", {}, dict(wb=A + 8), CS + _ALIGN),
    ("cs", dict(bias=A), dict(bias=A + 8), CS + _ALIGN),
    ("cs", {}, dict(ldx=BIG), CS + ": row stride too large"),
    ("cs", {}, dict(ldy=BIG), CS + ": row stride too large"),
    ("cs", {}, dict(M=1024), _CS_SHAPE),
    ("cs", {}, dict(M=0), _CS_SHAPE),
    ("cs", {}, dict(K=128), _CS_SHAPE),    # mio_gemm_blocked_weight_ok takes K = 128, the column scale asks K >= 256
    ("cs", dict(ldx=2048), dict(K=1056), _CS_SHAPE),  # ... and K % 64 == 0
    ("cs", dict(ldy=4104), dict(N=4100), _CS_SHAPE),
    ("cs", {}, dict(cs_lo=-128), _CS_RANGE),
    ("cs", {}, dict(cs_hi=4224), _CS_RANGE),
    ("cs", {}, dict(cs_lo=64), _CS_RANGE),
    ("cs", {}, dict(cs_hi=192), _CS_RANGE),
    ("cs", {}, dict(cs_lo=256), _CS_RANGE),  # cs_lo > cs_hi
    # ---- mio_gemm_ln_bw
    ("ln", {}, dict(x=None), LN + ": x, wb, y must be non-null"),
    ("ln", {}, dict(wb=None), LN + ": x, wb, y must be non-null"),
    ("ln", {}, dict(y=None), LN + ": x, wb, y must be non-null"),
    ("ln", dict(M=0), dict(x=None), LN + ": x, wb, y must be non-null"),
    ("ln", {}, dict(M=-1), LN + _SIZES),
    ("ln", {}, dict(N=0), LN + _SIZES),
    ("ln", dict(M=0), dict(K=0), LN + _SIZES),
    ("ln", {}, dict(dtype=2), LN + _DTYPE),
    ("ln", {}, dict(act=6), LN + _ACT),
    ("ln", {}, dict(flags=8), LN + ": unknown flag"),
    ("ln", {}, dict(bias_gate=A), LN + ": bias_gate belongs to the gated stage (act == SWIGLU)"),
    ("ln", dict(act=SWIGLU, ldr=4096), dict(residual=A), LN + ": the gated stage takes no residual"),
    ("ln", dict(act=SWIGLU, bias_gate=A), dict(bias_gate=A + 8), LN + _ALIGN),
    ("ln", {}, dict(M=1024), LN + _LN_SHAPE),
    ("ln", FOLD, dict(K=992), LN + _LN_SHAPE),          # the consumer needs K % 256 == 0
    ("ln", STATS, dict(act=GELU), LN + _LN_SHAPE),      # the producer has no activation
    ("ln", dict(act=SWIGLU), dict(N=4160, ldy=4160), LN + _LN_SHAPE),  # the gated stage needs N % 128 == 0
    ("ln", dict(FOLD, ldr=4096), dict(residual=A), LN + ": the consumer form takes no residual"),
    ("ln", FOLD, dict(ln_slots=9), _LN_SLOTS),
    ("ln", FOLD, dict(ln_slots=-1), _LN_SLOTS),
    ("ln", dict(ln_stats=A, ln_slots=8, K=4096, ldx=4096), dict(ln_slots=0), _LN_SLOTS),  # ln_slots == 0 means K / 256
    ("ln", dict(ln_stats=A, ln_slots=0), BADY, LN + _ALIGN),
    ("ln", dict(ln_slots=9), BADY, LN + _ALIGN),       # no ln_stats: ln_slots is not read
    ("ln", STATS, dict(residual=None), LN + _LN_PRODUCER),
    ("ln", dict(RES, flags=4), dict(residual=None), LN + ": RES_BLOCKED without a residual"),
    ("ln", {}, dict(ldx=1028), LN + _STRIDES),
    ("ln", {}, dict(ldy=4100), LN + _STRIDES),
    ("ln", RES, dict(ldr=4100), LN + _STRIDES),
    ("ln", {}, dict(ldx=1016), LN + _STRIDES),
    ("ln", {}, dict(ldy=4088), LN + _STRIDES),
    ("ln", RES, dict(ldr=4088), LN + _STRIDES),
    ("ln", dict(flags=1, ldx=4), BADY, LN + _ALIGN),    # a blocked operand's stride is replaced by its row length
    ("ln", dict(flags=2, ldy=4), BADY, LN + _ALIGN),
    ("ln", dict(RES, flags=4, ldr=BIG + 4), BADY, LN + _ALIGN),
    ("ln", {}, dict(ldx=BIG), LN + ": row stride too large"),
    ("ln", {}, dict(ldy=BIG), LN + ": row stride too large"),
    ("ln", RES, dict(ldr=BIG), LN + ": row stride too large"),
    ("ln", {}, dict(x=A + 8), LN + _ALIGN),
    ("ln", {}, dict(wb=A + 8), LN + _ALIGN),
    ("ln", RES, dict(residual=A + 8), LN + _ALIGN),
    ("ln", dict(bias=A), dict(bias=A + 8), LN + _ALIGN),
    ("ln", FOLD, dict(ln_stats=A + 8), LN + _ALIGN),
    ("ln", STATS, dict(stats_out=A + 8), LN + _ALIGN),
    ("ln", dict(cs_hi=128, ldr=4096), dict(residual=A), _LN_RANGE),
    ("ln", dict(cs_hi=128), dict(cs_lo=-128), _LN_RANGE),
    ("ln", dict(cs_hi=128), dict(cs_hi=4224), _LN_RANGE),
    ("ln", dict(cs_hi=128), dict(cs_lo=64), _LN_RANGE),
    ("ln", dict(cs_hi=128), dict(cs_hi=192), _LN_RANGE),
    ("ln", dict(RES, cs_lo=192, cs_hi=64), BADY, LN + _ALIGN),  # cs_lo >= cs_hi: off, whatever the values
    # ---- the fused MLP on the 256-tile kernels: all three entry points report as mio_fused_mlp_fwd
    ("mlp", {}, dict(workspace=None), MLP + ": workspace must be non-null"),
    ("mlp", {}, dict(act=NONE), MLP + ": an activation is required"),
    ("mlp", {}, dict(x=None), MLP + ": x, w1, w2, y must be non-null"),
    ("mlp", {}, dict(w1=None), MLP + ": x, w1, w2, y must be non-null"),
    ("mlp", {}, dict(w2=None), MLP + ": x, w1, w2, y must be non-null"),
    ("mlp", {}, dict(y=None), MLP + ": x, w1, w2, y must be non-null"),
    ("mlp", {}, dict(dtype=2), MLP + _DTYPE),
    ("mlp", {}, dict(x=A + 8), MLP + _ALIGN),
    ("mlp", {}, dict(w1=A + 8), MLP + _ALIGN),
    ("mlp", {}, dict(w2=A + 8), MLP + _ALIGN),
    ("mlp", {}, dict(y=A + 8), MLP + _ALIGN),
    ("mlp", dict(b1=A), dict(b1=A + 8), MLP + _ALIGN),
    ("mlp", dict(b2=A), dict(b2=A + 8), MLP + _ALIGN),
    ("mlp", dict(residual=A), dict(residual=A + 8), MLP + _ALIGN),
    ("mlp", {}, dict(workspace=A + 8), MLP + _ALIGN),
    ("mlp_bw", {}, dict(workspace=None), MLP + ": workspace must be non-null"),
    ("mlp_bw", {}, dict(act=NONE), MLP + ": an activation is required"),
    ("mlp_bw", dict(x_blocked=1), dict(w2=None), MLP + ": x, w1, w2, y must be non-null"),
    ("mlp_bw", {}, dict(dtype=-1), MLP + _DTYPE),
    ("mlp_bw", dict(x_blocked=1), dict(y=A + 8), MLP + _ALIGN),
    ("mlp_bw", {}, dict(M=300), _MLP_SHAPE),
    ("mlp_bw", {}, dict(M=0), _MLP_SHAPE),
    ("mlp_bw", dict(x_blocked=1), dict(d=1056), _MLP_SHAPE),   # d % 64
    ("mlp_bw", {}, dict(I=4224), _MLP_SHAPE),                  # I % 256
    ("mlp_glu", {}, dict(bg=A + 8), MLPGLU + _ALIGN),
    ("mlp_glu", {}, dict(M=300), _GLU_SHAPE),
    ("mlp_glu", {}, dict(I=4224), _GLU_SHAPE),
    ("mlp_glu", {}, dict(M=0), _MLP_SHAPE),                    # as found: M == 0 passes the gated check and fails the shared one
    ("mlp_glu", {}, dict(workspace=None), MLP + ": workspace must be non-null"),
    ("mlp_glu", dict(x_blocked=1), dict(x=None), MLP + ": x, w1, w2, y must be non-null"),
    ("mlp_glu", {}, dict(dtype=2), MLP + _DTYPE),
    ("mlp_glu", dict(b1=A), dict(b1=A + 8), MLP + _ALIGN),
    # ---- the fused MLP as two mio_gemm_bias_act launches: stage 1's refusals come under that prefix
    ("mlp2", {}, dict(workspace=None), MLP + ": workspace must be non-null"),
    ("mlp2", {}, dict(act=NONE), MLP + ": an activation is required"),
    ("mlp2", {}, dict(x=None), P + ": x, w, y must be non-null"),
    ("mlp2", {}, dict(w1=None), P + ": x, w, y must be non-null"),
    ("mlp2", {}, dict(I=0), P + _SIZES),
    ("mlp2", {}, dict(dtype=2), P + _DTYPE),
    ("mlp2", {}, dict(act=6), P + _ACT),
    ("mlp2", dict(act=SWIGLU, wg=A), dict(wg=None), _GATE),
    ("mlp2", {}, dict(wg=A), _GATE),
    ("mlp2", {}, dict(d=252), P + _N8),
    ("mlp2", {}, dict(x=A + 8), P + _ALIGN),
    ("mlp2", dict(b1=A), dict(b1=A + 8), P + _ALIGN),
    ("mlp", dict(act=SWIGLU, wg=A), dict(x=None), P + ": x, w, y must be non-null"),  # SwiGLU on plain weights: two launches
    # ---- the one-time weight preparations
    ("wblock", {}, dict(w=None), WB + ": w and wb must be non-null"),
    ("wblock", {}, dict(wb=None), WB + ": w and wb must be non-null"),
    ("wblock", {}, dict(dtype=2), WB + _DTYPE),
    ("wblock", {}, dict(N=0), WB + _WB_SIZES),
    ("wblock", {}, dict(K=0), WB + _WB_SIZES),
    ("wblock", {}, dict(K=48), WB + _WB_SIZES),
    ("wblock", {}, dict(ldw=1016), WB + _WB_SIZES),
    ("wblock", {}, dict(ldw=1028), WB + _WB_SIZES),
    ("wblock", {}, dict(w=A + 8), WB + _ALIGN),
    ("wblock", {}, dict(wb=A + 8), WB + _ALIGN),
    ("wglu", {}, dict(w_gate=None), WG + ": w_gate, w_up and wb must be non-null"),
    ("wglu", {}, dict(w_up=None), WG + ": w_gate, w_up and wb must be non-null"),
    ("wglu", {}, dict(wb=None), WG + ": w_gate, w_up and wb must be non-null"),
    ("wglu", {}, dict(dtype=2), WG + _DTYPE),
    ("wglu", {}, dict(N=0), WG + _WB_SIZES),
    ("wglu", {}, dict(K=0), WG + _WB_SIZES),
    ("wglu", {}, dict(K=48), WG + _WB_SIZES),
    ("wglu", {}, dict(ldw=1016), WG + _WB_SIZES),
    ("wglu", {}, dict(ldw=1028), WG + _WB_SIZES),
    ("wglu", {}, dict(w_gate=A + 8), WG + _ALIGN),
    ("wglu", {}, dict(w_up=A + 8), WG + _ALIGN),
    ("wglu", {}, dict(wb=A + 8), WG + _ALIGN),
    ("fold", {}, dict(w=None), FW + ": w, gamma, w_scaled, bias_out must be non-null"),
    ("fold", {}, dict(gamma=None), FW + ": w, gamma, w_scaled, bias_out must be non-null"),
    ("fold", {}, dict(w_scaled=None), FW + ": w, gamma, w_scaled, bias_out must be non-null"),
    ("fold", {}, dict(bias_out=None), FW + ": w, gamma, w_scaled, bias_out must be non-null"),
    ("fold", {}, dict(dtype=2), FW + _DTYPE),
    ("fold", {}, dict(N=0), FW + ": bad sizes (K <= 8192)"),
    ("fold", {}, dict(K=0), FW + ": bad sizes (K <= 8192)"),
    ("fold", {}, dict(K=8200), FW + ": bad sizes (K <= 8192)"),
    ("fold", {}, dict(ldw=1016), FW + ": bad sizes (K <= 8192)"),
    ("reduce", {}, dict(stats_in=None), SR + ": null pointer"),
    ("reduce", {}, dict(stats_out=None), SR + ": null pointer"),
    ("reduce", {}, dict(slots_in=0), SR + ": slots_in must be a multiple of slots_out"),
    ("reduce", {}, dict(slots_out=0), SR + ": slots_in must be a multiple of slots_out"),
    ("reduce", {}, dict(slots_in=12), SR + ": slots_in must be a multiple of slots_out"),
    ("reduce", {}, dict(M=-1), SR + ": slots_in must be a multiple of slots_out"),
    # ---- mio_gemm_route
    ("route", {}, dict(M=-1), RT + _SIZES),
    ("route", {}, dict(N=0), RT + _SIZES),
    ("route", {}, dict(K=0), RT + _SIZES),
    ("route", {}, dict(act=6), RT + _ACT),
    ("route", {}, dict(act=-1), RT + _ACT),
    ("route", {}, dict(w_layout=3), RT + ": w_layout must be 0 (row-major), 1 (blocked) or 2 (gate / up interleaved)"),
    ("route", {}, dict(w_layout=-1), RT + ": w_layout must be 0 (row-major), 1 (blocked) or 2 (gate / up interleaved)"),
    ("route", {}, dict(w_layout=2), _RT_PAIR),
    ("route", dict(w_layout=1), dict(act=SWIGLU), _RT_PAIR),
    ("route", {}, dict(N=4092), RT + _N8),
    ("route", {}, dict(K=1020), RT + _N8),
    ("route", {}, dict(ldx=1028), RT + _STRIDES),
    ("route", {}, dict(ldw=1028), RT + _STRIDES),
    ("route", {}, dict(ldy=4100), RT + _STRIDES),
    ("route", dict(has_residual=1, ldr=4096), dict(ldr=4100), RT + _STRIDES),
    ("route", {}, dict(ldx=1016), RT + _STRIDES),
    ("route", {}, dict(ldw=1016), RT + _STRIDES),
    ("route", {}, dict(ldy=4088), RT + _STRIDES),
    ("route", dict(w_layout=1), dict(ldw=1016), RT + _STRIDES),  # as found: a blocked weight's ldw is still checked as given
    ("route", {}, dict(fold_in=1), RT + ": the LayerNorm forms take a blocked weight"),
    ("route", dict(has_residual=1, ldr=4096), dict(stats_out=1), RT + ": the LayerNorm forms take a blocked weight"),
    ("route", dict(w_layout=1), dict(ldx=BIG), RT + _BW_LARGE),
    ("route", dict(w_layout=1), dict(ldy=BIG), RT + _BW_LARGE),
    ("route", dict(w_layout=1, has_residual=1, ldr=4096), dict(ldr=BIG), RT + _BW_LARGE),
    ("route", dict(w_layout=1, fold_in=1), dict(M=1024), RT + _LN_SHAPE),
    ("route", dict(w_layout=2, act=SWIGLU), dict(M=1024), RT + _LN_SHAPE),
    ("route", dict(w_layout=1, has_residual=1, ldr=4096, stats_out=1), dict(act=GELU), RT + _LN_SHAPE),
    ("route", dict(w_layout=1, fold_in=1, ldr=4096), dict(has_residual=1), RT + ": the consumer and gated forms take no residual"),
    ("route", dict(w_layout=2, act=SWIGLU, ldr=4096), dict(has_residual=1), RT + ": the consumer and gated forms take no residual"),
    ("route", dict(w_layout=1, has_residual=1, ldr=4096, stats_out=1), dict(has_residual=0), RT + _LN_PRODUCER),
    ("route", dict(w_layout=1), dict(M=1024), _RT_SHAPE),
    ("route", dict(w_layout=1), dict(K=96), _RT_SHAPE),
]

# doubly-wrong calls (base, common, fault, fault): refused, with the message either fault gets alone
PAIRS = [
    ("plain", {}, dict(dtype=2), dict(act=6)),
    ("plain", {}, dict(K=60), dict(x=A + 8)),
    ("plain", {}, dict(ldx=68), dict(ldy=120)),
    ("plain", {}, dict(w=None), dict(N=0)),
    ("bw", {}, dict(act=SWIGLU), dict(ldx=1028)),
    ("bw", {}, dict(ldx=BIG), dict(M=1024)),
    ("bw", {}, dict(x=None), dict(dtype=2)),
    ("bw", {}, dict(wb=A + 8), dict(M=0)),
    ("cs", {}, dict(K=128), dict(cs_lo=64)),
    ("cs", {}, dict(ldy=BIG), dict(cs_hi=192)),
    ("cs", {}, dict(dtype=2), dict(ldx=1016)),
    ("ln", {}, dict(flags=8), dict(act=6)),
    ("ln", {}, dict(dtype=2), dict(M=1024)),
    ("ln", {}, dict(bias_gate=A), dict(ldx=1028)),
    ("ln", FOLD, dict(ln_slots=9), dict(x=A + 8)),
    ("ln", dict(cs_hi=128), dict(cs_lo=64), dict(ldy=BIG)),
    ("ln", STATS, dict(act=GELU), dict(stats_out=A + 8)),
    ("mlp", {}, dict(workspace=None), dict(act=NONE)),
    ("mlp", {}, dict(x=None), dict(dtype=2)),
    ("mlp_bw", {}, dict(dtype=2), dict(y=A + 8)),
    ("mlp_glu", {}, dict(bg=A + 8), dict(M=300)),
    ("mlp2", {}, dict(dtype=2), dict(x=A + 8)),
    ("wblock", {}, dict(dtype=2), dict(K=48)),
    ("route", {}, dict(w_layout=3), dict(N=4092)),
    ("route", {}, dict(fold_in=1), dict(ldx=1028)),
    ("route", dict(w_layout=1), dict(ldx=BIG), dict(M=1024)),
    ("route", dict(w_layout=1, fold_in=1, ldr=4096), dict(has_residual=1), dict(M=1024)),
]

# calls that are accepted and launch nothing: (base, changes, return value)
EMPTY = [
    ("plain", dict(M=0), 0),
    ("plain", dict(M=0, x=None, y=None), 0),
    ("ln", dict(M=0), 0),
    ("ln", dict(M=0, dtype=2), 0),               # M == 0 returns right after the null and size checks
    ("ln", dict(M=0, flags=8, act=6, ldx=4), 0),
    ("mlp2", dict(M=0, workspace=None, x=None, y=None), 0),
    ("mlp", dict(M=0, workspace=None, x=None, y=None), 0),
    ("reduce", {}, 0),
    ("route", dict(M=0), 0),                     # MIO_GEMM_ROUTE_EMPTY
    ("route", dict(M=0, w_layout=1, ldx=BIG), 0),  # ... before the blocked-weight forms' stride limit
    ("route", dict(M=0, w_layout=1, fold_in=1), 0),
]


def _L():
    from mio import _lib
    return _lib


def _call(base, *changes):
    name, args = BASES[base]
    args = dict(args)
    for c in changes:
        args.update(c)
    names = SIG[name].split()
    assert set(args) == set(names), (name, set(args) ^ set(names))
    fn = getattr(_L().lib, name)
    vals = [args[n] for n in names]
    return fn(*vals) if name == RT else fn(*vals, None)


def _err():
    return _L().lib.mio_last_error().decode()


def _route(M, N, K, ldx, ldw, ldy, ldr, act, res, w, fold=0, stats=0):
    return _L().lib.mio_gemm_route(M, N, K, ldx, ldw, ldy, ldr, act, int(bool(res)), w, int(bool(fold)), int(bool(stats)))


def _judge(base, *changes):
    """The valid neighbour, by the host-only queries: what would launch is never called."""
    lib = _L().lib
    name, args = BASES[base]
    a = dict(args)
    for c in changes:
        a.update(c)
    if name == RT or (name in (P, LN, SR) and a["M"] == 0) or (name == MLP and a["M"] == 0):
        assert _call(base, *changes) >= 0, _err()
        if name != LN:
            return
    if name == P:
        assert _route(a["M"], a["N"], a["K"], a["ldx"], a["ldw"], a["ldy"], a["ldr"], a["act"], a["residual"], 0) >= 0, _err()
        assert _call(base, *changes, dict(M=0)) == 0, _err()
    elif name in (BW, CS):
        ok = lib.mio_gemm_col_scale_ok if name == CS else lib.mio_gemm_blocked_weight_ok
        assert ok(a["M"], a["N"], a["K"], a["act"]) == 1
        ldx = a["K"] if a["x_blocked"] else a["ldx"]
        res = a.get("residual")
        assert _route(a["M"], a["N"], a["K"], ldx, a["K"], a["ldy"], a.get("ldr", 0), a["act"], res, 1) >= 0, _err()
    elif name == LN:
        if a["M"] == 0:
            return
        fold, stats = a["ln_stats"] is not None, a["stats_out"] is not None
        assert lib.mio_gemm_ln_ok(a["M"], a["N"], a["K"], a["act"], int(fold), int(stats)) == 1
        ldx = a["K"] if a["flags"] & 1 else a["ldx"]
        ldy = a["N"] if a["flags"] & 2 else a["ldy"]
        ldr = a["N"] if a["flags"] & 4 else a["ldr"]
        w = 2 if a["act"] == SWIGLU else 1
        assert _route(a["M"], a["N"], a["K"], ldx, a["K"], ldy, ldr, a["act"], a["residual"], w, fold, stats) >= 0, _err()
    elif name in (MLP, MLPBW, MLPGLU):
        M, d, I = a["M"], a["d"], a["I"]
        act = a.get("act", SWIGLU)
        blocked = lib.mio_fused_mlp_blocked_weight_ok(M, d, I, act) == 1
        if name != MLP:
            assert blocked
        w2 = 0 if name == MLP else 1
        w1 = w2 if act != SWIGLU else 2 * w2
        if not blocked or (act == SWIGLU and w2 == 0):
            w1 = w2 = 0
        assert _route(M, I, d, d, d, I, 0, act, False, w1) >= 0, _err()
        assert _route(M, d, I, I, I, d, d, NONE, a["residual"], w2) >= 0, _err()
    # mio_weight_block, mio_weight_block_glu, mio_ln_fold_weight: no host-only query (GPU tests of the module docstring)


def _id(c):
    base, common = c[:2]
    faults = [f for f in c[2:] if isinstance(f, dict)]
    txt = lambda d: ",".join(f"{k}={v if not isinstance(v, int) or v < A else 'A+%d' % (v - A)}" for k, v in d.items())
    return f"{base}[{txt(common)}]" + "".join("-" + txt(f) for f in faults)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_gemm_refusal_and_valid_neighbour(case):
    lib = _L().lib
    base, common, fault, msg = case
    assert fault and msg.startswith("mio_")
    _judge(base, common)
    assert lib.mio_fa3_route(None) < 0  # a refusal of another family in between: the message read below is this call's own
    assert _call(base, common, fault) != 0
    assert _err() == msg


@pytest.mark.parametrize("case", PAIRS, ids=_id)
def test_gemm_doubly_wrong_call_is_refused_with_either_message(case):
    base, common, f1, f2 = case
    singles = []
    for f in (f1, f2):
        assert _call(base, common, f) != 0
        singles.append(_err())
    assert singles[0] != singles[1]
    _judge(base, common)
    assert _L().lib.mio_fa3_route(None) < 0
    assert _call(base, common, f1, f2) != 0
    assert _err() in singles


@pytest.mark.parametrize("case", EMPTY, ids=lambda c: f"{c[0]}[{','.join(f'{k}={v}' for k, v in c[1].items())}]")
def test_gemm_calls_that_launch_nothing(case):
    base, changes, want = case
    assert _call(base, changes) == want, _err()


def test_every_gemm_entry_point_is_covered():
    L = _L()
    used = {BASES[c[0]][0] for c in CASES}
    assert used == set(SIG)
    for name in SIG:
        assert name in L.EXPORTS and len(getattr(L.lib, name).argtypes) == len(SIG[name].split()) + (name != RT)
        assert name in {c[3].split(":")[0] for c in CASES if BASES[c[0]][0] == name}
    assert any(c[3] == _MLP_SHAPE for c in CASES)
    assert len(PAIRS) >= 12


# ---- launch and route agreement ----------------------------------------------------------------------------------------
# test_gemm_route_host.py's tile-count boundary, K-rule and stride-limit cases: (M, N, K, ldx, ldy, ldr)
_T = 256 * 16
SHAPES = [(255 * 256, 256, 1024), (256 * 256, 256, 1024), (255 * 256 + 1, 256, 1024), (_T, _T - 248, 1024), (_T, 15 * 256 + 8, 1024),
          (_T, 15 * 256, 1024), (1, 65536, 1024), (1, 65536 - 256, 1024), (65536, 8, 1024), (65536 - 256, 8, 1024),
          (255 * 256, 256, 40)] + [(_T, _T, K) for K in (96, 128, 64, 8, 40, 264, 256, 136, 160)]
AGREE = [(n, *BENCH[n][0], None, None, None) for n in sorted(BENCH)]
AGREE += [(f"{M}x{N}x{K}-act{act}-{form}", M, N, K, act, form == "stats", 2 if act == SWIGLU else 1, form == "fold",
           form == "stats", None, None, None)
          for M, N, K in SHAPES for act, form in ((NONE, "bw"), (GELU, "bw"), (NONE, "fold"), (GELU, "fold"), (NONE, "stats"),
                                                  (SWIGLU, "glu"), (SWIGLU, "fold"))]
AGREE += [(f"stride-{which}-{ld}", _T, _T, 1024, NONE, which == "ldr", 1, False, False,
           ld if which == "ldx" else None, ld if which == "ldy" else None, ld if which == "ldr" else None)
          for which in ("ldx", "ldy", "ldr") for ld in (STRIDE_MAX, BIG)]


@pytest.mark.parametrize("case", AGREE, ids=lambda c: c[0])
def test_launch_gate_and_route_agree(case):
    """The *_ok query that gates a blocked-weight launch entry point (with that entry point's stride limit) and mio_gemm_route
    under the matching w_layout: both accept or both refuse."""
    lib = _L().lib
    _, M, N, K, act, res, w, fold, stats, ldx, ldy, ldr = case
    ldx, ldy, ldr = ldx or K, ldy or N, (ldr or N) if res else 0
    w = w or 1  # the benchmark's plain-weight GEMMs: the same shapes take the blocked weight
    if fold or stats or act == SWIGLU:
        gate = lib.mio_gemm_ln_ok(M, N, K, act, int(fold), int(stats))
    elif "col_scale" in case[0]:
        gate = lib.mio_gemm_col_scale_ok(M, N, K, act)
    else:
        gate = lib.mio_gemm_blocked_weight_ok(M, N, K, act)
    gate = gate == 1 and max(ldx, ldy, ldr) * 512 < 0x7fffffff
    r = _route(M, N, K, ldx, K, ldy, ldr, act, res, w, fold, stats)
    assert (r >= 0) == gate, (r, gate, _err())
    if r >= 0:
        assert _L().GEMM_ROUTES[r].startswith("p8w")


def test_route_and_gates_at_m_zero_as_found():
    """M == 0: mio_gemm_route answers "empty" for every weight layout while every *_ok query answers 0.  mio_gemm_bias_act and
    mio_gemm_ln_bw return 0 (EMPTY above), mio_gemm_bias_act_bw / _bw_cs refuse (CASES)."""
    lib = _L().lib
    for w, act, fold in ((0, NONE, 0), (1, NONE, 0), (1, NONE, 1), (2, SWIGLU, 0)):
        assert _route(0, 1024, 1024, 1024, 1024, 1024, 0, act, False, w, fold) == 0
    assert lib.mio_gemm_blocked_weight_ok(0, 1024, 1024, NONE) == 0 and lib.mio_gemm_col_scale_ok(0, 1024, 1024, NONE) == 0
    assert lib.mio_gemm_ln_ok(0, 1024, 1024, NONE, 1, 0) == 0 and lib.mio_fused_mlp_blocked_weight_ok(0, 1024, 4096, GELU) == 0


def test_col_scale_route_gap_as_found():
    """Known gap: mio_gemm_col_scale_ok also asks K >= 256 and K % 64 == 0, and mio_gemm_route has no column-scale
    argument, so the route query names a kernel for a column-scale call the launch refuses."""
    from mio import ops
    lib = _L().lib
    assert lib.mio_gemm_blocked_weight_ok(_T, _T, 128, NONE) == 1 and lib.mio_gemm_col_scale_ok(_T, _T, 128, NONE) == 0
    x, w = (torch.empty(_T, 128, dtype=torch.bfloat16, device="meta") for _ in range(2))
    assert ops.gemm_route(x, w, w_blocked=w, col_scale=(0, 128, 0.5)) == "p8w"
    assert _call("cs", dict(K=128, ldx=128)) != 0 and _err() == _CS_SHAPE

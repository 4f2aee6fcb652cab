"""Hostile memory around every operand of the GEMM family (a plain helper module, not a conftest), after tests/_hostile.py.

mio_gemm_bias_act, its blocked-weight forms (_bw, _bw_cs), mio_gemm_ln_bw / mio_gemm_rms_bw, the three fused-MLP forwards and
the weight preparations are launched on operands that are views into larger buffers, three times at the same addresses, with
the bytes the launch has no business with holding
  benign   finite randn,
  nan      0xFF in every byte (a NaN in bf16 / fp16 / fp32 / e4m3fn),
  huge     finfo(dtype).max / 8 with random signs in 16-bit buffers, 1e30 in fp32 buffers (statistics, scales), +-448 in e4m3fn
           weight bytes.
0 x finite = 0, so a kernel that lets a value it does not own into a product or a sum -- a chunk past K against the zero
filled tail, a padding row of a blocked operand, a statistics slot it was not given -- computes the right numbers on
`benign` and NaN on `nan`.  fmaxf / v_max drop a NaN operand, so a value that only enters the variance clamp of the fold
consumer is invisible to `nan`; `huge` is for that.

OWNERSHIP, from the contract in include/mio_hip.h and the docstrings of mio.ops (not from kernel code).  Owned inputs:
  x[m, k], m < M, k < K (row-major at m * ldx + k; blocked at the blocked-layout offset of (m, k));
  w[n, k], w_gate[n, k], n < N, k < K;  a prepared weight (mio_weight_block, mio_weight_block_glu, mio_ln_fold_weight): the
  whole prepared buffer -- every case prepares it, under each fill, from a source that sits in hostile memory itself, so the
  prepared bytes are an owned OUTPUT of the case as well;
  bias[n], bias_gate[n], gamma[k], beta[k];  residual[m, n], m < M, n < N;
  ln_stats[s][m][0..1], s < ln_slots, m < M -- under mio_gemm_rms_bw only entry [1], the sum of squares.
Not owned, by class (CLASS_NAMES; every failure names the classes that reach the result):
  past K        columns K .. ld of x, w, w_gate (and of an e4m3fn weight)
  past N        columns N .. ld of the residual and of y; the elements around a bias, a scale, gamma, beta
  guard row     rows in front of row 0 and rows >= M (x, residual, y) or >= N (weights) of the enclosing buffer; the elements
                around a blocked operand, a prepared weight, a statistics buffer
  padding row   rows M .. ceil(M / 256) * 256 of a blocked x, a blocked residual, a blocked y and of every statistics slot
  spare slot    statistics slots >= ln_slots
  rms sum entry the sums of the statistics under mio_gemm_rms_bw
  workspace     the pre-fill of a fused-MLP workspace and the bytes around it
Owned outputs: y[m, n], m < M, n < N; stats_out rows < M; the prepared weights.  What the kernels do with the rest
(include/mio_hip.h states it): the padding rows of a blocked y are NOT written (csrc/gemm8w_kernel.h predicates every output
store on the row being < M) and are held to their pre-fill; the rows M .. ceil(M / 256) * 256 of every stats_out slot ARE
written -- the producer stores all 256 rows of a tile, those past M holding statistics of clamped, owned rows -- so they must
not depend on the fill either and are compared bit for bit, but against no reference; mio_ln_stats_reduce sums the padding
rows of its input into the padding rows of its output, which are therefore written with unspecified values (SCRATCH: not
compared, not held to the pre-fill).  The inside of a workspace is scratch as well.

judge(run, built): see its docstring.  Model is the torch model of these launch forms that tests/test_hostile_gemm_host.py
proves the harness on, clean and with planted defects.
"""
from __future__ import annotations

from dataclasses import dataclass, field, replace
from typing import Dict, Optional, Tuple

import torch

import _gemm_check as gc
import _rms_check as rc
from _hostile import FILLS, HostileFailure, bits, blocked_index  # noqa: F401  (FILLS: re-exported)

(OWNED, PAST_K, PAST_N, GUARD_ROW, PAD_ROW, SPARE_SLOT, RMS_SUM, WORKSPACE) = range(8)
CLASS_NAMES = {PAST_K: "past K", PAST_N: "past N", GUARD_ROW: "guard row", PAD_ROW: "padding row", SPARE_SLOT: "spare slot",
               RMS_SUM: "rms sum entry", WORKSPACE: "workspace"}
G_ROWS = 256  # guard rows on each side of a row-major operand: a whole row tile of the widest kernel past M or N is poison
G_1D = 8      # guard elements on each side of a 1-D or blocked buffer (16 bytes of a 16-bit type: pointers stay aligned)
PAD_LD = 72   # elements between the row length and the row stride: a whole 64-k step behind K is poison, not the next row
EPS = 1e-5
ROUTES = ("t128", "t256", "p8w", "p8w_res", "p8w_fold", "p8w_stats", "glu_t128x64", "glu_t256x128", "p8w_glu", "p8w_glu_fold")
ENTRY_POINTS = ("mio_gemm_bias_act", "mio_gemm_bias_act_bw", "mio_gemm_bias_act_bw_cs", "mio_gemm_ln_bw", "mio_gemm_rms_bw",
                "mio_fused_mlp_fwd", "mio_fused_mlp_fwd_bw", "mio_fused_mlp_glu_fwd_bw", "mio_weight_block",
                "mio_weight_block_glu", "mio_ln_fold_weight", "mio_weight_quant_w8", "mio_ln_stats_reduce")


def _names(classes):
    return tuple(CLASS_NAMES[c] for c in classes)


# ---- cases -------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    kind: str                   # gemm | mlp | prep
    entry: str                  # the C entry point the case launches (one of ENTRY_POINTS)
    route: str                  # gemm: the route mio_gemm_route must name; mlp: "path/stage1/stage2"; prep: ""
    M: int
    N: int                      # mlp: I
    K: int                      # mlp: d
    classes: Tuple[int, ...]    # the not-owned classes the case claims (tests/test_hostile_gemm_host.py: >= 8 bytes of each)
    act: str = "none"
    bias: bool = True
    res: bool = False
    w_layout: int = 0           # 0 row-major, 1 blocked, 2 gate / up interleaved
    x_blk: bool = False
    y_blk: bool = False
    res_blk: bool = False
    fold: bool = False          # the consumer form: ln_stats given
    stats_out: bool = False
    col_scale: Optional[Tuple[int, int, float]] = None
    spare: int = 1              # statistics slots behind the ln_slots the launch is given
    slots_out: int = 0          # mio_ln_stats_reduce (N: slots in)

    @property
    def glu(self):
        return self.act == "swiglu"

    @property
    def rms(self):
        return self.entry == "mio_gemm_rms_bw"


_RM = (PAST_K, PAST_N, GUARD_ROW)


def _table():
    g = lambda name, entry, route, M, N, K, classes, **kw: Case(name, "gemm", entry, route, M, N, K, classes, **kw)  # noqa: E731
    plain, bw, cs, ln, rms = ("mio_gemm_bias_act", "mio_gemm_bias_act_bw", "mio_gemm_bias_act_bw_cs", "mio_gemm_ln_bw",
                              "mio_gemm_rms_bw")
    MR = 8192 - 7   # 32 row tiles, the last one ragged: the fewest tiles the folded kernels take (test_gpu_gemm_matrix.MR)
    cases = [
        # the K tail is zero-filled through mio_zero16: K 40 = one 8-chunk past a 32-k step, 4104 = 128 steps and a chunk
        g("t128_k40", plain, "t128", 37, 72, 40, _RM, act="gelu", res=True),
        g("t128_k4104_tail", plain, "t128", 37, 72, 4104, _RM),
        g("t256_k96", plain, "t256", 4096 + 100, 4096 - 8, 96, _RM, act="relu"),
        g("p8w_k128", plain, "p8w", 4096 + 100, 4096 - 8, 128, _RM),
        g("p8w_blocked_w_k544", bw, "p8w", 4096 + 37, 4096 + 8, 544, _RM, act="silu", w_layout=1),
        g("p8w_blocked_x", bw, "p8w", 4096 + 37, 4096, 256, (PAST_K, PAST_N, GUARD_ROW, PAD_ROW), act="gelu", w_layout=1,
          x_blk=True),
        g("p8w_col_scale_band_to_n", cs, "p8w", 8192 + 100, 3072 + 128, 512, _RM, act="gelu", w_layout=1,
          col_scale=(2048, 3072 + 128, 0.18033688)),
        g("p8w_res_ldr", plain, "p8w_res", 4096 + 100, 4096 - 8, 160, _RM, act="gelu", res=True),
        g("p8w_res_blocked_res", ln, "p8w_res", 4096 + 37, 4096, 256, (PAST_K, PAST_N, GUARD_ROW, PAD_ROW), res=True, w_layout=1,
          x_blk=True, res_blk=True, y_blk=True),
        g("glu_t128x64", plain, "glu_t128x64", 129, 136, 72, _RM, act="swiglu"),
        g("glu_t256x128", plain, "glu_t256x128", 4096 + 1, 2048 + 8, 1024, _RM, act="swiglu"),
        g("p8w_glu_blocked_x", ln, "p8w_glu", 4096 + 100, 2048, 256, (PAST_K, PAST_N, GUARD_ROW, PAD_ROW), act="swiglu",
          w_layout=2, x_blk=True),
        g("p8w_glu_rows", ln, "p8w_glu", 4096 + 100, 2048, 256, _RM, act="swiglu", w_layout=2),
        g("p8w_stats", ln, "p8w_stats", MR, 2048, 128, _RM + (SPARE_SLOT,), res=True, w_layout=1, stats_out=True),
        g("p8w_stats_blocked", ln, "p8w_stats", MR, 2048, 128, (PAST_K, PAST_N, GUARD_ROW, PAD_ROW, SPARE_SLOT), res=True,
          w_layout=1, stats_out=True, x_blk=True, y_blk=True, res_blk=True),
    ]
    fold_cls = (PAST_K, PAST_N, GUARD_ROW, PAD_ROW, SPARE_SLOT)
    for entry, tag, extra in ((ln, "ln", ()), (rms, "rms", (RMS_SUM,))):
        cases += [
            g(f"p8w_fold_{tag}", entry, "p8w_fold", MR, 2048, 512, fold_cls + extra, act="gelu", w_layout=1, fold=True),
            g(f"p8w_fold_{tag}_blocked_x", entry, "p8w_fold", MR, 2048, 512, fold_cls + extra, w_layout=1, fold=True,
              x_blk=True, col_scale=(1024, 2048, 0.25)),
            g(f"p8w_glu_fold_{tag}", entry, "p8w_glu_fold", MR, 1024, 512, fold_cls + extra, act="swiglu", w_layout=2,
              fold=True),
        ]
    m = lambda name, entry, route, M, d, I, classes, **kw: Case(name, "mlp", entry, route, M, I, d, classes, **kw)  # noqa: E731
    MB = 16384 + 100   # ragged; with d = I = 1024 both stages have the tiles of the 256-tile kernels
    cases += [
        m("mlp_two_launch_gelu", "mio_fused_mlp_fwd", "two_launch/t128/t128", 300 + 5, 256, 512, (GUARD_ROW, PAST_N, WORKSPACE),
          act="gelu", res=True),
        m("mlp_two_launch_swiglu", "mio_fused_mlp_fwd", "two_launch/glu_t128x64/t128", 300 + 5, 256, 512,
          (GUARD_ROW, PAST_N, WORKSPACE), act="swiglu"),
        m("mlp_blocked_plain_w", "mio_fused_mlp_fwd", "blocked/p8w/p8w", MB, 1024, 1024, (GUARD_ROW, PAST_N, WORKSPACE),
          act="gelu"),
        m("mlp_bw", "mio_fused_mlp_fwd_bw", "blocked/p8w/p8w_res", MB, 1024, 1024, (PAST_K, GUARD_ROW, PAST_N, WORKSPACE),
          act="gelu", res=True, w_layout=1),
        m("mlp_bw_blocked_x", "mio_fused_mlp_fwd_bw", "blocked/p8w/p8w", MB, 1024, 1024,
          (PAST_K, GUARD_ROW, PAST_N, PAD_ROW, WORKSPACE), act="silu", w_layout=1, x_blk=True),
        m("mlp_glu_bw", "mio_fused_mlp_glu_fwd_bw", "blocked/p8w_glu/p8w_res", MB, 1024, 1024,
          (PAST_K, GUARD_ROW, PAST_N, WORKSPACE), act="swiglu", res=True, w_layout=2),
    ]
    p = lambda name, entry, M, N, K, classes, **kw: Case(name, "prep", entry, "", M, N, K, classes, **kw)  # noqa: E731
    cases += [
        p("prep_block", "mio_weight_block", 0, 300, 96, (PAST_K, GUARD_ROW)),
        p("prep_block_glu", "mio_weight_block_glu", 0, 200, 64, (PAST_K, GUARD_ROW)),
        p("prep_fold_k264", "mio_ln_fold_weight", 0, 70, 264, (PAST_K, GUARD_ROW, PAST_N)),
        p("prep_fold_k2304", "mio_ln_fold_weight", 0, 10, 2304, (PAST_K, GUARD_ROW, PAST_N)),   # the 32-elements-per-thread kernel
        p("prep_quant_w8", "mio_weight_quant_w8", 0, 70, 272, (PAST_K, GUARD_ROW, PAST_N)),
        p("prep_stats_reduce", "mio_ln_stats_reduce", 512 + 37, 16, 0, (PAD_ROW, SPARE_SLOT, GUARD_ROW), slots_out=8),
    ]
    assert len({c.name for c in cases}) == len(cases)
    return cases


CASES = _table()


def coverage():
    """{route or entry point: the not-owned classes its cases are run against}."""
    cov: Dict[str, set] = {}
    for c in CASES:
        keys = [c.entry] + ([c.route] if c.kind == "gemm" else c.route.split("/")[1:] if c.kind == "mlp" else [])
        for k in keys:
            cov.setdefault(k, set()).update(_names(c.classes))
    return cov


def _shrink(v, keep=256):
    return v if v <= 2 * keep else keep + (v % keep or keep)


def shrunk(c: Case) -> Case:
    """The case at the sizes the CPU model is run at: fewer tiles, the same ragged edges (M, N modulo 256; K modulo 256)."""
    M, N = _shrink(c.M), _shrink(c.N)
    K = c.K if c.K <= 544 else 256 + c.K % 256
    cs = None if c.col_scale is None else (N - 128, N, c.col_scale[2])
    return replace(c, M=M, N=N, K=K, col_scale=cs)


# ---- buffers -----------------------------------------------------------------------------------------------------------
def _is16(dt):
    return dt in (torch.bfloat16, torch.float16)


class Buf:
    """One backing buffer, flat: .data (benign values everywhere; owned output elements 0xFF), .cls (class per element,
    OWNED = 0), .role in | out, .scratch (bool per element or None: the launch may write these, nobody reads them), and where
    the operand sits in it: .off / .shape / .strides of its view (elements), .form mat | blk | vec | stats | flat."""

    def __init__(self, name, role, data, cls, off, shape, strides, form, scratch=None):
        self.name, self.role, self.data, self.cls = name, role, data, cls
        self.off, self.shape, self.strides, self.form, self.scratch = off, tuple(shape), tuple(strides), form, scratch
        self._sign = None

    def view(self, t):
        return t.as_strided(self.shape, self.strides, self.off)

    def ptr(self, t):
        return t.data_ptr() + self.off * t.element_size()

    def sign(self):
        if self._sign is None:
            g = torch.Generator().manual_seed(self.data.numel() + len(self.name))
            self._sign = torch.randint(0, 2, self.data.shape, generator=g, dtype=torch.int8) * 2 - 1
        return self._sign

    def where(self, i):
        """(row, column) of flat element i in the operand's logical coordinates (guards: rows / columns outside it)."""
        e = i - self.off
        if self.form == "mat":
            return e // self.strides[0] if e >= 0 else -1 - (-e - 1) // self.strides[0], e % self.strides[0]
        if self.form == "blk":
            C = self.shape[1]
            blk, r = divmod(e, 8192)
            return blk // (C // 32) * 256 + r // 32, blk % (C // 32) * 32 + r % 32
        if self.form == "stats":
            return e // 2 % self.shape[1], e // (2 * self.shape[1])   # (row, slot)
        return 0, e


def _ff(n, dtype):
    return torch.full((n * torch.empty((), dtype=dtype).element_size(),), 255, dtype=torch.uint8).view(dtype)


def _benign(n, dtype, gen, scale=1.0):
    if dtype == torch.uint8:   # e4m3fn bytes: any finite pattern
        b = torch.randint(0, 256, (n,), generator=gen, dtype=torch.int16)
        return torch.where(b % 128 == 127, b - 1, b).to(torch.uint8)
    return (torch.randn(n, generator=gen) * scale).to(dtype)


def _mat(name, role, rows, cols, dtype, gen, past, value=None, pad=PAD_LD, scale=1.0):
    """[rows, cols] at row stride cols + pad inside G_ROWS guard rows on each side."""
    ld = cols + pad
    n = (rows + 2 * G_ROWS) * ld
    cls = torch.full((rows + 2 * G_ROWS, ld), GUARD_ROW, dtype=torch.uint8)
    cls[G_ROWS:G_ROWS + rows, :cols] = OWNED
    cls[G_ROWS:G_ROWS + rows, cols:] = past
    b = Buf(name, role, _benign(n, dtype, gen, scale), cls.reshape(-1), G_ROWS * ld, (rows, cols), (ld, 1), "mat")
    b.view(b.data)[:] = value if value is not None else b.view(_ff(n, dtype))
    return b


def _vec(name, role, n, dtype, gen, value=None, cls_guard=PAST_N):
    tot = n + 2 * G_1D
    cls = torch.full((tot,), cls_guard, dtype=torch.uint8)
    cls[G_1D:G_1D + n] = OWNED
    b = Buf(name, role, _benign(tot, dtype, gen), cls, G_1D, (n,), (1,), "vec")
    b.view(b.data)[:] = value if value is not None else _ff(n, dtype)
    return b


def _blk(name, role, M, C, dtype, gen, value=None):
    """The blocked activation layout of a logical [M, C] (C % 32 == 0): ceil(M / 256) * 256 rows, G_1D elements around."""
    mp = (M + 255) // 256 * 256
    tot = mp * C + 2 * G_1D
    cls = torch.full((tot,), GUARD_ROW, dtype=torch.uint8)
    inner = cls[G_1D:G_1D + mp * C]
    inner[:] = PAD_ROW
    idx = blocked_index(M, C)
    inner[idx.reshape(-1)] = OWNED
    b = Buf(name, role, _benign(tot, dtype, gen), cls, G_1D, (mp, C), (C, 1), "blk")
    b.data[G_1D:G_1D + mp * C][idx] = value if value is not None else _ff(M * C, dtype).view(M, C)
    return b


def _stats(name, role, slots, spare, M, gen, value=None, rms=False, written_pad=False, scratch_pad=False):
    """[slots + spare][ceil(M / 256) * 256][2] fp32.  written_pad: the padding rows of the given slots are owned outputs
    (module docstring); scratch_pad: they are written with unspecified values."""
    mp = (M + 255) // 256 * 256
    tot = (slots + spare) * mp * 2 + 2 * G_1D
    cls = torch.full((tot,), GUARD_ROW, dtype=torch.uint8)
    inner = cls[G_1D:-G_1D].view(slots + spare, mp, 2)
    inner[:] = SPARE_SLOT
    inner[:slots, M:] = OWNED if written_pad else PAD_ROW
    inner[:slots, :M] = OWNED
    if rms:
        inner[:slots, :M, 0] = RMS_SUM
    scratch = None
    if scratch_pad:
        scratch = torch.zeros(tot, dtype=torch.bool)
        scratch[G_1D:-G_1D].view(slots + spare, mp, 2)[:slots, M:] = True
    b = Buf(name, role, _benign(tot, torch.float32, gen, 30.0), cls, G_1D, (slots + spare, mp, 2), (mp * 2, 2, 1), "stats",
            scratch)
    own = b.view(b.data)[:slots]
    if value is not None:
        own[:, :M] = torch.where(inner[:slots, :M] == OWNED, value, own[:, :M])
    else:
        b.view(bits(b.data))[:slots][inner[:slots] == OWNED] = -1
    return b


def _flat(name, role, n, dtype, gen, inner_cls=OWNED, guard_cls=GUARD_ROW, scratch=False):
    """n elements the launch owns as a whole (a prepared weight: an owned output) or may scribble on (a workspace)."""
    tot = n + 2 * G_1D
    cls = torch.full((tot,), guard_cls, dtype=torch.uint8)
    cls[G_1D:G_1D + n] = inner_cls
    sc = None
    if scratch:
        sc = torch.zeros(tot, dtype=torch.bool)
        sc[G_1D:G_1D + n] = True
    b = Buf(name, role, _benign(tot, dtype, gen), cls, G_1D, (n,), (1,), "flat", sc)
    if inner_cls == OWNED:
        b.view(b.data)[:] = _ff(n, dtype)
    return b


@dataclass
class Built:
    case: Case
    dtype: torch.dtype
    bufs: Dict[str, Buf]
    logical: Dict[str, torch.Tensor]   # compact copies of the owned inputs (CPU)
    meta: dict = field(default_factory=dict)


def build(c: Case, dtype, seed=0) -> Built:
    gen = torch.Generator().manual_seed(seed * 7919 + sum(ord(ch) for ch in c.name))
    return {"gemm": _build_gemm, "mlp": _build_mlp, "prep": _build_prep}[c.kind](c, dtype, gen)


def _rand(gen, shape, dtype, scale=1.0, shift=0.0):
    return (torch.randn(shape, generator=gen) * scale + shift).to(dtype)


def _act_operand(name, role, blk, M, C, dtype, gen, past, value=None):
    return _blk(name, role, M, C, dtype, gen, value) if blk else _mat(name, role, M, C, dtype, gen, past, value)


def _wb_elems(c: Case, N, K):
    return ((N + 127) // 128 * 256 if c.w_layout == 2 else (N + 255) // 256 * 256) * K


def _build_gemm(c: Case, dtype, gen) -> Built:
    M, N, K = c.M, c.N, c.K
    bufs, lg = {}, {}
    fold = c.fold
    lg["x"] = _rand(gen, (M, K), dtype, 2.0, 1.0) if fold else _rand(gen, (M, K), dtype)
    bufs["x"] = _act_operand("x", "in", c.x_blk, M, K, dtype, gen, PAST_K, lg["x"])
    lg["w"] = _rand(gen, (N, K), dtype, K ** -0.5)
    bufs["w"] = _mat("w", "in", N, K, dtype, gen, PAST_K, lg["w"])
    if c.glu:
        lg["wg"] = _rand(gen, (N, K), dtype, K ** -0.5)
        bufs["wg"] = _mat("wg", "in", N, K, dtype, gen, PAST_K, lg["wg"])
    vecs = []
    if fold:   # the projection behind a norm: gamma (beta, bias) are folded into the prepared weight (and bias)
        lg["gamma"] = _rand(gen, (K,), dtype, 0.2, 1.0)
        vecs.append(("gamma", K))
        if not c.rms:
            lg["beta"] = _rand(gen, (K,), dtype, 0.1)
            vecs.append(("beta", K))
    if c.bias:
        lg["bias"] = _rand(gen, (N,), dtype, 0.5 if not fold else 0.1)
        vecs.append(("bias", N))
        if c.glu:
            lg["bias_g"] = _rand(gen, (N,), dtype, 0.5 if not fold else 0.1)
            vecs.append(("bias_g", N))
    for name, n in vecs:
        bufs[name] = _vec(name, "in", n, dtype, gen, lg[name])
    if fold and not c.rms:   # mio_ln_fold_weight writes the row-major folded weight and the folded bias
        bufs["bias_f"] = _vec("bias_f", "out", N, dtype, gen)
        bufs["ws"] = _flat("ws", "out", N * K, dtype, gen)
        if c.glu:
            bufs["bias_gf"] = _vec("bias_gf", "out", N, dtype, gen)
            bufs["wsg"] = _flat("wsg", "out", N * K, dtype, gen)
    elif fold:               # w * gamma rounded once (mio.ops.rms_fold_weight: torch ops), blocked by the library
        bufs["ws"] = _flat("ws", "out", N * K, dtype, gen)
        if c.glu:
            bufs["wsg"] = _flat("wsg", "out", N * K, dtype, gen)
    if c.w_layout:
        bufs["wb"] = _flat("wb", "out", _wb_elems(c, N, K), dtype, gen)
    if c.res:
        lg["res"] = _rand(gen, (M, N), dtype)
        bufs["res"] = _act_operand("res", "in", c.res_blk, M, N, dtype, gen, PAST_N, lg["res"])
    bufs["y"] = _act_operand("y", "out", c.y_blk, M, N, dtype, gen, PAST_N)
    if fold:
        slots = K // 256
        xd = lg["x"].double().view(M, slots, 256)
        st = torch.stack([xd.sum(-1).t(), (xd * xd).sum(-1).t()], -1).float()   # [slots, M, 2]
        lg["stats"] = st
        bufs["ln_stats"] = _stats("ln_stats", "in", slots, c.spare, M, gen, st, rms=c.rms)
    if c.stats_out:
        bufs["stats_out"] = _stats("stats_out", "out", N // 256, 1, M, gen, written_pad=True)
    return Built(c, dtype, bufs, lg, dict(tile=128 if c.route in ("t128", "glu_t128x64") else 256))


def _build_mlp(c: Case, dtype, gen) -> Built:
    M, I, d = c.M, c.N, c.K
    bufs, lg = {}, {}
    bw = c.w_layout != 0
    pad = PAD_LD if bw else 0    # the plain entry point takes contiguous weights; a blocked one is prepared from any stride
    lg["x"] = _rand(gen, (M, d), dtype)
    bufs["x"] = _blk("x", "in", M, d, dtype, gen, lg["x"]) if c.x_blk else _mat("x", "in", M, d, dtype, gen, PAST_K, lg["x"], 0)
    for name, shape, scale in (("w1", (I, d), d ** -0.5), ("wg", (I, d), d ** -0.5), ("w2", (d, I), I ** -0.5)):
        if name == "wg" and not c.glu:
            continue
        lg[name] = _rand(gen, shape, dtype, scale)
        bufs[name] = _mat(name, "in", shape[0], shape[1], dtype, gen, PAST_K, lg[name], pad)
    for name, n in (("b1", I), ("bg", I), ("b2", d)):
        if name == "bg" and not c.glu:
            continue
        lg[name] = _rand(gen, (n,), dtype, 0.5)
        bufs[name] = _vec(name, "in", n, dtype, gen, lg[name])
    if bw:
        bufs["w1b"] = _flat("w1b", "out", _wb_elems(c, I, d), dtype, gen)
        bufs["w2b"] = _flat("w2b", "out", (d + 255) // 256 * 256 * I, dtype, gen)
    if c.res:
        lg["res"] = _rand(gen, (M, d), dtype)
        bufs["res"] = _mat("res", "in", M, d, dtype, gen, PAST_N, lg["res"], 0)
    bufs["y"] = _mat("y", "out", M, d, dtype, gen, PAST_N, None, 0)
    bufs["work"] = _flat("work", "out", (M + 255) // 256 * 256 * I, dtype, gen, WORKSPACE, WORKSPACE, scratch=True)
    return Built(c, dtype, bufs, lg, dict(tile=256 if c.route.startswith("blocked") else 128))


def _build_prep(c: Case, dtype, gen) -> Built:
    N, K = c.N, c.K
    bufs, lg = {}, {}
    e = c.entry
    if e == "mio_ln_stats_reduce":
        M, slots_in = c.M, c.N
        st = torch.randn(slots_in, M, 2, generator=gen) * 30
        st[..., 1] = st[..., 1] ** 2
        lg["stats"] = st
        bufs["stats_in"] = _stats("stats_in", "in", slots_in, c.spare, M, gen, st)
        bufs["stats_red"] = _stats("stats_red", "out", c.slots_out, 1, M, gen, scratch_pad=True)
        return Built(c, dtype, bufs, lg, dict(tile=256))
    lg["w"] = _rand(gen, (N, K), dtype, 0.05, 0.01)
    bufs["w"] = _mat("w", "in", N, K, dtype, gen, PAST_K, lg["w"])
    if e == "mio_weight_block":
        bufs["wb"] = _flat("wb", "out", (N + 255) // 256 * 256 * K, dtype, gen)
    elif e == "mio_weight_block_glu":
        lg["wg"] = _rand(gen, (N, K), dtype, 0.05)
        bufs["wg"] = _mat("wg", "in", N, K, dtype, gen, PAST_K, lg["wg"])
        bufs["wb"] = _flat("wb", "out", (N + 127) // 128 * 256 * K, dtype, gen)
    elif e == "mio_ln_fold_weight":
        for name, n, sc, sh in (("gamma", K, 0.2, 1.0), ("beta", K, 0.1, 0.0), ("bias", N, 0.1, 0.0)):
            lg[name] = _rand(gen, (n,), dtype, sc, sh)
            bufs[name] = _vec(name, "in", n, dtype, gen, lg[name])
        bufs["ws"] = _flat("ws", "out", N * K, dtype, gen)
        bufs["bias_f"] = _vec("bias_f", "out", N, dtype, gen)
    elif e == "mio_weight_quant_w8":
        bufs["w8"] = _mat("w8", "out", N, K, torch.uint8, gen, PAST_K, None, 16)
        bufs["scale"] = _vec("scale", "out", N, torch.float32, gen)
    return Built(c, dtype, bufs, lg, dict(tile=256))


# ---- fills -------------------------------------------------------------------------------------------------------------
def poison(d, mask, fill, sign):
    """The elements of the flat tensor d under mask := `fill` (nan | huge; benign leaves them), in place."""
    if fill == "benign":
        return d
    if fill == "nan":
        bits(d)[mask] = -1 if d.element_size() > 1 else 255
    elif _is16(d.dtype):
        d[mask] = (sign[mask].float() * (torch.finfo(d.dtype).max / 8)).to(d.dtype)
    elif d.dtype == torch.float32:
        d[mask] = 1e30
    else:   # e4m3fn bytes: +-448
        d[mask] = torch.where(sign[mask] > 0, 0x7E, 0xFE).to(torch.uint8)
    return d


def inputs(built: Built, fill: str, only=None) -> Dict[str, torch.Tensor]:
    """Every buffer of a launch (fresh flat tensors): the not-owned elements holding `fill` (only: just these classes, the
    rest benign), owned inputs their data, owned outputs 0xFF bytes."""
    out = {}
    for name, bf in built.bufs.items():
        m = bf.cls != OWNED
        if only is not None:
            m = m & torch.isin(bf.cls, torch.tensor(sorted(only), dtype=torch.uint8))
        out[name] = poison(bf.data.clone(), m, fill, bf.sign())
    return out


class Embedded:
    """One operand of a launch as a view inside a larger buffer on the operand's own device, for the tests that launch
    through mio.ops (the decode GEMMs, the row kernels): .view is value.shape elements at offset `at` of a buffer of shape
    `shape`.  fill(f) rewrites the buffer in place (the same addresses for every fill): the bytes around the view hold f, the
    view holds value -- or, for an output (value None, of `out_shape`), 0xFF bytes.  own_index: only these flat elements of the
    view are the launch's (the rows below M of a blocked output); the rest of the view is poisoned and held like the bytes around
    it.  untouched(): after the launch, every byte the launch does not own (an input that is not `written`: every byte) is what
    fill() wrote.  An e4m3fn operand is kept as bytes; .view shows them as float8_e4m3fn."""

    def __init__(self, value, shape, at=None, out_shape=None, dtype=None, device=None, seed=0, own_index=None, written=None):
        self.value = value
        vshape = tuple(value.shape) if value is not None else tuple(out_shape)
        dtype = value.dtype if value is not None else dtype
        device = value.device if value is not None else device
        self.fp8 = dtype == torch.float8_e4m3fn
        store = torch.uint8 if self.fp8 else dtype
        at = (0,) * len(shape) if at is None else tuple(at)
        self.buf = torch.empty(shape, dtype=store, device=device)
        self.idx = tuple(slice(a, a + n) for a, n in zip(at, vshape))
        self.owned = torch.zeros(shape, dtype=torch.bool, device=device)
        self.owned[self.idx] = True
        if own_index is not None:
            ov = torch.zeros(self.owned[self.idx].numel(), dtype=torch.bool, device=device)
            ov[own_index.reshape(-1).to(device)] = True
            self.owned[self.idx] = ov.view(vshape)
        self.written = (value is None) if written is None else written
        g = torch.Generator().manual_seed(seed + self.buf.numel())
        self.sign = (torch.randint(0, 2, (self.buf.numel(),), generator=g, dtype=torch.int8) * 2 - 1).to(device)
        self.benign = _benign(self.buf.numel(), store, g).to(device)
        self.snap = None

    @property
    def view(self):
        v = self.buf[self.idx]
        return v.view(torch.float8_e4m3fn) if self.fp8 else v

    def fill(self, fill):
        flat = self.buf.view(-1)
        flat.copy_(self.benign)
        poison(flat, ~self.owned.view(-1), fill, self.sign)
        if self.value is not None:
            self.buf[self.idx] = self.value.view(torch.uint8) if self.fp8 else self.value
        else:
            bits(flat)[self.owned.view(-1)] = -1 if flat.element_size() > 1 else 255
        self.snap = bits(flat).clone()
        return self

    def untouched(self):
        same = bits(self.buf.view(-1)) == self.snap
        return bool(same[~self.owned.view(-1)].all()) if self.written else bool(same.all())


# ---- the judgement -----------------------------------------------------------------------------------------------------
def _first(mask):
    return int(torch.nonzero(mask.reshape(-1))[0])


def _histogram(bf: Buf, d, tile):
    """{(row tile, column tile): differing elements} of the flat difference mask d, largest first."""
    h: Dict[Tuple[int, int], int] = {}
    idx = torch.nonzero(d.reshape(-1)).reshape(-1)[:200000]
    e = idx - bf.off
    if bf.form == "mat":
        r, cc = e // bf.strides[0], e % bf.strides[0]
    elif bf.form == "blk":
        C = bf.shape[1]
        blk, q = e // 8192, e % 8192
        r, cc = blk // (C // 32) * 256 + q // 32, blk % (C // 32) * 32 + q % 32
    elif bf.form == "stats":
        r, cc = e // 2 % bf.shape[1], e // (2 * bf.shape[1]) * tile
    else:
        r, cc = torch.zeros_like(e), e
    for key, n in zip(*torch.unique(torch.stack([r // tile, cc // tile], 1), dim=0, return_counts=True)):
        h[(int(key[0]), int(key[1]))] = int(n)
    return dict(sorted(h.items(), key=lambda kv: -kv[1])[:8])


def _launch(run, built, given, fill):
    """One launch; then: every input equals its snapshot byte for byte, every not-owned output byte holds its pre-fill."""
    snap = {k: v.clone() for k, v in given.items()}
    after = run(built, given)
    for name, bf in built.bufs.items():
        changed = bits(after[name]) != bits(snap[name])
        if bf.role == "out":
            changed = changed & (bf.cls != OWNED)
        if bf.scratch is not None:
            changed = changed & ~bf.scratch
        if changed.any():
            i = _first(changed)
            cl = CLASS_NAMES.get(int(bf.cls[i]), "owned")
            verb = "input modified" if bf.role == "in" else "not-owned output written"
            raise HostileFailure(f"{built.case.name} fill {fill}: {verb}: {name} at (row, column) {bf.where(i)} [{cl}], "
                                 f"{int(changed.sum())} elements; route {built.case.route or built.case.entry}", fill, name, [cl])
    return after


def _judged(bf: Buf):
    m = bf.cls == OWNED
    return m & ~bf.scratch if bf.scratch is not None else m


def _diff(built, base, after):
    for name, bf in built.bufs.items():
        if bf.role == "out":
            d = (bits(after[name]) != bits(base[name])) & _judged(bf)
            if d.any():
                return name, d
    return None


def nonvacuous(built: Built):
    """Every class the case claims is there, with at least 8 bytes; every class that is there is claimed."""
    have: Dict[int, int] = {}
    for bf in built.bufs.values():
        for cl, n in zip(*torch.unique(bf.cls, return_counts=True)):
            have[int(cl)] = have.get(int(cl), 0) + int(n) * bf.data.element_size()
    have.pop(OWNED, None)
    c = built.case
    thin = [CLASS_NAMES[x] for x in c.classes if have.get(x, 0) < 8]
    assert not thin, f"{c.name}: fewer than 8 bytes of the claimed classes {thin}"
    extra = [CLASS_NAMES[x] for x in have if x not in c.classes]
    assert not extra, f"{c.name}: holds not-owned classes it does not claim: {extra}"
    return have


def judge(run, built: Built, fills=("nan", "huge"), device=None):
    """run(built, bufs) -> bufs after the launch ({name: flat CPU tensor}, every buffer of built.bufs).

    1. `benign` launch: the result within the unchanged _gemm_check.check / BARS of the case's route against the fp64
       reference computed from compact copies of the owned inputs (check_reference; device: where that reference runs).
       A failure here is raised behind step 2: where a fill finds the same defect, its report says more.
    2. each of `fills`: every owned output byte (y, stats_out, the prepared weights) equals the benign launch's.
       tests/test_gpu_repeatable.py holds reruns of these routes bit-identical, so a difference is the poison's doing; the
       report names the fill, the tensor, the first differing element, the route, a per-tile histogram of the differing
       elements and -- from one relaunch per class with only that class poisoned -- the classes that reach the result.
    3. after every launch: not-owned bytes of every buffer hold their pre-fill (inputs: every byte).
    Raises HostileFailure (an AssertionError)."""
    nonvacuous(built)
    c = built.case
    base = _launch(run, built, inputs(built, "benign"), "benign")
    wrong = None
    try:
        check_reference(built, base, device)
    except HostileFailure:
        raise
    except AssertionError as e:   # raised behind the fills: what they find says more about the same defect
        wrong = e
    for fill in fills:
        after = _launch(run, built, inputs(built, fill), fill)
        bad = _diff(built, base, after)
        if bad is None:
            continue
        name, d = bad
        bf = built.bufs[name]
        guilty = []
        for cl in c.classes:
            try:
                one = run(built, inputs(built, fill, only={cl}))
            except Exception:
                continue
            if _diff(built, base, one) is not None:
                guilty.append(CLASS_NAMES[cl])
        raise HostileFailure(
            f"{c.name} fill {fill}: {name} differs from the benign launch in {int(d.sum())} elements, first at (row, column) "
            f"{bf.where(_first(d))}; not-owned memory that reaches the result: {guilty or 'no single class'}; route "
            f"{c.route or c.entry}; differing elements per {built.meta['tile']}-tile (row tile, column tile): "
            f"{_histogram(bf, d, built.meta['tile'])}", fill, name, guilty)
    if wrong is not None:
        raise wrong
    return base


# ---- the references ----------------------------------------------------------------------------------------------------
def unblock(flat, M, C):
    """The logical [M, C] of a blocked operand's inner elements (flat, ceil(M / 256) * 256 * C of them)."""
    return flat.reshape(-1)[blocked_index(M, C)]


def glu_rows(I):
    """(source row, is_up) per row of the interleaved gate / up weight of include/mio_hip.h, [ceil(I / 128) * 256]."""
    r = torch.arange((I + 127) // 128 * 256)
    return r // 256 * 128 + r % 256 // 64 * 32 + r % 32, (r // 32) % 2 == 1


def block_rows(w, rows=None):
    """mio_weight_block of the row-major w [N, K] (K % 32 == 0): the flat blocked elements, padding rows zero."""
    N, K = w.shape
    np_ = (N + 255) // 256 * 256 if rows is None else rows
    full = torch.zeros(np_, K, dtype=w.dtype)
    full[:N] = w
    out = torch.empty(np_ * K, dtype=w.dtype)
    out[blocked_index(np_, K)] = full
    return out


def block_glu(wg, wu):
    """mio_weight_block_glu: the interleaved rows (zero past I), blocked."""
    I, K = wg.shape
    src, up = glu_rows(I)
    ok = src < I
    rows = torch.where(up[:, None], wu[src.clamp_max(I - 1)], wg[src.clamp_max(I - 1)])
    rows = torch.where(ok[:, None], rows, torch.zeros((), dtype=wg.dtype))
    return block_rows(rows, rows.shape[0])


def _out(built, after, name, M, C):
    bf = built.bufs[name]
    v = bf.view(after[name])
    return unblock(v, M, C) if bf.form == "blk" else v


def check_reference(built: Built, after, device=None):
    """The benign launch against the family's existing references and bars."""
    c, dtype, lg = built.case, built.dtype, built.logical
    if c.kind == "gemm":
        M, N, K = c.M, c.N, c.K
        y = _out(built, after, "y", M, N)
        if c.w_layout:   # the prepared weight is what the library's own preparation of the owned source gives
            want = block_glu(lg["wg"], lg["w"]) if (c.glu and not c.fold) else None if c.fold else block_rows(lg["w"])
            if want is not None:
                assert torch.equal(bits(built.bufs["wb"].view(after["wb"])), bits(want)), f"{c.name}: the blocked weight"
        if c.fold:
            ws = built.bufs["ws"].view(after["ws"]).view(N, K)
            wsg = built.bufs["wsg"].view(after["wsg"]).view(N, K) if c.glu else None
            want = block_glu(wsg, ws) if c.glu else block_rows(ws)
            assert torch.equal(bits(built.bufs["wb"].view(after["wb"])), bits(want)), f"{c.name}: the blocked folded weight"
            if c.rms:
                bias, bias_g = lg.get("bias"), lg.get("bias_g")
                fn, eps = rc.reference_fold_rms, EPS
            else:
                bias = built.bufs["bias_f"].view(after["bias_f"])
                bias_g = built.bufs["bias_gf"].view(after["bias_gf"]) if c.glu else None
                fn, eps = gc.reference_fold, EPS
            kw = dict(ws_gate=wsg, bias_gate=bias_g) if c.glu else {}
            ref = fn(lg["x"], lg["stats"], ws, bias, eps=eps, act=c.act, col_scale=c.col_scale, device=device, **kw)
        else:
            ref = gc.reference(lg["x"], lg["w"], lg.get("bias"), c.act, lg.get("wg"), lg.get("bias_g"), lg.get("res"),
                               c.col_scale, device=device)
        gc.check(y, ref, dtype, c.route, what=c.name)
        if c.stats_out:   # (sum, sum of squares) of the stored rows within the fp32 summation bound (test_gpu_gemm_matrix)
            st = built.bufs["stats_out"].view(after["stats_out"])[:N // 256, :M].double()
            yf = y.double().view(M, N // 256, 256)
            s, q = yf.sum(-1).t(), (yf * yf).sum(-1).t()
            gam = lambda n: n * gc.U32 / (1 - n * gc.U32)  # noqa: E731
            assert bool(((st[..., 0] - s).abs() <= gam(256) * yf.abs().sum(-1).t()).all()), f"{c.name}: row sums"
            assert bool(((st[..., 1] - q).abs() <= gam(257) * q).all()), f"{c.name}: row sums of squares"
    elif c.kind == "mlp":
        M, I, d = c.M, c.N, c.K
        ref = gc.reference_mlp(lg["x"], lg["w1"], lg["b1"], lg["w2"], lg["b2"], c.act, lg.get("wg"), lg.get("bg"),
                               lg.get("res"), device=device)
        gc.check(built.bufs["y"].view(after["y"]), ref, dtype, c.route.split("/")[2], what=c.name)
        if c.w_layout:
            want = block_glu(lg["wg"], lg["w1"]) if c.glu else block_rows(lg["w1"])
            assert torch.equal(bits(built.bufs["w1b"].view(after["w1b"])), bits(want)), f"{c.name}: the blocked fc1 weight"
            assert torch.equal(bits(built.bufs["w2b"].view(after["w2b"])), bits(block_rows(lg["w2"]))), c.name
    else:
        _check_prep(built, after)


def quant_w8_reference(w):
    """mio_weight_quant_w8 of include/mio_hip.h on finite rows: (bytes [N, K] uint8, scale [N] fp32)."""
    a = w.float().abs().amax(1)
    scale = torch.where(a == 0, torch.ones_like(a), a / 448.0)
    q = (w.float() * (1.0 / scale)[:, None]).clamp(-448.0, 448.0)
    return q.to(torch.float8_e4m3fn).view(torch.uint8), scale


def _check_prep(built, after):
    c, lg = built.case, built.logical
    e, N, K = c.entry, c.N, c.K
    if e == "mio_weight_block":      # bit-exact: a permutation of the owned rows, the padding rows zero
        assert torch.equal(bits(built.bufs["wb"].view(after["wb"])), bits(block_rows(lg["w"]))), c.name
    elif e == "mio_weight_block_glu":
        assert torch.equal(bits(built.bufs["wb"].view(after["wb"])), bits(block_glu(lg["wg"], lg["w"]))), c.name
    elif e == "mio_ln_fold_weight":  # (judged element by element in test_gpu_gemm_matrix.test_ln_fold_weight_rows)
        ws = built.bufs["ws"].view(after["ws"]).view(N, K).double()
        wg = lg["w"].double() * lg["gamma"].double()
        exact = wg - wg.mean(1, keepdim=True)
        d = gc._gamma(K + 1) * wg.abs().mean(1, keepdim=True) * (1 + gc.U32) + gc.U32 * exact.abs()
        near = (ws - exact).abs() <= d + gc.ulp16(exact.abs() + d, built.dtype)
        assert bool(near.all()), f"{c.name}: a prepared element is no neighbour of its value"
        assert bool(torch.isfinite(built.bufs["bias_f"].view(after["bias_f"]).float()).all()), c.name
    elif e == "mio_weight_quant_w8":
        q, s = quant_w8_reference(lg["w"])
        assert torch.equal(built.bufs["scale"].view(after["scale"]), s), f"{c.name}: scales"
        assert torch.equal(built.bufs["w8"].view(after["w8"]), q), f"{c.name}: quantised bytes"
    else:
        M, per = c.M, c.N // c.slots_out
        out = built.bufs["stats_red"].view(after["stats_red"])[:c.slots_out, :M].double()
        terms = lg["stats"].double().view(c.slots_out, per, M, 2)
        assert bool(((out - terms.sum(1)).abs() <= gc._gamma(per) * terms.abs().sum(1)).all()), c.name


# ---- the CPU model of the launch forms ---------------------------------------------------------------------------------
DEFECTS = ("x_chunk_past_k", "w_row_clamp_n", "bias_unclamped", "res_row_m", "pad_row_in_stats", "rms_uses_sum", "spare_slot",
           "store_row_past_m", "clamp_only", "input_modified")


def _act64(z, act):
    return gc._act64(z, act)


class Model:
    """A torch model of the launch forms, in fp64, that reads its operands through the embedded views.  defect: one of
    DEFECTS, a planted out-of-ownership access.  A planted READ enters the result at weight zero (0 x value), as the value of
    a clamped row or a zero-filled chunk does in the kernels: right on `benign`, NaN on `nan`.
      x_chunk_past_k    the 8 columns of x behind K are multiplied with a zero weight chunk
      w_row_clamp_n     weight rows past N are clamped to row N, not N - 1: the products of those rows belong to columns that
                        are never stored, so a plain-weight launch shows nothing; the preparation of a blocked weight copies
                        row N into the padding rows, which are owned output
      bias_unclamped    the bias vector of the last column group is read at N, and enters column N - 1 at weight zero
      res_row_m         residual row M is read and added, at weight zero, into row M - 1
      pad_row_in_stats  the first padding row of a blocked x is summed into the producer's statistics of row M - 1
      rms_uses_sum      the RMS form takes the mean from the sum entries (at weight zero)
      spare_slot        the slot behind ln_slots is summed as well (at weight zero)
      store_row_past_m  one row past M of a blocked y is stored
      clamp_only        a spare slot's sum of squares enters the variance only through fmax: a NaN drops out
      input_modified    one bit of w is flipped"""

    def __init__(self, defect=None):
        assert defect is None or defect in DEFECTS
        self.defect = defect

    def __call__(self, built: Built, t):
        {"gemm": self._gemm, "mlp": self._mlp, "prep": self._prep}[built.case.kind](built, t)
        if self.defect == "input_modified":
            bits(t["w1" if built.case.kind == "mlp" else "w" if "w" in t else "stats_in"]).view(-1)[G_1D + 3] ^= 1
        return t

    # -- pieces
    def _rows(self, built, t, name, M, C):
        """The logical [M, C] fp64 of an activation operand."""
        bf = built.bufs[name]
        v = bf.view(t[name])
        return (unblock(v, M, C) if bf.form == "blk" else v).double()

    def _block(self, built, t, src_names, out_name, N, K, glu):
        """The weight preparation: t[out_name] := blocked(src)."""
        d = self.defect
        srcs = []
        for s in src_names:
            if isinstance(s, str):
                bf = built.bufs[s]
                v = bf.view(t[s])
                extra = 1 if d == "w_row_clamp_n" and bf.form == "mat" else 0   # the row behind the last: a guard row
                srcs.append(t[s].as_strided((N + extra, K), bf.strides, bf.off) if extra else v)
            else:
                srcs.append(s)
        if glu:
            I = N
            src, up = glu_rows(I)
            rows = torch.where(up[:, None], srcs[1][src.clamp_max(I - 1)], srcs[0][src.clamp_max(I - 1)])
            rows = torch.where((src < I)[:, None], rows, torch.zeros((), dtype=rows.dtype))
            if srcs[0].shape[0] > I:   # the planted clamp: the padding rows that stand for row I take it
                for r in torch.nonzero(src == I).reshape(-1).tolist():
                    rows[r] = srcs[1 if up[r] else 0][I]
            out = block_rows(rows, rows.shape[0])
        else:
            w = srcs[0]
            np_ = (N + 255) // 256 * 256
            out = block_rows(w[:min(w.shape[0], np_)], np_)
        built.bufs[out_name].view(t[out_name])[:] = out

    def _fold_weight(self, built, t, wname, bias_name, ws_name, bout_name, N, K):
        w = built.bufs[wname].view(t[wname]).double()
        gam = built.bufs["gamma"].view(t["gamma"]).double()
        wg = w * gam
        built.bufs[ws_name].view(t[ws_name])[:] = gc.rn16(wg - wg.mean(1, keepdim=True), built.dtype).to(built.dtype).reshape(-1)
        b = w @ built.bufs["beta"].view(t["beta"]).double()
        if bias_name in t:
            b = b + built.bufs[bias_name].view(t[bias_name]).double()
        built.bufs[bout_name].view(t[bout_name])[:] = gc.rn16(b, built.dtype).to(built.dtype)

    def _gemm(self, built, t):
        c, d, dtype = built.case, self.defect, built.dtype
        M, N, K = c.M, c.N, c.K
        B = built.bufs
        x = self._rows(built, t, "x", M, K)
        # -- the weights the product takes
        if c.fold:
            if c.rms:
                for wn, sn in (("w", "ws"), ("wg", "wsg")):
                    if wn in t:
                        prod = B[wn].view(t[wn]).float() * B["gamma"].view(t["gamma"]).float()
                        B[sn].view(t[sn])[:] = prod.to(dtype).reshape(-1)
                bias = B["bias"].view(t["bias"]).double() if "bias" in t else None
                bias_g = B["bias_g"].view(t["bias_g"]).double() if "bias_g" in t else None
            else:
                self._fold_weight(built, t, "w", "bias", "ws", "bias_f", N, K)
                bias = B["bias_f"].view(t["bias_f"]).double()
                bias_g = None
                if c.glu:
                    self._fold_weight(built, t, "wg", "bias_g", "wsg", "bias_gf", N, K)
                    bias_g = B["bias_gf"].view(t["bias_gf"]).double()
            ws = B["ws"].view(t["ws"]).view(N, K)
            wsg = B["wsg"].view(t["wsg"]).view(N, K) if c.glu else None
            self._block(built, t, [wsg, ws] if c.glu else [ws], "wb", N, K, c.glu)
            w, wg = ws.double(), None if wsg is None else wsg.double()
        else:
            if c.w_layout:
                self._block(built, t, ["wg", "w"] if c.glu else ["w"], "wb", N, K, c.glu)
            w = B["w"].view(t["w"]).double()
            wg = B["wg"].view(t["wg"]).double() if c.glu else None
            bias = B["bias"].view(t["bias"]).double() if "bias" in t else None
            bias_g = B["bias_g"].view(t["bias_g"]).double() if "bias_g" in t else None
        acc = x @ w.t()
        accg = x @ wg.t() if c.glu else None
        if d == "x_chunk_past_k" and B["x"].form == "mat":
            bf = B["x"]
            tail = t["x"].as_strided((M, 8), bf.strides, bf.off + K).double()
            acc = acc + tail @ torch.zeros(8, N, dtype=torch.float64)
        # -- the read-out
        if c.fold:
            bf = B["ln_stats"]
            st = bf.view(t["ln_stats"]).double()
            slots = K // 256
            sm, sq = st[:slots, :M, 0].sum(0), st[:slots, :M, 1].sum(0)
            if d == "spare_slot":
                sq = sq + 0.0 * st[slots, :M, 1]
            if c.rms:
                var = sq / K
                if d == "rms_uses_sum":
                    var = var + 0.0 * sm
            else:
                var = (sq / K - (sm / K) ** 2).clamp_min(0.0)
            if d == "clamp_only":
                var = torch.fmax(var, st[slots, :M, 1] * 1e-20 - 1.0)
            r = (var + EPS) ** -0.5
            acc = acc * r[:, None]
            accg = accg * r[:, None] if c.glu else None
        z = acc if bias is None else acc + bias
        if d == "bias_unclamped" and "bias" in t and not c.fold:
            bf = B["bias"]
            z[:, N - 1] = z[:, N - 1] + 0.0 * t["bias"][bf.off + N].double()
        if c.glu:
            zg = accg if bias_g is None else accg + bias_g
            yv = _act64(zg, "silu") * z
        else:
            yv = _act64(z, c.act)
        if c.col_scale is not None:
            lo, hi, s = c.col_scale
            yv[:, lo:hi] = yv[:, lo:hi] * float(torch.tensor(s, dtype=torch.float32))
        if c.res:
            yv = yv + self._rows(built, t, "res", M, N)
            if d == "res_row_m" and B["res"].form == "mat":
                bf = B["res"]
                yv[M - 1] = yv[M - 1] + 0.0 * t["res"].as_strided((N,), (1,), bf.off + M * bf.strides[0]).double()
        yr = gc.rn16(yv, dtype).to(dtype)
        by = B["y"]
        if by.form == "blk":
            by.view(t["y"]).reshape(-1)[blocked_index(M, N)] = yr
            if d == "store_row_past_m" and M % 256:
                by.view(t["y"]).reshape(-1)[blocked_index(M + 1, N)[M]] = yr[M - 1]
        else:
            by.view(t["y"])[:] = yr
        if c.stats_out:
            yf = yr.double().view(M, N // 256, 256)
            so = B["stats_out"].view(t["stats_out"])
            st = torch.stack([yf.sum(-1).t(), (yf * yf).sum(-1).t()], -1)
            if d == "pad_row_in_stats" and B["x"].form == "blk" and M % 256:
                pad = B["x"].view(t["x"]).reshape(-1)[blocked_index(M + 1, K)[M]].double().sum()
                st[:, M - 1, 0] = st[:, M - 1, 0] + 0.0 * pad
            so[:N // 256, :M] = st.float()
            so[:N // 256, M:] = st[:, M - 1:M].float()   # the rows past M: statistics of the clamped last row

    def _mlp(self, built, t):
        c, d, dtype = built.case, self.defect, built.dtype
        M, I, K = c.M, c.N, c.K
        B = built.bufs
        if c.w_layout:
            self._block(built, t, ["wg", "w1"] if c.glu else ["w1"], "w1b", I, K, c.glu)
            self._block(built, t, ["w2"], "w2b", K, I, False)
        x = self._rows(built, t, "x", M, K)
        z = x @ B["w1"].view(t["w1"]).double().t() + B["b1"].view(t["b1"]).double()
        if c.glu:
            zg = x @ B["wg"].view(t["wg"]).double().t() + B["bg"].view(t["bg"]).double()
            h = _act64(zg, "silu") * z
        else:
            h = _act64(z, c.act)
        if d == "bias_unclamped":
            h[:, I - 1] = h[:, I - 1] + 0.0 * t["b1"][B["b1"].off + I].double()
        # the intermediate goes through the workspace, rounded to the storage dtype (blocked where the route says so)
        work = B["work"].view(t["work"])
        hr = gc.rn16(h, dtype).to(dtype)
        if c.route.startswith("blocked"):
            work[blocked_index(M, I)] = hr
            h = unblock(work, M, I).double()
        else:
            work[:M * I] = hr.reshape(-1)
            h = work[:M * I].view(M, I).double()
        yv = h @ B["w2"].view(t["w2"]).double().t() + B["b2"].view(t["b2"]).double()
        if c.res:
            yv = yv + B["res"].view(t["res"]).double()
            if d == "res_row_m":
                bf = B["res"]
                yv[M - 1] = yv[M - 1] + 0.0 * t["res"].as_strided((K,), (1,), bf.off + M * bf.strides[0]).double()
        B["y"].view(t["y"])[:] = gc.rn16(yv, dtype).to(dtype)

    def _prep(self, built, t):
        c, d = built.case, self.defect
        e, N, K = c.entry, c.N, c.K
        B = built.bufs
        if e == "mio_weight_block":
            self._block(built, t, ["w"], "wb", N, K, False)
        elif e == "mio_weight_block_glu":
            self._block(built, t, ["wg", "w"], "wb", N, K, True)
        elif e == "mio_ln_fold_weight":
            w = B["w"].view(t["w"])
            gam = B["gamma"].view(t["gamma"])
            wg = w.float() * gam.float()              # (fp32 as the kernel; the row mean of the unrounded products)
            ws = (wg - (wg.double().mean(1, keepdim=True)).float()).to(built.dtype)
            if d == "x_chunk_past_k":
                bf = B["w"]
                ws = (ws.float() + 0.0 * t["w"].as_strided((N, 1), bf.strides, bf.off + K).float()).to(built.dtype)
            B["ws"].view(t["ws"])[:] = ws.reshape(-1)
            b = B["bias"].view(t["bias"]).double() + w.double() @ B["beta"].view(t["beta"]).double()
            B["bias_f"].view(t["bias_f"])[:] = b.to(built.dtype)
        elif e == "mio_weight_quant_w8":
            w = B["w"].view(t["w"])
            if d == "x_chunk_past_k":
                bf = B["w"]
                w = t["w"].as_strided((N, K + 8), bf.strides, bf.off)   # the row maximum taken over a chunk too many
                a = w.float().abs().amax(1)
                a = torch.where(torch.isnan(a), torch.full_like(a, float("nan")), a)
                scale = torch.where(a == 0, torch.ones_like(a), a / 448.0)
                q = (w[:, :K].float() * (1.0 / scale)[:, None]).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
            else:
                q, scale = quant_w8_reference(w)
            B["w8"].view(t["w8"])[:] = q
            B["scale"].view(t["scale"])[:] = scale
        else:
            M, per = c.M, c.N // c.slots_out
            st = B["stats_in"].view(t["stats_in"])
            mp = st.shape[1]
            src = st[:c.N].double().view(c.slots_out, per, mp, 2).sum(1)
            if d == "spare_slot":
                src = src + 0.0 * st[c.N].double()
            B["stats_red"].view(t["stats_red"])[:c.slots_out] = src.float()   # the padding rows too, from the input's


# ---- the launch ----------------------------------------------------------------------------------------------------------
def _dt(dtype):
    from mio import _lib
    return _lib.MIO_BF16 if dtype == torch.bfloat16 else _lib.MIO_FP16


def strides_of(built: Built):
    """(ldx, ldw, ldy, ldr) of a gemm case as the entry points and mio_gemm_route take them (a blocked operand: its row length)."""
    c, B = built.case, built.bufs
    ldx = c.K if c.x_blk else B["x"].strides[0]
    ldw = c.K if c.w_layout else B["w"].strides[0]
    ldy = c.N if c.y_blk else B["y"].strides[0]
    ldr = 0 if not c.res else c.N if c.res_blk else B["res"].strides[0]
    return ldx, ldw, ldy, ldr


def route(built: Built):
    """The route of the case's launch: mio_gemm_route (gemm; host-only) or mio.ops.fused_mlp_route's rule (mlp)."""
    from mio import _lib, ops
    c = built.case
    act = ops._ACT[c.act]
    if c.kind == "gemm":
        ldx, ldw, ldy, ldr = strides_of(built)
        return ops._gemm_route(c.M, c.N, c.K, ldx, ldw, ldy, ldr, act, c.res, c.w_layout, c.fold, c.stats_out)
    M, I, d = c.M, c.N, c.K
    ok = bool(_lib.lib.mio_fused_mlp_blocked_weight_ok(M, d, I, act))
    blocked = ok and (c.w_layout != 0 or not c.glu)
    w2 = _lib.W_BLOCKED if blocked and c.w_layout else _lib.W_PLAIN
    w1 = _lib.W_GLU if blocked and c.glu else w2
    return "/".join(["blocked" if blocked else "two_launch", ops._gemm_route(M, I, d, d, d, I, 0, act, False, w1),
                     ops._gemm_route(M, d, I, I, I, d, d, _lib.ACT_NONE, c.res, w2)])


def launch(built: Built, t, stream=0):
    """The case's launches through the C ABI on the device buffers t ({name: flat tensor}): the weight preparations from
    their hostile sources first, then the entry point.  Every pointer is its embedded view's."""
    import ctypes

    from mio import _lib, ops
    lib, c, B = _lib.lib, built.case, built.bufs
    dt = _dt(built.dtype)
    P = lambda n: B[n].ptr(t[n]) if n in t else None  # noqa: E731
    ok = lambda rc: _lib.check(rc)  # noqa: E731
    f32 = ctypes.c_float
    if c.kind == "gemm":
        M, N, K = c.M, c.N, c.K
        assert route(built) == c.route, (c.name, route(built))
        ldx, ldw, ldy, ldr = strides_of(built)
        act = ops._ACT[c.act]
        wsrc, gsrc, wld = "w", "wg", B["w"].strides[0]
        bias, bias_g = P("bias"), P("bias_g")
        if c.fold:
            if c.rms:
                for wn, sn in (("w", "ws"), ("wg", "wsg")):
                    if wn in t:
                        B[sn].view(t[sn]).copy_((B[wn].view(t[wn]).float() * B["gamma"].view(t["gamma"]).float())
                                                .to(built.dtype).reshape(-1))
            else:
                ok(lib.mio_ln_fold_weight(P("w"), wld, P("gamma"), P("beta"), P("bias"), P("ws"), P("bias_f"), N, K, dt, stream))
                bias = P("bias_f")
                if c.glu:
                    ok(lib.mio_ln_fold_weight(P("wg"), wld, P("gamma"), P("beta"), P("bias_g"), P("wsg"), P("bias_gf"), N, K, dt,
                                              stream))
                    bias_g = P("bias_gf")
            wsrc, gsrc, wld = "ws", "wsg", K
        if c.w_layout == 1:
            ok(lib.mio_weight_block(P(wsrc), wld, P("wb"), N, K, dt, stream))
        elif c.w_layout == 2:
            ok(lib.mio_weight_block_glu(P(gsrc), P(wsrc), wld, P("wb"), N, K, dt, stream))
        lo, hi, val = c.col_scale if c.col_scale is not None else (0, 0, 1.0)
        if c.entry == "mio_gemm_bias_act":
            ok(lib.mio_gemm_bias_act(P("x"), P("w"), bias, P("wg"), bias_g, P("res"), P("y"), M, N, K, ldx, ldw, ldy, ldr, act,
                                     dt, stream))
        elif c.entry == "mio_gemm_bias_act_bw":
            ok(lib.mio_gemm_bias_act_bw(P("x"), P("wb"), bias, P("res"), P("y"), M, N, K, ldx, ldy, ldr, act, dt, int(c.x_blk),
                                        stream))
        elif c.entry == "mio_gemm_bias_act_bw_cs":
            ok(lib.mio_gemm_bias_act_bw_cs(P("x"), P("wb"), bias, P("y"), M, N, K, ldx, ldy, act, dt, int(c.x_blk), lo, hi,
                                           f32(val), stream))
        else:
            fn = lib.mio_gemm_rms_bw if c.rms else lib.mio_gemm_ln_bw
            flags = int(c.x_blk) | 2 * int(c.y_blk) | 4 * int(c.res_blk)
            ok(fn(P("x"), P("wb"), bias, bias_g, P("res"), P("y"), M, N, K, ldx, ldy, ldr, act, dt, flags, P("ln_stats"),
                  K // 256 if c.fold else 0, f32(EPS), P("stats_out"), lo, hi, f32(val), stream))
    elif c.kind == "mlp":
        M, I, d = c.M, c.N, c.K
        assert route(built) == c.route, (c.name, route(built))
        act = ops._ACT[c.act]
        assert B["work"].shape[0] * 2 >= lib.mio_fused_mlp_workspace_bytes(M, d, I, act)
        if c.w_layout == 1:
            ok(lib.mio_weight_block(P("w1"), B["w1"].strides[0], P("w1b"), I, d, dt, stream))
        elif c.w_layout == 2:
            ok(lib.mio_weight_block_glu(P("wg"), P("w1"), B["w1"].strides[0], P("w1b"), I, d, dt, stream))
        if c.w_layout:
            ok(lib.mio_weight_block(P("w2"), B["w2"].strides[0], P("w2b"), d, I, dt, stream))
        tail = (P("res"), P("y"), P("work"), M, d, I)
        if c.entry == "mio_fused_mlp_fwd":
            ok(lib.mio_fused_mlp_fwd(P("x"), P("w1"), P("b1"), P("wg"), P("bg"), P("w2"), P("b2"), *tail, act, dt, stream))
        elif c.entry == "mio_fused_mlp_fwd_bw":
            ok(lib.mio_fused_mlp_fwd_bw(P("x"), P("w1b"), P("b1"), P("w2b"), P("b2"), *tail, act, dt, int(c.x_blk), stream))
        else:
            ok(lib.mio_fused_mlp_glu_fwd_bw(P("x"), P("w1b"), P("b1"), P("bg"), P("w2b"), P("b2"), *tail, dt, int(c.x_blk),
                                            stream))
    else:
        N, K, e = c.N, c.K, c.entry
        ldw = B["w"].strides[0] if "w" in B else 0
        if e == "mio_weight_block":
            ok(lib.mio_weight_block(P("w"), ldw, P("wb"), N, K, dt, stream))
        elif e == "mio_weight_block_glu":
            ok(lib.mio_weight_block_glu(P("wg"), P("w"), ldw, P("wb"), N, K, dt, stream))
        elif e == "mio_ln_fold_weight":
            ok(lib.mio_ln_fold_weight(P("w"), ldw, P("gamma"), P("beta"), P("bias"), P("ws"), P("bias_f"), N, K, dt, stream))
        elif e == "mio_weight_quant_w8":
            ok(lib.mio_weight_quant_w8(P("w"), ldw, P("w8"), B["w8"].strides[0], P("scale"), N, K, dt, stream))
        else:
            ok(lib.mio_ln_stats_reduce(P("stats_in"), c.N, P("stats_red"), c.slots_out, c.M, stream))
    for name, bf in B.items():
        assert bf.ptr(t[name]) % 16 == 0, (c.name, name)

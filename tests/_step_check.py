"""One whole decode step, judged stage by stage (a plain helper module, not a conftest).

The per-operation checkers (_rms_check, _gemm_check / _w8_check, _rope_check, _qknorm_check, _decode_check, _moe_check,
_sampling_check) each own one kernel.  This module chains the kernels the way a serving loop does -- RMSNorm, fused QKV decode
GEMM, the cache write on strided views of the QKV result (in place on q), paged decode, out-projection with the residual, RMSNorm,
MLP (dense SwiGLU or mixture of experts) with the residual, final RMSNorm, LM head, sampler -- and judges every stage of every step
against fp64 computed from THE DEVICE'S OWN INPUTS TO THAT STAGE (the stored 16-bit / fp8 values, the cache as stored), under the
unchanged bar of the checker that owns the operation.  No tolerance is introduced here: every number comes from those modules.

  StepSpec      one decoder form (frozen dataclass); FORMS are the three the tests run, SEAMS / reach() what their schedules reach.
  StepState     the tensors of a run on one device: constants (weights, tables, the teacher-forcing hidden-state table, the
                uniforms of every step) and the state that moves under a captured graph (context lengths, caches, fp8 scales,
                sampler rows, the row index of the hidden-state table).
  between()     the in-place updates a serving loop makes between two steps (row index, uniforms, one change of the fp8 scales,
                two sampler rows through set_row).
  build_step()  the step on mio.ops and the existing modules (mio.sampling.Sampler's tensors, MoEMLP's parameters and router);
                nothing in it synchronises or reads device data on the host.  Returns a dict of every stage's output.
  TorchStep     a torch / CPU model of the same step (fp32 stage arithmetic, one rounding where the header says so) with a
                defect= argument.  It exists only to prove the harness on the CPU (tests/test_step_check.py).
  judge_step()  raises StageFailure(stage, ...) at the first stage outside its bar.

Teacher forcing: the step's input hidden states are row `idx` of a fixed table, not an embedding of the sampled token, so a
rounding difference cannot fork a run.

The rules at the seams, all from include/mio_hip.h and restated in the references here, never special-cased per test:
  * a token's cache position is context_lengths[b] - q_len + i (lengths AFTER the append); a position past the block-table row is
    skipped and the cache keeps its bytes; decode ignores keys at positions >= table_width * block_size;
  * a rotating write's token whose position is outside [0, max_position) writes nothing and gets a q_out row of zeros, which
    then feeds attention (a zero query weighs every visible key alike); a token whose cache row is skipped still gets its q;
  * decode has no causal mask among the q_len rows; with a window row qi sees ctx - q_len + qi - left <= j < ctx.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional, Tuple

import torch

import _decode_check as dc
import _gemm_check as gc
import _hostile_decode as hd
import _moe_check as mc
import _qknorm_check as qk
import _rms_check as rms
import _rope_check as rc
import _sampling_check as sc
import _w8_check as w8c

F8 = torch.float8_e4m3fn
BF, FP = torch.bfloat16, torch.float16
STEPS = 24
SCALE_STEP = 12          # the fp8 scales change in place before this step
ROW_STEPS = (8, 15)      # Sampler.set_row before these steps
SWING = (20, 21)         # MoE forms: every token to one set of experts, then spread over all of them
STAGES = ("ctx", "input", "norm1", "qkv", "cache_write", "attention", "attn_out", "norm2", "router", "moe_route", "mlp_up",
          "mlp_down", "norm_f", "lm_head", "sample")


class StageFailure(AssertionError):
    def __init__(self, stage: str, msg: str):
        super().__init__(f"[{stage}] {msg}")
        self.stage = stage


@dataclass(frozen=True)
class StepSpec:
    name: str
    dtype: torch.dtype
    B: int
    q_len: int
    H: int
    Hkv: int
    D: int
    rot_dim: int                 # 0: no rotary (the plain write)
    pairing: Optional[str]       # "neox" | "interleaved" | None
    qk_norm: bool
    cache: str                   # "kv16" | "fp8"
    block_size: int
    window_left: int             # -1: none
    layers: int
    layer_idx: int
    gemm: str                    # "gemm_skinny" | "gemm_skinny_w8"
    mlp: str                     # "dense" | "moe"
    E: int
    top_k: int
    renormalize: bool
    activation: str
    d: int
    I: int
    V: int
    start_ctx: Tuple[int, ...]
    table_width: int
    max_position: int
    seed: int
    steps: int = STEPS
    eps: float = 1e-6

    @property
    def T(self):
        return self.B * self.q_len

    @property
    def cap(self):
        """Keys a block-table row holds; also the fixed max_seq_len of every decode launch, so the plan never changes."""
        return self.table_width * self.block_size

    @property
    def kv8(self):
        return self.cache == "fp8"

    @property
    def write(self):
        return "plain" if not self.rot_dim else ("qknorm_rope" if self.qk_norm else "rope")

    @property
    def interleaved(self):
        return self.pairing == "interleaved"


# The three forms.  Against the sizes the task sketches: the whole-token-row decode kernel is only ever chosen from 16 sequences
# on (dec_rows_ok), so the fp8 form runs B = 16 with one query vector per key; the other two stay at B <= 4.  A decode split holds
# at least 256 keys (dec_nsplit*), so the form that crosses a split boundary has a 20-page table row.
FORMS = (
    StepSpec("gqa-bf16-qknorm-kv16-dense", BF, B=4, q_len=1, H=8, Hkv=2, D=128, rot_dim=64, pairing="neox", qk_norm=True,
             cache="kv16", block_size=16, window_left=-1, layers=2, layer_idx=1, gemm="gemm_skinny", mlp="dense", E=0, top_k=0,
             renormalize=False, activation="swiglu", d=256, I=512, V=1003, start_ctx=(5, 250, 290, 0), table_width=20,
             max_position=300, seed=11),
    StepSpec("rows-fp16-rope-fp8-moe8", FP, B=16, q_len=1, H=4, Hkv=4, D=64, rot_dim=64, pairing="interleaved", qk_norm=False,
             cache="fp8", block_size=16, window_left=40, layers=3, layer_idx=1, gemm="gemm_skinny_w8", mlp="moe", E=8, top_k=2,
             renormalize=True, activation="swiglu", d=256, I=512, V=1000,
             start_ctx=(40, 85, 10, 0, 15, 16, 17, 31, 47, 60, 72, 3, 55, 64, 90, 33), table_width=6, max_position=128, seed=12),
    StepSpec("head-bf16-plain-kv16-moe64-verify", BF, B=2, q_len=4, H=2, Hkv=1, D=96, rot_dim=0, pairing=None, qk_norm=False,
             cache="kv16", block_size=16, window_left=-1, layers=2, layer_idx=0, gemm="gemm_skinny", mlp="moe", E=64, top_k=8,
             renormalize=False, activation="swiglu", d=256, I=512, V=65544, start_ctx=(6, 98), table_width=8, max_position=0,
             seed=13),
)


# ---- what a form's schedule reaches, from host-only queries -------------------------------------------------------------------
ALIGNED = 1 << 20  # a fake 16-byte aligned device address: the route queries dereference nothing


def decode_route(spec: StepSpec) -> str:
    """The decode kernel the step's paged_attention_forward takes (mio_fa3_decode_window_route / _kv8_route), from the strides the
    step hands over: q a view of the fused QKV rows, o [B, q_len, H, D] seen head-major."""
    from mio import _lib
    N = (spec.H + 2 * spec.Hkv) * spec.D
    qs = (C.c_int64 * 3)(spec.q_len * N, spec.D, N)
    os_ = (C.c_int64 * 3)(spec.q_len * spec.H * spec.D, spec.D, spec.H * spec.D)
    tail = (spec.B, spec.H, spec.Hkv, spec.q_len, spec.D, spec.layers, spec.layer_idx, spec.block_size, spec.table_width, spec.cap,
            1.0 / math.sqrt(spec.D))
    dt = 0 if spec.dtype == BF else 1
    if spec.kv8:
        r = _lib.lib.mio_fa3_decode_kv8_route(*([ALIGNED] * 8), qs, os_, *tail, spec.window_left, dt, None, None)
    else:
        r = _lib.lib.mio_fa3_decode_window_route(*([ALIGNED] * 6), qs, os_, *tail, spec.window_left, -1, dt, None, None)
    assert r >= 0, (spec.name, _lib.lib.mio_last_error().decode())
    return _lib.DECODE_ROUTES[r]


def decode_plan(spec: StepSpec, route: str):
    """(nsplit, split_len) of the step's decode launch: tests/_hostile_decode.plan, the suite's mirror of dec_plan."""
    case = hd.Case(spec.name, route, spec.kv8, spec.dtype, spec.B, spec.H, spec.Hkv, spec.D, spec.q_len, spec.block_size,
                   spec.window_left, spec.cap, tuple(spec.start_ctx), spec.table_width, False, 0, "none")
    return hd.plan(case)


def router_gemm(spec: StepSpec) -> str:
    """The GEMM MoEMLP._router_logits takes for the step's T rows: "skinny" or the gemm_bias_act route name."""
    from mio import ops
    Ep = (spec.E + 7) // 8 * 8
    if ops.gemm_skinny_ok(spec.T, Ep, spec.d, "none"):
        return "skinny"
    x = torch.empty(spec.T, spec.d, dtype=spec.dtype)
    return ops.gemm_route(x, torch.empty(Ep, spec.d, dtype=spec.dtype))


def reach(spec: StepSpec) -> set:
    """The names of what the form and its schedule reach (the coverage table of tests/test_step_check.py)."""
    from mio import ops
    got = {"write:" + spec.write, "gemm:" + spec.gemm, "mlp:" + spec.mlp, "cache:" + spec.cache}
    route = decode_route(spec)
    got.add("decode:" + route)
    got.add("sampler:lds" if spec.V <= 65536 else "sampler:reread")
    if spec.V % 8:
        got.add("V%8")
    nsplit, split_len = decode_plan(spec, route)
    bs, cap, q_len, left = spec.block_size, spec.cap, spec.q_len, spec.window_left
    for b, c0 in enumerate(spec.start_ctx):
        for s in range(spec.steps):
            after = c0 + (s + 1) * q_len
            for pos in range(after - q_len, after):
                if pos > 0 and pos % bs == 0 and pos < cap:
                    got.add("seam:page")
                if spec.rot_dim and pos >= spec.max_position:
                    got.add("seam:max_position")
                if pos >= cap and (not spec.rot_dim or pos < spec.max_position):
                    got.add("seam:table_full")
            before = after - q_len
            if nsplit > 1 and 0 < before and (min(before, cap) - 1) // split_len != (min(after, cap) - 1) // split_len:
                got.add("seam:split")
            if left >= 0 and max(0, before - q_len - left) < bs <= max(0, after - q_len - left):
                got.add("seam:window_page")
    if spec.mlp == "moe":
        got.add("moe_up_splits:%d" % ops.moe_up_splits(spec.T, spec.top_k, spec.E, spec.I, spec.d, spec.activation))
        got.add("moe_down_splits:%d" % ops.moe_down_splits(spec.T, spec.top_k, spec.E, spec.d, spec.I))
    return got


NEEDED = {"write:qknorm_rope", "write:rope", "write:plain", "decode:head", "decode:rows", "decode:gqa", "gemm:gemm_skinny",
          "gemm:gemm_skinny_w8", "mlp:dense", "mlp:moe", "cache:kv16", "cache:fp8", "sampler:lds", "sampler:reread", "V%8",
          "seam:page", "seam:split", "seam:window_page", "seam:table_full", "seam:max_position"}


# ---- the tensors of a run -------------------------------------------------------------------------------------------------------
def quantize_w8(w: torch.Tensor):
    """(w8, scale) by ops.quantize_weight_w8's formula in torch: both backends read these very bytes and scales."""
    wf = w.float()
    scale = wf.abs().amax(1) / 448.0
    scale = torch.where(scale > 0, scale, torch.ones_like(scale))
    inv = (torch.tensor(1.0) / scale)[:, None]
    return (wf * inv).clamp(-448, 448).to(F8), scale


_CONSTS: dict = {}


def consts(spec: StepSpec) -> SimpleNamespace:
    """The constants and the initial moving state of a form on the CPU, drawn once per process from spec.seed."""
    if spec.name in _CONSTS:
        return _CONSTS[spec.name]
    g = torch.Generator().manual_seed(spec.seed)
    dt, d, I, V, H, Hkv, D, T = spec.dtype, spec.d, spec.I, spec.V, spec.H, spec.Hkv, spec.D, spec.T
    rn = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(dt)  # noqa: E731
    c = SimpleNamespace()
    c.g1, c.g2, c.gf = ((1 + 0.1 * torch.randn(d, generator=g)).to(dt) for _ in range(3))
    c.qw, c.kw = ((1 + 0.1 * torch.randn(D, generator=g)).to(dt) for _ in range(2))
    c.w = {"qkv": rn((H + 2 * Hkv) * D, d, scale=d ** -0.5), "wo": rn(d, H * D, scale=(H * D) ** -0.5),
           "lm": rn(V, d, scale=2 * d ** -0.5)}
    if spec.mlp == "dense":
        c.w.update(up=rn(I, d, scale=d ** -0.5), gate=rn(I, d, scale=d ** -0.5), down=rn(d, I, scale=I ** -0.5))
    else:
        E = spec.E
        c.router = rn(E, d, scale=2 * d ** -0.5)
        c.w_up, c.w_gate, c.w_down = rn(E, I, d, scale=d ** -0.5), rn(E, I, d, scale=d ** -0.5), rn(E, d, I, scale=I ** -0.5)
    c.w8 = {k: quantize_w8(v) for k, v in c.w.items()} if spec.gemm == "gemm_skinny_w8" else None
    if spec.rot_dim:
        inv_freq = 10000.0 ** (-torch.arange(0, spec.rot_dim, 2, dtype=torch.float64) / spec.rot_dim)
        ang = torch.arange(spec.max_position, dtype=torch.float64)[:, None] * inv_freq[None, :]
        c.cos, c.sin = ang.cos().float(), ang.sin().float()
    c.hidden = rn(spec.steps, T, d)
    if spec.mlp == "moe":   # the routing swing: large rows along router directions, so norm2's rows are those directions
        rw, g2 = c.router.float(), c.g2.float()
        one = rw[:spec.top_k].sum(0) / g2
        c.hidden[SWING[0]] = (8 * one / one.pow(2).mean().sqrt()).to(dt).expand(T, d)
        for t in range(T):
            pick = [(t * spec.top_k + j) % spec.E for j in range(spec.top_k)]
            v = rw[pick].sum(0) / g2
            c.hidden[SWING[1], t] = (8 * v / v.pow(2).mean().sqrt()).to(dt)
    c.u_table = torch.rand(spec.steps, T, generator=g)
    # pages: every sequence owns table_width pages of a permutation; three spare pages belong to nobody
    nb = spec.B * spec.table_width + 3
    perm = torch.randperm(nb, generator=g)
    c.bt = perm[3:].view(spec.B, spec.table_width).to(torch.int32).contiguous()
    c.spare = perm[:3].clone()
    shape = (nb, spec.layers, spec.block_size, Hkv, D)
    c.k_scale0 = torch.tensor([0.9, 0.0125, 1.7][:spec.layers], dtype=torch.float32)
    c.v_scale0 = torch.tensor([1.3, 0.0111, 0.47][:spec.layers], dtype=torch.float32)
    if spec.kv8:
        c.kc0 = dc.quantise(torch.randn(shape, generator=g), float(c.k_scale0[spec.layer_idx]))
        c.vc0 = dc.quantise(torch.randn(shape, generator=g), float(c.v_scale0[spec.layer_idx]))
    else:
        c.kc0, c.vc0 = rn(*shape), rn(*shape)
    c.cu = (torch.arange(spec.B + 1) * spec.q_len).to(torch.int32)
    c.ctx0 = torch.tensor(spec.start_ctx, dtype=torch.int32)
    _CONSTS[spec.name] = c
    return c


class CpuSampler:
    """mio.sampling.Sampler's tensors and set_row on the CPU (the class itself refuses a CPU device)."""

    def __init__(self, batch: int):
        self.batch = batch
        self.temperature = torch.zeros(batch)
        self.top_k = torch.zeros(batch, dtype=torch.int32)
        self.top_p = torch.ones(batch)
        self.min_p = torch.zeros(batch)
        self.u = torch.zeros(batch)

    def set_row(self, i, temperature=None, top_k=None, top_p=None, min_p=None):
        for t, v in ((self.temperature, temperature), (self.top_k, top_k), (self.top_p, top_p), (self.min_p, min_p)):
            if v is not None:
                t[i].fill_(v)


_ROWS = (dict(temperature=1.0), dict(temperature=0.0), dict(temperature=0.8, top_k=40, top_p=0.9),
         dict(temperature=1.3, min_p=0.05))


class StepState:
    """A run's tensors on `device`.  hostile: the pages no table row names and all other layers hold NaN (fp8: byte 0x7f)."""

    def __init__(self, spec: StepSpec, device="cpu", hostile: bool = False):
        c = consts(spec)
        self.spec, self.device = spec, torch.device(device)
        to = lambda t: t.to(self.device)  # noqa: E731
        self.g1, self.g2, self.gf, self.qw, self.kw = (to(t) for t in (c.g1, c.g2, c.gf, c.qw, c.kw))
        self.w = {k: to(v) for k, v in c.w.items()}
        self.w8 = None if c.w8 is None else {k: (to(q), to(s)) for k, (q, s) in c.w8.items()}
        if spec.rot_dim:
            self.cos, self.sin = to(c.cos), to(c.sin)
        self.hidden, self.u_table, self.bt, self.cu = to(c.hidden), to(c.u_table), to(c.bt), to(c.cu)
        if spec.mlp == "moe":
            self.router, self.w_up, self.w_gate, self.w_down = (to(t) for t in (c.router, c.w_up, c.w_gate, c.w_down))
        # ---- what moves under a captured step
        self.ctx = c.ctx0.clone().to(self.device)
        kc, vc = c.kc0.clone(), c.vc0.clone()
        if hostile:
            for cache in (kc, vc):
                nan = dc.nan_cache(cache.shape, cache.dtype)
                other = [l for l in range(spec.layers) if l != spec.layer_idx]
                cache[:, other] = nan[:, other]
                cache[c.spare] = nan[c.spare]
        self.k_cache, self.v_cache = to(kc), to(vc)
        self.k_scale, self.v_scale = to(c.k_scale0.clone()), to(c.v_scale0.clone())
        self.idx = torch.zeros(1, dtype=torch.int64, device=self.device)
        if self.device.type == "cuda":
            from mio.sampling import Sampler
            self.sampler = Sampler(spec.T, self.device)
        else:
            self.sampler = CpuSampler(spec.T)
        for i in range(spec.T):
            self.sampler.set_row(i, **_ROWS[i % len(_ROWS)])
        self.moe = None
        if spec.mlp == "moe" and self.device.type == "cuda":
            from mio.kernels.mlp import MoEConfig, MoEMLP
            m = MoEMLP(spec.d, spec.I, spec.E, spec.top_k, MoEConfig(spec.activation, spec.renormalize, spec.dtype))
            m = m.to(device=self.device, dtype=spec.dtype)
            with torch.no_grad():
                m.router.weight.copy_(self.router)
                m.w_up.copy_(self.w_up)
                m.w_gate.copy_(self.w_gate)
                m.w_down.copy_(self.w_down)
            self.moe = m

    def snapshot(self) -> SimpleNamespace:
        """The moving state on the CPU."""
        f = lambda t: t.detach().to("cpu", copy=True)  # noqa: E731
        s = self.sampler
        return SimpleNamespace(ctx=f(self.ctx), k_cache=f(self.k_cache), v_cache=f(self.v_cache), k_scale=f(self.k_scale),
                               v_scale=f(self.v_scale), idx=int(f(self.idx)), temperature=f(s.temperature), top_k=f(s.top_k),
                               top_p=f(s.top_p), min_p=f(s.min_p), u=f(s.u))


def between(spec: StepSpec, st: StepState, step: int) -> None:
    """What the loop changes before step `step`, all in place: the hidden-state row index, the uniforms, the fp8 scales once
    mid-run, two sampler rows through set_row."""
    st.idx.fill_(step)
    st.sampler.u.copy_(st.u_table[step])
    if spec.kv8 and step == SCALE_STEP:
        l = spec.layer_idx
        st.k_scale[l:l + 1].mul_(1.5)
        st.v_scale[l:l + 1].mul_(1.25)
    if step == ROW_STEPS[0]:
        st.sampler.set_row(0, temperature=0.0)                           # a sampling row turns greedy
    if step == ROW_STEPS[1]:
        st.sampler.set_row(1, temperature=0.9, top_k=5, top_p=0.8)       # a greedy row starts sampling


# ---- the step on the HIP kernels ------------------------------------------------------------------------------------------------
def build_step(spec: StepSpec, st: StepState, keep=None):
    """step() -> dict of stage outputs (keep: only these names, so everything else is freed inside the step and a graph pool
    recycles it).  Every launch is a mio.ops call; the torch ops are the in-place advance of context_lengths (the first node), the
    gather of the hidden-state row, views, and one clone of q before the write overwrites it (the judge needs the write's input)."""
    from mio import ops
    dt, B, q_len, H, Hkv, D, T = spec.dtype, spec.B, spec.q_len, spec.H, spec.Hkv, spec.D, spec.T
    HD, KD, bs, layer = H * D, Hkv * D, spec.block_size, spec.layer_idx
    kv = dict(k_scale=st.k_scale, v_scale=st.v_scale) if spec.kv8 else {}
    smp = st.sampler

    def gemm(name, x, act="none", gate=None, residual=None):
        if spec.gemm == "gemm_skinny":
            return ops.gemm_skinny(x, st.w[name], None, act, None if gate is None else st.w[gate], None, residual)
        q, s = st.w8[name]
        qg, sg = (None, None) if gate is None else st.w8[gate]
        return ops.gemm_skinny_w8(x, q, s, None, act, qg, sg, None, residual)

    def step():
        out = {}
        st.ctx.add_(q_len)
        x = st.hidden.index_select(0, st.idx).view(T, spec.d)
        xn = ops.rmsnorm(x, st.g1, spec.eps)
        qkv = gemm("qkv", xn)
        q, k, v = qkv[:, :HD].view(T, H, D), qkv[:, HD:HD + KD].view(T, Hkv, D), qkv[:, HD + KD:].view(T, Hkv, D)
        q_pre = q.clone()
        tables = (st.k_cache, st.v_cache, st.bt, st.cu, st.ctx, bs, layer)
        if spec.write == "qknorm_rope":
            ops.qknorm_rope_and_cache_varlen(q, k, v, *tables, st.cos, st.sin, st.qw, st.kw, eps=spec.eps,
                                             interleaved=spec.interleaved, q_out=q, **kv)
        elif spec.write == "rope":
            ops.rope_and_cache_varlen(q, k, v, *tables, st.cos, st.sin, interleaved=spec.interleaved, q_out=q, **kv)
        else:
            ops.reshape_and_cache_varlen(k, v, *tables, **kv)
        o = torch.empty(B, q_len, H, D, dtype=dt, device=qkv.device)
        ops.paged_attention_forward(q.view(B, q_len, H, D).permute(0, 2, 1, 3), o.permute(0, 2, 1, 3), st.k_cache, st.v_cache,
                                    st.bt, st.ctx, bs, spec.cap, layer, window_size=(spec.window_left, -1), **kv)
        y1 = gemm("wo", o.view(T, HD), residual=x)
        xn2 = ops.rmsnorm(y1, st.g2, spec.eps)
        if spec.mlp == "dense":
            h = gemm("up", xn2, "swiglu", gate="gate")
            y2 = gemm("down", h, residual=y1)
        else:
            m = st.moe
            rl = m._router_logits(xn2, dt)
            route = ops.moe_route(rl, spec.top_k, spec.renormalize)
            h = ops.moe_up(xn2, route, m.w_up.detach(), spec.activation, m.w_gate.detach())
            y2 = ops.moe_down(h, route, m.w_down.detach(), residual=y1)
            out.update(router_logits=rl, route_ids=route.ids, route_weights=route.weights, route_offsets=route.expert_offsets,
                       route_sorted=route.sorted_rows, route_pos=route.row_pos)
        xf = ops.rmsnorm(y2, st.gf, spec.eps)
        logits = gemm("lm", xf)
        tokens = ops.sample_tokens(logits, smp.temperature, smp.top_k, smp.top_p, smp.min_p, u=smp.u)
        out.update(x=x, norm1=xn, qkv=qkv, q_pre=q_pre, attn=o, attn_out=y1, norm2=xn2, mlp_h=h, mlp_out=y2, norm_f=xf,
                   logits=logits, tokens=tokens)
        return out if keep is None else {n: out[n] for n in keep}

    return step


def snap(stages: dict) -> dict:
    return {k: v.detach().to("cpu", copy=True) for k, v in stages.items()}


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.detach().contiguous().view(torch.uint8)


def same_bits(a: dict, b: dict, names=None) -> list:
    """The names whose tensors differ in any byte."""
    return [n for n in (names or a) if a[n].shape != b[n].shape or not torch.equal(bits(a[n]), bits(b[n]))]


# ---- the torch / CPU model ------------------------------------------------------------------------------------------------------
DEFECTS = ("rope_positions_frozen", "ctx_frozen", "page_row_early", "k_without_norm", "v_scale_for_k", "scale_frozen",
           "window_off_by_one", "out_proj_residual_dropped", "router_not_renormalised", "sampler_previous_logits",
           "sampler_row_frozen")


def _rms32(x, w, eps):
    xf = x.float()
    return (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + torch.tensor(eps, dtype=torch.float32)) * w.float())


def _rot32(n, cos, sin, pos, interleaved):
    """n fp32 [T, heads, D] rotated in its first 2 * cos.shape[1] elements at positions pos (long [T])."""
    half = cos.shape[1]
    rot = 2 * half
    c, s = cos[pos][:, None, :], sin[pos][:, None, :]
    y = n.clone()
    if interleaved:
        x1, x2 = n[..., 0:rot:2], n[..., 1:rot:2]
        y[..., 0:rot:2], y[..., 1:rot:2] = x1 * c - x2 * s, x2 * c + x1 * s
    else:
        x1, x2 = n[..., :half], n[..., half:rot]
        y[..., :half], y[..., half:rot] = x1 * c - x2 * s, x2 * c + x1 * s
    return y


class TorchStep:
    """The step in torch on the CPU: fp32 stage arithmetic, one rounding where the header says so.  defect: one of DEFECTS."""

    def __init__(self, spec: StepSpec, st: StepState, defect: Optional[str] = None):
        assert defect is None or defect in DEFECTS, defect
        self.spec, self.st, self.defect = spec, st, defect
        self.first = None          # what a "frozen at capture" defect captured
        self.prev_logits = None
        self.route = decode_route(spec)

    def _gemm(self, name, x, act="none", gate=None, residual=None):
        st = self.st

        def z(n):
            if st.w8 is None:
                return x.float() @ st.w[n].float().t()
            q, s = st.w8[n]
            return s[None, :] * (x.float() @ q.float().t())

        y = z(name)
        if act == "swiglu":
            y = torch.nn.functional.silu(z(gate)) * y
        if residual is not None:
            y = y + residual.float()
        return y.to(self.spec.dtype)

    def __call__(self):
        spec, st, df = self.spec, self.st, self.defect
        dt, B, q_len, H, Hkv, D, T = spec.dtype, spec.B, spec.q_len, spec.H, spec.Hkv, spec.D, spec.T
        HD, KD, bs, layer = H * D, Hkv * D, spec.block_size, spec.layer_idx
        out = {}
        if df != "ctx_frozen":
            st.ctx.add_(q_len)
        if self.first is None:
            self.first = SimpleNamespace(ctx=st.ctx.clone(), k_scale=st.k_scale.clone(), v_scale=st.v_scale.clone(),
                                         temperature=st.sampler.temperature.clone(), top_k=st.sampler.top_k.clone(),
                                         top_p=st.sampler.top_p.clone())
        x = st.hidden[int(st.idx)].view(T, spec.d)
        xn = _rms32(x, st.g1, spec.eps).to(dt)
        qkv = self._gemm("qkv", xn)
        q, k, v = qkv[:, :HD].view(T, H, D), qkv[:, HD:HD + KD].view(T, Hkv, D), qkv[:, HD + KD:].view(T, Hkv, D)
        q_pre = q.clone()
        # ---- the cache write
        tok = torch.arange(T)
        b_of, i_of = tok // q_len, tok % q_len
        pos = st.ctx.long()[b_of] - q_len + i_of
        rpos = (self.first.ctx.long()[b_of] - q_len + i_of) if df == "rope_positions_frozen" else pos
        live = torch.ones(T, dtype=torch.bool)
        ks, vs = st.k_scale[layer], st.v_scale[layer]
        if df == "scale_frozen":
            ks, vs = self.first.k_scale[layer], self.first.v_scale[layer]
        if df == "v_scale_for_k":
            ks = vs
        kf = k.float()
        if spec.rot_dim:
            live = (rpos >= 0) & (rpos < spec.max_position)
            rp = rpos.clamp(0, spec.max_position - 1)
            qn = _rms32(q, st.qw, spec.eps) if spec.qk_norm else q.float()
            kn = _rms32(k, st.kw, spec.eps) if (spec.qk_norm and df != "k_without_norm") else k.float()
            qr = _rot32(qn, st.cos, st.sin, rp, spec.interleaved)
            kf = _rot32(kn, st.cos, st.sin, rp, spec.interleaved)
            q.copy_(torch.where(live[:, None, None], qr, torch.zeros_like(qr)).to(dt))
        wpos = pos.clone()
        if df == "page_row_early":
            wpos = torch.where((pos % bs == 0) & (pos > 0), pos - 1, pos)
        ok = live & (wpos >= 0) & (wpos < spec.cap)
        if bool(ok.any()):
            blk = st.bt.long()[b_of[ok], wpos[ok] // bs]
            slot = wpos[ok] % bs
            if spec.kv8:
                inv_k, inv_v = torch.tensor(1.0) / ks, torch.tensor(1.0) / vs
                st.k_cache[blk, layer, slot] = (kf[ok] * inv_k).clamp(-448, 448).to(F8)
                st.v_cache[blk, layer, slot] = (v[ok].float() * inv_v).clamp(-448, 448).to(F8)
            else:
                st.k_cache[blk, layer, slot] = kf[ok].to(dt)
                st.v_cache[blk, layer, slot] = v[ok]
        # ---- attention: _decode_check.model, the fp32 chain the decode bars are taken from
        left = spec.window_left + (1 if (df == "window_off_by_one" and spec.window_left >= 0) else 0)
        sc_kw = dict(k_scale=float(st.k_scale[layer]), v_scale=float(st.v_scale[layer])) if spec.kv8 else {}
        o4 = dc.model(q.view(B, q_len, H, D).permute(0, 2, 1, 3), st.k_cache, st.v_cache, st.bt, st.ctx, bs, layer, dtype=dt,
                      p16=self.route == "gqa", left=left, **sc_kw)
        o = o4.permute(0, 2, 1, 3).contiguous()
        y1 = self._gemm("wo", o.view(T, HD), residual=None if df == "out_proj_residual_dropped" else x)
        xn2 = _rms32(y1, st.g2, spec.eps).to(dt)
        if spec.mlp == "dense":
            h = self._gemm("up", xn2, "swiglu", gate="gate")
            y2 = self._gemm("down", h, residual=y1)
        else:
            E, kk = spec.E, spec.top_k
            rl = (xn2.float() @ st.router.float().t()).to(dt)
            xc = mc.canon(rl)
            ids = torch.stack([mc.order(xc[t])[:kk] for t in range(T)])
            p = torch.softmax(rl.float(), -1)
            w = p.gather(1, ids)
            if spec.renormalize and df != "router_not_renormalised":
                w = w / w.sum(1, keepdim=True)
            offsets, srt, rpos_ = mc.group_rows(ids, E)
            tk = srt // kk
            ex = ids.reshape(-1)[srt]
            xf32 = xn2.float()[tk]
            up = torch.einsum("pd,pid->pi", xf32, st.w_up.float()[ex])
            ga = torch.einsum("pd,pid->pi", xf32, st.w_gate.float()[ex])
            h = (torch.nn.functional.silu(ga) * up).to(dt)
            z = torch.einsum("pi,pdi->pd", h.float(), st.w_down.float()[ex])        # by sorted position
            acc = torch.zeros(T, spec.d)
            for j in range(kk):
                acc = acc + w[:, j:j + 1] * z[rpos_[torch.arange(T) * kk + j]]
            y2 = (acc + y1.float()).to(dt)
            out.update(router_logits=rl, route_ids=ids.to(torch.int32), route_weights=w, route_offsets=offsets.to(torch.int32),
                       route_sorted=srt.to(torch.int32), route_pos=rpos_.to(torch.int32))
        xf = _rms32(y2, st.gf, spec.eps).to(dt)
        logits = self._gemm("lm", xf)
        smp = st.sampler
        src = logits
        if df == "sampler_previous_logits" and self.prev_logits is not None:
            src = self.prev_logits
        self.prev_logits = logits
        par = self.first if df == "sampler_row_frozen" else smp
        tokens = torch.empty(T, dtype=torch.int64)
        for r in range(T):
            ref = sc.reference(src[r].float().numpy(), float(par.temperature[r]), int(par.top_k[r]), float(par.top_p[r]),
                               float(smp.min_p[r]))
            tokens[r] = sc.token_of(ref, float(smp.u[r]))
        out.update(x=x, norm1=xn, qkv=qkv, q_pre=q_pre, attn=o, attn_out=y1, norm2=xn2, mlp_h=h, mlp_out=y2, norm_f=xf,
                   logits=logits, tokens=tokens)
        return out


# ---- the judge ------------------------------------------------------------------------------------------------------------------
def _stage(name):
    def deco(fn):
        def run(*a, **kw):
            try:
                return fn(*a, **kw)
            except StageFailure:
                raise
            except AssertionError as e:
                raise StageFailure(name, str(e)) from None
        return run
    return deco


def reference_stage(spec: StepSpec, stage: str, x, *, residual=None, weight=None) -> gc.Ref:
    """The fp64 reference and element bound (a _gemm_check.Ref) of one row-kernel or GEMM stage from the stage's stored input x:
    stage "norm1" / "norm2" / "norm_f" (weight: the norm's), "qkv" / "attn_out" / "mlp_up" / "mlp_down" / "lm_head" (the dense
    GEMMs, 16-bit or fp8 weights by spec.gemm) or "router".  The other stages' references need more than one operand and live in
    their _judge_* functions, each on the checker that owns the operation."""
    c = consts(spec)
    if stage.startswith("norm"):
        return rms.reference_rows(x, weight, spec.eps)
    if stage == "router":
        Ep = (spec.E + 7) // 8 * 8
        w = torch.cat([c.router, c.router.new_zeros(Ep - spec.E, spec.d)]) if Ep != spec.E else c.router
        return gc.reference(x, w)
    name, act, gate = {"qkv": ("qkv", "none", None), "attn_out": ("wo", "none", None), "mlp_up": ("up", "swiglu", "gate"),
                       "mlp_down": ("down", "none", None), "lm_head": ("lm", "none", None)}[stage]
    if spec.gemm == "gemm_skinny":
        return gc.reference(x, c.w[name], None, act, None if gate is None else c.w[gate], None, residual)
    q, s = c.w8[name]
    qg, sg = (None, None) if gate is None else c.w8[gate]
    return w8c.reference_w8(x, q, s, None, act, qg, sg, None, residual)


def _judge_norm(spec, stage, x, w, y):
    @_stage(stage)
    def run():
        gc.check(y, reference_stage(spec, stage, x, weight=w), spec.dtype, "rmsnorm", bars=False, what=stage)
    run()


def _bars(spec, stage, y, ref, route, key, pool):
    """gc.check under the bars of gc.BARS[key], as the tests that own the GEMMs apply them, with one difference of sample size:
    the worst row, the mean row and the worst 16x16 fragment are held per step; the fraction of elements that are not the
    round-to-nearest of the reference is a rate measured on matrices of 10^5 .. 10^7 elements, and one step's stage has a few
    hundred to a few thousand (one element of the 512 router logits is 0.002, above bf16's 0.00151), so it is pooled over the
    steps of a run in `pool` and held to the same bar by judge_pool()."""
    bars = gc.BARS[key]
    stt = gc.check(y, ref, spec.dtype, route, bars=(1.0,) + tuple(bars[1:]), what=stage)
    if pool is not None:
        rec = pool.setdefault(stage, [0.0, 0, bars[0]])
        rec[0] += stt["not_rn"] * ref.y.numel()
        rec[1] += ref.y.numel()


def judge_pool(spec: StepSpec, pool: dict) -> None:
    """The pooled not-round-to-nearest fractions of a run against their bars (_bars)."""
    for stage, (bad, n, bar) in pool.items():
        if n and bad / n > bar:
            raise StageFailure(stage, f"{bad:.0f} of {n} elements over the run are not the round-to-nearest of the reference: "
                                      f"{bad / n:.5f} (bar {bar})")


def _judge_gemm(spec, stage, x, y, residual=None, pool=None):
    @_stage(stage)
    def run():
        ref = reference_stage(spec, stage, x, residual=residual)
        # both decode GEMMs are held to the bars of (dtype, "t128"): tests/test_gpu_gemm_skinny.py, tests/_w8_check.py
        _bars(spec, stage, y, ref, "skinny" if spec.gemm == "gemm_skinny" else "skinny_w8", (spec.dtype, "t128"), pool)
    run()


def _rows_eq(a, b):
    return torch.equal(bits(a), bits(b))


@_stage("cache_write")
def _judge_cache_write(spec, c, before, st, after):
    dt, B, q_len, H, Hkv, D, T = spec.dtype, spec.B, spec.q_len, spec.H, spec.Hkv, spec.D, spec.T
    HD, KD, bs, layer = H * D, Hkv * D, spec.block_size, spec.layer_idx
    qkv = st["qkv"]
    q_out, k, v = qkv[:, :HD].reshape(T, H, D), qkv[:, HD:HD + KD].reshape(T, Hkv, D), qkv[:, HD + KD:].reshape(T, Hkv, D)
    q_pre = st["q_pre"]
    tok = torch.arange(T)
    b_of, i_of = tok // q_len, tok % q_len
    pos = after.ctx.long()[b_of] - q_len + i_of
    ks, vs = float(before.k_scale[layer]), float(before.v_scale[layer])
    rot = spec.rot_dim
    live = ((pos >= 0) & (pos < spec.max_position)) if rot else torch.ones(T, dtype=torch.bool)
    kref = kdel = None
    if rot:
        dead = ~live
        assert not bool((q_out[dead].float() != 0).any()), "a token at a dead rotation position has a q_out row that is not zeros"
        if bool(live.any()):
            pl = pos[live]
            if spec.qk_norm:
                qref, qdel = qk.reference(q_pre[live], c.qw, spec.eps, c.cos, c.sin, pl, spec.interleaved)
                kref, kdel = qk.reference(k[live], c.kw, spec.eps, c.cos, c.sin, pl, spec.interleaved)
                bad, _ = rc.outside16(q_out[live], qref, qdel, dt)
            else:
                qref, qdel = rc.reference(q_pre[live], c.cos, c.sin, pl, spec.interleaved)
                kref, kdel = rc.reference(k[live], c.cos, c.sin, pl, spec.interleaved)
                bad, _ = rc.outside16(q_out[live][..., :rot], qref, qdel, dt)
                assert _rows_eq(q_out[live][..., rot:], q_pre[live][..., rot:]), "q_out past rot_dim is not q"
            assert bad == 0, f"{bad} elements of q_out outside the rotation's interval"
    else:
        assert _rows_eq(q_out, q_pre), "the plain write changed q"
    ok = live & (pos >= 0) & (pos < spec.cap)
    want_k, want_v = before.k_cache.clone(), before.v_cache.clone()
    blk = c.bt.long()[b_of[ok], pos[ok] // bs]
    slot = pos[ok] % bs
    got_k = after.k_cache[blk, layer, slot]
    if bool(ok.any()):
        # V, and K where nothing is computed: exact bytes
        want_v[blk, layer, slot] = dc.quantise(v[ok], vs) if spec.kv8 else v[ok]
        exact_k = dc.quantise(k[ok], ks) if spec.kv8 else k[ok]
        if rot:
            sel = ok[live]                          # the live tokens whose row is written
            kr, kd = kref[sel], kdel[sel]
            width = D if spec.qk_norm else rot
            if spec.kv8:
                bad = rc.outside8(got_k[..., :width], kr, kd, ks)
            else:
                bad, _ = rc.outside16(got_k[..., :width], kr, kd, dt)
            assert bad == 0, f"{bad} elements of the cached K outside the interval of the rotated (normalised) key"
            exact_k[..., :width] = got_k[..., :width]   # judged above; the rest of the row must be the plain write's bytes
        want_k[blk, layer, slot] = exact_k
    for name, got, want in (("k_cache", after.k_cache, want_k), ("v_cache", after.v_cache, want_v)):
        diff = (bits(got) != bits(want)).view(got.shape[0], got.shape[1], got.shape[2], -1).any(-1)
        if bool(diff.any()):
            blk_, l_, s_ = (int(t) for t in diff.nonzero()[0])
            mine = bool(((blk == blk_) & (slot == s_)).any()) and l_ == layer
            raise AssertionError(f"{name}: {int(diff.sum())} slots differ from the write's contract, first (block {blk_}, layer "
                                 f"{l_}, slot {s_}), " + ("a row this step writes" if mine else "a row this step does not own"))


@_stage("attention")
def _judge_attention(spec, c, before, st, after, route):
    B, q_len, H, Hkv, D, T = spec.B, spec.q_len, spec.H, spec.Hkv, spec.D, spec.T
    q4 = st["qkv"][:, :H * D].reshape(B, q_len, H, D).permute(0, 2, 1, 3)
    o4 = st["attn"].permute(0, 2, 1, 3)
    kw = dict(left=spec.window_left)
    if spec.kv8:
        kw.update(k_scale=float(before.k_scale[spec.layer_idx]), v_scale=float(before.v_scale[spec.layer_idx]))
    args = (q4, after.k_cache, after.v_cache, c.bt, after.ctx, spec.block_size, spec.layer_idx)
    ref, lse = dc.reference(*args, **kw)
    mo = dc.model(*args, dtype=spec.dtype, p16=route == "gqa", **kw)
    dc.check(o4, ref, lse, spec.dtype, (spec.dtype, route, spec.cache), mo, what="step", win=spec.window_left >= 0)


@_stage("moe_route")
def _judge_route(spec, st):
    ref = mc.route_reference(st["router_logits"], spec.top_k, spec.renormalize)
    mc.check_route(ref, st["route_ids"], st["route_weights"], st["route_offsets"], st["route_sorted"], st["route_pos"], "step")


@_stage("sample")
def _judge_sample(spec, before, st):
    lg, tok = st["logits"].float().numpy(), st["tokens"]
    for r in range(spec.T):
        ref = sc.reference(lg[r], float(before.temperature[r]), int(before.top_k[r]), float(before.top_p[r]),
                           float(before.min_p[r]))
        adm = sc.admissible(ref, float(before.u[r])).tolist()
        assert int(tok[r]) in adm, (f"row {r}: token {int(tok[r])} is not admissible on the stored logits (admissible {adm[:4]}, "
                                    f"temperature {float(before.temperature[r])}, top_k {int(before.top_k[r])})")


def judge_step(spec: StepSpec, before, stages: dict, after, route: Optional[str] = None, pool: Optional[dict] = None) -> None:
    """before / after: StepState.snapshot() around the step (before: after between()); stages: snap() of the step's dict.  Raises
    StageFailure naming the first stage (in STAGES order) outside its bar.  pool: a dict shared by the steps of one run, for
    judge_pool() at its end."""
    c, st, dt = consts(spec), stages, spec.dtype
    route = route or decode_route(spec)
    if not torch.equal(after.ctx, before.ctx + spec.q_len):
        raise StageFailure("ctx", f"context_lengths {after.ctx.tolist()} after {before.ctx.tolist()} + {spec.q_len}")
    if not _rows_eq(st["x"].reshape(spec.T, spec.d), c.hidden[before.idx]):
        raise StageFailure("input", f"the hidden states are not row {before.idx} of the table")
    x = st["x"].reshape(spec.T, spec.d)
    _judge_norm(spec, "norm1", x, c.g1, st["norm1"])
    # the write's q is judged from q_pre; k and v of the stored buffer are the GEMM's own
    qkv_gemm = st["qkv"].clone()
    qkv_gemm[:, :spec.H * spec.D] = st["q_pre"].reshape(spec.T, -1)
    _judge_gemm(spec, "qkv", st["norm1"], qkv_gemm, pool=pool)
    _judge_cache_write(spec, c, before, st, after)
    _judge_attention(spec, c, before, st, after, route)
    _judge_gemm(spec, "attn_out", st["attn"].reshape(spec.T, -1), st["attn_out"], residual=x, pool=pool)
    _judge_norm(spec, "norm2", st["attn_out"], c.g2, st["norm2"])
    if spec.mlp == "dense":
        _judge_gemm(spec, "mlp_up", st["norm2"], st["mlp_h"], pool=pool)
        _judge_gemm(spec, "mlp_down", st["mlp_h"], st["mlp_out"], residual=st["attn_out"], pool=pool)
    else:
        @_stage("router")
        def router():
            ref = reference_stage(spec, "router", st["norm2"])
            ref = gc.Ref(ref.y[:, :spec.E], ref.tol[:, :spec.E], ref.K)
            rg = router_gemm(spec)
            _bars(spec, "router", st["router_logits"], ref, rg, (dt, "t128" if rg == "skinny" else rg), pool)
        router()
        _judge_route(spec, st)
        kern = SimpleNamespace(expert_offsets=st["route_offsets"], sorted_rows=st["route_sorted"], row_pos=st["route_pos"],
                               ids=st["route_ids"], weights=st["route_weights"], top_k=spec.top_k, num_experts=spec.E)

        @_stage("mlp_up")
        def up():
            # _moe_check.check_up's bars: (dtype, "t128")
            _bars(spec, "mlp_up", st["mlp_h"], mc.up_reference(st["norm2"], kern, c.w_up, spec.activation, c.w_gate), "moe_up",
                  (dt, "t128"), pool)

        @_stage("mlp_down")
        def down():
            mc.check_down(st["mlp_out"], mc.down_reference(st["mlp_h"], kern, c.w_down, residual=st["attn_out"]), dt, "step")
        up()
        down()
    _judge_norm(spec, "norm_f", st["mlp_out"], c.gf, st["norm_f"])
    _judge_gemm(spec, "lm_head", st["norm_f"], st["logits"], pool=pool)
    _judge_sample(spec, before, st)


def run_model(spec: StepSpec, defect: Optional[str] = None, steps=None, judge: bool = True):
    """The TorchStep loop over the schedule on the CPU; returns the records [(before, stages, after)]."""
    st = StepState(spec, "cpu")
    step = TorchStep(spec, st, defect)
    route = step.route
    recs, pool = [], {}
    for s in (range(spec.steps) if steps is None else steps):
        between(spec, st, s)
        before = st.snapshot()
        stages = snap(step())
        after = st.snapshot()
        if judge:
            try:
                judge_step(spec, before, stages, after, route, pool)
            except StageFailure as e:
                e.step = s
                raise
        recs.append((before, stages, after))
    if judge:
        try:
            judge_pool(spec, pool)
        except StageFailure as e:
            e.step = spec.steps
            raise
    return recs

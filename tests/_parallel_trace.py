"""Launch-record recorder for the tensor- and sequence-parallel sub-layers (a plain helper module, not a conftest).

record() replaces ops.gemm_bias_act, ops.fa3_fwd, ops.layernorm and ops.block_weight on the mio.ops module by recorders that launch
nothing: each notes its call and returns a torch.empty tensor of the shape and dtype the kernel would return, on the CPU.  Every
query stays real (ops.col_scale_ok, ops.fa3_k_prescaled_ok, ops.blocked_weight_ok), so which branch a module takes is decided as in
the product.  Without a process group tp_rank() is 0 and a ring of sp_size 2 attends its local shard only; every decision under
test is made from sizes and config alone, so that is enough.  The record of a call holds the function, the operands' shapes,
strides and dtypes, the flags of the launch (the column-scale value rounded to fp32, as the C ABI receives it) and whether the
optional operands were given.

CASES is the table of cases; run_case() runs one forward on a fresh module.  `python tests/_parallel_trace.py OUT.json` writes the
record of every case; tests/golden/parallel_traces.json is that file.
"""
from __future__ import annotations

import json
import os
import struct
import sys
import weakref
from typing import Callable, Dict, List, NamedTuple, Optional

import torch
import torch.nn as nn

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (_ROOT, os.path.join(_ROOT, "ml-inference-optimizer_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from mio import ops  # noqa: E402
from mio.parallelism import (ColumnParallelLinear, RowParallelLinear, SequenceParallelAttention, SequenceParallelConfig,  # noqa: E402
                             SequenceParallelMLP, TensorParallelAttention, TensorParallelConfig, TensorParallelMLP)

GOLDEN = os.path.join(_ROOT, "tests", "golden", "parallel_traces.json")
BF = torch.bfloat16


# ---- the recorders -----------------------------------------------------------------------------------------------------------
def _t(v: Optional[torch.Tensor]):
    return None if v is None else [list(v.shape), list(v.stride()), str(v.dtype).replace("torch.", "")]


def _f32(v: Optional[float]):
    return None if v is None else struct.unpack("f", struct.pack("f", v))[0]


class record:
    """with record() as calls: ...  -- calls is the list of call records of the block (.repacked holds a weak reference to every
    blocked copy the block made, .norm_params the (weight, bias) tensors of every layernorm call)."""

    def __enter__(self) -> List[dict]:
        self.calls: List[dict] = []
        self.repacked: List[weakref.ref] = []
        self.norm_params: List[tuple] = []
        self.saved = {n: getattr(ops, n) for n in ("gemm_bias_act", "fa3_fwd", "layernorm", "block_weight")}
        for n in self.saved:
            setattr(ops, n, getattr(self, "_" + n))
        return self.calls

    def __exit__(self, *exc):
        for n, fn in self.saved.items():
            setattr(ops, n, fn)
        return False

    def _gemm_bias_act(self, x, w, bias=None, activation="none", w_gate=None, bias_gate=None, residual=None, out=None,
                       w_blocked=None, x_blocked_shape=None, col_scale=None):
        assert w_gate is None and bias_gate is None and x_blocked_shape is None
        cs = None if col_scale is None else [col_scale[0], col_scale[1], _f32(col_scale[2])]
        self.calls.append({"fn": "gemm_bias_act", "x": _t(x), "w": _t(w), "bias": _t(bias), "activation": activation,
                           "col_scale": cs, "w_blocked": _t(w_blocked), "residual": _t(residual), "out": _t(out)})
        return out if out is not None else torch.empty(*x.shape[:-1], w.shape[0], dtype=x.dtype)

    def _fa3_fwd(self, q, k, v, *, layout="bshd", causal=False, softmax_scale=None, keep_mask=None, additive_mask=None,
                 return_lse=False, out=None, o_acc=None, lse=None, carry_in=False, write_out=True, q_offset=0, k_offset=0,
                 k_prescaled=False, out_blocked=False, window_size=(-1, -1)):
        assert not return_lse and not out_blocked and tuple(window_size) == (-1, -1) and keep_mask is None
        self.calls.append({"fn": "fa3_fwd", "q": _t(q), "k": _t(k), "v": _t(v), "layout": layout, "causal": causal,
                           "softmax_scale": _f32(softmax_scale), "k_prescaled": k_prescaled, "carry_in": carry_in,
                           "write_out": write_out, "q_offset": q_offset, "k_offset": k_offset, "mask": _t(additive_mask),
                           "out": _t(out), "o_acc": _t(o_acc), "lse": _t(lse)})
        if not write_out:
            return None
        return out if out is not None else torch.empty(q.shape, dtype=q.dtype)

    def _layernorm(self, x, weight, bias=None, eps=1e-5, residual=None, residual_alpha=1.0, return_sum=False, out_blocked=False):
        assert residual is None and not return_sum and not out_blocked
        self.norm_params.append((weight, bias))
        self.calls.append({"fn": "layernorm", "x": _t(x), "weight": _t(weight), "bias": _t(bias), "eps": eps})
        return torch.empty(x.shape, dtype=x.dtype)

    def _block_weight(self, w):
        self.calls.append({"fn": "block_weight", "w": _t(w)})
        wb = torch.empty((w.shape[0] + 255) // 256 * 256, w.shape[1], dtype=w.dtype)
        self.repacked.append(weakref.ref(wb))
        return wb


def k_answers(trace: List[dict]) -> List[tuple]:
    """[(col_scale of the GEMM that produced K, k_prescaled)] per attention launch: the column-scaled GEMM is the last one before
    the launches it feeds (a ring makes several launches on one K)."""
    out, cs, used = [], None, True
    for r in trace:
        if r["fn"] == "gemm_bias_act" and r["col_scale"] is not None:
            assert used, "a column-scaled projection without an attention launch behind it"
            cs, used = tuple(r["col_scale"]), False
        if r["fn"] == "fa3_fwd":
            out.append((cs, r["k_prescaled"]))
            used = True
    assert used, "a column-scaled projection without an attention launch behind it"
    return out


# ---- the cases ---------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    cls: str                           # the module under test
    build: Callable[[], dict]          # -> state: the module and its inputs
    call: Callable[[dict], object]
    kpre: Optional[bool] = None        # attention cases: K is expected pre-scaled / unscaled
    claims: Callable[[], None] = lambda: None   # the ops.*_ok facts that make the case the one it says it is


def _x(*shape, dtype=BF):
    return torch.zeros(*shape, dtype=dtype)


def _tp_case(name, kpre, shape=(3, 4096), d=1024, H=16, mask=False, cross=False, claims=lambda: None):
    B, S = shape

    def build():
        m = TensorParallelAttention(d, H, TensorParallelConfig(world_size=2, tp_size=2), causal=True, is_cross_attention=cross)
        m = m.to(BF).eval()
        st = {"m": m, "x": _x(B, S, d), "kw": {}}
        if mask:
            st["kw"]["attention_mask"] = _x(B, 1, 1, S)
        if cross:
            st["kw"]["encoder_hidden_states"] = _x(B, S, d)
        return st

    return Case(name, "TensorParallelAttention", build, lambda st: st["m"](st["x"], residual=st["x"], **st["kw"]), kpre, claims)


def _sp_case(name, kpre, shape=(4, 4096), d=1024, H=16, mode="ring", causal=True, zigzag=True, mask=False, claims=lambda: None):
    """(A ring takes an additive mask only without causal, and zig-zag placement only with it: the mask case is the non-causal
    ring with one change.)"""
    B, Sl = shape

    def build():
        cfg = SequenceParallelConfig(world_size=2, sp_size=2, attention_handling=mode, exchange="mesh", causal=causal, zigzag=zigzag)
        m = SequenceParallelAttention(d, H, cfg, attention_dropout=0.0).to(BF).eval()
        return {"m": m, "x": _x(B, Sl, d), "kw": {"attention_mask": _x(B, 1, 1, Sl)} if mask else {}}

    return Case(name, "SequenceParallelAttention", build, lambda st: st["m"](st["x"], residual=st["x"], **st["kw"]), kpre, claims)


def _tp_mlp_prenorm_fp32():
    d, I = 1024, 4096

    def build():
        m = TensorParallelMLP(d, I, TensorParallelConfig(world_size=2, tp_size=2), activation="gelu").to(BF).eval()
        return {"m": m, "x": _x(3, 4096, d), "norm": nn.LayerNorm(d)}  # the norm's parameters stay fp32: cast per use

    return Case("tp_mlp_prenorm_fp32", "TensorParallelMLP", build,
                lambda st: st["m"](st["x"], residual=st["x"], pre_norm=st["norm"]))


def _row_residual():
    def build():
        m = RowParallelLinear(4096, 1024, config=TensorParallelConfig(world_size=2, tp_size=2), input_is_parallel=True).to(BF).eval()
        return {"m": m, "x": _x(4, 4096, 2048), "res": _x(4, 4096, 1024)}

    return Case("row_parallel_residual", "RowParallelLinear", build, lambda st: st["m"](st["x"], residual=st["res"]))


def _sp_mlp():
    def build():
        cfg = SequenceParallelConfig(world_size=2, sp_size=2)
        return {"m": SequenceParallelMLP(1024, 4096, cfg).to(BF).eval(), "x": _x(4, 4096, 1024), "norm": nn.LayerNorm(1024).to(BF)}

    return Case("sp_mlp", "SequenceParallelMLP", build, lambda st: st["m"](st["x"], residual=st["x"], pre_norm=st["norm"]))


def column_linear():
    """A ColumnParallelLinear at the smallest blocked-weight shape, for an input of COLUMN_X (the cache tests build hundreds)."""
    assert ops.blocked_weight_ok(65536, 128, 128)
    return ColumnParallelLinear(128, 256, config=TensorParallelConfig(world_size=2, tp_size=2), gather_output=False).to(BF).eval()


COLUMN_X = (65536, 128)


# the ops.*_ok facts: every "unscaled" case differs from its taken case in the one term it names
def _taken():
    assert ops.col_scale_ok(3 * 4096, 1536, 1024) and ops.fa3_k_prescaled_ok(3, 4096, 4096, 8, 64, 1536, 1536)
    assert ops.col_scale_ok(4 * 4096, 1024, 1024) and ops.fa3_k_prescaled_ok(4, 2048, 2048, 16, 64, 1024, 1024, carry=True)
    assert ops.fa3_k_prescaled_ok(4, 4096, 4096, 16, 64, 1024, 1024, carry=True)


def _short():
    assert ops.col_scale_ok(96 * 128, 1536, 1024) and not ops.fa3_k_prescaled_ok(96, 128, 128, 8, 64, 1536, 1536)
    assert ops.col_scale_ok(64 * 256, 1024, 1024) and not ops.fa3_k_prescaled_ok(64, 128, 128, 16, 64, 1024, 1024, carry=True)


def _d128():
    assert ops.col_scale_ok(3 * 4096, 1536, 1024) and not ops.fa3_k_prescaled_ok(3, 4096, 4096, 4, 128, 1536, 1536)
    assert not ops.fa3_k_prescaled_ok(4, 2048, 2048, 8, 128, 1024, 1024, carry=True)


def _hidden256():
    assert not ops.col_scale_ok(3 * 4096, 384, 256) and ops.fa3_k_prescaled_ok(3, 4096, 4096, 2, 64, 384, 384)
    assert not ops.col_scale_ok(4 * 4096, 256, 256) and ops.fa3_k_prescaled_ok(4, 2048, 2048, 4, 64, 256, 256, carry=True)


def _odd_columns():
    """Everything says yes but the column range: 9 local heads of 64 = [576, 1152), and 17 heads of 64 = [0, 1088)."""
    assert ops.col_scale_ok(3 * 4096, 1728, 1152) and ops.fa3_k_prescaled_ok(3, 4096, 4096, 9, 64, 1728, 1728)
    assert ops.col_scale_ok(4 * 4096, 1088, 1088) and ops.fa3_k_prescaled_ok(4, 2048, 2048, 17, 64, 1088, 1088, carry=True)


CASES: List[Case] = [
    _tp_case("tp_self_taken", True, claims=_taken),                                          # 1
    _sp_case("sp_ring_zigzag_taken", True, claims=_taken),                                   # 2
    _tp_case("tp_self_mask", False, mask=True),                                              # 3
    _sp_case("sp_ring_noncausal_taken", True, causal=False, zigzag=False, claims=_taken),
    _sp_case("sp_ring_noncausal_mask", False, causal=False, zigzag=False, mask=True),        # 3
    _tp_case("tp_self_s128", False, shape=(96, 128), claims=_short),                         # 4
    _sp_case("sp_ring_zigzag_s256", False, shape=(64, 256), claims=_short),                  # 4
    _tp_case("tp_self_d128", False, H=8, claims=_d128),                                      # 5
    _sp_case("sp_ring_zigzag_d128", False, H=8, claims=_d128),                               # 5
    _tp_case("tp_self_hidden256", False, d=256, H=4, claims=_hidden256),                     # 6
    _sp_case("sp_ring_zigzag_hidden256", False, d=256, H=4, claims=_hidden256),              # 6
    _tp_case("tp_self_n576", False, d=1152, H=18, claims=_odd_columns),                      # 7
    _sp_case("sp_ring_zigzag_hidden1088", False, d=1088, H=17, claims=_odd_columns),         # 7
    _sp_case("sp_full_zigzag", False, mode="full"),                                          # 8
    _sp_case("sp_local", False, mode="local"),                                               # 9
    _sp_case("sp_ring_plain_taken", True, zigzag=False, claims=_taken),                      # 10
    _tp_case("tp_cross", False, cross=True),                                                 # 11
    _tp_mlp_prenorm_fp32(),                                                                  # 12
    _row_residual(),                                                                         # 13
    _sp_mlp(),                                                                               # 14
]


def case(name: str) -> Case:
    return next(c for c in CASES if c.name == name)


@torch.no_grad()
def run_case(c: Case) -> dict:
    """{"cls", "kpre", "trace"} of the first forward of a fresh module; the second forward on it must be the first without the
    weight repacks (the caches at work)."""
    c.claims()
    torch.manual_seed(0)
    st = c.build()
    with record() as cold:
        c.call(st)
    with record() as warm:
        c.call(st)
    assert warm == [r for r in cold if r["fn"] != "block_weight"], f"{c.name}: the second forward is not the first without repacks"
    if c.kpre is not None:
        ans = k_answers(cold)
        assert ans and all(k == c.kpre and (cs is not None) == c.kpre for cs, k in ans), (c.name, ans)
    return {"cls": c.cls, "kpre": c.kpre, "trace": cold}


def load_golden() -> Dict[str, dict]:
    with open(GOLDEN) as f:
        return json.load(f)


if __name__ == "__main__":
    with open(sys.argv[1], "w") as f:
        json.dump({c_.name: run_case(c_) for c_ in CASES}, f, indent=1, sort_keys=True)
        f.write("\n")

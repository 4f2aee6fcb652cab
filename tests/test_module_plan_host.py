"""CPU-only tests of mio._nn.attention_plan against the recorded launch traces (tests/golden/module_traces.json): for every
attention case the plan, called with that case's sizes and flags (ints and bools only), answers what the trace shows -- the
col_scale argument of the projection that produces K, and k_prescaled / out_blocked on the attention launch."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "module_traces.json")) as _f:
    GOLDEN = json.load(_f)
ATTN = sorted(n for n, c in GOLDEN.items() if c["attn"] is not None)
FLAGS = ("mask", "normalize_query", "return_softmax", "windowed", "rotary", "carry")


def _plan(a, **over):
    from mio._nn import attention_plan
    a = dict(a, **over)
    args = (a["B"], a["Sq"], a["Sk"], a["H"], a["Hkv"], a["D"], (a["k_rows"], a["k_n"], a["k_k"]), (a["k_lo"], a["k_hi"]),
            a["kv_stride"], None if a["o_n"] is None else (a["B"] * a["Sq"], a["o_n"], a["o_k"]))
    flat = [v for arg in args for v in (arg if isinstance(arg, tuple) else (arg,)) if v is not None]
    assert all(type(v) in (int, bool) for v in flat) and all(type(a[f]) is bool for f in FLAGS)
    return attention_plan(*args, **{f: a[f] for f in FLAGS})


def _evidence(trace):
    """[(col_scale of the K projection, k_prescaled, out_blocked)] per attention launch of the trace: the column-scaled GEMM is
    the last one before the launch (none: K left its projection unscaled)."""
    out, cs = [], None
    for r in trace:
        a = r["args"]
        if r["fn"] in ("gemm_bias_act", "gemm_ln") and a["col_scale"] is not None:
            assert cs is None, "two column-scaled projections in front of one attention launch"
            cs = tuple(a["col_scale"])
        if r["fn"] == "fa3_fwd":
            out.append((cs, a["k_prescaled"], a["out_blocked"]))
            cs = None
    assert cs is None, "a column-scaled projection without an attention launch behind it"
    return out


def test_the_record_covers_both_answers():
    ev = [e for n in ATTN for e in _evidence(GOLDEN[n]["trace"])]
    assert {(e[1], e[2]) for e in ev} == {(False, False), (True, False), (True, True)}


@pytest.mark.parametrize("name", ATTN)
def test_plan_answers_what_the_trace_shows(name):
    case = GOLDEN[name]
    plan = _plan(case["attn"])
    ev = _evidence(case["trace"])
    assert ev, "an attention case without an attention launch"
    for cs, kpre, oblk in ev:
        assert (plan.kpre, plan.out_blocked) == (kpre, oblk)
        assert plan.col_scale == cs  # the same float: (lo, hi, softmax_scale * log2(e))
        assert (plan.col_scale is not None) == plan.kpre


@pytest.mark.parametrize("flag", FLAGS)
def test_every_flag_alone_rules_pre_scaled_k_out(flag):
    a = GOLDEN["self_large_causal"]["attn"]
    assert _plan(a).kpre and _plan(a).out_blocked
    carry_d64 = flag == "carry"  # (the carry alone keeps pre-scaled K at head dim 64; it rules the blocked output out)
    p = _plan(a, **{flag: True})
    assert p.kpre == carry_d64 and not p.out_blocked and (p.col_scale is None) == (not carry_d64)


def test_plan_is_a_function_of_its_arguments():
    a = GOLDEN["self_large_causal"]["attn"]
    assert _plan(a) == _plan(a) and _plan(a, k_lo=a["k_lo"] + 64).kpre is False
    assert _plan(a, o_n=None, o_k=None) == _plan(a)._replace(out_blocked=False)
    assert not _plan(a, Sq=128, Sk=128).kpre and not _plan(a, D=128).kpre


_CHILD = """
import json, sys
sys.path[:0] = {paths!r}
from mio._nn import attention_plan
a = json.loads(sys.argv[1])
p = attention_plan(a["B"], a["Sq"], a["Sk"], a["H"], a["Hkv"], a["D"], (a["k_rows"], a["k_n"], a["k_k"]), (a["k_lo"], a["k_hi"]),
                   a["kv_stride"], (a["B"] * a["Sq"], a["o_n"], a["o_k"]))
print(json.dumps([p.kpre, p.col_scale is not None, p.out_blocked]))
"""


@pytest.mark.parametrize("var,want", [("MIO_NO_BLOCKED_W", [False, False, False]), ("MIO_NO_BLOCKED_X", [True, True, False])])
def test_switches_set_before_import(var, want):
    """MIO_NO_BLOCKED_W=1: no pre-scaled K (and so no blocked output); MIO_NO_BLOCKED_X=1: no blocked output."""
    env = dict(os.environ, **{var: "1"})
    code = _CHILD.format(paths=[ROOT, os.path.join(ROOT, "ml-inference-optimizer_amd")])
    r = subprocess.run([sys.executable, "-c", code, json.dumps(GOLDEN["self_large_causal"]["attn"])], env=env,
                       capture_output=True, text=True, check=True)
    assert json.loads(r.stdout.strip().splitlines()[-1]) == want

"""CPU-only tests of what the tensor- and sequence-parallel sub-layers ask of mio.ops (tests/_parallel_trace.py: recorders in
place of the four launching functions, every query real, no process group).

tests/golden/parallel_traces.json was recorded before these modules took their K-prescale decision from mio._nn.attention_plan
and their weight copies from a CastCache of their own: the same launches with the same arguments must come out now.  The cache
tests state what the modules' caches promise; the 300-module one is the single intended difference from that earlier state, where
a process-wide memo was emptied at 256 entries and the second pass made 300 repacks."""
import gc
import math
import struct

import pytest
import torch

import _parallel_trace as pt
from mio import ops

GOLDEN = pt.load_golden()
ATTENTION = ("TensorParallelAttention", "SequenceParallelAttention")


def test_the_record_has_every_case():
    assert sorted(GOLDEN) == sorted(c.name for c in pt.CASES)


@pytest.mark.parametrize("cls", ATTENTION)
def test_the_record_covers_both_answers(cls):
    got = {k for c in GOLDEN.values() if c["cls"] == cls for _, k in pt.k_answers(c["trace"])}
    assert got == {True, False}
    assert {c["kpre"] for c in GOLDEN.values() if c["cls"] == cls} == {True, False}


@pytest.mark.parametrize("name", [c.name for c in pt.CASES])
def test_trace_is_the_recorded_one(name):
    """(run_case also asserts the expected K answer and that a second forward repeats the first without any repack.)"""
    got, want = pt.run_case(pt.case(name)), GOLDEN[name]
    assert got["kpre"] == want["kpre"] and got["cls"] == want["cls"]
    assert len(got["trace"]) == len(want["trace"])
    for i, (g, w) in enumerate(zip(got["trace"], want["trace"])):
        assert g == w, (name, i)


def test_plan_scale_is_the_recorded_literal_in_fp32():
    """attention_plan computes (1 / sqrt(D)) * LOG2E where these modules had D ** -0.5 * 1.4426950408889634: the C ABI takes the
    scale as a 32-bit float, and the two round to the same one for every head dim a pre-scaled-K launch takes."""
    from mio._nn import LOG2E
    dims = [D for D in range(1, 513) if ops.fa3_k_prescaled_ok(1, 256, 256, 1, D, D, D)]
    assert 64 in dims and 96 in dims
    for D in dims:
        assert struct.pack("f", (1.0 / math.sqrt(D)) * LOG2E) == struct.pack("f", D ** -0.5 * 1.4426950408889634), D


# ---- the modules' caches -----------------------------------------------------------------------------------------------------
def _repacks(c, st):
    with pt.record() as calls:
        c.call(st)
    return [(i, r["w"][0]) for i, r in enumerate(calls) if r["fn"] == "block_weight"], calls


@pytest.mark.parametrize("name,param,shape,before", [
    ("tp_self_taken", lambda m: m.key.weight, [1536, 1024], 0),          # the concatenated q / k / v weight, made again
    ("tp_self_taken", lambda m: m.query.bias, None, None),               # a bias: concatenated again, nothing repacked
    ("sp_ring_zigzag_taken", lambda m: m.key.weight, [1024, 1024], 1),   # q, K, v, out: the repack stands before the second GEMM
    ("sp_mlp", lambda m: m.dense_4h_to_h.weight, [1024, 4096], 1),       # layernorm, fc1, fc2
    ("row_parallel_residual", lambda m: m.weight, [1024, 2048], 0),
    ("tp_mlp_prenorm_fp32", lambda m: m.dense_h_to_4h.weight, [2048, 1024], 0),
])
@torch.no_grad()
def test_in_place_update_repacks_that_weight_once(name, param, shape, before):
    c = pt.case(name)
    st = c.build()
    _repacks(c, st)
    assert _repacks(c, st)[0] == []
    param(st["m"]).add_(1)
    got, calls = _repacks(c, st)
    if shape is None:
        assert got == []
    else:
        assert [s for _, s in got] == [shape]
        assert [r["fn"] for r in calls[:got[0][0]]].count("gemm_bias_act") == before
    assert _repacks(c, st)[0] == []


@torch.no_grad()
def test_cast_norm_parameters_are_kept():
    """tp_mlp_prenorm_fp32: the fp32 norm's weight and bias reach the row kernel as bf16 copies, the same two on every forward,
    and new ones after an in-place update."""
    c = pt.case("tp_mlp_prenorm_fp32")
    st = c.build()
    rec = pt.record()
    with rec:
        c.call(st)
        c.call(st)
        st["norm"].weight.add_(1)
        c.call(st)
    (w0, b0), (w1, b1), (w2, b2) = rec.norm_params
    assert w0.dtype == b0.dtype == torch.bfloat16 and w1 is w0 and b1 is b0 and w2 is not w0 and b2 is b0


@torch.no_grad()
def test_300_modules_keep_their_blocked_weights():
    """Each module owns its copy: nothing is repacked on the second pass over 300 modules.  (Before, a process-wide memo emptied
    at 256 entries made that pass repack all 300: the one intended change of behaviour.)"""
    mods, x = [pt.column_linear() for _ in range(300)], torch.zeros(*pt.COLUMN_X, dtype=pt.BF)
    with pt.record() as first:
        for m in mods:
            m(x)
    with pt.record() as second:
        for m in mods:
            m(x)
    assert [r["fn"] for r in first].count("block_weight") == 300
    assert [r["fn"] for r in second] == ["gemm_bias_act"] * 300 and all(r["w_blocked"] is not None for r in second)


@pytest.mark.parametrize("name", ["tp_self_taken", "sp_ring_zigzag_taken", "sp_mlp", "row_parallel_residual"])
@torch.no_grad()
def test_blocked_copies_die_with_the_module(name):
    c = pt.case(name)
    st = c.build()
    rec = pt.record()
    with rec:
        c.call(st)
    assert rec.repacked and all(r() is not None for r in rec.repacked)
    del st
    gc.collect()
    assert all(r() is None for r in rec.repacked)

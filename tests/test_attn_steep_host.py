"""No-GPU tests of tests/_attn_steep.py: for every launch of tests/test_gpu_attention_steep.py (_attn_steep.CASES, both
storage dtypes) the inputs do what the profile is for, the 16-bit-P chain under the kernels' rules stays inside the bars
the GPU test applies, and the chain with a defect injected into its rare branch does not.

The input conditions, on move_plan over the fp64 scores of exactly the tensors the GPU test launches (fp8 cases: over the
cache the CPU quantisation formula gives):
  spikes   at least a quarter of the live rows move; at least half of the 16-row groups hold, at some tile, a row that moves
           and one that does not; at least a quarter of the moved rows carry >= 10 % of their final weight across a move;
           a carry: at least an eighth of the rows move at tile 0 of a later shard (the CARRY form of the move);
  rising   every row with three or more visible tiles moves at least twice;
  falling  no move after a row's first visible tile; at least half of the keys of every row that sees 512 or more lie
           below 2^-24 of the row maximum (their P runs through fp16's subnormals to zero).
One exception, by arithmetic: under window_size = (100, 0) a row sees 101 keys.  The lazy rule in bf16 moves a row only for
a key 2^6 above its maximum, which the ~64 keys of 2^score about 1.3 each before it cannot balance to 10 %: there the share
asked for is the quarter of what the window can hold at all, 100 * 1.3 / (2^spike_h + 100 * 1.3) / 4.

The defects (lazy_chain's `defect`): alpha not applied, alpha taken from the row 16 away, the next tile's scores not
shifted, the trigger ignored.  The first three must fail the judgement wherever rows move.  An ignored trigger leaves P
growing with the scores, which costs nothing until P leaves the storage format -- bf16 has fp32's exponent range, and
the margins exist for fp16's -- so that defect must fail exactly where 2^(row maximum - first reference) overflows the
dtype (every `rising` case in fp16, the longest in bf16), and is shown to pass elsewhere: no output check can see it there.
"""
import math

import pytest
import torch

import _attn_check as ac
import _attn_steep as st

DTYPES = [torch.bfloat16, torch.float16]
CASES = [pytest.param(c, id=c.id) for c in st.CASES]


# ---------------------------------------------------------------------------------------------------------------------
# move_plan and lazy_chain on hand-made scores
# ---------------------------------------------------------------------------------------------------------------------
def _scores(rows):
    """[1,1,R,128] scores: each row (a, b) holds a in tile 0 and b in tile 1 (one key each, the others 20 below)."""
    s = torch.full((1, 1, len(rows), 128), 0.0, dtype=torch.float64)
    for r, (a, b) in enumerate(rows):
        s[0, 0, r, :64] = a - 20.0
        s[0, 0, r, 64:] = b - 20.0
        s[0, 0, r, 5] = a
        s[0, 0, r, 70] = b
    return s


def test_move_plan_thresholds():
    """The three triggers at their edges: lazy moves at MARGIN + 1 above the last maximum (6 in bf16, 3 in fp16) and not
    just below; the threshold rules above 6; a wave-mate's trigger drags a row whose maximum merely grew; a carried row
    moves from lse + 1 (lazy, no margin) / lse + 6."""
    s = _scores([(0.0, 5.9), (0.0, 6.0), (0.0, 2.9), (0.0, 3.0), (0.0, -1.0)])
    assert st.move_plan(s, "lazy", dtype=torch.bfloat16)["moves"][0, 0, :, 1].tolist() == [False, True, False, False, False]
    assert st.move_plan(s, "lazy", dtype=torch.float16)["moves"][0, 0, :, 1].tolist() == [True, True, False, True, False]
    assert not st.move_plan(s, "lazy")["moves"][..., 0].any()  # a fresh row's first tile is no move
    t = _scores([(0.0, 6.0), (0.0, 0.5), (0.0, -1.0)])
    assert st.move_plan(t, "fwd3")["moves"][0, 0, :, 1].tolist() == [False, False, False]
    t = _scores([(0.0, 6.1), (0.0, 0.5), (0.0, -1.0)])
    assert st.move_plan(t, "fwd3")["moves"][0, 0, :, 1].tolist() == [True, True, False]  # row 1 dragged, row 2 did not grow
    far = torch.cat([t, _scores([(0.0, 0.5)] * 40)], dim=2)  # rows 32.. sit in another fwd1 wave, in the same fwd3 wave
    m1, m3 = st.move_plan(far, "fwd1")["moves"][0, 0, :, 1], st.move_plan(far, "fwd3")["moves"][0, 0, :, 1]
    assert not m1[32:].any() and m3[32:].all() and m1[:2].all()
    lse = torch.full((1, 1, 3), 4.0 / st.LOG2E, dtype=torch.float64)  # a carried reference of 4 base-2 units
    c = _scores([(4.9, 0.0), (5.0, 0.0), (10.1, 0.0)])
    assert st.move_plan(c, "lazy", carried_lse=lse)["moves"][0, 0, :, 0].tolist() == [False, True, True]
    assert st.move_plan(c, "fwd1", carried_lse=lse)["moves"][0, 0, :, 0].tolist() == [True, True, True]  # (two dragged)
    assert not st.move_plan(c[:, :, :2], "fwd1", carried_lse=lse[..., :2])["moves"].any()
    # share: the move at tile 1 carries tile 0's weight: one key of 2^0 (and 63 of 2^-20) against one of 2^6
    sh = st.move_plan(_scores([(0.0, 6.0)]), "lazy")["share"][0, 0, 0].item()
    assert abs(sh - 1.0 / 65.0) < 1e-4
    # hidden first tile: the row stays fresh, its first visible tile is no move
    h = _scores([(0.0, 9.0)])
    h[..., :64] = float("-inf")
    p = st.move_plan(h, "lazy", first_tile=1)
    assert not p["moves"].any() and p["sees"][0, 0, 0].tolist() == [False, True]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rule", ["lazy", "fwd3", "fwd1"])
def test_chain_follows_plan(dtype, rule):
    """lazy_chain keeps its reference by the rule move_plan emulates: with alpha dropped, exactly the rows the plan moves
    come out wrong."""
    case = next(c for c in st.CASES if c.profile == "spikes" and c.rule == rule and c.group == "dense" and not c.causal)
    prob, = st.build(case, dtype)
    ref, _ = st.reference(prob)
    good, _ = st.chain(case, dtype, prob)
    bad, _ = st.chain(case, dtype, prob, "alpha_dropped")
    moved = st.plan(case, dtype, prob)["moves"].any(-1)
    e_good, e_bad = ac.row_errors(good, ref) / ac.U[dtype], ac.row_errors(bad, ref) / ac.U[dtype]
    assert e_good.max() < 1.5
    assert torch.equal(bad.permute(0, 2, 1, 3)[~moved], good.permute(0, 2, 1, 3)[~moved])
    # (a dragged row's alpha can be within rounding of 1: count the rows that carried real weight across the move)
    heavy = moved & (st.plan(case, dtype, prob)["share"] >= 0.01)
    assert heavy.any() and (e_bad[heavy] > 10.0).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_reference_matches_attn_check(dtype):
    """_attn_steep.reference (softmax of the base-2 scores the plan sees) is _attn_check.reference on the dense cases,
    masks, offsets and pre-scaled K included."""
    for case in st.CASES:
        if case.group != "dense" or case.profile != "spikes":
            continue
        prob, = st.build(case, dtype)
        o, lse = st.reference(prob)
        ro, rlse = ac.reference(prob.q, prob.k, prob.v, causal=case.causal, softmax_scale=prob.ref_scale,
                                keep_mask=prob.extra["keep"], additive_mask=prob.extra["add"], q_offset=prob.extra["off"])
        assert torch.allclose(o, ro, rtol=0, atol=1e-9), case.id
        assert torch.allclose(lse, rlse, rtol=1e-12, atol=1e-9), case.id


# ---------------------------------------------------------------------------------------------------------------------
# every GPU case: the inputs
# ---------------------------------------------------------------------------------------------------------------------
def _share_bar(case, dtype):
    if case.window[0] >= 0 and case.rule == "lazy" and dtype == torch.bfloat16:
        bulk = case.window[0] * 1.3
        return bulk / (2.0 ** st.spike_h(case, dtype) + bulk) / 4.0
    return 0.1


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES)
def test_inputs_meet_conditions(dtype, case):
    r = st.conditions(case, dtype, _share_bar(case, dtype))
    assert r["live"] > 0
    if case.profile == "spikes":
        assert r["moved"] >= 0.25, r
        assert r["mixed"] >= 0.5, r
        assert r["carried"] >= 0.25, r
        if case.group == "carry":
            assert r["shard_tile0"] >= 0.125, r
    elif case.profile == "rising":
        assert r["three"] > 0 and r["twice"] == 1.0, r
        if case.group == "carry":
            assert r["shard_tile0"] == 1.0, r
    else:
        assert r["late"] == 0, r
        assert r["faint"] >= 0.5, r


def test_fp8_inputs_stay_in_range():
    """The fp8 cases' key column and spikes stay inside e4m3's range at k_scale 0.05 (no clamp at 448)."""
    for case in st.CASES:
        if case.group == "kv8":
            for dtype in DTYPES:
                for prob in st.build(case, dtype):
                    for x, sc in zip((prob.k, prob.v), st.KV8_SCALES):
                        assert (x.float().abs() / sc).max() < 448


# ---------------------------------------------------------------------------------------------------------------------
# every GPU case: the chain, clean and with each defect
# ---------------------------------------------------------------------------------------------------------------------
def _judged(case, dtype, defect):
    """(passes, statistics) of the chain over every problem of the case, judged as the GPU test judges the kernel."""
    ok, worst = True, {"worst": 0.0, "mean": 0.0, "group": 0.0, "lse": 0.0}
    for prob in st.build(case, dtype):
        ref, rlse = st.reference(prob)
        o, lse = st.chain(case, dtype, prob, defect)
        try:
            stt = st.judge(o.to(dtype), lse, ref, rlse, dtype, case.route, case.id)
        except AssertionError:
            ok = False
            continue
        for k in worst:
            worst[k] = max(worst[k], stt[k])
    return ok, worst


def _overflow_excess(case, dtype):
    """max over rows of (row maximum - the reference its first visible tile sets, or the carried one) minus log2 of the
    dtype's largest finite value: > 0 means an ignored trigger drives P to inf."""
    big = math.log2(torch.finfo(dtype).max)
    worst = -float("inf")
    for prob in st.build(case, dtype):
        full = st.plan(case, dtype, prob)["scores"]
        for lo, hi in st.shards(case, prob):
            s = full[..., lo:hi]
            if lo > 0:  # a carried row's first reference is its lse, without a margin
                first = torch.logsumexp(full[..., :lo] * st.LN2, dim=-1) * st.LOG2E
            else:
                first = torch.full(s.shape[:-1], float("-inf"), dtype=torch.float64)
                for t in range((s.shape[-1] + st.TILE - 1) // st.TILE - 1, -1, -1):
                    mx = s[..., t * st.TILE:(t + 1) * st.TILE].amax(-1)
                    first = torch.where(torch.isinf(mx), first, mx)
                if case.rule == "lazy":
                    first = first + st.MARGIN[dtype]
            worst = max(worst, float((s.amax(-1) - first).nan_to_num(-1e9).max()) - big)
    return worst


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES)
def test_chain_clean_passes_defects_fail(dtype, case):
    ok, stt = _judged(case, dtype, None)
    assert ok, f"the clean chain misses the bars: {stt}"
    moves = any(bool(st.plan(case, dtype, prob)["moves"].any()) for prob in st.build(case, dtype))
    assert moves == (case.profile != "falling")
    for defect in st.DEFECTS[:3]:
        ok, stt = _judged(case, dtype, defect)
        assert ok == (not moves), f"{defect}: {'passes' if ok else 'fails'} ({stt})"
    excess = _overflow_excess(case, dtype)
    if abs(excess) > 2.0:
        ok, stt = _judged(case, dtype, "trigger_ignored")
        assert ok == (excess < 0), f"trigger_ignored: {'passes' if ok else 'fails'} at excess {excess:.1f} ({stt})"

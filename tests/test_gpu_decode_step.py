"""One decode step end to end on the HIP kernels, the way a serving loop runs it: the stages of tests/_step_check.build_step chained
into one step, run eagerly and as ONE captured graph replayed over a 24-step schedule while the device-side state moves underneath
it (context lengths, cache contents, fp8 scales, sampler rows, uniforms, routing).  Every stage of every step is judged by
_step_check.judge_step against fp64 from the device's own inputs to that stage, under the bars of the checker that owns the
operation; the captured runs must also reproduce the eager run bit for bit.

What this owns that the per-operation tests do not: host values frozen at capture (positions, lengths, split counts, scales, routing
sizes), memory recycled between the launches of one graph, the hand-overs between stages (strided q / k / v views of one fused QKV
result with q_out aliasing q, router logits and LM-head rows taken by their row stride, the residual threaded through out-projection
and MoE down), and the seams that only appear as contexts grow (tests/test_step_check.py asserts that the schedules reach them: a
page boundary, a decode split boundary, a window leaving its first page, a full block-table row, a rotation position at
max_position)."""
import time

import pytest
import torch

import _step_check as sk

pytestmark = pytest.mark.gpu
DEV = "cuda"
FORMS = {f.name: f for f in sk.FORMS}
NAMES = list(FORMS)
MOE = [f.name for f in sk.FORMS if f.mlp == "moe"]

_RUNS: dict = {}   # (form, mode) -> records, computed once and left unchanged


def _sync():
    torch.cuda.synchronize()


def _loop(spec, st, run, steps):
    """[(before, stages, after)] of the schedule: between(), snapshot, run() -> dict of device tensors, snapshot."""
    recs = []
    for s in steps:
        sk.between(spec, st, s)
        before = st.snapshot()
        stages = sk.snap(run())
        recs.append((before, stages, st.snapshot()))
    return recs


def _eager(spec, steps=None):
    st = sk.StepState(spec, DEV)
    step = sk.build_step(spec, st)
    return _loop(spec, st, step, range(spec.steps) if steps is None else steps), st, step


def _capture(spec, st, keep=None):
    """Warm up on a side stream, capture one step on it, put the moving state back: (graph, the static stage tensors)."""
    step = sk.build_step(spec, st, keep)
    moving = (st.ctx, st.k_cache, st.v_cache)
    saved = [t.clone() for t in moving]
    sk.between(spec, st, 0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    _sync()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = step()
    for t, s0 in zip(moving, saved):
        t.copy_(s0)
    _sync()
    return g, static


def _replayed(spec, st, keep=None, steps=None):
    g, static = _capture(spec, st, keep)

    def run():
        g.replay()
        return static

    return _loop(spec, st, run, range(spec.steps) if steps is None else steps)


def _poison_allocator():
    """Leave NaN (and 0xFF bytes: NaN in every 16-bit and fp8 format too) in the caching allocator's free blocks, small pool and
    large, without empty_cache: whatever an eager launch or the warm-up gets from it next starts hostile."""
    junk = [torch.full((128 * 1024,), float("nan"), dtype=torch.float32, device=DEV) for _ in range(64)]        # 64 x 512 KiB
    junk += [torch.full((8 << 20,), float("nan"), dtype=torch.float32, device=DEV) for _ in range(4)]           # 4 x 32 MiB
    junk.append(torch.full((256 << 20,), 0xFF, dtype=torch.uint8, device=DEV))                                   # 256 MiB
    _sync()
    del junk


def _run(name, mode):
    key = (name, mode)
    if key not in _RUNS:
        spec = FORMS[name]
        t0 = time.perf_counter()
        if mode == "eager":
            recs, st, _ = _eager(spec)
        elif mode == "graph":
            recs = _replayed(spec, sk.StepState(spec, DEV))
        elif mode == "dropped":
            recs = _replayed(spec, sk.StepState(spec, DEV), keep=("logits", "tokens"))
        else:
            assert mode == "hostile"
            _poison_allocator()
            recs = _replayed(spec, sk.StepState(spec, DEV, hostile=True))
        _sync()
        print(f"\n[decode step] {name} {mode}: {spec.steps} steps in {time.perf_counter() - t0:.2f} s (snapshots included)")
        _RUNS[key] = recs
    return _RUNS[key]


def _judge_all(spec, recs):
    route, pool = sk.decode_route(spec), {}
    t0 = time.perf_counter()
    for s, (before, stages, after) in enumerate(recs):
        try:
            sk.judge_step(spec, before, stages, after, route, pool)
        except sk.StageFailure as e:
            raise AssertionError(f"{spec.name} step {s}: {e}") from None
    sk.judge_pool(spec, pool)
    print(f"[decode step] {spec.name}: judged {len(recs)} steps in {time.perf_counter() - t0:.2f} s on the CPU")


def _same_run(spec, got, want, names=None, caches="all"):
    """Every step's stage tensors (names: only these), context lengths and caches equal bit for bit.  caches="owned": only the
    pages the block tables name, at the step's layer (a hostile start differs elsewhere by construction)."""
    pages = sk.consts(spec).bt.long().flatten()
    for s, ((_, a, sa), (_, b, sb)) in enumerate(zip(got, want)):
        diff = sk.same_bits(a, b, names or sorted(b))
        assert not diff, f"{spec.name} step {s}: {diff} differ from the reference run"
        assert torch.equal(sa.ctx, sb.ctx), f"{spec.name} step {s}: context lengths differ"
        for n in ("k_cache", "v_cache"):
            x, y = getattr(sa, n), getattr(sb, n)
            if caches == "owned":
                x, y = x[pages, spec.layer_idx], y[pages, spec.layer_idx]
            assert torch.equal(sk.bits(x), sk.bits(y)), f"{spec.name} step {s}: {n} differs"


@pytest.mark.parametrize("name", NAMES)
def test_eager_steps_pass_stage_by_stage(name):
    spec = FORMS[name]
    _judge_all(spec, _run(name, "eager"))


@pytest.mark.parametrize("name", MOE)
def test_staged_moe_is_the_module(name):
    """The step calls the router, moe_route, moe_up and moe_down itself to expose their outputs; MoEMLP.forward on the same rows
    gives the same bits, so what is judged is what the module runs."""
    spec = FORMS[name]
    _, st, step = _eager(spec, steps=[0])
    sk.between(spec, st, 1)
    out = step()
    y = st.moe(out["norm2"], residual=out["attn_out"])
    _sync()
    assert torch.equal(sk.bits(y), sk.bits(out["mlp_out"]))


@pytest.mark.parametrize("name", NAMES)
def test_captured_step_replays_under_moving_state(name):
    """One capture, 24 replays; between replays only in-place changes (hidden-state row index, uniforms, the fp8 scales once, two
    sampler rows).  Every replay passes judge_step and equals the eager run from the same start, bit for bit: the headers promise
    identical bits on reruns and graph-capturability, so this is a condition, not a measurement."""
    spec = FORMS[name]
    recs = _run(name, "graph")
    _judge_all(spec, recs)
    _same_run(spec, recs, _run(name, "eager"))


@pytest.mark.parametrize("name", NAMES)
def test_captured_step_with_references_dropped(name):
    """The same capture holding only the final logits and the tokens, so the graph's pool hands one launch's freed intermediates
    and workspaces to the next: tokens, logits, context lengths and caches equal the full capture's at every step."""
    spec = FORMS[name]
    _same_run(spec, _run(name, "dropped"), _run(name, "graph"), names=("logits", "tokens"))


@pytest.mark.parametrize("name", NAMES)
def test_captured_step_from_a_hostile_start(name):
    """NaN left in the caching allocator's free blocks, every cache page no table row names and every other layer NaN: all stage
    tensors, and the caches where a sequence owns them, equal the plain capture's."""
    spec = FORMS[name]
    _same_run(spec, _run(name, "hostile"), _run(name, "graph"), caches="owned")


@pytest.mark.parametrize("name", MOE)
def test_one_graph_serves_both_ends_of_a_routing_swing(name):
    """One step's hidden states send every token to the same top_k experts, the next spreads them over all E: the same captured
    graph is right for both (the plan is a function of the sizes only), judged stage by stage and equal to eager."""
    spec = FORMS[name]
    recs = _replayed(spec, sk.StepState(spec, DEV), steps=sk.SWING)
    route, pool = sk.decode_route(spec), {}
    for before, stages, after in recs:
        sk.judge_step(spec, before, stages, after, route, pool)
    sk.judge_pool(spec, pool)
    one, spread = (r[1]["route_offsets"].long().diff() for r in recs)
    assert int((one > 0).sum()) == spec.top_k and int(one.max()) == spec.T, one.tolist()
    assert int((spread > 0).sum()) == spec.E, spread.tolist()
    _same_run(spec, recs, _eager(spec, steps=sk.SWING)[0])

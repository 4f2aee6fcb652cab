"""The decode-step harness of tests/_step_check.py proved on the CPU: the clean torch model of the step passes judge_step for every
form and every step of the schedule; each planted defect fails, at the stage that owns it; and the forms together reach every
cache-write entry point, decode route, GEMM kind, MLP kind, sampler row kind and seam the GPU test is there for (the routes and
split geometry from the host-only queries, so the table is checked without a GPU)."""
import pytest
import torch

import _step_check as sk

FORMS = {f.name: f for f in sk.FORMS}
GQA, ROWS, HEAD = (f.name for f in sk.FORMS)

# defect -> (the form it is planted in, the stage that must report it, the first step at which it can show)
PLANTED = {
    "rope_positions_frozen": (GQA, "cache_write", 1),
    "ctx_frozen": (GQA, "ctx", 0),
    "page_row_early": (HEAD, "cache_write", 2),          # sequence 0 (6 keys, 4 a step) opens page 1 in its third step
    "k_without_norm": (GQA, "cache_write", 0),
    "v_scale_for_k": (ROWS, "cache_write", 0),
    "scale_frozen": (ROWS, "cache_write", sk.SCALE_STEP),
    "window_off_by_one": (ROWS, "attention", 0),
    "out_proj_residual_dropped": (GQA, "attn_out", 0),
    "router_not_renormalised": (ROWS, "moe_route", 0),
    "sampler_previous_logits": (GQA, "sample", 1),
    "sampler_row_frozen": (GQA, "sample", sk.ROW_STEPS[0]),
}


@pytest.fixture(scope="module")
def clean():
    """The clean model's records per form, run once and left unchanged."""
    return {}


def _clean(clean, name):
    if name not in clean:
        clean[name] = sk.run_model(FORMS[name])
    return clean[name]


@pytest.mark.parametrize("name", list(FORMS))
def test_clean_model_passes_every_step(name, clean):
    recs = _clean(clean, name)
    spec = FORMS[name]
    assert len(recs) == spec.steps
    assert torch.equal(recs[-1][2].ctx, torch.tensor(spec.start_ctx, dtype=torch.int32) + spec.steps * spec.q_len)


def test_every_defect_is_planted():
    """Eleven of the twelve defects the harness was asked to catch.  The twelfth, "slots combined in expert order, not slot
    order", is a difference of fp32 rounding only: _moe_check's bound on the slot sum charges gamma'_k for k roundings on a sum of
    k terms IN ANY ORDER, so the derived bar cannot see it, and nothing is loosened or tightened to make it: it is not planted."""
    assert set(PLANTED) == set(sk.DEFECTS) and len(PLANTED) == 11


@pytest.mark.parametrize("defect", sk.DEFECTS)
def test_planted_defect_is_caught_at_its_stage(defect):
    name, stage, first = PLANTED[defect]
    with pytest.raises(sk.StageFailure) as e:
        sk.run_model(FORMS[name], defect)
    assert e.value.stage == stage, str(e.value)
    assert e.value.step >= first, (e.value.step, str(e.value))


def test_routing_swing_concentrates_then_spreads(clean):
    """The two swing steps of the MoE forms: every token on one set of top_k experts, then all experts in use."""
    for name in (ROWS, HEAD):
        spec, recs = FORMS[name], _clean(clean, name)
        one, spread = (recs[s][1]["route_offsets"].long().diff() for s in sk.SWING)
        assert int((one > 0).sum()) == spec.top_k and int(one.max()) == spec.T, one.tolist()
        assert int((spread > 0).sum()) == spec.E, spread.tolist()


def test_scale_change_and_row_updates_move_the_state(clean):
    recs = _clean(clean, ROWS)
    l = FORMS[ROWS].layer_idx
    assert torch.equal(recs[sk.SCALE_STEP][0].k_scale[l], recs[sk.SCALE_STEP - 1][0].k_scale[l] * 1.5)   # (an fp32 product)
    assert torch.equal(recs[sk.SCALE_STEP][0].v_scale[l], recs[sk.SCALE_STEP - 1][0].v_scale[l] * 1.25)
    assert float(recs[sk.ROW_STEPS[0] - 1][0].temperature[0]) > 0 and float(recs[sk.ROW_STEPS[0]][0].temperature[0]) == 0
    assert float(recs[sk.ROW_STEPS[1] - 1][0].temperature[1]) == 0 and int(recs[sk.ROW_STEPS[1]][0].top_k[1]) == 5


def test_forms_reach_what_the_step_test_is_for():
    per_form = {f.name: sk.reach(f) for f in sk.FORMS}
    got = set().union(*per_form.values())
    assert sk.NEEDED <= got, sorted(sk.NEEDED - got)
    # the seams sit where the schedule was built to put them
    assert {"decode:gqa", "seam:split", "seam:max_position", "seam:page", "V%8"} <= per_form[GQA]
    assert {"decode:rows", "seam:window_page", "seam:table_full", "cache:fp8"} <= per_form[ROWS]
    assert {"decode:head", "seam:table_full", "seam:page", "sampler:reread"} <= per_form[HEAD]
    assert len([f for f in sk.FORMS if f.V > 65536]) == 1
    for f in sk.FORMS:
        assert f.d == 256 and f.I == 512 and f.block_size == 16


def test_skipped_rows_and_dead_positions_follow_the_header(clean):
    """The two outcomes the schedule computes from the header's rules: once a sequence has filled its block-table row the cache
    keeps its bytes while the context goes on growing, and a token at rotation position >= max_position writes nothing and hands
    attention a zero query."""
    spec, recs = FORMS[ROWS], _clean(clean, ROWS)
    b = spec.start_ctx.index(85)
    full = [s for s in range(spec.steps) if int(recs[s][2].ctx[b]) > spec.cap]
    assert full and all(int(recs[s][2].ctx[b]) == 85 + s + 1 for s in full)
    pages = sk.consts(spec).bt[b].long()
    for s in full:
        assert torch.equal(sk.bits(recs[s][0].k_cache[pages]), sk.bits(recs[s][2].k_cache[pages]))
    spec, recs = FORMS[GQA], _clean(clean, GQA)
    b = spec.start_ctx.index(290)
    dead = [s for s in range(spec.steps) if int(recs[s][2].ctx[b]) - 1 >= spec.max_position]
    assert dead
    for s in dead:
        q = recs[s][1]["qkv"][b, :spec.H * spec.D]
        assert not bool((q.float() != 0).any())
        assert torch.isfinite(recs[s][1]["attn"][b].float()).all()

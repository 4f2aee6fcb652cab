"""CPU tests of the module-layer checker (tests/_module_check.py): the rounding model passes its own bars and agrees with the fp64
reference to within what its chain of roundings allows; the case table's shapes stand where the table says (ops.*_ok,
mio._nn.attention_plan) and fall one 256-row tile below; the branch is not drowned by the residual; every planted defect fails
judge(); and what the old whole-tensor bar says to each defect is printed (pytest -s shows it).

Shapes: 3 sequences of 257 rows = 771 rows (three 256-row tiles and a ragged tail of 3 rows; sequence boundaries off the tiles).
The MLP cases run d = 128, I = 256; the attention cases d = 256 with 4 heads of 64, because two of the defects need it: a K
column range of 256 (the scale that stops 128 columns early must leave a scaled part) and a neighbouring head on each side."""
import math

import pytest
import torch

import _module_check as mc

BF, FP = mc.BF, mc.FP
B, S = 3, 257
ATTN_D, ATTN_H, MLP_D, MLP_I = 256, 4, 128, 256

# name -> (spec, d, norm kind, folded form, keep mask, roundings on the route)
HOST = {
    "self_plain": (mc.attn_spec(H=ATTN_H, kpre=True), ATTN_D, None, False, False, 4),          # projection, P, context, output
    "self_prenorm_ln": (mc.attn_spec(H=ATTN_H, kpre=True), ATTN_D, "layernorm", False, False, 5),
    "self_prenorm_rms": (mc.attn_spec(H=ATTN_H, causal=False), ATTN_D, "rms", False, False, 5),
    "self_fold_ln": (mc.attn_spec(H=ATTN_H, kpre=True), ATTN_D, "layernorm", True, False, 6),   # weight, bias', then the four
    "self_fold_rms_kv2": (mc.attn_spec(H=ATTN_H, Hkv=2), ATTN_D, "rms", True, False, 5),
    "self_keep_mask": (mc.attn_spec(H=ATTN_H, causal=False), ATTN_D, None, False, True, 4),
    "self_window": (mc.attn_spec(H=ATTN_H, window=(64, 0)), ATTN_D, None, False, False, 4),
    "self_rotary": (mc.attn_spec(H=ATTN_H, rotary=64), ATTN_D, None, False, False, 5),
    "self_normalize_query": (mc.attn_spec(H=ATTN_H, causal=False, normq=True), ATTN_D, None, False, False, 5),
    "layer": (mc.attn_spec("layer", H=ATTN_H, kpre=True), ATTN_D, None, False, False, 4),
    "mlp_gelu": (mc.mlp_spec("gelu", MLP_I), MLP_D, None, False, False, 2),                    # intermediate, output
    "mlp_gelu_prenorm": (mc.mlp_spec("gelu", MLP_I), MLP_D, "layernorm", False, False, 3),
    "mlp_gelu_fold_ln": (mc.mlp_spec("gelu", MLP_I), MLP_D, "layernorm", True, False, 4),
    "mlp_swiglu": (mc.mlp_spec("swiglu", MLP_I), MLP_D, None, False, False, 2),
    "mlp_swiglu_fold_rms": (mc.mlp_spec("swiglu", MLP_I), MLP_D, "rms", True, False, 3),
    "mlp_erf_gelu": (mc.mlp_spec("gelu_erf", MLP_I), MLP_D, "layernorm", False, False, 3),
    "mlp_relu": (mc.mlp_spec("relu", MLP_I), MLP_D, None, False, False, 2),
    "mlp_silu": (mc.mlp_spec("silu", MLP_I), MLP_D, None, False, False, 2),
}
# defect -> the host case it is planted into
PLANTED = {
    "neighbour_residual": "mlp_gelu",
    "tail_no_residual": "self_plain",
    "kscale_short": "self_plain",
    "stats_shift": "mlp_gelu_fold_ln",
    "beta_unfolded": "self_fold_ln",
    "gate_up_swap": "mlp_swiglu",
    "head_shift": "self_prenorm_ln",
    "stale_gamma": "mlp_swiglu_fold_rms",
}
_CACHE: dict = {}


def _built(name, dtype):
    """The inputs, the fp64 reference (with its branch) and the clean model of a host case: computed once, left unchanged."""
    key = (name, dtype)
    if key not in _CACHE:
        spec, d, norm, fold, mask, _ = HOST[name]
        g = torch.Generator().manual_seed(mc.seed_of(name, dtype))
        P = mc.draw_params(spec, d, g, dtype)
        n = mc.draw_norm(norm, d, g, dtype) if norm else None
        x = mc.draw_rows(B, S, d, g, dtype)
        kw = dict(norm=n, keep=mc.keep_mask(B, S) if mask else None)
        ref, branch = mc.reference(spec, P, x, parts=True, **kw)
        kw["fold"] = fold
        _CACHE[key] = dict(spec=spec, P=P, x=x, kw=kw, ref=ref, branch=branch, model=mc.model(spec, P, x, dtype=dtype, **kw))
    return _CACHE[key]


@pytest.mark.parametrize("dtype", [BF, FP], ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", sorted(HOST))
def test_model_passes_its_bars_and_agrees_with_the_reference(name, dtype):
    """The model against itself is at its own bars with every margin to spare.  Against the reference: each of the R rounding
    points of the route moves an element by at most u relative (unit roundoff), a row's norm by about u / sqrt(3) on average;
    at a branch of the size of the residual nothing amplifies them, so a row is off by less than R u and the mean by less than
    R u / 2."""
    c = _built(name, dtype)
    mc.judge(c["model"], c["ref"], c["model"], dtype, S, "host", what=name, record=False)
    st = mc.measure(c["model"], c["ref"], dtype, S)
    R = HOST[name][5]
    assert 0.2 < st["mean"] < 0.5 * R and st["worst"] < R, f"{name}: model vs reference {st} with {R} roundings"
    assert st["tile"] < 1.5 * st["mean"] and st["seq"] < 1.5 * st["mean"]


def test_folded_and_unfolded_reference_are_one_function():
    """The folded read-out, evaluated without any rounding, is the unfolded sub-layer: the fold's algebra is right."""
    for name in ("self_fold_ln", "self_fold_rms_kv2", "mlp_gelu_fold_ln", "mlp_swiglu_fold_rms"):
        c = _built(name, BF)
        folded = mc._sublayer(mc._Arith(None, None), c["spec"], c["P"], c["x"], c["kw"]["norm"], True)[0]
        assert mc.row_errors(folded, c["ref"]).max().item() < 1e-12, name


@pytest.mark.parametrize("name", sorted(HOST))
def test_branch_is_not_drowned_by_the_residual(name):
    c = _built(name, BF)
    r = mc.branch_ratio(c["branch"], c["x"])
    assert 0.5 <= r <= 2.0, f"{name}: median ||branch|| / ||residual|| = {r:.2f}"


@pytest.mark.parametrize("dtype", [BF, FP], ids=["bf16", "fp16"])
@pytest.mark.parametrize("defect", sorted(mc.DEFECTS))
def test_planted_defect_fails_judge(defect, dtype):
    """Each defect, planted into the model, is refused by judge() against the clean model's bars.  The old verdict is printed: the
    whole-tensor statistic of tests/test_gpu_modules.py against the project's own clean 16-bit result, bar 3e-3."""
    c = _built(PLANTED[defect], dtype)
    bad = mc.model(c["spec"], c["P"], c["x"], dtype=dtype, defect=defect, **c["kw"])
    assert not torch.equal(bad, c["model"]), f"{defect}: the planted defect changed nothing"
    rel, accepted = mc.old_aggregate(bad, c["model"])
    st = mc.measure(bad, c["ref"], dtype, S)
    bar, _ = mc.bars(c["model"], c["ref"], dtype, S)
    print(f"\n{defect} ({mc.DEFECTS[defect]}) in {PLANTED[defect]} {str(dtype).split('.')[-1]}: old statistic {rel:.2e} -> "
          f"{'ACCEPTED' if accepted else 'refused'} by the old bar {mc.OLD_BAR:g}; rows: "
          + ", ".join(f"{k} {st[k]:.2f} u (bar {bar[k]:.2f})" for k in mc.MARGINS))
    with pytest.raises(AssertionError):
        mc.judge(bad, c["ref"], c["model"], dtype, S, "host", what=defect, record=False)


def test_what_the_old_bar_accepts_at_these_shapes():
    """At these shapes (771 rows, 3 sequences, 4 heads) the old whole-tensor bar accepts the single-row and the ragged-tile
    defect, in both dtypes.  It refuses the single-head defect only because two heads of one sequence are a sixth of this tensor
    (old statistic 0.22); at the GPU shape (63 sequences, 16 heads) they are 1 / 504 of it and the same fault moves the
    statistic by 0.22 * 6 / 504 = 2.7e-3, below the bar; the single row and the ragged tile weigh 21 times less there."""
    accepted = {}
    for defect, name in PLANTED.items():
        c = _built(name, BF)
        accepted[defect] = mc.old_aggregate(mc.model(c["spec"], c["P"], c["x"], dtype=BF, defect=defect, **c["kw"]), c["model"])[1]
    print("\naccepted by the old bar at the host shapes:", sorted(k for k, v in accepted.items() if v))
    assert {k for k, v in accepted.items() if v} == {"neighbour_residual", "tail_no_residual"}


def test_judge_stats_bound():
    """The statistics bound takes fp32 sums of the rows in any order and refuses a slot that read its neighbour row."""
    g = torch.Generator().manual_seed(5)
    rows = mc.draw_rows(2, 150, 512, g, BF)
    x = rows.reshape(-1, 2, 256).float()
    st = torch.stack([x.sum(-1).t(), x.square().sum(-1).t()], dim=-1)
    mc.judge_stats(st, rows, "fp32 sums")
    st4 = torch.stack([x.view(-1, 2, 4, 64).sum(-1).sum(-1).t(), x.square().view(-1, 2, 64, 4).sum(-1).sum(-1).t()], dim=-1)
    mc.judge_stats(st4, rows, "fp32 sums in another order")
    bad = st.clone()
    bad[1, 7] = st[1, 8]
    with pytest.raises(AssertionError):
        mc.judge_stats(bad, rows, "neighbour row")
    with pytest.raises(AssertionError):
        mc.judge_stats(st[:, :-1], rows, "short")


def test_rn16_is_the_direct_rounding():
    g = torch.Generator().manual_seed(6)
    v = torch.randn(4096, generator=g, dtype=torch.float64) * torch.logspace(-6, 4, 4096, dtype=torch.float64)
    for dt in (BF, FP):
        assert torch.equal(mc.rn16(v.float().double(), dt), v.float().to(dt).double())      # single rounding from fp32 values
        assert torch.equal(mc.rn16(mc.rn16(v, dt), dt), mc.rn16(v, dt))
    tie = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -40], dtype=torch.float64)                   # just above a bf16 tie
    assert mc.rn16(tie, BF).item() == 1.0 + 2.0 ** -7


# ---- the case table's claims (host-only queries of the built library) ----------------------------------------------------------
def _ops():
    from mio import ops
    return ops


def _plan(c, Bc, Sc, M):
    from mio._nn import attention_plan
    d, H = mc.SHAPES[c["shape"]][:2]
    sp = c["spec"]
    D = d // H
    kvd = sp["Hkv"] * D
    flags = dict(mask=bool(c.get("mask")), normalize_query=bool(sp.get("normq")), windowed=sp.get("window") is not None,
                 rotary=bool(sp.get("rotary")))
    if sp["kind"] == "self":
        n_tot = d + 2 * kvd
        return attention_plan(Bc, Sc, Sc, H, sp["Hkv"], D, (M, n_tot, d), (d, d + kvd), n_tot, (M, d, d), **flags)
    return attention_plan(Bc, Sc, Sc, H, sp["Hkv"], D, (M, kvd, d), (0, kvd), kvd, None, **flags)


def _attn_routes(c):
    return [r for r in c["routes"] if r.startswith("attn:")]


@pytest.mark.parametrize("name", [c["name"] for c in mc.CASES])
def test_case_stands_at_its_shape_and_falls_a_tile_below(name):
    ops = _ops()
    c = mc.case(name)
    d, H, Bc, Sc = mc.SHAPES[c["shape"]]
    M = Bc * Sc
    big = c["shape"] != "small"
    assert M % 256 != 0 or c["shape"] == "short", "rows must not be a multiple of the tile"
    assert c["shape"] == "short" or Sc % 256 not in (0, 255) and (Sc * 2) % 256 != 0   # sequence boundaries off the tiles
    specs = [c["spec"]] + ([c["mlp"]] if "mlp" in c else [])
    for sp in specs:
        if sp["op"] == "mlp":
            I, act = sp["I"], sp["act"]
            assert ops.fused_mlp_blocked_weight_ok(M, d, I, act) == big
            if big:
                assert not ops.fused_mlp_blocked_weight_ok(M - 256, d, I, act), "one tile below still takes the blocked kernels"
                assert not ops.fused_mlp_blocked_weight_ok(M, d, I - 256, act), "a smaller I still fills the chip"
            if c.get("stream") or c.get("fold"):
                assert ops.gemm_ln_ok(M, I, d, act, fold_in=True) and ops.gemm_ln_ok(M, d, I, "none", stats_out=True)
                assert not ops.gemm_ln_ok(M - 256, d, I, "none", stats_out=True)
            continue
        kvd = sp["Hkv"] * (d // H)
        n_tot = d + 2 * kvd
        assert ops.blocked_weight_ok(M, d, d) == big                       # the out-projection, the narrowest GEMM of the sub-layer
        if big:
            assert not ops.blocked_weight_ok(M - 256, d, d), "one tile below still takes the persistent kernel"
        plan = _plan(c, Bc, Sc, M)
        want = _attn_routes(c)[0]
        assert plan.kpre == bool(sp["kpre"]) == ("kpre" in want), f"{name}: plan {plan}"
        assert plan.out_blocked == want.endswith("+oblk"), f"{name}: plan {plan}"
        if plan.kpre:
            assert plan.col_scale[2] == (1.0 / math.sqrt(d // H)) * mc.LOG2E
            # one tile below the out-projection has left the persistent kernel: no blocked context (the wider fused projection
            # still fills the chip, so K may stay pre-scaled)
            assert not _plan(c, Bc, Sc, M - 256).out_blocked, "one tile below the context is still written blocked"
        if sp["kind"] == "self" and (c.get("stream") or c.get("fold")):
            assert ops.gemm_ln_ok(M, n_tot, d, "none", fold_in=True) and ops.gemm_ln_ok(M, d, d, "none", stats_out=True)
            assert not ops.gemm_ln_ok(M - 256, d, d, "none", stats_out=True)
    if name == "self_short_plain":   # everything says yes but the attention kernel at Sq <= 128
        assert ops.col_scale_ok(M, 3 * d, d) and not ops.fa3_k_prescaled_ok(Bc, Sc, Sc, H, d // H, 3 * d, 3 * d)
        assert ops.fa3_k_prescaled_ok(Bc, Sc + 1, Sc + 1, H, d // H, 3 * d, 3 * d)
    if name == "self_hd64_kv1":      # everything says yes but the K column range [1024, 1088)
        n = d + 2 * (d // H)
        assert ops.col_scale_ok(M, n, d) and ops.fa3_k_prescaled_ok(Bc, Sc, Sc, H, d // H, n, n)
    if name == "self_hd80_plain":
        assert ops.fa3_k_prescaled_ok(Bc, Sc, Sc, H, 80, 3 * d, 3 * d) and not ops.fa3_o_blocked_ok(Bc, Sc, Sc, H, 80, 3 * d, 3 * d)
    if name == "self_hd128_stream_out_in":
        assert ops.col_scale_ok(M, 3 * d, d) and not ops.fa3_k_prescaled_ok(Bc, Sc, Sc, H, 128, 3 * d, 3 * d)


def test_the_table_covers_what_it_promises():
    names = {c["name"] for c in mc.CASES}
    assert len(names) == len(mc.CASES)
    routes = {r for c in mc.CASES for r in c["routes"]}
    for r in ("gemm:p8w+cs", "gemm:p8w", "gemm:p8w_res", "gemm:p8w_stats", "gemm:p8w_fold", "gemm:p8w_fold+cs", "gemm:p8w_glu_fold",
              "gemm:t128", "attn:plain", "attn:kpre", "attn:kpre+oblk", "mlp:blocked/p8w/p8w_res", "mlp:blocked/p8w_glu/p8w_res",
              "mlp:two_launch/t128/t128", "mlp:two_launch/glu_t128x64/t128"):
        assert r in routes, r
    assert {c["shape"] for c in mc.CASES} == set(mc.SHAPES)
    assert {c["module"] for c in mc.CASES} == {"self", "layer", "mlp", "block", "chain", "cross_block"}
    acts = {sp["act"] for c in mc.CASES for sp in (c["spec"], c.get("mlp", {})) if sp.get("op") == "mlp"}
    assert acts == {"gelu", "gelu_erf", "relu", "silu", "swiglu"}
    assert set(PLANTED) == set(mc.DEFECTS)

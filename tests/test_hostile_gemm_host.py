"""tests/_hostile_gemm.py on the CPU: the (route, class) coverage table against mio_gemm_route_t of include/mio_hip.h, every
case of tests/test_gpu_gemm_hostile.py holding at least 8 bytes of every class it claims and taking the route it names (the
route query needs no device), the clean torch model of every launch form passing judge(), and every planted
out-of-ownership access failing it with its fill, its tensor and its class of memory named."""
import os
import re

import pytest
import torch

import _hostile_gemm as hg

BF = torch.bfloat16
CASES = {c.name: c for c in hg.CASES}
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "mio_hip.h")


def _built(name, dtype=BF):
    return hg.build(hg.shrunk(CASES[name]), dtype)


def _header_routes():
    text = open(HEADER).read()
    body = re.search(r"typedef enum \{([^}]*)\} mio_gemm_route_t;", text).group(1)
    return [m.lower() for m in re.findall(r"MIO_GEMM_ROUTE_(\w+)\s*=", body)]


# what each route can meet: a route added to the header fails here until it has cases and a row
WANT = {
    "t128": {"past K", "past N", "guard row"},
    "t256": {"past K", "past N", "guard row"},
    "p8w": {"past K", "past N", "guard row", "padding row", "workspace"},
    "p8w_res": {"past K", "past N", "guard row", "padding row", "workspace"},
    "p8w_fold": {"past K", "past N", "guard row", "padding row", "spare slot", "rms sum entry"},
    "p8w_stats": {"past K", "past N", "guard row", "padding row", "spare slot"},
    "glu_t128x64": {"past K", "past N", "guard row", "workspace"},
    "glu_t256x128": {"past K", "past N", "guard row"},
    "p8w_glu": {"past K", "past N", "guard row", "padding row", "workspace"},
    "p8w_glu_fold": {"past K", "past N", "guard row", "padding row", "spare slot", "rms sum entry"},
}


def test_coverage_table_against_the_header():
    routes = _header_routes()
    assert routes[0] == "empty" and len(routes) == len(set(routes)) >= 11
    cov = hg.coverage()
    assert set(routes) - {"empty"} == set(hg.ROUTES) == set(WANT), "a route of mio_gemm_route_t has no hostile-memory cases"
    for r in hg.ROUTES:
        assert WANT[r] <= cov.get(r, set()), (r, sorted(WANT[r] - cov.get(r, set())))
    for e in hg.ENTRY_POINTS:
        assert cov.get(e), f"{e} has no hostile-memory case"
    from mio import _lib
    assert set(_lib.GEMM_ROUTES.values()) == set(routes)
    print("\n".join(f"{k:28s} {sorted(v)}" for k, v in cov.items()))


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_holds_its_classes_and_takes_its_route(name):
    """Full size: at least 8 bytes of every claimed class, no class unclaimed, the route the case names, pointers aligned."""
    c = CASES[name]
    for dtype in (BF, torch.float16):
        b = hg.build(c, dtype)
        have = hg.nonvacuous(b)
        assert all(have[cl] >= 8 for cl in c.classes)
        if c.kind != "prep":
            assert hg.route(b) == c.route, (name, hg.route(b))
        for bf in b.bufs.values():
            assert bf.off * bf.data.element_size() % 16 == 0, (name, bf.name)
        if c.kind == "mlp":   # (large: one dtype is the same geometry)
            break


def test_fills():
    b = _built("p8w_fold_rms")
    for fill in ("nan", "huge"):
        given = hg.inputs(b, fill)
        for name, bf in b.bufs.items():
            m = bf.cls != hg.OWNED
            got = given[name][m]
            if fill == "nan":
                assert bool((hg.bits(given[name])[m] == -1).all()) and bool(torch.isnan(got.float()).all())
            elif got.dtype == torch.float32:
                assert bool((got == 1e30).all())
            else:
                assert bool((got.float().abs() == torch.finfo(BF).max / 8).all()) and 0 < int((got > 0).sum()) < got.numel()
            own = bf.cls == hg.OWNED
            assert torch.equal(hg.bits(given[name])[own], hg.bits(bf.data)[own])
    w8 = hg.inputs(_built("prep_quant_w8"), "huge")["w8"]
    m = hg.build(hg.shrunk(CASES["prep_quant_w8"]), BF).bufs["w8"].cls != hg.OWNED
    assert set(w8[m].tolist()) == {0x7E, 0xFE} and bool((w8[m].view(torch.float8_e4m3fn).float().abs() == 448).all())


@pytest.mark.parametrize("name", sorted(CASES))
def test_clean_model_passes(name):
    hg.judge(hg.Model(), _built(name))


def test_clean_model_passes_fp16():
    for name in ("t128_k40", "p8w_fold_ln", "p8w_glu_fold_rms", "p8w_stats_blocked", "mlp_glu_bw", "prep_fold_k264"):
        hg.judge(hg.Model(), _built(name, torch.float16))


def _fails(defect, name, fills=("nan", "huge")):
    with pytest.raises(hg.HostileFailure) as e:
        hg.judge(hg.Model(defect), _built(name), fills=fills)
    return e.value


@pytest.mark.parametrize("name,tensor", [("t128_k40", "y"), ("glu_t128x64", "y"), ("p8w_res_ldr", "y"), ("prep_fold_k264", "ws"),
                                         ("prep_quant_w8", "w8")])
def test_a_x_chunk_past_k_against_a_zero_weight_chunk(name, tensor):
    e = _fails("x_chunk_past_k", name)
    assert e.fill == "nan" and e.tensor == tensor and "past K" in e.classes and "differs from the benign launch" in str(e)
    assert "per" in str(e) and "route" in str(e)


@pytest.mark.parametrize("name", ["p8w_blocked_w_k544", "p8w_col_scale_band_to_n", "prep_block", "prep_block_glu"])
def test_b_w_row_clamped_to_n(name):
    """Visible where the clamped row lands in owned output: the padding rows of a prepared weight.  In a plain-weight launch
    it feeds columns that are never stored, which no judgement of outputs can see (and none needs to)."""
    e = _fails("w_row_clamp_n", name)
    assert e.fill == "nan" and e.tensor in ("wb", "w1b", "w2b") and e.classes == ("guard row",)
    hg.judge(hg.Model("w_row_clamp_n"), _built("t128_k40"))


@pytest.mark.parametrize("name", ["t128_k40", "p8w_k128", "glu_t256x128", "mlp_two_launch_gelu"])
def test_c_bias_read_unclamped(name):
    e = _fails("bias_unclamped", name)
    assert e.fill == "nan" and e.tensor == "y" and e.classes == ("past N",)


@pytest.mark.parametrize("name", ["t128_k40", "p8w_res_ldr", "p8w_stats", "mlp_bw"])
def test_d_residual_row_m_added_into_row_m_minus_1(name):
    e = _fails("res_row_m", name)
    assert e.fill == "nan" and e.tensor == "y" and e.classes == ("guard row",) and f"({hg.shrunk(CASES[name]).M - 1}," in str(e)


def test_e_padding_row_of_a_blocked_x_in_the_producers_statistics():
    e = _fails("pad_row_in_stats", "p8w_stats_blocked")
    assert e.fill == "nan" and e.tensor == "stats_out" and e.classes == ("padding row",)


@pytest.mark.parametrize("name", ["p8w_fold_rms", "p8w_fold_rms_blocked_x", "p8w_glu_fold_rms"])
def test_f_rms_form_uses_the_sum_entry(name):
    e = _fails("rms_uses_sum", name)
    assert e.fill == "nan" and e.tensor == "y" and e.classes == ("rms sum entry",)


@pytest.mark.parametrize("name,tensor", [("p8w_fold_ln", "y"), ("p8w_glu_fold_rms", "y"), ("prep_stats_reduce", "stats_red")])
def test_g_statistics_slot_past_ln_slots_summed(name, tensor):
    e = _fails("spare_slot", name)
    assert e.fill == "nan" and e.tensor == tensor and e.classes == ("spare slot",)


@pytest.mark.parametrize("name", ["p8w_res_blocked_res", "p8w_stats_blocked"])
def test_h_store_one_row_past_m_into_a_blocked_y(name):
    e = _fails("store_row_past_m", name)
    assert e.tensor == "y" and e.classes == ("padding row",) and "not-owned output written" in str(e)
    assert f"({hg.shrunk(CASES[name]).M}," in str(e)


@pytest.mark.parametrize("name", ["p8w_fold_ln", "p8w_glu_fold_ln"])
def test_i_value_in_the_variance_clamp_only_needs_the_huge_fill(name):
    hg.judge(hg.Model("clamp_only"), _built(name), fills=("nan",))   # a NaN operand drops out of a maximum: nothing to see
    e = _fails("clamp_only", name)
    assert e.fill == "huge" and e.tensor == "y" and e.classes == ("spare slot",)


@pytest.mark.parametrize("name,tensor", [("t128_k40", "w"), ("mlp_bw", "w1"), ("prep_stats_reduce", "stats_in")])
def test_j_input_modified(name, tensor):
    e = _fails("input_modified", name)
    assert e.tensor == tensor and "input modified" in str(e)


def test_a_wrong_benign_result_fails_the_unchanged_bars():
    """A model that is wrong on finite inputs (no hostile read at all) is caught by _gemm_check.check, not by the fills."""
    class Wrong(hg.Model):
        def __call__(self, built, t):
            super().__call__(built, t)
            bf = built.bufs["y"]
            bf.view(t["y"])[3, 5] += 1.0
            return t

    with pytest.raises(AssertionError) as e:
        hg.judge(Wrong(), _built("t128_k40"))
    assert not isinstance(e.value, hg.HostileFailure)


def test_nonvacuity_is_asserted():
    from dataclasses import replace
    c = hg.shrunk(CASES["t128_k40"])
    with pytest.raises(AssertionError, match="fewer than 8 bytes"):
        hg.judge(hg.Model(), hg.build(replace(c, classes=c.classes + (hg.SPARE_SLOT,)), BF))
    with pytest.raises(AssertionError, match="does not claim"):
        hg.judge(hg.Model(), hg.build(replace(c, classes=(hg.PAST_K,)), BF))


def test_padding_rows_rule():
    """The rule of include/mio_hip.h: the padding rows of a blocked y keep their pre-fill, those of stats_out are written (and
    judged bit for bit), those of mio_ln_stats_reduce's output are written with unspecified values."""
    b = _built("p8w_stats_blocked")
    M, N = b.case.M, b.case.N
    y, so = b.bufs["y"], b.bufs["stats_out"]
    assert int((y.cls == hg.PAD_ROW).sum()) == ((M + 255) // 256 * 256 - M) * N and int((y.cls == hg.OWNED).sum()) == M * N
    assert int((so.cls == hg.OWNED).sum()) == N // 256 * ((M + 255) // 256 * 256) * 2 and not (so.cls == hg.PAD_ROW).any()
    r = _built("prep_stats_reduce").bufs["stats_red"]
    assert r.scratch is not None and bool((r.cls[r.scratch] == hg.PAD_ROW).all()) and int(r.scratch.sum()) > 0


def test_embedded_views():
    """Embedded (the decode-GEMM and row-kernel tests' operands): the view holds the value under every fill, the bytes around it
    the fill; untouched() sees a write outside the view, and inside it where the operand is an input; of a blocked output only
    the rows below M are the launch's; an e4m3fn operand is poisoned as bytes."""
    v = torch.randn(5, 8).to(BF)
    e = hg.Embedded(v, (7, 16), (1, 0))
    for fill in hg.FILLS:
        e.fill(fill)
        assert torch.equal(e.view, v) and e.untouched() and e.view.data_ptr() == e.buf.data_ptr() + 32
        around = e.buf[~e.owned].float()
        assert bool({"benign": torch.isfinite(around) & (around.abs() < 10), "nan": torch.isnan(around),
                     "huge": around.abs() == torch.finfo(BF).max / 8}[fill].all())
    e.buf[0, 0] = 1.0
    assert not e.untouched()
    e.fill("nan").view[2, 2] += 1
    assert not e.untouched()
    o = hg.Embedded(None, (512 * 32 + 128,), (64,), out_shape=(512 * 32,), dtype=torch.float16, device="cpu",
                    own_index=hg.blocked_index(257, 32))
    o.fill("huge").view[hg.blocked_index(257, 32)] = 1.0
    assert o.untouched() and int(o.owned.sum()) == 257 * 32
    o.view[hg.blocked_index(258, 32)[257, 5]] = 2.0
    assert not o.untouched()
    q = hg.Embedded(torch.randn(4, 16).to(torch.float8_e4m3fn), (6, 32), (1, 0)).fill("huge")
    assert q.view.dtype == torch.float8_e4m3fn and set(q.buf[~q.owned].tolist()) == {0x7E, 0xFE}
    s = hg.Embedded(torch.rand(9), (25,), (8,)).fill("huge")
    assert bool((s.buf[~s.owned] == 1e30).all())

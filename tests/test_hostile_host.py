"""tests/_hostile.py on the CPU: the ownership rule against a brute-force visibility matrix, the case table of
tests/test_gpu_attention_hostile.py against the route tables (every case takes the route it names, on its embedded views,
without a copy), the clean torch model of every launch form passing judge(), and every planted out-of-ownership access
failing it with its fill and its class of memory named."""
import pytest
import torch

import _hostile as hs
from mio import _lib

BF = torch.bfloat16
CASES = {c.name: c for c in hs.CASES}


def _built(name, dtype=BF):
    return hs.build(hs.shrunk(CASES[name]), dtype)


def test_every_route_has_cases():
    for form, names in (("dense", _lib.FA3_ROUTES), ("varlen", _lib.FA3_VARLEN_ROUTES), ("paged", _lib.FA3_PAGED_ROUTES)):
        have = {c.route for c in hs.CASES if c.form == form}
        assert have == set(names.values()) - {"empty"}, (form, have)
    for form in ("dense", "varlen", "paged"):   # the windowed forms
        wins = {tuple(c.window) for c in hs.CASES if c.form == form and c.windowed}
        assert wins == {(0, 0), (63, 0), (64, 0), (100, 0), (64, 32), (-1, 100)}, (form, wins)


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_takes_its_route_on_its_views(name):
    """Full size, both dtypes: mio.ops hands the embedded views through (params() asserts every address) and the route
    query, which needs no device, names the case's route."""
    for dtype in (BF, torch.float16):
        b = hs.build(CASES[name], dtype)
        assert hs.route(b, hs.inputs(b, "benign")) == CASES[name].route


@pytest.mark.parametrize("name", sorted(CASES))
def test_ownership_against_brute_force(name):
    """tile not owned <=> no key of it is visible to any query of its sequence (user-mask routes: every tile owned); and
    the class maps agree with it row by row."""
    c = CASES[name]
    b = hs.build(c, BF)
    assert len(b.seqs) == (c.B if c.form == "dense" else len(c.lens_q))
    for i, (Lq, Lk, off) in enumerate(b.seqs):
        tiles = hs.owned_tiles(Lq, Lk, off, c.causal, c.window, c.mask is not None)
        vis = hs.visible(Lq, Lk, off, c.causal, c.window)
        brute = [bool(c.mask) or bool(vis[:, t * 64:(t + 1) * 64].any()) for t in range((Lk + 63) // 64)]
        assert tiles == brute, (name, i)
        key_owned = torch.tensor([tiles[j // 64] for j in range(Lk)], dtype=torch.bool)
        if c.form == "paged":
            bt, bs = b.bufs["table"].data, c.bs
            pos = torch.arange(Lk)
            got = (b.bufs["k_cache"].cls[bt[i, pos // bs].long(), hs.LAYER, pos % bs] == hs.OWNED).all(-1).all(-1)
            if not (c.shared and i < 2):   # a shared page is owned if either sequence owns it
                assert torch.equal(got, key_owned), (name, i)
            assert bool((got | ~key_owned).all())
            need = [bool(key_owned[j * bs:(j + 1) * bs].any()) for j in range(bt.shape[1])]
            assert (b.bufs["table"].cls[i] == hs.OWNED).tolist() == need, (name, i)
        else:
            sp = b.specs["k"]
            cls = sp.view(b.bufs[sp.buf].cls)
            if c.form == "dense":
                rows = cls[i] if c.layout == "bshd" else cls[i].permute(1, 0, 2)
            else:
                rows = cls[b.meta["cu_k"][i]:b.meta["cu_k"][i] + Lk]
            assert torch.equal((rows == hs.OWNED).all(-1).all(-1), key_owned), (name, i)


@pytest.mark.parametrize("name", sorted(CASES))
def test_clean_model_passes(name):
    hs.judge(hs.Model(), _built(name))


def test_clean_model_passes_fp16():
    for name in ("dense_fwd1_add_D40_rows", "varlen_D96_fused_c1", "paged_bs128_D64_c1", "window_paged_l64_r32_D64"):
        hs.judge(hs.Model(), _built(name, torch.float16))


def _fails(defect, name, fills=("nan", "huge")):
    with pytest.raises(hs.HostileFailure) as e:
        hs.judge(hs.Model(defect), _built(name), fills=fills)
    return e.value


DENSE, VARLEN, PAGED = "dense_fwd5_D64", "varlen_D64_split_c0", "paged_bs128_D64_c0"


@pytest.mark.parametrize("name,cls", [(DENSE, "guard row"), ("dense_fwd3_D96_bhsd", "guard row"),
                                      (VARLEN, "neighbour sequence"), (PAGED, "stale slot")])
def test_a_key_past_lk_at_weight_zero(name, cls):
    e = _fails("key_past_lk", name)
    assert e.fill == "nan" and cls in e.classes and "differs from the benign launch" in str(e)


@pytest.mark.parametrize("name", [VARLEN, "varlen_D128_fused_c1"])
def test_b_ragged_tile_reads_the_next_sequence(name):
    e = _fails("tile_into_next_seq", name)
    assert e.fill == "nan" and "neighbour sequence" in e.classes and "sequence" in str(e)


@pytest.mark.parametrize("name", [DENSE, "dense_fwd3_D120", VARLEN])
def test_c_chunk_past_d(name):
    e = _fails("chunk_past_d", name)
    assert e.fill == "nan" and "past D" in e.classes


def test_d_table_entry_past_the_last_needed_block():
    e = _fails("table_past_need", PAGED)
    assert e.fill == "nan" and hs.CLASS_NAMES[hs.TABLE] in e.classes


def test_e_other_layer_of_the_right_page():
    e = _fails("other_layer", PAGED)
    assert e.fill == "nan" and e.classes == ("other layer",)


@pytest.mark.parametrize("name", ["window_dense_l100_r0_D128", "window_varlen_l64_r0_D128", "window_paged_l63_r0_D128",
                                  "window_paged_l64_r32_D64"])
def test_f_windowed_pass_starts_a_tile_early(name):
    e = _fails("window_tile_early", name)   # paged: the early tile may also sit behind a table entry that is not needed
    assert e.fill == "nan" and "invisible tile" in e.classes and set(e.classes) <= {"invisible tile", hs.CLASS_NAMES[hs.TABLE]}


@pytest.mark.parametrize("name", [DENSE, PAGED])
def test_g_score_in_the_row_maximum_only_needs_the_huge_fill(name):
    hs.judge(hs.Model("max_only"), _built(name), fills=("nan",))   # a NaN operand drops out of a maximum: nothing to see
    e = _fails("max_only", name, fills=("huge",))
    assert e.fill == "huge" and ("guard row" in e.classes or "stale slot" in e.classes)
    assert _fails("max_only", name).fill == "huge"


@pytest.mark.parametrize("name", [DENSE, VARLEN, PAGED])
def test_h_output_row_past_the_sequence(name):
    e = _fails("output_row_past", name)
    assert e.tensor == "o" and e.classes == ("guard row",) and "not-owned output written" in str(e)


@pytest.mark.parametrize("name", [DENSE, VARLEN])
def test_i_output_bytes_past_d(name):
    e = _fails("output_past_d", name)
    assert e.tensor == "o" and e.classes == ("past D",) and "not-owned output written" in str(e)


@pytest.mark.parametrize("name,tensor", [(DENSE, "k"), (PAGED, "k_cache")])
def test_j_input_modified(name, tensor):
    e = _fails("input_modified", name)
    assert e.tensor == tensor and "input modified" in str(e)


def test_padding_rows_of_the_blocked_output_are_guards():
    """csrc/fa3_fwd5_body.inc predicates every output store on the query row being < Sq: the rows past B*Sq of the last
    256-row block are not written, so the harness holds them to their pre-fill."""
    b = _built("dense_fwd5_kpre_oblk_D64")
    cls = b.bufs["o"].cls
    c = b.case
    assert int((cls == hs.OWNED).sum()) == c.B * c.Sq * c.H * c.D and int((cls == hs.PAD_ROW).sum()) > 0


def test_nonvacuity_is_asserted():
    from dataclasses import replace
    with pytest.raises(AssertionError, match="declared classes of not-owned input are empty"):
        hs.judge(hs.Model(), hs.build(replace(hs.shrunk(CASES[DENSE]), invisible=True), BF))
    with pytest.raises(AssertionError, match="does not declare"):
        hs.judge(hs.Model(), hs.build(replace(hs.shrunk(CASES["window_dense_l0_r0_D64"]), invisible=False), BF))

"""tests/_hostile_decode.py on the CPU: the case table of tests/test_gpu_decode_hostile.py against the host-only route
queries (every case takes the route it names on its embedded views), the table's coverage, the clean torch model of the
launch passing judge() on every case in both dtypes, and every planted out-of-ownership access failing it with its fill,
its tensor and its class of memory named."""
import pytest
import torch

import _hostile_decode as hd

BF, FP = torch.bfloat16, torch.float16
CASES = {c.name: c for c in hd.CASES}
ROUTES, KINDS = ("head", "rows", "gqa"), (False, True)


_SEEN = {}   # case name -> the classes of memory its buffers hold, over every perspective


def _classes(b):
    seen = set()
    for p in [None] + b.persp:
        for name in b.bufs:
            seen |= set(torch.unique(hd.eff_cls(b, name, p)).tolist())
    return seen


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_takes_its_route_on_its_views(name):
    c = CASES[name]
    for dtype in (BF, FP):
        b = hd.build(c, dtype)
        assert hd.route(b, hd.inputs(b, "benign")) == c.route
        hd.nonvacuous(b)
    _SEEN[name] = _classes(b)


def test_table_covers_routes_kinds_and_axes():
    assert {(c.route, c.kv8, c.windowed) for c in hd.CASES} == {(r, k, w) for r in ROUTES for k in KINDS
                                                              for w in (False, True)}
    for r in ROUTES:
        for k in KINDS:
            cell = [c for c in hd.CASES if c.route == r and c.kv8 == k]
            kinds = {c.kind for c in cell}
            assert kinds >= {"none", "inside", "long", "short", "short_win", "sparse", "wide"} and \
                ("below" in kinds) == (r != "rows")
            for c in cell:
                ns, sl = hd.plan(c)
                assert (ns >= 2) == (c.kind != "below") and sl >= 32, c.name
                assert 1 in c.ctxs and c.ctxs.count(0) == 1 and c.B >= 3 and max(c.ctxs) <= c.msl, c.name
                if c.kind in ("inside", "short_win"):
                    assert c.left % 32 and c.left % c.bs and 0 < c.left < max(c.ctxs), c.name
                if c.kind == "below":
                    assert 0 <= c.left < c.q_len and c.q_len > 1, c.name
                if c.kind == "long":
                    assert c.msl == 2100 and hd.plan(c)[0] >= 2 and c.windowed, c.name
                if c.kind.startswith("short"):
                    assert c.cap < c.msl and {c.cap, c.cap + 5, c.cap + c.bs} <= set(c.ctxs), c.name
                if c.kind == "sparse":
                    assert c.msl == 32768 and max(c.ctxs) <= 300, c.name
                if c.kind == "wide":
                    assert c.left >= c.msl + c.q_len and not c.windowed, c.name
    assert {c.bs for c in hd.CASES} >= {1, 16, 64, 256}
    packed = sum(c.q_packed for c in hd.CASES)
    assert len(hd.CASES) // 3 <= packed <= len(hd.CASES) // 3 + 1
    assert {c.out_pad for c in hd.CASES} == {4, 8}
    assert {c.D for c in hd.CASES if c.route == "head"} - {64, 128}
    for dtype in (BF, FP):
        assert {(c.route, c.kv8) for c in hd.CASES if c.dtype == dtype} == {(r, k) for r in ROUTES for k in KINDS}


def test_every_class_has_elements_in_every_route_and_cache_kind():
    """(Run alone, this test builds the cases itself; after the route tests it reads what they recorded.)"""
    want = set(hd.CLASS_NAMES) - {hd.GUARD_SCALE}
    for r in ROUTES:
        for k in KINDS:
            seen = set()
            for c in hd.CASES:
                if c.route == r and c.kv8 == k:
                    if c.name not in _SEEN:
                        _SEEN[c.name] = _classes(hd.build(c))
                    seen |= _SEEN[c.name]
            assert seen >= want | ({hd.GUARD_SCALE} if k else set()), (r, k, [hd.CLASS_NAMES[x] for x in want - seen])


def test_ownership_against_the_contract_slot_by_slot():
    """Brute force over every key of every sequence of two windowed cases: owned <=> lo_b <= j < Lk_b, a table entry is
    owned <=> its block holds an owned slot, pre-window <=> every slot of it lies in front of lo_b."""
    for name in ("head-kv16-short_win", "gqa-fp8-below"):
        c = CASES[name]
        b = hd.build(c)
        cls, tcls = b.cache(b.bufs["k_cache"].cls), b.table(b.bufs["table"].cls)
        bt = b.table(b.bufs["table"].data)
        for s, n in enumerate(c.ctxs):
            lo, lk = max(0, n - c.q_len - c.left), min(n, c.max_blocks * c.bs)
            for j in range(min(b.alloc[s], c.cap)):
                got = int(cls[int(bt[s, j // c.bs]), hd.LAYER, j % c.bs, 0, 0])
                assert got == (hd.OWNED if lo <= j < lk else hd.PRE_WINDOW if j < lo else hd.STALE), (name, s, j)
            for e in range(c.max_blocks):
                owned = any(lo <= j < lk for j in range(e * c.bs, (e + 1) * c.bs))
                pre = (e + 1) * c.bs <= lo and e * c.bs < min(b.alloc[s], c.cap)
                assert int(tcls[s, e]) == (hd.OWNED if owned else hd.PRE_WINDOW if pre else hd.TABLE), (name, s, e)


@pytest.mark.parametrize("dtype", [BF, FP], ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_clean_model_passes(name, dtype):
    hd.judge(hd.Model(), hd.build(CASES[name], dtype))


def _fails(defect, name, **kw):
    with pytest.raises(hd.HostileFailure) as e:
        hd.judge(hd.Model(defect), hd.build(CASES[name]), **kw)
    return e.value


PLAIN, WIN, FP8 = "head-kv16-none", "head-kv16-inside", "head-fp8-none"
STALE, TABLE, PRE = (hd.CLASS_NAMES[x] for x in (hd.STALE, hd.TABLE, hd.PRE_WINDOW))


def test_01_slot_at_lk_at_weight_zero_needs_the_nan_fill():
    hd.judge(hd.Model("slot_at_lk"), hd.build(CASES[PLAIN]), fills=("huge",))   # 0 x huge = 0: nothing to see
    e = _fails("slot_at_lk", PLAIN)
    assert e.fill == "nan" and e.tensor == "o" and set(e.classes) <= {STALE, TABLE} and STALE in e.classes


def test_02_stale_score_in_the_running_maximum_needs_the_huge_fill():
    hd.judge(hd.Model("max_before_mask"), hd.build(CASES[PLAIN]), fills=("nan",))   # a maximum drops a NaN operand
    e = _fails("max_before_mask", PLAIN)
    assert e.fill == "huge" and e.tensor == "o" and set(e.classes) <= {STALE, TABLE} and STALE in e.classes


def test_03_table_entry_past_the_last_needed_block():
    e = _fails("table_past_need", PLAIN)
    # under `benign` the entries past the last needed block name the sequence's own stale pages: both classes reach it
    assert e.fill == "nan" and TABLE in e.classes and set(e.classes) <= {STALE, TABLE} and "per sequence" in str(e)


def test_04_windowed_walk_starts_a_page_early():
    e = _fails("page_early", WIN)
    assert e.fill == "nan" and e.classes == (PRE,)


def test_05_windowed_rows_start_a_key_early():
    e = _fails("key_early", WIN)
    assert e.fill == "nan" and e.classes == (PRE,)


def test_06_q_read_past_d():
    e = _fails("q_past_d", PLAIN)
    assert e.fill == "nan" and e.classes == ("past D",)


def test_07_q_read_at_the_next_head():
    e = _fails("q_next_head", PLAIN)
    assert e.fill == "nan" and e.classes == ("guard head",)


def test_08_fp8_scale_of_the_next_layer():
    e = _fails("scale_next_layer", FP8)
    assert e.fill == "nan" and e.classes == ("other layer",)


def test_09_context_length_of_the_next_sequence():
    e = _fails("ctx_next", PLAIN)
    assert e.fill == "nan" and hd.CLASS_NAMES[hd.GUARD_CTX] in e.classes


def test_10_empty_split_stores_no_lse():
    e = _fails("empty_no_lse", PLAIN, fills=("nan",), parts=("fills",))
    assert e.fill == "nan" and e.classes == ("workspace",) and "per sequence and split" in str(e)
    e = _fails("empty_no_lse", PLAIN, parts=("stale",))
    assert e.fill == "stale" and e.tensor == "o"


def test_11_merge_reads_one_split_too_many():
    e = _fails("merge_extra_split", PLAIN)
    assert e.fill in ("nan", "huge") and e.classes == ("workspace",)


def test_12_o_written_past_d():
    e = _fails("o_past_d", PLAIN)
    assert e.tensor == "o" and e.classes == ("past D",) and "not-owned bytes written" in str(e)


def test_13_partial_stored_past_the_workspace():
    e = _fails("partial_past_ws", PLAIN)
    assert e.tensor == "ws" and e.classes == (hd.CLASS_NAMES[hd.WS_GUARD],) and "not-owned bytes written" in str(e)


def test_14_last_block_through_the_next_sequences_table_row():
    hd.judge(hd.Model("table_next_row"), hd.build(CASES[PLAIN]), parts=("fills", "stale"))   # only a neighbour shows it
    e = _fails("table_next_row", PLAIN)
    assert e.fill == "nan" and e.classes == (hd.CLASS_NAMES[hd.NEIGHBOUR],) and "[sequence" in str(e)


def test_defects_are_all_planted():
    import inspect
    src = inspect.getsource(inspect.getmodule(test_defects_are_all_planted))
    assert all(f'"{d}"' in src for d in hd.DEFECTS) and len(hd.DEFECTS) == 14

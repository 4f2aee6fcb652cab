"""tests/_repeat.py on the CPU: planted differences are found and localised, equal snapshots with NaN compare equal, the driver
reports a launch that depends on its call index; and the case table of tests/test_gpu_repeatable.py covers every route, cache
write and row kernel, with shifted buffers that still pass each op's own argument checks and take the same route."""
import os
import re
import struct
from types import SimpleNamespace

import pytest
import torch

import _repeat as rp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _snap(**t):
    return rp.snapshot(t)


def _pair(shape, dtype=torch.bfloat16, seed=0):
    a = torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dtype)
    return a, a.clone()


def test_one_flipped_bit():
    a, b = _pair((700, 600))
    b.view(torch.int16)[513, 300] ^= 4
    d = rp.compare(_snap(y=a), _snap(y=b))["y"]
    assert (d.bytes, d.elements, d.first, d.total) == (1, 1, (513, 300), 700 * 600)
    assert d.tiles == {(2, 1): 1} and not d.attn
    text = rp.report({"y": d})
    assert "first at (513, 300)" in text and "(2, 1): 1" in text and "1 bytes in 1 of 420000" in text
    assert not any(rp.compare(_snap(y=a), _snap(y=a.clone())).values())


def test_one_tile_and_one_row():
    a, b = _pair((1000, 1024), torch.float16, 1)
    b[256:512, 768:1024] += 1.0
    d = rp.compare(_snap(y=a), _snap(y=b))["y"]
    assert d.tiles == {(1, 3): d.elements} and d.elements > 256 * 256 * 0.99 and d.first[0] == 256 and 768 <= d.first[1] < 772
    c = a.clone()
    c[777] = -c[777] - 1
    d = rp.compare(_snap(y=a), _snap(y=c))["y"]
    assert d.elements == 1024 and d.first == (777, 0) and d.tiles == {(3, j): 256 for j in range(4)}


def test_nan_payload_and_signed_zero():
    a = torch.zeros(4, 8)
    a[1, 2] = float("nan")
    a[3, 3] = float("nan")
    same = a.clone()
    assert not torch.equal(a, same)                                  # values: NaN != NaN
    assert not any(rp.compare(_snap(x=a), _snap(x=same)).values())   # bytes: the same NaN is the same
    b = a.clone()
    b.view(torch.int32)[1, 2] ^= 1                                   # still a NaN, another payload
    assert torch.isnan(b[1, 2])
    d = rp.compare(_snap(x=a), _snap(x=b))["x"]
    assert (d.bytes, d.elements, d.first) == (1, 1, (1, 2))
    c = a.clone()
    c[0, 5] = -0.0
    assert bool((c[0] == a[0]).all())                                # values: -0 == +0
    d = rp.compare(_snap(x=a), _snap(x=c))["x"]
    assert (d.bytes, d.elements, d.first) == (1, 1, (0, 5))
    assert struct.pack("<f", -0.0)[3] == 0x80


def test_attention_histograms():
    o, o2 = _pair((2, 300, 3, 64), seed=2)
    o2[1, 130:140, 2] = 0
    d = rp.compare(_snap(o=rp.Attn(o, "bshd")), _snap(o=rp.Attn(o2, "bshd")))["o"]
    assert set(d.attn) == {(1, 2, 2)} and d.first[:3] == (1, 130, 2) and not d.tiles
    cu = (0, 300, 377, 977)
    p, p2 = _pair((977, 2, 64), seed=3)
    p2[300 + 70, 1] = 0     # sequence 1, row 70
    p2[377 + 10, 0] = 0     # sequence 2, row 10
    d = rp.compare(_snap(o=rp.Attn(p, "thd", cu)), _snap(o=rp.Attn(p2, "thd", cu)))["o"]
    assert set(d.attn) == {(1, 1, 1), (2, 0, 0)}
    lse, lse2 = _pair((2, 977), torch.float32, 4)
    lse2[1, 376] += 1
    d = rp.compare(_snap(l=rp.Attn(lse, "ht", cu)), _snap(l=rp.Attn(lse2, "ht", cu)))["l"]
    assert d.attn == {(1, 1, 1): 1} and "(sequence, head, row // 64)" in rp.report({"l": d})


def test_snapshots_are_views_and_take_strided_results():
    buf = torch.zeros(10, 40)
    view = buf[1:9, 8:24]
    s = _snap(y=view, none=None)
    assert set(s) == {"y"} and s["y"].shape == (8, 16)
    buf[3, 10] = 1.0
    t = _snap(y=torch.zeros(8, 16))
    assert rp.compare(t, s)["y"].first == (2, 2)    # the snapshot reads the buffer as it is now
    assert rp.compare(_snap(s=torch.tensor(1.0)), _snap(s=torch.tensor(2.0)))["s"].elements == 1


def test_fresh_and_place():
    for shift in (0,) + rp.SHIFTS:
        f = rp.fresh((5, 24), torch.bfloat16, "cpu", shift)
        assert (f.view(torch.uint8) == 0xFF).all() and torch.isnan(f).all() and f.is_contiguous()
        base = f.untyped_storage().data_ptr()
        assert f.data_ptr() - base == shift
        src = torch.arange(5 * 24, dtype=torch.float32).view(5, 24)[:, :16]
        g = rp.place(src, shift)
        assert torch.equal(g, src) and g.stride() == src.stride() and g.data_ptr() - g.untyped_storage().data_ptr() == shift
        q = torch.arange(64, dtype=torch.uint8).view(torch.float8_e4m3fn).view(4, 16)
        assert torch.equal(rp.place(q, shift).view(torch.uint8), q.view(torch.uint8))
    assert all(s % 16 == 0 for s in rp.SHIFTS) and rp.SHIFTS[0] % 32 and rp.SHIFTS[1] % 64 and rp.SHIFTS[2] > 4096
    assert rp.aligned16(torch.zeros(64)[4:8]) and not rp.aligned16(torch.zeros(64)[1:8])


def _fake(conditions):
    calls = []

    def launch(p):
        p.out[2, 5] = float(len(calls))   # the launch's own call index: repeat 0 writes 0
        calls.append(p)
        return p.out

    def make(shift):
        out = rp.fresh((4, 300), torch.float32, "cpu", shift)
        return SimpleNamespace(out=out)

    judged = []
    res = rp.run_repeats(make, launch, lambda p, ret: {"out": ret}, conditions, repeats=rp.REPEATS,
                         judge=lambda p, ret: judged.append(float(ret[2, 5])))
    return res, calls, judged


def test_run_repeats_reports_the_call_index_element():
    res, calls, judged = _fake([rp.Condition(), rp.Condition("cold"), rp.Placement()])
    f = res.failure
    assert judged == [0.0] and f is not None and f.condition == "back-to-back"
    assert res.ran == ["back-to-back"] and len(calls) == 1 + rp.REPEATS and res.launches == 1 + rp.REPEATS   # nothing queued after it
    assert [i for i, _ in f.repeats] == list(range(1, rp.REPEATS + 1))
    for i, diffs in f.repeats:
        d = diffs["out"]
        assert (d.elements, d.first, d.tiles) == (1, (2, 5), {(0, 0): 1})
    with pytest.raises(AssertionError, match=r"condition 'back-to-back', repeat 1:\nout: . bytes in 1 of 1200 elements differ, first at \(2, 5\)"):
        res.check("fake")
    # every compared result is overwritten with 0xFF once compared; the judged one stays
    assert all((p.out.view(torch.uint8) == 0xFF).all() for p in calls[1:])
    assert calls[0].out[2, 5] == 0.0 and int((calls[0].out.view(torch.uint8) != 0xFF).sum()) == 4


def test_run_repeats_passes_a_reproducible_launch_and_places_buffers():
    seen = []

    def make(shift):
        seen.append(shift)
        return SimpleNamespace(out=rp.fresh((3, 16), torch.float16, "cpu", shift), x=rp.place(torch.ones(3, 16), shift))

    def launch(p):
        p.out.copy_(p.x * 3)
        p.x.zero_()      # an op that writes its input in place: the next launch gets a restored one
        return p.out

    res = rp.run_repeats(make, launch, lambda p, ret: {"out": ret, "x": p.x}, [rp.Condition(), rp.Placement()])
    assert res.failure is None and res.check("ok") is res
    assert seen == [0] + [0] * rp.REPEATS + list(rp.SHIFTS) and res.launches == 1 + rp.REPEATS + 3
    assert res.ran == ["back-to-back", "placement"]


# ---- the case table ------------------------------------------------------------------------------------------------------------
def _table():
    import test_gpu_repeatable as tg
    return tg


def test_every_route_write_and_row_kernel_has_a_case():
    from mio import _lib
    tg = _table()
    covered = {c for case in tg.CASES for c in case.covers}
    want = set()
    for prefix, routes in (("gemm", _lib.GEMM_ROUTES), ("fa3", _lib.FA3_ROUTES), ("fa3_varlen", _lib.FA3_VARLEN_ROUTES),
                           ("fa3_paged", _lib.FA3_PAGED_ROUTES), ("decode", _lib.DECODE_ROUTES)):
        want |= {f"{prefix}:{r}" for r in routes.values() if r != "empty"}
    # the cache-write and row-kernel entry points of include/mio_hip.h
    header = open(os.path.join(ROOT, "include", "mio_hip.h")).read()
    entries = set(re.findall(r"^int (mio_\w+)\(", header, re.M))
    op_of = {"rope_rows": "apply_rotary", "qknorm_rope_rows": "qk_norm_rotary"}
    writes = {e for e in entries if re.match(r"mio_(reshape_and_cache|rope_|qknorm_)", e)}
    assert len(writes) == 10, sorted(writes)
    names = {c.name for c in tg.CASES}
    for e in writes:
        op = e[len("mio_"):]
        kv8 = op.endswith("_kv8")
        op = op[:-4] if kv8 else op
        op = op_of.get(op, op)
        want.add(f"write:{op}")
        if op in tg.WRITES:
            assert f"{op}-{'fp8' if kv8 else 'kv16'}" in names, e
    rows = {e for e in entries if re.match(r"mio_(layernorm_fwd|rmsnorm_fwd|attn_merge)", e)}
    assert rows == {"mio_layernorm_fwd", "mio_layernorm_fwd_bx", "mio_rmsnorm_fwd", "mio_attn_merge"}
    want |= {"row:layernorm", "row:rmsnorm", "row:attn_merge"}
    assert any(n.startswith("layernorm") and n.endswith("blocked") for n in names)   # mio_layernorm_fwd_bx
    want |= {f"prep:{p}" for p in ("block_weight", "block_weight_glu", "ln_fold_weight", "rms_fold_weight", "quantize_weight_w8")}
    want |= {"skinny:w16", "skinny:w8", "fold:rms", "module:block_fold", "module:block_rms_swiglu", "module:decode_step"}
    want |= {f"mlp:{a}:{p}" for a in tg.MLP_ACTS for p in ("blocked", "two_launch")}
    assert want <= covered, sorted(want - covered)
    assert len(names) == len(tg.CASES), "case names repeat"
    # every decode family: route x cache kind x windowed, each a case whose launch splits (asserted on the GPU), and the slices
    dec = [c for c in tg.CASES if c.family == "decode"]
    assert len(dec) == 13 and any(c.name.endswith("bt-slice") for c in dec)
    # every condition runs on every case but the decode GEMMs, which are covered alone by their own files
    assert {c.family for c in tg.CASES if c.conditions != "all"} == {"decode_gemm"}


def test_shared_cache_slots_have_one_writer():
    tg = _table()
    for dtype in tg.DTYPES:
        for kv8 in (False, True):
            sc = tg._scene(dtype, kv8)
            assert torch.equal(sc.bt[1, :2], sc.bt[0, :2]), "the scene no longer shares its prefix pages"
            assert tg.single_writer(sc, sc.has_row) and tg.single_writer(sc, sc.live & sc.has_row)
            assert int(sc.has_row.sum()) > int((sc.live & sc.has_row).sum()) > 80
            assert int((sc.seq < 0).sum()) == 2 and int((~sc.has_row & (sc.seq >= 0)).sum()) == 7


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_shifted_buffers_pass_the_argument_checks(dtype, monkeypatch):
    """Every case whose operands can be built without a GPU: buffers shifted by 16, 48 and 4112 bytes keep every stride, stay
    16-byte aligned, pass the op's own argument checks (the route query runs them, with the device check out of the way) and
    take the unshifted route.  The cases that build their operands with device kernels (the GEMM tables, the decode GEMMs,
    ln_fold_weight) assert the same on the GPU."""
    from mio import ops
    monkeypatch.setattr(ops, "_need_cuda", lambda *ts: None)
    tg = _table()
    ran = 0
    for case in tg.CASES:
        if not case.host or dtype not in case.dtypes:
            continue
        prob = case.build(dtype, "cpu")
        tg.check_placement(case, prob, "cpu")
        ran += 1
    assert ran >= 45
    assert {c.family for c in tg.CASES if not c.host} <= {"gemm", "mlp", "decode_gemm", "prep", "module"}


def _stub_device_preparations(monkeypatch):
    """The GEMM tables build their operands on their DEV with device kernels.  The argument checks and route queries read shapes,
    strides and addresses only, so here DEV is the CPU and every preparation returns zeros of the shape the real one returns."""
    import test_gpu_gemm_matrix as gm
    import test_gpu_gemm_skinny as ts
    import test_gpu_gemm_skinny_w8 as t8
    from mio import ops
    tg = _table()
    for m in (gm, ts, t8, tg):
        monkeypatch.setattr(m, "DEV", "cpu")
    monkeypatch.setattr(tg, "_cus", lambda: 256)
    monkeypatch.setattr(ops, "_need_cuda", lambda *ts_: None)
    up = lambda n, m: (n + m - 1) // m  # noqa: E731
    monkeypatch.setattr(ops, "block_weight", lambda w: torch.zeros(up(w.shape[0], 256) * 256, w.shape[1], dtype=w.dtype))
    monkeypatch.setattr(ops, "block_weight_glu", lambda wg, wu: torch.zeros(up(wg.shape[0], 128) * 256, wg.shape[1], dtype=wg.dtype))

    def ln_fold_weight(w, gamma, beta, bias, blocked=True):
        ws = torch.zeros(w.shape, dtype=w.dtype)
        return (ops.block_weight(ws) if blocked else ws), torch.zeros(w.shape[0], dtype=w.dtype)

    def gemm_ln(x, w_blocked, bias, *, M, N, K, out_blocked=False, stats_out=False, **_):
        y = torch.zeros(up(M, 256) * 256 if out_blocked else M, N, dtype=x.dtype)
        return y, (torch.zeros(ops.ln_stats_shape(M, N), dtype=torch.float32) if stats_out else None)

    monkeypatch.setattr(ops, "ln_fold_weight", ln_fold_weight)
    monkeypatch.setattr(ops, "rms_fold_weight", lambda w, gamma, bias=None, blocked=True: (ln_fold_weight(w, gamma, None, bias, blocked)[0], bias))
    monkeypatch.setattr(ops, "gemm_ln", gemm_ln)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_shifted_buffers_of_the_gemm_tables_pass_the_argument_checks(dtype, monkeypatch):
    """The same for the cases whose operands the GEMM tables build (GEMM routes, fused MLP, decode GEMMs, ln_fold_weight), on
    shape-only operands.  The three module cases are left to the GPU run: their operands are modules on the device, only the
    input tensor moves, and there is no route query to ask."""
    _stub_device_preparations(monkeypatch)
    tg = _table()
    ran = set()
    for case in tg.CASES:
        if case.host or case.family == "module" or dtype not in case.dtypes:
            continue
        tg.check_placement(case, case.build(dtype, "cpu"), "cpu")
        ran.add(case.family)
    assert ran == {"gemm", "mlp", "decode_gemm", "prep"}
    assert sum(c.family == "module" for c in tg.CASES) == 3

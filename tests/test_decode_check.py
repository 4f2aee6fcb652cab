"""No-GPU self-test of tests/_decode_check.py: its reference agrees with the oracle, an fp64 result rounded to the storage
dtype passes, the model lies within 1 u of the reference, hostile_cache() fills what it says, the defects a decode kernel
can have are rejected when injected into one sequence or row of a mixed batch, and the case table of
tests/test_gpu_decode_matrix.py takes the routes it names and covers what it must.

The defects (each in bf16 and fp16, in a batch of contexts 5000, 4096, 4097, 2047, 1311, 129, 128, 33, 32, 31, 1, 0 unless
noted), and the verdict of the whole-tensor aggregate the decode tests used alone before (rel = mean|d| / mean|ref| and
max|d| < atol * max(1, max|ref|); OLD_ACCEPTS below, asserted):
  last_key        the ctx-4096 sequence loses its last key (5.9 u worst row in bf16)   old: passes in both
  last_8          the ctx-5000 sequence loses its last 8 keys (19 u)                   old: passes in both
  last_chunk      the ctx-5000 sequence loses its last 128 keys (67 u)                 old: bf16 passes, fp16 fails
  first_split     the ctx-5000 sequence loses the first of four splits (187 u)         old: fails in both
  extra_key       the ctx-4096 sequence includes slot ctx (26 u)                       old: passes in both
  merge_weight    one of four splits merged with weight 1, not exp(lse_s - M) (22 u)   old: bf16 passes, fp16 fails
  swapped_heads   two heads of a GQA group swapped in the ctx-1311 sequence            old: fails in both
  stale_empty     the empty sequence's rows left at 1e-3                               old: passes in both
  zero_row        one row of the ctx-2047 sequence all zero                            old: fails in both
  window_early / window_late   (q_len 3, left 1000) row 1 of the ctx-5000 sequence starts one key early / late
                  (8.9 u / 18 u)                                                       old: bf16 passes, fp16 fails
  no_v_scale      (fp8 cache) one split's partial output misses v_scale                old: fails in both
The model's worst row on these batches is 0.5-0.7 u, so the smallest of them is 8x the yardstick and 2.8x the bar.
"""
import ctypes as C
import functools
import math

import pytest
import torch

import oracle
import _decode_check as dc

BF, FP = torch.bfloat16, torch.float16
CTXS = [5000, 4096, 4097, 2047, 1311, 129, 128, 33, 32, 31, 1, 0]
ALIGNED = 1 << 20  # a fake 16-byte aligned device address: the route queries dereference nothing


def _friendly(ctxs, *, bs, Hkv, D, cache_dtype, g, scale=1.0):
    """A cache filled with randn everywhere, one spare block behind every sequence's last (slot ctx is finite)."""
    maxb = (max(ctxs) + bs - 1) // bs + 1
    nb = len(ctxs) * maxb
    vals = lambda: torch.randn(nb, 1, bs, Hkv, D, generator=g) * scale
    kc, vc = (vals().to(cache_dtype) for _ in range(2))
    bt = torch.randperm(nb, generator=g).view(len(ctxs), maxb).to(torch.int32)
    return kc, vc, bt


@functools.lru_cache(maxsize=None)
def _batch(dtype, kind):
    """(inputs, ref, lse, model_o) of the batch a defect is injected into; kind: plain / window / fp8."""
    g = torch.Generator().manual_seed({"plain": 1, "window": 2, "fp8": 3}[kind])
    H, Hkv, D, q_len, left, ctxs = 32, 4, 128, 1, -1, CTXS
    ks = vs = 1.0
    if kind == "window":
        H, Hkv, q_len, left, ctxs = 8, 2, 3, 1000, [5000, 300, 0, 1311]
    if kind == "fp8":
        H, Hkv, ctxs, ks, vs = 8, 2, [5000, 300, 0, 1311], 0.21, 0.47
    kc, vc, bt = _friendly(ctxs, bs=16, Hkv=Hkv, D=D, cache_dtype=dc.F8 if kind == "fp8" else dtype, g=g,
                           scale=3.0 if kind == "fp8" else 1.0)
    q = (torch.randn(len(ctxs), H, q_len, D, generator=g) * 1.5).to(dtype)
    ctx = torch.tensor(ctxs, dtype=torch.int32)
    inp = dict(q=q, kc=kc, vc=vc, bt=bt, ctx=ctx, left=left, ks=ks, vs=vs, scale=D ** -0.5)
    kw = dict(left=left, k_scale=ks, v_scale=vs)
    ref, lse = dc.reference(q, kc, vc, bt, ctx, 16, 0, **kw)
    mo = dc.model(q, kc, vc, bt, ctx, 16, 0, dtype=dtype, p16=True, **kw)
    return inp, ref, lse, mo


def _keys(inp, b, lo, hi, vis=None):
    """(o, lse) of sequence b over the keys lo .. hi-1 (fp64); vis [q_len, hi - lo] restricts rows."""
    k, v = dc.seq_kv(inp["kc"], inp["vc"], inp["bt"][b], hi, 16, 0, inp["ks"], inp["vs"])
    q_len = inp["q"].shape[2]
    if vis is None:
        vis = torch.ones(q_len, hi - lo, dtype=torch.bool)
    return dc.seq_attention(inp["q"][b], k[lo:hi], v[lo:hi], inp["scale"], vis)


def _merge(parts, weights=None):
    """Merge split states [(o, lse)] as decode_reduce_kernel does; weights overrides exp(lse_s - M) per split."""
    lses = torch.stack([l for _, l in parts])
    w = torch.exp(lses - lses.amax(0))
    if weights is not None:
        w = weights(w)
    return sum(wi[..., None] * o for wi, (o, _) in zip(w, parts)) / w.sum(0)[..., None]


def _mutate(name, dtype):
    kind = {"window_early": "window", "window_late": "window", "no_v_scale": "fp8"}.get(name, "plain")
    inp, ref, lse, mo = _batch(dtype, kind)
    o = ref.clone()
    if name == "last_key":
        o[1] = _keys(inp, 1, 0, 4095)[0]
    elif name == "last_8":
        o[0] = _keys(inp, 0, 0, 4992)[0]
    elif name == "last_chunk":
        o[0] = _keys(inp, 0, 0, 4872)[0]
    elif name == "first_split":
        o[0] = _keys(inp, 0, 1250, 5000)[0]
    elif name == "extra_key":
        o[1] = _keys(inp, 1, 0, 4097)[0]
    elif name == "merge_weight":
        parts = [_keys(inp, 0, a, a + 1250) for a in range(0, 5000, 1250)]
        assert torch.allclose(_merge(parts), ref[0], atol=1e-12)

        def one(w):
            w = w.clone()
            w[1] = 1.0
            return w
        o[0] = _merge(parts, one)
    elif name == "swapped_heads":
        o[4, [0, 1]] = ref[4, [1, 0]]
    elif name == "stale_empty":
        o[11] = 1e-3
    elif name == "zero_row":
        o[3, 5, 0] = 0
    elif name in ("window_early", "window_late"):
        vis = dc.seq_visible(5000, 5000, 3, 1000)
        lo = 5000 - 3 + 1 - 1000
        assert vis[1, lo] and not vis[1, lo - 1]
        if name == "window_early":
            vis[1, lo - 1] = True
        else:
            vis[1, lo] = False
        o[0] = _keys(inp, 0, 0, 5000, vis)[0]
    elif name == "no_v_scale":
        parts = [_keys(inp, 0, a, a + 1250) for a in range(0, 5000, 1250)]
        assert torch.allclose(_merge(parts), ref[0], atol=1e-12)
        parts[2] = (parts[2][0] / inp["vs"], parts[2][1])
        o[0] = _merge(parts)
    else:
        raise KeyError(name)
    return o.to(dtype), ref, lse, mo


MUTATIONS = ["last_key", "last_8", "last_chunk", "first_split", "extra_key", "merge_weight", "swapped_heads",
             "stale_empty", "zero_row", "window_early", "window_late", "no_v_scale"]
# what the old whole-tensor aggregate lets through (the module docstring's table)
OLD_ACCEPTS = {(m, BF) for m in ("last_key", "last_8", "last_chunk", "extra_key", "merge_weight", "stale_empty",
                                 "window_early", "window_late")} | {(m, FP) for m in ("last_key", "last_8", "extra_key",
                                                                                      "stale_empty")}


def test_reference_matches_oracle():
    g = torch.Generator().manual_seed(0)
    for dtype, bs, H, Hkv, D, q_len in ((BF, 16, 8, 2, 128, 1), (FP, 12, 4, 4, 80, 3)):
        ctxs = [300, 17, 0, 129, 1]
        kc, vc, bt = _friendly(ctxs, bs=bs, Hkv=Hkv, D=D, cache_dtype=dtype, g=g)
        q = torch.randn(len(ctxs), H, q_len, D, generator=g).to(dtype)
        ctx = torch.tensor(ctxs, dtype=torch.int32)
        o, lse = dc.reference(q, kc, vc, bt, ctx, bs, 0)
        assert torch.allclose(o, oracle.paged_attention_forward(q, kc, vc, bt, ctx, bs, 0), rtol=0, atol=1e-12)
        assert (lse[2] == float("-inf")).all() and torch.isfinite(lse[[0, 1, 3, 4]]).all() and (o[2] == 0).all()
        # a window that covers everything, an explicit scale, unit cache scales: the same numbers
        o2, lse2 = dc.reference(q, kc, vc, bt, ctx, bs, 0, left=400, scale=D ** -0.5, k_scale=1.0, v_scale=1.0)
        assert torch.allclose(o, o2, rtol=0, atol=1e-12) and torch.allclose(lse, lse2, rtol=0, atol=1e-12)


def test_reference_window_table_row_and_scales():
    g = torch.Generator().manual_seed(1)
    bs, H, Hkv, D, q_len = 8, 4, 2, 64, 3
    kc, vc, bt = _friendly([100], bs=bs, Hkv=Hkv, D=D, cache_dtype=BF, g=g)
    q = torch.randn(1, H, q_len, D, generator=g).to(BF)
    ctx = torch.tensor([100], dtype=torch.int32)
    k, v = dc.seq_kv(kc, vc, bt[0], 100, bs, 0)
    # row qi sees keys ctx - q_len + qi - left .. ctx - 1: by hand, row by row
    o, lse = dc.reference(q, kc, vc, bt, ctx, bs, 0, left=10)
    for qi in range(q_len):
        lo = 100 - q_len + qi - 10
        want, wl = dc.seq_attention(q[0, :, qi:qi + 1], k[lo:], v[lo:], D ** -0.5, torch.ones(1, 100 - lo, dtype=torch.bool))
        assert torch.allclose(o[0, :, qi], want[:, 0], atol=1e-12) and torch.allclose(lse[0, :, qi], wl[:, 0], atol=1e-12)
    # keys past the block-table row do not exist: a 9-block row (72 keys) of a 100-key context
    o, _ = dc.reference(q, kc, vc, bt[:, :9].contiguous(), ctx, bs, 0)
    want, _ = dc.seq_attention(q[0], k[:72], v[:72], D ** -0.5, torch.ones(q_len, 72, dtype=torch.bool))
    assert torch.allclose(o[0], want, atol=1e-12)
    # an fp8 cache stands for x8 * scale
    k8, v8 = dc.quantise(kc.float() * 3, 1.0), dc.quantise(vc.float() * 3, 1.0)
    o, _ = dc.reference(q, k8, v8, bt, ctx, bs, 0, k_scale=0.21, v_scale=0.47)
    want, _ = dc.reference(q, k8.double() * 0.21, v8.double() * 0.47, bt, ctx, bs, 0)
    assert torch.allclose(o, want, atol=1e-12)


@pytest.mark.parametrize("dtype", [BF, FP])
@pytest.mark.parametrize("kind", ["plain", "window", "fp8"])
def test_rounded_reference_and_model_pass(dtype, kind):
    inp, ref, lse, mo = _batch(dtype, kind)
    fam = (dtype, "gqa", "fp8" if kind == "fp8" else "kv16")
    st = dc.check(ref.to(dtype), ref, lse, dtype, fam, mo, "fp64 rounded")
    assert st["worst"] <= 0.75
    dc.check(mo, ref, lse, dtype, fam, mo, "model against its own bars")
    assert dc.measure(mo, ref, lse, dtype)["worst"] <= 1.0
    rel, mx, ok = dc.old_aggregate(ref.to(dtype), ref, dtype)
    assert ok and rel == 0


@pytest.mark.parametrize("p16", [False, True])
def test_model_within_one_u_on_the_matrix_data_kinds(p16):
    seen = set()
    for case in dc.CASES:
        key = (case["data"], case["kv8"], case["dtype"])
        if key in seen or (case["route"] == "gqa") != p16:
            continue
        seen.add(key)
        t = dc.build_case(case)
        ref, lse, mo = dc.case_reference(case, t)
        st = dc.measure(mo, ref, lse, case["dtype"])
        assert st["worst"] <= 1.0, (case["name"], st)
    assert len(seen) >= 12


@pytest.mark.parametrize("dtype", [BF, FP], ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", MUTATIONS)
def test_defect_is_rejected(name, dtype):
    o, ref, lse, mo = _mutate(name, dtype)
    fam = (dtype, "gqa", "fp8" if name == "no_v_scale" else "kv16")
    rel, mx, old_ok = dc.old_aggregate(o, ref, dtype)
    st = dc.measure(o, ref, lse, dtype)
    print(f"{name} {dtype}: old rel {rel:.2e} max {mx:.2e} -> {'pass' if old_ok else 'fail'}; worst row {st['worst']:.1f} u, "
          f"mean {st['mean']:.2f} u, sequence {st['seq']:.1f} u")
    with pytest.raises(AssertionError):
        dc.check(o, ref, lse, dtype, fam, mo, name)
    assert old_ok == ((name, dtype) in OLD_ACCEPTS)


def test_nonfinite_output_is_rejected():
    inp, ref, lse, mo = _batch(BF, "plain")
    o = ref.to(BF)
    o[11, 0, 0, 3] = float("nan")  # in an empty sequence's row
    with pytest.raises(AssertionError, match="non-finite"):
        dc.check(o, ref, lse, BF, (BF, "head", "kv16"), mo)


# ---- hostile_cache ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cache_dtype", [BF, FP, dc.F8])
@pytest.mark.parametrize("bs,max_blocks", [(16, None), (1, None), (12, 8)])
def test_hostile_cache_fill(cache_dtype, bs, max_blocks):
    g = torch.Generator().manual_seed(4)
    ctxs, L, layer, Hkv, D = [100, 0, 1, 37, 96, 101], 3, 1, 2, 16
    kc, vc, bt, nan_block = dc.hostile_cache(ctxs, block_size=bs, Hkv=Hkv, D=D, L=L, layer=layer, cache_dtype=cache_dtype,
                                             gen=g, max_blocks=max_blocks, k_scale=0.02, v_scale=0.02)
    nb, maxb = kc.shape[0], bt.shape[1]
    assert 0 <= nan_block < nb and bt.min() >= 0 and bt.max() < nb
    owned = torch.zeros(nb, bs, dtype=torch.bool)   # the slots reference() reads
    blocks = []
    for b, c in enumerate(ctxs):
        n = dc.seq_len_eff(c, maxb, bs)
        need = (n + bs - 1) // bs
        mine = bt[b, :need].tolist()
        blocks += mine
        assert (bt[b, need:] == nan_block).all()
        pos = torch.arange(n)
        owned[bt[b, pos // bs].long(), pos % bs] = True
    assert len(set(blocks)) == len(blocks) and nan_block not in blocks   # disjoint, and nobody owns the NaN block
    assert max_blocks is None or any(c > maxb * bs for c in ctxs)
    for cache in (kc, vc):
        nan = dc.is_nan_slots(cache)
        assert nan[:, [0, 2]].all()                      # the other layers
        assert torch.equal(nan[:, layer], ~owned)        # the tested layer: NaN exactly where nobody owns
        assert torch.isfinite(cache[:, layer][owned].float()).all()
    q = torch.randn(len(ctxs), 4, 2, D, generator=g).to(BF)
    o, lse = dc.reference(q, kc, vc, bt, torch.tensor(ctxs), bs, layer, left=5, k_scale=0.02, v_scale=0.02)
    assert torch.isfinite(o).all() and (lse[1] == float("-inf")).all()


# ---- the case table ------------------------------------------------------------------------------------------------
def _route(case):
    from mio import _lib
    qs, os_ = dc.case_strides(case)
    qs, os_ = (C.c_int64 * 3)(*qs), (C.c_int64 * 3)(*os_)
    dt = 0 if case["dtype"] == BF else 1
    tail = (case["B"], case["H"], case["Hkv"], case["q_len"], case["D"], dc.case_layers(case), dc.LAYER, case["bs"],
            case["max_blocks"], case["msl"], 1.0 / math.sqrt(case["D"]))
    if case["kv8"]:
        r = _lib.lib.mio_fa3_decode_kv8_route(ALIGNED, ALIGNED, ALIGNED, ALIGNED, ALIGNED, ALIGNED, ALIGNED, ALIGNED, qs,
                                              os_, *tail, case["left"], dt, None, None)
    else:
        r = _lib.lib.mio_fa3_decode_window_route(ALIGNED, ALIGNED, ALIGNED, ALIGNED, ALIGNED, ALIGNED, qs, os_, *tail,
                                                 case["left"], -1, dt, None, None)
    assert r >= 0, (case["name"], _lib.lib.mio_last_error().decode())
    return _lib.DECODE_ROUTES[r]


def test_dtype_ids():
    from mio import ops
    assert ops._dtype_id(torch.zeros(1, dtype=BF)) == 0 and ops._dtype_id(torch.zeros(1, dtype=FP)) == 1


@pytest.mark.parametrize("case", dc.CASES + dc.WORKSPACE_CASES, ids=lambda c: c["name"])
def test_case_route(case):
    assert _route(case) == case["route"]


def _windowed(case):
    return case["left"] >= 0 and not case["equal_unwindowed"]


def test_case_table_covers_all_twelve_kernels():
    names = [c["name"] for c in dc.CASES]
    assert len(set(names)) == len(names)
    assert {(c["route"], c["kv8"], _windowed(c)) for c in dc.CASES} == {(r, k, w) for r in ("head", "rows", "gqa")
                                                                        for k in (False, True) for w in (False, True)}
    fams = {dc.family(c) + (_windowed(c),) for c in dc.CASES}
    assert len(fams) == 24   # every (q dtype, route, cache kind) family with a window and without


def test_case_table_axes():
    for route in ("head", "rows", "gqa"):
        for kv8 in (False, True):
            cell = [c for c in dc.CASES if c["route"] == route and c["kv8"] == kv8]
            assert {c["bs"] for c in cell} >= {1, 8, 12, 16, 64, 256}
            assert {c["data"] for c in cell} == {"randn", "needle", "offset", "vmean"}
            assert {c["needle"] for c in cell} >= {"first", "last", "win_in", "win_out", "255", "256", "mid"}
            assert {c["dtype"] for c in cell if c["data"] == "randn"} == {BF, FP}
            lefts = {c["left"] for c in cell}
            assert {-1, 0, 37, 1050, 1029} <= lefts
            assert any(0 < c["left"] < c["q_len"] for c in cell) or route == "rows"
            assert any(c["equal_unwindowed"] and c["left"] >= c["msl"] + c["q_len"] for c in cell)
            assert any(c["msl"] == 32768 and max(c["ctxs"]) <= 300 for c in cell)
            assert any(c["q_packed"] for c in cell) and any(c["out_pad"] for c in cell)
            # a windowed case whose span left + q_len alone has several splits
            assert any(c["left"] >= 1024 and c["msl"] > c["left"] + c["q_len"] for c in cell)
            # a block-table row shorter than max_seq_len: contexts that fill it, exceed it by 5 and by a block
            short = [c for c in cell if c["max_blocks"] * c["bs"] < c["msl"]]
            assert {c["left"] >= 0 for c in short} == {False, True}
            for c in short:
                cap = c["max_blocks"] * c["bs"]
                assert {cap, cap + 5, cap + c["bs"]} <= set(c["ctxs"]) and max(c["ctxs"]) <= c["msl"]
            g = dc.GRAN[route]
            ctxs = set().union(*(c["ctxs"] for c in cell))
            assert {0, 1, g - 1, g, g + 1, 511, 512, 513, 1100, 2100} <= ctxs
            for bs in (8, 12, 16, 64, 256):
                assert any({bs - 1, bs, bs + 1} <= set(c["ctxs"]) for c in cell if c["bs"] == bs), (route, kv8, bs)
    head = [(c["D"], c["kv8"]) for c in dc.CASES if c["route"] == "head"]
    assert {d for d, k in head if not k} >= {8, 48, 80, 96, 112, 128, 64}
    assert {d for d, k in head if k} >= {16, 48, 80, 96, 112, 128}
    rows = {(c["kv8"], c["D"], c["Hkv"]) for c in dc.CASES if c["route"] == "rows"}
    assert rows >= {(False, 64, 2), (False, 64, 8), (False, 64, 16), (False, 64, 32), (True, 64, 4), (True, 64, 16),
                    (True, 64, 64)} and any(d == 128 for k, d, _ in rows if k) and any(d == 128 for k, d, _ in rows if not k)
    assert {c["B"] for c in dc.CASES if c["route"] == "rows"} == {16, 18}
    for kv8 in (False, True):
        gqa = [c for c in dc.CASES if c["route"] == "gqa" and c["kv8"] == kv8]
        assert {c["B"] for c in gqa} == {1, 3, 12} and {c["D"] for c in gqa} == {64, 128}
        assert {(c["H"] // c["Hkv"]) * c["q_len"] for c in gqa} >= {1, 2, 3, 6, 12, 16}
        assert {c["H"] // c["Hkv"] for c in gqa if c["q_len"] == 1} >= {1, 2, 3, 6, 12, 16}
        assert {c["bs"] for c in gqa} >= {1, 12}


def test_case_table_batches_and_splits():
    """At most 128 units and max_seq_len >= 1024, so every dec_nsplit* gives at least two splits; one empty sequence in
    every batch of three or more, none in a smaller one; at least two thirds of the rows live (from reference's lse)."""
    for c in dc.CASES + dc.WORKSPACE_CASES:
        units = {"head": c["B"] * c["H"] * c["q_len"], "rows": c["B"], "gqa": c["B"] * c["Hkv"]}[c["route"]]
        assert units <= 128 and c["msl"] >= 1024 and len(c["ctxs"]) == c["B"], c["name"]
        assert c["ctxs"].count(0) == (1 if c["B"] >= 3 else 0), c["name"]
        assert max(c["ctxs"]) <= c["msl"], c["name"]
        t = dc.build_case(c)
        _, lse = dc.reference(t["q"], t["kc"], t["vc"], t["bt"], t["ctx"], c["bs"], dc.LAYER, left=c["left"],
                              k_scale=t["k_scale"][dc.LAYER], v_scale=t["v_scale"][dc.LAYER])
        live = ~torch.isinf(lse)
        assert live.float().mean().item() >= 2 / 3 - 1e-9, c["name"]
        for b, n in enumerate(c["ctxs"]):
            assert live[b].all() if n > 0 else not live[b].any(), (c["name"], b)

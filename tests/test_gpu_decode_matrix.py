"""Paged decode on the GPU, every kernel route x cache kind x {window, none}, judged row by row against fp64.

Every case of tests/_decode_check.py's table goes through ops.paged_attention_forward over a hostile cache (every slot the
launch may not use is NaN, padded block-table entries name an all-NaN block) into a NaN-prefilled output, asserts the
kernel the launch takes, and is judged by _decode_check.check(): finite, exact zeros for empty rows, per-row error in
units of the dtype's unit roundoff against bars taken from the fp32 model of the same case.  Further: caches whose owned
blocks lie past 2^31 elements / 2^32 bytes, and launches through the C ABI with a workspace of exactly
mio_fa3_decode_workspace_bytes() between guard zones, all-NaN before the launch.
"""
import pytest
import torch

import _decode_check as dc

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _ops():
    from mio import ops
    return ops


def _device_inputs(case, t):
    """q (contiguous, or the q third of a packed [B, q_len, 3, H, D] projection) and the output view of a NaN-filled
    [B, H, q_len, D + out_pad] buffer, on the device."""
    B, H, q_len, D = case["B"], case["H"], case["q_len"], case["D"]
    if case["q_packed"]:
        qkv = torch.full((B, q_len, 3, H, D), float("nan"), dtype=case["dtype"], device=DEV)
        qkv[:, :, 0] = t["q"].permute(0, 2, 1, 3).to(DEV)
        q = qkv[:, :, 0].permute(0, 2, 1, 3)
    else:
        q = t["q"].to(DEV)
    buf = torch.full((B, H, q_len, D + case["out_pad"]), float("nan"), dtype=case["dtype"], device=DEV)
    assert (tuple(q.stride()[:3]), tuple(buf.stride()[:3])) == dc.case_strides(case)
    return q, buf, buf[..., :D]


def _scales(case, t):
    if not case["kv8"]:
        return {}
    return dict(k_scale=torch.tensor(t["k_scale"], dtype=torch.float32, device=DEV),
                v_scale=torch.tensor(t["v_scale"], dtype=torch.float32, device=DEV))


@pytest.mark.parametrize("case", dc.CASES, ids=lambda c: c["name"])
def test_decode_matrix(case):
    ops = _ops()
    t = dc.build_case(case)
    ref, lse, model_o = dc.case_reference(case, t)
    q, buf, out = _device_inputs(case, t)
    args = (t["kc"].to(DEV), t["vc"].to(DEV), t["bt"].to(DEV), t["ctx"].to(DEV), case["bs"], case["msl"], dc.LAYER)
    kw = dict(window_size=(case["left"], -1), **_scales(case, t))
    assert ops.paged_attention_route(q, out, *args, **kw) == case["route"]
    ops.paged_attention_forward(q, out, *args, **kw)
    torch.cuda.synchronize()
    if case["out_pad"]:
        assert torch.isnan(buf[..., case["D"]:]).all(), "the padding behind the output rows was written"
    windowed = case["left"] >= 0 and not case["equal_unwindowed"]
    dc.check(out, ref, lse, case["dtype"], dc.family(case), model_o, case["name"], win=windowed)
    if case["equal_unwindowed"]:   # a window of max_seq_len + q_len or more: the unwindowed kernel, bit for bit
        plain = torch.full_like(out, float("nan"))
        kw.pop("window_size")
        ops.paged_attention_forward(q, plain, *args, **kw)
        assert torch.equal(out, plain)


# ---- cache offsets past 2^31 elements / 2^32 bytes -----------------------------------------------------------------------
_HIGH = {  # route -> B, H, Hkv, D, out_pad: Hkv * D = 1024, so a 64-slot block is 65536 elements
    "head": (4, 8, 8, 128, 4), "rows": (16, 16, 16, 64, 0), "gqa": (4, 16, 8, 128, 0),
}


@pytest.mark.parametrize("kv8", [False, True], ids=["kv16", "fp8"])
@pytest.mark.parametrize("route", ["head", "rows", "gqa"])
def test_decode_high_cache_offsets(route, kv8):
    """The sequences' blocks are the highest of a device cache so large that every one of them starts past 2^31 elements
    (16-bit) or 2^32 bytes (fp8); the blocks below are zeros."""
    ops = _ops()
    B, H, Hkv, D, out_pad = _HIGH[route]
    bs = 64
    ctxs = ([700, 0, 64, 65, 513, 1, 300, 33] * 2)[:B]
    case = dict(name=f"high-{route}", route=route, kv8=kv8, dtype=torch.bfloat16, bs=bs, left=-1, msl=1100, ctxs=ctxs,
                max_blocks=(1100 + bs - 1) // bs + 1, data="randn", needle=None, q_packed=False, out_pad=out_pad,
                equal_unwindowed=False, seed=77, B=B, H=H, Hkv=Hkv, D=D, q_len=1)
    gen = torch.Generator().manual_seed(case["seed"])
    qv, fill = dc.make_inputs(case, gen)
    ks, vs = (0.0123, 0.0391) if kv8 else (1.0, 1.0)
    cache_dtype = dc.F8 if kv8 else case["dtype"]
    kc, vc, bt, _ = dc.hostile_cache(ctxs, block_size=bs, Hkv=Hkv, D=D, L=1, layer=0, cache_dtype=cache_dtype, gen=gen,
                                     max_blocks=case["max_blocks"], fill=fill, k_scale=ks, v_scale=vs)
    t = dict(q=qv.to(case["dtype"]), ctx=torch.tensor(ctxs, dtype=torch.int32))
    block_elems = bs * Hkv * D
    shift = ((1 << 32) if kv8 else (1 << 31)) // block_elems + 1   # zero blocks in front of the small cache
    assert shift * block_elems * kc.element_size() > (1 << 32)
    nb = kc.shape[0]
    kcd = torch.zeros((shift + nb, 1, bs, Hkv, D), dtype=cache_dtype, device=DEV)
    vcd = torch.zeros((shift + nb, 1, bs, Hkv, D), dtype=cache_dtype, device=DEV)
    kcd[shift:] = kc.to(DEV)
    vcd[shift:] = vc.to(DEV)
    kw = dict(k_scale=torch.tensor([ks], dtype=torch.float32, device=DEV),
              v_scale=torch.tensor([vs], dtype=torch.float32, device=DEV)) if kv8 else {}
    q, buf, out = _device_inputs(case, t)
    args = (kcd, vcd, (bt + shift).to(DEV), t["ctx"].to(DEV), bs, case["msl"], 0)
    assert ops.paged_attention_route(q, out, *args, **kw) == route
    ops.paged_attention_forward(q, out, *args, **kw)
    torch.cuda.synchronize()
    ref, lse = dc.reference(t["q"], kc, vc, bt, t["ctx"], bs, 0, k_scale=ks, v_scale=vs)
    model_o = dc.model(t["q"], kc, vc, bt, t["ctx"], bs, 0, dtype=case["dtype"], p16=route == "gqa", k_scale=ks,
                       v_scale=vs)
    dc.check(out, ref, lse, case["dtype"], dc.family(case), model_o, case["name"])
    del kcd, vcd
    torch.cuda.empty_cache()


# ---- the workspace ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", dc.WORKSPACE_CASES, ids=lambda c: c["name"])
def test_decode_workspace_is_enough(case):
    """mio_fa3_decode_workspace_bytes() knows neither the kv head count, the block size nor the cache's element size: a
    launch given exactly that many bytes, in the middle of a patterned buffer, leaves the bytes around them untouched.  The
    bytes themselves hold 0xFF before the launch (NaN as fp32): whatever a launch merges, it has stored itself."""
    from mio import _lib
    ops = _ops()
    lib = _lib.lib
    t = dc.build_case(case)
    ref, lse, model_o = dc.case_reference(case, t)
    q, buf, out = _device_inputs(case, t)
    sc = _scales(case, t)
    tensors = (q, out, t["kc"].to(DEV), t["vc"].to(DEV), t["bt"].to(DEV), t["ctx"].to(DEV))
    assert ops.paged_attention_route(*tensors, case["bs"], case["msl"], dc.LAYER, window_size=(case["left"], -1),
                                     **sc) == case["route"]
    args, dt, kv8, keep = ops._decode_args(*tensors, case["bs"], case["msl"], dc.LAYER, None, sc.get("k_scale"),
                                           sc.get("v_scale"))
    assert kv8 == case["kv8"]
    nbytes = lib.mio_fa3_decode_workspace_bytes(case["B"], case["H"], case["q_len"], case["D"], case["msl"])
    guard = (nbytes + 255) // 256 * 256   # at least the region's size on either side: an overrun stays inside the buffer
    pattern = 0xA5
    work = torch.full((2 * guard + nbytes,), pattern, dtype=torch.uint8, device=DEV)
    work[guard:guard + nbytes] = 0xFF   # what the launch finds in its workspace: NaN as fp32 partials and lse
    ws = work.data_ptr() + guard
    assert ws % 16 == 0
    stream = ops._stream()
    if kv8:
        rc = lib.mio_fa3_decode_paged_kv8(*args, case["left"], dt, ws, stream)
    elif case["left"] >= 0:
        rc = lib.mio_fa3_decode_paged_window(*args, case["left"], -1, dt, ws, stream)
    else:
        rc = lib.mio_fa3_decode_paged(*args, dt, ws, stream)
    assert rc == 0, lib.mio_last_error().decode()
    torch.cuda.synchronize()
    del keep
    assert (work[:guard] == pattern).all(), "bytes in front of the workspace were written"
    assert (work[guard + nbytes:] == pattern).all(), "bytes behind the workspace were written"
    assert (work[guard:guard + nbytes] != 0xFF).any(), "the workspace interior did not change: the case has a single split"
    dc.check(out, ref, lse, case["dtype"], dc.family(case), model_o, case["name"], win=case["left"] >= 0)


def test_stats_cover_every_family():
    """Every (q dtype, route, cache kind) family has been judged with a window and without (run alone, this test runs
    the first case of each family itself).  The measured maxima are printed (-s shows them) in the layout of
    _decode_check's docstring table."""
    want = {(d, r, k, w) for d in (dc.BF, dc.FP) for r in ("head", "rows", "gqa") for k in ("kv16", "fp8")
            for w in (False, True)}
    for case in dc.CASES:
        if dc.family(case) + (case["left"] >= 0 and not case["equal_unwindowed"],) not in dc.STATS:
            test_decode_matrix(case)
    print("\n" + dc.stats_table())
    assert want <= set(dc.STATS), sorted(map(str, want - set(dc.STATS)))

"""Attention forward by kernel route and geometry, against the fp64 oracle (tests/_attn_check.py).

Every case first asserts ops.fa3_route(...) -- the kernel mio_fa3_fwd picks -- is the route it is meant to test, then
checks the result row by row with _attn_check.check at the bars of that (dtype, route).  Both storage dtypes throughout.
"""
import math

import pytest
import torch

import _attn_check as ac

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
LOG2E = 1.4426950408889634


def _ops():
    from mio import ops
    return ops


def _rand(shape, dtype, g):
    return torch.randn(*shape, generator=g).to(dtype)


def _unblock(ob, B, Sq, H, D):
    M = ob.shape[0]
    return ob.view(M // 256, H * D // 32, 256, 32).permute(0, 2, 1, 3).reshape(M, H * D)[:B * Sq].view(B, Sq, H, D)


def run_case(dtype, route, *, B=1, Sq=200, Sk=333, H=2, Hkv=None, D=64, causal=False, q_offset=0, k_offset=0,
             layout="bshd", keep=None, add=None, kpre=False, oblk=False, fused=False, out_strided=False, seed=0,
             ref_on_gpu=False, what=""):
    """One ops.fa3_fwd launch of the given geometry: route asserted, result checked.  keep / add: 4-D masks (CPU)."""
    ops = _ops()
    Hkv = H if Hkv is None else Hkv
    g = torch.Generator().manual_seed(seed * 7919 + Sq * 31 + Sk * 17 + D)
    if fused:  # q / k / v as strided views of one [B, S, 3 H D] projection output
        assert Sq == Sk and Hkv == H and layout == "bshd"
        buf = _rand((B, Sq, 3 * H * D), dtype, g).to(DEV)
        qg, kg, vg = (buf[..., i * H * D:(i + 1) * H * D].view(B, Sq, H, D) for i in range(3))
    else:
        shp = (lambda S, h: (B, S, h, D)) if layout == "bshd" else (lambda S, h: (B, h, S, D))
        qg, kg, vg = (_rand(shp(S, h), dtype, g).to(DEV) for S, h in ((Sq, H), (Sk, Hkv), (Sk, Hkv)))
    scale = 1.0 / math.sqrt(D)
    ref_scale = scale
    if kpre:  # K as the projection epilogue hands it over: K * scale * log2(e), rounded once; scores are then base 2
        kg = (kg.float() * (scale * LOG2E)).to(dtype)
        ref_scale = math.log(2.0)
    kw = dict(layout=layout, causal=causal, q_offset=q_offset, k_offset=k_offset, k_prescaled=kpre, out_blocked=oblk,
              keep_mask=None if keep is None else keep.to(DEV), additive_mask=None if add is None else add.to(DEV))
    out = None
    if out_strided:  # a non-contiguous output: every row of a wider buffer
        out = torch.empty(B, Sq, H, 2 * D, dtype=dtype, device=DEV)[..., D:]
    assert ops.fa3_route(qg, kg, vg, out=out, return_lse=not oblk, **kw) == route, what
    res = ops.fa3_fwd(qg, kg, vg, out=out, return_lse=not oblk, **kw)
    if oblk:
        o, lse = _unblock(res, B, Sq, H, D), None
    else:
        o, lse = res
        if out is not None:
            assert o.data_ptr() == out.data_ptr()
    if layout == "bhsd":
        o = o.permute(0, 2, 1, 3)
    rdev = DEV if ref_on_gpu else None
    src = (qg, kg, vg) if ref_on_gpu else (qg.cpu(), kg.cpu(), vg.cpu())
    ref, rlse = ac.reference(*src, layout=layout, causal=causal, softmax_scale=ref_scale, keep_mask=keep,
                             additive_mask=add, q_offset=q_offset, k_offset=k_offset, device=rdev)
    if not ref_on_gpu:
        o, lse = o.cpu(), (None if lse is None else lse.cpu())
    return ac.check(o, ref, dtype, route, lse, rlse, what)


# ---------------------------------------------------------------------------------------------------------------------
# head dims on every route that accepts them
# ---------------------------------------------------------------------------------------------------------------------
_DIMS = [8, 16, 40, 64, 72, 88, 96, 104, 120, 128]
_D_CASES = ([("fwd5", D, False) for D in (8, 16, 40, 64)] + [("fwd5_kpre", D, True) for D in (8, 16, 40, 64)]
            + [("fwd3_kpre", D, True) for D in (72, 88, 96)] + [("fwd3", D, False) for D in (72, 88, 96, 104, 120, 128)])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("route,D,kpre", _D_CASES)
@pytest.mark.parametrize("causal", [False, True])
def test_head_dims_pipelined(dtype, route, D, kpre, causal):
    run_case(dtype, route, D=D, kpre=kpre, causal=causal, Sq=200, Sk=333 if not causal else 200)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", _DIMS)
def test_head_dims_sequential(dtype, D):
    run_case(dtype, "fwd1", D=D, Sq=100, Sk=333, causal=(D % 16 == 0))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D,H,causal", [(64, 2, False), (64, 2, True), (40, 4, True), (64, 8, False)])
def test_blocked_output(dtype, D, H, causal):
    run_case(dtype, "fwd5_kpre_oblk", B=2, Sq=300, Sk=300, H=H, D=D, kpre=True, oblk=True, causal=causal)


# ---------------------------------------------------------------------------------------------------------------------
# sequence edges
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Sq", [1, 127, 128, 129, 255, 256, 257, 300])
@pytest.mark.parametrize("Sk", [1, 63, 64, 65, 333, -1])
@pytest.mark.parametrize("D", [64, 96])
def test_sequence_edges(dtype, Sq, Sk, D):
    Sk = Sq + 77 if Sk < 0 else Sk
    route = "fwd1" if Sq <= 128 else ("fwd5" if D == 64 else "fwd3")
    run_case(dtype, route, Sq=Sq, Sk=Sk, D=D, causal=(D == 96))


# ---------------------------------------------------------------------------------------------------------------------
# causal offsets: keys fully in the past, fully in the future, partial overlap
# ---------------------------------------------------------------------------------------------------------------------
_OFFS = [(200, 0), (0, 300), (64, 128), (37, 0), (0, 91)]
_CAUSAL_ROUTES = [("fwd5", 64, False, 300), ("fwd5_kpre", 64, True, 300), ("fwd3", 128, False, 300),
                  ("fwd3_kpre", 96, True, 300), ("fwd1", 64, False, 100), ("fwd1", 128, False, 128)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("route,D,kpre,Sq", _CAUSAL_ROUTES)
@pytest.mark.parametrize("q_off,k_off", _OFFS)
def test_causal_offsets(dtype, route, D, kpre, Sq, q_off, k_off):
    run_case(dtype, route, Sq=Sq, Sk=200, D=D, kpre=kpre, causal=True, q_offset=q_off, k_offset=k_off)


# ---------------------------------------------------------------------------------------------------------------------
# heads: GQA ratios 1 / 2 / 8, B*H a multiple of 8 (XCD remap) and not
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,H,Hkv", [(1, 8, 8), (2, 4, 2), (1, 8, 1), (3, 2, 1), (1, 3, 3), (3, 8, 1)])
@pytest.mark.parametrize("route,D,kpre,Sq", [("fwd5", 64, False, 257), ("fwd3", 96, False, 257), ("fwd1", 128, False, 77),
                                             ("fwd5_kpre", 64, True, 257)])
def test_heads(dtype, B, H, Hkv, route, D, kpre, Sq):
    run_case(dtype, route, B=B, H=H, Hkv=Hkv, D=D, kpre=kpre, Sq=Sq, Sk=190, causal=True)


# ---------------------------------------------------------------------------------------------------------------------
# layouts: head-major, fused q/k/v views, non-contiguous output
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("route,D,kpre,Sq", [("fwd5", 64, False, 300), ("fwd3", 128, False, 300), ("fwd1", 96, False, 100),
                                             ("fwd3_kpre", 80, True, 300)])
@pytest.mark.parametrize("form", ["bhsd", "fused", "out_strided"])
def test_layouts(dtype, route, D, kpre, Sq, form):
    run_case(dtype, route, B=2, H=3, D=D, kpre=kpre, Sq=Sq, Sk=Sq, causal=True, layout="bhsd" if form == "bhsd" else "bshd",
             fused=form == "fused", out_strided=form == "out_strided")


# ---------------------------------------------------------------------------------------------------------------------
# user masks (fa3_fwd_kernel)
# ---------------------------------------------------------------------------------------------------------------------
def _keep_shapes(B, H, S, g):
    """Every keep-mask shape flash_attention canonicalises, as (mask given, canonical 4-D)."""
    from mio.ops import _canon_mask4
    full = (torch.rand(B, H, S, S, generator=g) > 0.3).to(torch.uint8).to(DEV)  # on the device: expand() stays stride 0
    full[..., 0] = 1
    forms = [full[:, 0, 0, :], full[:, 0, :1, :], full[:, 0], full[:, :1], full,
             full[:, :1, :1, :].expand(B, H, S, S)]  # an expand()ed (stride-0) view
    return [(m, _canon_mask4(m)) for m in forms]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("S,D,causal", [(100, 64, False), (300, 96, True), (128, 128, False), (129, 64, True)])
def test_keep_masks(dtype, S, D, causal):
    ops = _ops()
    B, H = 2, 2
    g = torch.Generator().manual_seed(S + D)
    q, k, v = (_rand((B, S, H, D), dtype, g) for _ in range(3))
    for i, (m, m4) in enumerate(_keep_shapes(B, H, S, g)):
        qg, kg, vg = q.to(DEV), k.to(DEV), v.to(DEV)
        assert ops.fa3_route(qg, kg, vg, keep_mask=m4, causal=causal) == "fwd1_keep"
        o = ops.flash_attention(qg, kg, vg, m, causal)
        ref, rlse = ac.reference(q, k, v, keep_mask=m4, causal=causal)
        ac.check(o.cpu(), ref, dtype, "fwd1_keep", None, rlse, f"keep form {i} {tuple(m.shape)}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Sq,Sk,D", [(100, 100, 64), (300, 300, 96), (64, 200, 128), (257, 100, 64)])
@pytest.mark.parametrize("shape", ["b1qk", "11qk", "bhqk", "b11k_expanded"])
@pytest.mark.parametrize("causal", [False, True])
def test_additive_masks(dtype, Sq, Sk, D, shape, causal):
    B, H = 2, 2
    g = torch.Generator().manual_seed(Sq + Sk + D)
    if shape == "b11k_expanded":
        add = (torch.randn(B, 1, 1, Sk, generator=g) * 2).to(DEV).expand(B, H, Sq, Sk)  # stride-0 view on the device
    else:
        dims = {"b1qk": (B, 1, Sq, Sk), "11qk": (1, 1, Sq, Sk), "bhqk": (B, H, Sq, Sk)}[shape]
        add = torch.randn(*dims, generator=g) * 2
        add[..., ::5] = -1e4
    run_case(dtype, "fwd1_add", B=B, H=H, Sq=Sq, Sk=Sk, D=D, add=add, causal=causal)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [64, 128])
def test_keep_mask_cross(dtype, D):
    g = torch.Generator().manual_seed(D)
    keep = (torch.rand(2, 2, 150, 333, generator=g) > 0.5).to(torch.uint8)
    keep[:, :, 7] = 0  # a row with no kept key: the -1e9 fill averages every key
    run_case(dtype, "fwd1_keep", B=2, Sq=150, Sk=333, D=D, keep=keep)
    run_case(dtype, "fwd1_keep", B=2, Sq=150, Sk=333, D=D, keep=keep, causal=True)


# ---------------------------------------------------------------------------------------------------------------------
# the (o_acc, lse) carry across K splits, and attn_merge with an empty side
# ---------------------------------------------------------------------------------------------------------------------
def run_carry(dtype, route, splits, *, B=1, Sq=300, H=2, D=64, kpre=False, causal=False, add=None, q_offset=0, seed=0,
              what=""):
    ops = _ops()
    Sk = splits[-1]
    g = torch.Generator().manual_seed(seed + Sq + D + len(splits))
    q, k, v = _rand((B, Sq, H, D), dtype, g), _rand((B, Sk, H, D), dtype, g), _rand((B, Sk, H, D), dtype, g)
    scale, ref_scale = 1.0 / math.sqrt(D), 1.0 / math.sqrt(D)
    if kpre:
        k = (k.float() * (scale * LOG2E)).to(dtype)
        ref_scale = math.log(2.0)
    qg, kg, vg = q.to(DEV), k.to(DEV), v.to(DEV)
    acc = torch.empty(B, Sq, H, D, dtype=torch.float32, device=DEV)
    lse = torch.empty(B, H, Sq, dtype=torch.float32, device=DEV)
    out = torch.empty(B, Sq, H, D, dtype=dtype, device=DEV)
    lo = 0
    for i, hi in enumerate(splits):
        last = i == len(splits) - 1
        kw = dict(causal=causal, q_offset=q_offset, k_offset=lo, k_prescaled=kpre, o_acc=acc, lse=lse, carry_in=i > 0,
                  write_out=last, out=out if last else None,
                  additive_mask=None if add is None else add[..., lo:hi].to(DEV))
        assert ops.fa3_route(qg, kg[:, lo:hi], vg[:, lo:hi], **kw) == route, what
        ops.fa3_fwd(qg, kg[:, lo:hi], vg[:, lo:hi], **kw)
        lo = hi
    ref, rlse = ac.reference(q, k, v, causal=causal, softmax_scale=ref_scale, additive_mask=add, q_offset=q_offset)
    ac.check(out.cpu(), ref, dtype, route, lse.cpu(), rlse, what)
    ac.check(acc.cpu(), ref, dtype, route, None, rlse, what + " (fp32 carry)")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("route,D,kpre,Sq", [("fwd5_kpre_carry", 64, True, 300), ("fwd5_kpre_carry", 40, True, 129),
                                             ("fwd3", 96, False, 300), ("fwd3", 128, False, 257),
                                             ("fwd1", 64, False, 128), ("fwd1", 128, False, 33)])
@pytest.mark.parametrize("splits", [(130, 333), (64, 129, 400)])
@pytest.mark.parametrize("causal", [False, True])
def test_carry_splits(dtype, route, D, kpre, Sq, splits, causal):
    run_carry(dtype, route, splits, Sq=Sq, D=D, kpre=kpre, causal=causal, q_offset=splits[-1] - Sq if causal else 0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_attn_merge_empty_side(dtype):
    ops = _ops()
    B, Sq, H, D, Sk = 2, 150, 2, 64, 200
    g = torch.Generator().manual_seed(5)
    q, k, v = (_rand((B, S, H, D), dtype, g) for S in (Sq, Sk, Sk))
    _o, lse_full = ops.fa3_fwd(q.to(DEV), k.to(DEV), v.to(DEV), return_lse=True)
    acc = torch.empty(B, Sq, H, D, dtype=torch.float32, device=DEV)
    lse = torch.empty(B, H, Sq, dtype=torch.float32, device=DEV)
    ops.fa3_fwd(q.to(DEV), k.to(DEV), v.to(DEV), o_acc=acc, lse=lse, write_out=False)
    ref, rlse = ac.reference(q, k, v)
    empty_o = torch.zeros_like(acc)
    empty_l = torch.full_like(lse, float("-inf"))
    for real_first in (True, False):
        a_o, a_l = (acc.clone(), lse.clone()) if real_first else (empty_o.clone(), empty_l.clone())
        b_o, b_l = (empty_o, empty_l) if real_first else (acc, lse)
        out = torch.empty(B, Sq, H, D, dtype=dtype, device=DEV)
        ops.attn_merge(a_o, a_l, b_o, b_l, out=out)
        ac.check(out.cpu(), ref, dtype, "merge", a_l.cpu(), rlse, f"merge real_first={real_first}")
    # both sides empty: the empty state
    a_o, a_l = empty_o.clone(), empty_l.clone()
    out = torch.empty(B, Sq, H, D, dtype=dtype, device=DEV)
    ops.attn_merge(a_o, a_l, empty_o, empty_l, out=out)
    assert (out == 0).all() and (a_l == float("-inf")).all()


# ---------------------------------------------------------------------------------------------------------------------
# Sk == 0: nothing is read; the empty (or carried) state is written
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D,Sq", [(64, 300), (96, 300), (128, 64)])
def test_empty_keys(dtype, D, Sq):
    ops = _ops()
    g = torch.Generator().manual_seed(D)
    q = _rand((1, Sq, 2, D), dtype, g).to(DEV)
    kv = torch.empty(1, 0, 2, D, dtype=dtype, device=DEV)
    assert ops.fa3_route(q, kv, kv) == "fwd1"
    o, lse = ops.fa3_fwd(q, kv, kv, causal=True, return_lse=True)
    assert (o == 0).all() and (lse == float("-inf")).all()
    add = torch.zeros(1, 1, Sq, 0, device=DEV)
    o, lse = ops.fa3_fwd(q, kv, kv, additive_mask=add, return_lse=True)
    assert (o == 0).all() and (lse == float("-inf")).all()
    # a carried state passes through unchanged
    acc = torch.randn(1, Sq, 2, D, device=DEV)
    lse_in = torch.randn(1, 2, Sq, device=DEV)
    lse_in[0, 0, :5] = float("-inf")
    acc[0, :5, 0] = 0
    a2, l2 = acc.clone(), lse_in.clone()
    out = ops.fa3_fwd(q, kv, kv, o_acc=a2, lse=l2, carry_in=True)
    assert torch.allclose(a2, acc, rtol=1e-6, atol=0) and torch.allclose(l2, lse_in, rtol=1e-6, atol=1e-6)
    assert torch.equal(l2[0, 0, :5], lse_in[0, 0, :5]) and (out[0, :5, 0] == 0).all()
    assert torch.equal(out, acc.to(dtype))
    with pytest.raises(ValueError):
        ops.fa3_fwd(q, kv, kv, k_prescaled=True)


# ---------------------------------------------------------------------------------------------------------------------
# left padding and -inf / finfo.min additive masks
# ---------------------------------------------------------------------------------------------------------------------
_FILLS = {"-inf": float("-inf"), "f32min": torch.finfo(torch.float32).min, "bf16min": torch.finfo(torch.bfloat16).min}
_PADS = (0, 17, 64, 130, 200)  # the last sequence is masked entirely


def _pad_mask(fill, S=200, Sq=None):
    Sq = S if Sq is None else Sq
    add = torch.zeros(len(_PADS), 1, Sq, S)
    for b, p in enumerate(_PADS):
        add[b, :, :, :p] = fill
    return add


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fill", list(_FILLS))
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D,Sq", [(64, 200), (96, 200), (128, 100)])
def test_left_padding_fa3_fwd(dtype, fill, causal, D, Sq):
    add = _pad_mask(_FILLS[fill], Sq=Sq)
    run_case(dtype, "fwd1_add", B=len(_PADS), H=2, Sq=Sq, Sk=200, D=D, add=add, causal=causal,
             what=f"left padding {fill}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fill", list(_FILLS))
def test_left_padding_ring_attention(dtype, fill):
    ops = _ops()
    B, H, S, D = len(_PADS), 2, 200, 64
    g = torch.Generator().manual_seed(11)
    q, k, v = (_rand((B, H, S, D), dtype, g) for _ in range(3))
    add = _pad_mask(_FILLS[fill])
    assert ops.fa3_route(q.to(DEV), k.to(DEV), v.to(DEV), layout="bhsd", additive_mask=add.to(DEV)) == "fwd1_add"
    o = ops.ring_attention_forward(q.to(DEV), k.to(DEV), v.to(DEV), add.to(DEV))
    ref, rlse = ac.reference(q, k, v, layout="bhsd", additive_mask=add)
    ac.check(o.view(B, S, H, D).cpu(), ref, dtype, "fwd1_add", None, rlse, f"ring left padding {fill}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fill", list(_FILLS))
@pytest.mark.parametrize("causal", [False, True])
def test_left_padding_two_shard_carry(dtype, fill, causal):
    """Shard 1 (keys 0 .. 99) is fully masked for the sequences padded by 100 and 130 tokens.  A row masked in every shard
    is only required to stay finite and inside the range of V across a carry: the lse of a fully masked shard sits at the
    -1e30 floor, where neither fp32 nor fp64 resolves the log(n) that would weigh the shards for an exact uniform average."""
    pads = (0, 17, 64, 100, 130)
    fillv = _FILLS[fill]
    add = torch.zeros(len(pads), 1, 100, 200)
    for b, p in enumerate(pads):
        add[b, :, :, :p] = fillv
    run_carry(dtype, "fwd1_add", (100, 200), B=len(pads), Sq=100, D=64, causal=causal, add=add,
              q_offset=100 if causal else 0, what=f"two-shard left padding {fill}")
    ops = _ops()
    g = torch.Generator().manual_seed(3)
    q, k, v = (_rand((1, S, 2, 64), dtype, g).to(DEV) for S in (100, 200, 200))
    full = torch.full((1, 1, 100, 200), fillv, device=DEV)
    acc = torch.empty(1, 100, 2, 64, device=DEV)
    lse = torch.empty(1, 2, 100, device=DEV)
    ops.fa3_fwd(q, k[:, :100], v[:, :100], additive_mask=full[..., :100], causal=causal, q_offset=100 if causal else 0,
                o_acc=acc, lse=lse, write_out=False)
    out = ops.fa3_fwd(q, k[:, 100:], v[:, 100:], additive_mask=full[..., 100:], causal=causal, q_offset=100 if causal else 0,
                      k_offset=100, o_acc=acc, lse=lse, carry_in=True)
    assert torch.isfinite(out).all() and torch.isfinite(lse).all()
    vf = v.float()
    assert (out.float() >= vf.amin(dim=1, keepdim=True) - 1e-2).all() and (out.float() <= vf.amax(dim=1, keepdim=True) + 1e-2).all()


# ---------------------------------------------------------------------------------------------------------------------
# a few large shapes (reference in float64 on the GPU)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("route,D,kpre,causal", [("fwd5", 64, False, True), ("fwd5_kpre", 64, True, False),
                                                 ("fwd3", 128, False, True), ("fwd3_kpre", 96, True, True)])
def test_large(dtype, route, D, kpre, causal):
    run_case(dtype, route, B=2, H=8, Hkv=2, Sq=2048, Sk=2048, D=D, kpre=kpre, causal=causal, ref_on_gpu=True)

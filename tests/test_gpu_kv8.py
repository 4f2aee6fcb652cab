"""FP8 (e4m3fn) paged KV cache on the GPU: quantising cache writes (ops.reshape_and_cache / reshape_and_cache_varlen with
k_scale / v_scale) and decode over the fp8 cache (ops.paged_attention_forward, mio_fa3_decode_paged_kv8).

Writes must equal the CPU formula (x.float() * (1 / scale)).clamp(-448, 448).to(float8_e4m3fn) byte for byte and leave
skipped positions untouched.  Decode is compared with an fp64 reference over the dequantised cache (K = k8 * k_scale,
V = v8 * v_scale) at the bars of the 16-bit decode tests, each case asserting its kernel.  On a library without the fp8
entry points every test fails at the symbol check, before an fp8 cache reaches any launch.
"""
import pytest
import torch

import _decode_check as dc

pytestmark = pytest.mark.gpu

DEV = "cuda"
F8 = torch.float8_e4m3fn
TOL = {torch.float16: (1e-3, 4e-3), torch.bfloat16: (3e-3, 2e-2)}
KV8_SYMBOLS = ("mio_reshape_and_cache_kv8", "mio_reshape_and_cache_varlen_kv8", "mio_fa3_decode_paged_kv8",
               "mio_fa3_decode_kv8_route")


@pytest.fixture(autouse=True)
def _kv8_symbols():
    # an older library would take an fp8 cache into the 16-bit write kernel (out of bounds): nothing fp8 runs without these
    from mio import _lib
    missing = [s for s in KV8_SYMBOLS if not hasattr(_lib.lib, s)]
    assert not missing, f"fp8 KV-cache entry points missing from the library: {missing}"


def _ops():
    from mio import ops
    return ops


def _quant_ref(x, s):
    """The cache-write formula on the CPU: x [..] 16-bit, s a python float (the fp32 scale)."""
    return (x.float() * (torch.tensor(1.0) / torch.tensor(s, dtype=torch.float32))).clamp(-448, 448).to(F8)


def _bytes(t):
    return t.cpu().view(torch.uint8)


# ---- cache writes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("per_layer", [False, True])
def test_kv8_write_varlen_byte_exact(dtype, per_layer):
    """Every 16-bit bit pattern (NaN, inf, subnormals, values far beyond 448 * scale) through the varlen write, with a
    sequence tail past its block-table row (skipped); layer 1 of 3."""
    ops = _ops()
    g = torch.Generator().manual_seed(11 + per_layer)
    Hkv, D, L, bs, layer = 2, 128, 3, 16, 1
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    key = bits.view(dtype).view(256, Hkv, D)                    # all 65536 values
    value = key[torch.randperm(256, generator=g)].contiguous()   # the same values, other rows
    scales = [0.37, 2.5, 1.0] if per_layer else [0.37]
    vscales = [1.75, 0.0625, 3.0] if per_layer else [1.75]
    ks = torch.tensor(scales, dtype=torch.float32, device=DEV)
    vs = torch.tensor(vscales, dtype=torch.float32, device=DEV)
    # 3 sequences of 100, 120 and 36 new tokens; seq 2 ends at 160, past its 9 * 16 = 144-key table row: its positions
    # 144 .. 159 are skipped
    maxb, nb = 9, 40
    bt = torch.randperm(nb, generator=g)[:3 * maxb].view(3, maxb).to(torch.int32)
    cu = torch.tensor([0, 100, 220, 256], dtype=torch.int32)
    ctx_t = torch.tensor([130, 120, 160], dtype=torch.int32)
    sentinel = 0x5A
    kc = torch.full((nb, L, bs, Hkv, D), sentinel, dtype=torch.uint8).view(F8)
    vc = kc.clone()
    kc_d, vc_d = kc.to(DEV), vc.to(DEV)
    ops.reshape_and_cache_varlen(key.to(DEV), value.to(DEV), kc_d, vc_d, bt.to(DEV), cu.to(DEV), ctx_t.to(DEV), bs,
                                 layer, k_scale=ks, v_scale=vs)
    torch.cuda.synchronize()
    ls = scales[layer] if per_layer else scales[0]
    lvs = vscales[layer] if per_layer else vscales[0]
    kref, vref = kc.clone(), vc.clone()
    for b in range(3):
        n = int(cu[b + 1] - cu[b])
        for i in range(n):
            pos = int(ctx_t[b]) - n + i
            if pos < 0 or pos // bs >= maxb:
                continue
            blk = int(bt[b, pos // bs])
            t = int(cu[b]) + i
            kref[blk, layer, pos % bs] = _quant_ref(key[t], ls)
            vref[blk, layer, pos % bs] = _quant_ref(value[t], lvs)
    got_k, got_v = _bytes(kc_d), _bytes(vc_d)
    assert torch.equal(got_k, _bytes(kref)), (got_k != _bytes(kref)).nonzero()[:8]
    assert torch.equal(got_v, _bytes(vref)), (got_v != _bytes(vref)).nonzero()[:8]
    # the skipped tail of seq 2 and the other layers kept the sentinel
    assert (got_k.view(nb, L, -1)[:, [0, 2]] == sentinel).all()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("per_layer", [False, True])
def test_kv8_write_one_token_byte_exact(dtype, per_layer):
    ops = _ops()
    g = torch.Generator().manual_seed(3 + per_layer)
    B, Hkv, D, L, bs, layer = 6, 4, 64, 2, 16, 1
    key = (torch.randn(B, 1, Hkv, D, generator=g) * 300).to(dtype)   # well past 448 * scale
    value = (torch.randn(B, 1, Hkv, D, generator=g) * 0.01).to(dtype)  # down into the e4m3 subnormals
    key[0, 0, 0, :4] = torch.tensor([float("nan"), float("inf"), -float("inf"), -0.0]).to(dtype)
    ks = torch.tensor([0.5, 0.8] if per_layer else [0.8], dtype=torch.float32, device=DEV)
    vs = torch.tensor([2.0, 0.03] if per_layer else [0.03], dtype=torch.float32, device=DEV)
    maxb = 4
    nb = B * maxb + 1
    bt = torch.randperm(nb, generator=g)[:B * maxb].view(B, maxb).to(torch.int32)
    ctx = torch.tensor([1, 17, 0, 64, 65, 40], dtype=torch.int32)  # 0: nothing; 65: past the table row (skipped)
    sentinel = 0x33
    kc = torch.full((nb, L, bs, Hkv, D), sentinel, dtype=torch.uint8).view(F8)
    kc_d, vc_d = kc.to(DEV), kc.clone().to(DEV)
    ops.reshape_and_cache(key.to(DEV), value.to(DEV), kc_d, vc_d, bt.to(DEV), ctx.to(DEV), bs, layer, k_scale=ks,
                          v_scale=vs)
    torch.cuda.synchronize()
    kref, vref = kc.clone(), kc.clone()
    for b in range(B):
        pos = int(ctx[b]) - 1
        if pos < 0 or pos // bs >= maxb:
            continue
        blk = int(bt[b, pos // bs])
        kref[blk, layer, pos % bs] = _quant_ref(key[b, 0], float(ks[-1 if not per_layer else layer]))
        vref[blk, layer, pos % bs] = _quant_ref(value[b, 0], float(vs[-1 if not per_layer else layer]))
    assert torch.equal(_bytes(kc_d), _bytes(kref))
    assert torch.equal(_bytes(vc_d), _bytes(vref))
    assert _bytes(kc_d)[..., 0].ne(sentinel).sum() > 0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("kv8", [False, True])
@pytest.mark.parametrize("Hkv,D", [(2, 16), (40, 128)])
def test_write_forms_share_the_chunk_store(dtype, kv8, Hkv, D):
    """The single-token write and the varlen write of one new token per sequence leave byte-identical caches, 16-bit and fp8:
    both go through the one chunk store of csrc/cache_write.hip.  (2, 16) is the smallest fp8 chunk; (40, 128) is 640 16-bit /
    320 fp8 chunks per token, more than one pass of the single-token kernel's 256 threads in both cache kinds.  K and V are
    strided views into one fused projection; sequence 3 is empty and sequence 4's position is past its table row: neither
    writes.  All comparisons are exact: the source bits for a 16-bit cache, _quant_ref for fp8."""
    ops = _ops()
    g = torch.Generator().manual_seed(7)
    B, bs, L, layer, maxb, H = 5, 16, 2, 1, 4, 2 * Hkv
    ctx = torch.tensor([1, 16, 17, 0, 65], dtype=torch.int32)  # lengths after the append
    qkv = (torch.randn(B, (H + 2 * Hkv) * D, generator=g) * 100).to(dtype)
    key = qkv[:, H * D:(H + Hkv) * D].view(B, Hkv, D)
    value = qkv[:, (H + Hkv) * D:].view(B, Hkv, D)
    nb = B * maxb + 3
    bt = torch.randperm(nb, generator=g)[:B * maxb].view(B, maxb).to(torch.int32)
    cu = torch.arange(B + 1, dtype=torch.int32)
    scales = dict(k_scale=torch.tensor([0.5, 0.37], device=DEV), v_scale=torch.tensor([2.0, 1.75], device=DEV)) if kv8 else {}
    sentinel = torch.full((nb, L, bs, Hkv, D * (1 if kv8 else 2)), 0x5A, dtype=torch.uint8).view(F8 if kv8 else dtype)
    qkv_d = qkv.to(DEV)
    key_d = qkv_d[:, H * D:(H + Hkv) * D].view(B, Hkv, D)
    value_d = qkv_d[:, (H + Hkv) * D:].view(B, Hkv, D)
    one = [sentinel.to(DEV), sentinel.to(DEV)]
    var = [sentinel.to(DEV), sentinel.to(DEV)]
    ops.reshape_and_cache(key_d[:, None], value_d[:, None], *one, bt.to(DEV), ctx.to(DEV), bs, layer, **scales)
    ops.reshape_and_cache_varlen(key_d, value_d, *var, bt.to(DEV), cu.to(DEV), ctx.to(DEV), bs, layer, **scales)
    torch.cuda.synchronize()
    ref = [sentinel.clone(), sentinel.clone()]
    written = torch.zeros(nb, L, bs, dtype=torch.bool)
    for b in range(B):
        pos = int(ctx[b]) - 1
        if pos < 0 or pos // bs >= maxb:
            continue
        row = (int(bt[b, pos // bs]), layer, pos % bs)
        written[row] = True
        ref[0][row] = _quant_ref(key[b], 0.37) if kv8 else key[b]
        ref[1][row] = _quant_ref(value[b], 1.75) if kv8 else value[b]
    assert written.sum() == 3
    for what, a, v, r in zip("KV", one, var, ref):
        a, v, r = _bytes(a), _bytes(v), _bytes(r)
        assert torch.equal(a, v), (what, (a != v).nonzero()[:8])            # the two forms, byte for byte
        assert (a[~written] == 0x5A).all() and (v[~written] == 0x5A).all(), what  # nothing outside the written rows of the layer
        assert torch.equal(a[written], r[written]), (what, (a != r).nonzero()[:8])  # the written rows: the reference's bytes


# ---- decode -----------------------------------------------------------------------------------------------------------------
def _judge(out, q, kc, vc, ks, vs, bt, ctx, bs, layer, left, dtype, route, what):
    """The decode result against _decode_check's fp64 reference over the dequantised cache (windowed when left >= 0):
    the whole-tensor bars of the 16-bit decode tests, then the per-row check against the fp32 model."""
    kw = dict(left=left, k_scale=ks, v_scale=vs)
    ref, lse = dc.reference(q, kc, vc, bt, ctx, bs, layer, **kw)
    _cmp(out, ref, dtype, what)
    model_o = dc.model(q, kc, vc, bt, ctx, bs, layer, dtype=dtype, p16=route == "gqa", **kw)
    dc.check(out, ref, lse, dtype, (dtype, route, "fp8"), model_o, what, win=left >= 0)


def _cmp(got, ref, dtype, what, tol=None):
    ref = ref.to(dtype).float()
    got = got.float().cpu()
    rel = ((got - ref).abs().mean() / ref.abs().mean().clamp_min(1e-12)).item()
    mx = (got - ref).abs().max().item()
    rtol, atol = tol or TOL[dtype]
    assert rel < rtol and mx < atol * max(1.0, ref.abs().max().item()), f"{what}: rel_err={rel:.3e} max={mx:.3e}"


def _f8_cache(ctxs, *, bs, Hkv, D, L, g):
    maxb = max((max(ctxs) + bs - 1) // bs, 1) + 1
    nb = len(ctxs) * maxb + 2
    kc = (torch.randn(nb, L, bs, Hkv, D, generator=g) * 3).to(F8)
    vc = (torch.randn(nb, L, bs, Hkv, D, generator=g) * 3).to(F8)
    bt = torch.randperm(nb, generator=g)[:len(ctxs) * maxb].view(len(ctxs), maxb).to(torch.int32)
    return kc, vc, bt


# (H, Hkv, D, B) per route: per-head (D 80 / 96), whole token rows (MHA, B >= 16, q_len 1), matrix core (GQA).  At D 128 one
# query vector per key also goes to the matrix core; its rows form runs when the output rows are not 16-byte aligned.
_GEOMS = {
    ("head", 80): (4, 2, 80, 5), ("head", 96): (6, 3, 96, 5),
    ("rows", 64): (8, 8, 64, 16), ("rows", 128): (4, 4, 128, 16),
    ("gqa", 64): (8, 2, 64, 5), ("gqa", 128): (8, 2, 128, 5),
}


@pytest.mark.parametrize("route,D", sorted(_GEOMS))
@pytest.mark.parametrize("q_len", [1, 3])
@pytest.mark.parametrize("bs", [16, 64])
@pytest.mark.parametrize("left", [-1, 37])
def test_kv8_decode_matches_reference(route, D, q_len, bs, left):
    ops = _ops()
    H, Hkv, D, B = _GEOMS[(route, D)]
    want = route
    if route == "rows" and q_len > 1:  # several query vectors per key: matrix core, or per head on unaligned output rows
        want = "head" if D == 128 else "gqa"
    dtype = torch.bfloat16 if bs == 16 else torch.float16
    g = torch.Generator().manual_seed(D * 7 + q_len * 3 + bs + (left > 0))
    L, layer = 2, 1
    ctxs = ([0, 1, 300, 1037, 64] * 4)[:B]
    kc, vc, bt = _f8_cache(ctxs, bs=bs, Hkv=Hkv, D=D, L=L, g=g)
    ks = torch.tensor([0.9, 0.21], dtype=torch.float32)
    vs = torch.tensor([1.3, 0.47], dtype=torch.float32)
    q = torch.randn(B, H, q_len, D, generator=g).to(dtype)
    ctx = torch.tensor(ctxs, dtype=torch.int32)
    pad = 4 if (route, D) == ("rows", 128) else 0  # output rows 4 elements apart from 16-byte alignment: not gqa
    out = torch.full((B, H, q_len, D + pad), float("nan"), dtype=dtype, device=DEV)[..., :D]
    args = (q.to(DEV), out, kc.to(DEV), vc.to(DEV), bt.to(DEV), ctx.to(DEV), bs, max(ctxs), layer)
    kw = dict(window_size=(left, -1), k_scale=ks.to(DEV), v_scale=vs.to(DEV))
    assert ops.paged_attention_route(*args, **kw) == want
    ops.paged_attention_forward(*args, **kw)
    _judge(out, q, kc, vc, float(ks[layer]), float(vs[layer]), bt, ctx, bs, layer, left, dtype, want,
           f"{want} D{D} q_len{q_len} bs{bs} left{left}")


@pytest.mark.parametrize("route", ["head", "rows", "gqa"])
def test_kv8_decode_shared_scale_and_splits(route):
    """One shared scale pair, long contexts (several splits merged by decode_reduce_kernel), bf16."""
    ops = _ops()
    H, Hkv, D, B = {"head": (4, 2, 80, 3), "rows": (16, 16, 64, 16), "gqa": (16, 2, 128, 3)}[route]
    g = torch.Generator().manual_seed(77)
    bs, L, layer = 16, 3, 2
    ctxs = ([4000, 2500, 1] * 6)[:B]
    kc, vc, bt = _f8_cache(ctxs, bs=bs, Hkv=Hkv, D=D, L=L, g=g)
    ks, vs = torch.tensor([0.33]), torch.tensor([2.0])
    q = torch.randn(B, H, 1, D, generator=g).to(torch.bfloat16)
    ctx = torch.tensor(ctxs, dtype=torch.int32)
    out = torch.empty(B, H, 1, D, dtype=torch.bfloat16, device=DEV)
    args = (q.to(DEV), out, kc.to(DEV), vc.to(DEV), bt.to(DEV), ctx.to(DEV), bs, max(ctxs), layer)
    kw = dict(k_scale=ks.to(DEV), v_scale=vs.to(DEV))
    assert ops.paged_attention_route(*args, **kw) == route
    ops.paged_attention_forward(*args, **kw)
    _judge(out, q, kc, vc, float(ks[0]), float(vs[0]), bt, ctx, bs, layer, -1, torch.bfloat16, route, route)


@pytest.mark.parametrize("route", ["head", "rows", "gqa"])
def test_kv8_write_then_decode_round_trip(route):
    """bf16 K/V written into an fp8 cache and decoded: within 5e-2 relative of the same decode over a bf16 cache."""
    ops = _ops()
    H, Hkv, D, B = {"head": (4, 2, 96, 4), "rows": (8, 8, 64, 16), "gqa": (8, 2, 64, 4)}[route]
    g = torch.Generator().manual_seed(5)
    bs, L, layer = 16, 2, 1
    ctxs = ([700, 33, 1, 250] * 4)[:B]
    T = sum(ctxs)
    k = torch.randn(T, Hkv, D, generator=g).to(torch.bfloat16)
    v = torch.randn(T, Hkv, D, generator=g).to(torch.bfloat16)
    maxb = (max(ctxs) + bs - 1) // bs
    nb = B * maxb
    bt = torch.randperm(nb, generator=g).view(B, maxb).to(torch.int32).to(DEV)
    cu = torch.tensor([0] + list(torch.tensor(ctxs).cumsum(0)), dtype=torch.int32, device=DEV)
    ctx = torch.tensor(ctxs, dtype=torch.int32, device=DEV)
    ks = torch.tensor([1.0, k.float().abs().max().item() / 448], dtype=torch.float32, device=DEV)
    vs = torch.tensor([1.0, v.float().abs().max().item() / 448], dtype=torch.float32, device=DEV)
    c16 = [torch.zeros(nb, L, bs, Hkv, D, dtype=torch.bfloat16, device=DEV) for _ in range(2)]
    c8 = [torch.zeros(nb, L, bs, Hkv, D, dtype=F8, device=DEV) for _ in range(2)]
    ops.reshape_and_cache_varlen(k.to(DEV), v.to(DEV), *c16, bt, cu, ctx, bs, layer)
    ops.reshape_and_cache_varlen(k.to(DEV), v.to(DEV), *c8, bt, cu, ctx, bs, layer, k_scale=ks, v_scale=vs)
    q = torch.randn(B, H, 1, D, generator=g).to(torch.bfloat16).to(DEV)
    o16 = torch.empty_like(q)
    o8 = torch.empty_like(q)
    ops.paged_attention_forward(q, o16, *c16, bt, ctx, bs, max(ctxs), layer)
    kw = dict(k_scale=ks, v_scale=vs)
    assert ops.paged_attention_route(q, o8, *c8, bt, ctx, bs, max(ctxs), layer, **kw) == route
    ops.paged_attention_forward(q, o8, *c8, bt, ctx, bs, max(ctxs), layer, **kw)
    rel = ((o8.float() - o16.float()).abs().mean() / o16.float().abs().mean()).item()
    assert rel < 5e-2, rel


# ---- routes and refusals -----------------------------------------------------------------------------------------------------
_CASES = {  # the benchmark cases (tools/kv8_bench.py): (H, Hkv, D, B, ctx, bs, left) -> route
    "a": ((16, 16, 64, 64, 4096, 16, -1), "rows"),
    "b": ((32, 4, 128, 64, 4096, 16, -1), "gqa"),
    "c": ((32, 8, 128, 8, 32768, 64, -1), "gqa"),
    "d": ((16, 16, 64, 8, 4096, 16, -1), "head"),
    "b_win": ((32, 4, 128, 64, 32768, 16, 4095), "gqa"),
}


@pytest.mark.parametrize("case", sorted(_CASES))
def test_kv8_ops_route_cases(case):
    ops = _ops()
    (H, Hkv, D, B, ctx, bs, left), want = _CASES[case]
    q = torch.zeros(B, H, 1, D, dtype=torch.bfloat16, device=DEV)
    kc = torch.zeros(2, 1, bs, Hkv, D, dtype=F8, device=DEV)  # the route reads no cache: two pages stand for all
    bt = torch.zeros(B, (ctx + bs - 1) // bs, dtype=torch.int32, device=DEV)
    cl = torch.full((B,), ctx, dtype=torch.int32, device=DEV)
    one = torch.ones(1, dtype=torch.float32, device=DEV)
    assert ops.paged_attention_route(q, q, kc, kc, bt, cl, bs, ctx, 0, window_size=(left, -1), k_scale=one,
                                     v_scale=one) == want


def _decode_setup(D=64, L=2):
    q = torch.zeros(2, 4, 1, D, dtype=torch.bfloat16, device=DEV)
    kc = torch.zeros(4, L, 16, 2, D, dtype=F8, device=DEV)
    bt = torch.zeros(2, 2, dtype=torch.int32, device=DEV)
    cl = torch.full((2,), 20, dtype=torch.int32, device=DEV)
    return q, kc, bt, cl


def test_kv8_ops_refusals():
    ops = _ops()
    one = torch.ones(1, dtype=torch.float32, device=DEV)
    q, kc, bt, cl = _decode_setup()
    out = torch.empty_like(q)
    for fn in (ops.paged_attention_forward, ops.paged_attention_route):
        call = lambda kc_=kc, D=64, **kw: fn(q if D == 64 else torch.zeros(2, 4, 1, D, dtype=torch.bfloat16, device=DEV),
                                            out if D == 64 else torch.zeros(2, 4, 1, D, dtype=torch.bfloat16, device=DEV),
                                            kc_, kc_, bt, cl, 16, 20, 0, **kw)
        with pytest.raises(ValueError, match="requires k_scale and v_scale"):
            call()
        with pytest.raises(ValueError, match="requires k_scale and v_scale"):
            call(k_scale=one)
        with pytest.raises(ValueError, match="float32"):
            call(k_scale=one.double(), v_scale=one)
        with pytest.raises(ValueError, match="num_layers"):
            call(k_scale=torch.ones(3, device=DEV), v_scale=one)
        with pytest.raises(ValueError, match="device"):
            call(k_scale=one.cpu(), v_scale=one)
        c16 = torch.zeros(4, 2, 16, 2, 64, dtype=torch.bfloat16, device=DEV)
        with pytest.raises(ValueError, match="fp8"):
            call(kc_=c16, k_scale=one, v_scale=one)
        for bad in (torch.float8_e5m2, torch.float8_e4m3fnuz, torch.int8, torch.uint8):
            with pytest.raises(ValueError, match="float8_e4m3fn"):
                call(kc_=kc.view(bad), k_scale=one, v_scale=one)
        k72 = torch.zeros(4, 2, 16, 2, 72, dtype=F8, device=DEV)
        with pytest.raises(ValueError, match="head_dim"):
            call(kc_=k72, D=72, k_scale=one, v_scale=one)
    # cache writes
    key = torch.zeros(2, 1, 2, 64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError, match="requires k_scale and v_scale"):
        ops.reshape_and_cache(key, key, kc, kc, bt, cl, 16, 0)
    with pytest.raises(ValueError, match="fp8"):
        c16 = torch.zeros(4, 2, 16, 2, 64, dtype=torch.bfloat16, device=DEV)
        ops.reshape_and_cache(key, key, c16, c16, bt, cl, 16, 0, k_scale=one, v_scale=one)
    with pytest.raises(ValueError, match="float8_e4m3fn"):
        ops.reshape_and_cache(key, key, kc.view(torch.float8_e5m2), kc.view(torch.float8_e5m2), bt, cl, 16, 0,
                              k_scale=one, v_scale=one)
    with pytest.raises(ValueError, match="contiguous"):
        kt = torch.zeros(4, 2, 16, 64, 2, dtype=F8, device=DEV).transpose(3, 4)
        ops.reshape_and_cache(key, key, kt, kt, bt, cl, 16, 0, k_scale=one, v_scale=one)
    kv = torch.zeros(3, 2, 64, dtype=torch.bfloat16, device=DEV)
    cu = torch.tensor([0, 1, 3], dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="requires k_scale and v_scale"):
        ops.reshape_and_cache_varlen(kv, kv, kc, kc, bt, cu, cl, 16, 0)
    with pytest.raises(ValueError, match="num_layers"):
        ops.reshape_and_cache_varlen(kv, kv, kc, kc, bt, cu, cl, 16, 0, k_scale=torch.ones(5, device=DEV), v_scale=one)
    # prefill over the paged cache does not read fp8
    qp = torch.zeros(3, 4, 64, dtype=torch.bfloat16, device=DEV)
    k64 = torch.zeros(4, 1, 64, 2, 64, dtype=F8, device=DEV)
    with pytest.raises(ValueError, match="fp8"):
        ops.flash_attention_varlen_paged(qp, k64, k64, bt, cu, cl, 2, 20)


def test_reshape_and_cache_checks_cache_dtype():
    """A bf16 key into an fp16 cache (the same bytes per element: the old one-token write copied it as garbage) and a
    non-contiguous cache are refused before any launch."""
    ops = _ops()
    key = torch.randn(2, 1, 2, 64, device=DEV).to(torch.bfloat16)
    kc = torch.zeros(4, 1, 16, 2, 64, dtype=torch.float16, device=DEV)
    bt = torch.zeros(2, 2, dtype=torch.int32, device=DEV)
    cl = torch.full((2,), 5, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="share a dtype"):
        ops.reshape_and_cache(key, key, kc, kc, bt, cl, 16, 0)
    with pytest.raises(ValueError, match="share a dtype"):
        ops.reshape_and_cache(key, key.half(), kc, kc, bt, cl, 16, 0)
    kt = torch.zeros(4, 1, 16, 64, 2, dtype=torch.bfloat16, device=DEV).transpose(3, 4)
    with pytest.raises(ValueError, match="contiguous"):
        ops.reshape_and_cache(key, key, kt, kt, bt, cl, 16, 0)
    assert (kc == 0).all()


# ---- modules -------------------------------------------------------------------------------------------------------------
def test_kv8_paged_module_matches_ops_composition():
    """FlashAttentionLayer's paged forward over an fp8 PagedKVCache equals q_proj -> paged_attention_forward(k_scale,
    v_scale) -> o_proj done through ops; without the scales it is refused."""
    from mio._nn import CastCache, compute_dtype, linear
    from mio.baseline.inference import PagedKVCache
    from mio.kernels.attention.flash_attention import FlashAttentionLayer
    ops = _ops()
    torch.manual_seed(9)
    hidden, H, Hkv, L, bs, layer = 256, 4, 2, 2, 16, 1
    D = hidden // H
    pc = PagedKVCache(num_blocks=32, block_size=bs, num_layers=L, num_heads=Hkv, head_dim=D, dtype=F8, device=DEV)
    k_scale, v_scale = pc.get_kv_scales()
    assert k_scale.dtype == torch.float32 and k_scale.shape == (L,) and (k_scale == 1).all() and k_scale.is_cuda
    assert pc.get_physical_caches()[0].dtype == F8
    k_scale[layer], v_scale[layer] = 0.02, 0.03
    kc, vc = pc.get_physical_caches()
    lens = [40, 7, 100]
    for s, n in enumerate(lens):
        pc.allocate_blocks_for_sequence(s, n)
    bt, cl, mx = pc.kernel_metadata(range(len(lens)))
    T = sum(lens)
    cu = torch.tensor([0, 40, 47, 147], dtype=torch.int32, device=DEV)
    k = torch.randn(T, Hkv, D, device=DEV).to(torch.float16)
    v = torch.randn(T, Hkv, D, device=DEV).to(torch.float16)
    ops.reshape_and_cache_varlen(k, v, kc, vc, bt, cu, cl, bs, layer, k_scale=k_scale, v_scale=v_scale)
    mod = FlashAttentionLayer(hidden, H, num_kv_heads=Hkv).to(DEV, torch.float16)
    x = torch.randn(3, 1, hidden, device=DEV).to(torch.float16)
    kw = dict(physical_kv_cache_k=kc, physical_kv_cache_v=vc, block_tables=bt, context_lengths=cl, kv_cache_block_size=bs,
              max_seq_len=mx, layer_idx=layer)
    with torch.no_grad():
        y = mod(x, k_scale=k_scale, v_scale=v_scale, **kw)
        with pytest.raises(ValueError, match="k_scale"):
            mod(x, **kw)
        dt = compute_dtype(mod.config.precision, x)
        c = CastCache()
        q = linear(x, mod.q_proj, c, dt).view(3, 1, H, D).permute(0, 2, 1, 3)
        o = torch.empty(3, 1, H, D, dtype=dt, device=DEV)
        ops.paged_attention_forward(q, o.permute(0, 2, 1, 3), kc, vc, bt, cl, bs, mx, layer, k_scale=k_scale,
                                    v_scale=v_scale)
        ref = linear(o.view(3, 1, hidden), mod.o_proj, c, dt)
    assert torch.equal(y, ref.to(y.dtype))
    assert pc.get_memory_usage()["total_physical_memory_mb"] == 2 * 32 * L * bs * Hkv * D / 2 ** 20

"""Attention forward over an fp8 (e4m3fn) paged KV cache (ops.flash_attention_varlen_paged with k_scale / v_scale,
mio_fa3_fwd_paged_kv8): chunked prefill, shared prefixes and windows over the one-byte cache.

The caches are written by ops.reshape_and_cache_varlen(..., k_scale=, v_scale=) from random 16-bit K / V with non-unit
scales; every page and slot nobody wrote holds fp8 NaN bytes (0x7F in K, 0xFF in V), which must never reach the output.
Each case asserts ops.fa3_paged_route first, then checks every sequence against the fp64 oracle (_attn_check) over the
gathered, dequantised context (x8.float() * scale) at the bars of the route's family, out and lse both.  With
power-of-two scales the dequantised cache is exact in 16 bits, and the fp8 launch must then agree with the 16-bit paged
launch over a cache holding those values.
"""
import ctypes

import pytest
import torch

import _attn_check as ac

pytestmark = pytest.mark.gpu

DEV = "cuda"
F8 = torch.float8_e4m3fn
DTYPES = [torch.bfloat16, torch.float16]
GUARD = 8


def _ops():
    from mio import ops
    return ops


def _cu(lens):
    c = [0]
    for n in lens:
        c.append(c[-1] + n)
    return torch.tensor(c, dtype=torch.int32, device=DEV)


def _nan_cache(nb, L, bs, Hkv, D):
    kc = torch.full((nb, L, bs, Hkv, D), 0x7F, dtype=torch.uint8, device=DEV).view(F8)
    vc = torch.full((nb, L, bs, Hkv, D), 0xFF, dtype=torch.uint8, device=DEV).view(F8)
    return kc, vc


def _fp8_cache(dtype, lens_k, *, bs, Hkv, D, L, layer, ks, vs, shared=0, spare=1, g=None):
    """fp8 caches filled with NaN bytes, a table of randomly permuted pages (`spare` allocated pages past each sequence's
    last; sequences 0 and 1 share their first `shared` pages), and each sequence's keys written at `layer` by
    reshape_and_cache_varlen from random 16-bit K / V (sequence 1 writes only past the shared prefix).  Returns
    (kc, vc, bt, k_scale, v_scale) with the scales fp32 [L] on the device."""
    ops = _ops()
    npages = [(n + bs - 1) // bs + spare for n in lens_k]
    nb = sum(npages) + 3
    perm = torch.randperm(nb, generator=g).tolist()
    width = max(npages + [1])
    bt = torch.zeros(len(lens_k), width, dtype=torch.int32)
    nxt = 0
    for b, n in enumerate(npages):
        for j in range(n):
            if b == 1 and j < shared:
                bt[b, j] = bt[0, j]
            else:
                bt[b, j] = perm[nxt]
                nxt += 1
    bt = bt.to(DEV)
    kc, vc = _nan_cache(nb, L, bs, Hkv, D)
    k_scale = torch.full((L,), 0.7, dtype=torch.float32, device=DEV)
    v_scale = torch.full((L,), 1.3, dtype=torch.float32, device=DEV)
    k_scale[layer], v_scale[layer] = ks, vs
    new = [n - (shared * bs if b == 1 and shared else 0) for b, n in enumerate(lens_k)]
    T = sum(new)
    if T > 0:
        # values spread over e4m3's range at these scales (|x| / scale up to ~4 sigma = ~40)
        k = (torch.randn(T, Hkv, D, generator=g) * 10 * ks).to(dtype).to(DEV)
        v = (torch.randn(T, Hkv, D, generator=g) * 10 * vs).to(dtype).to(DEV)
        cl = torch.tensor(lens_k, dtype=torch.int32, device=DEV)
        ops.reshape_and_cache_varlen(k, v, kc, vc, bt, _cu(new), cl, bs, layer, k_scale=k_scale, v_scale=v_scale)
    return kc, vc, bt, k_scale, v_scale


def _gather_deq(kc, vc, bt, lens, layer, ks, vs):
    """Per sequence, the dequantised fp64 keys / values 0 .. n-1 of its pages."""
    bs = kc.shape[2]
    out = []
    for b, n in enumerate(lens):
        pos = torch.arange(n, device=DEV)
        pages, slots = bt[b, pos // bs].long(), pos % bs
        out.append((kc[pages, layer, slots].double() * ks, vc[pages, layer, slots].double() * vs))
    return out


def _ref(q, k, v, causal, left, right, off, scale):
    """fp64 (o [1,Sq,H,D], lse [1,H,Sq]); q [Sq,H,D], k / v [Sk,Hkv,D] fp64; keys outside the (causal / window) band
    absent; off = Lk - Lq (bottom-right)."""
    Sq, H, D = q.shape
    Sk, Hkv = k.shape[0], k.shape[1]
    qd = q.double().permute(1, 0, 2)
    kd = k.repeat_interleave(H // Hkv, dim=1).permute(1, 0, 2)
    vd = v.repeat_interleave(H // Hkv, dim=1).permute(1, 0, 2)
    s = qd @ kd.transpose(-1, -2) * scale
    i = torch.arange(Sq, device=q.device).view(Sq, 1) + off
    j = torch.arange(Sk, device=q.device).view(1, Sk)
    vis = torch.ones(Sq, Sk, dtype=torch.bool, device=q.device)
    if causal or right >= 0:
        vis &= j <= i + (0 if causal else right)
    if left >= 0:
        vis &= j >= i - left
    s = s.masked_fill(~vis, float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - torch.where(torch.isfinite(lse), lse, torch.zeros_like(lse)).unsqueeze(-1))
    p = torch.where(vis.any(-1).view(1, Sq, 1), p, torch.zeros_like(p))
    o = (p @ vd).permute(1, 0, 2)
    return o[None].cpu(), lse[None].cpu()


def _check_oracle(out, lse, q, ctx, lens_q, eff, dtype, route, causal, window, what):
    D = q.shape[-1]
    scale = D ** -0.5
    for b in range(len(lens_q)):
        q0, Lq, Lk = sum(lens_q[:b]), lens_q[b], eff[b]
        if Lq == 0:
            continue
        k, v = ctx[b]
        ro, rl = _ref(q[q0:q0 + Lq], k, v, causal, window[0], window[1], Lk - Lq, scale)
        ac.check(out[q0:q0 + Lq][None].cpu(), ro, dtype, route, lse=lse[:, q0:q0 + Lq][None].cpu(), ref_lse=rl,
                 what=f"{what} seq {b} (Lq {Lq}, Lk {Lk})")


def run_kv8(dtype, lens_q, lens_k, *, H=2, Hkv=None, D=64, causal=False, bs=64, L=2, layer=1, shared=0, spare=1,
            window=(-1, -1), ks=0.05, vs=0.08, seed=0, what=""):
    """One guarded mio_fa3_fwd_paged_kv8 launch (route asserted, guard rows unchanged), every sequence vs the oracle."""
    from mio import _lib
    ops = _ops()
    Hkv = H if Hkv is None else Hkv
    g = torch.Generator().manual_seed(seed * 7919 + sum(lens_q) * 31 + sum(lens_k) * 17 + D + bs)
    kc, vc, bt, k_scale, v_scale = _fp8_cache(dtype, lens_k, bs=bs, Hkv=Hkv, D=D, L=L, layer=layer, ks=ks, vs=vs,
                                              shared=shared, spare=spare, g=g)
    Tq = sum(lens_q)
    q = torch.randn(Tq, H, D, generator=g).to(dtype).to(DEV)
    cu_q = _cu(lens_q)
    sk = torch.tensor(lens_k, dtype=torch.int32, device=DEV)
    mq, mk = max(lens_q + [1]), max(lens_k + [1])
    kw = dict(layer_idx=layer, causal=causal, window_size=window, k_scale=k_scale, v_scale=v_scale)
    route = ops.fa3_paged_route(q, kc, vc, bt, cu_q, sk, mq, mk, **kw)
    want = "empty" if Tq == 0 else ("fwd5" if D <= 64 else "fwd3")
    assert route == want, f"{what}: route {route}, expected {want}"

    sent = torch.tensor(-12345.0).to(dtype).item()
    obuf = torch.full((GUARD + Tq + GUARD, H, D), sent, dtype=dtype, device=DEV)
    lbuf = torch.full((GUARD + H * Tq + GUARD,), -54321.0, dtype=torch.float32, device=DEV)
    out = obuf[GUARD:GUARD + Tq]
    p, out, _lse, _keep, scales = ops._paged_args(q, kc, vc, bt, cu_q, sk, mq, mk, layer_idx=layer, causal=causal,
                                                  return_lse=True, out=out, k_scale=k_scale, v_scale=v_scale)
    p.lse = lbuf.data_ptr() + 4 * GUARD
    _lib.check(_lib.lib.mio_fa3_fwd_paged_kv8(ctypes.byref(p), scales[0], scales[1], window[0], window[1],
                                              torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert (obuf[:GUARD] == sent).all() and (obuf[GUARD + Tq:] == sent).all(), f"{what}: o guard rows overwritten"
    assert (lbuf[:GUARD] == -54321.0).all() and (lbuf[GUARD + H * Tq:] == -54321.0).all(), f"{what}: lse guard overwritten"
    lse = lbuf[GUARD:GUARD + H * Tq].view(H, Tq)
    ctx = _gather_deq(kc, vc, bt, lens_k, layer, ks, vs)
    _check_oracle(out, lse, q, ctx, lens_q, lens_k, dtype, route, causal, window, what)
    return out, lse


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [16, 64, 80, 96, 128])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("heads", [(16, 16), (32, 8)])
def test_kv8_prefill_matrix(dtype, D, causal, heads):
    """Chunk-over-prefix shapes: queries shorter than, equal to and longer than the cached keys, ragged lengths with an
    empty query chunk and an empty context, permuted pages, spare pages of NaN bytes."""
    H, Hkv = heads
    run_kv8(dtype, [300, 1, 0, 129, 200], [700, 64, 50, 129, 0], H=H, Hkv=Hkv, D=D, causal=causal,
            what=f"D{D} causal={causal} H{H}/{Hkv}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("bs", [64, 256])
def test_kv8_prefill_page_geometry(dtype, D, bs):
    """Block sizes 64 / 256, a shared prefix (sequences 0 and 1 share their first pages), layer 1 of a 3-layer cache whose
    other layers hold NaN bytes, two spare pages per sequence."""
    run_kv8(dtype, [200, 130, 77], [900, 1000, 333], H=4, Hkv=2, D=D, causal=True, bs=bs, L=3, layer=1, shared=2,
            spare=2, what=f"geometry bs{bs} D{D}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [64, 96, 128])
@pytest.mark.parametrize("window,causal", [((100, 0), True), ((64, 32), False), ((5000, 0), True), ((200, -1), False)])
def test_kv8_prefill_window(dtype, D, window, causal):
    """Sliding windows: left only (causal), left and right, a window wider than every context, left with no right
    bound."""
    run_kv8(dtype, [300, 1, 257], [900, 65, 257], H=4, Hkv=2, D=D, causal=causal, window=window,
            what=f"window {window} D{D}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("window", [(-1, -1), (130, 0)])
def test_kv8_prefill_exact_vs_16bit(dtype, D, window):
    """Power-of-two scales make the dequantised cache exact in 16 bits: the fp8 launch agrees with the 16-bit paged launch
    over a cache holding those values (out within 1 ulp, lse within 1e-5)."""
    ops = _ops()
    lens_q, lens_k, H, Hkv, layer = [260, 33, 128], [700, 33, 1000], 8, 4, 1
    g = torch.Generator().manual_seed(D + 7)
    ks, vs = 0.0625, 0.125
    kc, vc, bt, k_scale, v_scale = _fp8_cache(dtype, lens_k, bs=64, Hkv=Hkv, D=D, L=2, layer=layer, ks=ks, vs=vs, g=g)
    kc16 = (kc.float() * k_scale.view(1, -1, 1, 1, 1)).to(dtype)
    vc16 = (vc.float() * v_scale.view(1, -1, 1, 1, 1)).to(dtype)
    assert torch.equal(kc16[bt[0, 0].long(), layer].float(), kc[bt[0, 0].long(), layer].float() * ks)
    q = torch.randn(sum(lens_q), H, D, generator=g).to(dtype).to(DEV)
    cu_q, sk = _cu(lens_q), torch.tensor(lens_k, dtype=torch.int32, device=DEV)
    args = (q, kc, vc, bt, cu_q, sk, max(lens_q), max(lens_k))
    causal = True
    o8, l8 = ops.flash_attention_varlen_paged(*args, layer_idx=layer, causal=causal, return_lse=True, window_size=window,
                                              k_scale=k_scale, v_scale=v_scale)
    o16, l16 = ops.flash_attention_varlen_paged(q, kc16, vc16, *args[3:], layer_idx=layer, causal=causal,
                                                return_lse=True, window_size=window)
    torch.cuda.synchronize()
    assert torch.isfinite(o8).all()
    ulp = torch.finfo(dtype).eps * o16.float().abs().clamp_min(torch.finfo(dtype).tiny)
    assert ((o8.float() - o16.float()).abs() <= ulp * 1.0001).all(), f"out differs by more than 1 ulp (D{D} {window})"
    assert ((l8 - l16).abs() <= 1e-5).all(), f"lse differs (D{D} {window}): {(l8 - l16).abs().max().item()}"


def test_kv8_prefill_scale_updated_in_place():
    """The scales are read on the device at every launch: an in-place update between two calls changes the result to the
    one the new scales give."""
    ops = _ops()
    dtype, lens_q, lens_k, D, layer = torch.bfloat16, [150, 64], [500, 64], 64, 0
    g = torch.Generator().manual_seed(3)
    kc, vc, bt, k_scale, v_scale = _fp8_cache(dtype, lens_k, bs=64, Hkv=2, D=D, L=1, layer=layer, ks=0.05, vs=0.08, g=g)
    q = torch.randn(sum(lens_q), 4, D, generator=g).to(dtype).to(DEV)
    cu_q, sk = _cu(lens_q), torch.tensor(lens_k, dtype=torch.int32, device=DEV)
    args = (q, kc, vc, bt, cu_q, sk, max(lens_q), max(lens_k))
    kw = dict(layer_idx=layer, causal=True, return_lse=True, k_scale=k_scale, v_scale=v_scale)
    o1, l1 = ops.flash_attention_varlen_paged(*args, **kw)
    o1, l1 = o1.clone(), l1.clone()
    k_scale.mul_(1.7)
    v_scale.mul_(0.6)
    o2, l2 = ops.flash_attention_varlen_paged(*args, **kw)
    torch.cuda.synchronize()
    assert not torch.equal(o1, o2) and not torch.equal(l1, l2)
    ctx = _gather_deq(kc, vc, bt, lens_k, layer, 0.05 * 1.7, 0.08 * 0.6)
    _check_oracle(o2, l2, q, ctx, lens_q, lens_k, dtype, "fwd5", True, (-1, -1), "updated scales")


def test_kv8_prefill_errors():
    """Scales with a 16-bit cache, an e5m2 cache and a head dim not a multiple of 16 are refused; without scales the first
    error is decode's."""
    ops = _ops()
    q = torch.zeros(3, 4, 64, dtype=torch.bfloat16, device=DEV)
    k8 = torch.zeros(4, 1, 64, 2, 64, dtype=F8, device=DEV)
    bt = torch.zeros(2, 2, dtype=torch.int32, device=DEV)
    cu = torch.tensor([0, 1, 3], dtype=torch.int32, device=DEV)
    sk = torch.tensor([10, 20], dtype=torch.int32, device=DEV)
    one = torch.ones(1, device=DEV)
    with pytest.raises(ValueError, match="requires k_scale and v_scale"):
        ops.flash_attention_varlen_paged(q, k8, k8, bt, cu, sk, 2, 20)
    k16 = torch.zeros(4, 1, 64, 2, 64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError, match="fp8"):
        ops.flash_attention_varlen_paged(q, k16, k16, bt, cu, sk, 2, 20, k_scale=one, v_scale=one)
    with pytest.raises(ValueError, match="e4m3fn"):
        ops.flash_attention_varlen_paged(q, k8.view(torch.float8_e5m2), k8.view(torch.float8_e5m2), bt, cu, sk, 2, 20,
                                         k_scale=one, v_scale=one)
    q40 = torch.zeros(3, 4, 40, dtype=torch.bfloat16, device=DEV)
    k40 = torch.zeros(4, 1, 64, 2, 40, dtype=F8, device=DEV)
    with pytest.raises(ValueError, match="multiple of 16"):
        ops.flash_attention_varlen_paged(q40, k40, k40, bt, cu, sk, 2, 20, k_scale=one, v_scale=one)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [64, 128])
def test_kv8_chunked_prefill_then_decode(dtype, D):
    """End to end on an fp8 PagedKVCache: a 3-chunk chunked prefill (each chunk writes its K / V, then attends over the
    cache), then one fp8 decode step; every result against the oracle over the whole dequantised context."""
    from mio.baseline.inference import PagedKVCache
    ops = _ops()
    H, Hkv, L, layer, bs = 8, 2, 2, 1, 64
    pc = PagedKVCache(num_blocks=40, block_size=bs, num_layers=L, num_heads=Hkv, head_dim=D, dtype=F8, device=DEV)
    k_scale, v_scale = pc.get_kv_scales()
    k_scale[layer], v_scale[layer] = 0.04, 0.09
    kc, vc = pc.get_physical_caches()
    chunks = [[300, 100], [257, 1], [64, 190]]
    g = torch.Generator().manual_seed(D)
    done = [0, 0]
    for step, new in enumerate(chunks):
        for s in range(2):
            done[s] += new[s]
            pc.allocate_blocks_for_sequence(s, done[s])
        bt, cl, mx = pc.kernel_metadata([0, 1])
        T = sum(new)
        k = (torch.randn(T, Hkv, D, generator=g) * 0.4).to(dtype).to(DEV)
        v = (torch.randn(T, Hkv, D, generator=g) * 0.9).to(dtype).to(DEV)
        ops.reshape_and_cache_varlen(k, v, kc, vc, bt, _cu(new), cl, bs, layer, k_scale=k_scale, v_scale=v_scale)
        q = torch.randn(T, H, D, generator=g).to(dtype).to(DEV)
        o, lse = ops.flash_attention_varlen_paged(q, kc, vc, bt, _cu(new), cl, max(new), mx, layer_idx=layer, causal=True,
                                                  return_lse=True, k_scale=k_scale, v_scale=v_scale)
        ctx = _gather_deq(kc, vc, bt, list(done), layer, 0.04, 0.09)
        route = "fwd5" if D <= 64 else "fwd3"
        _check_oracle(o, lse, q, ctx, new, list(done), dtype, route, True, (-1, -1), f"chunk {step}")
    # one decode step: append a token per sequence, write it, attend
    for s in range(2):
        pc.append_token(s)
        done[s] += 1
    bt, cl, mx = pc.kernel_metadata([0, 1])
    k = (torch.randn(2, Hkv, D, generator=g) * 0.4).to(dtype).to(DEV)
    v = (torch.randn(2, Hkv, D, generator=g) * 0.9).to(dtype).to(DEV)
    ops.reshape_and_cache_varlen(k, v, kc, vc, bt, _cu([1, 1]), cl, bs, layer, k_scale=k_scale, v_scale=v_scale)
    qd = torch.randn(2, H, 1, D, generator=g).to(dtype).to(DEV)
    od = torch.empty_like(qd)
    ops.paged_attention_forward(qd, od, kc, vc, bt, cl, bs, mx, layer, k_scale=k_scale, v_scale=v_scale)
    torch.cuda.synchronize()
    ctx = _gather_deq(kc, vc, bt, list(done), layer, 0.04, 0.09)
    for s in range(2):
        ro, _rl = _ref(qd[s].permute(1, 0, 2), ctx[s][0], ctx[s][1], True, -1, -1, done[s] - 1, D ** -0.5)
        err = (od[s].permute(1, 0, 2)[None].float().cpu() - ro.float()).abs().max().item()
        assert err < 2e-2, f"decode seq {s}: max error {err}"

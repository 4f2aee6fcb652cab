"""Sliding-window attention forward: dense (ops.fa3_fwd / flash_attention), packed varlen and paged, window_size =
(left, right) with flash-attn's meaning.  Every case checks the route (the windowed fwd5 / fwd3 kernels) and compares
against an fp64 reference in which the keys outside the window are absent, judged by _attn_check at the bars of the
route's family.  Paged output equals windowed varlen on the gathered pages bit for bit; a window that covers everything
equals the unwindowed launch bit for bit wherever that launch also takes fwd5 / fwd3.
"""

import pytest
import torch

import _attn_check as ac

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _ops():
    from mio import ops
    return ops


def _ref(q, k, v, causal, left, right, off, scale):
    """fp64 (o [B,Sq,H,D], lse [B,H,Sq]) with keys outside the window absent; q [B,Sq,H,D], k / v [B,Sk,Hkv,D] (on the
    GPU in float64); off = q_offset - k_offset (bottom-right: Sk - Sq)."""
    B, Sq, H, D = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    qd = q.double().permute(0, 2, 1, 3)
    kd = k.double().repeat_interleave(H // Hkv, dim=2).permute(0, 2, 1, 3)
    vd = v.double().repeat_interleave(H // Hkv, dim=2).permute(0, 2, 1, 3)
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
    p = torch.where(vis.any(-1).view(1, 1, Sq, 1), p, torch.zeros_like(p))
    o = (p @ vd).permute(0, 2, 1, 3)
    return o.cpu(), lse.cpu()


def _family(D):
    return "fwd5" if D <= 64 else "fwd3"


_WINDOWS = [(0, 0), (63, 0), (64, 0), (65, 0), (127, 0), (1000, 0), ("S-1", 0), ("S+5", 0), (256, 256), (-1, 100),
            (100, -1)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D", [64, 80, 128])
@pytest.mark.parametrize("causal", [True, False])
def test_dense_window(dtype, D, causal):
    ops = _ops()
    g = torch.Generator(device="cpu").manual_seed(D + causal)
    for (Sq, Sk, H, Hkv, qo, ko) in ((700, 700, 4, 4, 0, 0), (129, 1100, 8, 2, 971, 0), (300, 200, 4, 1, 0, 50)):
        q = torch.randn(2, Sq, H, D, generator=g).to(dtype).to(DEV)
        k = torch.randn(2, Sk, Hkv, D, generator=g).to(dtype).to(DEV)
        v = torch.randn(2, Sk, Hkv, D, generator=g).to(dtype).to(DEV)
        for left, right in _WINDOWS:
            left = {"S-1": Sk - 1, "S+5": Sk + 5}.get(left, left)
            if causal and right > 0:
                continue
            kw = dict(causal=causal, q_offset=qo, k_offset=ko, window_size=(left, right))
            assert ops.fa3_route(q, k, v, **kw) == _family(D)
            o, lse = ops.fa3_fwd(q, k, v, return_lse=True, **kw)
            ro, rl = _ref(q, k, v, causal, left, right, qo - ko, D ** -0.5)
            ac.check(o.cpu(), ro, dtype, _family(D), lse.cpu(), rl, what=f"D{D} {Sq}x{Sk} causal={causal} w=({left},{right})")
        # a window past every key: the unwindowed launch, bit for bit (Sq > 128: it takes fwd5 / fwd3 too)
        if Sq > 128 and qo == ko == 0:
            w = (Sk + Sq, 0 if causal else -1)
            a = ops.fa3_fwd(q, k, v, causal=causal, window_size=w)
            assert torch.equal(a, ops.fa3_fwd(q, k, v, causal=causal))
        assert torch.equal(ops.fa3_fwd(q, k, v, causal=causal, window_size=(-1, -1)), ops.fa3_fwd(q, k, v, causal=causal))


def test_dense_window_gqa_flash_attention():
    ops = _ops()
    g = torch.Generator().manual_seed(3)
    q = torch.randn(1, 1000, 32, 128, generator=g).to(torch.bfloat16).to(DEV)
    k = torch.randn(1, 1000, 8, 128, generator=g).to(torch.bfloat16).to(DEV)
    v = torch.randn(1, 1000, 8, 128, generator=g).to(torch.bfloat16).to(DEV)
    o = ops.flash_attention(q, k, v, causal=True, window_size=(255, 0))
    ro, _ = _ref(q, k, v, True, 255, 0, 0, 128 ** -0.5)
    ac.check(o.cpu(), ro, torch.bfloat16, "fwd3", what="gqa flash_attention")
    for S in (1, 77):  # short sequences: the windowed kernels too (no fwd1 fallback)
        assert ops.fa3_route(q[:, :S], k[:, :S], v[:, :S], causal=True, window_size=(16, 0)) == "fwd3"
        o = ops.flash_attention(q[:, :S], k[:, :S], v[:, :S], causal=True, window_size=(16, 0))
        ro, _ = _ref(q[:, :S], k[:, :S], v[:, :S], True, 16, 0, 0, 128 ** -0.5)
        ac.check(o.cpu(), ro, torch.bfloat16, "fwd3", what=f"S={S}")


def _cu(lens):
    c = [0]
    for n in lens:
        c.append(c[-1] + n)
    return torch.tensor(c, dtype=torch.int32, device=DEV)


_LQ = [300, 0, 5, 700, 64, 1, 129, 200, 0, 513, 40, 256, 3, 1000, 77, 90]
_LK = [300, 100, 0, 900, 64, 50, 129, 130, 0, 513, 400, 700, 3, 1000, 20, 90]  # some Lq > Lk, some empty


def _varlen_ref_check(o, lse, q, k, v, lq, lk, causal, left, right, dtype, D, what):
    cq, ck = 0, 0
    for b, (nq, nk) in enumerate(zip(lq, lk)):
        if nq:
            qs, ks, vs = q[cq:cq + nq][None], k[ck:ck + nk][None], v[ck:ck + nk][None]
            if nk:
                ro, rl = _ref(qs, ks, vs, causal, left, right, nk - nq, D ** -0.5)
            else:
                ro = torch.zeros(1, nq, q.shape[1], D, dtype=torch.float64)
                rl = torch.full((1, q.shape[1], nq), float("-inf"), dtype=torch.float64)
            ac.check(o[cq:cq + nq][None].cpu(), ro, dtype, _family(D), lse[:, cq:cq + nq][None].cpu(), rl,
                     what=f"{what} seq {b}")
        cq += nq
        ck += nk


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("causal,window", [(True, (127, 0)), (True, (0, -1)), (False, (200, 64)), (False, (-1, 0)),
                                           (True, (5000, 0))])
def test_varlen_window(dtype, D, causal, window):
    ops = _ops()
    g = torch.Generator().manual_seed(D)
    H, Hkv = 8, 2
    q = torch.randn(sum(_LQ), H, D, generator=g).to(dtype).to(DEV)
    k = torch.randn(sum(_LK), Hkv, D, generator=g).to(dtype).to(DEV)
    v = torch.randn(sum(_LK), Hkv, D, generator=g).to(dtype).to(DEV)
    cq, ck = _cu(_LQ), _cu(_LK)
    args = (q, k, v, cq, ck, max(_LQ), max(_LK))
    assert ops.fa3_varlen_route(*args, causal=causal, window_size=window) == _family(D)
    o, lse = ops.flash_attention_varlen(*args, causal=causal, return_lse=True, window_size=window)
    _varlen_ref_check(o, lse, q, k, v, _LQ, _LK, causal, *window, dtype, D, f"varlen w={window}")
    if window[0] >= max(_LK) + max(_LQ) and window[1] in (-1, 0):
        a, la = ops.flash_attention_varlen(*args, causal=causal, return_lse=True)
        if window[1] == -1 or causal:
            assert torch.equal(o, a) and torch.equal(lse, la)
    a, la = ops.flash_attention_varlen(*args, causal=causal, return_lse=True, window_size=(-1, -1))
    b, lb = ops.flash_attention_varlen(*args, causal=causal, return_lse=True)
    assert torch.equal(a, b) and torch.equal(la, lb)


def _pages(lk, bs, Hkv, D, dtype, g):
    npages = [(n + bs - 1) // bs + 1 for n in lk]
    nb = sum(npages) + 3
    kc = torch.randn(nb, 1, bs, Hkv, D, generator=g).to(dtype).to(DEV)
    vc = torch.randn(nb, 1, bs, Hkv, D, generator=g).to(dtype).to(DEV)
    perm = torch.randperm(nb, generator=g)
    width = max(npages)
    bt = torch.zeros(len(lk), width, dtype=torch.int32)
    i = 0
    for b, n in enumerate(npages):
        bt[b, :n] = perm[i:i + n]
        i += n
    bt = bt.to(DEV)
    # the gathered contiguous K / V of every sequence
    ks, vs = [], []
    for b, n in enumerate(lk):
        pos = torch.arange(n, device=DEV)
        pg = bt[b, pos // bs].long()
        ks.append(kc[pg, 0, pos % bs])
        vs.append(vc[pg, 0, pos % bs])
    return kc, vc, bt, torch.cat(ks), torch.cat(vs)


@pytest.mark.parametrize("bs", [64, 256])
@pytest.mark.parametrize("D", [64, 128])
def test_paged_window_equals_varlen(bs, D):
    ops = _ops()
    dtype = torch.bfloat16
    g = torch.Generator().manual_seed(bs + D)
    H, Hkv = 8, 2
    kc, vc, bt, k, v = _pages(_LK, bs, Hkv, D, dtype, g)
    q = torch.randn(sum(_LQ), H, D, generator=g).to(dtype).to(DEV)
    cq, ck = _cu(_LQ), _cu(_LK)
    used = torch.tensor(_LK, dtype=torch.int32, device=DEV)
    for causal, w in ((True, (127, 0)), (False, (300, 100)), (True, (0, 0))):
        assert ops.fa3_paged_route(q, kc, vc, bt, cq, used, max(_LQ), max(_LK), causal=causal, window_size=w) == _family(D)
        o, lse = ops.flash_attention_varlen_paged(q, kc, vc, bt, cq, used, max(_LQ), max(_LK), causal=causal,
                                                  return_lse=True, window_size=w)
        a, la = ops.flash_attention_varlen(q, k, v, cq, ck, max(_LQ), max(_LK), causal=causal, return_lse=True,
                                           window_size=w)
        assert torch.equal(o, a) and torch.equal(lse, la), (causal, w)


def test_paged_window_chunked_prefill():
    """4096 cached + 512 new tokens per sequence, left = 1024: against the fp64 reference."""
    ops = _ops()
    dtype = torch.float16
    g = torch.Generator().manual_seed(21)
    H, Hkv, D, bs = 8, 8, 64, 64
    lk, lq = [4608, 4608, 600], [512, 512, 100]
    kc, vc, bt, k, v = _pages(lk, bs, Hkv, D, dtype, g)
    q = torch.randn(sum(lq), H, D, generator=g).to(dtype).to(DEV)
    cq, used = _cu(lq), torch.tensor(lk, dtype=torch.int32, device=DEV)
    o, lse = ops.flash_attention_varlen_paged(q, kc, vc, bt, cq, used, max(lq), max(lk), causal=True, return_lse=True,
                                              window_size=(1024, 0))
    _varlen_ref_check(o, lse, q, k, v, lq, lk, True, 1024, 0, dtype, D, "chunked prefill")


def test_window_graph_capture():
    """A windowed paged prefill and a windowed decode captured in one CUDA graph; replay equals eager."""
    ops = _ops()
    dtype = torch.bfloat16
    g = torch.Generator().manual_seed(4)
    H, Hkv, D, bs = 8, 2, 128, 64
    lk, lq = [900, 300], [200, 300]
    kc, vc, bt, _k, _v = _pages(lk, bs, Hkv, D, dtype, g)
    q = torch.empty(sum(lq), H, D, dtype=dtype, device=DEV)
    qd = torch.empty(2, H, 1, D, dtype=dtype, device=DEV)
    cq, used = _cu(lq), torch.tensor(lk, dtype=torch.int32, device=DEV)
    out = torch.empty_like(q)
    od = torch.empty_like(qd)

    def step():
        ops.flash_attention_varlen_paged(q, kc, vc, bt, cq, used, max(lq), max(lk), causal=True, out=out,
                                         window_size=(100, 0))
        ops.paged_attention_forward(qd, od, kc, vc, bt, used, bs, max(lk), 0, window_size=(100, -1))

    def fill(seed):
        gg = torch.Generator().manual_seed(seed)
        for t in (q, qd):
            t.copy_(torch.randn(t.shape, generator=gg).to(dtype))

    fill(1)
    step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    fill(2)
    graph.replay()
    torch.cuda.synchronize()
    o_graph, od_graph = out.clone(), od.clone()
    step()
    torch.cuda.synchronize()
    assert torch.equal(o_graph, out) and torch.equal(od_graph, od)


def test_module_window_config():
    """FlashAttentionConfig.window_size reaches the kernels: FlashAttention3 equals ops.flash_attention with the window,
    and the fp64 reference."""
    from mio.kernels.attention.flash_attention import FlashAttention3, FlashAttentionConfig
    ops = _ops()
    g = torch.Generator().manual_seed(8)
    q, k, v = (torch.randn(2, 600, 4, 64, generator=g).to(torch.bfloat16).to(DEV) for _ in range(3))
    m = FlashAttention3(FlashAttentionConfig(causal=True, precision="bf16", window_size=(100, 0)))
    o = m(q, k, v)
    assert torch.equal(o, ops.flash_attention(q, k, v, causal=True, window_size=(100, 0)))
    ro, _ = _ref(q, k, v, True, 100, 0, 0, 64 ** -0.5)
    ac.check(o.cpu(), ro, torch.bfloat16, "fwd5", what="module")

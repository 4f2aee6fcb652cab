"""Sliding-window paged decode (ops.paged_attention_forward(window_size=(left, -1)), mio_fa3_decode_paged_window).

Row qi of q_len sees the cached keys j < ctx with j >= ctx - q_len + qi - left.  Every case asserts the decode kernel the
launch takes (ops.paged_attention_route) and compares against an fp64 reference in which the keys outside the window are
absent, at the bars of the unwindowed decode tests (test_gpu_kernels.py).  A window that covers the whole context runs the
windowed kernel on the unwindowed splits and must be bitwise equal to the unwindowed launch; (-1, -1) is that launch.
"""
import pytest
import torch

import _decode_check as dc

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = {torch.float16: (1e-3, 4e-3), torch.bfloat16: (3e-3, 2e-2)}


def _ops():
    from mio import ops
    return ops


def _judge(out, q, kc, vc, bt, ctx, bs, layer, left, dtype, route, what):
    """The decode result against _decode_check's fp64 windowed reference: the whole-tensor bars of the unwindowed decode
    tests, then the per-row check against the fp32 model."""
    ref, lse = dc.reference(q, kc, vc, bt, ctx, bs, layer, left=left)
    _cmp(out, ref, dtype, what)
    model_o = dc.model(q, kc, vc, bt, ctx, bs, layer, dtype=dtype, p16=route == "gqa", left=left)
    dc.check(out, ref, lse, dtype, (dtype, route, "kv16"), model_o, what, win=left >= 0)


def _cmp(got, ref, dtype, what):
    ref = ref.to(dtype).float()
    got = got.float().cpu()
    rel = ((got - ref).abs().mean() / ref.abs().mean().clamp_min(1e-12)).item()
    mx = (got - ref).abs().max().item()
    rtol, atol = TOL[dtype]
    assert rel < rtol and mx < atol * max(1.0, ref.abs().max().item()), f"{what}: rel_err={rel:.3e} max={mx:.3e}"


def _cache(ctxs, *, bs, Hkv, D, L, dtype, g):
    maxb = max((max(ctxs) + bs - 1) // bs, 1) + 1
    nb = len(ctxs) * maxb + 2
    kc = torch.randn(nb, L, bs, Hkv, D, generator=g).to(dtype)
    vc = torch.randn(nb, L, bs, Hkv, D, generator=g).to(dtype)
    bt = torch.randperm(nb, generator=g)[:len(ctxs) * maxb].view(len(ctxs), maxb).to(torch.int32)
    return kc, vc, bt


# (H, Hkv, D, B) of each decode kernel: per-head (D 80), whole token rows (MHA, B >= 16, q_len 1), matrix-core GQA
_KERNELS = {"head": (4, 2, 80, 5), "rows": (8, 8, 64, 16), "gqa": (8, 2, 128, 5)}
_LEFTS = [0, 15, 16, 17, 1000, 1 << 20]


@pytest.mark.parametrize("kernel", ["head", "rows", "gqa"])
@pytest.mark.parametrize("q_len", [1, 4])
@pytest.mark.parametrize("bs", [16, 64])
def test_decode_window_matches_reference(kernel, q_len, bs):
    ops = _ops()
    H, Hkv, D, B = _KERNELS[kernel]
    if kernel == "rows" and q_len > 1:
        kernel = "gqa"  # several query vectors per key: the whole-row kernel takes one
    dtype = torch.bfloat16 if bs == 16 else torch.float16
    g = torch.Generator().manual_seed(q_len * 100 + bs + D)
    base = [1500, 1, 0, 700, 33, 1024, 3, 129]
    ctxs = (base * 3)[:B]
    L, layer, max_ctx = 2, 1, 1500
    kc, vc, bt = _cache(ctxs, bs=bs, Hkv=Hkv, D=D, L=L, dtype=dtype, g=g)
    q = (torch.randn(B, H, q_len, D, generator=g) * 1.5).to(dtype)
    ctx = torch.tensor(ctxs, dtype=torch.int32)
    args = (kc.to(DEV), vc.to(DEV), bt.to(DEV), ctx.to(DEV), bs, max_ctx, layer)
    qd = q.to(DEV)
    for left in _LEFTS:
        out = torch.full((B, H, q_len, D), float("nan"), dtype=dtype, device=DEV)
        ws = (left, -1)
        assert ops.paged_attention_route(qd, out, *args, window_size=ws) == kernel, (kernel, left, q_len)
        ops.paged_attention_forward(qd, out, *args, window_size=ws)
        _judge(out, q, kc, vc, bt, ctx, bs, layer, left, dtype, kernel, f"{kernel} q_len={q_len} bs={bs} left={left}")
        assert out[2].abs().max() == 0  # empty context -> zeros
        if left >= max_ctx + q_len:  # the window covers every context: the unwindowed launch, bit for bit
            plain = torch.full_like(out, float("nan"))
            ops.paged_attention_forward(qd, plain, *args)
            assert torch.equal(out, plain)


@pytest.mark.parametrize("kernel", ["head", "rows", "gqa"])
def test_decode_window_unbounded_is_unwindowed(kernel):
    ops = _ops()
    H, Hkv, D, B = _KERNELS[kernel]
    dtype = torch.bfloat16
    g = torch.Generator().manual_seed(5)
    ctxs = ([300, 17, 0, 129] * 4)[:B]
    kc, vc, bt = _cache(ctxs, bs=16, Hkv=Hkv, D=D, L=1, dtype=dtype, g=g)
    q = torch.randn(B, H, 1, D, generator=g).to(dtype).to(DEV)
    args = (kc.to(DEV), vc.to(DEV), bt.to(DEV), torch.tensor(ctxs, dtype=torch.int32, device=DEV), 16, 300, 0)
    a = torch.empty(B, H, 1, D, dtype=dtype, device=DEV)
    b = torch.empty_like(a)
    ops.paged_attention_forward(q, a, *args)
    ops.paged_attention_forward(q, b, *args, window_size=(-1, -1))
    assert torch.equal(a, b)
    assert ops.paged_attention_route(q, a, *args) == ops.paged_attention_route(q, a, *args, window_size=(-1, -1))


@pytest.mark.parametrize("kernel", ["rows", "gqa"])
def test_decode_window_long_context(kernel):
    """A 4096-key window at the end of 12k-token contexts: several splits inside the window, the split start off the
    block boundary, contexts shorter than the window."""
    ops = _ops()
    H, Hkv, D, _ = _KERNELS[kernel]
    B, bs, left = 16, 64, 4095
    dtype = torch.bfloat16
    g = torch.Generator().manual_seed(9)
    ctxs = [12000, 11001, 4000, 4097, 10000, 12000, 1, 0] * 2
    kc, vc, bt = _cache(ctxs, bs=bs, Hkv=Hkv, D=D, L=1, dtype=dtype, g=g)
    q = torch.randn(B, H, 1, D, generator=g).to(dtype)
    ctx = torch.tensor(ctxs, dtype=torch.int32)
    out = torch.empty(B, H, 1, D, dtype=dtype, device=DEV)
    args = (kc.to(DEV), vc.to(DEV), bt.to(DEV), ctx.to(DEV), bs, 12000, 0)
    assert ops.paged_attention_route(q.to(DEV), out, *args, window_size=(left, -1)) == kernel
    ops.paged_attention_forward(q.to(DEV), out, *args, window_size=(left, -1))
    _judge(out, q, kc, vc, bt, ctx, bs, 0, left, dtype, kernel, f"{kernel} long window")


def test_decode_window_graph_capture():
    """A cache write and a windowed decode captured in one CUDA graph; inputs refilled in place and replayed equal the
    eager result."""
    ops = _ops()
    g = torch.Generator().manual_seed(13)
    dtype = torch.float16
    H, Hkv, D, bs, B = 8, 2, 128, 16, 3
    ctxs = [700, 64, 1]
    kc, vc, bt = _cache([c + 1 for c in ctxs], bs=bs, Hkv=Hkv, D=D, L=1, dtype=dtype, g=g)
    kc, vc, bt = kc.to(DEV), vc.to(DEV), bt.to(DEV)
    cl = torch.tensor([c + 1 for c in ctxs], dtype=torch.int32, device=DEV)
    q = torch.empty(B, H, 1, D, dtype=dtype, device=DEV)
    k_new = torch.empty(B, 1, Hkv, D, dtype=dtype, device=DEV)
    v_new = torch.empty_like(k_new)
    out = torch.empty(B, H, 1, D, dtype=dtype, device=DEV)

    def step():
        ops.reshape_and_cache(k_new, v_new, kc, vc, bt, cl, bs, 0)
        ops.paged_attention_forward(q, out, kc, vc, bt, cl, bs, 701, 0, window_size=(100, -1))

    def fill(seed):
        gg = torch.Generator().manual_seed(seed)
        for t in (q, k_new, v_new):
            t.copy_(torch.randn(t.shape, generator=gg).to(dtype))

    fill(1)
    kc0, vc0 = kc.clone(), vc.clone()
    step()  # warm-up outside the capture (one-time kernel attributes)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    fill(2)
    kc.copy_(kc0)
    vc.copy_(vc0)
    graph.replay()
    torch.cuda.synchronize()
    o_graph = out.clone()
    kc.copy_(kc0)
    vc.copy_(vc0)
    step()
    torch.cuda.synchronize()
    assert torch.equal(o_graph, out)
    assert ops.paged_attention_route(q, out, kc, vc, bt, cl, bs, 701, 0, window_size=(100, -1)) == "gqa"
    _judge(out, q.cpu(), kc.cpu(), vc.cpu(), bt.cpu(), cl.cpu(), bs, 0, 100, dtype, "gqa", "graph")

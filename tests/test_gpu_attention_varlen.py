"""Packed variable-length attention forward (ops.flash_attention_varlen, mio_fa3_fwd_varlen) against the fp64 oracle.

Every case asserts ops.fa3_varlen_route first, then checks each sequence with _attn_check.check at the bars of the route's
kernel family (fwd5 / fwd3) against _attn_check.reference on that sequence's slice (causal: q_offset = Lk - Lq, bottom-right
aligned).  Wherever the dense ops.fa3_fwd call on one sequence routes to the same pipelined kernel, the varlen output and lse
of that sequence must be bitwise equal to it (same tiles in the same order).  o and lse carry guard rows before and after
the packed range, filled with a sentinel that must come back unchanged.  Both storage dtypes throughout.
"""
import ctypes

import pytest
import torch

import _attn_check as ac

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
GUARD = 8  # guard rows of o (tokens) and guard elements of lse on each side


def _ops():
    from mio import ops
    return ops


def _cu(lens):
    c = [0]
    for n in lens:
        c.append(c[-1] + n)
    return torch.tensor(c, dtype=torch.int32, device=DEV)


def _sentinel(dtype):
    return torch.tensor(-12345.0).to(dtype)


def run_varlen(dtype, lens_q, lens_k=None, *, H=2, Hkv=None, D=64, causal=False, fused=False, seed=0, ref_on_gpu=False,
               what=""):
    """One flash_attention_varlen launch through the C ABI with guarded o / lse buffers; route asserted, guards checked,
    every sequence checked against the oracle and (where the dense call takes the same kernel) against the dense call."""
    from mio import _lib
    ops = _ops()
    lens_k = list(lens_q) if lens_k is None else list(lens_k)
    Hkv = H if Hkv is None else Hkv
    B, Tq, Tk = len(lens_q), sum(lens_q), sum(lens_k)
    g = torch.Generator().manual_seed(seed * 7919 + Tq * 31 + Tk * 17 + D)
    if fused:  # self-attention on one [T, 3, H, D] buffer: q / k / v are strided views of it
        assert lens_q == lens_k and H == Hkv
        qkv = torch.randn(Tq, 3, H, D, generator=g).to(dtype).to(DEV)
        q, k, v = qkv[:, 0], qkv[:, 1], qkv[:, 2]
    else:
        q = torch.randn(Tq, H, D, generator=g).to(dtype).to(DEV)
        k = torch.randn(Tk, Hkv, D, generator=g).to(dtype).to(DEV)
        v = torch.randn(Tk, Hkv, D, generator=g).to(dtype).to(DEV)
    cu_q, cu_k = _cu(lens_q), _cu(lens_k)
    mq, mk = max(lens_q + [1]), max(lens_k + [1])
    route = ops.fa3_varlen_route(q, k, v, cu_q, cu_k, mq, mk, causal=causal, return_lse=True)
    want = "empty" if Tq == 0 else ("fwd5" if D <= 64 else "fwd3")
    assert route == want, f"{what}: route {route}, expected {want}"

    sent = _sentinel(dtype)
    obuf = torch.full((GUARD + Tq + GUARD, H, D), sent.item(), dtype=dtype, device=DEV)
    lbuf = torch.full((GUARD + H * Tq + GUARD,), -54321.0, dtype=torch.float32, device=DEV)
    out = obuf[GUARD:GUARD + Tq]
    p, out, _lse, keep = ops._varlen_params(q, k, v, cu_q, cu_k, mq, mk, causal=causal, return_lse=True, out=out)
    p.lse = lbuf.data_ptr() + 4 * GUARD
    _lib.check(_lib.lib.mio_fa3_fwd_varlen(ctypes.byref(p), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert (obuf[:GUARD] == sent).all() and (obuf[GUARD + Tq:] == sent).all(), f"{what}: o guard rows overwritten"
    assert (lbuf[:GUARD] == -54321.0).all() and (lbuf[GUARD + H * Tq:] == -54321.0).all(), f"{what}: lse guard overwritten"
    lse = lbuf[GUARD:GUARD + H * Tq].view(H, Tq)

    for b in range(B):
        q0, Lq, k0, Lk = sum(lens_q[:b]), lens_q[b], sum(lens_k[:b]), lens_k[b]
        if Lq == 0:
            continue
        qb, kb, vb = q[q0:q0 + Lq][None], k[k0:k0 + Lk][None], v[k0:k0 + Lk][None]
        ob, lb = out[q0:q0 + Lq][None], lse[:, q0:q0 + Lq][None]
        ref, ref_lse = ac.reference(qb, kb, vb, causal=causal, q_offset=Lk - Lq, device=DEV if ref_on_gpu else None)
        ac.check(ob, ref, dtype, route, lse=lb, ref_lse=ref_lse, what=f"{what} seq {b} (Lq {Lq}, Lk {Lk})")
        if Lk > 0 and ops.fa3_route(qb, kb, vb, causal=causal, q_offset=Lk - Lq, return_lse=True) == route:
            od, ld = ops.fa3_fwd(qb, kb, vb, causal=causal, q_offset=Lk - Lq, return_lse=True)
            assert torch.equal(ob, od), f"{what} seq {b} (Lq {Lq}, Lk {Lk}): output differs from the dense {route} call"
            assert torch.equal(lb, ld), f"{what} seq {b} (Lq {Lq}, Lk {Lk}): lse differs from the dense {route} call"
    return out, lse


MIXED = [0, 1, 63, 64, 65, 255, 256, 257, 1030, 1, 1100, 300]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [16, 64, 80, 96, 128])
@pytest.mark.parametrize("causal", [False, True])
def test_varlen_mixed_lengths(dtype, D, causal):
    """Lengths 0 .. 1100 in one batch (a length-1 sequence between two long ones), plus a sequence with queries and no keys."""
    run_varlen(dtype, MIXED + [200], MIXED + [0], D=D, causal=causal, what=f"mixed D{D} causal={causal}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [64, 128])
def test_varlen_causal_offsets(dtype, D):
    """Causal with Lq < Lk (chunked prefill against a prefix) and Lq > Lk (leading rows see no key: o 0, lse -inf)."""
    run_varlen(dtype, [300, 129, 700, 300, 64, 1000], [1200, 1000, 200, 1, 600, 1000], D=D, causal=True,
               what=f"offsets D{D}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ratio", [1, 4, 8])
@pytest.mark.parametrize("D", [64, 128])
def test_varlen_gqa(dtype, ratio, D):
    run_varlen(dtype, [513, 1, 300, 77], H=8, Hkv=8 // ratio, D=D, causal=True, what=f"gqa {ratio} D{D}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [64, 96])
def test_varlen_fused_qkv_views(dtype, D):
    """K / V (and Q) as strided views of one fused [total, 3, H, D] buffer."""
    run_varlen(dtype, [400, 3, 257, 129], H=4, D=D, causal=True, fused=True, what=f"fused D{D}")
    run_varlen(dtype, [400, 3, 257, 129], H=4, D=D, causal=False, fused=True, what=f"fused D{D}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [64, 128])
def test_varlen_many_sequences(dtype, D):
    """About 64 sequences of random lengths (some empty), random query / key lengths."""
    g = torch.Generator().manual_seed(D + (dtype == torch.float16))
    lq = torch.randint(0, 520, (64,), generator=g).tolist()
    lk = [n if i % 3 else int(torch.randint(0, 700, (1,), generator=g)) for i, n in enumerate(lq)]
    run_varlen(dtype, lq, lk, H=2, D=D, causal=bool(D == 64), what=f"many D{D}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_varlen_c2_size(dtype):
    """8 x 4096 causal at head dim 64 (the benchmark's attention shape), reference on the GPU."""
    run_varlen(dtype, [4096] * 8, H=16, D=64, causal=True, ref_on_gpu=True, what="C2")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", [64, 128])
def test_keep_mask_equivalence(dtype, causal, D):
    """Self-attention on a padded batch under a [B, S] keep-mask (random left and right padding): pad(varlen(unpad(.)))
    and ops.flash_attention(mask=keep) both match the oracle of the masked problem on the kept rows; the padding rows of
    pad_input's output are exactly zero."""
    ops = _ops()
    B, S, H = 5, 700, 4
    g = torch.Generator().manual_seed(11 + D + 2 * causal)
    q, k, v = (torch.randn(B, S, H, D, generator=g).to(dtype).to(DEV) for _ in range(3))
    keep = torch.zeros(B, S, dtype=torch.bool)
    for b in range(B):
        lo = int(torch.randint(0, 150, (1,), generator=g)) if b % 2 == 0 else 0    # left padding
        hi = S - (int(torch.randint(0, 150, (1,), generator=g)) if b % 2 == 1 else 0)  # right padding
        keep[b, lo:hi] = True
    keep[B - 1] = True  # one row with no padding
    keep_d = keep.to(DEV)
    qp, idx, cu, ms = ops.unpad_input(q, keep_d)
    kp, _, _, _ = ops.unpad_input(k, keep_d)
    vp, _, _, _ = ops.unpad_input(v, keep_d)
    assert ops.fa3_varlen_route(qp, kp, vp, cu, cu, ms, ms, causal=causal) == ("fwd5" if D <= 64 else "fwd3")
    o_var = ops.pad_input(ops.flash_attention_varlen(qp, kp, vp, cu, cu, ms, ms, causal=causal), idx, B, S)
    o_dense = ops.flash_attention(q, k, v, mask=keep_d, causal=causal)
    assert ops.fa3_route(q, k, v, causal=causal, keep_mask=keep_d[:, None, None, :]) == "fwd1_keep"
    assert (o_var[~keep_d] == 0).all(), "padding rows of pad_input's output are not zero"
    ref, ref_lse = ac.reference(q, k, v, causal=causal, keep_mask=keep[:, None, None, :])
    fam = "fwd5" if D <= 64 else "fwd3"
    for b in range(B):
        rows = keep[b].nonzero().flatten()
        r, rl = ref[b, rows][None], ref_lse[b][:, rows][None]
        ac.check(o_var[b, rows.to(DEV)][None], r, dtype, fam, ref_lse=rl, what=f"keep varlen b{b} causal={causal}")
        ac.check(o_dense[b, rows.to(DEV)][None], r, dtype, "fwd1_keep", ref_lse=rl, what=f"keep dense b{b} causal={causal}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_varlen_cuda_graph(dtype):
    """One capture and replay under torch.cuda.graph gives the eager result."""
    ops = _ops()
    lens = [300, 1, 700, 0, 129]
    g = torch.Generator().manual_seed(5)
    T = sum(lens)
    q, k, v = (torch.randn(T, 4, 64, generator=g).to(dtype).to(DEV) for _ in range(3))
    cu = _cu(lens)
    want, want_lse = ops.flash_attention_varlen(q, k, v, cu, cu, 700, 700, causal=True, return_lse=True)
    out = torch.empty_like(q)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up (attribute set-up) outside the capture
        ops.flash_attention_varlen(q, k, v, cu, cu, 700, 700, causal=True, out=out)
    torch.cuda.current_stream().wait_stream(s)
    out.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, lse = ops.flash_attention_varlen(q, k, v, cu, cu, 700, 700, causal=True, return_lse=True, out=out)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want) and torch.equal(lse, want_lse)

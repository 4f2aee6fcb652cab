"""Attention forward over the paged KV cache (ops.flash_attention_varlen_paged, mio_fa3_fwd_paged) and the many-token cache
write (ops.reshape_and_cache_varlen).

Every attention case asserts ops.fa3_paged_route first.  The paged kernels run the varlen kernels' bodies on the same tiles
in the same order, so after gathering each sequence's pages into contiguous K / V (plain torch indexing) the paged output
and lse must be bitwise equal to ops.flash_attention_varlen's; every sequence is also checked against the fp64 oracle
(_attn_check, bottom-right causal: q_offset = Lk - Lq) at the bars of the route's family.  o and lse carry guard rows that
must come back unchanged.
"""
import ctypes

import pytest
import torch

import _attn_check as ac

pytestmark = pytest.mark.gpu

DEV = "cuda"
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


def _paged_cache(dtype, lens_k, *, bs, Hkv, D, L=1, shared=0, spare=1, g=None):
    """A random cache (every layer finite data) and a table of randomly permuted pages, with `spare` allocated pages past
    each sequence's last; sequences 0 and 1 share their first `shared` pages (a common prefix)."""
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
    kc = torch.randn(nb, L, bs, Hkv, D, generator=g).to(dtype)
    vc = torch.randn(nb, L, bs, Hkv, D, generator=g).to(dtype)
    return kc.to(DEV), vc.to(DEV), bt.to(DEV)


def _gather(kc, vc, bt, lens, layer):
    bs = kc.shape[2]
    ks, vs = [], []
    for b, n in enumerate(lens):
        pos = torch.arange(n, device=DEV)
        pages, slots = bt[b, pos // bs].long(), pos % bs
        ks.append(kc[pages, layer, slots])
        vs.append(vc[pages, layer, slots])
    return torch.cat(ks), torch.cat(vs)


def run_paged(dtype, lens_q, lens_k, *, H=2, Hkv=None, D=64, causal=False, bs=64, L=1, layer=0, shared=0, spare=1,
              used_extra=None, max_k=None, seed=0, what=""):
    """One flash_attention_varlen_paged launch through the C ABI with guarded o / lse; route asserted, guards checked,
    bitwise equality with flash_attention_varlen on the gathered pages, every sequence against the oracle."""
    from mio import _lib
    ops = _ops()
    Hkv = H if Hkv is None else Hkv
    g = torch.Generator().manual_seed(seed * 7919 + sum(lens_q) * 31 + sum(lens_k) * 17 + D + bs)
    # lens_k: keys written per sequence; seqused_k = lens_k (+ used_extra); max_k cuts
    kc, vc, bt = _paged_cache(dtype, lens_k, bs=bs, Hkv=Hkv, D=D, L=L, shared=shared, spare=spare, g=g)
    used = list(lens_k) if used_extra is None else [n + e for n, e in zip(lens_k, used_extra)]
    mk = max(used + [1]) if max_k is None else max_k
    eff = [min(n, mk, bt.shape[1] * bs) for n in used]
    B, Tq = len(lens_q), sum(lens_q)
    q = torch.randn(Tq, H, D, generator=g).to(dtype).to(DEV)
    cu_q = _cu(lens_q)
    sk = torch.tensor(used, dtype=torch.int32, device=DEV)
    mq = max(lens_q + [1])
    route = ops.fa3_paged_route(q, kc, vc, bt, cu_q, sk, mq, mk, layer_idx=layer, causal=causal, return_lse=True)
    want = "empty" if Tq == 0 else ("fwd5" if D <= 64 else "fwd3")
    assert route == want, f"{what}: route {route}, expected {want}"

    sent = torch.tensor(-12345.0).to(dtype).item()
    obuf = torch.full((GUARD + Tq + GUARD, H, D), sent, dtype=dtype, device=DEV)
    lbuf = torch.full((GUARD + H * Tq + GUARD,), -54321.0, dtype=torch.float32, device=DEV)
    out = obuf[GUARD:GUARD + Tq]
    p, out, _lse, keep = ops._paged_params(q, kc, vc, bt, cu_q, sk, mq, mk, layer_idx=layer, causal=causal,
                                           return_lse=True, out=out)
    p.lse = lbuf.data_ptr() + 4 * GUARD
    _lib.check(_lib.lib.mio_fa3_fwd_paged(ctypes.byref(p), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert (obuf[:GUARD] == sent).all() and (obuf[GUARD + Tq:] == sent).all(), f"{what}: o guard rows overwritten"
    assert (lbuf[:GUARD] == -54321.0).all() and (lbuf[GUARD + H * Tq:] == -54321.0).all(), f"{what}: lse guard overwritten"
    lse = lbuf[GUARD:GUARD + H * Tq].view(H, Tq)

    # the same problem on contiguous K / V gathered from the pages
    k, v = _gather(kc, vc, bt, eff, layer)
    ov, lv = ops.flash_attention_varlen(q, k, v, cu_q, _cu(eff), mq, max(eff + [1]), causal=causal, return_lse=True)
    assert torch.equal(out, ov), f"{what}: output differs from flash_attention_varlen on the gathered pages"
    assert torch.equal(lse, lv), f"{what}: lse differs from flash_attention_varlen on the gathered pages"

    for b in range(B):
        q0, Lq, k0, Lk = sum(lens_q[:b]), lens_q[b], sum(eff[:b]), eff[b]
        if Lq == 0:
            continue
        qb, kb, vb = q[q0:q0 + Lq][None], k[k0:k0 + Lk][None], v[k0:k0 + Lk][None]
        ob, lb = out[q0:q0 + Lq][None], lse[:, q0:q0 + Lq][None]
        ref, ref_lse = ac.reference(qb, kb, vb, causal=causal, q_offset=Lk - Lq, device=DEV)
        ac.check(ob, ref, dtype, route, lse=lb, ref_lse=ref_lse, what=f"{what} seq {b} (Lq {Lq}, Lk {Lk})")
    return out, lse


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [32, 64, 80, 128])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("ratio", [1, 4, 8])
def test_paged_matches_varlen_bitwise(dtype, D, causal, ratio):
    """Chunk-over-prefix shapes: queries shorter than, equal to and longer than the cached keys."""
    run_paged(dtype, [300, 1, 129, 256], [700, 64, 129, 1000], H=8, Hkv=8 // ratio, D=D, causal=causal,
              what=f"D{D} causal={causal} gqa {ratio}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("bs", [64, 128, 256])
def test_paged_page_geometry(dtype, D, bs):
    """Block sizes 64 / 128 / 256 on permuted pages, a shared prefix (sequences 0 and 1 share their first pages), layer 1
    of a 3-layer cache whose other layers hold different data, and spare pages past each sequence."""
    run_paged(dtype, [200, 130, 77], [900, 1000, 333], H=4, Hkv=2, D=D, causal=True, bs=bs, L=3, layer=1, shared=2,
              spare=2, what=f"geometry bs{bs} D{D}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [64, 96])
@pytest.mark.parametrize("causal", [False, True])
def test_paged_edges(dtype, D, causal):
    """Lq = 1, Lq > Lk (rows without a visible key), Lk = 0, Lk not a multiple of 64, seqused_k shorter than the
    allocated pages, max_seqlen_k cutting the longest sequence."""
    run_paged(dtype, [1, 500, 40, 7, 300, 65], [1000, 100, 0, 63, 777, 4100], H=2, D=D, causal=causal, spare=2,
              used_extra=[0, -37, 0, -20, 0, 0], max_k=3000, what=f"edges D{D} causal={causal}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_paged_empty_batch(dtype):
    ops = _ops()
    kc = torch.zeros(4, 1, 64, 2, 64, dtype=dtype, device=DEV)
    q = torch.zeros(0, 2, 64, dtype=dtype, device=DEV)
    bt = torch.zeros(1, 2, dtype=torch.int32, device=DEV)
    sk = torch.tensor([10], dtype=torch.int32, device=DEV)
    cu = torch.tensor([0, 0], dtype=torch.int32, device=DEV)
    assert ops.fa3_paged_route(q, kc, kc, bt, cu, sk, 0, 10) == "empty"
    assert ops.flash_attention_varlen_paged(q, kc, kc, bt, cu, sk, 0, 10).shape == (0, 2, 64)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bs", [16, 64, 256])
def test_reshape_and_cache_varlen_byte_exact(dtype, bs):
    """Many tokens per sequence into permuted pages of layer 1 of 2; context_lengths after the append.  Only the written
    positions change, byte for byte; positions past a table row are skipped; a sequence with no new tokens writes
    nothing."""
    ops = _ops()
    g = torch.Generator().manual_seed(bs)
    Hkv, D, L, layer = 2, 64, 2, 1
    new = [300, 0, 1, 77, 5]
    ctx_after = [300, 40, 1000, 77, 8 * bs + 3]  # the last runs past its 8-page table row
    width = 8 if bs >= 64 else 80
    nb = len(new) * width + 2
    perm = torch.randperm(nb, generator=g)[:len(new) * width].view(len(new), width).to(torch.int32)
    kc = torch.randn(nb, L, bs, Hkv, D, generator=g).to(dtype)
    vc = torch.randn(nb, L, bs, Hkv, D, generator=g).to(dtype)
    T = sum(new)
    kv = torch.randn(T, 2, Hkv, 2 * D, generator=g).to(dtype)
    key, val = kv[:, 0, :, :D], kv[:, 1, :, D:]  # strided views
    ek, ev = kc.clone(), vc.clone()
    t = 0
    for b, n in enumerate(new):
        for i in range(n):
            pos = ctx_after[b] - n + i
            if 0 <= pos and pos // bs < width:
                ek[perm[b, pos // bs], layer, pos % bs] = key[t]
                ev[perm[b, pos // bs], layer, pos % bs] = val[t]
            t += 1
    kcd, vcd = kc.to(DEV), vc.to(DEV)
    ops.reshape_and_cache_varlen(key.to(DEV), val.to(DEV), kcd, vcd, perm.to(DEV), _cu(new),
                                 torch.tensor(ctx_after, dtype=torch.int32, device=DEV), bs, layer)
    torch.cuda.synchronize()
    assert torch.equal(kcd.cpu().view(torch.int16), ek.view(torch.int16))
    assert torch.equal(vcd.cpu().view(torch.int16), ev.view(torch.int16))


def _dense_ref(q, k, v):
    """fp64 causal attention of q [Lq, H, D] as the last Lq queries over k / v [Lk, Hkv, D]."""
    return ac.reference(q[None], k[None], v[None], causal=True, q_offset=k.shape[0] - q.shape[0], device=DEV)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [64, 128])
def test_chunked_prefill_then_decode_with_paged_kv_cache(dtype, D):
    """PagedKVCache drives a chunked prefill of ragged prompts (chunks of 256: reshape_and_cache_varlen, then
    flash_attention_varlen_paged causal) and a few decode steps (reshape_and_cache + paged_attention_forward).  Every
    output row matches dense causal attention over the whole sequence so far."""
    ops = _ops()
    from mio.baseline.inference import PagedKVCache
    g = torch.Generator().manual_seed(D)
    H, Hkv, L, layer, bs, chunk = 4, 2, 2, 1, 64, 256
    prompts = [300, 1000, 1537]
    pc = PagedKVCache(num_blocks=64, block_size=bs, num_layers=L, num_heads=Hkv, head_dim=D, dtype=dtype, device=DEV)
    kc, vc = pc.get_physical_caches()
    seqs = list(range(len(prompts)))
    K = [torch.randn(n + 4, Hkv, D, generator=g).to(dtype).to(DEV) for n in prompts]
    V = [torch.randn(n + 4, Hkv, D, generator=g).to(dtype).to(DEV) for n in prompts]
    Q = [torch.randn(n + 4, H, D, generator=g).to(dtype).to(DEV) for n in prompts]
    done = [0] * len(prompts)
    while any(d < n for d, n in zip(done, prompts)):
        step = [min(chunk, n - d) for d, n in zip(done, prompts)]
        for s in seqs:
            pc.allocate_blocks_for_sequence(s, done[s] + step[s])
        bt, cl, mx = pc.kernel_metadata(seqs)
        cu = _cu(step)
        k_new = torch.cat([K[s][done[s]:done[s] + step[s]] for s in seqs])
        v_new = torch.cat([V[s][done[s]:done[s] + step[s]] for s in seqs])
        q_new = torch.cat([Q[s][done[s]:done[s] + step[s]] for s in seqs])
        ops.reshape_and_cache_varlen(k_new, v_new, kc, vc, bt, cu, cl, bs, layer)
        assert ops.fa3_paged_route(q_new, kc, vc, bt, cu, cl, max(step), mx, layer_idx=layer, causal=True) == \
            ("fwd5" if D <= 64 else "fwd3")
        o, lse = ops.flash_attention_varlen_paged(q_new, kc, vc, bt, cu, cl, max(step), mx, layer_idx=layer, causal=True,
                                                  return_lse=True)
        for s in seqs:
            if step[s] == 0:
                continue
            a = sum(step[:s])
            e = done[s] + step[s]
            ref, ref_lse = _dense_ref(Q[s][done[s]:e], K[s][:e], V[s][:e])
            ac.check(o[a:a + step[s]][None], ref, dtype, "fwd5" if D <= 64 else "fwd3", lse=lse[:, a:a + step[s]][None],
                     ref_lse=ref_lse, what=f"prefill seq {s} rows {done[s]}..{e}")
        done = [d + n for d, n in zip(done, step)]
    for t in range(4):  # decode through the existing single-token path
        for s in seqs:
            pc.append_token(s)
        bt, cl, mx = pc.kernel_metadata(seqs)
        kk = torch.stack([K[s][prompts[s] + t] for s in seqs])[:, None]
        vv = torch.stack([V[s][prompts[s] + t] for s in seqs])[:, None]
        ops.reshape_and_cache(kk, vv, kc, vc, bt, cl, bs, layer)
        q = torch.stack([Q[s][prompts[s] + t] for s in seqs])[:, :, None]  # [B, H, 1, D]
        o = torch.empty_like(q)
        ops.paged_attention_forward(q, o, kc, vc, bt, cl, bs, mx, layer)
        for s in seqs:
            e = prompts[s] + t + 1
            ref, _ = _dense_ref(Q[s][e - 1:e], K[s][:e], V[s][:e])
            err = (o[s].permute(1, 0, 2).double() - ref[0].to(o.device)).norm() / ref.norm()
            assert err < 4 * ac.U[dtype], f"decode seq {s} step {t}: relative error {err:.3g}"
    for s in seqs:
        pc.free_sequence(s)


@pytest.mark.parametrize("dtype", DTYPES)
def test_paged_prefill_graph_capture(dtype):
    """The cache write and the paged attention captured in one CUDA graph; inputs refilled in place and replayed equal
    the eager result."""
    ops = _ops()
    g = torch.Generator().manual_seed(11)
    H, Hkv, D, bs, L = 4, 2, 64, 128, 1
    ctx_before = [500, 129, 0]
    new = [256, 100, 1]
    after = [a + n for a, n in zip(ctx_before, new)]
    width = max((n + bs - 1) // bs for n in after)
    nb = width * len(new) + 1
    bt = torch.randperm(nb, generator=g)[:width * len(new)].view(len(new), width).to(torch.int32).to(DEV)
    kc = torch.randn(nb, L, bs, Hkv, D, generator=g).to(dtype).to(DEV)
    vc = torch.randn(nb, L, bs, Hkv, D, generator=g).to(dtype).to(DEV)
    T = sum(new)
    cu, cl = _cu(new), torch.tensor(after, dtype=torch.int32, device=DEV)
    q = torch.empty(T, H, D, dtype=dtype, device=DEV)
    k_new = torch.empty(T, Hkv, D, dtype=dtype, device=DEV)
    v_new = torch.empty(T, Hkv, D, dtype=dtype, device=DEV)
    out = torch.empty(T, H, D, dtype=dtype, device=DEV)

    def step():
        ops.reshape_and_cache_varlen(k_new, v_new, kc, vc, bt, cu, cl, bs, 0)
        ops.flash_attention_varlen_paged(q, kc, vc, bt, cu, cl, max(new), max(after), causal=True, out=out)

    def fill(seed):
        gg = torch.Generator().manual_seed(seed)
        for t in (q, k_new, v_new):
            t.copy_(torch.randn(t.shape, generator=gg).to(dtype))

    fill(1)
    kc0, vc0 = kc.clone(), vc.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()  # warm-up (first launch sets kernel attributes outside the capture)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    fill(2)
    kc.copy_(kc0)
    vc.copy_(vc0)
    graph.replay()
    torch.cuda.synchronize()
    o_graph, kc_graph = out.clone(), kc.clone()
    kc.copy_(kc0)
    vc.copy_(vc0)
    step()
    torch.cuda.synchronize()
    assert torch.equal(o_graph, out)
    assert torch.equal(kc_graph, kc)

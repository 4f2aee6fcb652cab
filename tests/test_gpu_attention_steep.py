"""Attention prefill on scores that move the softmax reference (tests/_attn_steep.py), every route and launch form.

randn data at scale 1/sqrt(D) never moves a row's reference after its first tile, so the rare branches of the prefill
kernels -- move_ref of fa3_fwd5_body.inc / fa3_fwd3_body.inc, update of fa3_fwd3_body.inc, the ballot of fa3_fwd_kernel.h --
ran in their tile-0 form only.  The cases of _attn_steep.CASES (profiles `spikes`, `rising`, `falling`; dense, ring carry,
packed varlen, paged 16-bit (block sizes 64 and 128: the paged kernels take multiples of 64) and fp8, sliding window;
non-default softmax_scale on every launch that is not K-prescaled) make them run mid-stream;
tests/test_attn_steep_host.py proves on the CPU that the inputs do what they are meant to.
Every case asserts its route first, then judges each output row against the fp64 reference on the same tensors at the
unchanged bars of _attn_check.BARS for the route's family (_attn_steep.judge), and lse by the absolute bar u + 2^-13
(_attn_steep.lse_bar).  A failure names the worst row and the tiles at which move_plan says it moved.  Outputs carry guard
rows of a sentinel that must come back unchanged.

Measured by one run of this file on the MI355X (234 tests, 5.5 s of pytest wall time; tests/test_gpu_attention_matrix.py
takes about 3 s): the largest value over the judged results of each (dtype, family), output rows in units of u against the
family's bar in _attn_check.BARS, |lse - ref| absolute against 4.0e-3 (bf16) / 6.1e-4 (fp16).  Every family sits on steep
data where it sits on randn data; no kernel defect was found.

  dtype  family            n   worst (bar)   mean (bar)    16-row group (bar)  |lse - ref|
  bf16   fwd5             72   1.073 (2.9)   0.569 (1.2)   0.632 (1.8)         3.21e-03
  bf16   fwd5_kpre         6   0.980 (3.7)   0.584 (1.21)  0.634 (1.5)         1.79e-03
  bf16   fwd5_kpre_carry   4   0.839 (2.1)   0.561 (1.21)  0.608 (1.2)         2.57e-03
  bf16   fwd5_kpre_oblk    6   0.980 (1.9)   0.584 (1.17)  0.634 (1.3)         (no lse)
  bf16   fwd3             76   0.828 (1.8)   0.561 (1.18)  0.601 (1.4)         2.95e-03
  bf16   fwd3_kpre         6   0.824 (1.8)   0.579 (1.17)  0.618 (1.3)         1.62e-03
  bf16   fwd1             17   1.036 (2.1)   0.568 (1.24)  0.612 (1.4)         9.37e-06
  bf16   fwd1_add          6   1.006 (2.2)   0.512 (1.15)  0.573 (1.4)         1.09e-05
  bf16   fwd1_keep         6   0.939 (1.8)   0.559 (1.17)  0.606 (1.4)         1.00e-05
  fp16   fwd5             72   0.955 (2.9)   0.575 (1.21)  0.646 (1.6)         2.28e-04
  fp16   fwd5_kpre         6   0.913 (3.1)   0.581 (1.19)  0.637 (1.4)         1.64e-04
  fp16   fwd5_kpre_carry   4   0.798 (2.0)   0.558 (1.21)  0.601 (1.4)         3.13e-04
  fp16   fwd5_kpre_oblk    6   0.913 (1.9)   0.581 (1.17)  0.637 (1.3)         (no lse)
  fp16   fwd3             76   0.805 (1.9)   0.560 (1.18)  0.605 (1.6)         4.19e-04
  fp16   fwd3_kpre         6   0.913 (1.8)   0.578 (1.17)  0.613 (1.3)         1.81e-04
  fp16   fwd1             17   1.032 (2.5)   0.575 (1.22)  0.615 (1.3)         8.91e-06
  fp16   fwd1_add          6   1.071 (2.1)   0.510 (1.16)  0.588 (1.3)         1.11e-05
  fp16   fwd1_keep         6   0.858 (1.9)   0.557 (1.18)  0.597 (1.2)         9.03e-06
(fwd5 / fwd3 include the varlen, paged, fp8-cache and windowed launches, one judged result per sequence; a carry is judged
twice, the written output and the fp32 carry.)
"""
import pytest
import torch

import _attn_steep as st

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
GUARD = 8
SENT = -12345.0


def _ops():
    from mio import ops
    return ops


def _cu(lens):
    c = [0]
    for n in lens:
        c.append(c[-1] + n)
    return torch.tensor(c, dtype=torch.int32, device=DEV)


def _by_group(*groups):
    return [pytest.param(c, id=c.id) for c in st.CASES if c.group in groups]


def _unblock(ob, B, Sq, H, D):
    M = ob.shape[0]
    return ob.view(M // 256, H * D // 32, 256, 32).permute(0, 2, 1, 3).reshape(M, H * D)[:B * Sq].view(B, Sq, H, D)


def _guarded(shape, dtype, dim):
    """A sentinel-filled buffer with GUARD extra rows on each side of `dim`, and the view of the rows between them."""
    full = list(shape)
    full[dim] += 2 * GUARD
    buf = torch.full(full, SENT, dtype=dtype, device=DEV)
    return buf, buf.narrow(dim, GUARD, shape[dim])


def _guards_intact(buf, dim, n, what):
    sent = torch.tensor(SENT).to(buf.dtype)
    assert (buf.narrow(dim, 0, GUARD) == sent).all() and (buf.narrow(dim, GUARD + n, GUARD) == sent).all(), \
        f"{what}: guard rows overwritten"


# ---------------------------------------------------------------------------------------------------------------------
# dense ops.fa3_fwd (also the windowed form)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", _by_group("dense", "window_dense"))
def test_dense(dtype, case):
    ops = _ops()
    prob, = st.build(case, dtype)
    qg, kg, vg = prob.q.to(DEV), prob.k.to(DEV), prob.v.to(DEV)
    B, Sq, H, D = prob.q.shape
    keep, add = prob.extra["keep"], prob.extra["add"]
    kw = dict(causal=case.causal, q_offset=prob.extra["off"], softmax_scale=case.scale, k_prescaled=case.kpre,
              out_blocked=case.oblk, window_size=case.window, keep_mask=None if keep is None else keep.to(DEV),
              additive_mask=None if add is None else add.to(DEV))
    buf = out = None
    if not case.oblk:  # (the blocked output is allocated by the launch)
        buf, out = _guarded((B, Sq, H, D), dtype, 1)
    assert ops.fa3_route(qg, kg, vg, out=out, return_lse=not case.oblk, **kw) == case.route, case.id
    res = ops.fa3_fwd(qg, kg, vg, out=out, return_lse=not case.oblk, **kw)
    torch.cuda.synchronize()
    if case.oblk:
        o, lse = _unblock(res, B, Sq, H, D), None
    else:
        o, lse = res
        assert o.data_ptr() == out.data_ptr()
        _guards_intact(buf, 1, Sq, case.id)
    ref, rlse = st.reference(prob)
    st.judge(o.cpu(), None if lse is None else lse.cpu(), ref, rlse, dtype, case.route, case.id, lambda: st.plan(case, dtype, prob))


# ---------------------------------------------------------------------------------------------------------------------
# the (o_acc, lse) carry across K shards: B = 2, so the shard views of K / V are strided in the batch
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", _by_group("carry"))
def test_carry(dtype, case):
    ops = _ops()
    prob, = st.build(case, dtype)
    qg, kg, vg = prob.q.to(DEV), prob.k.to(DEV), prob.v.to(DEV)
    B, Sq, H, D = prob.q.shape
    acc = torch.empty(B, Sq, H, D, dtype=torch.float32, device=DEV)
    lse = torch.empty(B, H, Sq, dtype=torch.float32, device=DEV)
    buf, out = _guarded((B, Sq, H, D), dtype, 1)
    parts = st.shards(case, prob)
    for i, (lo, hi) in enumerate(parts):
        last = i == len(parts) - 1
        kw = dict(softmax_scale=case.scale, k_prescaled=case.kpre, k_offset=lo, o_acc=acc, lse=lse, carry_in=i > 0,
                  write_out=last, out=out if last else None)
        ks, vs = kg[:, lo:hi], vg[:, lo:hi]
        assert not ks.is_contiguous()
        assert ops.fa3_route(qg, ks, vs, **kw) == case.route, f"{case.id} shard {i}"
        ops.fa3_fwd(qg, ks, vs, **kw)
    torch.cuda.synchronize()
    _guards_intact(buf, 1, Sq, case.id)
    ref, rlse = st.reference(prob)
    pl = lambda: st.plan(case, dtype, prob)  # noqa: E731
    st.judge(out.cpu(), lse.cpu(), ref, rlse, dtype, case.route, case.id, pl)
    st.judge(acc.cpu(), None, ref, rlse, dtype, case.route, case.id + " (fp32 carry)", pl)


# ---------------------------------------------------------------------------------------------------------------------
# packed varlen, paged (16-bit and fp8 cache), and their windowed forms
# ---------------------------------------------------------------------------------------------------------------------
def _pack(probs):
    return (torch.cat([p.q[0] for p in probs]).to(DEV), torch.cat([p.k[0] for p in probs]).to(DEV),
            torch.cat([p.v[0] for p in probs]).to(DEV))


def _judge_sequences(case, dtype, probs, out, lse):
    q0 = 0
    for b, prob in enumerate(probs):
        Lq = prob.q.shape[1]
        ref, rlse = st.reference(prob)
        st.judge(out[q0:q0 + Lq][None].cpu(), lse[:, q0:q0 + Lq][None].cpu(), ref, rlse, dtype, case.route,
                 f"{case.id} seq {b} (Lq {Lq}, Lk {prob.k.shape[1]})", lambda prob=prob: st.plan(case, dtype, prob))
        q0 += Lq


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", _by_group("varlen", "window_varlen"))
def test_varlen(dtype, case):
    ops = _ops()
    probs = st.build(case, dtype)
    q, k, v = _pack(probs)
    cu_q, cu_k = _cu(case.lens_q), _cu(case.lens_k)
    mq, mk = max(case.lens_q), max(case.lens_k)
    buf, out = _guarded(tuple(q.shape), dtype, 0)
    kw = dict(causal=case.causal, softmax_scale=case.scale, return_lse=True, out=out, window_size=case.window)
    assert ops.fa3_varlen_route(q, k, v, cu_q, cu_k, mq, mk, **kw) == case.route, case.id
    o, lse = ops.flash_attention_varlen(q, k, v, cu_q, cu_k, mq, mk, **kw)
    torch.cuda.synchronize()
    assert o.data_ptr() == out.data_ptr()
    _guards_intact(buf, 0, q.shape[0], case.id)
    _judge_sequences(case, dtype, probs, o, lse)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", _by_group("paged", "kv8", "window_paged"))
def test_paged(dtype, case):
    """The context (a prefix in front of every chunk) goes into permuted pages through reshape_and_cache_varlen -- with
    k_scale 0.05 / v_scale 0.08 into an fp8 cache whose other bytes are NaN -- and the reference runs over what the cache
    then holds (for fp8: the CPU quantisation formula, dequantised)."""
    ops = _ops()
    probs = st.build(case, dtype)
    q, k, v = _pack(probs)
    bs, Hkv, D, L, layer = case.bs, case.Hkv, case.D, 2, 1
    g = torch.Generator().manual_seed(case.bs + D)
    npages = [(n + bs - 1) // bs + 1 for n in case.lens_k]  # one spare page past each sequence's last
    nb = sum(npages) + 3
    perm = torch.randperm(nb, generator=g)
    bt = torch.zeros(len(npages), max(npages), dtype=torch.int32)
    nxt = 0
    for b, n in enumerate(npages):
        bt[b, :n] = perm[nxt:nxt + n]
        nxt += n
    bt = bt.to(DEV)
    scales = {}
    if case.group == "kv8":
        kc = torch.full((nb, L, bs, Hkv, D), 0x7F, dtype=torch.uint8, device=DEV).view(st.F8)
        vc = torch.full((nb, L, bs, Hkv, D), 0xFF, dtype=torch.uint8, device=DEV).view(st.F8)
        ks, vs = st.KV8_SCALES
        scales = dict(k_scale=torch.tensor([0.7, ks], device=DEV), v_scale=torch.tensor([1.3, vs], device=DEV))
    else:
        kc = torch.randn(nb, L, bs, Hkv, D, generator=g).to(dtype).to(DEV)
        vc = torch.randn(nb, L, bs, Hkv, D, generator=g).to(dtype).to(DEV)
    used = torch.tensor(case.lens_k, dtype=torch.int32, device=DEV)
    ops.reshape_and_cache_varlen(k, v, kc, vc, bt, _cu(case.lens_k), used, bs, layer, **scales)
    cu_q = _cu(case.lens_q)
    mq, mk = max(case.lens_q), max(case.lens_k)
    buf, out = _guarded(tuple(q.shape), dtype, 0)
    kw = dict(layer_idx=layer, causal=case.causal, softmax_scale=case.scale, return_lse=True, out=out,
              window_size=case.window, **scales)
    assert ops.fa3_paged_route(q, kc, vc, bt, cu_q, used, mq, mk, **kw) == case.route, case.id
    o, lse = ops.flash_attention_varlen_paged(q, kc, vc, bt, cu_q, used, mq, mk, **kw)
    torch.cuda.synchronize()
    assert o.data_ptr() == out.data_ptr()
    _guards_intact(buf, 0, q.shape[0], case.id)
    if case.group == "kv8":  # the cache holds what the CPU formula says (the reference's keys and values)
        p0 = probs[0]
        pos = torch.arange(p0.k.shape[1], device=DEV)
        got = kc[bt[0, pos // bs].long(), layer, pos % bs].double().cpu() * st.KV8_SCALES[0]
        assert torch.equal(got, p0.kk[0]), "the fp8 cache differs from the CPU quantisation formula"
    _judge_sequences(case, dtype, probs, o, lse)

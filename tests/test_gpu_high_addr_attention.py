"""Attention prefill where the bytes a launch reads and writes lie beyond 2^31, 2^32 and 2^33 bytes of the tensors it is handed:
paged prefill over 16-bit and fp8 caches of just over 8 GiB (plain and windowed), packed varlen and dense launches on strided
views into wide buffers, and the two sides of the 4 GiB span limit of the pipelined kernels (csrc/fa3_route.h, span32).

The placements come from tests/_high_addr.py (its docstring has the rules, tests/test_high_addr_host.py checks them): every
byte of the large allocations is 0xFF (NaN as bf16, fp16 and e4m3fn) except the few live rows, and a truncated, sign-flipped
or wrapped address of any live row lies inside the same allocation, on filler -- a wrong read gives a non-finite output, a
wrong write is counted by the scan after the launch; nothing here can reach memory outside its allocations.

Two judgements per case, after the route is asserted: (a) output and lse are bit for bit those of the same launch on a compact
copy of the same data (a small cache holding the same pages at low numbers, contiguous tensors); (b) the compact result is
judged by _attn_check.check against the fp64 reference at the unchanged _attn_check.BARS of the route's family.  The fwd1
fallback past the span limit has no compact twin on the same kernel and is judged by (b) on its own result.

Span case (ii) (Sk = 100, the largest admitted stride): rows 51 .. 63 of key tile 0 have per-lane byte offsets row * stride * 2
above 2^31, computed as `int` in csrc/fa3_fwd3_body.inc / fa3_fwd5_body.inc and handed as the 32-bit VGPR offset of
`global_load_lds_dwordx4 v, s[base]`.  Why that offset would be zero-extended: unverified from a text when this test was
written -- no ISA manual or LLVM AMDGPU usage document ships with the toolchain; the public CDNA3 ISA guide describes the SADDR
form of GLOBAL as an SGPR base plus a 32-bit unsigned VGPR offset plus a signed immediate, which is what the kernels rely on.
test_span_limit is the first run of it: the view starts 4 GiB into its allocation, so a sign-extended
offset would read filler 4 GiB lower, not foreign memory.

Measured on the MI355X (one run of this file, 43 tests in 20.3 s of pytest wall time; test_stats_table prints this with -s):
the worst value over the file's judgements per (dtype, family), in units of u, over the unchanged bar of _attn_check.BARS.
                          worst row     mean          16-row group  lse                  judgements
  bf16  fwd5              1.068 / 2.9   0.626 / 1.2   0.763 / 1.8   1.20e-3 / 2.2e-3     73
  bf16  fwd3              0.976 / 1.8   0.612 / 1.18  0.712 / 1.4   1.10e-3 / 2.4e-3     73
  bf16  fwd5_kpre         0.932 / 3.7   0.589 / 1.21  0.644 / 1.5   1.15e-3 / 2.9e-3      6
  bf16  fwd5_kpre_oblk    0.912 / 1.9   0.561 / 1.17  0.639 / 1.3   (no lse)              4
  bf16  fwd1              0.882 / 2.1   0.592 / 1.24  0.633 / 1.4   1.54e-7 / 5.2e-7      8
  fp16  fwd5              1.011 / 2.9   0.667 / 1.21  0.773 / 1.6   1.56e-4 / 3.7e-4     73
  fp16  fwd3              0.956 / 1.9   0.655 / 1.18  0.706 / 1.6   1.43e-4 / 3.1e-4     73
  fp16  fwd5_kpre         0.926 / 3.1   0.592 / 1.19  0.644 / 1.4   1.75e-4 / 2.7e-4      6
  fp16  fwd5_kpre_oblk    1.005 / 1.9   0.562 / 1.17  0.644 / 1.3   (no lse)              4
  fp16  fwd1              0.876 / 2.5   0.586 / 1.22  0.628 / 1.3   1.48e-7 / 4.4e-7      8
Every launch on the high addresses was bit-equal to its compact twin; span case (ii) returned finite, bit-equal results on
fwd5 and fwd3 in both dtypes, so the 32-bit lane offset is taken as unsigned on this hardware and fa3_pick_route stays as it is.
"""
import math

import pytest
import torch

import _attn_check as ac
import _high_addr as ha

pytestmark = pytest.mark.gpu

DEV = "cuda"
F8 = torch.float8_e4m3fn
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
LOG2E = 1.4426950408889634
H, HKV, LAYER = ha.H, ha.HKV, ha.LAYER
# (causal, window): plain, causal, a causal window and a two-sided one -- with Lk of several hundred the first pass of the
# windowed kernels starts at a key tile > 0 (FaPageWalkWin::begin_pass), on a high page
MODES = [(False, (-1, -1)), (True, (-1, -1)), (True, (130, 0)), (False, (64, 32))]


def _ops():
    from mio import ops
    return ops


def _cu(lens):
    c = [0]
    for n in lens:
        c.append(c[-1] + n)
    return torch.tensor(c, dtype=torch.int32, device=DEV)


def _family(D):
    return "fwd5" if D <= 64 else "fwd3"


def _ref(q, k, v, causal, window, off, scale):
    """fp64 (o [1,Sq,H,D], lse [1,H,Sq]) on the GPU, keys outside the causal / window band absent; q [Sq,H,D], k / v
    [Sk,Hkv,D] (any float dtype; fp64 for a dequantised fp8 cache); off = Lk - Lq (bottom-right) or q_offset - k_offset."""
    Sq, Hq, D = q.shape
    Sk, Hk = k.shape[0], k.shape[1]
    qd = q.double().permute(1, 0, 2)
    kd = k.double().repeat_interleave(Hq // Hk, dim=1).permute(1, 0, 2)
    vd = v.double().repeat_interleave(Hq // Hk, dim=1).permute(1, 0, 2)
    s = qd @ kd.transpose(-1, -2) * scale
    i = torch.arange(Sq, device=q.device).view(Sq, 1) + off
    j = torch.arange(Sk, device=q.device).view(1, Sk)
    left, right = window
    vis = torch.ones(Sq, Sk, dtype=torch.bool, device=q.device)
    if causal or right >= 0:
        vis &= j <= i + (0 if causal else right)
    if left >= 0:
        vis &= j >= i - left
    s = s.masked_fill(~vis, float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - torch.where(torch.isfinite(lse), lse, torch.zeros_like(lse)).unsqueeze(-1))
    p = torch.where(vis.any(-1).view(1, Sq, 1), p, torch.zeros_like(p))
    return (p @ vd).permute(1, 0, 2)[None].cpu(), lse[None].cpu()


def _judge(o, lse, q, k, v, dtype, family, causal, window, off, scale, what):
    """3(b): one sequence / batch of a compact result (o [Sq,H,D], lse [H,Sq] or None) against the fp64 reference."""
    ro, rl = _ref(q, k, v, causal, window, off, scale)
    ac.check(o[None].cpu(), ro, dtype, family, lse=None if lse is None else lse[None].cpu(), ref_lse=rl, what=what)


def _same(hi, lo, what):
    """3(a): finite, and bit for bit the compact launch's."""
    o_hi, l_hi = hi
    o_lo, l_lo = lo
    assert torch.isfinite(o_hi).all(), f"{what}: non-finite output ({int((~torch.isfinite(o_hi)).sum())} values)"
    assert torch.equal(o_hi, o_lo), f"{what}: output differs from the launch on the compact copy"
    assert torch.equal(l_hi, l_lo), f"{what}: lse differs from the launch on the compact copy"


# ---- paged prefill ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp8", [False, True], ids=["kv16", "fp8"])
@pytest.mark.parametrize("bs,D", ha.PAGED_GEOM)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_paged_prefill_pages_around_the_boundaries(dtype, bs, D, fp8):
    """flash_attention_varlen_paged at layer 2 of 3-layer caches of just over 8 GiB each: the logical pages of three
    sequences (Lq / Lk 300 / 700, 77 / 77, 1 / 513) alternate between physical pages just below and just above 2^31, 2^32
    and 2^33 bytes; 16-bit and fp8 (per-layer scales, the other layers' different), every mode of MODES."""
    ops = _ops()
    case = ha.paged_attention_case(bs, D, 1 if fp8 else 2)
    info = case.info
    pages, nb, n = info["pages"], info["num_blocks"], len(info["pages"])
    lens_q, lens_k = ha.PAGED_LQ, ha.PAGED_LK
    g = torch.Generator().manual_seed(bs + D + fp8)
    ks, vs = (0.05, 0.08) if fp8 else (1.0, 1.0)
    cdt = F8 if fp8 else dtype
    kd = (torch.randn(n, bs, HKV, D, generator=g) * (10 * ks if fp8 else 1)).to(dtype)
    vd = (torch.randn(n, bs, HKV, D, generator=g) * (10 * vs if fp8 else 1)).to(dtype)
    if fp8:
        from test_gpu_kv8 import _quant_ref
        kd, vd = _quant_ref(kd, ks), _quant_ref(vd, vs)
    kd, vd = kd.to(DEV), vd.to(DEV)
    q = torch.randn(sum(lens_q), H, D, generator=g).to(dtype).to(DEV)
    kw = {}
    if fp8:
        kw = dict(k_scale=torch.tensor([0.7, 0.9, ks], dtype=torch.float32, device=DEV),
                  v_scale=torch.tensor([1.3, 0.4, vs], dtype=torch.float32, device=DEV))
    cu_q, sk = _cu(lens_q), torch.tensor(lens_k, dtype=torch.int32, device=DEV)
    mq, mk = max(lens_q), max(lens_k)
    bufs = ha.allocate(case)
    try:
        shape = (nb, ha.L, bs, HKV, D)
        kc, vc = ha.view(bufs, case, "k_cache", cdt, shape), ha.view(bufs, case, "v_cache", cdt, shape)
        bits = torch.uint8 if fp8 else torch.int16
        for j, page in enumerate(pages):
            kc[page, LAYER].view(bits).copy_(kd[j].view(bits))
            vc[page, LAYER].view(bits).copy_(vd[j].view(bits))
        # the compact twin: the same pages as pages 1 .. n of a small cache (page 0 and the other layers filler)
        width = D * kd.element_size()
        kcs = torch.full((n + 1, ha.L, bs, HKV, width), ha.FILL, dtype=torch.uint8, device=DEV).view(cdt)
        vcs = torch.full((n + 1, ha.L, bs, HKV, width), ha.FILL, dtype=torch.uint8, device=DEV).view(cdt)
        kcs.view(bits)[1:, LAYER] = kd.view(bits)
        vcs.view(bits)[1:, LAYER] = vd.view(bits)
        bt = torch.tensor(ha.block_table(lens_k, bs, pages), dtype=torch.int32, device=DEV)
        bts = torch.tensor(ha.block_table(lens_k, bs, list(range(1, n + 1))), dtype=torch.int32, device=DEV)
        need = ha.pages_needed(lens_k, bs)
        for causal, window in MODES:
            what = f"paged bs{bs} D{D} {'fp8' if fp8 else 'kv16'} causal={causal} w={window}"
            args = dict(layer_idx=LAYER, causal=causal, window_size=window, **kw)
            for c, t in ((kc, bt), (kcs, bts)):
                route = ops.fa3_paged_route(q, c, c, t, cu_q, sk, mq, mk, return_lse=True, **args)
                assert route == _family(D), f"{what}: route {route}"
            hi = ops.flash_attention_varlen_paged(q, kc, vc, bt, cu_q, sk, mq, mk, return_lse=True, **args)
            lo = ops.flash_attention_varlen_paged(q, kcs, vcs, bts, cu_q, sk, mq, mk, return_lse=True, **args)
            _same(hi, lo, what)
            p0 = 0
            for b, (Lq, Lk) in enumerate(zip(lens_q, lens_k)):
                q0 = sum(lens_q[:b])
                kb = kd[p0:p0 + need[b]].reshape(-1, HKV, D)[:Lk]
                vb = vd[p0:p0 + need[b]].reshape(-1, HKV, D)[:Lk]
                if fp8:
                    kb, vb = kb.double() * ks, vb.double() * vs
                _judge(lo[0][q0:q0 + Lq], lo[1][:, q0:q0 + Lq], q[q0:q0 + Lq], kb, vb, dtype, _family(D), causal, window,
                       Lk - Lq, D ** -0.5, f"{what} seq {b}")
                p0 += need[b]
        # the launches read only: every byte of the allocation outside the live pages is still filler
        assert ha.count_not_fill(bufs["kv"]) == ha.live_bytes(kd, vd), f"paged bs{bs} D{D}: the caches were written"
    finally:
        kc = vc = bufs = None
        torch.cuda.empty_cache()


# ---- packed varlen ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_varlen_strided_views_past_4gib(dtype, D):
    """flash_attention_varlen with q, k, v and o strided views (token stride 2^22 + 2048 elements) that start 4 GiB into one
    wide buffer: sequence 0 lies below 4 GiB of each view, sequence 1 across it, sequence 2 above it and across 8 GiB; each
    sequence's K / V span stays under 4 GiB (the route query would refuse otherwise).  lse is compact."""
    ops = _ops()
    case = ha.varlen_case(D)
    lens = ha.VARLEN_LENS
    T, pitch = sum(lens), case.info["pitch"] // 2
    g = torch.Generator().manual_seed(D)
    qc = torch.randn(T, H, D, generator=g).to(dtype).to(DEV)
    kc = torch.randn(T, HKV, D, generator=g).to(dtype).to(DEV)
    vc = torch.randn(T, HKV, D, generator=g).to(dtype).to(DEV)
    cu = _cu(lens)
    bufs = ha.allocate(case)
    try:
        qv = ha.view(bufs, case, "q", dtype, (T, H, D), (pitch, D, 1))
        kv = ha.view(bufs, case, "k", dtype, (T, HKV, D), (pitch, D, 1))
        vv = ha.view(bufs, case, "v", dtype, (T, HKV, D), (pitch, D, 1))
        ov = ha.view(bufs, case, "o", dtype, (T, H, D), (pitch, D, 1))
        qv.copy_(qc), kv.copy_(kc), vv.copy_(vc)
        assert (kv.data_ptr() - bufs["wide"].data_ptr()) >= 1 << 32 and kv.stride(0) * 2 * (lens[0] + lens[1]) > 1 << 32
        for causal, window in MODES:
            what = f"varlen D{D} causal={causal} w={window}"
            ov.view(torch.int16).fill_(-1)
            args = dict(causal=causal, window_size=window)
            for t in ((qv, kv, vv), (qc, kc, vc)):
                assert ops.fa3_varlen_route(*t, cu, cu, max(lens), max(lens), **args) == _family(D), what
            _, lse = ops.flash_attention_varlen(qv, kv, vv, cu, cu, max(lens), max(lens), return_lse=True, out=ov, **args)
            lo = ops.flash_attention_varlen(qc, kc, vc, cu, cu, max(lens), max(lens), return_lse=True, **args)
            oc = ov.contiguous()
            _same((oc, lse), lo, what)
            assert ha.count_not_fill(bufs["wide"]) == ha.live_bytes(qc, kc, vc, oc), f"{what}: bytes outside q, k, v, o changed"
            for b, n in enumerate(lens):
                r = slice(sum(lens[:b]), sum(lens[:b]) + n)
                _judge(lo[0][r], lo[1][:, r], qc[r], kc[r], vc[r], dtype, _family(D), causal, window, 0, D ** -0.5,
                       f"{what} seq {b}")
    finally:
        qv = kv = vv = ov = bufs = None
        torch.cuda.empty_cache()


# ---- dense -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_dense_batches_past_4_and_8_gib(dtype, D):
    """fa3_fwd with B = 3 and batch strides of 4 GiB + 4 MiB for q, k, v and o (batch 1 starts past 2^32 bytes, batch 2 past
    2^33), the four tensors side by side in the rows of one wide buffer, 4 GiB into it: fwd5 / fwd3 plain, causal and
    windowed, and (D 64) fwd5_kpre on pre-scaled K."""
    ops = _ops()
    case = ha.dense_attention_case(D)
    B, S = ha.DENSE_B, ha.DENSE_S
    bp, rp = ha.BATCH_PITCH // 2, case.info["row_bytes"] // 2
    g = torch.Generator().manual_seed(D + 1)
    qc = torch.randn(B, S, H, D, generator=g).to(dtype).to(DEV)
    kc = torch.randn(B, S, HKV, D, generator=g).to(dtype).to(DEV)
    vc = torch.randn(B, S, HKV, D, generator=g).to(dtype).to(DEV)
    scale = 1.0 / math.sqrt(D)
    modes = [(c, w, False) for c, w in MODES[:3]] + ([(False, (-1, -1), True), (True, (-1, -1), True)] if D == 64 else [])
    bufs = ha.allocate(case)
    try:
        qv = ha.view(bufs, case, "q", dtype, (B, S, H, D), (bp, rp, D, 1))
        kv = ha.view(bufs, case, "k", dtype, (B, S, HKV, D), (bp, rp, D, 1))
        vv = ha.view(bufs, case, "v", dtype, (B, S, HKV, D), (bp, rp, D, 1))
        ov = ha.view(bufs, case, "o", dtype, (B, S, H, D), (bp, rp, D, 1))
        qv.copy_(qc), vv.copy_(vc)
        for causal, window, kpre in modes:
            what = f"dense D{D} causal={causal} w={window} kpre={kpre}"
            kk = (kc.float() * (scale * LOG2E)).to(dtype) if kpre else kc
            kv.copy_(kk)
            ov.view(torch.int16).fill_(-1)
            family = "fwd5_kpre" if kpre else _family(D)
            args = dict(causal=causal, k_prescaled=kpre)
            if window != (-1, -1):
                args["window_size"] = window
            assert ops.fa3_route(qv, kv, vv, out=ov, return_lse=True, **args) == family, what
            assert ops.fa3_route(qc, kk, vc, return_lse=True, **args) == family, what
            _, lse = ops.fa3_fwd(qv, kv, vv, out=ov, return_lse=True, **args)
            lo = ops.fa3_fwd(qc, kk, vc, return_lse=True, **args)
            oc = ov.contiguous()
            _same((oc, lse), lo, what)
            assert ha.count_not_fill(bufs["wide"]) == ha.live_bytes(qc, kk, vc, oc), f"{what}: bytes outside q, k, v, o changed"
            for b in range(B):
                _judge(lo[0][b], lo[1][b], qc[b], kk[b], vc[b], dtype, family, causal, window, 0,
                       math.log(2.0) if kpre else scale, f"{what} batch {b}")
    finally:
        qv = kv = vv = ov = bufs = None
        torch.cuda.empty_cache()


# ---- the span limit --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [0, 1], ids=["pipelined", "fwd1"])
@pytest.mark.parametrize("which", ["i", "ii"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_span_limit(dtype, D, which, step):
    """Sq = 200 queries over K / V whose row stride is the largest span32 admits (step 0: fwd5 / fwd3; (i) Sk = 320, the last
    tile's scalar offset is 0.8 * 2^32 and the last row ends one step under 2^32; (ii) Sk = 100, lane offsets of rows 51 .. 63
    of tile 0 lie past 2^31 -- module docstring) and one step of 8 elements larger (step 1: fwd1, the only kernel that sees a
    span of 4 GiB or more).  K and V sit 4 GiB into one allocation with 4 GiB of filler behind them."""
    ops = _ops()
    case = ha.span_case(which, D, step)
    Sk, stride, Sq = case.info["Sk"], case.info["stride"], case.info["Sq"]
    g = torch.Generator().manual_seed(Sk + D)
    qc = torch.randn(1, Sq, 2, D, generator=g).to(dtype).to(DEV)
    kc = torch.randn(1, Sk, 1, D, generator=g).to(dtype).to(DEV)
    vc = torch.randn(1, Sk, 1, D, generator=g).to(dtype).to(DEV)
    family = _family(D) if step == 0 else "fwd1"
    bufs = ha.allocate(case)
    try:
        kv = ha.view(bufs, case, "k", dtype, (1, Sk, 1, D), (Sk * stride, stride, D, 1))
        vv = ha.view(bufs, case, "v", dtype, (1, Sk, 1, D), (Sk * stride, stride, D, 1))
        kv.copy_(kc), vv.copy_(vc)
        assert ha.span32(Sk, kv.stride(1), vv.stride(1)) == (step == 0)
        for causal in (False, True):
            what = f"span ({which}) D{D} stride {stride} causal={causal}"
            off = max(Sk - Sq, 0) if causal else 0   # (i): bottom-right, so that the queries see keys of the last tile
            args = dict(causal=causal, q_offset=off)
            assert ops.fa3_route(qc, kv, vv, return_lse=True, **args) == family, what
            hi = ops.fa3_fwd(qc, kv, vv, return_lse=True, **args)
            assert torch.isfinite(hi[0]).all(), f"{what}: non-finite output ({int((~torch.isfinite(hi[0])).sum())} values)"
            if step == 0:
                assert ops.fa3_route(qc, kc, vc, return_lse=True, **args) == family, what
                _same(hi, ops.fa3_fwd(qc, kc, vc, return_lse=True, **args), what)
            _judge(hi[0][0], hi[1][0], qc[0], kc[0], vc[0], dtype, family, causal, (-1, -1), off, D ** -0.5, what)
        assert ha.count_not_fill(bufs["wide"]) == ha.live_bytes(kc, vc), f"span ({which}) D{D}: K / V buffer was written"
    finally:
        kv = vv = bufs = None
        torch.cuda.empty_cache()


# ---- the blocked output ----------------------------------------------------------------------------------------------------
(OB, OSQ, OH, OHKV, OD), OSLAB = ha.BLOCKED_SHAPE, 512   # B * Sq * H * D = 2^31 + 2^17: o just over 4 GiB


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_dense_blocked_output_past_2_31_elements(dtype):
    """fa3_fwd(k_prescaled=True, out_blocked=True) (fwd5_kpre_oblk) with B * Sq * H * D just over 2^31: the blocked output index
    crosses 2^31 and 2^32 bytes (batches 8192 and 16384, one 256-row block each).  q, k and v repeat one random slab of 512
    batches, so every batch's block is bit-equal to the block of the slab's own launch; the batches on both sides of the two
    boundaries, the last one among them, are judged against the fp64 reference at the family's bars.  About 11 GiB alive."""
    from test_gpu_attention_matrix import _unblock
    ops = _ops()
    assert OB * OSQ * OH * OD > 1 << 31
    g = torch.Generator(device=DEV).manual_seed(7)
    scale = 1.0 / math.sqrt(OD)
    qs = torch.randn(OSLAB, OSQ, OH, OD, generator=g, device=DEV).to(dtype)
    ks = (torch.randn(OSLAB, OSQ, OHKV, OD, generator=g, device=DEV) * (scale * LOG2E)).to(dtype)   # K as the projection hands it over
    vs = torch.randn(OSLAB, OSQ, OHKV, OD, generator=g, device=DEV).to(dtype)
    q = torch.empty(OB, OSQ, OH, OD, dtype=dtype, device=DEV)
    k = torch.empty(OB, OSQ, OHKV, OD, dtype=dtype, device=DEV)
    v = torch.empty_like(k)
    for b in range(0, OB, OSLAB):
        n = min(OSLAB, OB - b)
        q[b:b + n], k[b:b + n], v[b:b + n] = qs[:n], ks[:n], vs[:n]
    args = dict(causal=True, k_prescaled=True, out_blocked=True)
    assert ops.fa3_route(q, k, v, **args) == "fwd5_kpre_oblk" and ops.fa3_route(qs, ks, vs, **args) == "fwd5_kpre_oblk"
    o = ops.fa3_fwd(q, k, v, **args)
    os_ = ops.fa3_fwd(qs, ks, vs, **args)
    torch.cuda.synchronize()
    assert o.shape == (OB * OSQ, OH * OD) and o.numel() * 2 > 1 << 32
    for b in range(0, OB, OSLAB):
        n = min(OSLAB, OB - b)
        assert torch.equal(o[b * OSQ:(b + n) * OSQ], os_[:n * OSQ]), f"blocked output of batches {b} .. differs from the slab's"
    for b in ((1 << 31) // (2 * OSQ * OH * OD) - 1, (1 << 31) // (2 * OSQ * OH * OD), OB - 2, OB - 1):
        ob = _unblock(o[b * OSQ:(b + 1) * OSQ], 1, OSQ, OH, OD)[0]
        assert torch.isfinite(ob).all(), f"batch {b}: non-finite output"
        j = b % OSLAB
        _judge(ob, None, qs[j], ks[j], vs[j], dtype, "fwd5_kpre_oblk", True, (-1, -1), 0, math.log(2.0), f"blocked output batch {b}")
    del q, k, v, o, os_, qs, ks, vs
    torch.cuda.empty_cache()


def test_stats_table():
    """Prints (-s) the worst measured statistics of this file's judgements per (dtype, family) beside the bars."""
    print()
    for (dtype, family), rec in sorted(ac.STATS.items(), key=str):
        bars = ac.BARS[(dtype, family)]
        print(f"{str(dtype).split('.')[-1]:9s}{family:12s} worst {rec['worst']:.3f}/{bars[0]} mean {rec['mean']:.3f}/{bars[1]} "
              f"group {rec['group']:.3f}/{bars[2]} lse {rec['lse']:.2e}/{bars[3]:.1e}  ({rec['n']} judgements)")

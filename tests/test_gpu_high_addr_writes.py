"""KV-cache writes, rotary embedding and the row kernels where the bytes a launch touches lie beyond 2^31, 2^32 and 2^33 bytes of
the tensors it is handed (csrc/cache_write.hip, csrc/rowops.hip).

Cache writes and rotary (placements from tests/_high_addr.py, checked by tests/test_high_addr_host.py): K and V caches of just
over 8 GiB each, 3 layers, written at layer 2 on pages just below and just above each boundary; the sources (key, value, q,
q_out) are strided views whose token stride of 64 MiB takes the packed tokens past 2^32 bytes, lying on filler of the same
allocation.  Every byte is 0xFF before the live rows are written, so a wrong source address reads 0xFF bytes (not the
expected row) and a wrong destination damages filler.  Writes are exact: the source bits for a 16-bit cache, test_gpu_kv8's
_quant_ref for an fp8 one, _rope_check's interval for rotated values; after each launch one scan of the whole allocation
counts the bytes that are not 0xFF, which must be exactly those of the expected live rows.

Row kernels: LayerNorm and RMSNorm over 2^21 + 300 rows of 1024 columns (x and y just over 4 GiB each), row-major and
blocked, with and without residual / sum: the rows around y's 2^31- and 2^32-byte offsets and the last ragged rows against the
fp64 references of _rows_check / _rms_check at their unchanged bounds, every row bit-equal to launches on copied slices of 64 Ki
rows, guard elements intact.  attn_merge at B * Sq * H * D just over 2^31 (o_a / o_b 8 GiB each, o_out 4 GiB): the rows
around 2^32 and 2^33 bytes of o_a and the tail against _rows_check's merge bound, everything bit-equal to merges of slices.

Measured on the MI355X (one run of this file, 50 tests in 43.5 s of pytest wall time; the tests print these with -s).  Cache
writes and apply_rotary: every byte exact, the scan's count equal to the expected one in every case; rotated q_out and K
(16-bit and fp8): 0 elements outside _rope_check's interval.  Row kernels: 0 elements outside the admissible interval in every
judged block, every slice bit-equal, guards intact; the largest share of ambiguous elements (intervals holding two 16-bit
values) over the judged blocks:
                          bf16      fp16
  layernorm, plain        0.0070    0.0438
  layernorm, residual     0.0078    0.0447
  rmsnorm, plain          0.0227    0.1813
  rmsnorm, residual       0.0228    0.1829
  attn_merge o_out        0.00053   0.00391   (cap _rows_check.CAP_MERGE = 0.01; o_a and lse inside within32 / lse_within)
"""
import functools

import pytest
import torch

import _high_addr as ha
import _rms_check as rc
import _rope_check as rp
import _rows_check as rw

pytestmark = pytest.mark.gpu

DEV = "cuda"
F8 = torch.float8_e4m3fn
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
LAYER = ha.LAYER
KS, VS = [0.7, 0.9, 0.011], [1.3, 0.4, 0.02]   # per layer; layer 2's make |x| / scale pass 448: the clamp is exercised


def _ops():
    from mio import ops
    return ops


def _quant(x, s):
    from test_gpu_kv8 import _quant_ref
    return _quant_ref(x.cpu(), s)


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _bytes(t):
    return t.contiguous().view(torch.uint8)


class _Arena:
    """The allocation of a write case with its views: caches [num_blocks, 3, bs, Hkv, D] (dtype or fp8) and the strided
    sources / q / q_out."""

    def __init__(self, case, dtype, fp8):
        i = case.info
        self.case, self.dtype, self.fp8, self.info = case, dtype, fp8, i
        self.bufs = ha.allocate(case)
        cdt = F8 if fp8 else dtype
        shape = (i["num_blocks"], ha.L, i["bs"], i["Hkv"], i["D"])
        self.kc, self.vc = (ha.view(self.bufs, case, n, cdt, shape) for n in ("k_cache", "v_cache"))
        self.bits = torch.uint8 if fp8 else torch.int16
        self.scales = dict(k_scale=torch.tensor(KS, dtype=torch.float32, device=DEV),
                           v_scale=torch.tensor(VS, dtype=torch.float32, device=DEV)) if fp8 else {}

    def src(self, name, rows, heads, every=1):
        """[rows, heads, D] view of the source columns `name`, every `every`-th token row of the case."""
        D = self.info["D"]
        return ha.view(self.bufs, self.case, name, self.dtype, (rows, heads, D), (every * ha.SRC_PITCH // 2, D, 1))

    def rows(self, cache, slots):
        """The cache rows [n, Hkv, D] at the (page, slot) of write_slots, read slice by slice."""
        return torch.stack([cache[p, LAYER, s] for _, p, s in slots])

    def refill(self, slots):
        for _, p, s in slots:
            self.kc[p, LAYER, s].view(self.bits).fill_(-1 if self.bits == torch.int16 else 0xFF)
            self.vc[p, LAYER, s].view(self.bits).fill_(-1 if self.bits == torch.int16 else 0xFF)

    def count(self):
        return ha.count_not_fill(self.bufs["kv"])

    def expected(self, x, scale):
        """The rows a write stores for the 16-bit source rows x: their bits, or _quant_ref's bytes."""
        return _quant(x, scale).to(DEV) if self.fp8 else x

    def close(self):
        self.kc = self.vc = self.bufs = None
        torch.cuda.empty_cache()


def _sources(dtype, T, Hkv, D, fp8, seed):
    g = torch.Generator().manual_seed(seed)
    k = (torch.randn(T, Hkv, D, generator=g) * (3.0 if fp8 else 1.0)).to(dtype).to(DEV)   # fp8: 3 sigma / 0.011 > 448
    v = (torch.randn(T, Hkv, D, generator=g) * (3.0 if fp8 else 1.0)).to(dtype).to(DEV)
    return k, v


def _exact(a, got, want, what):
    assert torch.equal(_bytes(got.view(a.bits)), _bytes(want.view(a.bits))), f"{what}: written rows differ from the expected bytes"


# ---- plain writes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp8", [False, True], ids=["kv16", "fp8"])
@pytest.mark.parametrize("bs,Hkv,D", ha.WRITE_GEOM)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_reshape_and_cache_varlen_high_pages(dtype, bs, Hkv, D, fp8):
    """76 new tokens of three sequences into pages around 2^31, 2^32 and 2^33 bytes of both caches; sequence 0's tokens cross
    from the page below 2^31 to the page above it; key / value are views whose token 64 starts past 2^32 bytes."""
    ops = _ops()
    case = ha.write_case(bs, Hkv, D, 1 if fp8 else 2)
    i = case.info
    T = i["T"]
    kx, vx = _sources(dtype, T, Hkv, D, fp8, bs + D)
    slots = ha.write_slots(i["new"], i["ctx"], bs, i["table"])
    cu = [0]
    for n in i["new"]:
        cu.append(cu[-1] + n)
    a = _Arena(case, dtype, fp8)
    try:
        key, value = a.src("key", T, Hkv), a.src("value", T, Hkv)
        key.copy_(kx), value.copy_(vx)
        assert key.stride(0) * 2 * (T - 1) > 1 << 32
        before = a.count()
        assert before == ha.live_bytes(kx, vx)
        ops.reshape_and_cache_varlen(key, value, a.kc, a.vc, _i32(i["table"]), _i32(cu), _i32(i["ctx"]), bs, LAYER, **a.scales)
        torch.cuda.synchronize()
        ek, ev = a.expected(kx, KS[LAYER]), a.expected(vx, VS[LAYER])
        what = f"varlen write bs{bs} Hkv{Hkv} D{D} {'fp8' if fp8 else 'kv16'}"
        _exact(a, a.rows(a.kc, slots), ek, what + " K")
        _exact(a, a.rows(a.vc, slots), ev, what + " V")
        assert a.count() == before + ha.live_bytes(ek.view(a.bits), ev.view(a.bits)), f"{what}: bytes outside the written rows changed"
    finally:
        key = value = None
        a.close()


@pytest.mark.parametrize("fp8", [False, True], ids=["kv16", "fp8"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_single_token_and_varlen_forms_agree_on_high_pages(dtype, fp8):
    """reshape_and_cache and reshape_and_cache_varlen with one new token per sequence: rows on the page below 2^31, the page
    above 2^32 and the page above 2^33, from source rows 0, 37 and 74 (the last past 2^32 bytes of the view); exact, and the
    two forms byte-identical."""
    ops = _ops()
    bs, Hkv, D = ha.WRITE_GEOM[0]
    case = ha.write_case(bs, Hkv, D, 1 if fp8 else 2)
    i = case.info
    ctx = [5, bs + 3, 3]
    slots = ha.write_slots([1, 1, 1], ctx, bs, i["table"])
    pb, lb = i["page_bytes"], i["layer_bytes"]
    starts = [p * pb + LAYER * lb for _, p, _ in slots]
    assert starts[0] + lb <= 1 << 31 and starts[1] >= 1 << 32 and starts[2] >= 1 << 33
    kx, vx = _sources(dtype, 3, Hkv, D, fp8, 5)
    a = _Arena(case, dtype, fp8)
    try:
        key, value = a.src("key", 3, Hkv, every=37), a.src("value", 3, Hkv, every=37)
        key.copy_(kx), value.copy_(vx)
        ek, ev = a.expected(kx, KS[LAYER]), a.expected(vx, VS[LAYER])
        want = ha.live_bytes(kx, vx, ek.view(a.bits), ev.view(a.bits))
        bt, cl = _i32(i["table"]), _i32(ctx)
        ops.reshape_and_cache(key[:, None], value[:, None], a.kc, a.vc, bt, cl, bs, LAYER, **a.scales)
        torch.cuda.synchronize()
        k1, v1 = a.rows(a.kc, slots), a.rows(a.vc, slots)
        assert a.count() == want, "single-token write: bytes outside the written rows changed"
        a.refill(slots)
        ops.reshape_and_cache_varlen(key, value, a.kc, a.vc, bt, _i32([0, 1, 2, 3]), cl, bs, LAYER, **a.scales)
        torch.cuda.synchronize()
        k2, v2 = a.rows(a.kc, slots), a.rows(a.vc, slots)
        assert a.count() == want, "varlen write of one token per sequence: bytes outside the written rows changed"
        _exact(a, k1, ek, "single-token K"), _exact(a, v1, ev, "single-token V")
        _exact(a, k2, k1, "varlen vs single-token K"), _exact(a, v2, v1, "varlen vs single-token V")
    finally:
        key = value = None
        a.close()


# ---- rotary ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp8", [False, True], ids=["kv16", "fp8"])
@pytest.mark.parametrize("interleaved", [False, True], ids=["neox", "gptj"])
@pytest.mark.parametrize("D,rot", [(128, 64), (64, 64)])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_rope_and_cache_varlen_high_pages(dtype, D, rot, interleaved, fp8):
    """The rotating write on the destinations of the plain one; q and q_out are views past 4 GiB, first apart, then q_out = q.
    Rotated values (q_out, K) inside _rope_check's interval; V, K past rot_dim and q past rot_dim are the plain write's bytes."""
    ops = _ops()
    bs, Hkv, heads = 64, 2, 4
    case = ha.write_case(bs, Hkv, D, 1 if fp8 else 2, heads=heads)
    i = case.info
    T = i["T"]
    kx, vx = _sources(dtype, T, Hkv, D, fp8, D + rot)
    qx = torch.randn(T, heads, D, generator=torch.Generator().manual_seed(rot)).to(dtype).to(DEV)
    slots = ha.write_slots(i["new"], i["ctx"], bs, i["table"])
    cu, pos = [0], []
    for n, c in zip(i["new"], i["ctx"]):
        cu.append(cu[-1] + n)
        pos += list(range(c - n, c))
    pos = torch.tensor(pos)
    cos, sin = ops.rope_tables(max(i["ctx"]) + 1, rot)
    qref, qdelta = rp.reference(qx.cpu(), cos, sin, pos, interleaved)
    kref, kdelta = rp.reference(kx.cpu(), cos, sin, pos, interleaved)
    ek, ev = None, None
    a = _Arena(case, dtype, fp8)
    try:
        key, value, q, q_out = a.src("key", T, Hkv), a.src("value", T, Hkv), a.src("q", T, heads), a.src("q_out", T, heads)
        key.copy_(kx), value.copy_(vx)
        ek, ev = a.expected(kx, KS[LAYER]), a.expected(vx, VS[LAYER])
        for alias in (False, True):
            what = f"rope write D{D} rot{rot} {'gptj' if interleaved else 'neox'} {'fp8' if fp8 else 'kv16'} alias={alias}"
            q.copy_(qx)
            q_out.view(torch.int16).fill_(-1)
            a.refill(slots)
            dst = q if alias else q_out
            got = ops.rope_and_cache_varlen(q, key, value, a.kc, a.vc, _i32(i["table"]), _i32(cu), _i32(i["ctx"]), bs, LAYER,
                                            cos.to(DEV), sin.to(DEV), interleaved=interleaved, q_out=dst, **a.scales)
            torch.cuda.synchronize()
            assert got.data_ptr() == dst.data_ptr()
            qo = dst.contiguous()
            out, _ = rp.outside16(qo.cpu()[..., :rot], qref, qdelta, dtype)
            assert out == 0, f"{what}: {out} rotated q elements outside the interval"
            assert torch.equal(_bytes(qo[..., rot:]), _bytes(qx[..., rot:])), f"{what}: q past rot_dim is not copied"
            krows, vrows = a.rows(a.kc, slots), a.rows(a.vc, slots)
            _exact(a, vrows, ev, what + " V")
            _exact(a, krows[..., rot:], ek[..., rot:], what + " K past rot_dim")
            if fp8:
                out = rp.outside8(krows.cpu()[..., :rot], kref, kdelta, KS[LAYER])
            else:
                out, _ = rp.outside16(krows.cpu()[..., :rot], kref, kdelta, dtype)
            assert out == 0, f"{what}: {out} rotated K elements outside the interval"
            live = [kx, vx, qo, krows.view(a.bits), vrows.view(a.bits)] + ([] if alias else [qx])
            assert a.count() == ha.live_bytes(*live), f"{what}: bytes outside the written rows changed"
    finally:
        key = value = q = q_out = dst = got = None
        a.close()


@pytest.mark.parametrize("interleaved", [False, True], ids=["neox", "gptj"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_apply_rotary_rows_past_4gib(dtype, D, interleaved):
    """apply_rotary on x and out whose row stride of 64 MiB takes the 80 tokens past 2^32 bytes (row 64), 4 GiB into one
    allocation: bit for bit the call on compact copies, apart and in place."""
    ops = _ops()
    case = ha.rotary_case(D)
    T, Hn, rot = ha.ROTARY_T, ha.ROTARY_HEADS, 64
    g = torch.Generator().manual_seed(D)
    xc = torch.randn(T, Hn, D, generator=g).to(dtype).to(DEV)
    pos = torch.randint(0, 500, (T,), generator=g).to(torch.int32).to(DEV)
    cos, sin = (t.to(DEV) for t in ops.rope_tables(500, rot))
    want = ops.apply_rotary(xc, cos, sin, pos, interleaved=interleaved)
    ref, delta = rp.reference(xc.cpu(), cos.cpu(), sin.cpu(), pos.cpu().long(), interleaved)
    assert rp.outside16(want.cpu()[..., :rot], ref, delta, dtype)[0] == 0
    bufs = ha.allocate(case)
    try:
        st = (ha.SRC_PITCH // 2, D, 1)
        x, out = ha.view(bufs, case, "x", dtype, (T, Hn, D), st), ha.view(bufs, case, "out", dtype, (T, Hn, D), st)
        assert x.stride(0) * 2 * (T - 1) > 1 << 32 and x.data_ptr() - bufs["wide"].data_ptr() >= 1 << 32
        x.copy_(xc)
        ops.apply_rotary(x, cos, sin, pos, interleaved=interleaved, out=out)
        assert torch.equal(out.contiguous(), want), "apply_rotary on the strided views differs from the compact call"
        assert ha.count_not_fill(bufs["wide"]) == ha.live_bytes(xc, want), "bytes outside x and out changed"
        out.view(torch.int16).fill_(-1)
        ops.apply_rotary(x, cos, sin, pos, interleaved=interleaved, out=x)
        assert torch.equal(x.contiguous(), want), "apply_rotary in place differs from the compact call"
        assert ha.count_not_fill(bufs["wide"]) == ha.live_bytes(want), "in place: bytes outside x changed"
    finally:
        x = out = bufs = None
        torch.cuda.empty_cache()


# ---- row kernels -----------------------------------------------------------------------------------------------------------
SLAB = 1 << 16                       # rows of the repeated slab and of the slices that are launched on their own
ROWS, COLS = ha.NORM_ROWS, ha.NORM_COLS
JUDGED = [((1 << 31) // (2 * COLS) - 16, 32), ((1 << 32) // (2 * COLS) - 16, 32), (ROWS - 300, 300)]   # (first row, rows)


@functools.lru_cache(maxsize=None)
def _slab(dtype, seed):
    return rw.layernorm_rows(dtype, SLAB, COLS, seed, offsets=False)[0]   # kept on the host (nothing writes to it)


def _big_rows(dtype, seed):
    """[ROWS, COLS]: one random slab of 64 Ki rows (_rows_check.layernorm_rows: row scales over five decades, planted rows)
    repeated, fresh random rows in the judged blocks and in three dozen other 16-row blocks."""
    slab = _slab(dtype, seed).to(DEV)
    x = torch.empty(ROWS, COLS, dtype=dtype, device=DEV)
    for r in range(0, ROWS, SLAB):
        n = min(SLAB, ROWS - r)
        x[r:r + n] = slab[:n]
    g = torch.Generator(device=DEV).manual_seed(seed)
    blocks = JUDGED + [(s * 57001 + 123, 16) for s in range(36)]
    for r, n in blocks:
        x[r:r + n] = (torch.randn(n, COLS, generator=g, device=DEV) * 10.0 ** (torch.rand(n, 1, generator=g, device=DEV) * 4 - 2)).to(dtype)
    return x


@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "residual_sum"])
@pytest.mark.parametrize("kind", ["layernorm", "rmsnorm"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_norm_rows_past_4gib(dtype, kind, with_res):
    """mio_layernorm_fwd / _bx and mio_rmsnorm_fwd over 2^21 + 300 rows of 1024 columns, row-major and blocked, without a residual
    and with one and sum_out (module docstring)."""
    from test_gpu_kernels import _unblock
    from test_gpu_rows import _launch, _unguarded
    rms = kind == "rmsnorm"
    eps = 1e-6 if rms else rw.EPS
    x = _big_rows(dtype, 1)
    w, b = rw.layernorm_params(dtype, COLS, 3, DEV)
    b = None if rms else b
    assert x.numel() * 2 > 1 << 32
    res = _big_rows(dtype, 2) if with_res else None
    for blocked in (False, True):
        what = f"{kind} residual={with_res} blocked={blocked}"
        y, s, ybuf, sbuf = _launch(dtype, x, res, w, b, 0.5, with_res, blocked=blocked, rms=rms, eps=eps)
        torch.cuda.synchronize()
        assert _unguarded(y, ybuf) == 0, f"{what}: guard elements around y were overwritten"
        if with_res:
            assert _unguarded(s, sbuf) == 0, f"{what}: guard elements around sum_out were overwritten"
        # every row: bit-equal to launches on copied slices of 64 Ki rows (256-row aligned)
        for r in range(0, ROWS, SLAB):
            n = min(SLAB, ROWS - r)
            xs = x[r:r + n].clone()
            rs = res[r:r + n].clone() if with_res else None
            y1, s1, _, _ = _launch(dtype, xs, rs, w, b, 0.5, with_res, blocked=blocked, rms=rms, eps=eps)
            if blocked:
                m = (n + 255) // 256 * 256
                got = _unblock(y[r:r + m], n, COLS)
                assert torch.equal(got, _unblock(y1, n, COLS)), f"{what}: rows {r} .. {r + n} differ from the slice's"
            else:
                assert torch.equal(y[r:r + n], y1), f"{what}: rows {r} .. {r + n} differ from the slice's"
            if with_res:
                assert torch.equal(s[r:r + n], s1), f"{what}: sum rows {r} .. {r + n} differ from the slice's"
            del xs, rs, y1, s1
        # the rows around y's 2^31- and 2^32-byte offsets and the ragged tail against fp64
        for r0, n in JUDGED:
            if blocked:
                lo = r0 // 256 * 256
                m = min((r0 + n + 255) // 256 * 256, y.shape[0]) - lo
                yr = _unblock(y[lo:lo + m], min(m, ROWS - lo), COLS)[r0 - lo:r0 - lo + n]
            else:
                yr = y[r0:r0 + n]
            src = x[r0:r0 + n]
            if with_res:
                sref, sbound = rc.sum_bound(src, res[r0:r0 + n], 0.5, dtype, device=DEV)
                serr = (s[r0:r0 + n].double() - sref).abs()
                assert bool((serr <= sbound).all()), f"{what}: sum rows {r0} ..: off by {(serr / sbound).max().item():.3g} x its bound"
                src = s[r0:r0 + n]
            ref = rc.reference_rows(src, w, eps, device=DEV) if rms else rw.reference_layernorm(src, w, b, eps, device=DEV)
            assert bool(torch.isfinite(yr).all()), f"{what}: non-finite output in rows {r0} .."
            amb = rw.admissible(yr, ref, dtype, f"{what} rows {r0} .. {r0 + n}")
            print(f"{what} {dtype} rows {r0}+{n}: outside 0, ambiguous {amb:.4f}")
        del y, s, ybuf, sbuf
        torch.cuda.empty_cache()
    del res
    del x
    torch.cuda.empty_cache()


MB, MSq, MH, MD = ha.MERGE_SHAPE
MSLAB = 512   # batches per slab / slice


def _merge_fill(o, lse, slab_o, slab_l):
    for b in range(0, MB, MSLAB):
        n = min(MSLAB, MB - b)
        o[b:b + n] = slab_o[:n]
        lse[b:b + n] = slab_l[:n]


@pytest.mark.parametrize("out_dtype", DTYPES, ids=IDS)
def test_attn_merge_past_2_31_elements(out_dtype):
    """attn_merge at B * Sq * H * D = 2^31 + 2^17 elements: o_a and o_b fp32 of 8 GiB each, the 16-bit o_out of 4 GiB (20 GiB
    alive with the slices).  Both sides repeat one slab of 512 batches (gaps, empties and scales of merge_states), so every
    slice of 512 batches has the same inputs: the whole result is bit-equal to one merge of the slab, slice by slice.  The
    batches around 2^32 and 2^33 bytes of o_a and the last one are judged by _rows_check's merge bound in fp64."""
    ops = _ops()
    n_el = MB * MSq * MH * MD
    assert n_el > 1 << 31
    oa_s, la_s, ob_s, lb_s = rw.merge_states(MSLAB, MSq, MH, MD, 9, DEV)   # one slab of 512 batches per side
    o_a = torch.empty(MB, MSq, MH, MD, dtype=torch.float32, device=DEV)
    o_b = torch.empty_like(o_a)
    l_a = torch.empty(MB, MH, MSq, dtype=torch.float32, device=DEV)
    l_b = torch.empty_like(l_a)
    _merge_fill(o_a, l_a, oa_s, la_s)
    _merge_fill(o_b, l_b, ob_s, lb_s)
    out = torch.full((n_el + 128,), -3.0e4, dtype=out_dtype, device=DEV)
    o_out = out[64:64 + n_el].view(MB, MSq, MH, MD)
    ops.attn_merge(o_a, l_a, o_b, l_b, out=o_out)
    torch.cuda.synchronize()
    assert bool((out[:64] == -3.0e4).all()) and bool((out[64 + n_el:] == -3.0e4).all()), "guard elements around o_out were overwritten"
    # the slab merged on its own
    so, sl = oa_s.clone(), la_s.clone()
    sout = torch.empty(MSLAB, MSq, MH, MD, dtype=out_dtype, device=DEV)
    ops.attn_merge(so, sl, ob_s, lb_s, out=sout)
    for b in range(0, MB, MSLAB):
        n = min(MSLAB, MB - b)
        assert torch.equal(o_a[b:b + n], so[:n]), f"o_a batches {b} .. differ from the slab's merge"
        assert torch.equal(l_a[b:b + n], sl[:n]), f"lse_a batches {b} .. differ from the slab's merge"
        assert torch.equal(o_out[b:b + n], sout[:n]), f"o_out batches {b} .. differ from the slab's merge"
        assert torch.equal(o_b[b:b + n], ob_s[:n]) and torch.equal(l_b[b:b + n], lb_s[:n]), "side b was written"
    per_b = MSq * MH * MD * 4
    for b0 in ((1 << 32) // per_b - 1, (1 << 33) // per_b - 1):   # (the second pair ends with the last batch)
        sl2 = torch.tensor([b0 % MSLAB, (b0 + 1) % MSLAB], device=DEV)
        ref, L, tol = rw.reference_merge(oa_s[sl2], la_s[sl2], ob_s[sl2], lb_s[sl2], device=DEV)
        what = f"merge batches {b0}, {b0 + 1}"
        rw.within32(o_a[b0:b0 + 2], ref, what)
        rw.lse_within(l_a[b0:b0 + 2], L, tol, what)
        amb = rw.admissible(o_out[b0:b0 + 2].reshape(-1, MD), ref, out_dtype, what)
        assert amb <= rw.CAP_MERGE, amb
        print(f"{what} {out_dtype}: outside 0, ambiguous {amb:.5f}")
    del o_a, o_b, l_a, l_b, out, o_out, so, sl, sout
    torch.cuda.empty_cache()

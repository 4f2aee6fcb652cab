"""The row kernels of csrc/rowops.hip on the GPU: LayerNorm (every CH instantiation and dispatch edge, every residual form, the
blocked output, the refusals) and the merge of two attention states, element by element against the fp64 references of
tests/_rows_check.py with its admissible-rounding judgement; the unrounded-sum path of RMSNorm, the same untested branch of the same
template."""
import ctypes
import functools

import pytest
import torch

import _rms_check as rc
import _rows_check as rw

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
FILL = -3.0e4  # guard fill: no output of these cases comes near it
EPS = rw.EPS
FORMS = {"none": None, "sum_alpha0.5": 0.5, "sum_alpha0.3": 0.3, "nosum": 0.3}  # form -> residual alpha


def _ops():
    from mio import ops
    return ops


def _lib():
    from mio import _lib
    return _lib


def _dt(dtype):
    return _lib().MIO_BF16 if dtype == torch.bfloat16 else _lib().MIO_FP16


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _guarded(n, dtype):
    """(a view of n elements 64 elements inside a filled buffer, 16-byte aligned; the buffer)."""
    buf = torch.full((n + 128,), FILL, dtype=dtype, device=DEV)
    return buf[64:64 + n], buf


def _unguarded(view, buf):
    """Elements of buf outside view that lost their fill."""
    return int((buf != FILL).sum()) - int((view != FILL).sum())


def _last_error():
    return _lib().lib.mio_last_error().decode("utf-8", "replace")


def _launch(dtype, x, res, w, b, alpha, want_sum, blocked=False, rms=False, eps=EPS, rows=None, expect=0):
    """mio_layernorm_fwd / _bx (rms: mio_rmsnorm_fwd) into guarded outputs.  Returns (y view, sum view or None, their buffers)."""
    lib = _lib().lib
    rows = x.shape[0] if rows is None else rows
    cols = x.shape[1]
    n = ((x.shape[0] + 255) // 256 * 256 if blocked else x.shape[0]) * cols
    y, ybuf = _guarded(n, dtype)
    y = y.view(-1, cols)
    s = sbuf = None
    if want_sum:
        s, sbuf = _guarded(x.shape[0] * cols, dtype)
        s = s.view(-1, cols)
    tail = (y.data_ptr(), _ptr(s), rows, cols, ctypes.c_float(eps), ctypes.c_float(alpha), _dt(dtype))
    if rms:
        rcode = lib.mio_rmsnorm_fwd(x.data_ptr(), _ptr(res), w.data_ptr(), *tail, int(blocked), _stream())
    else:
        entry = lib.mio_layernorm_fwd_bx if blocked else lib.mio_layernorm_fwd
        rcode = entry(x.data_ptr(), _ptr(res), w.data_ptr(), _ptr(b), *tail, _stream())
    assert (rcode == 0) == (expect == 0), _last_error()
    return y, s, ybuf, sbuf


@functools.lru_cache(maxsize=None)
def _case(dtype, rows, cols):
    return rw.ln_case(dtype, rows, cols, DEV)  # (shared by the forms; nothing writes to these)


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("cols", rw.LN_COLS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_layernorm_rows(dtype, cols, form):
    """One width and residual form over the row counts, with and without bias.  none: y against the reference on x.  sum: sum_out
    within _rms_check.sum_bound, y against the reference on the stored sum_out (the kernel normalises the rounded sum).  nosum:
    the C entry with sum_out = NULL (ops.layernorm(residual=..., return_sum=False)): y against the reference on the fp64 sum, with ds
    for its fp32 evaluation.  Every launch into guarded buffers, and bit-equal to ops.layernorm."""
    ops = _ops()
    alpha = FORMS[form]
    caps = rw.LnCaps(cols)
    for rows in rw.LN_ROWS:
        x, res, w, b, plain = _case(dtype, rows, cols)
        for bias in (b, None):
            what = f"layernorm rows {rows} cols {cols} {form} bias {bias is not None}"
            if form == "none":
                yg, _, ybuf, _ = _launch(dtype, x, None, w, bias, 1.0, False)
                y = ops.layernorm(x, w, bias, EPS)
                ref = rw.reference_layernorm(x, w, bias, EPS, device=DEV)
            elif form == "nosum":
                yg, _, ybuf, _ = _launch(dtype, x, res, w, bias, alpha, False)
                y = ops.layernorm(x, w, bias, EPS, residual=res, residual_alpha=alpha)
                s, ds = rw.unrounded_sum(x, res, alpha, device=DEV)
                ref = rw.reference_layernorm(s, w, bias, EPS, ds=ds, device=DEV)
            else:
                yg, sg, ybuf, sbuf = _launch(dtype, x, res, w, bias, alpha, True)
                y, s = ops.layernorm(x, w, bias, EPS, residual=res, residual_alpha=alpha, return_sum=True)
                assert torch.equal(sg, s) and _unguarded(sg, sbuf) == 0, what
                sref, sbound = rc.sum_bound(x, res, alpha, dtype, device=DEV)
                serr = (sg.double() - sref).abs()
                assert bool((serr <= sbound).all()), f"{what}: sum_out off by {(serr / sbound).max().item():.3g} x its bound"
                ref = rw.reference_layernorm(sg, w, bias, EPS, device=DEV)
            assert torch.equal(yg, y), f"{what}: ops.layernorm and the C entry differ"
            assert _unguarded(yg, ybuf) == 0, f"{what}: guard elements around y were overwritten"
            assert bool(torch.isfinite(yg).all()), f"{what}: non-finite output"
            rw.admissible(yg, ref, dtype, what)
            caps.add(ref, dtype, plain)
            if rows >= 32:
                want = torch.zeros(cols, dtype=dtype, device=DEV) if bias is None else bias
                assert torch.equal(yg[rw.ROW_ZERO], want), f"{what}: the zero row is not the bias bit for bit"
    plain_share, offset_share = caps.check(f"layernorm cols {cols} {form}")
    print(f"layernorm {dtype} cols {cols} {form}: outside 0, ambiguous {plain_share:.4f} (offset rows {offset_share:.4f})")


@pytest.mark.parametrize("cols", [520, 4096, 8192])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_rmsnorm_unrounded_sum(dtype, cols):
    """mio_rmsnorm_fwd with a residual and sum_out = NULL: the RMS instantiation of the branch test_layernorm_rows[nosum] runs."""
    ops = _ops()
    x, _ = rw.layernorm_rows(dtype, 257, cols, cols + 1, DEV)
    res, _ = rw.layernorm_rows(dtype, 257, cols, cols + 2, DEV, offsets=False)
    w, _ = rw.layernorm_params(dtype, cols, cols + 3, DEV)
    yg, _, ybuf, _ = _launch(dtype, x, res, w, None, 0.3, False, rms=True, eps=1e-6)
    assert torch.equal(yg, ops.rmsnorm(x, w, 1e-6, residual=res, residual_alpha=0.3)) and _unguarded(yg, ybuf) == 0
    s, ds = rw.unrounded_sum(x, res, 0.3, device=DEV)
    ref = rw.reference_rms(s, w, 1e-6, ds=ds, device=DEV)
    # (no cap here: _rms_check charges the sum gamma_cols, for any order, so at these widths many fp16 intervals hold two values;
    # the host self-test shows that the sum rounded by mistake still leaves them at each of these widths)
    amb = rw.admissible(yg, ref, dtype, f"rmsnorm cols {cols}, unrounded sum")
    print(f"rmsnorm {dtype} cols {cols} nosum: outside 0, ambiguous {amb:.4f}")
    assert bool((yg[rw.ROW_ZERO] == 0).all())


@pytest.mark.parametrize("cols", [32, 1024])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_layernorm_out_blocked(dtype, cols):
    """mio_layernorm_fwd_bx: bit for bit the row-major result after un-blocking, rows 258 .. 511 of the last 256-row block keep the
    fill; without a residual, with one and sum_out, and with one and no sum_out."""
    from test_gpu_kernels import _unblock
    rows = 257
    x, res, w, b, _ = _case(dtype, rows, cols)
    for r, want_sum in ((None, False), (res, True), (res, False)):
        y, s, ybuf, sbuf = _launch(dtype, x, r, w, b, 0.5, want_sum)
        yb, sb, ybbuf, sbbuf = _launch(dtype, x, r, w, b, 0.5, want_sum, blocked=True)
        assert torch.equal(_unblock(yb, rows, cols), y) and _unguarded(yb, ybbuf) == 0
        if want_sum:
            assert torch.equal(sb, s) and _unguarded(sb, sbbuf) == 0
        pad = yb.view(2, cols // 32, 256, 32)[1, :, 1:]
        assert bool((pad == FILL).all()), "rows past 257 of the blocked output were written"


def test_layernorm_refusals_launch_nothing():
    """Host-side refusals with valid pointers: cols 4104 (past the CH = 8 instantiation), cols 20, blocked output at cols 40."""
    dtype = torch.bfloat16
    for cols, blocked, words in ((4104, False, "cols > 4096"), (20, False, "multiple of 8"), (40, True, "multiple of 32")):
        x = torch.ones(4, cols, dtype=dtype, device=DEV)
        w = torch.ones(cols, dtype=dtype, device=DEV)
        y, _, ybuf, _ = _launch(dtype, x, None, w, None, 1.0, False, blocked=blocked, expect=1)
        assert words in _last_error(), _last_error()
        torch.cuda.synchronize()
        assert bool((ybuf == FILL).all()), f"cols {cols}: a refused call wrote to y"
    with pytest.raises(RuntimeError, match="cols > 4096"):
        _ops().layernorm(torch.ones(4, 4104, dtype=dtype, device=DEV), torch.ones(4104, dtype=dtype, device=DEV))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_layernorm_no_rows(dtype):
    """rows == 0 with valid non-null pointers: returns 0 and writes nothing."""
    x, res, w, b, _ = _case(dtype, 4, 64)
    for blocked in (False, True):
        y, s, ybuf, sbuf = _launch(dtype, x, res, w, b, 0.5, True, blocked=blocked, rows=0)
        torch.cuda.synchronize()
        assert bool((ybuf == FILL).all()) and bool((sbuf == FILL).all())


# ---- attn_merge --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", rw.MERGE_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("out_dtype", DTYPES + [None], ids=IDS + ["no_out"])
def test_attn_merge_rows(out_dtype, shape):
    """Two live states at every gap, per-row empties, D % 8 != 0, a thread count that is no multiple of 256 (the first shape: 1110;
    its B, H, Sq are all > 1 and the gaps independent per (b, h, s), so a wrong lse index fails): o_a and lse_a against the fp64
    merge, o_out admissible and the rounding of o_a, side b untouched, guards untouched; then the sides swapped: the same o and lse
    within the same bounds."""
    ops = _ops()
    B, Sq, H, D = shape
    st = rw.merge_states(*shape, seed=sum(shape), device=DEV)
    ref, L, tol_lse = rw.reference_merge(*st, device=DEV)
    for swap in (False, True):
        what = f"merge {shape} swapped {swap}"
        o_a, l_a, o_b, l_b = (t.clone() for t in ((st[2], st[3], st[0], st[1]) if swap else st))
        keep_o, keep_l = o_b.clone(), l_b.clone()
        out = buf = None
        if out_dtype is not None:
            out, buf = _guarded(B * Sq * H * D, out_dtype)
            out = out.view(B, Sq, H, D)
        ops.attn_merge(o_a, l_a, o_b, l_b, out=out)
        rw.within32(o_a, ref, what)
        rw.lse_within(l_a, L, tol_lse, what)
        assert torch.equal(o_b, keep_o) and torch.equal(l_b, keep_l), f"{what}: side b was written"
        if out is not None:
            amb = rw.admissible(out.view(-1, D), ref, out_dtype, what)
            assert amb <= rw.CAP_MERGE, amb
            assert torch.equal(out, o_a.to(out_dtype)), f"{what}: o_out is not the rounding of o_a"
            assert _unguarded(out, buf) == 0, f"{what}: guard elements around o_out were overwritten"
            print(f"merge {out_dtype} {shape} swapped {swap}: outside 0, ambiguous {amb:.5f}")


def test_attn_merge_no_queries():
    """Sq == 0 at the C level, with non-null pointers: returns 0 and writes nothing."""
    t = [torch.full((64,), 3.0, dtype=torch.float32, device=DEV) for _ in range(4)]
    out = torch.full((64,), FILL, dtype=torch.bfloat16, device=DEV)
    rcode = _lib().lib.mio_attn_merge(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), out.data_ptr(), 2, 0, 3, 8,
                                      _dt(torch.bfloat16), _stream())
    torch.cuda.synchronize()
    assert rcode == 0, _last_error()
    assert all(bool((x == 3.0).all()) for x in t) and bool((out == FILL).all())

"""The row kernels of csrc/rowops.hip on the GPU: LayerNorm (every CH instantiation and dispatch edge, every residual form, the
blocked output, the refusals) and the merge of two attention states, element by element against the fp64 references of
tests/_rows_check.py with its admissible-rounding judgement; the unrounded-sum path of RMSNorm, the same untested branch of the same
template."""
import ctypes
import functools

import pytest
import torch

import _hostile_gemm as hg
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


# ---- hostile memory around every operand (tests/_hostile_gemm.py) ------------------------------------------------------------------
def hostile_rows(dtype, rows, cols, x, res, w, b, alpha, want_sum, blocked, rms=False, eps=EPS):
    """One row-kernel launch form in hostile memory: x and the residual between guard rows, weight and bias 8 elements into
    their buffers, y (blocked: only its rows below `rows` are the launch's) and sum_out 64 elements into theirs.  The C ABI gives
    these kernels no row stride, so there are no columns past `cols` to poison.  Three launches at the same addresses (benign,
    NaN, huge): every output bit-equal to the benign launch's, every byte the launch does not own untouched.  Returns the benign
    (y, sum_out)."""
    lib = _lib().lib
    mp = (rows + 255) // 256 * 256
    ny = (mp if blocked else rows) * cols
    e = {"x": hg.Embedded(x, (rows + 2, cols), (1, 0)), "w": hg.Embedded(w, (cols + 16,), (8,), seed=1),
         "y": hg.Embedded(None, (ny + 128,), (64,), out_shape=(ny,), dtype=dtype, device=DEV,
                          own_index=hg.blocked_index(rows, cols) if blocked else None)}
    if res is not None:
        e["res"] = hg.Embedded(res, (rows + 2, cols), (1, 0), seed=2)
    if b is not None:
        e["b"] = hg.Embedded(b, (cols + 16,), (8,), seed=3)
    if want_sum:
        e["sum"] = hg.Embedded(None, (rows * cols + 128,), (64,), out_shape=(rows * cols,), dtype=dtype, device=DEV)
    p = lambda n: e[n].view.data_ptr() if n in e else None  # noqa: E731
    what = f"rows {rows} cols {cols} residual {res is not None} sum_out {want_sum} blocked {blocked} rms {rms}"
    got = {}
    for fill in hg.FILLS:
        for t in e.values():
            t.fill(fill)
        tail = (p("y"), p("sum"), rows, cols, ctypes.c_float(eps), ctypes.c_float(alpha), _dt(dtype))
        if rms:
            rcode = lib.mio_rmsnorm_fwd(p("x"), p("res"), p("w"), *tail, int(blocked), _stream())
        else:
            rcode = (lib.mio_layernorm_fwd_bx if blocked else lib.mio_layernorm_fwd)(p("x"), p("res"), p("w"), p("b"), *tail, _stream())
        assert rcode == 0, _last_error()
        torch.cuda.synchronize()
        for n, t in e.items():
            assert t.untouched(), f"{what} fill {fill}: bytes of {n} that the launch does not own were overwritten"
        y = e["y"].view[hg.blocked_index(rows, cols).to(DEV)] if blocked else e["y"].view.view(rows, cols)
        got[fill] = (y.clone(), e["sum"].view.view(rows, cols).clone() if want_sum else None)
    for fill in ("nan", "huge"):
        for i, name in enumerate(("y", "sum_out")):
            if got[fill][i] is not None:
                d = got[fill][i].view(torch.int16) != got["benign"][i].view(torch.int16)
                assert not bool(d.any()), (f"{what} fill {fill}: {int(d.sum())} elements of {name} differ from the benign launch, "
                                           f"first at (row, column) {tuple(d.nonzero()[0].tolist())}")
    return got["benign"]


@pytest.mark.parametrize("blocked", [False, True], ids=["rows", "blocked"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_layernorm_hostile_memory(dtype, blocked):
    """mio_layernorm_fwd and mio_layernorm_fwd_bx through hostile_rows: one chunk per lane and the widest instantiation, a ragged
    width, a partly filled last workgroup and a second 256-row block, without a residual, with one and sum_out, with one and
    none.  The benign launch is ops.layernorm's result bit for bit (which test_layernorm_rows judges against fp64)."""
    ops = _ops()
    for rows, cols in ((5, 64), (257, 1024), (3, 4096)) if blocked else ((5, 8), (257, 520), (3, 4096)):
        x, res, w, b, _ = _case(dtype, rows, cols)
        for r, want_sum, bias in ((None, False, b), (res, True, b), (res, False, None)):
            y, s = hostile_rows(dtype, rows, cols, x, r, w, bias, 0.5, want_sum, blocked)
            want = ops.layernorm(x, w, bias, EPS, residual=r, residual_alpha=0.5, return_sum=want_sum)
            ws = None
            if want_sum:
                want, ws = want
            assert torch.equal(y, want) and (ws is None or torch.equal(s, ws)), (rows, cols, want_sum)


@pytest.mark.parametrize("shape", rw.MERGE_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("out_dtype", DTYPES + [None], ids=IDS + ["no_out"])
def test_attn_merge_hostile_memory(out_dtype, shape):
    """mio_attn_merge with o_a, lse_a, o_b, lse_b and o_out 8 (o_out: 64) elements into buffers whose other bytes hold, in three
    launches at the same addresses, finite randn, NaN and 1e30: the merged (o_a, lse_a) and o_out bit-equal to the benign
    launch's -- which is ops.attn_merge's result on plain tensors bit for bit --, side b and every byte around the five
    operands untouched."""
    ops, lib = _ops(), _lib().lib
    B, Sq, H, D = shape
    st = rw.merge_states(*shape, seed=sum(shape), device=DEV)
    e = {n: hg.Embedded(t.reshape(-1), (t.numel() + 16,), (8,), seed=i, written=n in ("o_a", "lse_a"))
         for i, (n, t) in enumerate(zip(("o_a", "lse_a", "o_b", "lse_b"), st))}
    if out_dtype is not None:
        n = B * Sq * H * D
        e["out"] = hg.Embedded(None, (n + 128,), (64,), out_shape=(n,), dtype=out_dtype, device=DEV)
    p = lambda n: e[n].view.data_ptr() if n in e else None  # noqa: E731
    got = {}
    for fill in hg.FILLS:
        for t in e.values():
            t.fill(fill)
        rcode = lib.mio_attn_merge(p("o_a"), p("lse_a"), p("o_b"), p("lse_b"), p("out"), B, Sq, H, D,
                                   _dt(out_dtype or torch.bfloat16), _stream())
        assert rcode == 0, _last_error()
        torch.cuda.synchronize()
        for n, t in e.items():
            assert t.untouched(), f"merge {shape} fill {fill}: bytes of {n} that the launch does not own were overwritten"
        got[fill] = [hg.bits(e[n].view).clone() for n in ("o_a", "lse_a") + (("out",) if out_dtype is not None else ())]
    for fill in ("nan", "huge"):
        for a, b_, n in zip(got[fill], got["benign"], ("o_a", "lse_a", "o_out")):
            assert torch.equal(a, b_), f"merge {shape} fill {fill}: {int((a != b_).sum())} elements of {n} differ from the benign launch"
    o_a, l_a, o_b, l_b = (t.clone() for t in st)
    out = None if out_dtype is None else torch.empty(B, Sq, H, D, dtype=out_dtype, device=DEV)
    ops.attn_merge(o_a, l_a, o_b, l_b, out=out)
    want = [o_a, l_a] + ([out] if out is not None else [])
    for a, t in zip(got["benign"], want):
        assert torch.equal(a, hg.bits(t.reshape(-1))), f"merge {shape}: the benign launch is not ops.attn_merge's result"


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

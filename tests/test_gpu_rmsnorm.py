"""RMSNorm on the GPU: the row kernel (ops.rmsnorm) and the RMS form of the folded consumer GEMM (ops.gemm_ln(norm="rms")) against
the fp64 references of tests/_rms_check.py, element by element; the LayerNorm fold's bits unchanged; the modules."""
import ctypes

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import _gemm_check as gc
import _rms_check as rc

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
FILL = -3.0e4  # guard fill: no output of these cases comes near it
EPS = 1e-6
# one chunk, a full single-chunk wave, a ragged second chunk, LayerNorm's limit, just past it, RMSNorm's limit
COLS = [8, 512, 520, 1024, 4096, 4104, 8192]
ROWS = [1, 3, 5, 257]


def _ops():
    from mio import ops
    return ops


def _rand(shape, dtype, scale=1.0, seed=0, shift=0.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(shape, device=DEV, generator=g) * scale + shift).to(dtype)


def _rows_input(dtype, rows, cols, seed):
    """[rows, cols]: row scales log-uniform over 1e-2 .. 1e2; from 32 rows on, row 5 is zero, row 17 constant and row 29 has a
    single non-zero element.  Returns (x, the index of the zero row or None)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    scale = 10.0 ** (torch.rand(rows, 1, device=DEV, generator=g) * 4 - 2)
    x = torch.randn(rows, cols, device=DEV, generator=g) * scale
    zero = None
    if rows >= 32:
        zero = 5
        x[5] = 0
        x[17] = scale[17]
        x[29] = 0
        x[29, (29 * 37) % cols] = scale[29, 0]
    return x.to(dtype), zero


def _guarded_launch(dtype, x, res, w, alpha, blocked):
    """mio_rmsnorm_fwd into an output that is a view inside a filled buffer (64 elements either side, 16-byte aligned).  Returns
    (y view, sum view or None, their buffers)."""
    from mio import _lib
    rows, cols = x.shape
    n = ((rows + 255) // 256 * 256 if blocked else rows) * cols
    ybuf = torch.full((n + 128,), FILL, dtype=dtype, device=DEV)
    y = ybuf[64:64 + n].view(-1, cols)
    sbuf = s = None
    if res is not None:
        sbuf = torch.full((rows * cols + 128,), FILL, dtype=dtype, device=DEV)
        s = sbuf[64:64 + rows * cols].view(rows, cols)
    rcode = _lib.lib.mio_rmsnorm_fwd(x.data_ptr(), None if res is None else res.data_ptr(), w.data_ptr(), y.data_ptr(),
                                     None if s is None else s.data_ptr(), rows, cols, ctypes.c_float(EPS), ctypes.c_float(alpha),
                                     _lib.MIO_BF16 if dtype == torch.bfloat16 else _lib.MIO_FP16, int(blocked),
                                     torch.cuda.current_stream().cuda_stream)
    assert rcode == 0, _lib.lib.mio_last_error()
    return y, s, ybuf, sbuf


def _unguarded(view, buf):
    """Elements of buf outside view that lost their fill."""
    return int((buf != FILL).sum()) - int((view != FILL).sum())


def _row_case(dtype, rows, cols, with_res, seed=0):
    """One shape through ops.rmsnorm and through the guarded launch (bit-equal): sum_out within sum_bound, y within the element
    bound of reference_rows on what the kernel normalised.  Returns (y, ref) of the launch."""
    ops = _ops()
    x, zero = _rows_input(dtype, rows, cols, seed)
    w = _rand((cols,), dtype, 0.2, seed + 1, shift=1.0)
    what = f"rmsnorm rows {rows} cols {cols} residual {with_res}"
    if with_res:
        res, _ = _rows_input(dtype, rows, cols, seed + 2)
        y, s = ops.rmsnorm(x, w, EPS, residual=res, residual_alpha=0.5, return_sum=True)
        yg, sg, ybuf, sbuf = _guarded_launch(dtype, x, res, w, 0.5, False)
        assert torch.equal(sg, s) and _unguarded(sg, sbuf) == 0, what
        sref, sbound = rc.sum_bound(x, res, 0.5, dtype, device=DEV)
        serr = (s.double() - sref).abs()
        assert bool((serr <= sbound).all()), f"{what}: sum_out off by {(serr / sbound).max().item():.3g} x its bound"
    else:
        y, s = ops.rmsnorm(x, w, EPS, return_sum=True)
        assert s is x  # (no residual: the sum is the input itself)
        yg, _, ybuf, _ = _guarded_launch(dtype, x, None, w, 1.0, False)
    assert torch.equal(yg, y), what
    ref = rc.reference_rows(s, w, EPS, device=DEV)
    gc.check(yg, ref, dtype, "rmsnorm", guard=ybuf, fill=FILL, bars=False, what=what)
    if zero is not None:
        assert bool((y[zero] == 0).all()), f"{what}: the zero row is not exactly zero"
    return y, ref


@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "residual_sum"])
@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_rmsnorm_rows(dtype, cols, with_res):
    for rows in ROWS:
        _row_case(dtype, rows, cols, with_res, seed=cols + rows)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_rmsnorm_not_round_to_nearest_share(dtype):
    """The statistical bar: over all widths, plain and with residual, at 257 rows."""
    bad = total = 0
    for cols in COLS:
        for with_res in (False, True):
            y, ref = _row_case(dtype, 257, cols, with_res, seed=7 * cols)
            bad += rc.not_rn(y, ref, dtype) * y.numel()
            total += y.numel()
    share = bad / total
    print(f"rmsnorm not round-to-nearest share {dtype}: {share:.3e}")
    assert share <= rc.ROW_NOT_RN[dtype], (share, rc.ROW_NOT_RN[dtype])


@pytest.mark.parametrize("cols", [32, 1024])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_rmsnorm_out_blocked(dtype, cols):
    """The blocked output is bit for bit the row-major one, and the rows past 257 of the last 256-row block are not written.
    (With a residual the sum is stored in every launch compared, so each normalises the rounded sum.)"""
    from test_gpu_kernels import _unblock
    ops = _ops()
    rows = 257
    x, _ = _rows_input(dtype, rows, cols, cols)
    res, _ = _rows_input(dtype, rows, cols, cols + 1)
    w = _rand((cols,), dtype, 0.2, cols + 2, shift=1.0)
    for r in (None, res):
        y, s = ops.rmsnorm(x, w, EPS, residual=r, residual_alpha=0.5, return_sum=True)
        yb, sb = ops.rmsnorm(x, w, EPS, residual=r, residual_alpha=0.5, return_sum=True, out_blocked=True)
        assert tuple(yb.shape) == (512, cols) and torch.equal(_unblock(yb, rows, cols), y) and torch.equal(sb, s)
        yg, _, ybuf, _ = _guarded_launch(dtype, x, r, w, 0.5, True)
        assert torch.equal(_unblock(yg, rows, cols), y) and _unguarded(yg, ybuf) == 0
        pad = yg.view(2, cols // 32, 256, 32)[1, :, 1:]
        assert bool((pad == FILL).all()), "rows past M of the blocked output were written"


@pytest.mark.parametrize("blocked", [False, True], ids=["rows", "blocked"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_rmsnorm_hostile_memory(dtype, blocked):
    """mio_rmsnorm_fwd through test_gpu_rows.hostile_rows: x and the residual between guard rows, the weight inside guards, y
    (blocked: only its rows below `rows`) and sum_out inside guards; three launches at the same addresses with finite randn,
    NaN and huge values in every byte the launch does not own: outputs bit-equal, those bytes untouched.  One chunk, a ragged
    second chunk and RMSNorm's widest rows; a partly filled last workgroup and a second 256-row block.  The benign launch is
    ops.rmsnorm's result bit for bit (which test_rmsnorm_rows judges against fp64)."""
    from test_gpu_rows import hostile_rows
    ops = _ops()
    for rows, cols in ((5, 32), (257, 1024), (3, 8192)) if blocked else ((5, 8), (257, 520), (3, 8192)):
        x, _ = _rows_input(dtype, rows, cols, cols + rows)
        res, _ = _rows_input(dtype, rows, cols, cols + rows + 1)
        w = _rand((cols,), dtype, 0.2, cols + 2, shift=1.0)
        for r, want_sum in ((None, False), (res, True), (res, False)):
            y, s = hostile_rows(dtype, rows, cols, x, r, w, None, 0.5, want_sum, blocked, rms=True, eps=EPS)
            want = ops.rmsnorm(x, w, EPS, residual=r, residual_alpha=0.5, return_sum=want_sum)
            ws = None
            if want_sum:
                want, ws = want
            assert torch.equal(y, want) and (ws is None or r is None or torch.equal(s, ws)), (rows, cols, want_sum)


def test_rmsnorm_refuses_wide_rows():
    ops = _ops()
    with pytest.raises(ValueError, match="8192"):
        ops.rmsnorm(torch.zeros(2, 8200, device=DEV, dtype=torch.bfloat16), torch.ones(8200, device=DEV, dtype=torch.bfloat16))


# ---- the fold --------------------------------------------------------------------------------------------------------------
MR = 8192 - 7  # 32 row tiles, the last one ragged (test_gpu_gemm_matrix.MR: the smallest fold shapes)


def _rms_consumer(dtype, route, y, st, N, act, seed, col_scale=None, blocked=False, bars=True, what=""):
    """test_gpu_gemm_matrix._fold_consumer's RMS twin: one consumer launch on the stream y with the statistics st, the route
    asserted, judged against rc.reference_fold_rms of what the kernel reads with the LayerNorm fold's bars.  Returns
    (z, bias, (blocked weight, launch keywords))."""
    from test_gpu_gemm_matrix import _seam_rows
    ops = _ops()
    M, K = y.shape
    gam = _rand((K,), dtype, 0.2, seed + 4, shift=1.0)
    wc, bc = _rand((N, K), dtype, K ** -0.5, seed + 6), _rand((N,), dtype, 0.1, seed + 7)
    ws, b = ops.rms_fold_weight(wc, gam, bc, blocked=False)
    assert b is bc and torch.equal(ws, (wc.double() * gam.double()).to(dtype)), "rms_fold_weight is not one rounding of w * gamma"
    kw = dict(M=M, N=N, K=K, activation=act, ln_stats=st, eps=EPS, norm="rms")
    rkw = {}
    if act == "swiglu":
        wg, bg = _rand((N, K), dtype, K ** -0.5, seed + 8), _rand((N,), dtype, 0.1, seed + 9)
        wgs, _ = ops.rms_fold_weight(wg, gam, bg, blocked=False)
        wb = ops.block_weight_glu(wgs, ws)
        kw["bias_gate"] = bg
        rkw = dict(ws_gate=wgs, bias_gate=bg)
    else:
        wb, b2 = ops.rms_fold_weight(wc, gam, bc)
        assert torch.equal(wb, ops.block_weight(ws)) and b2 is bc, "the blocked fold is not block_weight(ws)"
    if col_scale is not None:
        kw["col_scale"] = col_scale
    assert ops.gemm_route(y, wb, bc, **kw) == route, what
    z, none = ops.gemm_ln(y, wb, bc, **kw)
    assert none is None and tuple(z.shape) == (M, N)
    if blocked:  # the same launch through the blocked activation layout on both sides: bit for bit
        from test_gpu_kernels import _block, _unblock
        zb, _ = ops.gemm_ln(_block(y), wb, bc, x_blocked=True, out_blocked=True, **kw)
        assert torch.equal(_unblock(zb, M, N), z), "blocked x / blocked output differs from the row-major launch"
    stl = ops.ln_stats_for_launch(st, M)
    rows = _seam_rows(M) if K >= 4096 else None
    pick = (lambda t: t) if rows is None else (lambda t: t[rows])  # noqa: E731
    ref = rc.reference_fold_rms(pick(y), stl[:, :M] if rows is None else stl[:, rows], ws, bc, eps=EPS, act=act,
                                col_scale=col_scale, device=DEV, **rkw)
    gc.check(pick(z), ref, dtype, route, bars=gc.BARS[(dtype, route)] if bars else False,
             what=what or f"rms fold M {M} N {N} K {K} {act}")
    return z, bc, (wb, kw)


def _rms_case(dtype, route, N, K, act, seed=0, **kw):
    from test_gpu_gemm_matrix import _fold_stream
    y, st = _fold_stream(dtype, MR, K, seed)
    return y, st, _rms_consumer(dtype, route, y, st, N, act, seed, **kw)


@pytest.mark.parametrize("K", [256, 1024, 2304, 8192])  # 1, 4, 9 -> 3 and 32 -> 8 statistic slots
@pytest.mark.parametrize("act", ["none", "gelu", "swiglu"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_rms_fold(dtype, act, K):
    if act == "swiglu":
        _rms_case(dtype, "p8w_glu_fold", 1024, K, act, seed=K)
    else:
        _rms_case(dtype, "p8w_fold", 2048, K, act, seed=K + 1)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_rms_fold_col_scale(dtype):
    _rms_case(dtype, "p8w_fold", 2048, 1024, "gelu", seed=4, col_scale=(1024, 2048, 0.25))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_rms_fold_blocked_in_and_out(dtype):
    _rms_case(dtype, "p8w_fold", 2048, 1024, "none", seed=5, blocked=True)


@pytest.mark.parametrize("route,N,act", [("p8w_fold", 2048, "none"), ("p8w_glu_fold", 1024, "swiglu")])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_rms_fold_sum_slot_is_dead(dtype, route, N, act):
    """The same launch with every sum entry of the statistics replaced by NaN gives the same bits."""
    ops = _ops()
    y, st, (z, b, (wb, kw)) = _rms_case(dtype, route, N, 1024, act, seed=12)
    st2 = st.clone()
    st2[..., 0] = float("nan")
    kw["ln_stats"] = st2
    z2, _ = ops.gemm_ln(y, wb, b, **kw)
    assert torch.equal(z2, z), "the statistics' sum entries reach the output of the RMS form"


@pytest.mark.parametrize("route,N,act", [("p8w_fold", 2048, "none"), ("p8w_glu_fold", 1024, "swiglu")])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_rms_fold_adversarial_stream(dtype, route, N, act):
    """test_gpu_gemm_matrix._fold_adversarial for the RMS form: the adversarial stream with statistics built by the test and NaN
    in the statistics rows past M: inside the element bound everywhere, a zero row gives exactly the bias (act none), and the
    output is bit for bit that of the same launch with the padding rows zeroed."""
    from test_gpu_gemm_matrix import _adversarial_stream, _built_stats
    ops = _ops()
    M, K = 8192 - 100, 1024
    y, zero = _adversarial_stream(dtype, M, K, 7)
    z, b, (wb, kw) = _rms_consumer(dtype, route, y, _built_stats(y, float("nan")), N, act, 7, bars=False,
                                   what=f"adversarial stream {act}")
    if act == "none":
        assert torch.equal(z[zero], b.expand(int(zero.sum()), N)), "a zero row is not the bias"
    kw["ln_stats"] = _built_stats(y, 0.0)
    z0, _ = ops.gemm_ln(y, wb, b, **kw)
    assert torch.equal(z0, z), "the statistics rows past M reach the output"


def test_rms_fold_needs_stats_and_a_known_norm():
    ops = _ops()
    x = torch.zeros(MR, 1024, device=DEV, dtype=torch.bfloat16)
    wb = torch.zeros(2048, 1024, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="ln_stats"):
        ops.gemm_ln(x, wb, None, M=MR, N=2048, K=1024, norm="rms")
    with pytest.raises(ValueError, match="norm"):
        ops.gemm_ln(x, wb, None, M=MR, N=2048, K=1024, norm="x")


def test_layernorm_fold_bits_unchanged_by_norm_argument():
    """One p8w_fold LayerNorm launch: with and without the explicit norm="layernorm", bit for bit, and inside the LayerNorm
    fold's own reference and bars."""
    from test_gpu_gemm_matrix import _fold_stream
    ops = _ops()
    dtype, N, K = torch.bfloat16, 2048, 1024
    y, st = _fold_stream(dtype, MR, K, 3)
    gam, bet = _rand((K,), dtype, 0.2, 4, shift=1.0), _rand((K,), dtype, 0.1, 5)
    wc, bc = _rand((N, K), dtype, K ** -0.5, 6), _rand((N,), dtype, 0.1, 7)
    ws, bfold = ops.ln_fold_weight(wc, gam, bet, bc, blocked=False)
    wb = ops.block_weight(ws)
    kw = dict(M=MR, N=N, K=K, ln_stats=st, eps=1e-5)
    assert ops.gemm_route(y, wb, bfold, **kw) == ops.gemm_route(y, wb, bfold, norm="layernorm", **kw) == "p8w_fold"
    z, _ = ops.gemm_ln(y, wb, bfold, **kw)
    z2, _ = ops.gemm_ln(y, wb, bfold, norm="layernorm", **kw)
    assert torch.equal(z, z2)
    ref = gc.reference_fold(y, st, ws, bfold, eps=1e-5, device=DEV)
    gc.check(z, ref, dtype, "p8w_fold", bars=gc.BARS[(dtype, "p8w_fold")], what="LayerNorm fold beside the RMS form")


# ---- modules -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [1e-6, None])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_fused_rmsnorm_module(dtype, eps):
    """FusedRMSNorm (fp32 parameters, 16-bit activations) against torch.nn.functional.rms_norm in fp32: within the row kernel's
    element bound plus one 16-bit ulp (the fp32 reference's own error is far below it)."""
    from mio.synthetic import FusedRMSNorm
    d = 1024
    m = FusedRMSNorm(d, eps=eps).to(DEV)
    with torch.no_grad():
        m.weight.copy_(_rand((d,), dtype, 0.2, 1, shift=1.0).float())  # fp32 values the 16-bit cast keeps
    x = _rand((3, 50, d), dtype, 2.0, 2, shift=0.3)
    y = m(x)
    assert y.dtype == dtype and y.shape == x.shape
    e = eps if eps is not None else torch.finfo(dtype).eps
    want = F.rms_norm(x.float(), (d,), m.weight, e).double().reshape(-1, d)
    ref = rc.reference_rows(x.reshape(-1, d), m.weight.to(dtype), e, device=DEV)
    err = (y.double().reshape(-1, d) - want).abs()
    assert bool((err <= gc.element_bound(ref, dtype) + gc.ulp16(want, dtype)).all()), (err.max().item())


def _rel(a, b):
    return ((a.float() - b.float()).abs().mean() / b.float().abs().mean()).item()


def test_block_swiglu_rmsnorm_folded():
    """synthetic.Block(norm="rms", activation="swiglu") at the shapes and initialisation of
    test_gpu_modules.test_block_swiglu_layernorm_folded: both RMSNorms folded into the GEMMs, against the same block with separate
    RMSNorm kernels, under that test's bar."""
    from mio.synthetic import Block, FusedRMSNorm
    torch.manual_seed(9)
    d, H, I, B, S = 1024, 16, 2048, 4, 4096
    blk = Block(d, H, I, causal=True, precision="bf16", activation="swiglu", norm="rms").to(DEV, torch.bfloat16).eval()
    assert isinstance(blk.ln_1, FusedRMSNorm) and isinstance(blk.ln_2, FusedRMSNorm)
    with torch.no_grad():
        for p_ in blk.parameters():
            p_.copy_(torch.randn_like(p_) * 0.03)
        blk.ln_1.weight.add_(1.0)
        blk.ln_2.weight.add_(1.0)
        x = torch.randn(B, S, d, device=DEV, dtype=torch.bfloat16) + 0.3
        assert blk.stream_ok(B, S, torch.bfloat16)
        y = blk(x)
        ref = blk(x, fold=False)
    rel = _rel(y, ref)
    assert rel < 3e-3, rel


def test_block_gelu_rmsnorm_second_pass_through_stream():
    """A GELU block, second pass through a ResidualStream (ln_1 folded too), as
    test_gpu_modules.test_block_other_head_dims_layernorm_folded does, under its bars."""
    from mio.synthetic import Block
    from mio._nn import ResidualStream
    torch.manual_seed(10)
    d, H, I, B, S = 1024, 16, 2048, 4, 4096
    blk = Block(d, H, I, causal=True, precision="bf16", norm="rms").to(DEV, torch.bfloat16).eval()
    with torch.no_grad():
        for p_ in blk.parameters():
            p_.copy_(torch.randn_like(p_) * 0.02)
        blk.ln_1.weight.add_(1.0)
        blk.ln_2.weight.add_(1.0)
        x = torch.randn(B, S, d, device=DEV, dtype=torch.bfloat16) + 0.3
        assert blk.stream_ok(B, S, torch.bfloat16)
        s1 = blk(x, stream_out=True)
        assert isinstance(s1, ResidualStream)
        y = blk(s1)
        ref1 = blk(x, fold=False)
        ref = blk(ref1, fold=False)
    rel1, rel = _rel(s1.dense(), ref1), _rel(y, ref)
    assert rel1 < 3e-3 and rel < 4e-3, (rel1, rel)


def test_tensor_parallel_sublayer_refuses_rmsnorm():
    from mio.parallelism.tensor_parallel import TensorParallelMLP
    d = 256
    mlp = TensorParallelMLP(d, 2 * d, activation="gelu").to(DEV, torch.bfloat16)
    x = torch.zeros(2, 8, d, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(TypeError, match="LayerNorm"):
        mlp(x, residual=x, pre_norm=nn.RMSNorm(d).to(DEV, torch.bfloat16))

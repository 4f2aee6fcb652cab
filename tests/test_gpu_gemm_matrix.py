"""Every GEMM kernel route (mio._lib.GEMM_ROUTES) in bf16 and fp16 against the fp64 reference of tests/_gemm_check.py.

Each case first asserts the route its call takes (ops.gemm_route / ops.fused_mlp_route, the rule the launch switches on), then
judges the output with _gemm_check.check: finite, guards untouched, the first-principles element bound and the per-(dtype, route)
statistical bars.  Cases are listed per route in CASES; test_every_route_has_cases (no GPU) proves the table covers every route.
The LayerNorm-fold routes are not faithfully rounded (the weights are re-rounded by mio_ln_fold_weight): their cases assert the
route and judge the value with the bar of test_gpu_kernels.py's fold tests.  The cases beyond 32-bit offsets (an output over
4 GiB, an x over 2 GiB, row strides at and past the per-tile offset limit) check 16-row blocks on both sides of every 2^31- and
2^32-byte boundary and the last, ragged, row tile in fp64 on the GPU."""
import pytest
import torch

import _gemm_check as gc

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
STRIDE_MAX = 0x7fffffff // 512 // 8 * 8  # the longest row stride (elements) the 32-bit per-tile offsets take
ACTS = ["none", "gelu", "gelu_erf", "relu", "silu"]
FILL = -3.0e4                            # guard fill: no output of these cases comes near it


def _ops():
    from mio import ops
    return ops


def _rand(shape, dtype, scale=1.0, seed=0, shift=0.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(shape, device=DEV, generator=g) * scale + shift).to(dtype)


def _free():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _operands(dtype, M, N, K, act="none", bias=True, res=False, seed=0, ldx=None, gate=False, bias_gate=True):
    """x [M, K] (row stride ldx), w [N, K] scaled to unit-size outputs, bias, residual, gate weight / bias."""
    if ldx is None or ldx == K:
        x = _rand((M, K), dtype, seed=seed)
    else:  # a view of rows ldx apart in a buffer that ends with the last row
        buf = torch.empty((M - 1) * ldx + K, dtype=dtype, device=DEV)
        x = buf.as_strided((M, K), (ldx, 1))
        x.copy_(_rand((M, K), dtype, seed=seed))
    w = _rand((N, K), dtype, K ** -0.5, seed + 1)
    b = _rand((N,), dtype, 0.5, seed + 2) if bias else None
    r = _rand((M, N), dtype, 1.0, seed + 3) if res else None
    wg = _rand((N, K), dtype, K ** -0.5, seed + 4) if gate else None
    bg = _rand((N,), dtype, 0.5, seed + 5) if (gate and bias_gate) else None
    return x, w, b, r, wg, bg


def _gemm(dtype, route, M, N, K, act="none", bias=True, res=False, ldx=None, guard=False, blocked_w=False, blocked_x=False,
          col_scale=None, bias_gate=True, seed=0, what=""):
    """One gemm_bias_act call: route asserted, the whole output checked."""
    ops = _ops()
    gate = act == "swiglu"
    x, w, b, r, wg, bg = _operands(dtype, M, N, K, act, bias, res, seed, ldx, gate, bias_gate)
    kw = {}
    if res:
        kw["residual"] = r
    if gate:
        kw.update(w_gate=wg, bias_gate=bg)
    if blocked_w:
        kw["w_blocked"] = ops.block_weight(w)
    if col_scale is not None:
        kw["col_scale"] = col_scale
    buf = None
    if guard:  # the output as a view inside a buffer filled with FILL: one row and 16 columns on either side
        buf = torch.full((M + 2, N + 32), FILL, dtype=dtype, device=DEV)
        kw["out"] = buf[1:M + 1, 16:N + 16]
    xin = x
    if blocked_x:
        xin = ops.block_weight(x)  # the blocked activation layout is the blocked weight layout with m in the place of n
        kw["x_blocked_shape"] = (M, K)
    assert ops.gemm_route(xin, w, b, act, **kw) == route, what
    y = ops.gemm_bias_act(xin, w, b, act, **kw)
    ref = gc.reference(x, w, b, act, wg, bg, r, col_scale, device=DEV)
    gc.check(y, ref, dtype, route, guard=buf, fill=FILL, what=what)


# ---- the cases, per route: name -> callable(dtype) ---------------------------------------------------------------------
def _t128():
    c = {
        "m1_n8_k8": lambda dt: _gemm(dt, "t128", 1, 8, 8, res=True),
        "m37_n72_k4104_tail": lambda dt: _gemm(dt, "t128", 37, 72, 4104, bias=False),
        "x_stride_k_plus_8": lambda dt: _gemm(dt, "t128", 37, 72, 40, "gelu", ldx=48, res=True),
        "guarded_out": lambda dt: _gemm(dt, "t128", 37, 72, 40, "silu", guard=True, res=True),
        "m300_n512_k1024": lambda dt: _gemm(dt, "t128", 300, 512, 1024, "gelu", res=True),
    }
    for i, a in enumerate(ACTS):
        c[f"m37_n72_k40_{a}_bias"] = lambda dt, a=a: _gemm(dt, "t128", 37, 72, 40, a)
        c[f"m37_n8_k8_{a}_res_nobias"] = lambda dt, a=a: _gemm(dt, "t128", 37, 8, 8, a, bias=False, res=True)
    return c


def _t256():
    c = {}
    for i, K in enumerate((8, 40, 264, 64, 96)):
        for j, a in enumerate(ACTS):
            if (i + j) % 2 == 0 or K == 96:  # every K and every activation, half the grid
                c[f"k{K}_{a}"] = lambda dt, K=K, a=a: _gemm(dt, "t256", 4096, 4096, K, a, res=(K % 64 == 0), seed=K)
    c["k96_guarded"] = lambda dt: _gemm(dt, "t256", 4096 + 100, 4096 - 8, 96, "relu", guard=True)
    # x rows 4 Mi elements apart: the row stride is past the 32-bit per-tile offsets (a buffer of about 4 GiB)
    c["x_stride_past_limit"] = lambda dt: _gemm(dt, "t256", 512, 32768, 256, "gelu", ldx=STRIDE_MAX + 8)
    return c


def _p8w():
    c = {
        "tiles_256": lambda dt: _gemm(dt, "p8w", 65536, 256, 256, "gelu"),
        "tiles_257": lambda dt: _gemm(dt, "p8w", 65536 + 256, 256, 128),
        "skinny_m1": lambda dt: _gemm(dt, "p8w", 1, 65536, 128, "silu"),
        "skinny_m200_n_ragged8": lambda dt: _gemm(dt, "p8w", 200, 65536 + 8, 160),
        "skinny_n8": lambda dt: _gemm(dt, "p8w", 65536, 8, 256, "relu"),
        "skinny_n24": lambda dt: _gemm(dt, "p8w", 65536 + 100, 24, 544, "gelu"),
        "k4096": lambda dt: _gemm(dt, "p8w", 4096, 4096, 4096),
        "n_ragged248_k160": lambda dt: _gemm(dt, "p8w", 4096, 4096 - 248, 160, "gelu_erf", bias=False),
        "blocked_w_k544": lambda dt: _gemm(dt, "p8w", 4096 + 37, 4096 + 8, 544, "silu", blocked_w=True),
        "blocked_x": lambda dt: _gemm(dt, "p8w", 4096 + 37, 4096, 256, "gelu", blocked_w=True, blocked_x=True),
        "col_scale_all": lambda dt: _gemm(dt, "p8w", 4096, 4096, 256, col_scale=(0, 4096, 0.125), blocked_w=True),
        "col_scale_band_to_n": lambda dt: _gemm(dt, "p8w", 8192 + 100, 3072 + 128, 512, "gelu",
                                                col_scale=(2048, 3072 + 128, 0.18033688), blocked_w=True),
        "guarded_out": lambda dt: _gemm(dt, "p8w", 4096 + 100, 4096 - 8, 128, guard=True),
        "out_stride_at_limit": lambda dt: _strided_out(dt),
    }
    for a in ACTS:
        c[f"act_{a}_k128"] = lambda dt, a=a: _gemm(dt, "p8w", 4096 + 1, 4096, 128, a, seed=3)
    return c


def _p8w_res():
    c = {
        "tiles_256": lambda dt: _gemm(dt, "p8w_res", 4096, 4096, 128, res=True),
        "tiles_257": lambda dt: _gemm(dt, "p8w_res", 65536 + 256, 256, 160, "gelu", res=True),
        "skinny_m1": lambda dt: _gemm(dt, "p8w_res", 1, 65536, 128, res=True),
        "skinny_n8": lambda dt: _gemm(dt, "p8w_res", 65536 + 13, 8, 544, "silu", res=True),
        "k4096": lambda dt: _gemm(dt, "p8w_res", 4096 + 100, 4096 + 8, 4096, res=True),
        "n_ragged248_nobias": lambda dt: _gemm(dt, "p8w_res", 4096, 4096 - 248, 256, "relu", bias=False, res=True),
        "blocked_w_x": lambda dt: _gemm(dt, "p8w_res", 4096 + 37, 4096, 256, blocked_w=True, blocked_x=True, res=True),
        "guarded_out": lambda dt: _gemm(dt, "p8w_res", 4096 + 100, 4096 - 8, 160, "gelu", guard=True, res=True),
    }
    for a in ACTS:
        c[f"act_{a}"] = lambda dt, a=a: _gemm(dt, "p8w_res", 4096 + 1, 4096, 128, a, res=True, blocked_w=True, seed=5)
    return c


def _glu_t128x64():
    return {
        "m37_n72_k40": lambda dt: _gemm(dt, "glu_t128x64", 37, 72, 40, "swiglu"),
        "n_ragged_no_bias": lambda dt: _gemm(dt, "glu_t128x64", 300, 200, 264, "swiglu", bias=False),
        "n_ragged_no_bias_gate": lambda dt: _gemm(dt, "glu_t128x64", 300, 1000, 1024, "swiglu", bias_gate=False),
        "guarded_out": lambda dt: _gemm(dt, "glu_t128x64", 129, 136, 72, "swiglu", guard=True),
    }


def _glu_t256x128():
    return {
        "n4104": lambda dt: _gemm(dt, "glu_t256x128", 4096, 4096 + 8, 256, "swiglu"),
        "n_ragged_no_bias_k40": lambda dt: _gemm(dt, "glu_t256x128", 4096 + 100, 2048 - 8, 40, "swiglu", bias=False),
        "guarded_no_bias_gate": lambda dt: _gemm(dt, "glu_t256x128", 4096 + 1, 2048 + 8, 1024, "swiglu", guard=True,
                                                 bias_gate=False),
    }


def _glu_ln(dtype, route, M, N, K, fold=False, seed=0, what=""):
    """The gated stage through block_weight_glu + gemm_ln (plain, or the LayerNorm consumer behind a producer's statistics)."""
    ops = _ops()
    x, wu, bu, _, wg, bg = _operands(dtype, M, N, K, "swiglu", True, False, seed, gate=True)
    if not fold:
        wb = ops.block_weight_glu(wg, wu)
        assert ops.gemm_route(x, wb, bu, "swiglu", M=M, N=N, K=K, bias_gate=bg) == route
        h, _ = ops.gemm_ln(x, wb, bu, M=M, N=N, K=K, activation="swiglu", bias_gate=bg)
        gc.check(h, gc.reference(x, wu, bu, "swiglu", wg, bg, device=DEV), dtype, route, what=what)
        return
    _fold_case(dtype, route, M, N, K, "swiglu", seed)


def _fold_case(dtype, route, M, N, K, act, seed=0):
    """Producer (residual GEMM + statistics) -> consumer with the LayerNorm folded into its weights: route asserted, value
    against the fp64 LayerNorm -> linear with the bar of the fold tests in test_gpu_kernels.py (the fold re-rounds the weights)."""
    import oracle
    from test_gpu_kernels import _cmp
    ops = _ops()
    x0 = _rand((M, K), dtype, seed=seed)
    r0 = _rand((M, K), dtype, 2.0, seed + 1, shift=1.0)
    wp, bp = _rand((K, K), dtype, 0.03, seed + 2), _rand((K,), dtype, 0.1, seed + 3)
    gam, bet = _rand((K,), dtype, 0.2, seed + 4, shift=1.0), _rand((K,), dtype, 0.1, seed + 5)
    wc, bc = _rand((N, K), dtype, 0.03, seed + 6), _rand((N,), dtype, 0.1, seed + 7)
    y, st = ops.gemm_ln(x0, ops.block_weight(wp), bp, M=M, N=K, K=K, residual=r0, stats_out=True)
    rows = torch.cat([torch.arange(0, M, 97, device=DEV), torch.tensor([255, 256, M - 1], device=DEV)])
    ln = oracle.layernorm(y[rows].cpu(), gam.cpu(), bet.cpu(), 1e-5).double()
    if act == "swiglu":
        wg, bg = _rand((N, K), dtype, 0.03, seed + 8), _rand((N,), dtype, 0.1, seed + 9)
        wgf, bgf = ops.ln_fold_weight(wg, gam, bet, bg, blocked=False)
        wuf, buf = ops.ln_fold_weight(wc, gam, bet, bc, blocked=False)
        wb = ops.block_weight_glu(wgf, wuf)
        assert ops.gemm_route(y, wb, buf, "swiglu", M=M, N=N, K=K, ln_stats=st, bias_gate=bgf) == route
        z, _ = ops.gemm_ln(y, wb, buf, M=M, N=N, K=K, activation="swiglu", ln_stats=st, bias_gate=bgf)
        want = torch.nn.functional.silu(ln @ wg.cpu().double().t() + bg.cpu().double()) * \
            (ln @ wc.cpu().double().t() + bc.cpu().double())
    else:
        wfb, bfold = ops.ln_fold_weight(wc, gam, bet, bc)
        assert ops.gemm_route(y, wfb, bfold, act, M=M, N=N, K=K, ln_stats=st) == route
        z, _ = ops.gemm_ln(y, wfb, bfold, M=M, N=N, K=K, activation=act, ln_stats=st)
        want = ln @ wc.cpu().double().t() + bc.cpu().double()
        if act == "gelu":
            want = torch.nn.functional.gelu(want, approximate="tanh")
    assert torch.isfinite(z).all()
    _cmp(z[rows], want, dtype, f"{route} {act}")


def _p8w_glu():
    return {
        "gemm_ln_n2048": lambda dt: _glu_ln(dt, "p8w_glu", 4096, 2048, 256),
        "gemm_ln_ragged_m_k1024": lambda dt: _glu_ln(dt, "p8w_glu", 4096 + 100, 2048, 1024, seed=2),
        "fused_mlp_blocked": lambda dt: _mlp(dt, "swiglu", True, True, "p8w_glu"),
    }


def _p8w_glu_fold():
    return {"gemm_ln_fold": lambda dt: _glu_ln(dt, "p8w_glu_fold", 16500, 2048, 1024, fold=True)}


def _p8w_fold():
    return {
        "none": lambda dt: _fold_case(dt, "p8w_fold", 16500, 2048, 1024, "none"),
        "gelu": lambda dt: _fold_case(dt, "p8w_fold", 16500, 2048, 1024, "gelu", seed=1),
    }


def _stats_case(dtype, M, N, K, seed=0):
    """The producer form: y = x w^T + b + r checked as p8w_stats, and stats_out[slot][row] = (sum, sum of squares) of the
    kernel's own stored y over the slot's 256 columns, against fp64 within the fp32 summation bound gamma_n sum |terms|."""
    ops = _ops()
    x, w, b, r, _, _ = _operands(dtype, M, N, K, res=True, seed=seed)
    wb = ops.block_weight(w)
    assert ops.gemm_route(x, wb, b, M=M, N=N, K=K, residual=r, stats_out=True) == "p8w_stats"
    y, st = ops.gemm_ln(x, wb, b, M=M, N=N, K=K, residual=r, stats_out=True)
    gc.check(y, gc.reference(x, w, b, residual=r, device=DEV), dtype, "p8w_stats")
    yf = y.double().view(M, N // 256, 256)
    s, q = yf.sum(-1).t(), (yf * yf).sum(-1).t()
    gam = lambda n: n * gc.U32 / (1 - n * gc.U32)  # noqa: E731  (any order, an accumulator that truncates included)
    bs, bq = gam(256) * yf.abs().sum(-1).t(), gam(257) * (yf * yf).sum(-1).t()
    es, eq = (st[:, :M, 0].double() - s).abs(), (st[:, :M, 1].double() - q).abs()
    assert bool((es <= bs).all()), f"row sums off by {(es / bs).max().item():.3g} x the bound"
    assert bool((eq <= bq).all()), f"row sums of squares off by {(eq / bq).max().item():.3g} x the bound"


def _p8w_stats():
    return {
        "n1024_k1024": lambda dt: _stats_case(dt, 16500, 1024, 1024),
        "n256_k128_tiles_257": lambda dt: _stats_case(dt, 65536 + 256, 256, 128, seed=1),
        "n2048_k4096": lambda dt: _stats_case(dt, 8192 + 7, 2048, 4096, seed=2),
    }


def _empty():
    def run(dt):
        ops = _ops()
        x, w = torch.empty(0, 64, dtype=dt, device=DEV), _rand((128, 64), dt)
        assert ops.gemm_route(x, w) == "empty"
        y = ops.gemm_bias_act(x, w, None, "gelu")
        assert tuple(y.shape) == (0, 128)
    return {"m0": run}


CASES = {
    "empty": _empty(),
    "t128": _t128(),
    "t256": _t256(),
    "p8w": _p8w(),
    "p8w_res": _p8w_res(),
    "p8w_fold": _p8w_fold(),
    "p8w_stats": _p8w_stats(),
    "glu_t128x64": _glu_t128x64(),
    "glu_t256x128": _glu_t256x128(),
    "p8w_glu": _p8w_glu(),
    "p8w_glu_fold": _p8w_glu_fold(),
}


def test_every_route_has_cases():
    """No GPU: every route of mio._lib.GEMM_ROUTES has cases here, and each case runs in both dtypes (test_gemm_route)."""
    from mio import _lib
    assert set(CASES) == set(_lib.GEMM_ROUTES.values())
    for route, cases in CASES.items():
        assert len(cases) >= 1, route
    assert len(CASES["empty"]) == 1
    ids = {(r, n, str(dt)) for r, n, dt in _PARAMS}
    for route, cases in CASES.items():
        for name in cases:
            assert all((route, name, str(dt)) in ids for dt in DTYPES), (route, name)


_PARAMS = [(r, n, dt) for r in CASES for n in CASES[r] for dt in DTYPES]


@pytest.mark.gpu
@pytest.mark.parametrize("route,name,dtype", _PARAMS, ids=[f"{r}-{n}-{str(d).split('.')[-1]}" for r, n, d in _PARAMS])
def test_gemm_route(route, name, dtype):
    try:
        CASES[route][name](dtype)
    finally:
        _free()


# ---- the output beyond 32-bit offsets: p8w at 4 GiB of y, 2 GiB of x, a row stride at the limit -------------------------------
def _blocks_around(byte_offsets, row_bytes, M):
    """16-row blocks on both sides of each byte boundary, the first rows and the last, ragged, row tile."""
    starts = {0}
    for b in byte_offsets:
        r = b // row_bytes
        starts.add(max(0, min(M - 16, r - 8)))
        starts.add(max(0, min(M - 16, r + 1)))
    last = (M - 1) // 256 * 256
    rows = sorted({i for s in starts for i in range(s, s + 16)} | set(range(last, M)))
    return torch.tensor(rows, device=DEV)


def _sampled(dtype, route, M, N, K, act, row_boundaries_of, seed=0):
    ops = _ops()
    x, w, b, _, _, _ = _operands(dtype, M, N, K, act, True, False, seed)
    assert ops.gemm_route(x, w, b, act) == route
    y = ops.gemm_bias_act(x, w, b, act)
    rows = row_boundaries_of(M, N, K)
    ref = gc.reference(x[rows], w, b, act, device=DEV)
    gc.check(y[rows], ref, dtype, route, what=f"sampled rows of M {M} N {N} K {K}")
    del y, x


def _strided_out(dtype):
    """y with a row stride just under the per-tile offset limit, a ragged last row tile (44 of 256 rows): the kernel's dropped
    out-of-range stores run at the largest offsets its buffer descriptors reach; the gap between rows is a guard."""
    ops = _ops()
    M, N, K = 300, 32768, 128
    x, w, b, _, _, _ = _operands(dtype, M, N, K, "gelu", True, False, 7)
    buf = torch.full((M * STRIDE_MAX,), FILL, dtype=dtype, device=DEV)
    y = buf.as_strided((M, N), (STRIDE_MAX, 1))
    assert ops.gemm_route(x, w, b, "gelu", out=y) == "p8w"
    ops.gemm_bias_act(x, w, b, "gelu", out=y)
    gc.check(y, gc.reference(x, w, b, "gelu", device=DEV), dtype, "p8w", guard=buf, fill=FILL, what="row stride at the limit")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_output_over_4gib(dtype):
    """M 2^20 + 100, N 2056 (ragged by 8), K 128: 4.3 GB of output."""
    torch.cuda.reset_peak_memory_stats()
    try:
        _sampled(dtype, "p8w", (1 << 20) + 100, 2048 + 8, 128, "gelu",
                 lambda M, N, K: _blocks_around([1 << 31, 1 << 32], N * 2, M))
    finally:
        _free()
    assert torch.cuda.max_memory_allocated() < 16e9


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_x_over_2gib(dtype):
    """M 270000 (ragged), K 4096: 2.2 GB of x; N 264."""
    try:
        _sampled(dtype, "p8w", 270000, 256 + 8, 4096, "none", lambda M, N, K: _blocks_around([1 << 31], K * 2, M), seed=4)
    finally:
        _free()


@pytest.mark.gpu
def test_gemm_fp16_subnormal_outputs():
    """Normal fp16 inputs near 2^-12 whose products land in the subnormal range: the element bound with the fixed 2^-24
    spacing, on the 128x128 and the persistent kernels."""
    ops = _ops()
    dt = torch.float16
    for route, (M, N, K) in (("t128", (37, 72, 40)), ("p8w", (4096, 4096, 256)), ("t256", (4096, 4096, 96))):
        g = torch.Generator(device=DEV).manual_seed(M)
        x = ((torch.rand(M, K, device=DEV, generator=g) + 1) * 2.0 ** -12).to(dt)
        sign = torch.where(torch.rand(N, K, device=DEV, generator=g) < 0.5, -1.0, 1.0)
        w = (sign * (torch.rand(N, K, device=DEV, generator=g) + 1) * 2.0 ** -11).to(dt)  # normal, |w| in [2^-11, 2^-10)
        assert ops.gemm_route(x, w) == route
        y = ops.gemm_bias_act(x, w)
        ref = gc.reference(x, w, device=DEV)
        assert ref.y.abs().max().item() < 2.0 ** -14
        gc.check(y, ref, dt, route, bars=False, what="subnormal outputs")
        _free()


# ---- fused MLP: both paths, every activation, ragged M, with and without residual -------------------------------------------
def _mlp(dtype, act, blocked, res, want1=None, seed=0):
    ops = _ops()
    if blocked:
        M, d, I = 16384 + 100, 1024, 1024
    else:
        M, d, I = 300 + 5, 256, 512
    x = _rand((1, M, d), dtype, seed=seed)
    w1, b1 = _rand((I, d), dtype, d ** -0.5, seed + 1), _rand((I,), dtype, 0.5, seed + 2)
    w2, b2 = _rand((d, I), dtype, I ** -0.5, seed + 3), _rand((d,), dtype, 0.5, seed + 4)
    wg, bg = (_rand((I, d), dtype, d ** -0.5, seed + 5), _rand((I,), dtype, 0.5, seed + 6)) if act == "swiglu" else (None, None)
    r = _rand((1, M, d), dtype, seed=seed + 7) if res else None
    kw = {}
    if blocked and (act == "swiglu" or res):  # blocked weights; else the plain weights on the same two-stage path
        kw["fc1_blocked"] = ops.block_weight_glu(wg, w1) if act == "swiglu" else ops.block_weight(w1)
        kw["fc2_blocked"] = ops.block_weight(w2)
    rt = ops.fused_mlp_route(x, w1, b1, w2, b2, act, wg, bg, residual=r, **kw)
    want = {"path": "blocked" if blocked else "two_launch",
            "stage1": want1 or (("p8w_glu" if act == "swiglu" else "p8w") if blocked else
                                ("glu_t128x64" if act == "swiglu" else "t128")),
            "stage2": ("p8w_res" if res else "p8w") if blocked else "t128"}
    assert rt == want, rt
    y = ops.fused_mlp(x, w1, b1, w2, b2, act, wg, bg, residual=r, **kw)
    ref = gc.reference_mlp(x[0], w1, b1, w2, b2, act, wg, bg, None if r is None else r[0], device=DEV)
    gc.check(y[0], ref, dtype, rt["stage2"], what=f"fused mlp {act} {rt['path']}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("blocked", [True, False], ids=["blocked", "two_launch"])
@pytest.mark.parametrize("act", ["gelu", "gelu_erf", "relu", "silu", "swiglu"])
def test_fused_mlp_paths(dtype, blocked, act):
    try:
        for res in (False, True):
            _mlp(dtype, act, blocked, res, seed=3 * res)
            _free()
    finally:
        _free()

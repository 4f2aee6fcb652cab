"""Every GEMM kernel route (mio._lib.GEMM_ROUTES) in bf16 and fp16 against the fp64 reference of tests/_gemm_check.py.

Each case first asserts the route its call takes (ops.gemm_route / ops.fused_mlp_route, the rule the launch switches on), then
judges the output with _gemm_check.check: finite, guards untouched, the first-principles element bound and the per-(dtype, route)
statistical bars.  Cases are listed per route in CASES; test_every_route_has_cases (no GPU) proves the table covers every route.
The LayerNorm-fold routes are judged against _gemm_check.reference_fold, built from what the consumer reads (the stream, the
statistics handed to the launch, the folded weights and biases).  The cases beyond 32-bit offsets (an output over
4 GiB, an x over 2 GiB, row strides at and past the per-tile offset limit) check 16-row blocks on both sides of every 2^31- and
2^32-byte boundary and the last, ragged, row tile in fp64 on the GPU."""
from types import SimpleNamespace

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


class Parts:
    """A case in three callables, so that tests/test_gpu_repeatable.py can repeat the launch alone:
    build(dtype) -> p, a SimpleNamespace of the operands (route asserted by the host query); launch(p) -> what the call returns,
    reading its operands from p only; judge(p, ret): the checks.  Calling the case runs the three in order."""

    def __init__(self, build, launch, judge):
        self.build, self.launch, self.judge = build, launch, judge

    def __call__(self, dtype):
        p = self.build(dtype)
        self.judge(p, self.launch(p))


def _gemm_build(dtype, route, M, N, K, act="none", bias=True, res=False, ldx=None, guard=False, blocked_w=False, blocked_x=False,
                col_scale=None, bias_gate=True, seed=0, what=""):
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
    p = SimpleNamespace(dtype=dtype, route=route, shape=(M, N, K), act=act, x=x, xin=xin, w=w, b=b, r=r, wg=wg, bg=bg, kw=kw,
                        buf=buf, col_scale=col_scale, what=what)
    assert _gemm_route_of(p) == route, what
    return p


def _gemm_route_of(p):
    return _ops().gemm_route(p.xin, p.w, p.b, p.act, **p.kw)


def _gemm_launch(p):
    return _ops().gemm_bias_act(p.xin, p.w, p.b, p.act, **p.kw)


def _gemm_judge(p, y):
    ref = gc.reference(p.x, p.w, p.b, p.act, p.wg, p.bg, p.r, p.col_scale, device=DEV)
    gc.check(y, ref, p.dtype, p.route, guard=p.buf, fill=FILL, what=p.what)


def _gemm_parts(route, M, N, K, act="none", **kw):
    """One gemm_bias_act call: route asserted, the whole output checked."""
    return Parts(lambda dt: _gemm_build(dt, route, M, N, K, act, **kw), _gemm_launch, _gemm_judge)


# ---- the cases, per route: name -> callable(dtype) ---------------------------------------------------------------------
def _t128():
    c = {
        "m1_n8_k8": _gemm_parts("t128", 1, 8, 8, res=True),
        "m37_n72_k4104_tail": _gemm_parts("t128", 37, 72, 4104, bias=False),
        "x_stride_k_plus_8": _gemm_parts("t128", 37, 72, 40, "gelu", ldx=48, res=True),
        "guarded_out": _gemm_parts("t128", 37, 72, 40, "silu", guard=True, res=True),
        "m300_n512_k1024": _gemm_parts("t128", 300, 512, 1024, "gelu", res=True),
    }
    for i, a in enumerate(ACTS):
        c[f"m37_n72_k40_{a}_bias"] = _gemm_parts("t128", 37, 72, 40, a)
        c[f"m37_n8_k8_{a}_res_nobias"] = _gemm_parts("t128", 37, 8, 8, a, bias=False, res=True)
    return c


def _t256():
    c = {}
    for i, K in enumerate((8, 40, 264, 64, 96)):
        for j, a in enumerate(ACTS):
            if (i + j) % 2 == 0 or K == 96:  # every K and every activation, half the grid
                c[f"k{K}_{a}"] = _gemm_parts("t256", 4096, 4096, K, a, res=(K % 64 == 0), seed=K)
    c["k96_guarded"] = _gemm_parts("t256", 4096 + 100, 4096 - 8, 96, "relu", guard=True)
    # x rows 4 Mi elements apart: the row stride is past the 32-bit per-tile offsets (a buffer of about 4 GiB)
    c["x_stride_past_limit"] = _gemm_parts("t256", 512, 32768, 256, "gelu", ldx=STRIDE_MAX + 8)
    return c


def _p8w():
    c = {
        "tiles_256": _gemm_parts("p8w", 65536, 256, 256, "gelu"),
        "tiles_257": _gemm_parts("p8w", 65536 + 256, 256, 128),
        "skinny_m1": _gemm_parts("p8w", 1, 65536, 128, "silu"),
        "skinny_m200_n_ragged8": _gemm_parts("p8w", 200, 65536 + 8, 160),
        "skinny_n8": _gemm_parts("p8w", 65536, 8, 256, "relu"),
        "skinny_n24": _gemm_parts("p8w", 65536 + 100, 24, 544, "gelu"),
        "k4096": _gemm_parts("p8w", 4096, 4096, 4096),
        "n_ragged248_k160": _gemm_parts("p8w", 4096, 4096 - 248, 160, "gelu_erf", bias=False),
        "blocked_w_k544": _gemm_parts("p8w", 4096 + 37, 4096 + 8, 544, "silu", blocked_w=True),
        "blocked_x": _gemm_parts("p8w", 4096 + 37, 4096, 256, "gelu", blocked_w=True, blocked_x=True),
        "col_scale_all": _gemm_parts("p8w", 4096, 4096, 256, col_scale=(0, 4096, 0.125), blocked_w=True),
        "col_scale_band_to_n": _gemm_parts("p8w", 8192 + 100, 3072 + 128, 512, "gelu",
                                                col_scale=(2048, 3072 + 128, 0.18033688), blocked_w=True),
        "guarded_out": _gemm_parts("p8w", 4096 + 100, 4096 - 8, 128, guard=True),
        "out_stride_at_limit": lambda dt: _strided_out(dt),
    }
    for a in ACTS:
        c[f"act_{a}_k128"] = _gemm_parts("p8w", 4096 + 1, 4096, 128, a, seed=3)
    return c


def _p8w_res():
    c = {
        "tiles_256": _gemm_parts("p8w_res", 4096, 4096, 128, res=True),
        "tiles_257": _gemm_parts("p8w_res", 65536 + 256, 256, 160, "gelu", res=True),
        "skinny_m1": _gemm_parts("p8w_res", 1, 65536, 128, res=True),
        "skinny_n8": _gemm_parts("p8w_res", 65536 + 13, 8, 544, "silu", res=True),
        "k4096": _gemm_parts("p8w_res", 4096 + 100, 4096 + 8, 4096, res=True),
        "n_ragged248_nobias": _gemm_parts("p8w_res", 4096, 4096 - 248, 256, "relu", bias=False, res=True),
        "blocked_w_x": _gemm_parts("p8w_res", 4096 + 37, 4096, 256, blocked_w=True, blocked_x=True, res=True),
        "guarded_out": _gemm_parts("p8w_res", 4096 + 100, 4096 - 8, 160, "gelu", guard=True, res=True),
    }
    for a in ACTS:
        c[f"act_{a}"] = _gemm_parts("p8w_res", 4096 + 1, 4096, 128, a, res=True, blocked_w=True, seed=5)
    return c


def _glu_t128x64():
    return {
        "m37_n72_k40": _gemm_parts("glu_t128x64", 37, 72, 40, "swiglu"),
        "n_ragged_no_bias": _gemm_parts("glu_t128x64", 300, 200, 264, "swiglu", bias=False),
        "n_ragged_no_bias_gate": _gemm_parts("glu_t128x64", 300, 1000, 1024, "swiglu", bias_gate=False),
        "guarded_out": _gemm_parts("glu_t128x64", 129, 136, 72, "swiglu", guard=True),
    }


def _glu_t256x128():
    return {
        "n4104": _gemm_parts("glu_t256x128", 4096, 4096 + 8, 256, "swiglu"),
        "n_ragged_no_bias_k40": _gemm_parts("glu_t256x128", 4096 + 100, 2048 - 8, 40, "swiglu", bias=False),
        "guarded_no_bias_gate": _gemm_parts("glu_t256x128", 4096 + 1, 2048 + 8, 1024, "swiglu", guard=True,
                                                 bias_gate=False),
    }


def _ln_route_of(p):
    """The route of a gemm_ln launch described by p (x, wb, b, kw)."""
    return _ops().gemm_route(p.x, p.wb, p.b, **p.kw)


def _ln_launch(p):
    return _ops().gemm_ln(p.x, p.wb, p.b, **p.kw)


def _glu_ln_build(dtype, route, M, N, K, seed=0, what=""):
    ops = _ops()
    x, wu, bu, _, wg, bg = _operands(dtype, M, N, K, "swiglu", True, False, seed, gate=True)
    wb = ops.block_weight_glu(wg, wu)
    p = SimpleNamespace(dtype=dtype, route=route, shape=(M, N, K), x=x, wb=wb, b=bu, wu=wu, wg=wg, bg=bg, what=what,
                        kw=dict(M=M, N=N, K=K, activation="swiglu", bias_gate=bg))
    assert _ln_route_of(p) == route
    return p


def _glu_ln_judge(p, ret):
    gc.check(ret[0], gc.reference(p.x, p.wu, p.b, "swiglu", p.wg, p.bg, device=DEV), p.dtype, p.route, what=p.what)


def _glu_ln_parts(route, M, N, K, **kw):
    """The gated stage through block_weight_glu + gemm_ln."""
    return Parts(lambda dt: _glu_ln_build(dt, route, M, N, K, **kw), _ln_launch, _glu_ln_judge)


EPS = 1e-5


def _built_stats(y, pad):
    """The consumer's statistics built by the test: fp64 slot sums of the stored stream rounded to fp32, rows past M = pad."""
    M, K = y.shape
    st = torch.full(_ops().ln_stats_shape(M, K), pad, dtype=torch.float32, device=DEV)
    yd = y.double().view(M, K // 256, 256)
    st[:, :M, 0] = yd.sum(-1).t().float()
    st[:, :M, 1] = (yd * yd).sum(-1).t().float()
    return st


def _fold_stream(dtype, M, K, seed, mean=1.0):
    """(y, statistics): the residual stream and its row statistics from the real producer (gemm_ln(..., residual=,
    stats_out=True), the chain the modules run) where that GEMM [M, K, K] has the tiles for the 256-tile kernels -- with
    M = MR from K 2048 on, at K 256 with M 65436 and at K 1024 with M 16500 -- row mean about mean / 2.2 deviations (the
    residual's 2 and the product's 1 add to sqrt 5).  Else (MR with K 256, 768, 1024) the residual alone with statistics built
    by the test and NaN in the rows past M: row mean mean / 2 deviations."""
    ops = _ops()
    r0 = _rand((M, K), dtype, 2.0, seed + 1, shift=mean)
    if ops.gemm_ln_ok(M, K, K, "none", stats_out=True):
        x0 = _rand((M, K), dtype, seed=seed)
        wp, bp = _rand((K, K), dtype, K ** -0.5, seed + 2), _rand((K,), dtype, 0.1, seed + 3)
        return ops.gemm_ln(x0, ops.block_weight(wp), bp, M=M, N=K, K=K, residual=r0, stats_out=True)
    return r0, _built_stats(r0, float("nan"))


def _seam_rows(M):
    """16-row blocks: the first rows, both sides of every 256-row tile seam, the whole ragged last tile."""
    return _blocks_around([256 * k for k in range(1, (M - 1) // 256 + 1)], 1, M)


def _fold_consumer(dtype, route, y, st, N, act, seed, col_scale=None, blocked=False, bars=True, what=""):
    """One consumer launch on the stream y with the statistics st: the route asserted, the output judged by gc.check against
    gc.reference_fold of what the kernel reads -- the whole output, or at K >= 4096 (where the fp64 reference is large) the
    16-row blocks of _seam_rows.  Returns (z, folded bias, the launch's keyword arguments)."""
    p = _fold_build(dtype, route, y, st, N, act, seed, col_scale, what)
    z, none = _ln_launch(p)
    _fold_judge(p, (z, none), blocked=blocked, bars=bars)
    return z, p.b, (p.wb, p.kw)


def _fold_build(dtype, route, y, st, N, act, seed, col_scale=None, what=""):
    """The consumer's operands on the stream y (p.x) with the statistics st: the folded weights, the launch's keyword arguments,
    the route asserted."""
    ops = _ops()
    M, K = y.shape
    gam, bet = _rand((K,), dtype, 0.2, seed + 4, shift=1.0), _rand((K,), dtype, 0.1, seed + 5)
    wc, bc = _rand((N, K), dtype, K ** -0.5, seed + 6), _rand((N,), dtype, 0.1, seed + 7)
    ws, bfold = ops.ln_fold_weight(wc, gam, bet, bc, blocked=False)
    kw = dict(M=M, N=N, K=K, activation=act, ln_stats=st, eps=EPS)
    rkw = {}
    if act == "swiglu":
        wg, bg = _rand((N, K), dtype, K ** -0.5, seed + 8), _rand((N,), dtype, 0.1, seed + 9)
        wgs, bgf = ops.ln_fold_weight(wg, gam, bet, bg, blocked=False)
        wb = ops.block_weight_glu(wgs, ws)
        kw["bias_gate"] = bgf
        rkw = dict(ws_gate=wgs, bias_gate=bgf)
    else:
        wb, bfold2 = ops.ln_fold_weight(wc, gam, bet, bc)
        assert torch.equal(wb, ops.block_weight(ws)) and torch.equal(bfold2, bfold), "the blocked fold is not block_weight(ws)"
    if col_scale is not None:
        kw["col_scale"] = col_scale
    p = SimpleNamespace(dtype=dtype, route=route, shape=(M, N, K), act=act, x=y, wb=wb, b=bfold, kw=kw, ws=ws, rkw=rkw,
                        col_scale=col_scale, what=what)
    assert _ln_route_of(p) == route, what
    return p


def _fold_judge(p, ret, blocked=False, bars=True):
    ops = _ops()
    z, none = ret
    (M, N, K), y, kw = p.shape, p.x, p.kw
    assert none is None and tuple(z.shape) == (M, N)
    if blocked:  # the same launch through the blocked activation layout on both sides: bit for bit
        from test_gpu_kernels import _block, _unblock
        zb, _ = ops.gemm_ln(_block(y), p.wb, p.b, x_blocked=True, out_blocked=True, **kw)
        assert torch.equal(_unblock(zb, M, N), z), "blocked x / blocked output differs from the row-major launch"
    stl = ops.ln_stats_for_launch(kw["ln_stats"], M)  # what gemm_ln itself hands to the launch (the same call gives the same bits)
    rows = _seam_rows(M) if K >= 4096 else None
    pick = (lambda t: t) if rows is None else (lambda t: t[rows])  # noqa: E731
    ref = gc.reference_fold(pick(y), stl[:, :M] if rows is None else stl[:, rows], p.ws, p.b, eps=EPS, act=p.act,
                            col_scale=p.col_scale, device=DEV, **p.rkw)
    gc.check(pick(z), ref, p.dtype, p.route, bars=bars, what=p.what or f"fold M {M} N {N} K {K} {p.act}")


def _fold_parts(route, M, N, K, act, seed=0, mean=1.0, produced=False, col_scale=None, blocked=False, bars=True, what=""):
    """Producer (residual GEMM + statistics) -> consumer with the LayerNorm folded into its weights.  produced=True: the case
    relies on the real producer's stream (its mean in deviations)."""
    def build(dtype):
        assert not produced or _ops().gemm_ln_ok(M, K, K, "none", stats_out=True)
        y, st = _fold_stream(dtype, M, K, seed, mean)
        return _fold_build(dtype, route, y, st, N, act, seed, col_scale, what)

    return Parts(build, _ln_launch, lambda p, ret: _fold_judge(p, ret, blocked=blocked, bars=bars))


def _adversarial_stream(dtype, M, K, seed):
    """A stream no producer would write: row scales log-uniform over 1e-2 .. 1e2 and shuffled, row means of 0, 1, 4 and 32
    deviations, and in every 64 rows one of zeros, one constant and one with a single non-zero element."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    scale = 10.0 ** (torch.rand(M, 1, device=DEV, generator=g) * 4 - 2)
    mean = torch.tensor([0.0, 1.0, 4.0, 32.0], device=DEV)[torch.arange(M, device=DEV) % 4][:, None]
    y = (torch.randn(M, K, device=DEV, generator=g) + mean) * scale
    i = torch.arange(M, device=DEV)
    zero, const, single = i % 64 == 5, i % 64 == 17, i % 64 == 29
    y[zero] = 0
    y[const] = scale[const].expand(-1, K)
    y[single] = 0
    y[single, (i[single] * 37) % K] = scale[single, 0]
    return y.to(dtype), zero


def _fold_adversarial(dtype, route, M, N, K, act, seed=0):
    """The adversarial stream with statistics built by the test and NaN in the statistics rows past M (which the producer never
    writes and the consumer reads): finite, inside the element bound everywhere, a zero row gives exactly b' (act none), and
    the output is bit for bit that of the same launch with the padding rows zeroed.  No bars: relative row statistics mean
    nothing on degenerate rows."""
    ops = _ops()
    y, zero = _adversarial_stream(dtype, M, K, seed)
    assert (M + 255) // 256 * 256 - M >= 7
    z, bfold, (wb, kw) = _fold_consumer(dtype, route, y, _built_stats(y, float("nan")), N, act, seed, bars=False,
                                        what=f"adversarial stream {act}")
    if act == "none":
        assert torch.equal(z[zero], bfold.expand(int(zero.sum()), N)), "a zero row is not the folded bias"
    kw["ln_stats"] = _built_stats(y, 0.0)
    z0, _ = ops.gemm_ln(y, wb, bfold, **kw)
    assert torch.equal(z0, z), "the statistics rows past M reach the output"


def _p8w_glu():
    return {
        "gemm_ln_n2048": _glu_ln_parts("p8w_glu", 4096, 2048, 256),
        "gemm_ln_ragged_m_k1024": _glu_ln_parts("p8w_glu", 4096 + 100, 2048, 1024, seed=2),
        "fused_mlp_blocked": lambda dt: _mlp(dt, "swiglu", True, True, "p8w_glu"),
    }


MR = 8192 - 7  # 32 row tiles, the last one ragged: with N 2048 (1024 gated) the fewest tiles the 256-tile kernels take
MP = 16500     # 65 row tiles, the last one ragged: with them a producer of width 1024 (4 column tiles) has its 256 tiles


def _p8w_glu_fold():
    c = {"gemm_ln_fold": _fold_parts("p8w_glu_fold", MP, 2048, 1024, "swiglu")}
    for K in (256, 1024, 2304):  # 1, 4 and 9 -> 3 statistic slots
        c[f"k{K}"] = _fold_parts("p8w_glu_fold", MR, 1024, K, "swiglu", seed=K)
    c["adversarial_stream"] = lambda dt: _fold_adversarial(dt, "p8w_glu_fold", 8192 - 100, 1024, 1024, "swiglu", seed=11)
    return c


def _p8w_fold():
    c = {
        "none": _fold_parts("p8w_fold", MP, 2048, 1024, "none"),
        "gelu": _fold_parts("p8w_fold", MP, 2048, 1024, "gelu", seed=1),
        "k256_none": _fold_parts("p8w_fold", 65536 - 100, 256, 256, "none", seed=2),
        "k256_gelu": _fold_parts("p8w_fold", 65536 - 100, 256, 256, "gelu", seed=3),
        # M 16500: the producer GEMM [M, 1024, 1024] has the tiles, so these run the chain the modules run
        "col_scale_half": _fold_parts("p8w_fold", MP, 2048, 1024, "gelu", seed=4, col_scale=(1024, 2048, 0.25)),
        "blocked_x_and_out": _fold_parts("p8w_fold", MP, 2048, 1024, "none", seed=5, blocked=True),
        # a residual of mean 8.8 and deviation 2 under a product of deviation 1: 8.8 / sqrt 5 = 3.9 deviations of mean
        "mean_4_deviations": _fold_parts("p8w_fold", MP, 2048, 1024, "gelu", seed=6, mean=8.8, produced=True),
        "adversarial_stream": lambda dt: _fold_adversarial(dt, "p8w_fold", 8192 - 100, 2048, 1024, "none", seed=7),
    }
    # statistic slots: 3, 8 (the LDS region full), 9 -> 3, 11 -> 1, 16 -> 8, 32 -> 8 (the last through ln_fold_weight_kernel<T, 32>)
    for i, K in enumerate((768, 2048, 2304, 2816, 4096, 8192)):
        c[f"k{K}"] = _fold_parts("p8w_fold", MR, 2048, K, ("gelu", "none")[i % 2], seed=K)
    return c


def _stats_parts(M, N, K, seed=0):
    """The producer form: y = x w^T + b + r checked as p8w_stats, and stats_out[slot][row] = (sum, sum of squares) of the
    kernel's own stored y over the slot's 256 columns, against fp64 within the fp32 summation bound gamma_n sum |terms|."""
    def build(dtype):
        x, w, b, r, _, _ = _operands(dtype, M, N, K, res=True, seed=seed)
        p = SimpleNamespace(dtype=dtype, route="p8w_stats", shape=(M, N, K), x=x, w=w, wb=_ops().block_weight(w), b=b, r=r,
                            kw=dict(M=M, N=N, K=K, residual=r, stats_out=True))
        assert _ln_route_of(p) == "p8w_stats"
        return p

    return Parts(build, _ln_launch, _stats_judge)


def _stats_judge(p, ret):
    y, st = ret
    (M, N, K), dtype = p.shape, p.dtype
    gc.check(y, gc.reference(p.x, p.w, p.b, residual=p.r, device=DEV), dtype, "p8w_stats")
    yf = y.double().view(M, N // 256, 256)
    s, q = yf.sum(-1).t(), (yf * yf).sum(-1).t()
    gam = lambda n: n * gc.U32 / (1 - n * gc.U32)  # noqa: E731  (any order, an accumulator that truncates included)
    bs, bq = gam(256) * yf.abs().sum(-1).t(), gam(257) * (yf * yf).sum(-1).t()
    es, eq = (st[:, :M, 0].double() - s).abs(), (st[:, :M, 1].double() - q).abs()
    assert bool((es <= bs).all()), f"row sums off by {(es / bs).max().item():.3g} x the bound"
    assert bool((eq <= bq).all()), f"row sums of squares off by {(eq / bq).max().item():.3g} x the bound"


def _p8w_stats():
    return {
        "n1024_k1024": _stats_parts(16500, 1024, 1024),
        "n256_k128_tiles_257": _stats_parts(65536 + 256, 256, 128, seed=1),
        "n2048_k4096": _stats_parts(8192 + 7, 2048, 4096, seed=2),
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
    _mlp_parts(act, blocked, res, want1, seed)(dtype)


def _mlp_parts(act, blocked, res, want1=None, seed=0):
    return Parts(lambda dt: _mlp_build(dt, act, blocked, res, want1, seed), _mlp_launch, _mlp_judge)


def _mlp_route_of(p):
    return _ops().fused_mlp_route(p.x, p.w1, p.b1, p.w2, p.b2, p.act, p.wg, p.bg, residual=p.r, **p.kw)


def _mlp_launch(p):
    return _ops().fused_mlp(p.x, p.w1, p.b1, p.w2, p.b2, p.act, p.wg, p.bg, residual=p.r, **p.kw)


def _mlp_judge(p, y):
    r = p.r
    ref = gc.reference_mlp(p.x[0], p.w1, p.b1, p.w2, p.b2, p.act, p.wg, p.bg, None if r is None else r[0], device=DEV)
    gc.check(y[0], ref, p.dtype, p.route["stage2"], what=f"fused mlp {p.act} {p.route['path']}")


def _mlp_build(dtype, act, blocked, res, want1=None, seed=0):
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
    p = SimpleNamespace(dtype=dtype, act=act, x=x, w1=w1, b1=b1, w2=w2, b2=b2, wg=wg, bg=bg, r=r, kw=kw)
    p.route = _mlp_route_of(p)
    want = {"path": "blocked" if blocked else "two_launch",
            "stage1": want1 or (("p8w_glu" if act == "swiglu" else "p8w") if blocked else
                                ("glu_t128x64" if act == "swiglu" else "t128")),
            "stage2": ("p8w_res" if res else "p8w") if blocked else "t128"}
    assert p.route == want, p.route
    return p


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


# ---- the two small kernels of the LayerNorm fold, directly ------------------------------------------------------------------
def _floor16(v, dtype):
    """The largest value of the 16-bit grid that is <= v (fp64 in, fp64 out)."""
    r = gc.rn16(v, dtype)
    below = gc.ulp16(r - gc.ulp16(r, dtype) / 4, dtype)  # (the spacing below a power of two is the smaller one)
    return torch.where(r > v, r - below, r)


def _ceil16(v, dtype):
    return -_floor16(-v, dtype)


def _fold_weight_call(w, gamma, beta, bias):
    """mio_ln_fold_weight on w [N, K] with its own row stride (any ldw >= K: the kernel reads single elements)."""
    from mio import _lib
    N, K = w.shape
    ws = torch.full((N, K), float("nan"), dtype=w.dtype, device=DEV)
    bo = torch.full((N,), float("nan"), dtype=w.dtype, device=DEV)
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    rc = _lib.lib.mio_ln_fold_weight(w.data_ptr(), w.stride(0), gamma.data_ptr(), p(beta), p(bias), ws.data_ptr(), bo.data_ptr(),
                                     N, K, _ops()._dtype_id(w), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _lib.lib.mio_last_error()
    return ws, bo


# below one pass of the 256 threads, off the 256 grid, the switch between the two kernels
FOLD_K = [8, 255, 256, 2048, 2049, 4096, 8192]
FOLD_N = 64


def _fold_weight_inputs(dtype, K, spread, g):
    """(gamma, w, beta, bias): gamma = 1 + 0.2 n with ldw = K, or gamma = +-2^j, j in -6 .. 6 (a spread of 4096) with ldw = K + 8
    and NaN in the gap between rows.  Random rows, a zero row (3), a row with one dominant element (5) and, under the spread, a
    row with w gamma = 0.75 in every column (9)."""
    rnd = lambda *sh: torch.randn(*sh, device=DEV, generator=g)  # noqa: E731
    if spread:
        j = torch.randint(-6, 7, (K,), device=DEV, generator=g)
        sign = torch.where(torch.rand(K, device=DEV, generator=g) < 0.5, -1.0, 1.0)
        gamma = (sign * 2.0 ** j).to(dtype)
    else:
        gamma = (1 + 0.2 * rnd(K)).to(dtype)
    buf = torch.full((FOLD_N, K + 8 if spread else K), float("nan"), dtype=dtype, device=DEV)
    w = buf[:, :K]
    w.copy_((rnd(FOLD_N, K) * 0.03 + 0.01).to(dtype))
    w[3] = 0
    w[5, (7 * K) // 11] = 8.0
    if spread:
        w[9] = (0.75 / gamma.double()).to(dtype)
        assert torch.equal(w[9].double() * gamma.double(), torch.full((K,), 0.75, dtype=torch.float64, device=DEV))
    return gamma, w, (0.1 * rnd(K)).to(dtype), (0.1 * rnd(FOLD_N)).to(dtype)


def _check_fold_rows(ws, w, gamma, dtype, spread, tag):
    """The prepared rows ws against the exact centred rows e = w gamma - mean_k(w gamma) in fp64 (test_ln_fold_weight_rows)."""
    K = w.shape[1]
    gK, gK1, u1 = gc._gamma(K), gc._gamma(K + 1), gc.U32
    wg = w.double() * gamma.double()
    e = wg - wg.mean(1, keepdim=True)
    if spread:
        e[9] = 0
    d = gK1 * wg.abs().mean(1, keepdim=True) * (1 + u1) + u1 * e.abs()
    wsd = ws.double()
    out = (wsd < _floor16(e - d, dtype)) | (wsd > _ceil16(e + d, dtype))
    assert not bool(out.any()), f"{tag}: {int(out.sum())} elements are no neighbour of their exact value"
    assert not bool(wsd[3].any()), f"{tag}: the zero row"
    if spread:
        assert not bool(wsd[9].any()), f"{tag}: the constant row is not exactly zero"
    rs, plain = wsd.sum(1).abs(), gc.rn16(e, dtype).sum(1).abs()
    undecided = (gc.rn16(e - d, dtype) != gc.rn16(e + d, dtype)).double() * gc.ulp16(e.abs() + d, dtype)
    worse = rs > plain + gK * wsd.abs().sum(1) + undecided.sum(1)
    assert not bool(worse.any()), f"{tag}: rows {worse.nonzero().flatten().tolist()} sum farther from zero than plain rounding"
    ulp = (wsd.abs().amax(1) * 2.0 ** -(gc._P[dtype] - 1)).clamp_min(1e-300)  # of the row's largest element, the dtype's own
    print(f"{tag}: |row sum| at most {(rs / ulp).max().item():.3f} ulp of the row's largest element "
          f"(plain rounding {(plain / ulp).max().item():.3f})")
    assert bool((rs <= 2 * ulp).all()), f"{tag}: |row sum| {(rs / ulp).max().item():.3f} ulp of the largest element"


def _check_bias_out(bo, w, beta, bias, dtype, tag):
    """bias_out against b + w beta in fp64: the kernel's fp32 value is within tol = gamma_{K+1} (|b| + |w||beta|) of it (exact
    products, K + 1 terms in any order) and is rounded ONCE, to nearest: half a 16-bit ulp, taken at |b + w beta| + tol."""
    N, K = w.shape
    gK1 = gc._gamma(K + 1)
    want = torch.zeros(N, dtype=torch.float64, device=DEV) if bias is None else bias.double()
    tol = gK1 * want.abs()
    if beta is not None:
        want = want + w.double() @ beta.double()
        tol = tol + gK1 * (w.double().abs() @ beta.double().abs())
    err = (bo.double() - want).abs()
    bnd = gc.ulp16(want.abs() + tol, dtype) / 2 + tol
    assert bool((err <= bnd).all()), f"{tag}: bias_out off by {(err / bnd).max().item():.3g} x (half an ulp + the fp32 bound)"


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["bfloat16", "float16"])
@pytest.mark.parametrize("K", FOLD_K)
def test_ln_fold_weight_rows(dtype, K):
    """mio_ln_fold_weight on 64 rows against fp64: w' = gamma o w - mean_k(gamma o w), b' = b + w beta.
    The two weight sets of _fold_weight_inputs (under the spread, row 9's products, partial sums and mean are exact in fp32, so
    its centred row is exactly zero), each with and without beta and bias.
      * every prepared element is one of the two 16-bit neighbours of its exact value e, allowing for the kernel's fp32
        evaluation: the products are exact, their sum of K terms is off by at most gamma_K sum|w gamma|, the division and
        the subtraction round once each, so the kernel's e lies within d = gamma_{K+1} mean|w gamma| (1 + u') + u' |e| of e and
        the stored value in [floor16(e - d), ceil16(e + d)];
      * |row sum| <= 2 ulp of the row's largest element (the dtype's ulp, as test_gemm_ln_fold_stream_with_large_mean has
        it): the limit that judges every K;
      * |row sum| <= that of the plain rounding of the same exact row + what the kernel cannot see: its fp32 evaluation of the sum
        it minimises (gamma_K sum|w'|) and one ulp for each element whose plain rounding is not decided within d.  This slack is
        the worst case over summation orders and grows like K ulp while the plain rounding's sum grows like sqrt(K / 12) ulp:
        the comparison discriminates at K 8 .. 256 (a slack of an ulp or so in bf16) and no longer from K of a few thousand
        on -- at K 8192 in fp16 d is about an ulp of a typical element and nearly every element is undecided -- where it
        holds for any row inside the 2-ulp limit;
      * bias_out is within half a 16-bit ulp + gamma_{K+1} (|b| + |w||beta|) of b + w beta (_check_bias_out);
      * the prepared weight does not depend on beta or bias."""
    g = torch.Generator(device=DEV).manual_seed(K)
    for spread in (False, True):
        gamma, w, beta0, bias0 = _fold_weight_inputs(dtype, K, spread, g)
        first = None
        for beta, bias in ((beta0, bias0), (None, bias0), (beta0, None), (None, None)):
            tag = f"K {K} ldw {w.stride(0)} beta {beta is not None} bias {bias is not None}"
            ws, bo = _fold_weight_call(w, gamma, beta, bias)
            assert bool(torch.isfinite(ws).all() and torch.isfinite(bo).all()), tag
            if first is None:
                first = ws
                _check_fold_rows(ws, w, gamma, dtype, spread, tag)
            else:
                assert torch.equal(ws, first), f"{tag}: the prepared weight depends on beta / bias"
            _check_bias_out(bo, w, beta, bias, dtype, tag)
    _free()


@pytest.mark.gpu
@pytest.mark.parametrize("slots_in,slots_out", [(16, 8), (9, 3), (11, 1), (32, 8)])
def test_ln_stats_reduce(slots_in, slots_out):
    """mio_ln_stats_reduce, ragged M: out[s'] = the sum of slots_in / slots_out consecutive slots, every value of the rows inside M
    within gamma_per sum|terms| of the fp64 sum; the rows past M (NaN here) stay out of them."""
    from mio import _lib
    M = 512 + 37
    mp = (M + 255) // 256 * 256
    per = slots_in // slots_out
    g = torch.Generator(device=DEV).manual_seed(slots_in)
    st = torch.randn(slots_in, mp, 2, device=DEV, generator=g) * 30
    st[..., 1] = st[..., 1] ** 2
    st[:, M:] = float("nan")
    out = torch.full((slots_out, mp, 2), float("nan"), dtype=torch.float32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    assert _lib.lib.mio_ln_stats_reduce(st.data_ptr(), slots_in, out.data_ptr(), slots_out, M, stream) == 0
    terms = st[:, :M].double().view(slots_out, per, M, 2)
    err = (out[:, :M].double() - terms.sum(1)).abs()
    bnd = gc._gamma(per) * terms.abs().sum(1)
    assert bool(torch.isfinite(out[:, :M]).all()) and bool((err <= bnd).all()), (err / bnd.clamp_min(1e-300)).max().item()


@pytest.mark.gpu
def test_stats_cover_every_route():
    """Every (dtype, route) with cases has been judged with its bars (run alone, this test runs the first case of each route
    itself).  The measured maxima are printed (-s shows them) in the layout of _gemm_check.BARS."""
    want = {(dt, r) for dt in DTYPES for r in CASES if r != "empty"}
    assert want == set(gc.BARS)
    for dt, route in sorted(want - set(gc.STATS), key=str):
        try:
            next(iter(CASES[route].values()))(dt)
        finally:
            _free()
    print("\n" + gc.stats_table())
    assert want <= set(gc.STATS), sorted(map(str, want - set(gc.STATS)))
    assert all(v["n"] > 0 and v["mean"] > 0 for v in gc.STATS.values())

"""The FP8 x FP8 GEMM for tall inputs (ops.gemm_f8 / mio_gemm_f8; e4m3fn bytes on both sides, one fp32 scale per row of x and per
output column) against fp64 from the very bytes and scales the kernel reads, with the checker of tests/_gemm_check.py.

reference_f8() is tests/_w8_check.reference_w8's construction with s[m, n] = x_scale[m] * w_scale[n] in fp64 in place of the column
scale.  The bound on the pre-activation value is
    tz = |s| gamma_K (|x8||w8|^T) + 2^-24 (2 |s acc| + |z|)
the products of two 4-bit significands are exact, gamma_K covers K terms summed in any order at one fp32 ulp each, the 2 is the fp32
product x_scale * w_scale in front of the read-out's fma.  The unit of the bound is unchanged: no case measured left it.  The bars
start from the 16-bit tiled kernel's, gc.BARS[(dtype, "t128")]; see BARS below for the one this file had to set itself."""
import pytest
import torch

import _gemm_check as gc
import _w8_check as w8c

pytestmark = pytest.mark.gpu
DEV = "cuda"
FP8 = torch.float8_e4m3fn
DTYPES = [torch.bfloat16, torch.float16]
FILL = -3.0e4
# 1 below and 1 above the 256-row / 256-column tile (SwiGLU: 128 columns) with three K steps; less than one step; one fragment; ragged
EXACT = [(1, 8, 16), (16, 16, 128), (17, 24, 144), (255, 264, 384), (257, 248, 384), (300, 520, 1040)]
RANDOM = [(257, 264, 400), (64, 1032, 1040)]
# (fraction not round-to-nearest, worst row, mean row, worst 16x16 fragment) in u.  The first MI355X run of this file measured the
# fraction at 7 - 8 x the 16-bit kernels' bar on every case with the element bound held: the instruction's internal sum of a step's
# 128 products is coarser than an fp32 sum (about 2^-15 of |z| on these wide-range bytes, independent of K; profiles/gemm_f8.md).  So
# the fraction's bar is this file's own, 2 x the worst measured; the other three are the lower of that and gc.BARS[(dtype, "t128")].
BARS = {torch.bfloat16: (0.0434, 1.20, 0.860, 1.18),  # measured worst: 2.17e-02 0.601 0.430 0.784
        torch.float16: (0.224, 1.20, 0.858, 1.32)}    # measured worst: 1.12e-01 0.598 0.429 0.789
assert all(b <= a for dt in BARS for a, b in zip(w8c.BARS[dt][1:], BARS[dt][1:]))


def _ops():
    from mio import ops
    return ops


def reference_f8(x8, xs, w8, ws, bias=None, act="none", w8g=None, wsg=None, bg=None, res=None) -> gc.Ref:
    f = lambda t: None if t is None else t.to(DEV, torch.float64)  # noqa: E731
    K = x8.shape[1]
    xf, gam = w8c.widen(x8, DEV), gc._gamma(K)

    def pre(q, s, b):
        qf, sf = w8c.widen(q, DEV), f(xs).reshape(-1, 1) * f(s).reshape(1, -1)
        acc, S = xf @ qf.t(), xf.abs() @ qf.abs().t()
        z = sf * acc if b is None else sf * acc + f(b)
        return z, sf.abs() * (gam * S) + gc.EPS32 * (2.0 * (sf * acc).abs() + z.abs())

    z, tz = pre(w8, ws, bias)
    zg, tzg = pre(w8g, wsg, bg) if act == "swiglu" else (None, None)
    y, tol = gc._finish(z, tz, act, zg, tzg, None, f(res))
    return gc.Ref(y, tol, K)


def _judge(y, ref, dtype, what, **kw):
    print(f"{what} {dtype}: " + " ".join(f"{k} {v:.3g}" for k, v in gc.measure(y, ref, dtype).items()))
    gc.check(y, ref, dtype, "gemm_f8", bars=BARS[dtype], what=what, **kw)


def _bytes(rows, K, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, K, generator=g) * 64.0).clamp(-448.0, 448.0).to(FP8).to(DEV)


def _scales(n, unit, phase):
    """fp32 [n]: unit times a factor in [1, 1.37) that differs on every element and is no power of two."""
    i = torch.arange(n, dtype=torch.float64)
    return (unit * (1.0 + 0.37 * torch.frac((i + phase) * 0.6180339887))).to(torch.float32).to(DEV)


def _rand(shape, dtype, scale, seed):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype).to(DEV)


def _operands(M, N, K, dtype, act, extras, seed=0):
    """(args, kwargs) of one ops.gemm_f8 call: z about N(0, 1), bias about 0.5, residual about 1."""
    kw = dict(activation=act, out_dtype=dtype)
    if act == "swiglu":
        kw.update(w8_gate=_bytes(N, K, seed + 4), w_scale_gate=_scales(N, K ** -0.5 / 64.0 * 1.23, 0.25))
    if extras:
        kw.update(bias=_rand((N,), dtype, 0.5, seed + 2), residual=_rand((M, N), dtype, 1.0, seed + 3))
        if act == "swiglu":
            kw["bias_gate"] = _rand((N,), dtype, 0.5, seed + 5)
    return (_bytes(M, K, seed), _scales(M, 1.0 / 64.0, 0.5), _bytes(N, K, seed + 1), _scales(N, K ** -0.5 / 64.0, 0.0)), kw


def _ref(args, kw):
    return reference_f8(*args, kw.get("bias"), kw["activation"], kw.get("w8_gate"), kw.get("w_scale_gate"), kw.get("bias_gate"),
                        kw.get("residual"))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,K", EXACT)
def test_exact(M, N, K, dtype):
    """Small integers under power-of-two scales: |sum| <= 4 K < 2^24, the fp32 accumulator is exact in any order, and the output is
    the fp64 product rounded to the 16-bit grid, bit for bit.  Every byte depends on its k: a K-chunk mix-up between the two
    operands' fragments changes the sums."""
    g = torch.Generator().manual_seed(M * 7 + N)
    x8 = torch.randint(-2, 3, (M, K), generator=g).float().to(FP8).to(DEV)
    w8 = torch.randint(-2, 3, (N, K), generator=g).float().to(FP8).to(DEV)
    xs = torch.exp2((torch.arange(M) % 5 - 2).float()).to(DEV)
    ws = torch.exp2((torch.arange(N) % 3 - 1).float()).to(DEV)
    assert _ops().gemm_f8_route(M, N, K) == "f8_t256x256"
    y = _ops().gemm_f8(x8, xs, w8, ws, out_dtype=dtype)
    want = gc.rn16(reference_f8(x8, xs, w8, ws).y, dtype)
    assert y.dtype == dtype and torch.equal(y.double(), want), f"{int((y.double() != want).sum())} of {M * N} elements differ"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("extras", [True, False], ids=["bias_res", "bare"])
@pytest.mark.parametrize("act", ["none", "gelu", "swiglu"])
@pytest.mark.parametrize("M,N,K", RANDOM)
def test_random(M, N, K, act, extras, dtype):
    args, kw = _operands(M, N, K, dtype, act, extras)
    _judge(_ops().gemm_f8(*args, **kw), _ref(args, kw), dtype, f"{(M, N, K)} {act} extras={extras}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_quantisers_fit(dtype):
    """Operands made by ops.quantize_rows_f8 and ops.quantize_weight_w8, judged on the bytes they produced; gemm_w8a8 is the same
    two calls."""
    ops, (M, N, K) = _ops(), RANDOM[0]
    x, w = _rand((3, M // 3 + 1, K), dtype, 1.0, 1)[:, :-1], _rand((N, K), dtype, K ** -0.5, 2)  # (x: a strided view)
    x8, xs = ops.quantize_rows_f8(x)
    w8, ws = ops.quantize_weight_w8(w)
    assert x8.shape == (x.numel() // K, K) and x8.dtype == FP8 and xs.shape == (x8.shape[0],)
    y = ops.gemm_f8(x8, xs, w8, ws, activation="gelu", out_dtype=dtype)
    _judge(y, reference_f8(x8, xs, w8, ws, act="gelu"), dtype, "quantised operands")
    y2 = ops.gemm_w8a8(x, w8, ws, activation="gelu")
    assert y2.shape == (*x.shape[:-1], N) and torch.equal(y2.reshape(-1, N), y)


@pytest.mark.parametrize("dtype", DTYPES)
def test_hostile_memory(dtype):
    """Every operand as a view into a buffer of NaN bit patterns (0x7f bytes, NaN scales, biases and residual rows and columns),
    the output as a view into a filled buffer: the result is the compact call's bit for bit and nothing outside the view is
    written."""
    ops, (M, N, K) = _ops(), RANDOM[0]
    args, kw = _operands(M, N, K, dtype, "swiglu", True)
    want = ops.gemm_f8(*args, **kw)

    def mat(t, fill):  # t [R, C] as rows 2 .. R + 2, columns 16 .. 16 + C of a filled buffer
        R, C = t.shape
        buf = torch.full((R + 4, (C + 48) // 16 * 16), fill, dtype=torch.uint8 if t.dtype == FP8 else t.dtype, device=DEV)
        v = buf.view(t.dtype)[2:R + 2, 16:16 + C]
        v.copy_(t)
        return v

    def vec(t):
        buf = torch.full((t.numel() + 16,), float("nan"), dtype=t.dtype, device=DEV)
        buf[8:8 + t.numel()] = t
        return buf[8:8 + t.numel()]

    x8, xs, w8, ws = args
    hx, hw, hg = mat(x8, 0x7f), mat(w8, 0x7f), mat(kw["w8_gate"], 0x7f)
    assert ops._w8_ok(hx, "x8") is hx and ops._w8_ok(hw, "w8") is hw and hx.stride(0) > K
    hs = vec(ws)
    assert ops._w8_scale(hs, N, "w_scale").data_ptr() == hs.data_ptr()
    guard = torch.full((M + 2, N + 32), FILL, dtype=dtype, device=DEV)
    out = guard[1:M + 1, 16:16 + N]
    y = ops.gemm_f8(hx, vec(xs), hw, hs, vec(kw["bias"]), "swiglu", hg, vec(kw["w_scale_gate"]), vec(kw["bias_gate"]),
                    mat(kw["residual"], float("nan")), out, dtype)
    assert y.data_ptr() == out.data_ptr() and torch.equal(y, want)
    _judge(y, _ref(args, kw), dtype, "hostile", guard=guard, fill=FILL)


def test_rerun_is_bit_identical():
    args, kw = _operands(300, 520, 1040, torch.bfloat16, "gelu", True)
    a, b = _ops().gemm_f8(*args, **kw), _ops().gemm_f8(*args, **kw)
    torch.randn(1 << 20, device=DEV).sum()
    assert torch.equal(a, b) and torch.equal(a, _ops().gemm_f8(*args, **kw))


@pytest.mark.parametrize("B,S", [(1, 65), (3, 43)])
@pytest.mark.parametrize("kind", ["FusedMLPSwiGLU", "FusedMLPGeluTanh"])
def test_module(kind, B, S, monkeypatch):
    """gemm_fp8=True: norm-less forward = quantise rows, fc1 (with the gate), quantise rows of h, fc2 with the residual; each GEMM
    stage is judged on the bytes it read, recomputed through ops from the module's cached copies, and the module returns the
    second stage's bits.  gemm_fp8=False: the 16-bit ops.fused_mlp call, bit for bit."""
    from mio.kernels import mlp
    ops, dt, d, I = _ops(), torch.bfloat16, 128, 272
    torch.manual_seed(5)
    x = torch.randn(B, S, d, device=DEV, dtype=dt)
    mod = getattr(mlp, kind)(d, I, mlp.FusedMLPConfig(precision="bf16", gemm_fp8=True)).to(DEV, dt)
    act, gate = mod._kernel_activation(), getattr(mod, "fc1_gate", None)
    monkeypatch.setattr(ops, "gemm_f8_ok", lambda *a: True)
    y = mod(x, residual=x)
    c = mod._cast
    (w1, s1), (w2, s2) = c.get_w8(mod.fc1.weight, dt), c.get_w8(mod.fc2.weight, dt)
    g8, gs = (None, None) if gate is None else c.get_w8(gate.weight, dt)
    gb = None if gate is None else gate.bias.detach()
    b1, b2 = mod.fc1.bias.detach(), mod.fc2.bias.detach()
    x8, xs = ops.quantize_rows_f8(x)
    h = ops.gemm_f8(x8, xs, w1, s1, b1, act, g8, gs, gb, out_dtype=dt)
    _judge(h, reference_f8(x8, xs, w1, s1, b1, act, g8, gs, gb), dt, f"{kind} fc1")
    h8, hs = ops.quantize_rows_f8(h)
    y2 = ops.gemm_f8(h8, hs, w2, s2, b2, residual=x, out_dtype=dt)
    _judge(y2, reference_f8(h8, hs, w2, s2, b2, res=x.reshape(-1, d)), dt, f"{kind} fc2")
    assert y.shape == x.shape and torch.equal(y.reshape(-1, d), y2)
    mod.config.gemm_fp8 = False
    gw, gbias = mod._gate(dt)
    want = ops.fused_mlp(x, mod.fc1.weight.detach(), b1, mod.fc2.weight.detach(), b2, act, gw, gbias, residual=x)
    assert torch.equal(mod(x, residual=x), want)

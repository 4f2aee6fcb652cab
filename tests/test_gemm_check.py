"""No-GPU self-test of tests/_gemm_check.py: its reference agrees with the oracle, the correctly rounded fp64 result passes,
and the signatures of typical GEMM-kernel bugs, applied to that result, are rejected."""
import pytest
import torch

import oracle
import _gemm_check as gc

M, N, K = 64, 288, 96  # 3 K-tiles of 32; 288 columns: a neighbouring 128-column tile exists for the fragment swap


def _inputs(dtype, seed=0, act="none", residual=False, bias=True):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g).to(dtype)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(dtype)
    b = (torch.randn(N, generator=g) * 0.5).to(dtype) if bias else None
    kw = dict(bias=b, act=act)
    if act == "swiglu":
        kw["w_gate"] = (torch.randn(N, K, generator=g) * K ** -0.5).to(dtype)
        kw["bias_gate"] = (torch.randn(N, generator=g) * 0.5).to(dtype)
    if residual:
        kw["residual"] = torch.randn(M, N, generator=g).to(dtype)
    return x, w, kw


def _rounded(ref, dtype):
    return gc.rn16(ref.y, dtype).to(dtype)


def _rejected(y, ref, dtype, **kw):
    with pytest.raises(AssertionError):
        gc.check(y, ref, dtype, "t128", what="perturbed", **kw)


@pytest.mark.parametrize("act", ["none", "gelu", "gelu_erf", "relu", "silu", "swiglu"])
def test_reference_matches_oracle(act):
    x, w, kw = _inputs(torch.bfloat16, act=act, residual=act != "swiglu")
    ref = gc.reference(x, w, **kw)
    eye = torch.eye(N, dtype=torch.float64)
    if act == "none":  # the oracle's MLP has an activation: the plain linear layer
        want = torch.nn.functional.linear(x.double(), w.double(), kw["bias"].double()) + kw["residual"].double()
        assert torch.allclose(ref.y, want, rtol=0, atol=1e-12)
        return
    want = oracle.fused_mlp(x, w, kw["bias"], eye, None, act, kw.get("w_gate"), kw.get("bias_gate"),
                            residual=kw.get("residual"))
    assert torch.allclose(ref.y, want, rtol=0, atol=1e-12)


def test_reference_mlp_matches_oracle():
    x, w1, kw = _inputs(torch.float16, act="gelu")
    g = torch.Generator().manual_seed(3)
    w2 = (torch.randn(K, N, generator=g) * N ** -0.5).to(torch.float16)
    b2 = (torch.randn(K, generator=g) * 0.5).to(torch.float16)
    ref = gc.reference_mlp(x, w1, kw["bias"], w2, b2, "gelu")
    want = oracle.fused_mlp(x, w1, kw["bias"], w2, b2, "gelu")  # unrounded intermediate
    assert (ref.y - want).abs().max().item() < 5e-3 * want.abs().max().item()


def test_rn16_and_ulp16_on_the_grid():
    for dt in (torch.bfloat16, torch.float16):
        v = torch.randn(100000, dtype=torch.float64) * 10
        r = gc.rn16(v, dt)
        # on the grid, and nearest: what the 16-bit type holds exactly, no farther than half an ulp
        assert torch.equal(r.to(dt).double(), r)
        assert bool(((r - v).abs() <= gc.ulp16(v, dt) / 2).all())
        # agrees with torch's conversion of values exactly representable in fp32 (one rounding there too)
        v32 = v.float().double()
        assert torch.equal(gc.rn16(v32, dt), v32.float().to(dt).double())
    # fp16 subnormals: fixed spacing 2^-24; bf16 keeps fp32's exponent range
    assert gc.ulp16(torch.tensor([2.0 ** -20, 2.0 ** -14, 0.0], dtype=torch.float64), torch.float16).tolist() == \
        [2.0 ** -24, 2.0 ** -24, 2.0 ** -24]
    assert gc.ulp16(torch.tensor([1.0, 1.5, 2.0 ** -126], dtype=torch.float64), torch.bfloat16).tolist() == \
        [2.0 ** -7, 2.0 ** -7, 2.0 ** -133]
    # a double rounding the direct one does not make: 1 + 2^-8 + 2^-30 is above bf16's tie, fp32 rounds it onto the tie
    v = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -30], dtype=torch.float64)
    assert gc.rn16(v, torch.bfloat16).item() == 1.0 + 2.0 ** -7 and v.float().to(torch.bfloat16).item() == 1.0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("act", ["none", "gelu", "silu", "swiglu"])
def test_rounded_result_passes(dtype, act):
    x, w, kw = _inputs(dtype, act=act, residual=act != "swiglu")
    ref = gc.reference(x, w, **kw)
    st = gc.check(_rounded(ref, dtype), ref, dtype, "t128", what="rounded fp64")
    assert st["not_rn"] == 0.0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_rejects_double_rounding_before_the_residual(dtype):
    x, w, kw = _inputs(dtype, act="gelu", residual=True)
    ref = gc.reference(x, w, **kw)
    a = gc.reference(x, w, bias=kw["bias"], act="gelu")
    y = gc.rn16(gc.rn16(a.y, dtype) + kw["residual"].double(), dtype).to(dtype)
    _rejected(y, ref, dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_rejects_round_toward_zero(dtype):
    x, w, kw = _inputs(dtype, act="none", residual=True)
    ref = gc.reference(x, w, **kw)
    q = gc.ulp16(ref.y, dtype)
    y = (torch.trunc(ref.y / q) * q).to(dtype)
    _rejected(y, ref, dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_rejects_bias_shifted_by_one_column(dtype):
    x, w, kw = _inputs(dtype, act="relu")
    ref = gc.reference(x, w, **kw)
    bad = gc.reference(x, w, bias=torch.roll(kw["bias"], 1), act="relu")
    _rejected(_rounded(bad, dtype), ref, dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_rejects_a_k_tile_left_out(dtype):
    x, w, kw = _inputs(dtype, act="silu", residual=True)
    ref = gc.reference(x, w, **kw)
    x2 = x.clone()
    x2[:, 32:64] = 0
    _rejected(_rounded(gc.reference(x2, w, **kw), dtype), ref, dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_rejects_one_fragment_from_a_neighbouring_tile(dtype):
    x, w, kw = _inputs(dtype, act="none", residual=True)
    ref = gc.reference(x, w, **kw)
    y = _rounded(ref, dtype)
    y[16:32, 16:32] = y[16:32, 144:160]
    _rejected(y, ref, dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_rejects_one_guard_element_overwritten(dtype):
    x, w, kw = _inputs(dtype, act="gelu")
    ref = gc.reference(x, w, **kw)
    fill = -77.0
    buf = torch.full((M + 3, N + 24), fill, dtype=dtype)
    view = buf[1:M + 1, 8:N + 8]
    view.copy_(_rounded(ref, dtype))
    gc.check(view, ref, dtype, "t128", guard=buf, fill=fill, what="guarded")
    buf[M + 1, 8] = 0.0  # the row just past the view
    with pytest.raises(AssertionError, match="guard"):
        gc.check(view, ref, dtype, "t128", guard=buf, fill=fill)
    buf[M + 1, 8] = fill
    buf[5, N + 8] = 1.0  # the column just past the view
    with pytest.raises(AssertionError, match="guard"):
        gc.check(view, ref, dtype, "t128", guard=buf, fill=fill)


def test_rejects_non_finite():
    x, w, kw = _inputs(torch.bfloat16)
    ref = gc.reference(x, w, **kw)
    y = _rounded(ref, torch.bfloat16)
    y[3, 7] = float("nan")
    with pytest.raises(AssertionError, match="non-finite"):
        gc.check(y, ref, torch.bfloat16, "t128")


def test_subnormal_fp16_bound():
    """fp16 outputs in the subnormal range: the bound holds with the fixed spacing 2^-24, and one spacing too many fails."""
    g = torch.Generator().manual_seed(5)
    x = ((torch.rand(M, K, generator=g) + 1) * 2.0 ** -12).to(torch.float16)
    w = ((torch.rand(N, K, generator=g) - 0.5) * 2.0 ** -6).to(torch.float16)
    ref = gc.reference(x, w)
    assert ref.y.abs().max().item() < 2.0 ** -14  # every output subnormal
    y = _rounded(ref, torch.float16)
    gc.check(y, ref, torch.float16, "t128", bars=False, what="subnormal")
    y2 = y.clone()
    y2[0, 0] = (y2[0, 0].double() + 2 * 2.0 ** -24).to(torch.float16)
    with pytest.raises(AssertionError, match="rounding bound"):
        gc.check(y2, ref, torch.float16, "t128", bars=False)

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


# ---- LayerNorm fold: reference_fold() against an fp32 model of the consumer, and the defects it must reject ----------------------
FM, FN, FK = 384, 256, 512  # three 128-row groups, two statistic slots
EPS = 1e-5
# Limits of this self-test (no kernel route): a result within half an ulp of ref has a normwise error of at most 1 u per row and
# per fragment; rounding errors uniform in +-ulp/2 on significands uniform in [1, 2) give a mean row of 2 / sqrt(12) / sqrt(7/3)
# = 0.38 u.  The fp32 model adds its accumulation and rstd noise: a quarter more, and up to 5 % of the elements across a tie.  On
# the stream with a mean of 32 deviations a real rstd error of one u' (2 m^2 + 1) / 2 = 1.2e-4 is a quarter of fp16's u, 4.9e-4:
# up to a quarter of the elements may cross a tie there.
FOLD_LIMITS = {1.0: (0.05, 1.25, 0.5, 1.25), 32.0: (0.25, 1.25, 0.5, 1.25)}


def _fold_inputs(dtype, mean_over_std, glu=False, seed=0):
    """A stream with row scales spread over 0.5 .. 2 (so that a neighbour's rstd is a wrong one), row 7 all zero; fp32 slot
    sums of the stored stream; centred weights rounded to the dtype, folded biases."""
    g = torch.Generator().manual_seed(seed)
    scale = 2.0 ** (torch.rand(FM, 1, generator=g) * 2 - 1)
    y = ((torch.randn(FM, FK, generator=g) + mean_over_std) * scale)
    y[7] = 0
    y = y.to(dtype)
    yd = y.double().view(FM, FK // 256, 256)
    stats = torch.stack([yd.sum(-1).t(), (yd * yd).sum(-1).t()], -1).float().contiguous()  # [slots, M, 2]
    gamma = (1 + 0.2 * torch.randn(FK, generator=g)).to(dtype).double()
    out = {"y": y, "stats": stats}
    for nm in ("", "_gate") if glu else ("",):
        w = (torch.randn(FN, FK, generator=g) * 0.05).to(dtype).double() * gamma
        out["w_plain" + nm] = gc.rn16(w, dtype).to(dtype)                       # gamma o W, uncentred
        out["ws" + nm] = gc.rn16(w - w.mean(1, keepdim=True), dtype).to(dtype)
        out["b" + nm] = (torch.randn(FN, generator=g) * 0.3).to(dtype)
    return out


def _rstd32(stats, K, eps=EPS):
    """The kernel's operation order in fp32: slots added one by one, the rounded 1 / K, mu, sq ik - mu mu, clamp, + eps, rsqrt."""
    sm, sq = torch.zeros_like(stats[0, :, 0]), torch.zeros_like(stats[0, :, 0])
    for s in range(stats.shape[0]):
        sm, sq = sm + stats[s, :, 0], sq + stats[s, :, 1]
    ik = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(K), dtype=torch.float32)
    mu = sm * ik
    return torch.rsqrt(torch.clamp_min(sq * ik - mu * mu, 0.0) + torch.tensor(eps, dtype=torch.float32))


def _emulate(d, dtype, act="none", r=None, ws=None, bias_first=False, up_unscaled=False):
    """fp32 model of the consumer: fp32 accumulation, acc * rstd + b', the activation, one rounding to the dtype."""
    r = (_rstd32(d["stats"], FK) if r is None else r)[:, None]
    y = d["y"].float()
    pre = lambda w, b: (y @ w.float().t() + b.float()) * r if bias_first else (y @ w.float().t()) * r + b.float()  # noqa: E731
    z = pre(d["ws"] if ws is None else ws, d["b"])
    if act == "swiglu":
        if up_unscaled:
            z = y @ d["ws"].float().t() + d["b"].float()
        z = torch.nn.functional.silu(pre(d["ws_gate"], d["b_gate"])) * z
    elif act == "gelu":
        z = torch.nn.functional.gelu(z, approximate="tanh")
    return z.to(dtype)


def _fold_ref(d, act="none"):
    return gc.reference_fold(d["y"], d["stats"], d["ws"], d["b"], eps=EPS, act=act, ws_gate=d.get("ws_gate"),
                             bias_gate=d.get("b_gate"))


def _fold_rejected(z, ref, dtype, mean):
    """Rejected by a judgement of the values (the element bound or a statistical limit), not by a mismatch of shape or dtype."""
    with pytest.raises(AssertionError, match=r"outside the rounding bound|\(bar "):
        gc.check(z, ref, dtype, "fold model", bars=FOLD_LIMITS[mean], what="planted defect")


FOLD_PARAMS = [(dt, m) for dt in (torch.bfloat16, torch.float16) for m in (1.0, 32.0)]
FOLD_IDS = [f"{str(dt).split('.')[-1]}-mean{int(m)}" for dt, m in FOLD_PARAMS]


def test_reference_fold_is_layernorm_then_linear():
    """With exact statistics and an exactly centred weight the fold reference is the oracle's LayerNorm -> linear."""
    d = _fold_inputs(torch.bfloat16, 1.0)
    yd = d["y"].double().view(FM, FK // 256, 256)
    stats = torch.stack([yd.sum(-1).t(), (yd * yd).sum(-1).t()], -1)  # fp64
    w = torch.randn(FN, FK, dtype=torch.float64, generator=torch.Generator().manual_seed(9)) * 0.05
    gamma, beta = torch.rand(FK, dtype=torch.float64) + 0.5, torch.randn(FK, dtype=torch.float64) * 0.1
    wg = w * gamma
    ref = gc.reference_fold(d["y"], stats, wg - wg.mean(1, keepdim=True), d["b"].double() + w @ beta, eps=EPS)
    want = oracle.layernorm(d["y"], gamma, beta, EPS).double() @ w.t() + d["b"].double()
    rows = torch.arange(FM) != 7  # (the zero row: eps as fp32 in the reference, fp64 in the oracle; both give b')
    assert torch.allclose(ref.y[rows], want[rows], rtol=0, atol=1e-9)


def test_rstd_interval_order_of_magnitude():
    """dr / r grows with the square of the stream's mean: about 1e-6 at 1 deviation, 8e-4 at 32 (two slots)."""
    for m, lo, hi in ((1.0, 3e-7, 3e-6), (32.0, 3e-4, 2e-3)):
        d = _fold_inputs(torch.float16, m)
        r, r_lo, r_hi = gc.rstd_interval(d["stats"], FK, EPS)
        rel = (torch.maximum(r_hi - r, r - r_lo) / r)[torch.arange(FM) != 7]
        assert lo < rel.median().item() < hi, (m, rel.median().item())
        assert bool((r_lo <= r).all() and (r <= r_hi).all())


@pytest.mark.parametrize("dtype,mean", FOLD_PARAMS, ids=FOLD_IDS)
@pytest.mark.parametrize("act", ["none", "gelu", "swiglu"])
def test_fold_model_passes(dtype, mean, act):
    d = _fold_inputs(dtype, mean, glu=act == "swiglu")
    ref = _fold_ref(d, act)
    st = gc.check(_emulate(d, dtype, act), ref, dtype, "fold model", bars=FOLD_LIMITS[mean], what="fp32 model")
    assert ("fold model" not in {k[1] for k in gc.STATS}) and st["frag"] > 0
    # the zero row: r = eps^-1/2 on a zero accumulator, the output is act(b') within the epilogue's own terms
    assert ref.tol[7].max().item() <= 64 * gc.EPS32 * max(1.0, ref.y[7].abs().max().item())
    # the rstd of the fp32 model lies inside the interval
    r32 = _rstd32(d["stats"], FK).double()
    _, r_lo, r_hi = gc.rstd_interval(d["stats"], FK, EPS)
    assert bool((r_lo <= r32).all() and (r32 <= r_hi).all())


@pytest.mark.parametrize("dtype,mean", FOLD_PARAMS, ids=FOLD_IDS)
def test_rejects_rstd_of_the_neighbouring_16_rows(dtype, mean):
    d = _fold_inputs(dtype, mean)
    r = _rstd32(d["stats"], FK)
    r[16:32] = r[0:16].clone()
    _fold_rejected(_emulate(d, dtype, r=r), _fold_ref(d), dtype, mean)


@pytest.mark.parametrize("dtype,mean", FOLD_PARAMS, ids=FOLD_IDS)
def test_rejects_a_statistics_slot_left_out_for_one_group(dtype, mean):
    d = _fold_inputs(dtype, mean)
    r = _rstd32(d["stats"], FK)
    r[128:256] = _rstd32(d["stats"][:1], FK)[128:256]  # the group's second slot never arrived
    _fold_rejected(_emulate(d, dtype, "gelu", r=r), _fold_ref(d, "gelu"), dtype, mean)


@pytest.mark.parametrize("dtype,mean", FOLD_PARAMS, ids=FOLD_IDS)
def test_rejects_rstd_applied_after_the_bias(dtype, mean):
    d = _fold_inputs(dtype, mean)
    _fold_rejected(_emulate(d, dtype, bias_first=True), _fold_ref(d), dtype, mean)


@pytest.mark.parametrize("dtype,mean", FOLD_PARAMS, ids=FOLD_IDS)
def test_rejects_swiglu_up_half_unscaled(dtype, mean):
    d = _fold_inputs(dtype, mean, glu=True)
    _fold_rejected(_emulate(d, dtype, "swiglu", up_unscaled=True), _fold_ref(d, "swiglu"), dtype, mean)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_rejects_eps_left_out_on_a_zero_row(dtype):
    d = _fold_inputs(dtype, 1.0)
    z = _emulate(d, dtype, r=_rstd32(d["stats"], FK, eps=0.0))
    assert not bool(torch.isfinite(z[7]).any())
    with pytest.raises(AssertionError, match="non-finite"):
        gc.check(z, _fold_ref(d), dtype, "fold model", bars=FOLD_LIMITS[1.0])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_rejects_uncentred_weight_on_a_stream_with_large_mean(dtype):
    d = _fold_inputs(dtype, 32.0)
    _fold_rejected(_emulate(d, dtype, ws=d["w_plain"]), _fold_ref(d), dtype, 32.0)

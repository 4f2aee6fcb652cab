"""No-GPU self-test of tests/_rows_check.py: an fp32 model of each row kernel's operation sequence (LayerNorm in the kernel's own lane
order) lies inside the admissible interval everywhere, the planted defects a whole-tensor tolerance lets through are each reported,
and the cap conditions hold for the very inputs tests/test_gpu_rows.py uses."""
import math

import pytest
import torch

import _gemm_check as gc
import _rms_check as rc
import _rows_check as rw

DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
EPS = rw.EPS
ROWS = 64  # from 32 rows on the builder plants its zero, constant, single-element and offset rows
MODEL_COLS = [64, 520, 2056, 4096]


def _f32(v):
    return torch.tensor(v, dtype=torch.float32)


# ---- fp32 model of layernorm_kernel<T, CH, false> ----------------------------------------------------------------------------------
def _wsum(v):
    """The kernel's row sum of v [rows, cols] in fp32: chunk c of 8 elements belongs to lane c % 64, a lane adds the elements of its
    chunks one by one (absent chunks are zeros), then the xor butterfly 32, 16, ..., 1.  [rows, 1]."""
    rows, cols = v.shape
    nch = cols // 8
    v = torch.nn.functional.pad(v.reshape(rows, nch, 8), (0, 0, 0, (-nch) % 64)).view(rows, -1, 64, 8)
    acc = torch.zeros(rows, 64)
    for j in range(v.shape[1]):
        for i in range(8):
            acc = acc + v[:, j, :, i]
    o = 32
    while o >= 1:
        acc = acc + acc[:, torch.arange(64) ^ o]
        o >>= 1
    assert bool((acc == acc[:, :1]).all())  # every lane ends with the same sum
    return acc[:, :1]


def _sum32(x, res, alpha):
    """v = x + alpha * res as the kernel forms it in fp32."""
    return x.float() + _f32(alpha) * res.float()


def _ln_model(s, w, b, dtype, defect=None):
    """The kernel's sequence on the fp32 rows s (16-bit values, or the unrounded sum), one rounding to dtype at the end.  defect: one
    of the planted ones."""
    rows, cols = s.shape
    n = _f32(float(cols))
    m = _wsum(s) / n
    if defect == "padded_mean":  # the mean over the chunks the wave holds, not the ones the row has
        m = _wsum(s) / _f32(float(math.ceil(cols / 512) * 512))
    d = s - m
    if defect == "onepass":
        var = _wsum(s * s) / n - m * m
    else:
        var = _wsum(d * d) / (n - 1 if defect == "n-1" else n)
    r = torch.rsqrt(var + _f32(EPS) * (_f32(1.1) if defect == "eps" else 1))
    if defect == "neighbour_mean":  # chunk 1 of every row centred with the row above's mean
        d = d.clone()
        d[:, 8:16] = s[:, 8:16] - torch.roll(m, 1, 0)
    o = d * r * w.float()
    if b is not None:
        bf = b.float().clone()
        if defect == "bias_chunk":
            bf[16:24] = 0
        o = o + bf
    return o.to(dtype)


def _ln_inputs(dtype, cols, rows=ROWS, seed=0):
    x, plain = rw.layernorm_rows(dtype, rows, cols, seed + cols)
    res, _ = rw.layernorm_rows(dtype, rows, cols, seed + cols + 1)
    w, b = rw.layernorm_params(dtype, cols, seed + cols + 2)
    return x, res, w, b, plain


def _rejected(y, ref, dtype):
    with pytest.raises(AssertionError, match="outside the admissible interval"):
        rw.admissible(y, ref, dtype, "planted defect")


# ---- the judgement -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_admissible_is_one_value_where_tol_is_zero(dtype):
    v = torch.randn(64, 96, dtype=torch.float64) * 3
    ref = gc.Ref(v, torch.zeros_like(v), 96)
    y = gc.rn16(v, dtype).to(dtype)
    assert rw.admissible(y, ref, dtype, "rounded") == 0.0
    y2 = y.clone()
    y2[3, 5] = (y2[3, 5].double() + gc.ulp16(v[3, 5], dtype)).to(dtype)  # the next 16-bit value
    with pytest.raises(AssertionError, match=r"1 of 6144 elements outside the admissible interval; worst at \(3, 5\)"):
        rw.admissible(y2, ref, dtype, "one ulp")
    y2 = y.clone()
    y2[0, 0] = float("nan")
    with pytest.raises(AssertionError, match="outside the admissible interval"):
        rw.admissible(y2, ref, dtype, "nan")


def test_admissible_lets_either_neighbour_pass_across_a_boundary():
    # 1 + 2^-8 is bf16's tie between 1 and 1 + 2^-7: with a tolerance both neighbours are admissible, the ones beyond are not
    v = torch.full((1, 4), 1.0 + 2.0 ** -8, dtype=torch.float64)
    ref = gc.Ref(v, torch.full_like(v, 1e-6), 4)
    y = torch.tensor([[1.0, 1.0 + 2.0 ** -7, 1.0, 1.0 + 2.0 ** -7]], dtype=torch.bfloat16)
    assert rw.admissible(y, ref, torch.bfloat16) == 1.0
    for bad in (1.0 - 2.0 ** -8, 1.0 + 2.0 ** -6):
        y2 = y.clone()
        y2[0, 2] = bad
        _rejected(y2, ref, torch.bfloat16)


def test_ulp32():
    v = torch.tensor([1.0, 1.5, -3.0, 2.0 ** -126, 2.0 ** -130, 0.0], dtype=torch.float64)
    assert rw.ulp32(v).tolist() == [2.0 ** -23, 2.0 ** -23, 2.0 ** -22, 2.0 ** -149, 2.0 ** -149, 2.0 ** -149]


# ---- LayerNorm: the model passes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [False, True], ids=["plain", "bias"])
@pytest.mark.parametrize("cols", MODEL_COLS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_layernorm_model_passes(dtype, cols, bias):
    x, _, w, b, plain = _ln_inputs(dtype, cols)
    b = b if bias else None
    ref = rw.reference_layernorm(x, w, b, EPS)
    rw.admissible(_ln_model(x.float(), w, b, dtype), ref, dtype, f"fp32 model cols {cols}")
    # the zero row: the bias alone is admissible (exactly 0 without one); the constant row: the reference is the bias too, with a
    # tolerance for the mean's rounding error times eps^-1/2
    want = torch.zeros(cols, dtype=torch.float64) if b is None else b.double()
    lo, hi = rw.interval(ref, dtype)
    assert torch.equal(lo[rw.ROW_ZERO], want) and torch.equal(hi[rw.ROW_ZERO], want)
    assert torch.equal(ref.y[rw.ROW_CONST], want)
    assert bool(torch.isfinite(ref.tol).all())


@pytest.mark.parametrize("cols", MODEL_COLS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_layernorm_model_passes_on_the_stored_and_on_the_unrounded_sum(dtype, cols):
    x, res, w, b, _ = _ln_inputs(dtype, cols)
    for alpha in (0.5, 0.3):
        v = _sum32(x, res, alpha)
        s16 = v.to(dtype)  # sum_out requested: stored, and the rounded value normalised
        sref, sbound = rc.sum_bound(x, res, alpha, dtype)
        assert bool(((s16.double() - sref).abs() <= sbound).all())
        rw.admissible(_ln_model(s16.float(), w, b, dtype), rw.reference_layernorm(s16, w, b, EPS), dtype, f"stored sum {alpha}")
        s, ds = rw.unrounded_sum(x, res, alpha)  # no sum_out: the fp32 sum normalised
        assert bool(((v.double() - s).abs() <= ds).all())
        rw.admissible(_ln_model(v, w, b, dtype), rw.reference_layernorm(s, w, b, EPS, ds=ds), dtype, f"unrounded sum {alpha}")


@pytest.mark.parametrize("cols", [520, 4096, 8192])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_rmsnorm_model_passes_on_the_unrounded_sum(dtype, cols):
    x, res, w, _, _ = _ln_inputs(dtype, cols)
    v = _sum32(x, res, 0.3)
    r = torch.rsqrt(_wsum(v * v) / _f32(float(cols)) + _f32(1e-6))
    s, ds = rw.unrounded_sum(x, res, 0.3)
    ref = rw.reference_rms(s, w, 1e-6, ds=ds)
    rw.admissible((v * r * w.float()).to(dtype), ref, dtype, "rms, unrounded sum")
    _rejected((v.to(dtype).float() * r * w.float()).to(dtype), ref, dtype)  # the sum rounded though none was asked for
    # with ds = 0 it is _rms_check.reference_rows
    r0, r1 = rw.reference_rms(x, w, 1e-6, ds=torch.zeros(x.shape)), rc.reference_rows(x, w, 1e-6)
    assert torch.equal(r0.y, r1.y) and torch.allclose(r0.tol, r1.tol, rtol=1e-12, atol=0)


# ---- LayerNorm: the planted defects fail -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("defect", ["n-1", "eps"])
@pytest.mark.parametrize("cols", MODEL_COLS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_rejects_variance_over_cols_minus_one_and_a_wrong_eps(dtype, cols, defect):
    """Caught at every width in both dtypes: n - 1 moves every element by 1 / (2 cols) relative, far more than tol, so the elements
    near a rounding boundary leave their interval; eps * 1.1 is caught on the rows of small scale, where eps is the larger part of
    the variance."""
    x, _, w, b, _ = _ln_inputs(dtype, cols)
    _rejected(_ln_model(x.float(), w, b, dtype, defect), rw.reference_layernorm(x, w, b, EPS), dtype)


def _narrow_rows(dtype, cols):
    """Rows whose deviation is far below their mean, for the one-pass variance.  fp16: offset 64, deviation 0.25 (mean / std 256).
    bf16 holds 8 significand bits, so a Gaussian row cannot carry a mean beyond about 32 deviations, and at the builder's 16 the
    one-pass error is of the size of tol; but a row of the two adjacent values 254 and 255 has mean / std >= 509, and at 4096
    columns the sum of squares (65 025 each, 2.7e8 in all) is past 2^24 and rounds at every butterfly step."""
    g = torch.Generator().manual_seed(cols)
    if dtype == torch.float16:
        return (64 + 0.25 * torch.randn(ROWS, cols, generator=g)).to(dtype)
    return (254.0 + (torch.rand(ROWS, cols, generator=g) < torch.rand(ROWS, 1, generator=g) * 0.8 + 0.1)).to(dtype)


@pytest.mark.parametrize("dtype,cols", [(torch.float16, 64), (torch.bfloat16, 4096)], ids=["fp16-64", "bf16-4096"])
def test_rejects_one_pass_variance(dtype, cols):
    x = _narrow_rows(dtype, cols)
    w, b = rw.layernorm_params(dtype, cols, 3)
    ref = rw.reference_layernorm(x, w, b, EPS)
    rw.admissible(_ln_model(x.float(), w, b, dtype), ref, dtype, "two-pass model on narrow rows")
    _rejected(_ln_model(x.float(), w, b, dtype, "onepass"), ref, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_rejects_mean_over_the_padded_chunk_count(dtype):
    x, _, w, b, _ = _ln_inputs(dtype, 520)
    _rejected(_ln_model(x.float(), w, b, dtype, "padded_mean"), rw.reference_layernorm(x, w, b, EPS), dtype)


@pytest.mark.parametrize("defect", ["neighbour_mean", "bias_chunk"])
@pytest.mark.parametrize("cols", [64, 520])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_rejects_one_chunk_with_the_neighbours_mean_or_without_bias(dtype, cols, defect):
    """64 elements (one chunk of every row) of 4096 or 33 280 are wrong; a mean relative error over the tensor does not see them."""
    x, _, w, b, _ = _ln_inputs(dtype, cols)
    _rejected(_ln_model(x.float(), w, b, dtype, defect), rw.reference_layernorm(x, w, b, EPS), dtype)


@pytest.mark.parametrize("cols", [64, 2056])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_rejects_the_sum_rounded_where_it_should_not_be_and_the_reverse(dtype, cols):
    x, res, w, b, _ = _ln_inputs(dtype, cols)
    v = _sum32(x, res, 0.3)
    s, ds = rw.unrounded_sum(x, res, 0.3)
    _rejected(_ln_model(v.to(dtype).float(), w, b, dtype), rw.reference_layernorm(s, w, b, EPS, ds=ds), dtype)
    _rejected(_ln_model(v, w, b, dtype), rw.reference_layernorm(v.to(dtype), w, b, EPS), dtype)


# ---- LayerNorm: the caps, for the inputs of tests/test_gpu_rows.py --------------------------------------------------------------
@pytest.mark.parametrize("cols", rw.LN_COLS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_layernorm_caps_hold_for_the_gpu_cases(dtype, cols):
    caps = {form: rw.LnCaps(cols) for form in ("none", "sum", "nosum")}
    for rows in rw.LN_ROWS:
        x, res, w, b, plain = rw.ln_case(dtype, rows, cols)
        for bias in (b, None):
            caps["none"].add(rw.reference_layernorm(x, w, bias, EPS), dtype, plain)
            caps["sum"].add(rw.reference_layernorm(_sum32(x, res, 0.3).to(dtype), w, bias, EPS), dtype, plain)
            s, ds = rw.unrounded_sum(x, res, 0.3)
            caps["nosum"].add(rw.reference_layernorm(s, w, bias, EPS, ds=ds), dtype, plain)
    for form, c in caps.items():
        print(f"layernorm {IDS[DTYPES.index(dtype)]} cols {cols} {form}: ambiguous {c.check(form)}")


# ---- merge -------------------------------------------------------------------------------------------------------------------------
_LOG2E = 1.4426950408889634


def _merge_model(o_a, lse_a, o_b, lse_b, dtype, defect=None):
    """fp32 model of attn_merge_kernel + attn_merge_lse_kernel: returns (o fp32, o in dtype, lse)."""
    B, Sq, H, D = o_a.shape
    ninf = float("-inf")

    def weights(la, lb):
        mx = torch.maximum(la, lb)
        live = mx != ninf
        mxs = torch.where(live, mx, torch.zeros_like(mx))
        ea, eb = (torch.exp2((l - mxs) * _f32(_LOG2E)) for l in (la, lb))
        inv = 1.0 / (ea + eb)
        zero = torch.zeros_like(mx)
        if defect == "no_renorm":
            inv = torch.ones_like(inv)
        return torch.where(live, ea * inv, zero), torch.where(live, eb * inv, zero), mx, ea + eb, live

    _, _, mx, S, live = weights(lse_a, lse_b)
    lse = torch.where(live, mx + torch.log(S), torch.full_like(mx, ninf))
    rows = lambda t: t.permute(0, 2, 1).unsqueeze(-1)  # noqa: E731
    if defect == "transposed":  # li = (b * Sq + s) * H + hh
        rows = lambda t: t.reshape(B, Sq, H, 1)  # noqa: E731
    wa, wb, _, _, _ = weights(lse if defect == "lse_first" else lse_a, lse_b)
    if defect == "half_empty":
        mixed = (lse_a == ninf) ^ (lse_b == ninf)
        wa, wb = torch.where(mixed, torch.full_like(wa, 0.5), wa), torch.where(mixed, torch.full_like(wb, 0.5), wb)
    o = rows(wa) * o_a + rows(wb) * o_b
    return o, o.to(dtype), lse


@pytest.mark.parametrize("shape", rw.MERGE_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_merge_model_passes_and_cap(dtype, shape):
    st = rw.merge_states(*shape, seed=sum(shape))
    ref, L, tol_lse = rw.reference_merge(*st)
    o32, o16, lse = _merge_model(*st, dtype)
    rw.within32(o32, ref, "merge model")
    amb = rw.admissible(o16, ref, dtype, "merge model")
    assert amb <= rw.CAP_MERGE, amb
    rw.lse_within(lse, L, tol_lse, "merge model")
    # the reference is the plain formula, and c of tol_lse = u' (|L| + c) stays below 4
    la, lb = st[1].double(), st[3].double()
    both = torch.isinf(la) & torch.isinf(lb)
    assert torch.allclose(L[~both], torch.logaddexp(la, lb)[~both], rtol=1e-14, atol=1e-14) and bool((L[both] == float("-inf")).all())
    c = (tol_lse[~both] - gc.U32 * L[~both].abs()) / gc.U32
    assert 1.0 <= c.min().item() and c.max().item() < 4.0
    rows = both.permute(0, 2, 1).reshape(-1)
    assert bool((ref.y[rows] == 0).all()) and bool((ref.tol[rows] == 0).all())


def test_merge_states_hold_every_kind_of_row():
    """The first GPU shape: both sides live at every gap, a side empty, both empty; equal lse exactly."""
    _, la, _, lb = rw.merge_states(*rw.MERGE_SHAPES[0], seed=sum(rw.MERGE_SHAPES[0]))
    ea, eb = torch.isinf(la), torch.isinf(lb)
    assert bool((ea & ~eb).any()) and bool((~ea & eb).any()) and bool((ea & eb).any())
    gap = (la - lb)[~ea & ~eb]
    assert bool((gap == 0).any())
    for want in rw.GAPS:
        assert bool(((gap - want).abs() < 1e-2).any()), want


@pytest.mark.parametrize("defect", ["transposed", "no_renorm", "lse_first", "half_empty"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_rejects_merge_defects(dtype, defect):
    """Each at the first GPU shape (B, Sq, H all > 1, so that the transposed lse index reads another row's lse), in the fp32 result
    and in the 16-bit one."""
    shape = rw.MERGE_SHAPES[0]
    st = rw.merge_states(*shape, seed=sum(shape))
    ref, _, _ = rw.reference_merge(*st)
    o32, o16, _ = _merge_model(*st, dtype, defect)
    _rejected(o16, ref, dtype)
    with pytest.raises(AssertionError, match="outside the bound"):
        rw.within32(o32, ref, defect)


def test_rejects_lse_off_by_an_fp32_ulp_or_two_and_a_finite_empty_lse():
    st = rw.merge_states(*rw.MERGE_SHAPES[0], seed=1)
    _, L, tol = rw.reference_merge(*st)
    lse = L.float()
    rw.lse_within(lse, L, tol)
    i = int(torch.argmax(torch.where(torch.isinf(L), torch.zeros_like(L), L.abs())))
    bad = lse.clone().reshape(-1)
    bad[i] = bad[i] + 3 * rw.ulp32(L.reshape(-1)[i]).float()
    with pytest.raises(AssertionError, match="lse values outside"):
        rw.lse_within(bad.view_as(lse), L, tol)
    bad = lse.clone()
    bad[torch.isinf(L)] = -1e30
    with pytest.raises(AssertionError, match="not -inf"):
        rw.lse_within(bad, L, tol)

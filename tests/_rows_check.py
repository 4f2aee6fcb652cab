"""Checker of the two oldest row kernels of csrc/rowops.hip, shared by tests/test_rows_check.py (host) and tests/test_gpu_rows.py
(a plain helper module, not a conftest): fp64 references of LayerNorm (layernorm_kernel<T, CH, false>) and of the merge of two
attention states (attn_merge_kernel / attn_merge_lse_kernel), each with the per-element bound `tol` on what a correct kernel's fp32
arithmetic may add before its one rounding to the storage dtype, the judgement admissible(), and the builders of the inputs both
test files use.  u' = 2^-23 (_gemm_check.U32, one full fp32 ulp) is charged for every fp32 rounding and for every hardware unit
that is accurate to 1 ulp (v_rsq_f32, v_exp_f32, v_log_f32, v_rcp_f32), as _gemm_check.C_EP charges them.  No fitted constant and no
number taken from a kernel run anywhere in this file.

The judgement (admissible).  A correct kernel rounds an fp32 value v' with |v' - ref.y| <= ref.tol ONCE to the 16-bit type.
Round-to-nearest is monotone, so
        rn16(ref.y - tol) <= y <= rn16(ref.y + tol)
for every element.  Where the interval [ref.y - tol, ref.y + tol] holds no rounding boundary of the 16-bit grid, exactly one 16-bit
value is admissible; elements whose interval holds a boundary ("ambiguous") may take either neighbour.  That is much sharper than
_gemm_check.element_bound, which allows a whole ulp everywhere, and needs no measured share.  It judges nothing where nearly every
interval is ambiguous, so the share of ambiguous elements -- a property of the inputs and the reference, not of the kernel -- is
capped (cap_plain, CAP_OFFSET, CAP_MERGE), on the host for the very inputs the GPU tests use and again in the GPU tests.

LayerNorm (reference_layernorm).  y = T((s - m) r w + b), m = mean(s), r = (mean((s - m)^2) + eps)^-1/2, from the s the kernel
normalises: x, or with a residual the kernel's own stored 16-bit sum_out (its rounding is judged apart, _rms_check.sum_bound), or,
where no sum_out is requested, the unrounded fp32 sum (`ds`, below).  With m, d = s - m, V = mean(d^2), r exact in fp64:
  * the summation contract.  A row kernel sums a row with every term passing through at most
        k = 8 ceil(cols / 512) + 6
    additions: 8 CH sequential adds per lane (CH = ceil(cols / 512) chunks of 8 elements), then the six steps of the wave's
    butterfly; the adds of a ragged last chunk's padded zeros are exact.  The error of such a sum is at most gamma_k sum |t|,
    gamma_k = k u' / (1 - k u').  This is an ACCURACY CONTRACT for a row kernel, not an accident of this one: a kernel that summed
    a row sequentially (k = cols) would rightly fail it, as it should;
  * the mean: the sum and the (correctly rounded) division by cols:            dm = gamma_{k+1} mean|s|;
  * d' = fl(s - m'):                                                           dd = dm + u' (|d| + dm);
  * the centred second moment, from d' and with the product's rounding (or none where it is fused into the add), the sum and the
    division:                                     dv = mean(2 |d| dd + dd^2) + gamma_{k+2} (V + mean(2 |d| dd + dd^2));
  * the eps add and v_rsq_f32: the interval of _rms_check._interval(V, dv, eps) -- an interval, not a linearisation, so that constant
    rows (V = 0 and d' the mean's own rounding error, magnified by eps^-1/2) and zero rows work:  r_hi, dr;
  * the products d' r and (d' r) w, u' each:
        tol = |w| (dd r_hi + |d| dr + (|d| + dd) r_hi ((1 + u')^2 - 1));
  * with a bias, the add (or the fma that takes the second product's rounding with it):          tol += u' (|y| + tol).
  A zero row has d = dd = 0: the reference is the bias with tol = u' |b|, an interval that holds the bias alone; the tests also
  assert those bits.  eps is the fp32 value the kernel is handed.  This toolchain compiles x / (float)cols to the correctly rounded
  division sequence (v_div_scale / v_div_fmas / v_div_fixup) and rsqrtf to v_rsq_f32 behind an exact power-of-two scaling of
  arguments below 2^-126, which the interval covers as it stands.
  * ds: a per-element bound on what the kernel's s may differ from the one given -- the path res != NULL, sum_out == NULL, which
    normalises the unrounded fp32 sum v = fl(x + alpha res) (one fma, or a product and an add):  ds = u' (|alpha res| + |s|) around
    the fp64 s = x + f32(alpha) res.  It moves the mean by at most mean(ds) and each d' by ds + mean(ds):
        dm = gamma_{k+1} (mean|s| + mean(ds)) + mean(ds),      dd = dm + ds + u' (|d| + dm + ds).
    (reference_rms with ds is _rms_check.reference_rows widened the same way: the second moment Q moves by mean(2 |s| ds + ds^2),
    tol = |w| (ds r_hi + |s| dr + (|s| + ds) r_hi ((1 + u')^2 - 1)).)

Merge (reference_merge).  From the fp32 states o_a, o_b [B, Sq, H, D] and lse_a, lse_b [B, H, Sq] as the kernel reads them, in fp64:
        L = logaddexp(l_a, l_b),   w_x = exp(l_x - L),   o = w_a o_a + w_b o_b;
a row empty on both sides (both lse -inf) has o = 0 and L = -inf, exactly.  The kernel's sequence, mx = max(l_a, l_b), D_x = |l_x - mx|:
  * t = fl(l_x - mx); __expf is, on this toolchain, the product t * float(log2 e) and v_exp_f32 on it, with no scaling of results
    below the smallest normal.  Each of the two roundings is charged u' (twice what round-to-nearest costs), which covers the
    representation error of float(log2 e), 2^-26.2, as well: the exponent is off by at most 2 u' D_x, and with v_exp_f32's ulp
        e_x' = e_x (1 + eps_x),     eps_x = expm1(2 u' D_x) (1 + u') + u'       (about u' (1 + 2 D_x));
    a side with l_x = -inf has e_x' = 0 = e_x exactly (eps_x := 0);
  * S' = fl(e_a' + e_b'), S in [1, 2]:       eps_S = q + u' (1 + q),  q = w_a eps_a + w_b eps_b;
  * inv = 1.0f / S', compiled to the correctly rounded division sequence here (charged u', as v_rcp_f32 would be):
        eps_i = (1 + eps_S / (1 - eps_S)) (1 + u') - 1;
  * the weight w_x' = fl(e_x' inv):          E_x = (1 + eps_x) (1 + eps_i) (1 + u') - 1      (about eps_x + eps_S + 3 u');
  * o' = fl(fl(w_a' a) + fl(w_b' b)) (or with the add fused into one product), p_x = |w_x o_x|, t_x = p_x ((1 + E_x) (1 + u') - 1):
        tol_o = t_a + t_b + u' (p_a + t_a + p_b + t_b) + 2^-126 (|a| + |b|),
    to first order  p_a (eps_a + eps_S + 5 u') + p_b (eps_b + eps_S + 5 u') + 2^-126 (|a| + |b|).  The last term is for a weight
    below the smallest normal, 2^-126, which v_exp_f32 may flush to zero or return with a subnormal's precision (gaps beyond 87);
    what that does to S' is below 2^-126 relative and lies in the slack of the doubled charges;
  * the fp32 result o_a is judged by |o_a - o| <= tol_o + ulp32(o) / 2, the 16-bit o_out by admissible();
  * lse: S' as above, so ln S' is off by eps_S / (1 - eps_S); __logf is, on this toolchain, v_log_f32 (1 ulp of log2 S in [0, 1])
    and the product with ln 2 evaluated in two-float arithmetic and rounded once -- charged u' each, as the plain one-instruction
    product the issue names would be; then the add of mx, one rounding of a value of about |L|:
        tol_lse = (eps_S / (1 - eps_S) + 2 u' ln S) (1 + u') + u' |L| = u' (|L| + c),
    c = (eps_S + 2 u' ln S) / u' counted per element; over all gaps q <= 1.55 u', so c <= 1.55 + 1 + 2 ln 2 < 4.  Where L is -inf
    the kernel's lse is -inf exactly.
"""
from __future__ import annotations

import math

import torch

import _rms_check as rc
from _gemm_check import U32, Ref, _gamma, rn16, ulp16

TINY32 = 2.0 ** -126
EPS = 1e-5

# ---- the cases of tests/test_gpu_rows.py (the host self-test asserts the caps for these very inputs) -----------------------------
LN_COLS = [8, 64, 512, 520, 1024, 1032, 2048, 2056, 4096]  # CH = 1 / 2 / 4 / 8, each threshold from both sides
LN_ROWS = [1, 3, 4, 5, 257]                                # a partly filled last workgroup, row >= rows exits
MERGE_SHAPES = [(2, 37, 3, 20), (1, 300, 2, 64), (3, 1, 5, 128), (2, 5, 4, 4)]  # (B, Sq, H, D)
# the largest share of ambiguous elements (module docstring) a case family may have
CAP_MERGE = 0.01
CAP_OFFSET = 0.40


def cap_plain(cols: int) -> float:
    """LayerNorm rows without an offset."""
    return 0.10 if cols <= 2056 else 0.20


def sum_depth(cols: int) -> int:
    """k of the summation contract (module docstring)."""
    return 8 * math.ceil(cols / 512) + 6


def ulp32(v: torch.Tensor) -> torch.Tensor:
    """Spacing of the fp32 grid at the fp64 values v (2^-149 below the smallest normal), as _gemm_check.ulp16."""
    a = v.abs()
    _, e = torch.frexp(a)
    e = torch.where(a > 0, e - 1, torch.full_like(e, -126)).clamp_min(-126)
    return torch.bitwise_left_shift((e - 23 + 1023).to(torch.int64), 52).view(torch.float64)


def _dev(device):
    return torch.device("cpu") if device is None else torch.device(device)


# ---- the judgement ---------------------------------------------------------------------------------------------------------------
def interval(ref: Ref, dtype):
    """(lo, hi): the 16-bit values between which a correct kernel's output lies (module docstring)."""
    return rn16(ref.y - ref.tol, dtype), rn16(ref.y + ref.tol, dtype)


def ambiguous(ref: Ref, dtype) -> torch.Tensor:
    """The elements whose admissible interval holds more than one 16-bit value."""
    lo, hi = interval(ref, dtype)
    return lo != hi


def share(mask: torch.Tensor) -> float:
    return mask.double().mean().item() if mask.numel() else 0.0


def admissible(y: torch.Tensor, ref: Ref, dtype, what: str = "") -> float:
    """Assert rn16(ref.y - tol) <= y <= rn16(ref.y + tol) for every element of the 16-bit y; returns the share of ambiguous
    elements."""
    tag = f"{what} [{str(dtype).split('.')[-1]}]"
    assert y.dtype == dtype, f"{tag}: dtype {y.dtype}"
    assert y.numel() == ref.y.numel(), f"{tag}: {y.numel()} elements, the reference has {ref.y.numel()}"
    yf = y.to(ref.y.device, torch.float64).reshape(ref.y.shape)
    lo, hi = interval(ref, dtype)
    bad = ~((yf >= lo) & (yf <= hi))  # (a NaN is outside)
    if bool(bad.any()):
        q = ulp16(ref.y, dtype)
        dist = torch.where(bad, torch.maximum(lo - yf, yf - hi) / q, torch.zeros_like(yf))
        dist = torch.where(torch.isfinite(dist), dist, torch.full_like(dist, float("inf")))
        i = int(torch.argmax(dist.reshape(-1)))
        m, n = divmod(i, ref.y.shape[1])
        raise AssertionError(f"{tag}: {int(bad.sum())} of {bad.numel()} elements outside the admissible interval; worst at "
                             f"({m}, {n}): y {yf[m, n].item():.9g} ref {ref.y[m, n].item():.9g} tol {ref.tol[m, n].item():.3g} "
                             f"interval [{lo[m, n].item():.9g}, {hi[m, n].item():.9g}]")
    return share(lo != hi)


def within32(o: torch.Tensor, ref: Ref, what: str = "") -> None:
    """The fp32 result of the merge: |o - ref| <= tol + ulp32(ref) / 2."""
    of = o.to(ref.y.device, torch.float64).reshape(ref.y.shape)
    err = (of - ref.y).abs()
    bnd = ref.tol + ulp32(ref.y) / 2
    bad = ~(err <= bnd)
    if bool(bad.any()):
        i = int(torch.argmax(torch.where(bad, err - bnd, torch.zeros_like(err)).nan_to_num(nan=float("inf")).reshape(-1)))
        m, n = divmod(i, ref.y.shape[1])
        raise AssertionError(f"{what} [fp32]: {int(bad.sum())} of {bad.numel()} elements outside the bound; worst at ({m}, {n}): "
                             f"o {of[m, n].item():.9g} ref {ref.y[m, n].item():.9g} |err| {err[m, n].item():.3g} "
                             f"bound {bnd[m, n].item():.3g}")


def lse_within(lse: torch.Tensor, L: torch.Tensor, tol: torch.Tensor, what: str = "") -> None:
    """The merged lse: within tol of L, and exactly -inf where L is."""
    lf = lse.to(L.device, torch.float64).reshape(L.shape)
    empty = L == float("-inf")
    assert bool((lf[empty] == float("-inf")).all()), f"{what}: lse of a row empty on both sides is not -inf"
    err = (lf - L)[~empty].abs()
    bad = ~(err <= tol[~empty])
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} lse values outside u' (|L| + c); worst "
                                 f"{(err / tol[~empty]).nan_to_num(nan=float('inf')).max().item():.3g} x its bound")


# ---- LayerNorm -------------------------------------------------------------------------------------------------------------------
def reference_layernorm(s, w, b, eps: float, *, ds=None, device=None) -> Ref:
    """fp64 LayerNorm of the rows s [rows, cols] (what the kernel normalises) with the 16-bit weight w and bias b (or None), and
    its element bound; ds: a bound on |the kernel's s - s|, [rows, cols] (module docstring)."""
    dev = _dev(device)
    cols = s.shape[-1]
    sf = s.to(dev, torch.float64).reshape(-1, cols)
    wf = w.to(dev, torch.float64)
    k = sum_depth(cols)
    if ds is None:
        dsf = torch.zeros((), dtype=torch.float64, device=dev)
        mds = dsf
    else:
        dsf = ds.to(dev, torch.float64).reshape(-1, cols)
        mds = dsf.mean(-1, keepdim=True)
    m = sf.mean(-1, keepdim=True)
    dm = _gamma(k + 1) * (sf.abs().mean(-1, keepdim=True) + mds) + mds
    d = sf - m
    ad = d.abs()
    dd = dm + dsf + U32 * (ad + dm + dsf)
    V = (d * d).mean(-1, keepdim=True)
    pert = (2.0 * ad * dd + dd * dd).mean(-1, keepdim=True)
    dv = pert + _gamma(k + 2) * (V + pert)
    r, r_hi, dr = rc._interval(V, dv, eps)
    y = d * r * wf
    tol = wf.abs() * (dd * r_hi + ad * dr + (ad + dd) * r_hi * ((1.0 + U32) ** 2 - 1.0))
    if b is not None:
        y = y + b.to(dev, torch.float64)
        tol = tol + U32 * (y.abs() + tol)
    return Ref(y, tol, cols)


def reference_rms(s, w, eps: float, *, ds, device=None) -> Ref:
    """_rms_check.reference_rows for rows the kernel holds to within ds of s (the unrounded-sum path; module docstring)."""
    dev = _dev(device)
    cols = s.shape[-1]
    sf, wf = s.to(dev, torch.float64).reshape(-1, cols), w.to(dev, torch.float64)
    dsf = ds.to(dev, torch.float64).reshape(-1, cols)
    a = sf.abs()
    Q = (sf * sf).mean(-1, keepdim=True)
    pert = (2.0 * a * dsf + dsf * dsf).mean(-1, keepdim=True)
    r, r_hi, dr = rc._interval(Q, pert + _gamma(cols + 1) * (Q + pert), eps)
    return Ref(sf * wf * r, wf.abs() * (dsf * r_hi + a * dr + (a + dsf) * r_hi * ((1.0 + U32) ** 2 - 1.0)), cols)


def unrounded_sum(x, res, alpha: float, device=None):
    """(fp64 s = x + f32(alpha) res, ds = u' (|alpha res| + |s|)): what the kernel normalises where it stores no sum."""
    dev = _dev(device)
    ar = res.to(dev, torch.float64) * rc._f32(alpha)
    s = x.to(dev, torch.float64) + ar
    return s, U32 * (ar.abs() + s.abs())


# planted rows, from 32 rows on
ROW_ZERO, ROW_CONST, ROW_SINGLE = 5, 17, 29
ROWS_OFFSET4 = (41, 42, 43, 44)
ROWS_OFFSET16 = (53, 54, 55, 56)  # at cols <= 512


def layernorm_rows(dtype, rows: int, cols: int, seed: int, device=None, offsets: bool = True):
    """[rows, cols] in dtype: row scales log-uniform over 1e-3 .. 1e2 (with eps 1e-5 the eps term matters on the small rows).  From
    32 rows on: row 5 zero, row 17 constant, row 29 with one non-zero element, rows 41 .. 44 with an offset of 4 deviations and, at
    cols <= 512, rows 53 .. 56 with one of 16 (offsets=False: those rows stay as drawn -- the residual, so that a sum's mean is at
    most the 4 or 16 deviations of its x).  Drawn on the host whatever `device` is, so that the host self-test sees the values
    the GPU tests use.  Returns (x, plain) with plain the [rows] mask (on the host) of the rows without an offset."""
    g = torch.Generator().manual_seed(seed)
    scale = 10.0 ** (torch.rand(rows, 1, generator=g) * 5 - 3)
    z = torch.randn(rows, cols, generator=g)
    plain = torch.ones(rows, dtype=torch.bool)
    if rows >= 32:
        z[ROW_ZERO] = 0
        z[ROW_CONST] = 1
        z[ROW_SINGLE] = 0
        z[ROW_SINGLE, (29 * 37) % cols] = 1
        for rr, off in ((ROWS_OFFSET4, 4.0), (ROWS_OFFSET16 if cols <= 512 else (), 16.0)):
            for i in rr:
                z[i] += off if offsets else 0.0
                plain[i] = False
    return (z * scale).to(dtype).to(_dev(device)), plain


def layernorm_params(dtype, cols: int, seed: int, device=None):
    """(weight about 1, bias about 0.1), [cols] in dtype."""
    g = torch.Generator().manual_seed(seed)
    w = (1 + 0.2 * torch.randn(cols, generator=g)).to(dtype)
    b = (0.1 * torch.randn(cols, generator=g)).to(dtype)
    return w.to(_dev(device)), b.to(_dev(device))


def ln_case(dtype, rows: int, cols: int, device=None):
    """(x, res, w, b, plain) of the GPU tests' LayerNorm case (rows, cols)."""
    seed = 16 * cols + rows
    x, plain = layernorm_rows(dtype, rows, cols, seed, device)
    res, _ = layernorm_rows(dtype, rows, cols, seed + 1000003, device, offsets=False)
    w, b = layernorm_params(dtype, cols, seed + 2000003, device)
    return x, res, w, b, plain


class LnCaps:
    """The cap conditions of one LayerNorm case family (one dtype, width and residual form, over its row counts, with and without
    bias): the ambiguous elements of the rows without an offset and of the offset rows, counted from the references alone."""

    def __init__(self, cols: int):
        self.cols = cols
        self.amb = [0, 0]
        self.n = [0, 0]

    def add(self, ref: Ref, dtype, plain: torch.Tensor) -> None:
        amb = ambiguous(ref, dtype).sum(-1).cpu()
        for i, rows in enumerate((plain, ~plain)):
            self.amb[i] += int(amb[rows].sum())
            self.n[i] += int(rows.sum()) * ref.y.shape[1]

    def shares(self):
        return tuple(a / n if n else 0.0 for a, n in zip(self.amb, self.n))

    def check(self, what: str = ""):
        plain, offset = self.shares()
        assert plain <= cap_plain(self.cols), f"{what}: {plain:.3f} of the elements without an offset are ambiguous"
        assert offset <= CAP_OFFSET, f"{what}: {offset:.3f} of the offset rows' elements are ambiguous"
        return plain, offset


# ---- merge -----------------------------------------------------------------------------------------------------------------------
GAPS = (0.0, 1e-3, -1e-3, 5.0, -5.0, 30.0, -30.0, 90.0, -90.0, 200.0, -200.0)


def merge_states(B: int, Sq: int, H: int, D: int, seed: int, device=None):
    """(o_a, lse_a, o_b, lse_b), fp32: o [B, Sq, H, D] random with a scale of its own per (b, s, h); lse [B, H, Sq] independent per
    (b, h, s), lse_a - lse_b drawn from GAPS plus noise of 1e-4 (none on the gap 0: equal lse).  About 5 % of the rows are empty on
    side a, 5 % on side b and 2 % on both: lse -inf and o 0, the empty-state convention.  Drawn on the host (layernorm_rows)."""
    g = torch.Generator().manual_seed(seed)
    o = [torch.randn(B, Sq, H, D, generator=g) * 10.0 ** (torch.rand(B, Sq, H, 1, generator=g) * 2 - 1) for _ in range(2)]
    la = torch.randn(B, H, Sq, generator=g) * 3
    gap = torch.tensor(GAPS)[torch.randint(len(GAPS), (B, H, Sq), generator=g)]
    gap = gap + 1e-4 * torch.randn(B, H, Sq, generator=g) * (gap != 0)
    lb = la - gap
    u = torch.rand(B, H, Sq, generator=g)
    for t, l, empty in ((o[0], la, (u < 0.05) | ((u >= 0.10) & (u < 0.12))), (o[1], lb, (u >= 0.05) & (u < 0.12))):
        l[empty] = float("-inf")
        t[empty.permute(0, 2, 1)] = 0
    dev = _dev(device)
    return o[0].to(dev), la.to(dev), o[1].to(dev), lb.to(dev)


def reference_merge(o_a, lse_a, o_b, lse_b, device=None):
    """(Ref of o [B Sq H, D], fp64 L [B, H, Sq], tol_lse [B, H, Sq]) of one merge from its fp32 inputs (module docstring)."""
    dev = _dev(device)
    a, b = o_a.to(dev, torch.float64), o_b.to(dev, torch.float64)
    la, lb = lse_a.to(dev, torch.float64), lse_b.to(dev, torch.float64)
    D = a.shape[-1]
    ninf = float("-inf")
    mx = torch.maximum(la, lb)
    both = mx == ninf
    mxs = torch.where(both, torch.zeros_like(mx), mx)
    ea, eb = torch.exp(la - mxs), torch.exp(lb - mxs)           # (exp(-inf) = 0: an empty side)
    S = torch.where(both, torch.ones_like(mx), ea + eb)          # in [1, 2]
    wa, wb = torch.where(both, torch.zeros_like(S), ea / S), torch.where(both, torch.zeros_like(S), eb / S)
    L = torch.where(both, torch.full_like(mx, ninf), mxs + torch.log(S))

    def eps_x(l):
        gapx = torch.where(l == ninf, torch.zeros_like(l), (l - mxs).abs())
        e = torch.expm1(2.0 * U32 * gapx) * (1.0 + U32) + U32
        return torch.where(l == ninf, torch.zeros_like(e), e)

    epa, epb = eps_x(la), eps_x(lb)
    q = wa * epa + wb * epb
    eps_s = q + U32 * (1.0 + q)
    ln_err = eps_s / (1.0 - eps_s)
    eps_i = (1.0 + ln_err) * (1.0 + U32) - 1.0
    rows = lambda t: t.permute(0, 2, 1).reshape(-1, 1)  # noqa: E731  [B, H, Sq] -> the rows of o, [B Sq H, 1]
    a2, b2 = a.reshape(-1, D), b.reshape(-1, D)
    tol = torch.zeros_like(a2)
    y = torch.zeros_like(a2)
    psum = torch.zeros_like(a2)
    for o2, w, ep in ((a2, wa, epa), (b2, wb, epb)):
        E = (1.0 + ep) * (1.0 + eps_i) * (1.0 + U32) - 1.0
        p = rows(w) * o2
        t = p.abs() * rows((1.0 + E) * (1.0 + U32) - 1.0)
        y = y + p
        tol = tol + t
        psum = psum + p.abs() + t
    tol = tol + U32 * psum + TINY32 * (a2.abs() + b2.abs())
    live = rows(~both)
    y, tol = torch.where(live, y, torch.zeros_like(y)), torch.where(live, tol, torch.zeros_like(tol))
    tol_lse = (ln_err + 2.0 * U32 * torch.log(S)) * (1.0 + U32) + U32 * torch.where(both, torch.zeros_like(L), L).abs()
    return Ref(y, tol, D), L, torch.where(both, torch.zeros_like(tol_lse), tol_lse)

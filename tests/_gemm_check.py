"""GEMM checker shared by the GPU GEMM tests (a plain helper module, not a conftest).

reference(): the fp64 result of one gemm_bias_act-style call from the same 16-bit inputs the kernel reads:
    y = s * act(x w^T + b) + r         (act != swiglu; s the column scale, r the residual, added after the activation)
    y = silu(x w_g^T + b_g) * (x w^T + b)
with the activations of oracle/mlp.py.  On the CPU, or on the GPU in float64 for large shapes.  Next to the value it carries a
per-element bound `tol` on everything a correct kernel may add to the error before its one rounding to the storage dtype.

check() asserts:
  1. every output is finite, and elements of a guarded output buffer outside the view keep their fill;
  2. the element bound, from first principles (no fitting):  |y - ref| <= max(ulp(ref), ulp(|ref| + tol) / 2) + tol,  with
       tol = L * gamma_K * (|x||w|^T + |b|) + 2^-24 * ((c + 3 |e|) |a| + 4 |z| + 2 |r|)          (times |s| where scaled)
     * ulp is the spacing of the 16-bit grid at ref, computed from fp64 directly (bf16 2^(e-7), fp16 2^(e-10), fp16
       subnormals a fixed 2^-24); the first term is the final rounding of a value within tol of ref: at most half an ulp of
       |ref| + tol, which is at most ulp(ref) unless tol moves it across a binade.
     * gamma_K = (K+1) u' / (1 - (K+1) u'), u' = 2^-23: the classic bound |fl(sum) - sum| <= gamma_{n-1} sum |terms| for n
       terms summed in ANY order (tree, blocked, MFMA-internal), with u' one full fp32 ulp so that an accumulator that
       truncates instead of rounding is covered too.  The K products of 16-bit values are exact in fp32 (8x8 or 11x11 bit
       significands), and the bias add is the (K+1)-th term.  |x||w|^T is evaluated in fp64.
     * L bounds |act'|: 1 (none, relu), 1.1 (silu: max 1.0998), 1.13 (gelu tanh / erf: max 1.129).  SwiGLU by the product rule:
       gamma (1.1 S_g |z_u| + |silu(z_g)| S_u) + 1.1 gamma^2 S_g S_u.
     * the epilogue's own fp32 math (fast_exp2 / fast_rcp: v_exp_f32, v_rcp_f32, 1 ulp each, and about c = 8 roundings in
       all) costs c fp32 ulps of the activation value a; the exp2 argument e (silu: z log2 e; gelu: z (c0 + c1 z^2)) is
       formed with about 3 roundings, an absolute error of 3 |e| 2^-24 that exp2 turns into a relative one of ln 2 times
       that, which the sigmoid factor does not enlarge; erf's cancellation in 1 + erf(z / sqrt 2) for negative z is an
       absolute error of about 2 ulp of 1 times |z| / 2; the residual add rounds once in fp32 (2^-24 (|a| + |r|)).
     The bound is tight for bf16 at any K and for fp16 at small K (gamma_K S is far below an ulp); for fp16 with K in the
     thousands gamma_K S reaches tens of ulps and the bound is loose by design -- a worst-case summation bound, which real
     accumulation (errors of random sign) stays far inside.  The statistical bars below are what judge those cases tightly.
  3. statistical bars per (dtype, route), set like _attn_check.BARS from one run of tests/test_gpu_gemm_matrix.py on the
     MI355X at no more than 2x the worst value measured (written next to each bar):
       * the fraction of elements that are not the round-to-nearest(-even) of ref on the 16-bit grid;
       * per-row normwise error ||y - ref|| / ||ref|| in units of u (bf16 2^-8, fp16 2^-11): worst row and mean;
       * the worst normwise error of one 16x16 output fragment, in u: one mis-mapped fragment or tile fails it.
STATS collects the measured values of every check() call of a process (max per (dtype, route)).

LayerNorm fold (reference_fold(), the routes p8w_fold and p8w_glu_fold).  The consumer reads the raw stream y [M, K], per row
s <= 8 fp32 slots of (sum, sum of squares), the 16-bit centred weight ws of mio_ln_fold_weight and the folded bias b', and stores
    z = act(r (y ws^T) + b'),   mu = sum_s sum_s / K,   v = max(sum_s sq_s / K - mu^2, 0),   r = (v + eps)^-1/2
(SwiGLU: silu(r (y wg'^T) + bg') * (r (y wu'^T) + bu'), one r for both halves).  The reference evaluates this in fp64 from those very
tensors -- the statistics as the launch gets them (behind mio_ln_stats_reduce where ops.gemm_ln applies it), eps as the fp32
value the kernel is handed -- so neither the weights' re-rounding nor the producer's summation is part of the error judged: what
is left is the consumer's own fp32 arithmetic.  The bound on the pre-activation value, tz, replaces L gamma_K (|x||w|^T + |b|)
above; everything behind it (activation, epilogue terms, column scale, SwiGLU product rule) is the same code, _finish():
    tz = r_hi gamma_K |y||ws|^T  +  |y ws^T| dr  +  2^-24 (|r y ws^T| + |z|)
  * accumulator: gamma_K |y||ws|^T as above (K exact products, no bias among them), times the upper end r_hi of the rstd interval;
  * rstd: the kernel's operation sequence is s - 1 adds per sum, the rounded 1/K, the products sum * ik and sq * ik, mu * mu, the
    subtraction, the clamp (exact), the eps add and v_rsq_f32.  Each rounding is charged one full fp32 ulp u' = 2^-23.  With
    A = sum_s |sum_s| / K >= |mu| and Q = sum_s |sq_s| / K, g = gamma_{s+1} (s - 1 adds, 1/K, the product):
        |fl(mu) - mu| <= g A,   |fl(sq ik) - Q| <= g Q,   |fl(fl(mu)^2) - mu^2| <= ((1 + g)^2 (1 + u') - 1) A^2 =: (m2 - 1) A^2,
        the subtraction adds u' ((1 + g) Q + m2 A^2),   so   dv = g Q + (m2 - 1) A^2 + u' ((1 + g) Q + m2 A^2),
    about (2 s + 4) u' (Q + A^2): an error relative to the SECOND MOMENT, not to the variance.  The kernel's v lies in
    [max(v - dv, 0), v + dv]; the eps add and v_rsq_f32 (1 ulp) widen the interval by u' each:
        r_lo = ((v + dv + eps) (1 + u'))^-1/2 (1 - u'),   r_hi = ((max(v - dv, 0) + eps) (1 - u'))^-1/2 (1 + u'),
        dr = max(r_hi - r, r - r_lo).
    An interval, not a linearisation: on constant rows (v = 0) and rows with a large mean dv is comparable to v + eps.  For a
    stream whose mean is m deviations, dr / r is about (s + 2) u' (2 m^2 + 1): 1e-6 at m = 1 and s = 2, 8e-4 at m = 32 -- above
    fp16's half ulp (2.4e-4).  That is the sensitivity of the sum-of-squares variance to the stream's mean, and the bound shows it;
  * read-out: one fp32 rounding of r * acc + b' as an fma, or one each of the product and the sum where it is not contracted:
    2^-24 (|r acc| + |z|).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import torch

import oracle

U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
_P = {torch.bfloat16: 8, torch.float16: 11}        # significand bits (with the implicit one)
_EMIN = {torch.bfloat16: -126, torch.float16: -14}  # exponent of the smallest normal
U32 = 2.0 ** -23                                   # one full fp32 ulp: the summation bound's unit
EPS32 = 2.0 ** -24                                 # fp32 unit roundoff
C_EP = 8.0                                         # fp32 roundings of the epilogue (fast_exp2 / fast_rcp: 1 ulp each)
LIP = {"none": 1.0, "relu": 1.0, "silu": 1.1, "gelu": 1.13, "gelu_erf": 1.13}
FRAG = 16
_LOG2E = 1.4426950408889634
_C0 = 2.0 * math.sqrt(2.0 / math.pi) * _LOG2E
_C1 = 0.044715 * _C0

_BF, _FP = torch.bfloat16, torch.float16
# (dtype, route) -> (fraction not round-to-nearest, worst row, mean row, worst 16x16 fragment) in units of u; each the largest
# value one run of tests/test_gpu_gemm_matrix.py measured on the MI355X (in the comment, same order) times 2 at most
BARS = {
    (_BF, "t128"): (0.00151, 1.36, 0.881, 1.18),          # 7.56e-04 0.683 0.441 0.594
    (_BF, "t256"): (0.000571, 0.937, 0.857, 1.33),        # 2.86e-04 0.469 0.429 0.669
    (_BF, "p8w"): (0.00360, 1.97, 0.860, 1.76),           # 1.80e-03 0.989 0.430 0.881
    (_BF, "p8w_res"): (0.00265, 1.78, 0.853, 1.54),       # 1.33e-03 0.892 0.427 0.770
    (_BF, "p8w_stats"): (0.000524, 1.05, 0.847, 1.11),    # 2.62e-04 0.528 0.424 0.555
    (_BF, "glu_t128x64"): (0.000500, 1.27, 0.855, 1.35),  # 2.50e-04 0.636 0.428 0.677
    (_BF, "glu_t256x128"): (0.000505, 1.04, 0.849, 1.60), # 2.53e-04 0.522 0.425 0.804
    (_BF, "p8w_glu"): (0.000513, 1.19, 0.849, 1.63),      # 2.57e-04 0.596 0.425 0.819
    # the LayerNorm-fold routes against reference_fold(), over the cases whose stream mean is at most 4 deviations
    (_BF, "p8w_fold"): (0.000870, 1.14, 0.852, 1.23),     # 4.35e-04 0.573 0.426 0.615
    (_BF, "p8w_glu_fold"): (0.000836, 1.20, 0.848, 1.54), # 4.18e-04 0.600 0.424 0.771
    (_FP, "t128"): (0.0143, 1.66, 1.09, 1.32),            # 7.20e-03 0.832 0.545 0.663
    (_FP, "t256"): (0.00179, 0.926, 0.856, 1.27),         # 8.99e-04 0.463 0.428 0.639
    (_FP, "p8w"): (0.0306, 1.98, 0.867, 1.79),            # 1.53e-02 0.994 0.434 0.897
    (_FP, "p8w_res"): (0.0225, 1.81, 0.849, 1.50),        # 1.13e-02 0.909 0.425 0.754
    (_FP, "p8w_stats"): (0.00353, 1.07, 0.847, 1.09),     # 1.77e-03 0.537 0.424 0.549
    (_FP, "glu_t128x64"): (0.00353, 1.29, 0.845, 1.42),   # 1.77e-03 0.650 0.423 0.713
    (_FP, "glu_t256x128"): (0.00364, 1.07, 0.848, 1.57),  # 1.82e-03 0.539 0.424 0.786
    (_FP, "p8w_glu"): (0.00372, 1.13, 0.849, 1.57),       # 1.86e-03 0.567 0.425 0.786
    (_FP, "p8w_fold"): (0.00790, 1.21, 0.852, 1.32),      # 3.95e-03 0.605 0.426 0.664
    (_FP, "p8w_glu_fold"): (0.00558, 1.16, 0.848, 1.59),  # 2.79e-03 0.584 0.424 0.798
}

STATS: dict = {}


def stats_table() -> str:
    """STATS in the layout of the BARS table: the measured maxima, and the count of check() calls behind them."""
    name = {_BF: "_BF", _FP: "_FP"}
    rows = [f'    ({name[d]}, "{r}"): {v["not_rn"]:.2e} {v["worst"]:.3f} {v["mean"]:.3f} {v["frag"]:.3f}   ({v["n"]} checks)'
            for (d, r), v in sorted(STATS.items(), key=lambda kv: (name[kv[0][0]], kv[0][1]))]
    return "\n".join(["(dtype, route): not round-to-nearest, worst row, mean row, worst 16x16 fragment (u)"] + rows)


def ulp16(v: torch.Tensor, dtype) -> torch.Tensor:
    """Spacing of the 16-bit grid of `dtype` at the fp64 values v (subnormal spacing below the smallest normal)."""
    a = v.abs()
    _, e = torch.frexp(a)                 # a = m 2^e, m in [0.5, 1): floor(log2 a) = e - 1 (exact, no log2 rounding)
    e = torch.where(a > 0, e - 1, torch.full_like(e, _EMIN[dtype]))
    e = e.clamp_min(_EMIN[dtype])
    # 2^(e - p + 1) from its fp64 bit pattern: exact on any device (torch.ldexp goes through a float32 pow, which on the GPU
    # is not exact for every integer exponent)
    return torch.bitwise_left_shift((e - (_P[dtype] - 1) + 1023).to(torch.int64), 52).view(torch.float64)


def rn16(v: torch.Tensor, dtype) -> torch.Tensor:
    """Round-to-nearest-even of fp64 values onto the 16-bit grid, directly (tensor.to(bfloat16) would round twice, through
    fp32).  Returned in fp64; overflow is not handled (the tests stay far below the largest finite value)."""
    q = ulp16(v, dtype)
    return torch.round(v / q) * q  # v / q and the product are exact (powers of two); torch.round ties to even


def _act64(z: torch.Tensor, act: str) -> torch.Tensor:
    if act == "none":
        return z
    if act == "gelu":
        return oracle.mlp.gelu_tanh(z)
    if act == "gelu_erf":
        return torch.nn.functional.gelu(z)
    if act == "relu":
        return torch.relu(z)
    if act == "silu":
        return torch.nn.functional.silu(z)
    raise ValueError(act)


def _exp_arg(z: torch.Tensor, act: str) -> torch.Tensor:
    if act == "silu":
        return z.abs() * _LOG2E
    if act == "gelu":
        return z.abs() * (_C0 + _C1 * z * z)
    return torch.zeros_like(z)


@dataclass
class Ref:
    y: torch.Tensor     # fp64 [M, N]
    tol: torch.Tensor   # fp64 [M, N]: the non-rounding part of the element bound
    K: int


def _gamma(n: int) -> float:
    """gamma_n with u' = one full fp32 ulp: the bound on a sum of n + 1 terms in any order (module docstring)."""
    return n * U32 / (1.0 - n * U32)


def _finish(z, tz, act: str, zg=None, tzg=None, col_scale=None, rf=None):
    """Everything behind the pre-activation value, shared by reference() and reference_fold(): z (and zg, the SwiGLU gate) are the
    fp64 pre-activation values, tz / tzg the bound on what the kernel's fp32 evaluation of them may be off by.  Returns (y, tol):
    the activation (Lipschitz bound, product rule for SwiGLU), the epilogue's own fp32 terms, column scale and residual."""
    if act == "swiglu":
        sg = torch.nn.functional.silu(zg)
        a = sg * z
        tol = LIP["silu"] * tzg * z.abs() + sg.abs() * tz + LIP["silu"] * tzg * tz
        tol = tol + EPS32 * ((C_EP + 3.0 * _exp_arg(zg, "silu")) * a.abs() + 4.0 * z.abs())
    else:
        a = _act64(z, act)
        tol = LIP[act] * tz + EPS32 * ((C_EP + 3.0 * _exp_arg(z, act)) * a.abs() + 4.0 * z.abs())
    if col_scale is not None:
        lo, hi, s = int(col_scale[0]), int(col_scale[1]), float(col_scale[2])
        sc = torch.ones(a.shape[-1], dtype=torch.float64, device=a.device)
        sc[lo:hi] = s
        a = a * sc
        tol = tol * sc.abs() + EPS32 * a.abs()
    y = a
    if rf is not None:
        rf = rf.reshape(y.shape)
        y = y + rf
        tol = tol + 2.0 * EPS32 * (a.abs() + rf.abs())
    return y, tol


def reference(x, w, bias=None, act: str = "none", w_gate=None, bias_gate=None, residual=None, col_scale=None,
              device=None) -> Ref:
    """fp64 reference of y = act(x w^T + bias) (+ residual) [or SwiGLU], x [M, K], w [N, K] (any strides), and its element
    bound (module docstring).  col_scale = (lo, hi, s): columns [lo, hi) times s after the activation."""
    dev = torch.device("cpu") if device is None else torch.device(device)
    f = lambda t: None if t is None else t.to(dev, torch.float64)  # noqa: E731
    xf, wf, bf, rf = f(x), f(w), f(bias), f(residual)
    K = xf.shape[-1]
    xf = xf.reshape(-1, K)
    gam = _gamma(K + 1)
    ax = xf.abs()

    def pre(wf, bf):
        z, S = xf @ wf.t(), ax @ wf.abs().t()
        if bf is not None:
            z, S = z + bf, S + bf.abs()
        return z, gam * S

    z, tz = pre(wf, bf)
    zg, tzg = pre(f(w_gate), f(bias_gate)) if act == "swiglu" else (None, None)
    y, tol = _finish(z, tz, act, zg, tzg, col_scale, rf)
    return Ref(y, tol, K)


def rstd_interval(stats, K: int, eps: float):
    """(r, r_lo, r_hi), fp64 [rows]: the LayerNorm-fold consumer's rstd from the statistics it reads -- stats [slots, rows, 2] =
    fp32 (sum, sum of squares) per 256-column slot -- and the interval its fp32 evaluation stays in (module docstring)."""
    st = stats.to(torch.float64)
    s = st.shape[0]
    e = float(torch.tensor(eps, dtype=torch.float32))           # the kernel takes eps as an fp32 argument
    mu = st[..., 0].sum(0) / K
    A = st[..., 0].abs().sum(0) / K
    Q = st[..., 1].sum(0) / K
    Qa = st[..., 1].abs().sum(0) / K
    v = (Q - mu * mu).clamp_min(0.0)
    g1 = _gamma(s + 1)
    m2 = (1.0 + g1) ** 2 * (1.0 + U32)                          # fl(fl(mu)^2) <= m2 A^2
    dv = g1 * Qa + (m2 - 1.0) * A * A + U32 * ((1.0 + g1) * Qa + m2 * A * A)
    r = (v + e) ** -0.5
    r_lo = ((v + dv + e) * (1.0 + U32)) ** -0.5 * (1.0 - U32)
    r_hi = (((v - dv).clamp_min(0.0) + e) * (1.0 - U32)) ** -0.5 * (1.0 + U32)
    return r, r_lo, r_hi


def reference_fold(y, stats, ws, bias=None, *, eps: float = 1e-5, act: str = "none", ws_gate=None, bias_gate=None,
                   col_scale=None, device=None) -> Ref:
    """fp64 reference of one LayerNorm-fold consumer call, z = act(r (y ws^T) + bias) [SwiGLU: silu(r (y ws_gate^T) + bias_gate)
    * (r (y ws^T) + bias)], from exactly what the kernel reads: the stream y [M, K], the statistics handed to the launch
    (stats [slots, >= M rows, 2], rows as y's), the folded 16-bit weight(s) and bias(es) of ln_fold_weight, eps; and its element
    bound (module docstring, "LayerNorm fold")."""
    dev = torch.device("cpu") if device is None else torch.device(device)
    f = lambda t: None if t is None else t.to(dev, torch.float64)  # noqa: E731
    yf = f(y)
    K = yf.shape[-1]
    yf = yf.reshape(-1, K)
    M = yf.shape[0]
    r, r_lo, r_hi = (t[:, None] for t in rstd_interval(stats[:, :M].to(dev), K, eps))
    dr = torch.maximum(r_hi - r, r - r_lo)
    gam = _gamma(K)
    ay = yf.abs()

    def pre(wf, bf):
        acc, S = yf @ wf.t(), ay @ wf.abs().t()
        z = r * acc if bf is None else r * acc + bf
        # accumulator at the upper end of r, rstd on the exact accumulator, the read-out's fma (or a product and a sum)
        return z, r_hi * (gam * S) + acc.abs() * dr + EPS32 * ((r * acc).abs() + z.abs())

    z, tz = pre(f(ws), f(bias))
    zg, tzg = pre(f(ws_gate), f(bias_gate)) if act == "swiglu" else (None, None)
    out, tol = _finish(z, tz, act, zg, tzg, col_scale)
    return Ref(out, tol, K)


def reference_mlp(x, w1, b1, w2, b2, act: str, w_gate=None, bias_gate=None, residual=None, dtype=None, device=None) -> Ref:
    """fp64 reference of the fused MLP y = (h w2^T + b2) (+ residual), h = the stage-1 result rounded to the storage dtype as
    the kernel stores it.  Where the stage-1 value's bound interval [ref - tol, ref + tol] holds a rounding boundary of the
    16-bit grid the kernel may store the other neighbour: the bound adds |w2| (one ulp of such h) for those."""
    dtype = x.dtype if dtype is None else dtype
    r1 = reference(x, w1, b1, act, w_gate, bias_gate, device=device)
    h = rn16(r1.y, dtype)
    tie = rn16(r1.y - r1.tol, dtype) != rn16(r1.y + r1.tol, dtype)
    dh = torch.where(tie, ulp16(r1.y.abs() + r1.tol, dtype), torch.zeros_like(h))
    r2 = reference(h, w2, b2, residual=residual, device=device)
    if bool(tie.any()):
        r2.tol = r2.tol + dh @ w2.to(r2.y.device, torch.float64).abs().t()
    return r2


def element_bound(ref: Ref, dtype) -> torch.Tensor:
    return torch.maximum(ulp16(ref.y, dtype), ulp16(ref.y.abs() + ref.tol, dtype) / 2) + ref.tol


def _norm_stat(d: torch.Tensor, r: torch.Tensor, dims) -> torch.Tensor:
    num = (d * d).sum(dims).sqrt()
    den = (r * r).sum(dims).sqrt()
    return num / torch.where(den > 0, den, torch.ones_like(den))


def measure(y: torch.Tensor, ref: Ref, dtype) -> dict:
    """The statistics check() bounds (module docstring, item 3)."""
    yf = y.to(ref.y.device, torch.float64).reshape(ref.y.shape)
    u = U[dtype]
    d = yf - ref.y
    rows = _norm_stat(d, ref.y, 1) / u
    M, N = d.shape
    pm, pn = (-M) % FRAG, (-N) % FRAG
    dp = torch.nn.functional.pad(d, (0, pn, 0, pm)).view((M + pm) // FRAG, FRAG, (N + pn) // FRAG, FRAG)
    rp = torch.nn.functional.pad(ref.y, (0, pn, 0, pm)).view_as(dp)
    frag = _norm_stat(dp, rp, (1, 3)) / u
    not_rn = (yf != rn16(ref.y, dtype)).double().mean()
    return {"not_rn": not_rn.item(), "worst": rows.max().item() if M else 0.0, "mean": rows.mean().item() if M else 0.0,
            "frag": frag.max().item() if M else 0.0}


def check(y: torch.Tensor, ref: Ref, dtype, route: str, *, guard: Optional[torch.Tensor] = None, fill=None, what: str = "",
          bars=True) -> dict:
    """Assert the kernel output y ([M, N] view, any strides, in dtype) against ref: finite, guard untouched (guard = the
    whole buffer y is a view of, filled with `fill` before the launch), the element bound, and -- unless bars=False (inputs
    built to land in the subnormal range, where a relative statistic means nothing) -- the bars of (dtype, route); bars = a
    4-tuple in the order of BARS: these fixed limits in their place (the checker's self-tests, which are no kernel route and are
    not recorded in STATS).  Returns the measured statistics."""
    tag = f"{what} [{route} {str(dtype).split('.')[-1]}]"
    y2 = y.reshape(ref.y.shape) if y.dim() != 2 else y
    assert tuple(y2.shape) == tuple(ref.y.shape), f"{tag}: shape {tuple(y2.shape)} vs {tuple(ref.y.shape)}"
    assert y2.dtype == dtype, f"{tag}: dtype {y2.dtype}"
    assert bool(torch.isfinite(y2).all()), f"{tag}: non-finite output ({int((~torch.isfinite(y2)).sum())} values)"
    if guard is not None:
        # the view's elements are guard elements too: what differs from the fill outside it = all of them - the view's
        assert y2.untyped_storage().data_ptr() == guard.untyped_storage().data_ptr(), f"{tag}: y is not a view of guard"
        bad = int((guard != fill).sum()) - int((y2 != fill).sum())
        assert bad == 0, f"{tag}: {bad} guard elements outside the output view were overwritten"
    yf = y2.to(ref.y.device, torch.float64)
    err = (yf - ref.y).abs()
    bnd = element_bound(ref, dtype)
    over = err > bnd
    if bool(over.any()):
        i = int(torch.argmax((err / bnd).reshape(-1)))
        m, n = divmod(i, ref.y.shape[1])
        raise AssertionError(f"{tag}: {int(over.sum())} elements outside the rounding bound; worst at ({m}, {n}): "
                             f"y {yf[m, n].item():.6g} ref {ref.y[m, n].item():.6g} |err| {err[m, n].item():.3g} "
                             f"bound {bnd[m, n].item():.3g}")
    if bars is False:
        return {}
    st = measure(y2, ref, dtype)
    if bars is True:
        key = (dtype, route)
        rec = STATS.setdefault(key, {"not_rn": 0.0, "worst": 0.0, "mean": 0.0, "frag": 0.0, "n": 0})
        for name in ("not_rn", "worst", "mean", "frag"):
            rec[name] = max(rec[name], st[name])
        rec["n"] += 1
        bars = BARS[key]
    not_rn, worst, mean, frag = bars
    assert st["not_rn"] <= not_rn and st["worst"] <= worst and st["mean"] <= mean and st["frag"] <= frag, (
        f"{tag}: not round-to-nearest {st['not_rn']:.4f} (bar {not_rn}), worst row {st['worst']:.3f} u (bar {worst}), "
        f"mean row {st['mean']:.3f} u (bar {mean}), worst 16x16 fragment {st['frag']:.3f} u (bar {frag})")
    return st

"""RMSNorm checker shared by the RMSNorm tests (a plain helper module, not a conftest): fp64 references of the row kernel
(ops.rmsnorm) and of the RMS form of the folded consumer GEMM (ops.gemm_ln(..., norm="rms")), each with the per-element bound
`tol` on what a correct kernel's fp32 arithmetic may add before its one rounding to the storage dtype.  The references are
judged with _gemm_check.element_bound / _gemm_check.check; u' = 2^-23 (one full fp32 ulp, _gemm_check.U32) is charged for every
rounding, as _gemm_check charges them, so a unit that truncates is covered too.  No fitted constants.

Row kernel (reference_rows).  y = T(s * r * w), r = (mean(s^2) + eps)^-1/2, from the 16-bit s and w the kernel reads (with a
residual: s is the kernel's own stored sum_out, so the sum's rounding is judged apart, sum_bound()).  The kernel's operation
sequence and its cost:
  * s_i^2: exact in fp32 (8 x 8 or 11 x 11 bit significands), fused into the add or not;
  * the sum of `cols` non-negative terms in any order (per lane, then across the wave): relative error gamma_cols
    (_gemm_check._gamma(cols): n + 1 terms in any order); the zero padding of a ragged last chunk adds exactly;
  * the division by cols: one rounding.  With Q = mean(s^2): |fl - Q| <= dv = gamma_{cols+1} Q;
  * the eps add and the reciprocal square root (v_rsq_f32, 1 ulp): u' each, an interval (not a linearisation: on a zero row
    Q = 0 and eps is all there is):
        r_lo = ((Q + dv + eps) (1 + u'))^-1/2 (1 - u'),   r_hi = ((max(Q - dv, 0) + eps) (1 - u'))^-1/2 (1 + u'),
        dr = max(r_hi - r, r - r_lo);
  * the two products s * r and (s r) * w: u' each.
        tol = |s w| (dr + r_hi ((1 + u')^2 - 1)).
A zero row has tol = 0 and reference 0: the kernel's 0 * r * w is exactly 0, which the tests also assert.  eps is the fp32
value the kernel is handed.

The sum (sum_bound).  s = T(x + alpha res): alpha * res and the add round once each in fp32 (once together where fused):
    ts = u' (|alpha res| + |x + alpha res|),      |sum_out - (x + alpha res)| <= ulp16(|ref| + ts) / 2 + ts:
half a 16-bit ulp of the fp32 value, which lies within ts of the exact sum.

RMS fold (reference_fold_rms), the routes p8w_fold / p8w_glu_fold behind mio_gemm_rms_bw: _gemm_check.reference_fold's twin.
The consumer reads the raw stream y [M, K], per row s <= 8 fp32 slots of (sum, sum of squares) -- of which it uses the second --
the 16-bit weight ws = T(w gamma) of ops.rms_fold_weight and the bias, and stores z = act(r (y ws^T) + b), r = (Q + eps)^-1/2,
Q = sum_s sq_s / K.  The kernel's rstd sequence is s - 1 adds, the rounded 1 / K, the product sq * ik, the eps add and
v_rsq_f32; there are no mean terms:
    dv = gamma_{s+1} sum_s |sq_s| / K,      r_lo, r_hi, dr as above.
Everything behind rstd is _gemm_check's: tz = r_hi gamma_K |y||ws|^T + |y ws^T| dr + 2^-24 (|r y ws^T| + |z|), then _finish().
"""
from __future__ import annotations

import torch

import _gemm_check as gc
from _gemm_check import EPS32, U32, Ref, _finish, _gamma

_BF, _FP = torch.bfloat16, torch.float16
# dtype -> the fraction of elements of ops.rmsnorm's output that are not the round-to-nearest of reference_rows() on the 16-bit
# grid, over all cases of one test: the largest value one run of tests/test_gpu_rmsnorm.py measured on the MI355X (in the
# comment) times 2 at most
ROW_NOT_RN = {
    _BF: 2.7e-05,  # 1.370e-05
    _FP: 1.4e-04,  # 7.484e-05
}


def _f32(v: float) -> float:
    return float(torch.tensor(v, dtype=torch.float32))


def _interval(Q, dv, eps: float):
    """(r, dr) from the exact second moment Q, the bound dv on its fp32 evaluation, eps as an fp32 value (module docstring)."""
    e = _f32(eps)
    r = (Q + e) ** -0.5
    r_lo = ((Q + dv + e) * (1.0 + U32)) ** -0.5 * (1.0 - U32)
    r_hi = (((Q - dv).clamp_min(0.0) + e) * (1.0 - U32)) ** -0.5 * (1.0 + U32)
    return r, r_hi, torch.maximum(r_hi - r, r - r_lo)


def reference_rows(s, w, eps: float, device=None) -> Ref:
    """fp64 RMSNorm of the 16-bit rows s [rows, cols] with the 16-bit weight w [cols], and its element bound."""
    dev = torch.device("cpu") if device is None else torch.device(device)
    sf, wf = s.to(dev, torch.float64), w.to(dev, torch.float64)
    cols = sf.shape[-1]
    sf = sf.reshape(-1, cols)
    Q = (sf * sf).mean(-1, keepdim=True)
    r, r_hi, dr = _interval(Q, _gamma(cols + 1) * Q, eps)
    sw = sf * wf
    return Ref(sw * r, sw.abs() * (dr + r_hi * ((1.0 + U32) ** 2 - 1.0)), cols)


def sum_bound(x, res, alpha: float, dtype, device=None):
    """(fp64 x + alpha res, the bound on |sum_out - it|), [rows, cols] (module docstring, "The sum")."""
    dev = torch.device("cpu") if device is None else torch.device(device)
    xf, ar = x.to(dev, torch.float64), res.to(dev, torch.float64) * _f32(alpha)
    ref = xf + ar
    ts = U32 * (ar.abs() + ref.abs())
    return ref, gc.ulp16(ref.abs() + ts, dtype) / 2 + ts


def rstd_interval_rms(stats, K: int, eps: float):
    """(r, r_hi, dr), fp64 [rows], of the RMS consumer from the statistics it reads: stats [slots, rows, 2]; only [..., 1] (the
    sums of squares) is read, so the sums may hold anything."""
    sq = stats[..., 1].to(torch.float64)
    s = sq.shape[0]
    return _interval(sq.sum(0) / K, _gamma(s + 1) * sq.abs().sum(0) / K, eps)


def reference_fold_rms(y, stats, ws, bias=None, *, eps: float = 1e-6, act: str = "none", ws_gate=None, bias_gate=None,
                       col_scale=None, device=None) -> Ref:
    """fp64 reference of one RMS-fold consumer call, z = act(r (y ws^T) + bias) [SwiGLU: silu(r (y ws_gate^T) + bias_gate) *
    (r (y ws^T) + bias)], from exactly what the kernel reads -- the stream y [M, K], the statistics handed to the launch (stats
    [slots, >= M rows, 2], rows as y's), the 16-bit weight(s) of rms_fold_weight and the bias(es), eps -- and its element bound."""
    dev = torch.device("cpu") if device is None else torch.device(device)
    f = lambda t: None if t is None else t.to(dev, torch.float64)  # noqa: E731
    yf = f(y)
    K = yf.shape[-1]
    yf = yf.reshape(-1, K)
    M = yf.shape[0]
    r, r_hi, dr = (t[:, None] for t in rstd_interval_rms(stats[:, :M].to(dev), K, eps))
    gam = _gamma(K)
    ay = yf.abs()

    def pre(wf, bf):
        acc, S = yf @ wf.t(), ay @ wf.abs().t()
        z = r * acc if bf is None else r * acc + bf
        return z, r_hi * (gam * S) + acc.abs() * dr + EPS32 * ((r * acc).abs() + z.abs())

    z, tz = pre(f(ws), f(bias))
    zg, tzg = pre(f(ws_gate), f(bias_gate)) if act == "swiglu" else (None, None)
    out, tol = _finish(z, tz, act, zg, tzg, col_scale)
    return Ref(out, tol, K)


def not_rn(y, ref: Ref, dtype) -> float:
    """The fraction of elements of y that are not the round-to-nearest of ref.y on the 16-bit grid."""
    return (y.to(ref.y.device, torch.float64).reshape(ref.y.shape) != gc.rn16(ref.y, dtype)).double().mean().item()

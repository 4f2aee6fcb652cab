"""QK-norm checker shared by the QK-norm tests (a plain helper module, not a conftest): the fp64 reference of the per-head
RMSNorm followed by the rotary rotation, and a per-element interval composed from the two models the project already has.
No constant is fitted.

reference(): for a head row x[0 .. D) (16-bit), a weight w[0 .. D) (16-bit) and the fp32 eps the kernel is handed,
    n[d] = x[d] r w[d],   r = (mean_{d < D}(x[d]^2) + eps)^-1/2,
then the first rot = 2 * cos.shape[1] elements of n rotated as _rope_check.reference rotates (same fp32 table entries), the
others n itself; everything in fp64.

The allowance delta of an element, on what a correct kernel's fp32 arithmetic may add before its ONE rounding to storage:
  * the norm: _rms_check.reference_rows with cols = D, tol_n = |x w| (dr + r_hi ((1 + u')^2 - 1)); dr is its _interval's (the
    sum of D squares in any order, the division by D, the eps add, v_rsq_f32), the second term the two products x * r * w;
  * the rotation of the (inexact, unrounded) n adds _rope_check's three-rounding term:
        delta(y1) = |c| tol_n1 + |s| tol_n2 + 4 * 2^-24 (|n1 c| + |n2 s|),      y1 = n1 c - n2 s,
        delta(y2) = |c| tol_n2 + |s| tol_n1 + 4 * 2^-24 (|n2 c| + |n1 s|),      y2 = n2 c + n1 s;
  * an element past rot has delta = tol_n.
The judgement is _rope_check.outside16 / outside8: the stored value lies in [rn(ref - delta), rn(ref + delta)], for the fp8 cache
in the scaled domain (scaled_bounds8).  The bar is zero elements outside.  There is no 16-bit rounding between the norm and the
rotation in this model, so a kernel that rounds n first is (rightly) outside it.
"""
from __future__ import annotations

import torch

import _rms_check as rms
from _rope_check import EPS, outside8, outside16  # noqa: F401  (the judgement is _rope_check's, on whole head rows)


def reference(x, w, eps: float, cos, sin, positions, interleaved):
    """x [T, heads, D] 16-bit, w [D] 16-bit, eps a python float (used as its fp32 value), cos / sin fp32 [P, rot / 2], positions
    long [T] inside [0, P): (ref, delta) fp64 [T, heads, D] in storage order."""
    T, Hn, D = x.shape
    half = cos.shape[1]
    rot = 2 * half
    r = rms.reference_rows(x.reshape(T * Hn, D), w, eps)
    n, tn = r.y.view(T, Hn, D), r.tol.view(T, Hn, D)
    c = cos[positions].to(torch.float64)[:, None, :]
    s = sin[positions].to(torch.float64)[:, None, :]
    nr, tr = n[..., :rot], tn[..., :rot]
    if interleaved:
        n1, n2, t1, t2 = nr[..., 0::2], nr[..., 1::2], tr[..., 0::2], tr[..., 1::2]
    else:
        n1, n2, t1, t2 = nr[..., :half], nr[..., half:], tr[..., :half], tr[..., half:]
    y1, y2 = n1 * c - n2 * s, n2 * c + n1 * s
    d1 = c.abs() * t1 + s.abs() * t2 + 4 * EPS * ((n1 * c).abs() + (n2 * s).abs())
    d2 = c.abs() * t2 + s.abs() * t1 + 4 * EPS * ((n2 * c).abs() + (n1 * s).abs())
    if interleaved:
        y, d = torch.stack([y1, y2], -1).flatten(-2), torch.stack([d1, d2], -1).flatten(-2)
    else:
        y, d = torch.cat([y1, y2], -1), torch.cat([d1, d2], -1)
    return torch.cat([y, n[..., rot:]], -1), torch.cat([d, tn[..., rot:]], -1)


def rms16(x, w, eps: float):
    """The first step of the two-step chain the fused forms replace: the per-head RMSNorm as torch ops in fp32, rounded to x's
    16-bit dtype (x [..., D], w [D])."""
    xf = x.float()
    r = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return (xf * r * w.float()).to(x.dtype)

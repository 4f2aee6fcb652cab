"""Checker of the decode-step GEMM on weight-only FP8 (ops.gemm_skinny_w8), a plain helper module next to tests/_gemm_check.py,
whose element bound, statistics and check() it uses.

reference_w8(): the fp64 result from the very bytes and scales the kernel reads,
    z = s * (x q^T) + b            (q the e4m3fn weight bytes widened exactly, s the fp32 scale of the column, b the bias)
    y = act(z) (+ r)               SwiGLU: silu(z_gate) * z (+ r), the gate with its own bytes, scales and bias
so the quantisation of a weight is not part of the error judged.  The bound on what the kernel's fp32 evaluation of z may be off by
    tz = |s| gamma_K (|x||q|^T)  +  2^-24 (|s acc| + |z|)
  * the first term is the summation bound of K exact products in any order (gc._gamma: split-K, MFMA-internal, truncating
    accumulators): a product of an 8- or 11-bit significand (bf16, fp16) and a 4-bit one (e4m3) is exact in fp32, and no bias is
    among the terms;
  * the second term is the read-out's fma(acc, s, b), or a product and a sum where it is not contracted.
Everything behind z (activation, epilogue terms, SwiGLU product rule, residual) is gc._finish, as for the 16-bit kernel.

The statistical bars are those of the 16-bit decode-step GEMM's tests, gc.BARS[(dtype, "t128")]: the extra multiply is 2^-24
relative, far below a 16-bit ulp, and the summation is the same code.  judge() records the measured statistics in gc.STATS as the
row (dtype, "skinny_w8")."""
import torch

import _gemm_check as gc

FP8 = torch.float8_e4m3fn
BARS = {dt: gc.BARS[(dt, "t128")] for dt in (torch.bfloat16, torch.float16)}


def widen(q: torch.Tensor, dev) -> torch.Tensor:
    """e4m3fn bytes as fp64 (exact: through fp32, which holds every e4m3 value)."""
    return q.to(dev).to(torch.float32).to(torch.float64)


def reference_w8(x, w8, w_scale, bias=None, act: str = "none", w8_gate=None, w_scale_gate=None, bias_gate=None, residual=None,
                 device=None) -> gc.Ref:
    """fp64 reference of one gemm_skinny_w8 call and its element bound (module docstring).  x [M, K] (any strides; K may be 0),
    w8 / w8_gate [N, K] torch.float8_e4m3fn, scales fp32 [N] or one element."""
    dev = torch.device("cpu") if device is None else torch.device(device)
    f = lambda t: None if t is None else t.to(dev, torch.float64)  # noqa: E731
    K = x.shape[-1]
    xf = f(x)
    xf = xf if xf.dim() == 2 else xf.reshape(-1, K)
    ax, gam = xf.abs(), gc._gamma(K)

    def pre(q, s, b):
        assert q.dtype == FP8 and s.dtype == torch.float32
        qf, sf = widen(q, dev), f(s).reshape(1, -1)
        acc, S = xf @ qf.t(), ax @ qf.abs().t()
        z = sf * acc if b is None else sf * acc + f(b)
        return z, sf.abs() * (gam * S) + gc.EPS32 * ((sf * acc).abs() + z.abs())

    z, tz = pre(w8, w_scale, bias)
    zg, tzg = pre(w8_gate, w_scale_gate, bias_gate) if act == "swiglu" else (None, None)
    y, tol = gc._finish(z, tz, act, zg, tzg, None, f(residual))
    return gc.Ref(y, tol, K)


def judge(y, ref, dtype, what, guard=None, fill=None):
    """gc.check under BARS[dtype]; the measured statistics go to gc.STATS as the row (dtype, "skinny_w8")."""
    st = gc.check(y, ref, dtype, "skinny_w8", guard=guard, fill=fill, bars=BARS[dtype], what=what)
    rec = gc.STATS.setdefault((dtype, "skinny_w8"), {"not_rn": 0.0, "worst": 0.0, "mean": 0.0, "frag": 0.0, "n": 0})
    for name in ("not_rn", "worst", "mean", "frag"):
        rec[name] = max(rec[name], st[name])
    rec["n"] += 1
    return st

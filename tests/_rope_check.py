"""Rotary-embedding checker shared by the rotary tests (a plain helper module, not a conftest).

reference(): the fp64 rotation y1 = x1 c - x2 s, y2 = x2 c + x1 s of the first rot_dim = 2 * cos.shape[1] elements of every
head, from the same 16-bit inputs and the same fp32 table entries the kernels read, together with the error allowance
delta = 4 * 2^-24 * (|x1 c| + |x2 s|) of each output element (for y2: |x2 c| + |x1 s|): it covers the three fp32 roundings
of the evaluation (two products and a sum, or one product and one fused multiply-add) with margin.

rn(): round to nearest even from fp64 straight to a storage format (bf16, fp16, e4m3fn).  torch's own casts from fp64 go
through fp32 and so round twice; this one looks the two neighbouring representable values up in the sorted table of the
format's finite values and takes the nearer (a tie: the one with the even bit pattern).

outside16() / outside8(): how many stored elements lie outside [rn(ref - delta), rn(ref + delta)].  For the fp8 cache the
interval is taken in the scaled domain: ref * inv, delta * inv + 2^-24 |ref * inv| (the multiply by inv rounds once more),
clamped to +-448 before the e4m3 rounding; inv is the fp32 reciprocal of the scale.  Nothing here is measured: a plain fp32
evaluation stays inside these intervals, and about 2e-5 (bf16) to 1.4e-4 (fp16) of its elements differ from rn(ref), so
equality with rn(ref) would be the wrong test and the interval is tight.
"""
from __future__ import annotations

import torch

F8 = torch.float8_e4m3fn
EPS = 2.0 ** -24

_TABLES: dict = {}


def _table(dtype):
    """(values fp64 ascending, even-pattern flags) of the finite values of dtype, -0 dropped."""
    if dtype not in _TABLES:
        if dtype == F8:
            bits = torch.arange(256, dtype=torch.int32)
            vals = bits.to(torch.uint8).view(F8).to(torch.float64)
        else:
            bits = torch.arange(65536, dtype=torch.int32)
            vals = bits.to(torch.int16).view(dtype).to(torch.float64)
        sign_bit = 0x80 if dtype == F8 else 0x8000
        keep = torch.isfinite(vals) & (bits != sign_bit)
        vals, bits = vals[keep], bits[keep]
        order = torch.argsort(vals)
        _TABLES[dtype] = (vals[order].contiguous(), (bits[order] & 1) == 0)
    return _TABLES[dtype]


def rn(x, dtype):
    """fp64 x rounded to nearest even into dtype, as fp64 values (x within the format's finite range)."""
    vals, even = _table(dtype)
    x = x.to(torch.float64)
    hi = torch.searchsorted(vals, x.contiguous()).clamp(1, vals.numel() - 1)
    lo = hi - 1
    dl, dh = x - vals[lo], vals[hi] - x
    take_hi = (dh < dl) | ((dh == dl) & even[hi])
    return torch.where(take_hi, vals[hi], vals[lo])


def reference(x, cos, sin, positions, interleaved):
    """x [T, heads, D] 16-bit, cos / sin fp32 [P, rot / 2], positions long [T] inside [0, P): (ref, delta) fp64
    [T, heads, rot] in storage order."""
    half = cos.shape[1]
    rot = 2 * half
    c = cos[positions].to(torch.float64)[:, None, :]
    s = sin[positions].to(torch.float64)[:, None, :]
    xr = x[..., :rot].to(torch.float64)
    if interleaved:
        x1, x2 = xr[..., 0::2], xr[..., 1::2]
    else:
        x1, x2 = xr[..., :half], xr[..., half:]
    y1, y2 = x1 * c - x2 * s, x2 * c + x1 * s
    d1 = 4 * EPS * ((x1 * c).abs() + (x2 * s).abs())
    d2 = 4 * EPS * ((x2 * c).abs() + (x1 * s).abs())
    if interleaved:
        return torch.stack([y1, y2], -1).flatten(-2), torch.stack([d1, d2], -1).flatten(-2)
    return torch.cat([y1, y2], -1), torch.cat([d1, d2], -1)


def outside16(y, ref, delta, dtype):
    """Number of elements of y (16-bit, the shape of ref) outside [rn(ref - delta), rn(ref + delta)], and the number that
    differ from rn(ref) (reported, never asserted)."""
    yv = y.to(torch.float64)
    bad = (yv < rn(ref - delta, dtype)) | (yv > rn(ref + delta, dtype)) | torch.isnan(yv)
    return int(bad.sum()), int((yv != rn(ref, dtype)).sum())


def scaled_bounds8(ref, delta, scale):
    """(lo, hi) fp64 e4m3 values of the interval of the fp8 cache's rotated K; scale a python float (the fp32 scale)."""
    inv = (torch.tensor(1.0, dtype=torch.float32) / torch.tensor(scale, dtype=torch.float32)).to(torch.float64)
    rs = ref * inv
    ds = delta * inv + EPS * rs.abs()
    return rn((rs - ds).clamp(-448, 448), F8), rn((rs + ds).clamp(-448, 448), F8)


def outside8(y8, ref, delta, scale):
    """Number of e4m3 elements of y8 outside the interval of scaled_bounds8."""
    lo, hi = scaled_bounds8(ref, delta, scale)
    yv = y8.to(torch.float32).to(torch.float64)
    return int(((yv < lo) | (yv > hi) | torch.isnan(yv)).sum())

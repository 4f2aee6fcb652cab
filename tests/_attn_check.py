"""Attention-forward checker shared by the GPU attention tests (a plain helper module, not a conftest).

reference(): the fp64 oracle (oracle.attention_with_lse's formula) with the library's mask conventions
(include/mio_hip.h): without a user mask, causal-excluded keys are absent (-inf); with one, they get the reference's -1e9
fill (oracle.standard_attention); keep-masked keys get -1e9; additive entries are floored at -1e30.  Evaluated on the same
16-bit inputs the kernel sees, on the CPU or -- for sizes the CPU cannot do in seconds -- on the GPU in float64.

check(): judges a kernel result against it, row by row (a row = one (batch, head, query) output vector of D values):
  * every output finite, and lse finite wherever the reference's is;
  * rows with no visible key: o exactly 0 and lse exactly -inf;
  * per-row normwise relative error ||o - ref|| / ||ref|| in units of the storage dtype's unit roundoff u (bf16 2^-8,
    fp16 2^-11): its worst row, its mean over all rows, and its worst mean over one 16-row group of consecutive queries
    (the unit a mis-applied rescale or a wrong lane-to-row mapping of the kernels corrupts);
  * |lse - ref_lse| / max(1, |ref_lse|) per row.
The bars are per dtype and kernel family (the route names of mio._lib.FA3_ROUTES), set from one run of
tests/test_gpu_attention_matrix.py on the MI355X at no more than 2x the worst value measured (written next to each bar).
STATS collects the measured values of every check() call of a process (max per (dtype, family)).
"""
from __future__ import annotations

import math
from typing import Optional

import torch

import oracle

U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
ADD_MASK_FLOOR = -1e30  # MIO_MASK_ADD_F32 entries below count as this (include/mio_hip.h)
GROUP = 16              # query rows per group of the group-mean statistic

# (dtype, family) -> (worst row, mean over rows, worst 16-row group mean) in units of u, and the lse bar; each the largest value one
# run of tests/test_gpu_attention_matrix.py measured on the MI355X (in the comment, same order) times 2, rounded down
_BF, _FP = torch.bfloat16, torch.float16
BARS = {
    (_BF, "fwd5"): (2.9, 1.2, 1.8, 2.2e-3),            # 1.451 0.602 0.922 1.12e-3
    (_BF, "fwd5_kpre"): (3.7, 1.21, 1.5, 2.9e-3),      # 1.882 0.607 0.779 1.45e-3
    (_BF, "fwd5_kpre_carry"): (2.1, 1.21, 1.2, 3.1e-4),# 1.081 0.610 0.644 1.59e-4
    (_BF, "fwd5_kpre_oblk"): (1.9, 1.17, 1.3, 0.0),    # 0.955 0.587 0.661 (no lse)
    (_BF, "fwd3"): (1.8, 1.18, 1.4, 2.4e-3),           # 0.941 0.593 0.713 1.25e-3
    (_BF, "fwd3_kpre"): (1.8, 1.17, 1.3, 2.3e-3),      # 0.949 0.589 0.657 1.18e-3
    (_BF, "fwd1"): (2.1, 1.24, 1.4, 5.2e-7),           # 1.077 0.624 0.720 2.62e-7
    (_BF, "fwd1_keep"): (1.8, 1.17, 1.4, 3.6e-7),      # 0.930 0.589 0.702 1.83e-7
    (_BF, "fwd1_add"): (2.2, 1.15, 1.4, 3.7e-7),       # 1.133 0.575 0.704 1.85e-7
    (_BF, "merge"): (2.0, 1.18, 1.2, 1.8e-4),            # 1.017 0.593 0.645 9.14e-5
    (_FP, "fwd5"): (2.9, 1.21, 1.6, 3.7e-4),           # 1.486 0.606 0.804 1.89e-4
    (_FP, "fwd5_kpre"): (3.1, 1.19, 1.4, 2.7e-4),      # 1.558 0.599 0.740 1.35e-4
    (_FP, "fwd5_kpre_carry"): (2.0, 1.21, 1.4, 4.9e-5),  # 1.006 0.606 0.717 2.47e-5
    (_FP, "fwd5_kpre_oblk"): (1.9, 1.17, 1.3, 0.0),    # 0.975 0.587 0.664 (no lse)
    (_FP, "fwd3"): (1.9, 1.18, 1.6, 3.1e-4),           # 0.992 0.594 0.833 1.58e-4
    (_FP, "fwd3_kpre"): (1.8, 1.17, 1.3, 3.2e-4),      # 0.915 0.588 0.650 1.62e-4
    (_FP, "fwd1"): (2.5, 1.22, 1.3, 4.4e-7),           # 1.267 0.614 0.667 2.24e-7
    (_FP, "fwd1_keep"): (1.9, 1.18, 1.2, 3.1e-7),      # 0.974 0.592 0.633 1.59e-7
    (_FP, "fwd1_add"): (2.1, 1.16, 1.3, 5.9e-7),       # 1.091 0.582 0.687 2.96e-7
    (_FP, "merge"): (1.6, 1.17, 1.2, 2.1e-5),          # 0.840 0.589 0.629 1.05e-5
}

STATS: dict = {}


def reference(q, k, v, *, layout="bshd", causal=False, softmax_scale=None, keep_mask=None, additive_mask=None,
              q_offset=0, k_offset=0, device=None):
    """fp64 (o [B,Sq,H,D], lse [B,H,Sq]) of one fa3_fwd call, on `device` (default: the CPU).  q/k/v in `layout`; masks
    4-D and broadcastable to [B,H,Sq,Sk] as fa3_fwd takes them."""
    dev = torch.device("cpu") if device is None else torch.device(device)
    if layout == "bhsd":
        q, k, v = (t.permute(0, 2, 1, 3) for t in (q, k, v))
    qf, kf, vf = (t.to(dev, torch.float64) for t in (q, k, v))
    B, Sq, H, D = qf.shape
    Sk, Hkv = kf.shape[1], kf.shape[2]
    scale = (1.0 / math.sqrt(D)) if softmax_scale is None else softmax_scale
    if Hkv != H:
        kf = kf.repeat_interleave(H // Hkv, dim=2)
        vf = vf.repeat_interleave(H // Hkv, dim=2)
    s = torch.einsum("bshd,bkhd->bhsk", qf, kf) * scale
    user_mask = keep_mask is not None or additive_mask is not None
    if causal:
        qi = torch.arange(Sq, device=dev)[:, None] + q_offset
        ki = torch.arange(Sk, device=dev)[None, :] + k_offset
        s = s.masked_fill((ki > qi)[None, None], oracle.attention.NEG_FILL if user_mask else float("-inf"))
    if keep_mask is not None:
        s = torch.where(keep_mask.to(dev) != 0, s, torch.full_like(s, oracle.attention.NEG_FILL))
    if additive_mask is not None:
        s = s + additive_mask.to(dev, torch.float64).clamp_min(ADD_MASK_FLOOR)
    # max-subtracted (exp(s - lse) would lose the row sum next to a -1e30 floor: -1e30 + log(n) rounds to -1e30)
    m = s.amax(dim=-1) if Sk > 0 else torch.full(s.shape[:-1], float("-inf"), dtype=s.dtype, device=dev)
    empty = torch.isinf(m) & (m < 0)
    p = torch.exp(s - torch.where(empty, torch.zeros_like(m), m)[..., None])
    p = torch.where(empty[..., None], torch.zeros_like(p), p)
    l = p.sum(-1)
    lse = torch.where(empty, m, m + torch.log(l))
    o = torch.einsum("bhsk,bkhd->bshd", p / torch.where(empty, torch.ones_like(l), l)[..., None], vf)
    return o, lse


def row_errors(o, ref):
    """Per-row normwise relative error of o against ref ([B,Sq,H,D] both) as [B,H,Sq] float64; rows whose reference
    is exactly 0 count their absolute norm."""
    d = (o.to(ref.device, torch.float64) - ref).permute(0, 2, 1, 3)
    rn = ref.permute(0, 2, 1, 3).norm(dim=-1)
    return d.norm(dim=-1) / torch.where(rn > 0, rn, torch.ones_like(rn))


def measure(o, ref, dtype, lse=None, ref_lse=None):
    """The statistics check() bounds: dict(worst, mean, group in units of u; lse)."""
    u = U[dtype]
    live = ~(torch.isinf(ref_lse) & (ref_lse < 0)) if ref_lse is not None else torch.ones(ref.shape[0], ref.shape[2],
                                                                                        ref.shape[1], dtype=torch.bool)
    e = row_errors(o, ref) / u
    e = torch.where(live.to(e.device), e, torch.zeros_like(e))
    n_live = max(int(live.sum()), 1)
    B, H, Sq = e.shape
    pad = (-Sq) % GROUP
    eg = torch.nn.functional.pad(e, (0, pad)).view(B, H, -1, GROUP)
    lg = torch.nn.functional.pad(live.to(e.device).double(), (0, pad)).view(B, H, -1, GROUP).sum(-1).clamp_min(1)
    st = {"worst": e.max().item(), "mean": e.sum().item() / n_live, "group": (eg.sum(-1) / lg).max().item(), "lse": 0.0}
    if lse is not None and ref_lse is not None:
        lv = live.to(ref_lse.device)
        dl = (lse.to(ref_lse.device, torch.float64) - ref_lse).abs() / ref_lse.abs().clamp_min(1.0)
        st["lse"] = torch.where(lv, dl, torch.zeros_like(dl)).max().item() if lv.any() else 0.0
    return st


def check(o, ref, dtype, family, lse=None, ref_lse=None, what=""):
    """Assert the kernel result (o [B,Sq,H,D] in dtype, lse [B,H,Sq] fp32 or None) matches the fp64 reference (ref,
    ref_lse) within the bars of (dtype, family).  Returns the measured statistics."""
    tag = f"{what} [{family} {str(dtype).split('.')[-1]}]"
    assert o.shape == ref.shape, f"{tag}: shape {tuple(o.shape)} vs {tuple(ref.shape)}"
    assert torch.isfinite(o).all(), f"{tag}: non-finite output ({int((~torch.isfinite(o)).sum())} values)"
    if ref_lse is not None:
        empty = torch.isinf(ref_lse) & (ref_lse < 0)
        oe = o.to(ref.device).permute(0, 2, 1, 3)[empty]
        assert (oe == 0).all(), f"{tag}: rows with no visible key are not exactly 0"
        if lse is not None:
            lsed = lse.to(ref_lse.device)
            assert torch.isfinite(lsed[~empty]).all(), f"{tag}: non-finite lse where the reference's is finite"
            assert (lsed[empty] == float("-inf")).all(), f"{tag}: lse of rows with no visible key is not -inf"
    st = measure(o, ref, dtype, lse, ref_lse)
    key = (dtype, family)
    rec = STATS.setdefault(key, {"worst": 0.0, "mean": 0.0, "group": 0.0, "lse": 0.0, "n": 0})
    for name in ("worst", "mean", "group", "lse"):
        rec[name] = max(rec[name], st[name])
    rec["n"] += 1
    worst, mean, group, lse_bar = BARS[key]
    assert st["worst"] <= worst and st["mean"] <= mean and st["group"] <= group and st["lse"] <= lse_bar, (
        f"{tag}: worst row {st['worst']:.2f} u (bar {worst}), mean {st['mean']:.3f} u (bar {mean}), "
        f"16-row group {st['group']:.2f} u (bar {group}), lse {st['lse']:.2e} (bar {lse_bar:.0e})")
    return st

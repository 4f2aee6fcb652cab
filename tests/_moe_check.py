"""The fp64 restatement of the mixture-of-experts decode step (mio_moe_route, mio_moe_up, mio_moe_down; the semantics are stated
in include/mio_hip.h) and what a correct fp32 kernel may differ from it by.  A plain helper module, not a conftest;
tests/test_moe_check.py checks the checker.  Every stage is judged from the very bytes its launch reads: the router from the stored
logits, up from x, the weights and the route, down from the h and the routing weights THE KERNELS WROTE, so a stage carries only
its own error.

Route (route_reference, check_route).  ids, expert_offsets, sorted_rows and row_pos are exactly determined by the stored logits
(NaN -> -inf; a before b iff x_a > x_b, or x_a == x_b and a < b) and are compared for equality.  The weights get an allowance,
derived as tests/_sampling_check.py derives its own; u = 2^-24 is fp32's unit roundoff, u' = 2^-23 one full ulp.
  * The kernel forms p^_e = exp2(fl(fl(x_e - m) fl(log2 e))): the exponent t_e = (x_e - m) log2 e carries three roundings (the
    subtraction, the constant, the product), a relative error gamma3 = 3u / (1 - 3u), which exp2 turns into the relative error
    expm1(|t_e| ln2 gamma3) of its value -- the rounding of the exponent amplified by |x - m| -- and v_exp_f32 adds its stated
    1 ulp:  rho_e = (1 + expm1(|t_e| ln2 gamma3)) (1 + u') - 1.  (+inf counts as the largest finite fp32, so x - m never is
    inf - inf; x_e == m gives exactly 1 in the kernel as here.)
  * Z^ = the sum of the E <= 256 terms p^_e in ANY order, charged a full ulp per add: |Z^ - sum p^| <= gamma'_{E-1} sum p^ with
    gamma'_n = n u' / (1 - n u').  With the terms' own errors:  a_Z = sum_e rho_e p_e / Z + gamma'_{E-1} (1 + max rho), relative.
  * w_j = fl(p^_j / Z^): relative error r_j = (1 + rho_j) (1 + u) / (1 - a_Z) - 1.
  * renormalised: w'_j = fl(w_j / S^), S^ the sum of the k weights (k - 1 adds, a full ulp each, any order):
    r'_j = (1 + r_j) (1 + u) / (1 - (max_i r_i + gamma'_{k-1} (1 + max_i r_i))) - 1.
  * a p below the normal range may be flushed: an absolute 2^-126 per term, which the division by Z >= 1 does not enlarge and the
    renormalisation enlarges by at most 1 / S <= E <= 2^8 (S >= w_max = 1 / Z >= 1 / E): an absolute floor of 2^-117 on every
    weight.
  A row with no finite logit: ids 0 .. k - 1 and weights exactly 0 (sign included).

Up (up_reference).  Per expert, tests/_gemm_check.reference on the gathered rows (x[sorted_rows[p] // k], the expert's weights and
biases): its element bound holds for any summation order, the split of K included.  h is indexed by sorted position.  check_up
holds h to that bound and to the statistical bars of _gemm_check.BARS[(dtype, "t128")], the bars tests/test_gpu_gemm_skinny.py
judges the decode-step GEMM by: measured on a kernel with the same accumulation and epilogue, not on the code under test.

Down (down_reference).  With z_j = h[row_pos[t k + j]] W_e^T + b_e (e = ids[t, j]) and S_j = |h||W_e|^T + |b_e| in fp64:
    y = sum_j w_j z_j + r,     tol = sum_j |w_j| gamma'_{K+1} S_j  +  gamma'_k sum_j |w_j| (|z_j| + gamma'_{K+1} S_j)  +  2u (|a| + |r|)
  * gamma'_{K+1} S_j: the K exact products and the bias as the (K+1)-th term, summed in any order (inside an MFMA, across the
    chunks, across the slices), a full ulp per add as _gemm_check charges it; times |w_j|;
  * the slot sum: one rounding per product w_j z^_j and k - 1 adds, k roundings on a sum of k terms: gamma'_k times the sum of
    the terms' magnitudes (each at most |w_j| (|z_j| + its own bound));
  * the residual add rounds once: 2u (|a| + |r|), a = the slot sum, as _gemm_check writes its own;
  * the final rounding to the 16-bit grid: _gemm_check.element_bound.
No fitted constant.  composed_reference() chains the three for the module test, where the kernel's h may be the other neighbour
of a value whose bound interval holds a rounding boundary (one ulp of such h times |W|, as _gemm_check.reference_mlp) and its
routing weight may differ by the route's allowance (times |z_j|).
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

import _gemm_check as gc

FLT_MAX = float(torch.finfo(torch.float32).max)
U = 2.0 ** -24
U32 = 2.0 ** -23
GAMMA3 = 3 * U / (1 - 3 * U)
LOG2E = 1.4426950408889634
FLOOR = 2.0 ** -117


def _gam(n: int) -> float:
    return n * U32 / (1.0 - n * U32)


@dataclass
class RouteRef:
    ids: torch.Tensor           # int64 [T, k]
    weights: torch.Tensor       # fp64 [T, k]
    allow: torch.Tensor         # fp64 [T, k]: what |kernel weight - weights| may reach
    offsets: torch.Tensor       # int64 [E + 1]
    sorted_rows: torch.Tensor   # int64 [T k]
    row_pos: torch.Tensor       # int64 [T k]
    top_k: int
    num_experts: int


def canon(x: torch.Tensor) -> torch.Tensor:
    """fp64 of the stored logits as the order reads them: NaN -> -inf (+inf stays above every finite value)."""
    x = x.detach().to("cpu", torch.float64).clone()
    x[torch.isnan(x)] = -math.inf
    return x


def order(xc: torch.Tensor) -> torch.Tensor:
    """Expert indices of one row from first to last: a before b iff x_a > x_b, or x_a == x_b and a < b."""
    return torch.sort(-xc, stable=True).indices


def group_rows(ids: torch.Tensor, E: int):
    """(offsets [E + 1], sorted_rows [T k], row_pos [T k]) of ids [T, k]: the routed rows r = t k + j grouped by expert in ascending r."""
    flat = ids.reshape(-1)
    sorted_rows = torch.sort(flat, stable=True).indices
    counts = torch.bincount(flat, minlength=E)
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(counts, 0)])
    row_pos = torch.empty_like(sorted_rows)
    row_pos[sorted_rows] = torch.arange(flat.numel())
    return offsets, sorted_rows, row_pos


def route_reference(logits: torch.Tensor, top_k: int, renormalize: bool) -> RouteRef:
    """The routing of logits [T, E] (any float dtype: the stored values), module docstring."""
    xc = canon(logits)
    T, E = xc.shape
    k = top_k
    ids = torch.zeros(T, k, dtype=torch.int64)
    w = torch.zeros(T, k, dtype=torch.float64)
    allow = torch.zeros(T, k, dtype=torch.float64)
    for t in range(T):
        row = xc[t]
        if not bool(torch.isfinite(row.clamp(max=FLT_MAX)).any()):
            ids[t] = torch.arange(k)
            continue
        o = order(row)[:k]
        v = row.clamp(max=FLT_MAX)               # +inf counts as the largest finite fp32
        m = v.max()
        d = v - m
        p = torch.exp(d)
        p[v == -math.inf] = 0.0
        tt = torch.where(torch.isfinite(d), d.abs() * LOG2E, torch.zeros_like(d))
        rho = torch.where(p >= 2.0 ** -126, (1 + torch.expm1(tt.clamp(max=300.0) * math.log(2.0) * GAMMA3)) * (1 + U32) - 1,
                          torch.zeros_like(p))
        rho[d == 0] = 0.0                        # exactly 1 in the kernel
        Z = p.sum()
        a_Z = float((rho * p).sum() / Z + _gam(E - 1) * (1 + rho.max()))
        wj = p[o] / Z
        r = (1 + rho[o]) * (1 + U) / (1 - a_Z) - 1
        if renormalize:
            S = wj.sum()
            wj = wj / S
            rmax = float(r.max())
            r = (1 + r) * (1 + U) / (1 - (rmax + _gam(k - 1) * (1 + rmax))) - 1
        ids[t], w[t], allow[t] = o, wj, wj * r + FLOOR
    offsets, sorted_rows, row_pos = group_rows(ids, E)
    return RouteRef(ids, w, allow, offsets, sorted_rows, row_pos, k, E)


def check_route(ref: RouteRef, ids, weights, offsets, sorted_rows, row_pos, what: str = "") -> float:
    """Assert a routing (any integer / float tensors of the reference's shapes) against ref; returns the largest weight error in
    units of its allowance."""
    c = lambda t: t.detach().to("cpu")  # noqa: E731
    for name, got, want in (("ids", ids, ref.ids), ("expert_offsets", offsets, ref.offsets), ("sorted_rows", sorted_rows, ref.sorted_rows),
                            ("row_pos", row_pos, ref.row_pos)):
        got = c(got).to(torch.int64).reshape(want.shape)
        if not torch.equal(got, want):
            i = int((got != want).reshape(-1).nonzero()[0])
            raise AssertionError(f"{what}: {name} differs from the reference in {int((got != want).sum())} places, first at flat index "
                                 f"{i}: {int(got.reshape(-1)[i])} vs {int(want.reshape(-1)[i])}")
    w = c(weights).to(torch.float64).reshape(ref.weights.shape)
    assert bool(torch.isfinite(w).all()), f"{what}: non-finite routing weights"
    err = (w - ref.weights).abs()
    dead = ref.allow == 0                       # rows with no finite logit: exactly +0
    if bool(dead.any()):
        assert not bool((w[dead] != 0).any()) and not bool(torch.signbit(w[dead]).any()), f"{what}: a row with no finite logit has a weight that is not +0"
    live = ~dead
    ratio = float((err[live] / ref.allow[live]).max()) if bool(live.any()) else 0.0
    if ratio > 1.0:
        i = int(torch.argmax((err / ref.allow.clamp_min(1e-300)).masked_fill(dead, 0).reshape(-1)))
        t, j = divmod(i, ref.top_k)
        raise AssertionError(f"{what}: weights outside the allowance ({ratio:.3g} x), worst at (token {t}, slot {j}): "
                             f"{w[t, j].item():.9g} vs {ref.weights[t, j].item():.9g}, allowance {ref.allow[t, j].item():.3g}")
    return ratio


def _route_parts(route):
    """(offsets, sorted_rows, row_pos, ids, weights, k, E) as CPU tensors (int64 / fp64) of a RouteRef or an ops.MoERoute."""
    i = lambda t: t.detach().to("cpu", torch.int64)  # noqa: E731
    off = route.offsets if isinstance(route, RouteRef) else route.expert_offsets
    return (i(off), i(route.sorted_rows), i(route.row_pos), i(route.ids), route.weights.detach().to("cpu", torch.float64),
            route.top_k, route.num_experts)


def up_reference(x, route, w_up, act: str, w_gate=None, b_up=None, b_gate=None, device=None) -> gc.Ref:
    """fp64 h [T k, I] by sorted position and its element bound: _gemm_check.reference per expert on the gathered rows."""
    off, srt, _, _, _, k, E = _route_parts(route)
    rows, I, d = srt.numel(), w_up.shape[1], w_up.shape[2]
    dev = torch.device("cpu") if device is None else torch.device(device)
    y = torch.zeros(rows, I, dtype=torch.float64, device=dev)
    tol = torch.zeros_like(y)
    for e in range(E):
        lo, hi = int(off[e]), int(off[e + 1])
        if hi == lo:
            continue
        tok = (srt[lo:hi] // k).to(x.device)
        pick = lambda t: None if t is None else t[e]  # noqa: E731
        r = gc.reference(x[tok], w_up[e], pick(b_up), act, pick(w_gate), pick(b_gate), device=dev)
        y[lo:hi], tol[lo:hi] = r.y, r.tol
    return gc.Ref(y, tol, d)


def check_up(h, ref: gc.Ref, dtype, what: str, guard=None, fill=None) -> dict:
    return gc.check(h, ref, dtype, "moe_up", guard=guard, fill=fill, bars=gc.BARS[(dtype, "t128")], what=what)


def down_reference(h, route, w_down, b_down=None, residual=None, *, weights=None, dh=None, w_allow=None, device=None) -> gc.Ref:
    """fp64 y [T, d] and its bound (module docstring) from h [T k, I] by sorted position and the routing weights (route.weights, or
    `weights`): both as the launch reads them.  dh [T k, I] / w_allow [T, k]: what h and the weights may differ by from what
    the kernel read (composed_reference only)."""
    _, _, pos, ids, w_r, k, E = _route_parts(route)
    dev = torch.device("cpu") if device is None else torch.device(device)
    f = lambda t: None if t is None else t.detach().to(dev, torch.float64)  # noqa: E731
    w = w_r.to(dev) if weights is None else f(weights)
    T = ids.shape[0]
    hf, Wf, bf = f(h), f(w_down), f(b_down)
    d, K = Wf.shape[1], Wf.shape[2]
    gK, gk = _gam(K + 1), _gam(k)
    y = torch.zeros(T, d, dtype=torch.float64, device=dev)
    tol = torch.zeros_like(y)
    mag = torch.zeros_like(y)
    ids_d, pos_d = ids.to(dev), pos.to(dev)
    for e in range(E):
        sel = (ids_d == e).nonzero()                  # [n, 2]: (token, slot)
        if sel.numel() == 0:
            continue
        tt, jj = sel[:, 0], sel[:, 1]
        rows = pos_d[tt * k + jj]
        z = hf[rows] @ Wf[e].t()
        S = hf[rows].abs() @ Wf[e].abs().t()
        if bf is not None:
            z, S = z + bf[e], S + bf[e].abs()
        tz = gK * S
        if dh is not None:
            tz = tz + f(dh)[rows] @ Wf[e].abs().t()
        wj = w[tt, jj][:, None]
        y.index_put_((tt,), wj * z, accumulate=True)
        term = wj.abs() * tz
        if w_allow is not None:
            wa = f(w_allow)[tt, jj][:, None]
            term = term + wa * (z.abs() + tz)
        tol.index_put_((tt,), term, accumulate=True)
        mag.index_put_((tt,), wj.abs() * (z.abs() + tz), accumulate=True)
    tol = tol + gk * mag
    if residual is not None:
        rf = f(residual).reshape(T, d)
        tol = tol + 2.0 * gc.EPS32 * (y.abs() + rf.abs())
        y = y + rf
    return gc.Ref(y, tol, K)


def check_down(y, ref: gc.Ref, dtype, what: str, guard=None, fill=None) -> None:
    gc.check(y, ref, dtype, "moe_down", guard=guard, fill=fill, bars=False, what=what)


def composed_reference(x, logits, top_k: int, renormalize: bool, w_up, w_down, act: str, w_gate=None, b_up=None, b_gate=None,
                       b_down=None, residual=None, dtype=None, device=None):
    """(RouteRef, Ref of y) of the whole step from x and the stored router logits: the fp64 chain softmax -> top-k -> per-expert
    MLP -> weighted sum, with h rounded to the storage dtype as the kernel stores it, under the composed bound."""
    dtype = x.dtype if dtype is None else dtype
    rr = route_reference(logits, top_k, renormalize)
    r1 = up_reference(x, rr, w_up, act, w_gate, b_up, b_gate, device=device)
    h = gc.rn16(r1.y, dtype)
    tie = gc.rn16(r1.y - r1.tol, dtype) != gc.rn16(r1.y + r1.tol, dtype)
    dh = torch.where(tie, gc.ulp16(r1.y.abs() + r1.tol, dtype), torch.zeros_like(h))
    return rr, down_reference(h, rr, w_down, b_down, residual, dh=dh, w_allow=rr.allow, device=device)

"""The fp64 reference of token sampling (mio_sample_tokens; the semantics are stated in include/mio_hip.h), the allowance a
correct fp32 kernel gets against it, and builders of cases whose answer is a single token and a single kept set.  A plain
helper module (numpy only), not a conftest; tests/test_sampling_check.py checks the checker.

Reference.  reference(x, T, k, p, q) restates the semantics on the stored logit values in fp64: NaN -> -inf, +inf -> the
largest finite fp32, the order by lexsort on (index, -x), top-k, top-p over the renormalised top-k set, min-p, and the CDF over
the kept set in ascending token index.

Allowance (derived; no fitted constant).  u = 2^-24 is the unit roundoff of fp32.  The kernel computes
    w^_i = exp2(fl(fl(x_i - m) * c)),  c = fl(fl(log2 e) / T)
so its exponent is t_i (1 + theta), |theta| <= gamma4 = 4u / (1 - 4u): one rounding each for the subtraction, the constant,
the division and the product.  2^(t theta) is a relative error of expm1(|t_i| ln 2 gamma4) -- the rounding of the exponent is
amplified by |t_i| -- and v_exp_f32 adds its stated 1 ulp, 2^-23 relative:
    rho_i = (1 + expm1(|t_i| ln2 gamma4)) (1 + 2^-23) - 1,      w^_i = w_i (1 + rho_i') with |rho_i'| <= rho_i.
A mass is the sum of the w^_i truncated to the kernel's quantum, 2^-40 (64-bit fixed point; a result below the normal range
may also be flushed, 2^-126, far below the quantum).  The sums themselves are integer sums: the kernel's summation depth is 0
and the term depth * 2^-24 * mass of a floating-point tree vanishes; what is left of it is the one conversion of a 60-bit sum
to fp64 where a mass is multiplied by p or u, 2^-50 relative with room to spare.  So for a set S
    allowance(S) = sum_S rho_i w_i + |S| (2^-40 + 2^-126) + 2^-50 mass(S).
The allowance is additive over disjoint sets.  In the draw the kernel looks for C^_{i-1} <= u Z^ < C^_i; with C^_i = C_i + e_i
and Z^ = Z + e_i + e_tail this moves the interval ends by (1 - u) e_i - u e_tail against u Z, at most
max(allowance(prefix), allowance(tail)) <= allowance(S3).  So admissible(u) is every kept token whose CDF interval meets
[u Z - a, u Z + a], a the allowance on Z.
A probability is fl(w^_i / fl(Z^)): its allowance is p_i ((1 + rho_i) (1 + u)^2 / (1 - a / Z) - 1) + 2^-126.

Case builders place p in the middle of a token's mass and u in the middle of a kept token's CDF interval, for tokens that weigh
at least 2^-10 of the set, and ASSERT that the margin to either side is at least 8 times the allowance: a condition on the case,
not a tolerance on the kernel.  Then the reference's kept set and token are the only admissible ones.
"""
from dataclasses import dataclass

import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)
U = 2.0 ** -24
GAMMA4 = 4 * U / (1 - 4 * U)
QUANTUM = 2.0 ** -40 + 2.0 ** -126
LOG2E = 1.4426950408889634
U_MAX = float(np.float32(1.0) - np.float32(2.0 ** -24))   # the largest fp32 below 1
MIN_SHARE = 2.0 ** -10
MARGIN = 8.0


def canon(x):
    """The values the stored logits count as: NaN -> -inf, +inf -> the largest finite fp32."""
    x = np.asarray(x, dtype=np.float64).copy()
    x[np.isnan(x)] = -np.inf
    x[x == np.inf] = FLT_MAX
    return x


def order(xc):
    """Token indices from first to last: i before j iff x_i > x_j, or x_i == x_j and i < j."""
    return np.lexsort((np.arange(xc.size), -xc))


@dataclass
class Ref:
    V: int
    token_first: int          # the first token of the order; -1 for a row with no finite logit
    greedy: bool
    S1: np.ndarray            # kept sets as index arrays in the ORDER (first to last)
    S2: np.ndarray
    S3: np.ndarray            # in ascending token index
    w: np.ndarray             # fp64 [V]
    rho: np.ndarray           # the relative allowance of each w
    Z1: float
    Z: float
    cdf: np.ndarray           # inclusive, over S3 in ascending token index
    probs: np.ndarray         # fp64 [V]
    a_Z1: float               # the allowance on Z1 and on Z
    a_Z: float

    @property
    def kept(self):
        return int(self.S3.size)

    def probs_allowance(self):
        """Per token: what |probs_out - probs| may reach on S3 (0 outside it: those entries are exactly 0)."""
        out = np.zeros(self.V)
        if self.kept and not self.greedy:
            s = self.S3
            out[s] = self.probs[s] * ((1 + self.rho[s]) * (1 + U) ** 2 / (1 - self.a_Z / self.Z) - 1) + 2.0 ** -126
        return out


def mass_allowance(w, rho, idx, depth=0):
    """depth: the summation depth of a floating-point evaluation (the kernel's integer sums: 0)."""
    return float((rho[idx] * w[idx]).sum() + idx.size * QUANTUM + (2.0 ** -50 + depth * U) * w[idx].sum())


def reference(x, T, k=None, p=None, q=None, depth=0):
    """x: the stored logits of one row (any float array); T, p, q: numbers (taken as the fp32 the kernel reads); k: an int.
    None turns a filter off."""
    xc = canon(x)
    V = xc.size
    T = float(np.float32(T))
    zero = np.zeros(V)
    none = np.zeros(0, dtype=np.int64)
    if not np.isfinite(xc).any():
        return Ref(V, -1, False, none, none, none, zero, zero, 0.0, 0.0, np.zeros(0), zero, 0.0, 0.0)
    o = order(xc)
    first = int(o[0])
    if np.isnan(T) or T <= 0:
        w = zero.copy()
        w[first] = 1.0
        s = np.array([first])
        return Ref(V, first, True, s, s, s, w, zero, 1.0, 1.0, np.ones(1), w.copy(), 0.0, 0.0)
    m = xc.max()
    with np.errstate(over="ignore", invalid="ignore"):
        d = xc - m
        w = np.exp(d / T)
        t = np.where(np.isfinite(d), d / T * LOG2E, 0.0)
    w[xc == -np.inf] = 0.0
    # below the normal range the kernel's w is 0 or a denormal: an absolute error under 2^-126, which QUANTUM carries
    rho = np.where(w >= 2.0 ** -126, (1 + np.expm1(np.minimum(np.abs(t), 256.0) * np.log(2.0) * GAMMA4)) * (1 + 2.0 ** -23) - 1, 0.0)
    S1 = o if (k is None or k <= 0 or k >= V) else o[:int(k)]
    Z1 = float(w[S1].sum())
    S2 = S1
    if p is not None:
        pf = float(np.float32(p))
        if not (np.isnan(pf) or pf >= 1):
            before = np.cumsum(w[S1]) - w[S1]
            keep = before < pf * Z1
            keep[0] = True
            S2 = S1[keep]
    S3 = S2
    if q is not None:
        qf = float(np.float32(q))
        if not (np.isnan(qf) or qf <= 0):
            keep = w[S2] >= qf
            keep[0] = True
            S3 = S2[keep]
    S3i = np.sort(S3)
    Z = float(w[S3i].sum())
    probs = zero.copy()
    probs[S3i] = w[S3i] / Z
    return Ref(V, first, False, S1, S2, S3i, w, rho, Z1, Z, np.cumsum(w[S3i]), probs, mass_allowance(w, rho, S1, depth),
               mass_allowance(w, rho, S3i, depth))


def clamp_u(u):
    u = float(np.float32(u))
    if np.isnan(u) or u < 0:
        return 0.0
    return min(u, U_MAX)


def token_of(ref, u):
    """The reference's own draw: the token of S3 with C_i - w_i <= u Z < C_i (the last one should rounding carry past the end)."""
    if ref.token_first < 0:
        return -1
    if ref.greedy:
        return ref.token_first
    j = int(np.searchsorted(ref.cdf, clamp_u(u) * ref.Z, side="right"))
    return int(ref.S3[min(j, ref.kept - 1)])


def admissible(ref, u):
    """The tokens of S3 whose CDF interval [C_i - w_i, C_i) meets [u Z - a, u Z + a], a the allowance on Z."""
    if ref.token_first < 0:
        return np.array([-1])
    if ref.greedy:
        return np.array([ref.token_first])
    x = clamp_u(u) * ref.Z
    lo = ref.cdf - ref.w[ref.S3]
    ok = (lo <= x + ref.a_Z) & (ref.cdf > x - ref.a_Z) & (ref.w[ref.S3] > 0)
    ok[-1] |= bool(x + ref.a_Z >= ref.cdf[-1])    # a search carried past the end returns the last token of S3
    return ref.S3[ok]


# ---- case builders ---------------------------------------------------------------------------------------------------------
def tie_groups(xc, within=None):
    """(first position in the order, size) of every group of equal values among the first `within` tokens of the order."""
    o = order(xc)
    v = xc[o][: (o.size if within is None else within)]
    starts = np.flatnonzero(np.r_[True, v[1:] != v[:-1]])
    return o, starts, np.diff(np.r_[starts, v.size])


def k_inside_ties(x, min_ties=3, which=0):
    """A top-k whose cut falls strictly inside a group of at least min_ties equal logits: at least one of them stays and at
    least one goes.  which picks among the groups (from the top of the order).  None if the row has no such group."""
    xc = canon(x)
    _, starts, sizes = tie_groups(xc)
    big = np.flatnonzero(sizes >= min_ties)
    if big.size == 0:
        return None
    g = big[min(which, big.size - 1)]
    k = int(starts[g] + sizes[g] // 2)          # half of the group (at least one) stays
    assert starts[g] < k < starts[g] + sizes[g]
    return k


def mid_p(x, T, k=None, inside_ties=False, which=0, depth=0):
    """A top-p in the middle of the mass of a token j of the (top-k) set that weighs at least 2^-10 of it:
    p = fp32((before_j + w_j / 2) / Z1), so j is the last token kept.  inside_ties: j sits in a group of at least 3 equal logits
    of that set and is not its last, so the cut falls strictly inside the group.  Asserts the margin; None if no token
    qualifies."""
    ref = reference(x, T, k, depth=depth)
    w = ref.w[ref.S1]
    before = np.cumsum(w) - w
    ok = (w / ref.Z1 >= MIN_SHARE) & (w / 2 > 1.01 * MARGIN * ref.a_Z1)   # the second only bites for deep fp32 sums
    if inside_ties:
        _, starts, sizes = tie_groups(canon(x), ref.S1.size)
        inner = np.zeros(w.size, dtype=bool)
        for s, n in zip(starts, sizes):
            if n >= 3:
                inner[s:s + n - 1] = True
        ok &= inner
    cand = np.flatnonzero(ok)
    if cand.size == 0:
        return None
    j = int(cand[min(which, cand.size - 1)]) if inside_ties else int(cand[(which * 7919 + cand.size // 2) % cand.size])
    p = float(np.float32((before[j] + w[j] / 2) / ref.Z1))
    margin = min(p * ref.Z1 - before[j], before[j] + w[j] - p * ref.Z1)
    assert margin >= MARGIN * ref.a_Z1 and 0 < p < 1, (margin, ref.a_Z1, p)
    got = reference(x, T, k, p)
    assert got.S2.size == j + 1
    return p


def top_p_clear(x, T, k, p):
    """top-p p (any value, not a built one) decides every token of the top-k set with room: the mass before the last token kept
    and the mass before the first one dropped are at least 8 allowances away from p Z1."""
    ref = reference(x, T, k, p)
    if p is None or ref.greedy or ref.token_first < 0:
        return True
    pf = float(np.float32(p))
    if np.isnan(pf) or pf >= 1 or pf <= 0:
        return True
    w = ref.w[ref.S1]
    edges = np.cumsum(w)[ref.S2.size - 2: ref.S2.size] if ref.S2.size > 1 else np.cumsum(w)[:1]
    return bool((np.abs(edges - pf * ref.Z1) >= MARGIN * ref.a_Z1).all())


def min_p_clear(ref, q):
    """min-p q decides every token of S2 with room: no w within 8 allowances of q.  The ties of the maximum weigh exactly 1 in
    the kernel as in the reference (x - m == 0), so q = 1 decides them exactly."""
    qf = float(np.float32(q))
    if ref.greedy or ref.token_first < 0 or np.isnan(qf) or qf <= 0:
        return True
    w, rho = ref.w[ref.S2], ref.rho[ref.S2]
    return bool((np.abs(w - qf) >= MARGIN * (rho * w + 2.0 ** -126))[w != 1.0].all())


def mid_u(ref, which=0):
    """A uniform in the middle of the CDF interval of a kept token that weighs at least 2^-10 of Z, and that token.  Asserts the
    margin."""
    w = ref.w[ref.S3]
    cand = np.flatnonzero((w / ref.Z >= MIN_SHARE) & (w / 2 > 1.01 * MARGIN * ref.a_Z))
    assert cand.size
    j = int(cand[(which * 7919 + cand.size // 3) % cand.size])
    u = float(np.float32((ref.cdf[j] - w[j] / 2) / ref.Z))
    margin = min(u * ref.Z - (ref.cdf[j] - w[j]), ref.cdf[j] - u * ref.Z)
    assert margin >= MARGIN * ref.a_Z and 0 <= u < 1, (margin, ref.a_Z)
    assert token_of(ref, u) == int(ref.S3[j]) and admissible(ref, u).tolist() == [int(ref.S3[j])]
    return u, int(ref.S3[j])


def check_probs(ref, probs):
    """(entries outside S3 that are not exactly 0, entries of S3 outside the allowance, the largest excess ratio)."""
    probs = np.asarray(probs, dtype=np.float64)
    mask = np.zeros(ref.V, dtype=bool)
    mask[ref.S3] = True
    outside = int((probs[~mask] != 0).sum()) + int(np.signbit(probs[~mask]).sum())
    if ref.greedy:
        return outside, int((probs[mask] != 1.0).sum()), 0.0
    allow = ref.probs_allowance()
    err = np.abs(probs - ref.probs)[mask]
    bad = int((err > allow[mask]).sum()) + int(np.isnan(probs).sum())
    return outside, bad, float((err / allow[mask]).max()) if err.size else 0.0

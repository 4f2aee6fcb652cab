"""CPU-only: the checker of tests/_sampling_check.py is itself checked.  A plain fp32 evaluation of the sampling semantics -- the
kernel's operation chain for the weights, masses summed in fp32 in two orders or in the kernel's 2^-40 fixed point -- gives the
reference's token and kept set on every constructed case and probabilities inside the allowance; each of nine planted defects is
caught on at least one constructed case."""
import functools

import numpy as np
import pytest

import _sampling_check as sc

F32 = np.float32
V = 50257


def _bf16(x):
    """Round fp32 values to bf16 (nearest even), returned as fp32."""
    b = np.asarray(x, dtype=F32).view(np.uint32)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(F32)


def _row(seed, n=V):
    return _bf16(np.random.default_rng(seed).standard_normal(n).astype(F32) * F32(2.5))


def _fsum(v, chunk):
    """fp32 sum of v: chunks of `chunk` summed one element after the other, then the chunk sums likewise; and its depth."""
    v = np.asarray(v, dtype=F32)
    if v.size == 0:
        return F32(0), 0
    pad = (-v.size) % chunk
    v = np.concatenate([v, np.zeros(pad, F32)]).reshape(-1, chunk)
    part = np.cumsum(v, axis=1, dtype=F32)[:, -1]
    return np.cumsum(part, dtype=F32)[-1], (chunk - 1) + (part.size - 1)


def evaluate(x, T, k=None, p=None, q=None, u=0.0, mode="fixed", defect=None):
    """(token, kept, probs fp32 [V]) of one row by a plain fp32 evaluation.  mode "fixed": masses in 2^-40 fixed point (exact
    integer sums, as the kernel); ("float", chunk): fp32 sums in chunks.  defect plants one named error."""
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    xc = sc.canon(x)
    if defect == "a NaN logit wins the argmax":
        xc[np.isnan(x)] = np.inf
    idx = np.arange(n)
    if not np.isfinite(np.where(xc == np.inf, 0, xc)).any():
        return -1, 0, np.zeros(n, F32)
    skey = xc
    if defect == "negative logits ordered by magnitude":
        skey = np.where(xc < 0, -1e300 - np.where(np.isfinite(xc), xc, -1e299), xc)
    o = np.lexsort((idx, -skey))
    T32 = F32(T)
    if np.isnan(T32) or T32 <= 0:
        pr = np.zeros(n, F32)
        pr[o[0]] = 1
        return int(o[0]), 1, pr
    m = F32(min(xc.max(), sc.FLT_MAX))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        c = F32(F32(sc.LOG2E) / T32)
        d = np.minimum(xc, sc.FLT_MAX).astype(F32) - m
        t = (d * c).astype(F32)
        w = np.where(np.isnan(t), F32(0), np.exp2(t).astype(F32))
    w = np.where(d == 0, F32(1), np.minimum(w, F32(1))).astype(F32)

    def mass(ws):
        if mode == "fixed":
            return float(np.floor(ws.astype(np.float64) * 2.0 ** 40).sum()) * 2.0 ** -40
        return float(_fsum(ws, mode[1])[0])

    def cum(ws):
        if mode == "fixed":
            return np.cumsum(np.floor(ws.astype(np.float64) * 2.0 ** 40)) * 2.0 ** -40
        return np.cumsum(ws, dtype=F32).astype(np.float64)

    k_on = k is not None and 0 < k < n
    p_on = p is not None and not np.isnan(F32(p)) and F32(p) < 1
    q_on = q is not None and not np.isnan(F32(q)) and F32(q) > 0

    def top_k(s):
        if not k_on:
            return s
        if defect == "ties at the top-k threshold cut by highest index":
            s = s[np.lexsort((-s, -skey[s]))]
        return s[:k]

    def top_p(s):
        if not p_on:
            return s
        ws = w[s]
        z1 = mass(ws)
        inc = cum(ws)
        thr = float(F32(p)) * z1
        keep = inc <= thr if defect == "top-p drops the token that crosses p" else (inc - ws.astype(np.float64)) < thr
        if defect != "the first token dropped when p = 0":
            keep[0] = True
        return s[keep]

    s = top_p(top_k(o)) if defect != "top-p before top-k" else top_k(top_p(o))
    if s.size == 0:
        return -1, 0, np.zeros(n, F32)
    if q_on:
        ratio = w[s] / F32(mass(w[s])) if defect == "min-p against the sum" else w[s]
        keep = ratio >= F32(q)
        keep[0] = True
        s = s[keep]
    s3 = s if defect == "the draw over the descending order" else np.sort(s)
    Z = mass(w[s3])
    C = cum(w[s3])
    uu = float(F32(u)) if defect == "no clamp at the end" else sc.clamp_u(u)
    j = int(np.searchsorted(C, uu * Z, side="right"))
    if defect == "no clamp at the end":
        tok = int(s3[j]) if j < s3.size else n
    else:
        tok = int(s3[min(j, s3.size - 1)])
    pr = np.zeros(n, F32)
    pr[s3] = w[s3] / F32(Z)
    return tok, int(s3.size), pr


def _cases(seed, depth=0):
    """Constructed cases of one logit row: (x, T, k, p, q, u, ref, token)."""
    x = _row(seed)
    out = []
    for T in (0.7, 1.0, 1.5):
        for k in (None, 1, 50, 1000, sc.k_inside_ties(x, 3, seed)):
            ps = [None]
            for inside in (False, True):
                if k != 1:
                    pm = sc.mid_p(x, T, k, inside_ties=inside, which=seed, depth=depth)
                    if pm is not None:
                        ps.append(pm)
            for p in ps:
                for q in (None, 0.05):
                    ref = sc.reference(x, T, k, p, q, depth=depth)
                    if q is not None and not sc.min_p_clear(sc.reference(x, T, k, p, depth=depth), q):
                        continue
                    for which in range(2):
                        u, tok = sc.mid_u(ref, which + seed)
                        out.append((x, T, k, p, q, u, ref, tok))
    return out


@functools.lru_cache(maxsize=None)
def _all_cases(depth=0):
    return {seed: _cases(seed, depth) for seed in range(3)}


@pytest.fixture(scope="module")
def cases():
    return _all_cases(0)


def test_builders_cover_ties_inside_the_cut(cases):
    """The constructed cases include top-k and top-p cuts that fall strictly inside a group of at least 3 equal logits."""
    n_k = n_p = 0
    for cs in cases.values():
        for x, T, k, p, q, u, ref, tok in cs:
            xc = sc.canon(x)
            if k not in (None, 1):
                v = xc[ref.S1[-1]]
                n_k += (xc == v).sum() >= 3 and (xc[sc.order(xc)[k]] == v)
            if p is not None:
                v = xc[ref.S2[-1]]
                in_s1 = xc[ref.S1] == v
                n_p += in_s1.sum() >= 3 and (xc[ref.S2] == v).sum() < in_s1.sum()
    assert n_k >= 10 and n_p >= 10, (n_k, n_p)


@pytest.mark.parametrize("mode", ["fixed", ("float", 64), ("float", 1024)])
def test_plain_fp32_evaluation_lies_inside_the_model(mode):
    """Tokens and kept counts equal the reference's on every constructed case; the probabilities are exactly 0 outside the kept
    set and inside the allowance on it -- for the fixed-point masses with the kernel's summation depth 0, for the fp32 sums
    with theirs (the cases are then built with margins against that allowance)."""
    depth = 0 if mode == "fixed" else _fsum(np.zeros(V, F32), mode[1])[1]
    total = 0
    worst = 0.0
    for seed, cs in _all_cases(depth).items():
        for x, T, k, p, q, u, ref, tok in cs:
            got_tok, got_kept, pr = evaluate(x, T, k, p, q, u, mode=mode)
            assert got_tok == tok and got_kept == ref.kept, (seed, T, k, p, q, u)
            outside, bad, ratio = sc.check_probs(ref, pr)
            assert outside == 0 and bad == 0, (seed, T, k, p, q, outside, bad, ratio)
            worst = max(worst, ratio)
            total += 1
    print(f"{mode}: {total} cases, largest error / allowance {worst:.3f}")
    assert total >= 100


def _special_cases():
    """Cases aimed at single defects, next to the constructed ones."""
    x = _row(11, 4097)
    nan_row = x.copy()
    nan_row[[5, 4000]] = np.nan
    return [
        ("p = 0", x, 1.0, None, 0.0, None, 0.3),
        ("u just below 1", x, 1.0, 50, None, None, float(F32(1) - F32(2.0 ** -24))),
        ("u = 1", x, 1.0, None, None, None, 1.0),
        ("NaN logits, greedy", nan_row, 0.0, None, None, None, 0.5),
        ("NaN logits, sampled", nan_row, 1.0, 3, None, None, 0.5),
        ("k = V - 1", x, 1.0, x.size - 1, None, None, 0.5),
    ]


DEFECTS = [
    "ties at the top-k threshold cut by highest index",
    "top-p before top-k",
    "top-p drops the token that crosses p",
    "min-p against the sum",
    "the draw over the descending order",
    "no clamp at the end",
    "negative logits ordered by magnitude",
    "a NaN logit wins the argmax",
    "the first token dropped when p = 0",
]


def _judge(x, T, k, p, q, u, got):
    """True if (token, kept, probs) passes what the GPU tests ask: token admissible and in S3, kept equal, probs inside."""
    ref = sc.reference(x, T, k, p, q)
    tok, kept, pr = got
    if kept != ref.kept or tok not in sc.admissible(ref, u).tolist():
        return False
    outside, bad, _ = sc.check_probs(ref, pr)
    return outside == 0 and bad == 0


def _defect_cases(cases):
    return [c[:6] for c in cases[0][::2]] + [c[1:] for c in _special_cases()]


def test_sound_evaluation_passes_the_defect_cases(cases):
    for x, T, k, p, q, u in _defect_cases(cases):
        assert _judge(x, T, k, p, q, u, evaluate(x, T, k, p, q, u)), (T, k, p, q, u)


@pytest.mark.parametrize("defect", DEFECTS)
def test_planted_defects_are_caught(cases, defect):
    caught = sum(not _judge(x, T, k, p, q, u, evaluate(x, T, k, p, q, u, defect=defect))
                 for x, T, k, p, q, u in _defect_cases(cases))
    print(f"{defect}: caught on {caught} cases")
    assert caught >= 1, defect


def test_reference_edges():
    """The reference on the rows the semantics single out."""
    none = sc.reference(np.array([np.nan, -np.inf, np.nan]), 1.0)
    assert none.token_first == -1 and none.kept == 0 and not none.probs.any() and sc.token_of(none, 0.5) == -1
    x = np.array([1.0, 3.0, 3.0, -0.0, 0.0, np.inf, np.nan, np.inf])
    g = sc.reference(x, 0.0)
    assert g.greedy and g.token_first == 5 and g.kept == 1 and g.probs[5] == 1
    r = sc.reference(x, 1.0, 2)
    assert sorted(r.S1.tolist()) == [5, 7] and r.Z1 == 2.0          # two +inf: both the largest finite value, w = 1
    assert sc.reference(x, 1.0, None, None, 1.0).S3.tolist() == [5, 7]   # q = 1: only ties of the max
    assert sc.reference(x, 1.0, None, 0.0).S3.tolist() == [5]            # p = 0: the first token
    assert sc.reference(x, 1.0, 8).kept == 8 and sc.reference(x, 1.0, 0).kept == 8 and sc.reference(x, 1.0, None, 1.0).kept == 8
    o = sc.order(sc.canon(x)).tolist()
    assert o == [5, 7, 1, 2, 0, 3, 4, 6]                                  # -0 == +0 by index; NaN last
    y = np.array([0.0, 0.0, 0.0, 0.0])
    r = sc.reference(y, 1.0)
    assert sc.token_of(r, 0.0) == 0 and sc.token_of(r, 1.0) == 3 and sc.token_of(r, -0.5) == 0 and sc.token_of(r, 0.49) == 1
    assert sc.clamp_u(np.nan) == 0.0 and sc.clamp_u(2.0) == sc.U_MAX

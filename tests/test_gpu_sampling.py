"""GPU tests of token sampling (mio_sample_tokens through ops.sample_tokens / sampling_probs / mio.sampling.Sampler), judged
against the fp64 reference of tests/_sampling_check.py.

Constructed cases (p in the middle of a token's mass, u in the middle of a kept token's CDF interval, margins of 8 allowances
asserted on the CPU) have a single admissible answer: token and kept count must EQUAL the reference's, and the probabilities must
be exactly 0 outside the kept set and inside the derived allowance on it.  Edge and random-u cases are judged by membership in
admissible(u) and S3.

Hostile memory: the logits sit in a buffer whose every other element -- in front of the first row, between the rows, behind the
last -- holds the dtype's largest finite value, so a read past a row's V elements would win the argmax (NaN filler would hide
that: NaN counts as -inf).  Outputs start as 0xFF; the gaps of a strided probs_out must keep those bytes.

The logits of the shape sweep are bf16-valued (coarse rows are multiples of 1/4), so one reference per (V, row) serves bf16, fp16
and fp32 alike; test_fp32_full_significand covers keys whose low 16 bits differ."""
import functools

import numpy as np
import pytest
import torch

import _repeat as rp
import _sampling_check as sc

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
PAD = 64  # elements of filler in front of and behind the logits (a multiple of 16 bytes in every dtype)
U_BELOW_1 = float(np.float32(1) - np.float32(2.0 ** -24))


def _ops():
    from mio import ops
    return ops


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def _values(V, rows, seed):
    """[rows, V] fp64 logits that bf16, fp16 and fp32 all hold exactly: odd rows N(0, 2.5^2) rounded to bf16 (ties are frequent
    near the top), even rows rounded to multiples of 1/4 (large tie groups everywhere)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, V, generator=g) * 2.5
    x[0::2] = (x[0::2] * 4).round() / 4
    x = x.to(torch.bfloat16).float()
    x[x.abs() < 2.0 ** -14] = 0.0   # below fp16's normal range: keep the three dtypes on the same values
    assert torch.equal(x.to(torch.float16).float(), x)
    return x.double().numpy()


def _hostile(vals, dtype, ld, shift):
    """vals [B, V] on the device as a [B, V] view with row stride ld inside a buffer filled with the dtype's largest finite
    value; the view's base is 16-byte aligned and lies `shift` bytes into its allocation."""
    B, V = vals.shape
    buf = rp.fresh((2 * PAD + B * ld,), dtype, DEV, shift)
    buf.fill_(torch.finfo(dtype).max)
    x = buf[PAD:].as_strided((B, V), (ld, 1))
    x.copy_(torch.as_tensor(np.ascontiguousarray(vals)).to(dtype))
    assert x.data_ptr() % 16 == 0
    return x


def _param(vals, dtype):
    return None if vals is None else torch.tensor(vals, dtype=dtype, device=DEV)


def _launch(x, T, k, p, q, u, ldp=None, want=("tokens", "kept", "probs")):
    """One raw launch into 0xFF outputs; returns (tokens, kept, probs view, probs buffer with its gaps)."""
    from mio import _lib
    B, V = x.shape
    ldp = V if ldp is None else ldp
    tok = rp.fresh((B,), torch.int64, DEV) if "tokens" in want else None
    kept = rp.fresh((B,), torch.int32, DEV) if "kept" in want else None
    full = rp.fresh((B, ldp), torch.float32, DEV) if "probs" in want else None
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    ld = x.stride(0) if B > 1 else V
    rc = _lib.lib.mio_sample_tokens(x.data_ptr(), ld, T.data_ptr(), ptr(k), ptr(p), ptr(q), ptr(u), ptr(tok), ptr(kept),
                                    ptr(full), ldp, B, V, _ops()._SAMPLE_DTYPES[x.dtype], torch.cuda.current_stream().cuda_stream)
    _lib.check(rc)
    return tok, kept, (None if full is None else full[:, :V]), full


def _gaps_untouched(full, V):
    gap = full[:, V:]
    return gap.numel() == 0 or bool((gap.contiguous().view(torch.uint8) == 0xFF).all())


# ---- cases ---------------------------------------------------------------------------------------------------------------------
class Row:
    """One row's parameters and its reference; exact: the reference's token is the only admissible one."""

    def __init__(self, x, T, k=None, p=None, q=None, u=0.5, exact=False, which=0):
        self.T, self.k, self.p, self.q = T, k, p, q
        self.ref = sc.reference(x, T, k, p, q)
        self.u, self.exact = u, exact
        # every row, built or not, decides its kept set with room (a condition on the case, checked on the CPU)
        assert sc.top_p_clear(x, T, k, p) and (q is None or sc.min_p_clear(sc.reference(x, T, k, p), q)), (T, k, p, q)
        if exact:
            self.u, self.token = sc.mid_u(self.ref, which) if not (self.ref.greedy or self.ref.token_first < 0) else \
                (u, self.ref.token_first)


def _constructed(x, T, k, with_p, q, which=0, inside=False):
    """A row with a single answer: p (if asked) in the middle of a token's mass, q only where it decides every token with room,
    u in the middle of a kept token's interval.  A builder that finds no eligible token leaves that filter off."""
    p = sc.mid_p(x, T, k, inside_ties=inside, which=which) if with_p and k != 1 else None
    if p is None and with_p and inside:
        p = sc.mid_p(x, T, k, which=which)
    if q is not None and not sc.min_p_clear(sc.reference(x, T, k, p), q):
        q = None
    return Row(x, T, k, p, q, exact=True, which=which)


def _tensors(rows):
    f = lambda vs, fill: [fill if v is None else v for v in vs]  # noqa: E731
    return (_param([r.T for r in rows], torch.float32), _param(f([r.k for r in rows], 0), torch.int32),
            _param(f([r.p for r in rows], 1.0), torch.float32), _param(f([r.q for r in rows], 0.0), torch.float32),
            _param([r.u for r in rows], torch.float32))


def _judge(rows, tok, kept, probs, what=""):
    tok = None if tok is None else tok.cpu().tolist()
    kept = None if kept is None else kept.cpu().tolist()
    probs = None if probs is None else probs.cpu().numpy()
    worst = 0.0
    for b, r in enumerate(rows):
        tag = (what, b, r.T, r.k, r.p, r.q, r.u)
        if kept is not None:
            assert kept[b] == r.ref.kept, (tag, kept[b], r.ref.kept)
        if tok is not None:
            if r.exact:
                assert tok[b] == r.token, (tag, tok[b], r.token)
            else:
                assert tok[b] in sc.admissible(r.ref, r.u).tolist() and (tok[b] in r.ref.S3.tolist() or r.ref.kept == 0), \
                    (tag, tok[b], sc.admissible(r.ref, r.u).tolist()[:8])
        if probs is not None:
            outside, bad, ratio = sc.check_probs(r.ref, probs[b])
            assert outside == 0 and bad == 0, (tag, outside, bad, ratio)
            worst = max(worst, ratio)
    return worst


# ---- shapes --------------------------------------------------------------------------------------------------------------------
SHAPES = [1, 7, 64, 257, 4097, 50257, 65536, 65537, 131080, 262144]   # 65536 | 65537: the LDS-residency edge of 16-bit rows


@functools.lru_cache(maxsize=None)
def _shape_case(V):
    """The rows of the shape sweep at one V, shared by the three dtypes: greedy, unfiltered, top-k (cut inside ties where the row
    has them), top-p, min-p, all three, and (short rows) k = V - 1 and a top-p cut inside ties."""
    nrows = 8 if V <= 65537 else 4
    x = _values(V, nrows, seed=V)
    kt = [sc.k_inside_ties(x[b], 3, b) for b in range(nrows)]
    rows = [Row(x[0], 0.0, exact=True),
            _constructed(x[1], 1.0, None, False, None, 1),
            _constructed(x[2], 0.7, kt[2] or min(50, V), True, 0.05, 2, inside=True),
            _constructed(x[3], 1.5, None, True, None, 3)]
    if nrows == 8:
        rows += [_constructed(x[4], 1.0, kt[4] or min(50, V), False, None, 4),
                 _constructed(x[5], 0.7, None, False, 0.05, 5),
                 _constructed(x[6], 1.0, V - 1, True, None, 6, inside=True),
                 _constructed(x[7], 1.5, min(1000, V), True, 0.05, 7)]
    return x, rows


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("V", SHAPES)
def test_shapes(V, dtype):
    """Every vocabulary size, packed rows (ld = V: odd row starts) at shift 0 and padded rows (ld = V + 24) at shift 16, in
    hostile memory; probs_out with and without a row gap."""
    x, rows = _shape_case(V)
    params = _tensors(rows)
    for ld, shift, ldp in ((V, 0, V + 5), (V + 24, 16, V)):
        xd = _hostile(x, DTYPES[dtype], ld, shift)
        tok, kept, probs, full = _launch(xd, *params, ldp=ldp)
        torch.cuda.synchronize()
        worst = _judge(rows, tok, kept, probs, f"V={V} {dtype} ld={ld}")
        assert _gaps_untouched(full, V)
        print(f"V={V} {dtype} ld={ld} shift={shift}: largest probs error / allowance {worst:.3f}")


@pytest.mark.parametrize("V", [4097, 50257])
def test_fp32_full_significand(V):
    """fp32 logits whose keys differ in every digit of the four-level select (the shape sweep's values end in 16 zero bits),
    with exact ties planted at the top-k cut."""
    g = torch.Generator().manual_seed(V)
    x = (torch.randn(4, V, generator=g) * 2.5)
    x[2, torch.randperm(V, generator=g)[:9]] = x[2].topk(40).values[-1]      # nine ties of rank 40
    x = x.double().numpy()
    k2 = sc.k_inside_ties(x[2], 3)
    assert k2 is not None
    rows = [_constructed(x[0], 1.0, 50, True, 0.05, 0), _constructed(x[1], 0.7, None, True, None, 1),
            _constructed(x[2], 1.0, k2, False, None, 2), _constructed(x[3], 1.5, V - 1, False, None, 3)]
    xd = _hostile(x, torch.float32, V, 16)
    tok, kept, probs, _ = _launch(xd, *_tensors(rows))
    torch.cuda.synchronize()
    _judge(rows, tok, kept, probs, f"fp32 V={V}")


# ---- every combination, and the grid -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _combo_rows(V, nlogit):
    x = _values(V, nlogit, seed=1000 + V)
    rows, src = [], []
    i = 0
    for T in (0.7, 1.0, 1.5):
        for k in ("off", 1, 50, V - 1, V):
            for with_p in (False, True):
                for q in (None, 0.05):
                    for j in range(nlogit):
                        xb = x[j]
                        kk = None if k == "off" else k
                        if k == 50 and j % 2 == 0:
                            kk = sc.k_inside_ties(xb, 3, i % 5) or 50
                        rows.append(_constructed(xb, T, kk, with_p, q, i, inside=(i % 2 == 0)))
                        src.append(j)
                        i += 1
    return x, rows, src


def _ties_inside(x, rows, src):
    """How many rows cut strictly inside a group of at least 3 equal logits: by top-k, by top-p."""
    n_k = n_p = 0
    for r, j in zip(rows, src):
        xc = sc.canon(x[j])
        ref = r.ref
        if r.k not in (None, 1) and r.k < xc.size:
            v = xc[ref.S1[-1]]
            n_k += bool((xc == v).sum() >= 3 and xc[sc.order(xc)[r.k]] == v)
        if r.p is not None:
            v = xc[ref.S2[-1]]
            in_s1 = xc[ref.S1] == v
            n_p += bool(in_s1.sum() >= 3 and (xc[ref.S2] == v).sum() < in_s1.sum())
    return n_k, n_p


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_every_combination_on_a_grid_of_300(dtype):
    """B = 300 rows of V = 257: every (T, k, p, q) combination of T in {0.7, 1, 1.5}, k in {off, 1, 50, V - 1, V}, p in {off,
    mid-token}, q in {off, 0.05} on five logit rows; token and kept count equal the reference's."""
    V = 257
    x, rows, src = _combo_rows(V, 5)
    assert len(rows) == 300
    n_k, n_p = _ties_inside(x, rows, src)
    assert n_k >= 10 and n_p >= 10, (n_k, n_p)   # the cut falls strictly inside >= 3 ties, on the CPU side
    xd = _hostile(x[src], DTYPES[dtype], V, 16)
    tok, kept, probs, _ = _launch(xd, *_tensors(rows))
    torch.cuda.synchronize()
    _judge(rows, tok, kept, probs, f"grid {dtype}")


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_every_combination_long_rows(dtype):
    """The same 60 combinations at V = 4097 (several chunks per lane, every wave busy)."""
    V = 4097
    x, rows, src = _combo_rows(V, 1)
    assert len(rows) == 60
    n_k, n_p = _ties_inside(x, rows, src)
    assert n_k >= 3 and n_p >= 3, (n_k, n_p)
    xd = _hostile(x[src], DTYPES[dtype], V + 24, 0)
    tok, kept, probs, _ = _launch(xd, *_tensors(rows))
    torch.cuda.synchronize()
    _judge(rows, tok, kept, probs, f"combos {dtype}")


# ---- greedy ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("V", [257, 65537])
def test_greedy(V, dtype):
    """The first token of the order, bits-exact: on random rows, a row of all-equal logits, the maximum repeated at both ends,
    +0 / -0 ties, T = 0, T < 0 and T = NaN."""
    x = _values(V, 6, seed=7 + V)
    x[1] = 1.25
    top = x[2].max() + 1
    x[2, [0, V - 1]] = top
    x[3] = np.where(np.arange(V) % 2 == 0, -0.0, 0.0)
    x[4, 0] = x[4].max()            # a tie of the maximum with index 0
    rows = [Row(x[b], T, k, p, q, u=0.9, exact=True)
            for b, (T, k, p, q) in enumerate([(0.0, None, None, None), (0.0, 5, 0.5, 0.1), (-1.0, None, None, None),
                                              (float("nan"), 3, None, None), (0.0, None, 0.0, None), (-0.0, 1, None, 1.0)])]
    assert [r.token for r in rows][1:4] == [0, 0, 0]
    xd = _hostile(x, DTYPES[dtype], V, 16)
    tok, kept, probs, _ = _launch(xd, *_tensors(rows))
    torch.cuda.synchronize()
    want = torch.tensor([r.token for r in rows])
    assert torch.equal(tok.cpu(), want) and (kept.cpu() == 1).all()
    onehot = torch.zeros(6, V)
    onehot[torch.arange(6), want] = 1.0
    assert torch.equal(probs.cpu().view(torch.int32), onehot.view(torch.int32))


# ---- edges -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_edges(dtype):
    """Clamped uniforms, the filters' end values, rows with no finite logit, +inf, NaN among finite logits; greedy beside filtered
    beside unfiltered rows in one launch.  Judged by admissible(u) and membership in S3."""
    V = 4097
    base = _values(V, 2, seed=99)
    specs = []  # (values, T, k, p, q, u)
    for u in (0.0, U_BELOW_1, 1.0, -0.5, float("nan")):
        specs.append((base[0], 1.0, None, None, None, u))
        specs.append((base[1], 0.7, 50, None, None, u))
    specs += [(base[0], 1.0, None, 0.0, None, 0.7), (base[1], 1.0, None, 1.0, None, 0.7), (base[0], 1.0, None, None, 1.0, 0.7),
              (base[1], 1.0, 1, None, None, 0.7), (base[0], 1.0, None, -1.0, None, 0.2), (base[0], 1.0, None, None, 2.0, 0.2),
              (base[0], 1.0, -3, float("nan"), float("nan"), 0.2), (base[0], 1.0, V, 1.5, -1.0, 0.2), (base[0], 0.0, 50, 0.5, 0.1, 0.2)]
    ninf = np.full(V, -np.inf)
    nan = np.full(V, np.nan)
    one_inf = base[1].copy()
    one_inf[1234] = np.inf
    two_inf = base[0].copy()
    two_inf[[7, 4000]] = np.inf
    some_nan = base[1].copy()
    some_nan[[0, 5, V - 1]] = np.nan
    some_nan[np.argmax(base[1])] = np.nan
    mixed = np.where(np.arange(V) % 3 == 0, -np.inf, base[0])
    specs += [(ninf, 1.0, 50, 0.9, 0.05, 0.5), (nan, 1.0, None, None, None, 0.5), (ninf, 0.0, None, None, None, 0.5),
              (one_inf, 1.0, None, None, None, 0.9), (one_inf, 0.0, None, None, None, 0.9), (two_inf, 1.0, 5, None, None, 0.7),
              (some_nan, 0.0, None, None, None, 0.5), (some_nan, 1.0, 20, None, None, 0.5), (mixed, 1.0, None, None, None, 0.99),
              (mixed, 1.5, V - 1, 0.99, None, 0.999), (base[0], 1e-30, None, None, None, 0.5), (base[0], 1e30, 10, None, None, 0.5)]
    x = np.stack([s[0] for s in specs])
    rows = [Row(s[0], *s[1:5], u=s[5]) for s in specs]
    xd = _hostile(x, DTYPES[dtype], V, 16)
    tok, kept, probs, _ = _launch(xd, *_tensors(rows))
    torch.cuda.synchronize()
    assert not torch.isnan(probs).any()
    _judge(rows, tok, kept, probs, f"edges {dtype}")
    t = tok.cpu().tolist()
    none = [i for i, r in enumerate(rows) if r.ref.token_first < 0]
    assert len(none) == 3 and all(t[i] == -1 for i in none) and not probs[none].any() and not kept[none].any()
    assert (tok >= -1).all() and (tok < V).all()


def test_null_filters_and_optional_outputs():
    """Null top_k / top_p / min_p pointers turn the filters off; every subset of the outputs gives the same bits."""
    V = 4097
    x = _values(V, 4, seed=5)
    rows = [_constructed(x[b], T, None, False, None, b) for b, T in enumerate((1.0, 0.7, 1.5, 1.0))]
    xd = _hostile(x, torch.bfloat16, V, 16)
    T, k, p, q, u = _tensors(rows)
    tok, kept, probs, _ = _launch(xd, T, None, None, None, u)
    torch.cuda.synchronize()
    _judge(rows, tok, kept, probs, "null filters")
    assert (kept == V).all()
    rows2 = [_constructed(x[b], 1.0, 50, True, 0.05, b) for b in range(4)]
    T, k, p, q, u = _tensors(rows2)
    tok, kept, probs, _ = _launch(xd, T, k, p, q, u)
    for want in (("tokens",), ("kept",), ("probs",), ("tokens", "probs"), ("kept", "probs")):
        t2, k2, p2, _ = _launch(xd, T, k, p, q, u if "tokens" in want else None, want=want)
        torch.cuda.synchronize()
        assert t2 is None or torch.equal(t2, tok)
        assert k2 is None or torch.equal(k2, kept)
        assert p2 is None or torch.equal(p2.view(torch.int32), probs.view(torch.int32))
    _judge(rows2, tok, kept, probs, "all filters")


# ---- random u ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_random_u(dtype):
    """64 rows sharing one logit row, u from a seeded generator: every token lies in admissible(u) and S3; at most one row in 64
    may have more than one admissible token (checked on the CPU, the seed chosen so)."""
    V, B = 50257, 64
    x = _values(V, 2, seed=3)[1]
    ref = sc.reference(x, 0.9, 200, 0.97, 0.001)
    assert sc.top_p_clear(x, 0.9, 200, 0.97) and sc.min_p_clear(sc.reference(x, 0.9, 200, 0.97), 0.001)
    for seed in range(8):
        u = torch.rand(B, generator=torch.Generator().manual_seed(seed)).tolist()
        adm = [sc.admissible(ref, v).tolist() for v in u]
        if sum(len(a) > 1 for a in adm) <= 1:
            break
    else:
        raise AssertionError("no seed meets the cap")
    xd = _hostile(np.broadcast_to(x, (B, V)), DTYPES[dtype], V, 0)
    ops = _ops()
    tok, kept = ops.sample_tokens(xd, 0.9, top_k=200, top_p=0.97, min_p=0.001, u=torch.tensor(u, device=DEV), return_kept=True)
    torch.cuda.synchronize()
    s3 = set(ref.S3.tolist())
    for b, t in enumerate(tok.cpu().tolist()):
        assert t in adm[b] and t in s3, (b, u[b], t, adm[b])
    assert (kept == ref.kept).all()
    assert len(set(tok.cpu().tolist())) > 8    # the draw does move with u


# ---- reruns ------------------------------------------------------------------------------------------------------------------
def _mixed_rows(x, V, frac):
    """Eight rows of mixed kinds -- unfiltered, every filter, greedy -- with p in the middle of a token's mass (so the kept set
    has a single answer) and arbitrary uniforms (b + frac) / 8, judged by admissible(u)."""
    specs = [(1.0, None, False, None), (0.7, 50, True, 0.02), (1.5, None, True, None), (1.0, 1000, False, None),
             (0.0, None, False, None), (1.0, None, False, 0.01), (0.9, 40, True, None), (1.2, V - 1, True, 1e-4)]
    rows = []
    for b, (T, k, with_p, q) in enumerate(specs):
        p = sc.mid_p(x[b], T, k, which=b) if with_p else None
        if q is not None and not sc.min_p_clear(sc.reference(x[b], T, k, p), q):
            q = None
        rows.append(Row(x[b], T, k, p, q, u=(b + frac) / len(specs)))
    return rows


class _Noise(rp.Condition):
    """Matrix products on a second stream, queued before the launches."""
    name = "co-run"

    def start(self):
        self.side = torch.cuda.Stream()
        self.a = torch.randn(8192, 8192, device=DEV, dtype=torch.bfloat16)
        done = torch.cuda.Event()
        done.record(torch.cuda.current_stream())
        self.side.wait_event(done)
        with torch.cuda.stream(self.side):
            for _ in range(64):
                self.a @ self.a

    def stop(self):
        torch.cuda.synchronize()


class _BackToBack(rp.Condition):
    def stop(self):
        torch.cuda.synchronize()


@pytest.mark.parametrize("dtype,V", [("bf16", 50257), ("bf16", 131080), ("fp32", 50257), ("fp16", 4097)])
def test_reruns_are_bit_identical(dtype, V):
    """The same launch 8 times back to back, and 8 times beside matrix products on a second stream: tokens, kept counts and
    probabilities are byte-identical (masses are integer sums: no order of arrival can change them)."""
    B = 8
    x = _values(V, B, seed=17)
    rows = _mixed_rows(x, V, 0.37)
    params = _tensors(rows)

    def make(shift):
        return _hostile(x, DTYPES[dtype], V, shift)

    def written(st, ret):
        return {"tokens": ret[0], "kept": ret[1], "probs": ret[2]}

    res = rp.run_repeats(make, lambda xd: _launch(xd, *params), written, [_BackToBack(), _Noise()],
                         judge=lambda st, ret: _judge(rows, ret[0], ret[1], ret[2], "reruns"))
    res.check(f"sample_tokens {dtype} V={V}")
    assert res.launches == 17


def test_rows_are_independent():
    """Permuting the rows of a batch permutes the outputs and changes nothing else."""
    V, B = 4097, 8
    x = _values(V, B, seed=23)
    rows = _mixed_rows(x, V, 0.5)
    xd = _hostile(x, torch.float16, V, 0)
    params = _tensors(rows)
    tok, kept, probs, _ = _launch(xd, *params)
    perm = torch.tensor([3, 7, 0, 5, 1, 6, 2, 4], device=DEV)
    xp = _hostile(x[perm.cpu().numpy()], torch.float16, V, 0)
    tok2, kept2, probs2, _ = _launch(xp, *[t[perm].contiguous() for t in params])
    torch.cuda.synchronize()
    assert torch.equal(tok2, tok[perm]) and torch.equal(kept2, kept[perm])
    assert torch.equal(probs2.view(torch.int32), probs[perm].view(torch.int32))


# ---- the Python surface --------------------------------------------------------------------------------------------------------
def test_ops_surface():
    """Scalars broadcast, [..., V] flattens, sampling_probs equals return_probs, the generator path is reproducible, and
    refusals raise the documented types."""
    ops = _ops()
    V = 1000
    x = torch.as_tensor(_values(V, 6, seed=31)).to(torch.bfloat16).to(DEV)
    u = torch.rand(6, generator=torch.Generator().manual_seed(1)).to(DEV)
    tok, kept, probs = ops.sample_tokens(x, 0.8, top_k=50, top_p=0.95, u=u, return_kept=True, return_probs=True)
    assert tok.shape == (6,) and tok.dtype == torch.int64 and kept.dtype == torch.int32 and probs.shape == (6, V)
    rows = [Row(x[b].double().cpu().numpy(), 0.8, 50, 0.95, None, u=float(u[b])) for b in range(6)]
    _judge(rows, tok, kept, probs, "ops")
    t3 = ops.sample_tokens(x.view(2, 3, V), 0.8, top_k=50, top_p=0.95, u=u)
    assert t3.shape == (2, 3) and torch.equal(t3.flatten(), tok)
    assert torch.equal(ops.sampling_probs(x, 0.8, top_k=50, top_p=0.95), probs)
    g = torch.Generator(device=DEV).manual_seed(5)
    a = ops.sample_tokens(x, 1.0, generator=g)
    g.manual_seed(5)
    assert torch.equal(a, ops.sample_tokens(x, 1.0, generator=g))
    assert ops.sample_tokens(x, 0.0).tolist() == [int(np.argmax(r)) for r in x.float().cpu().numpy()]   # the lowest index on ties
    # a view with a row stride and an offset base goes through a copy or as it is; the answer is the same
    wide = torch.zeros(6, V + 3, dtype=torch.bfloat16, device=DEV)
    wide[:, 3:] = x
    assert torch.equal(ops.sample_tokens(wide[:, 3:], 0.8, top_k=50, top_p=0.95, u=u), tok)
    with pytest.raises(ValueError, match="stride"):
        ops.sample_tokens(x.t().contiguous().t(), 1.0)
    with pytest.raises(ValueError, match="bf16, fp16 or fp32"):
        ops.sample_tokens(x.double(), 1.0)
    with pytest.raises(ValueError, match="temperature must be a contiguous"):
        ops.sample_tokens(x, torch.ones(5, device=DEV))
    with pytest.raises(ValueError, match="top_k must be a contiguous"):
        ops.sample_tokens(x, 1.0, top_k=torch.ones(6, device=DEV))
    with pytest.raises(ValueError, match="not both"):
        ops.sample_tokens(x, 1.0, u=u, generator=g)
    assert ops.sample_tokens(x[:0], 1.0).shape == (0,)


def test_sampler_steps_and_graph():
    """Two steps with a set_row between them give what ops.sample_tokens gives; one step captured in a graph (one stream, no
    parallel branches) and replayed with new u and new logits contents equals the eager result."""
    from mio.sampling import Sampler
    ops = _ops()
    V, B = 4097, 4
    vals = _values(V, 3 * B, seed=41)
    logits = [torch.as_tensor(vals[i * B:(i + 1) * B]).to(torch.bfloat16).to(DEV) for i in range(3)]
    s = Sampler(B, DEV)
    ptrs = [t.data_ptr() for t in (s.temperature, s.top_k, s.top_p, s.min_p, s.u)]
    s.set_row(0, temperature=0.8, top_k=50, top_p=0.95)
    s.set_row(1, temperature=1.0)
    s.set_row(3, temperature=1.3, min_p=0.05)
    g = torch.Generator(device=DEV).manual_seed(9)
    t0 = s(logits[0], generator=g)
    want = ops.sample_tokens(logits[0], s.temperature.clone(), s.top_k.clone(), s.top_p.clone(), s.min_p.clone(), u=s.u.clone())
    assert torch.equal(t0, want) and int(t0[2]) == int(np.argmax(vals[2]))   # row 2 is still greedy
    s.set_row(2, temperature=0.7, top_k=5)
    s.set_row(0, top_k=0, top_p=1.0)
    t1 = s(logits[1], generator=g)
    want = ops.sample_tokens(logits[1], s.temperature.clone(), s.top_k.clone(), s.top_p.clone(), s.min_p.clone(), u=s.u.clone())
    assert torch.equal(t1, want)
    assert ptrs == [t.data_ptr() for t in (s.temperature, s.top_k, s.top_p, s.min_p, s.u)]
    assert s.top_k.tolist() == [0, 0, 5, 0] and s.top_p[0] == 1.0
    # capture: static logits and uniforms, one launch
    static = logits[0].clone()
    out = None
    ops.sample_tokens(static, s.temperature, s.top_k, s.top_p, s.min_p, u=s.u)   # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.sample_tokens(static, s.temperature, s.top_k, s.top_p, s.min_p, u=s.u)
    for i in (2, 1):
        static.copy_(logits[i])
        s.u.copy_(torch.rand(B, generator=torch.Generator().manual_seed(i)).to(DEV))
        s.set_row(1, temperature=0.5 + i)
        graph.replay()
        torch.cuda.synchronize()
        eager = ops.sample_tokens(logits[i], s.temperature.clone(), s.top_k.clone(), s.top_p.clone(), s.min_p.clone(),
                                  u=s.u.clone())
        assert torch.equal(out, eager), i

"""The mixture-of-experts decode step (ops.moe_route / moe_up / moe_down / moe_mlp, mio.kernels.mlp.MoEMLP) in bf16 and fp16
against the fp64 restatement of tests/_moe_check.py, stage by stage: the router by equality (ids, offsets, sorted rows, inverse)
and by its derived fp32 allowance (weights); up under _gemm_check's element bound and the bars of (dtype, "t128"), as the
decode-step GEMM is judged; down, from the h and the weights the kernels wrote, under the element bound derived in
_moe_check.py.  The shapes are the tables of tests/_moe_cases.py, the smallest that reach each seam; what they reach under the
plan is asserted on the CPU (tests/test_moe_host.py::test_case_tables_reach_the_seams)."""
from types import SimpleNamespace

import pytest
import torch

import _hostile_gemm as hg
import _moe_cases as cs
import _moe_check as mc
import _repeat as rp

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
FILL = -3.0e4  # guard fill: no output of these cases comes near it


def _ops():
    from mio import ops
    return ops


def _lib():
    from mio import _lib
    return _lib.lib


def _rand(shape, dtype, scale=1.0, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(shape, device=DEV, generator=g) * scale).to(dtype)


def _p(t):
    return None if t is None else t.data_ptr()


def _route_of(c, renormalize=True, dtype=torch.float32):
    """The routing of case c, written as logits, and its reference; the ids are the ones asked for."""
    choice = cs.choice_of(c)
    logits = cs.logits_for(choice, c.E, dtype).to(DEV)
    route = _ops().moe_route(logits, c.k, renormalize)
    ref = mc.route_reference(logits, c.k, renormalize)
    assert torch.equal(ref.ids, choice)
    mc.check_route(ref, *route[:5], what=c.what)
    return route, ref


def _strided(value, shape):
    """value as the leading view of a NaN-filled buffer of `shape`: wider rows, more rows per expert."""
    buf = torch.full(shape, float("nan"), dtype=value.dtype, device=DEV)
    idx = tuple(slice(0, n) for n in value.shape)
    buf[idx] = value
    return buf[idx]


def _operands(c, dtype, pads=False):
    """One grouped GEMM's operands: a [rows, K] (x: T rows; h: T k rows), w [E, N, K] scaled by K^-1/2, biases 0.5, residual [T, N].
    pads: x rows 8 elements wider, weight rows 16 wider and one spare row per expert (ldx > K, ldw > K, expert_stride > N ldw)."""
    o = SimpleNamespace()
    o.x = _rand((c.T, c.K), dtype, seed=c.seed)
    o.h = _rand((c.T * c.k, c.K), dtype, seed=c.seed + 1)
    o.w = _rand((c.E, c.N, c.K), dtype, max(c.K, 1) ** -0.5, c.seed + 2)
    o.wg = _rand((c.E, c.N, c.K), dtype, max(c.K, 1) ** -0.5, c.seed + 3) if c.glu else None
    o.b = _rand((c.E, c.N), dtype, 0.5, c.seed + 4) if c.bias else None
    o.bg = _rand((c.E, c.N), dtype, 0.5, c.seed + 5) if (c.bias and c.glu) else None
    o.r = _rand((c.T, c.N), dtype, 1.0, c.seed + 6) if c.res else None
    if pads:
        o.x, o.h = _strided(o.x, (c.T, c.K + 8)), _strided(o.h, (c.T * c.k, c.K + 8))
        o.w = _strided(o.w, (c.E, c.N + 1, c.K + 16))
        o.wg = None if o.wg is None else _strided(o.wg, (c.E, c.N + 1, c.K + 16))
    return o


def _guarded(rows, N, dtype):
    """An output view inside a buffer filled with FILL: one row and 16 columns on either side."""
    buf = torch.full((rows + 2, (N + 32 + 7) // 8 * 8), FILL, dtype=dtype, device=DEV)
    return buf, buf[1:rows + 1, 16:N + 16]


def _run_up(c, dtype, route, o, what=None):
    ops = _ops()
    if c.split is not None:
        assert (ops.moe_up_splits(c.T, c.k, c.E, c.N, c.K, c.act) > 1) == c.split, c.what
    buf, out = _guarded(c.T * c.k, c.N, dtype)
    h = ops.moe_up(o.x, route, o.w, c.act, o.wg, o.b, o.bg, out=out)
    assert h.data_ptr() == out.data_ptr()
    mc.check_up(h, mc.up_reference(o.x, route, o.w, c.act, o.wg, o.b, o.bg, device=DEV), dtype, what or c.what, guard=buf, fill=FILL)
    return h


def _run_down(c, dtype, route, o, what=None):
    ops = _ops()
    if c.split is not None:
        assert (ops.moe_down_splits(c.T, c.k, c.E, c.N, c.K) > 1) == c.split, c.what
    buf, out = _guarded(c.T, c.N, dtype)
    y = ops.moe_down(o.h, route, o.w, o.b, o.r, out=out)
    assert y.data_ptr() == out.data_ptr()
    mc.check_down(y, mc.down_reference(o.h, route, o.w, o.b, o.r, device=DEV), dtype, what or c.what, guard=buf, fill=FILL)
    return y


def _run(c, dtype, side, pads=False):
    route, _ = _route_of(c)
    o = _operands(c, dtype, pads)
    return _run_up(c, dtype, route, o) if side == "up" else _run_down(c, dtype, route, o)


def _side(c):
    return "down" if "down" in c.what else "up"


# ---- router ------------------------------------------------------------------------------------------------------------------------
def _router_logits(T, E, k, dtype, seed):
    """[T, E] inside [T, E + pad] whose padding is 0xFF bytes (NaN).  Ordinary rows are a permutation of i / 16 - 8, i < E: distinct,
    exact in bf16, 1/16 apart -- thousands of allowances between the k-th and the (k+1)-th logit on the stored values.  Then, as T
    allows: all-equal rows, exact ties straddling the k-th place, NaN / +inf / -inf entries, rows with no finite logit."""
    g = torch.Generator().manual_seed(seed)
    x = torch.stack([torch.randperm(E, generator=g).float() / 16 - 8 for _ in range(T)])
    inf, nan = float("inf"), float("nan")
    if T >= 5:
        x[0] = 1.25
        top = x[1].topk(min(k + 1, E)).indices
        x[1, top[k - 1:]] = float(x[1, top[k - 1]])                      # the k-th and the (k+1)-th are equal
        x[2, torch.randperm(E, generator=g)[:max(1, E // 3)]] = nan
        x[2, 0] = inf
        x[2, E - 1] = -inf if E > 1 else x[2, E - 1]
        x[3] = nan
        x[4] = -inf
    if T == 64:
        x[5, :] = x[5, 0]                                         # all equal again, at another value
        x[6, ::2] = inf                                           # several +inf: ties among the largest
        x[7] = nan
        x[7, E - 1] = -3.0                                        # one finite logit among NaN
        grp = torch.randperm(E, generator=g)[:max(2, E // 2)]
        x[8, grp] = 7.5                                           # a group of equal maxima larger than k, or all of it inside
    buf = torch.full((T, E + 24), 0, dtype=dtype, device=DEV)
    buf.view(torch.uint8).fill_(0xFF)
    buf[:, :E] = x.to(dtype).to(DEV)
    return buf[:, :E]


@pytest.mark.parametrize("ldtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("E", cs.ROUTER_E)
def test_router(E, ldtype):
    """Every (k, T, renormalize) of the issue's table at this E and logits dtype: ids, offsets, sorted rows and the inverse by
    equality, weights within the derived allowance; ld > E with NaN bytes behind every row; ties to the lowest index; NaN as -inf;
    rows with no finite logit give ids 0 .. k - 1 and weights +0."""
    ops = _ops()
    worst = 0.0
    for k in cs.router_ks(E):
        for T in cs.ROUTER_T:
            logits = _router_logits(T, E, k, ldtype, seed=E * 100 + k * 10 + T)
            assert T == 1 or logits.stride(0) > E
            for renorm in (True, False):
                route = ops.moe_route(logits, k, renorm)
                what = f"E {E} k {k} T {T} renorm {renorm} {ldtype}"
                worst = max(worst, mc.check_route(mc.route_reference(logits, k, renorm), *route[:5], what=what))
                assert route.top_k == k and route.num_experts == E
                if T >= 5:
                    assert route.ids[0].tolist() == list(range(k)) and route.ids[3].tolist() == list(range(k))
                    assert not bool(route.weights[3:5].view(torch.int32).any())   # exactly +0
    print(f"router E {E} {ldtype}: largest weight error {worst:.3f} allowances")


def test_router_out_buffers():
    """out= writes into the caller's buffers and returns them; a MoERoute made for another shape is refused."""
    ops = _ops()
    logits = _router_logits(5, 8, 2, torch.bfloat16, 1)
    a = ops.moe_route(logits, 2)
    b = ops.moe_route(logits, 2, out=ops.MoERoute(*[torch.full_like(t, -1) for t in a[:5]], 2, 8))
    assert all(torch.equal(x, y) for x, y in zip(a[:5], b[:5])) and b.ids.data_ptr() != a.ids.data_ptr()
    with pytest.raises(ValueError):
        ops.moe_route(logits, 1, out=a)
    # contiguous logits whose first element is off a 16-byte boundary are copied, not refused
    buf = torch.zeros(5 * 8 + 4, dtype=torch.bfloat16, device=DEV)
    off = buf[4:].view(5, 8).copy_(logits)
    assert off.is_contiguous() and off.data_ptr() % 16 == 8
    c = ops.moe_route(off, 2)
    assert all(torch.equal(x, y) for x, y in zip(a[:5], c[:5]))
    with pytest.raises(ValueError):
        ops.moe_route(torch.zeros(65, 8, device=DEV), 2)


# ---- rows per expert ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("i", range(len(cs.ROWS)), ids=[c.what.replace(" ", "-") for c in cs.ROWS])
def test_rows_per_expert(dtype, i):
    """Experts with exactly 0, 1, 15, 16, 17, 33 and 64 rows in one launch (every count of row fragments, full and ragged, in a
    kernel built for four), all 64 tokens on the same experts, and one token among 256 experts: up (SwiGLU, gelu) and down."""
    c = cs.ROWS[i]
    route, ref = _route_of(c)
    if c.routing == "mixed":
        assert tuple(torch.diff(route.expert_offsets).tolist()) == cs.MIXED_COUNTS
    o = _operands(c, dtype)
    _run_up(c, dtype, route, o) if _side(c) == "up" else _run_down(c, dtype, route, o)


# ---- K and N seams -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [1, 15, 72, 1000])
def test_n_edges(dtype, N):
    """One column, part of a 4-column group, a second workgroup of 8 columns, many workgroups; K 8, K 40 (one slice: up finishes in
    its first kernel) and K 1032 (K % 32 == 8; several slices: fp32 partial rows of N % 4 != 0 elements are written and read element
    by element).  Up with silu and SwiGLU, down with a residual.  x rows, weight rows and experts are further apart than they are
    long, the gaps NaN; the outputs are guarded views."""
    for c in cs.N_EDGES:
        if c.N == N:
            _run(c, dtype, _side(c), pads=True)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("act", cs.ACTS)
def test_every_activation(dtype, act):
    """Each activation through the first kernel's epilogue (one slice) and through the reduction's (several), with and without
    biases."""
    calls = [c for c in cs.EVERY_ACTIVATION if c.act == act]
    assert len(calls) == 4
    for c in calls:
        _run(c, dtype, "up")


@pytest.mark.parametrize("dtype", DTYPES)
def test_down_options(dtype):
    """Down at one slice and at several, bias and residual on and off."""
    for c in cs.DOWN_OPTIONS:
        _run(c, dtype, "down", pads=True)


# T -> (a K of one slice, a K of several): the slice is at least 8 T k, in steps of 32 (32, 160 and 512 k); all K % 32 == 8
ONE_EXPERT_K = {1: (40, 328), 17: (40, 488), 64: (40, 1544)}


def _decode_gemm(x, w, b, act, wg=None, bg=None, r=None):
    """ops.gemm_skinny.  One row of N % 8 != 0 columns goes to mio_gemm_skinny itself with ldy = N padded to 8: ops.gemm_skinny
    hands the launch the row stride torch reports for a one-row view, which is N, and the launch refuses it."""
    ops, lib = _ops(), _lib()
    (M, K), N = x.shape, w.shape[0]
    if M > 1 or N % 8 == 0:
        return ops.gemm_skinny(x, w, b, act, wg, bg, residual=r)
    a = ops._ACT[act]
    y = torch.empty(1, (N + 7) // 8 * 8, dtype=x.dtype, device=DEV)
    n = lib.mio_gemm_skinny_workspace_bytes(M, N, K, a)
    ws = torch.empty(n // 4, dtype=torch.float32, device=DEV) if n else None
    rc = lib.mio_gemm_skinny(_p(x), _p(w), _p(b), _p(wg), _p(bg), _p(r), _p(y), _p(ws), M, N, K, K, w.stride(0), y.stride(0),
                             0 if r is None else r.stride(0), a, ops._dtype_id(x), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.mio_last_error().decode()
    return y[:, :N]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", sorted(ONE_EXPERT_K))
def test_one_expert_is_the_decode_gemm(dtype, T):
    """E = 1, top_k = 1: the route is the identity with weights exactly 1.0f, and the split rule is the decode-step GEMM's (one
    expert aimed at, T rows for it).  The grouped GEMMs and the decode-step GEMM run one K loop, one partial store, one slice sum
    and one epilogue, so up equals ops.gemm_skinny on the same x, weight, bias and activation bit for bit (SwiGLU and gelu), and down
    (bias, residual) equals ops.gemm_skinny(..., residual=...) bit for bit: 1.0f * z is z, and 0.f + the one slice's partial is
    the accumulator but for -0, which the bias add turns into +0 on both sides.  N 70 (N % 4 != 0: the partials go element by
    element, the last workgroup is ragged) and N 72; one slice and several, asserted through the host queries."""
    ops = _ops()
    route = ops.moe_route(torch.zeros(T, 1, device=DEV), 1)
    rows = torch.arange(T, dtype=torch.int32, device=DEV)
    assert torch.equal(route.weights.view(torch.int32), torch.ones(T, 1, device=DEV).view(torch.int32))
    assert torch.equal(route.sorted_rows, rows) and torch.equal(route.row_pos.reshape(-1), rows)
    seen = set()
    for N in (70, 72):
        for K in ONE_EXPERT_K[T]:
            x = _rand((T, K), dtype, seed=K + T)
            w, wg = _rand((1, N, K), dtype, K ** -0.5, 1), _rand((1, N, K), dtype, K ** -0.5, 2)
            b, bg = _rand((1, N), dtype, 0.5, 3), _rand((1, N), dtype, 0.5, 4)
            r = _rand((T, (N + 7) // 8 * 8), dtype, 1.0, 5)[:, :N]  # (a residual's row stride is a multiple of 8 elements)
            for act in ("swiglu", "gelu"):
                n = ops.gemm_skinny_splits(T, N, K, act)
                assert ops.moe_up_splits(T, 1, 1, N, K, act) == n, (T, N, K, act)
                seen.add(n > 1)
                glu = act == "swiglu"
                want = _decode_gemm(x, w[0], b[0], act, wg[0] if glu else None, bg[0] if glu else None)
                got = ops.moe_up(x, route, w, act, wg if glu else None, b, bg if glu else None)
                assert torch.equal(got.view(torch.int16), want.view(torch.int16)), f"up T {T} N {N} K {K} {act} {dtype}"
            n = ops.gemm_skinny_splits(T, N, K, "none")
            assert ops.moe_down_splits(T, 1, 1, N, K) == n, (T, N, K)
            seen.add(n > 1)
            want = _decode_gemm(x, w[0], b[0], "none", r=r)
            got = ops.moe_down(x, route, w, b, r)
            assert torch.equal(got.view(torch.int16), want.view(torch.int16)), f"down T {T} N {N} K {K} {dtype}"
    assert seen == {False, True}


@pytest.fixture(scope="module")
def deep_weights():
    """dtype -> (w, w_gate, bias, bias_gate) of the DEEP table, built on first use, shared by its cases (column prefixes) and never
    written."""
    made = {}

    def get(dtype):
        if dtype not in made:
            E, N, K = cs.DEEP[0].E, cs.DEEP[0].N, cs.DEEP_LDW
            made[dtype] = (_rand((E, N, K), dtype, K ** -0.5, 11), _rand((E, N, K), dtype, K ** -0.5, 12),
                           _rand((E, N), dtype, 0.5, 13), _rand((E, N), dtype, 0.5, 14))
        return made[dtype]

    yield get
    made.clear()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("table", ["split", "unsplit"])
def test_deep_pipeline(dtype, table, deep_weights):
    """Slices of 3, 4 and 6 chunks (plain and SwiGLU): the reload of the first register set, the rewrite of an LDS buffer one
    barrier after its last read, the exits at an odd and at an even chunk count.  split: two slices; the K of the table are
    column prefixes of one weight, so ldw > K.  unsplit: one slice of 5 (9) chunks, 64 tokens x 8 slots over 256 experts."""
    if table == "unsplit":
        for c in cs.DEEP_UNSPLIT:
            _run(c, dtype, "up")
        return
    w, wg, b, bg = deep_weights(dtype)
    for c in cs.DEEP:
        route, _ = _route_of(c)
        o = SimpleNamespace(x=_rand((c.T, c.K), dtype, seed=c.seed), w=w[:, :, :c.K], wg=wg[:, :, :c.K] if c.glu else None, b=b,
                            bg=bg if c.glu else None)
        _run_up(c, dtype, route, o)


# ---- hostile memory ------------------------------------------------------------------------------------------------------------------
def _embedded_step(c, dtype, route):
    """The whole step of hostile case c with every operand a view inside a larger buffer (tests/_hostile_gemm.Embedded) and only
    the ACTIVE experts' weights and biases owned: x one guard token either side and 8 columns of padding; the weights 16 columns of
    row padding and one spare row per expert; h one guard row either side (the rows >= T k); y one row and 16 columns either side;
    both workspaces whole."""
    d, I = cs.HOSTILE_DI[c.what]
    T, k, E = c.T, c.k, c.E
    active = torch.zeros(E, dtype=torch.bool)
    active[cs.choice_of(c).reshape(-1)] = True
    assert not bool(active.all())

    def own(shape):
        return torch.arange(int(torch.tensor(shape).prod())).view(shape)[active].reshape(-1)

    def weight(N, K, seed):
        return hg.Embedded(_rand((E, N, K), dtype, K ** -0.5, seed), (E, N + 1, K + 16), seed=seed, own_index=own((E, N, K)))

    def bias(N, seed):
        return hg.Embedded(_rand((E, N), dtype, 0.5, seed), (E + 2, N), (1, 0), seed=seed, own_index=own((E, N)))

    lib, a = _lib(), _ops()._ACT[c.act]
    e = {"x": hg.Embedded(_rand((T, d), dtype, seed=c.seed), (T + 2, d + 8), (1, 0)),
         "w_up": weight(I, d, c.seed + 1), "b_up": bias(I, c.seed + 3), "w_down": weight(d, I, c.seed + 5), "b_down": bias(d, c.seed + 6),
         "res": hg.Embedded(_rand((T, d), dtype, seed=c.seed + 7), (T + 1, d + 8), seed=7),
         "h": hg.Embedded(None, (T * k + 2, (I + 7) // 8 * 8 + 8), (1, 0), out_shape=(T * k, I), dtype=dtype, device=DEV),
         "y": hg.Embedded(None, (T + 2, (d + 32 + 7) // 8 * 8), (1, 16), out_shape=(T, d), dtype=dtype, device=DEV)}
    if c.glu:
        e["w_gate"], e["b_gate"] = weight(I, d, c.seed + 2), bias(I, c.seed + 4)
    for name, n in (("ws_up", lib.mio_moe_up_workspace_bytes(T, k, E, I, d, a)), ("ws_down", lib.mio_moe_down_workspace_bytes(T, k, E, d, I))):
        e[name] = hg.Embedded(None, (max(n // 4, 4),), out_shape=(max(n // 4, 4),), dtype=torch.float32, device=DEV)
        e[name].owned[:] = False  # scratch: pre-filled like padding, and free to change
    return e, d, I, a


def _embedded_launch(c, dtype, route, e, d, I, a):
    """mio_moe_up then mio_moe_down on the embedded operands, through the C ABI so that the workspaces are the test's."""
    lib, ops = _lib(), _ops()
    v = lambda n: e[n].view if n in e else None  # noqa: E731
    st = torch.cuda.current_stream().cuda_stream
    x, wu, wd, h, y, r = v("x"), v("w_up"), v("w_down"), v("h"), v("y"), v("res")
    rc = lib.mio_moe_up(_p(x), _p(wu), _p(v("b_up")), _p(v("w_gate")), _p(v("b_gate")), _p(route.expert_offsets), _p(route.sorted_rows),
                        _p(h), _p(e["ws_up"].buf), c.T, c.k, c.E, I, d, x.stride(0), wu.stride(1), wu.stride(0), h.stride(0), a,
                        ops._dtype_id(x), st)
    assert rc == 0, lib.mio_last_error().decode()
    rc = lib.mio_moe_down(_p(h), _p(wd), _p(v("b_down")), _p(route.ids), _p(route.weights), _p(route.expert_offsets), _p(route.row_pos),
                          _p(r), _p(y), _p(e["ws_down"].buf), c.T, c.k, c.E, d, I, h.stride(0), wd.stride(1), wd.stride(0), y.stride(0),
                          r.stride(0), ops._dtype_id(x), st)
    assert rc == 0, lib.mio_last_error().decode()
    torch.cuda.synchronize()
    return h, y


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("i", range(len(cs.HOSTILE)), ids=[c.what.replace(" ", "-") for c in cs.HOSTILE])
def test_hostile_memory(dtype, i):
    """Nothing a launch does not own reaches its arithmetic: every byte of the weights and biases of the experts no token selected,
    the padding between rows and between experts, the guard tokens around x, the h rows >= T k, both workspaces, the guards around
    h and y -- filled with finite randn (benign), 0xFF bytes (NaN) and +-finfo.max / 8 in turn, at the same addresses.  The benign
    launch is judged against the fp64 references; the other two must equal it bit for bit in h and in y; after each, every byte a
    launch does not own is what it was."""
    c = cs.HOSTILE[i]
    route, _ = _route_of(c)
    e, d, I, a = _embedded_step(c, dtype, route)
    active = torch.zeros(c.E, dtype=torch.bool)
    active[cs.choice_of(c).reshape(-1)] = True
    got = {}
    for fill in hg.FILLS:
        for n, t in e.items():
            t.fill(fill)
            if n[:2] in ("w_", "b_"):  # (fill() puts the whole value back: the idle experts' slices are poisoned here)
                cs.poison_idle(t, active, fill)
                assert cs.idle_is_hostile(t, active, fill), (c.what, n, fill)
        h, y = _embedded_launch(c, dtype, route, e, d, I, a)
        for n, t in e.items():
            if not n.startswith("ws_"):
                assert t.untouched(), f"{c.what} fill {fill}: bytes of {n} that the launch does not own were overwritten"
        got[fill] = (h.clone(), y.clone())
    v = lambda n: e[n].value if n in e else None  # noqa: E731
    hb, yb = got["benign"]
    mc.check_up(hb, mc.up_reference(v("x"), route, v("w_up"), c.act, v("w_gate"), v("b_up"), v("b_gate"), device=DEV), dtype, "hostile " + c.what)
    mc.check_down(yb, mc.down_reference(hb, route, v("w_down"), v("b_down"), v("res"), device=DEV), dtype, "hostile " + c.what)
    for fill in ("nan", "huge"):
        for name, t, base in (("h", got[fill][0], hb), ("y", got[fill][1], yb)):
            diff = t.view(torch.int16) != base.view(torch.int16)
            assert not bool(diff.any()), (f"{c.what} fill {fill}: {int(diff.sum())} elements of {name} differ from the benign launch, "
                                          f"first at (row, column) {tuple(diff.nonzero()[0].tolist())}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_row_independence(dtype):
    """With one token's x row NaN, that token's output row is NaN and every other row is bit-identical to the clean run -- at one
    slice and at several, and with 64 tokens sharing experts."""
    ops = _ops()
    for c in cs.HOSTILE:
        d, I = cs.HOSTILE_DI[c.what]
        route, _ = _route_of(c)
        x = _rand((c.T, d), dtype, seed=c.seed)
        wu, wg, wd = (_rand(s, dtype, s[2] ** -0.5, c.seed + j) for j, s in enumerate([(c.E, I, d), (c.E, I, d), (c.E, d, I)], 1))
        r = _rand((c.T, d), dtype, seed=c.seed + 9)
        run = lambda xx: ops.moe_mlp(xx, route, wu, wd, c.act, wg if c.glu else None, residual=r)  # noqa: E731
        clean = run(x).clone()
        t0 = c.T // 2
        bad = x.clone()
        bad[t0] = float("nan")
        y = run(bad)
        assert bool(torch.isnan(y[t0]).all()), c.what
        keep = torch.arange(c.T, device=DEV) != t0
        assert torch.equal(y[keep].view(torch.int16), clean[keep].view(torch.int16)), c.what
        assert bool(torch.isfinite(clean).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_workspace_hygiene(dtype):
    """Through the C ABI with workspaces of exactly mio_moe_{up,down}_workspace_bytes inside larger NaN buffers, pre-filled with NaN:
    the results are finite and right, and nothing outside the workspaces is touched."""
    lib, ops = _lib(), _ops()
    c = cs.HOSTILE[1]
    d, I = cs.HOSTILE_DI[c.what]
    T, k, E = c.T, c.k, c.E
    a = ops._ACT[c.act]
    route, _ = _route_of(c)
    x = _rand((T, d), dtype, seed=1)
    wu, wg, wd = (_rand(s, dtype, s[2] ** -0.5, 1 + j) for j, s in enumerate([(E, I, d), (E, I, d), (E, d, I)], 1))
    n_up, n_down = lib.mio_moe_up_workspace_bytes(T, k, E, I, d, a), lib.mio_moe_down_workspace_bytes(T, k, E, d, I)
    s_up, s_down = lib.mio_moe_up_splits(T, k, E, I, d, a), lib.mio_moe_down_splits(T, k, E, d, I)
    assert s_up > 1 and n_up == s_up * T * k * I * 4 * 2 and n_down == s_down * T * k * d * 4
    pad = 1024
    bigs = [torch.full((n // 4 + 2 * pad,), float("nan"), dtype=torch.float32, device=DEV) for n in (n_up, n_down)]
    before = [b.view(torch.int32).clone() for b in bigs]
    ws_up, ws_down = (b[pad:pad + n // 4] for b, n in zip(bigs, (n_up, n_down)))
    h = torch.empty(T * k, I, dtype=dtype, device=DEV)
    y = torch.empty(T, d, dtype=dtype, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    assert lib.mio_moe_up(_p(x), _p(wu), None, _p(wg), None, _p(route.expert_offsets), _p(route.sorted_rows), _p(h), _p(ws_up), T, k, E,
                          I, d, d, d, I * d, I, a, ops._dtype_id(x), st) == 0, lib.mio_last_error().decode()
    assert lib.mio_moe_down(_p(h), _p(wd), None, _p(route.ids), _p(route.weights), _p(route.expert_offsets), _p(route.row_pos), None,
                            _p(y), _p(ws_down), T, k, E, d, I, I, I, d * I, d, 0, ops._dtype_id(x), st) == 0, lib.mio_last_error().decode()
    torch.cuda.synchronize()
    mc.check_up(h, mc.up_reference(x, route, wu, c.act, wg, device=DEV), dtype, "workspace up")
    mc.check_down(y, mc.down_reference(h, route, wd, device=DEV), dtype, "workspace down")
    for b, b0 in zip(bigs, before):
        after = b.view(torch.int32)
        assert torch.equal(after[:pad], b0[:pad]) and torch.equal(after[-pad:], b0[-pad:])
    assert bool(torch.isfinite(ws_up).all()) and bool(torch.isfinite(ws_down).all())  # every partial that is read was written


def test_empty_call():
    """T == 0 launches nothing and returns 0: through the C ABI with null pointers, and through the ops with empty tensors."""
    lib, ops = _lib(), _ops()
    assert lib.mio_moe_route(None, 8, None, None, None, None, None, 0, 8, 2, 1, 0, None) == 0
    w = _rand((8, 72, 40), torch.bfloat16)
    assert lib.mio_moe_up(None, _p(w), None, None, None, None, None, None, None, 0, 2, 8, 72, 40, 40, 40, 72 * 40, 72, 0, 0, None) == 0
    assert lib.mio_moe_down(None, _p(w), None, None, None, None, None, None, None, None, 0, 2, 8, 72, 40, 40, 40, 72 * 40, 72, 0, 0, None) == 0
    route = ops.moe_route(torch.empty(0, 8, dtype=torch.bfloat16, device=DEV), 2)
    assert tuple(route.ids.shape) == (0, 2) and route.expert_offsets.tolist() == [0] * 9
    stale = ops.MoERoute(*[torch.full_like(t, -1) for t in route[:5]], 2, 8)   # the caller's buffers: the offsets are zeroed too
    assert ops.moe_route(torch.empty(0, 8, dtype=torch.bfloat16, device=DEV), 2, out=stale).expert_offsets.tolist() == [0] * 9
    y = ops.moe_mlp(torch.empty(0, 40, dtype=torch.bfloat16, device=DEV), route, w, _rand((8, 40, 72), torch.bfloat16), "gelu")
    assert tuple(y.shape) == (0, 40)


# ---- the module --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def moe_modules():
    """(dtype, E, k) -> an MoEMLP with fp32 parameters (so that forward reads cast copies), built on first use."""
    made = {}

    def get(dtype, E, k):
        from mio.kernels.mlp import MoEConfig, MoEMLP
        if (dtype, E, k) not in made:
            torch.manual_seed(E)
            m = MoEMLP(264, 136, E, k, MoEConfig(dtype=dtype)).to(DEV)
            with torch.no_grad():
                m.router.weight.mul_(8.0)  # logits a few units apart
            made[(dtype, E, k)] = m
        return made[(dtype, E, k)]

    yield get
    made.clear()


def _judge_module(m, x, res, dtype, what):
    """m(x, res) against the fp64 chain softmax -> top-k -> per-expert linear -> weighted sum, given the module's own router logits
    (the routing is then the module's by construction: the order is exact on stored values), under the composed bound."""
    y = m(x, res)
    x2 = x.reshape(-1, x.shape[-1])
    logits = torch.cat([m._router_logits(x2[lo:lo + 64], dtype) for lo in range(0, x2.shape[0], 64)])
    cast = lambda p: p.detach().to(dtype)  # noqa: E731
    _, ref = mc.composed_reference(x2, logits, m.top_k, m.config.renormalize, cast(m.w_up), cast(m.w_down), "swiglu", cast(m.w_gate),
                                   residual=None if res is None else res.reshape(x2.shape), device=DEV)
    assert y.shape == x.shape and y.dtype == x.dtype
    mc.check_down(y.reshape(x2.shape), ref, dtype, what)
    return y


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("E,k", [(8, 2), (60, 4)])
@pytest.mark.parametrize("T", [1, 17, 64, 150])
def test_module(dtype, E, k, T, moe_modules):
    """MoEMLP at d 264, I 136: one token, a ragged fragment, a full launch and 150 tokens in three chunks, with a residual."""
    m = moe_modules(dtype, E, k)
    x = _rand((1, T, 264), dtype, seed=T)
    _judge_module(m, x, _rand((1, T, 264), dtype, seed=T + 1), dtype, f"module E {E} k {k} T {T}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_module_sees_in_place_update(dtype, moe_modules):
    """After an in-place update of one expert's w_down the output changes, and is the updated weights' output."""
    from mio.kernels.mlp import MoEConfig, MoEMLP
    torch.manual_seed(3)
    m = MoEMLP(264, 136, 8, 2, MoEConfig(dtype=dtype)).to(DEV)
    x = _rand((17, 264), dtype, seed=5)
    y0 = _judge_module(m, x, None, dtype, "before the update").clone()
    route = _ops().moe_route(m._router_logits(x, dtype), 2)
    e = int(route.ids[0, 0])
    with torch.no_grad():
        m.w_down[e].mul_(-2.0)
    y1 = _judge_module(m, x, None, dtype, "after the update")
    hit = (route.ids == e).any(1)
    assert bool(hit[0]) and not torch.equal(y1[hit], y0[hit])
    assert torch.equal(y1[~hit].view(torch.int16), y0[~hit].view(torch.int16))  # tokens that do not use the expert: the same bits


# ---- graph and reruns --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_graph_replays_under_new_routing(dtype):
    """moe_route + moe_mlp captured on one stream (no parallel branches) after a warm-up on it; the router logits are then
    overwritten in place so that other experts are chosen, and a replay must equal an eager call on the new logits bit for bit:
    the plan consults no device value, and nothing of the routing lives on the host."""
    ops = _ops()
    c = cs.HOSTILE[1]
    d, I = cs.HOSTILE_DI[c.what]
    T, k, E = c.T, c.k, c.E
    x = _rand((T, d), dtype, seed=1)
    wu, wg, wd = (_rand(s, dtype, s[2] ** -0.5, 1 + j) for j, s in enumerate([(E, I, d), (E, I, d), (E, d, I)], 1))
    first = cs.logits_for(cs.choice_of(c), E, dtype).to(DEV)
    second = cs.logits_for((cs.choice_of(c) + 3) % E, E, dtype).to(DEV)
    logits = first.clone()
    route = ops.moe_route(logits, k)
    out = torch.zeros(T, d, dtype=dtype, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up on the capture stream
        ops.moe_mlp(x, ops.moe_route(logits, k, out=route), wu, wd, "swiglu", wg, out=out)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.moe_mlp(x, ops.moe_route(logits, k, out=route), wu, wd, "swiglu", wg, out=out)
    for want in (second, first):
        logits.copy_(want)
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        eager_route = ops.moe_route(want, k)
        eager = ops.moe_mlp(x, eager_route, wu, wd, "swiglu", wg)
        assert torch.equal(route.ids, eager_route.ids) and torch.equal(route.sorted_rows, eager_route.sorted_rows)
        assert torch.equal(out.view(torch.int16), eager.view(torch.int16))
    assert not torch.equal(ops.moe_route(first, k).ids, ops.moe_route(second, k).ids)


class _BackToBack(rp.Condition):
    name = "back-to-back"

    def stop(self):
        torch.cuda.synchronize()


class _BesideMatmuls(rp.Condition):
    """Matrix products queued on a second stream before the first launch: the launches run beside them."""
    name = "beside matrix products"

    def start(self):
        self.side = torch.cuda.Stream()
        self.side.wait_stream(torch.cuda.current_stream())
        a = torch.randn(4096, 4096, device=DEV, dtype=torch.bfloat16)
        with torch.cuda.stream(self.side):
            for _ in range(12):
                a = (a @ a).clamp_(-1, 1)

    def stop(self):
        torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", ["unsplit", "split"])
def test_reruns_are_bit_identical(dtype, which):
    """moe_route, moe_up and moe_down write the same bytes on every launch, back to back and beside matrix products on a second
    stream, at one slice and at several (tests/_repeat.run_repeats)."""
    ops = _ops()
    c = next(c for c in cs.HOSTILE if c.what == which)
    d, I = cs.HOSTILE_DI[c.what]
    T, k, E = c.T, c.k, c.E
    assert (ops.moe_up_splits(T, k, E, I, d, c.act) > 1) == (which == "split")
    src = SimpleNamespace(logits=_router_logits(T, E, k, dtype, 3).contiguous(), x=_rand((T, d), dtype, seed=1),
                          wu=_rand((E, I, d), dtype, d ** -0.5, 2), wg=_rand((E, I, d), dtype, d ** -0.5, 3),
                          wd=_rand((E, d, I), dtype, I ** -0.5, 4), r=_rand((T, d), dtype, seed=5))

    def make(shift):
        return SimpleNamespace(**{n: rp.place(t, shift) for n, t in vars(src).items()})

    def launch(p):
        route = ops.moe_route(p.logits, k)
        h = ops.moe_up(p.x, route, p.wu, c.act, p.wg)
        return route, h, ops.moe_down(h, route, p.wd, residual=p.r)

    def written(p, ret):
        route, h, y = ret
        return {"ids": route.ids, "weights": route.weights, "offsets": route.expert_offsets, "sorted_rows": route.sorted_rows,
                "row_pos": route.row_pos, "h": h, "y": y}

    rp.run_repeats(make, launch, written, [_BackToBack(), _BesideMatmuls()]).check(f"moe {which} {dtype}")

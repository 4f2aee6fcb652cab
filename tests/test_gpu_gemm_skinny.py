"""The decode-step GEMM (ops.gemm_skinny / mio_gemm_skinny, 1 <= M <= 64) in bf16 and fp16 against the fp64 reference of
tests/_gemm_check.py, under the statistical bars of the route these shapes take in ops.gemm_bias_act (t128) -- the element bound
holds for any summation order, the split of K included.  The shapes are the tables of tests/_skinny_cases.py, the smallest that
reach each seam: every count of row fragments, K tails and K below one step and K 0, one slice and several (asserted through
ops.gemm_skinny_splits, so both kernels' epilogues are known to have run), slices of three and more chunks of the kernel's
double-buffered loop (plain and SwiGLU, every count of row fragments), N down to one column and past a workgroup's 64, with and
without partials, every activation, strides of x, w, the residual and the output, operands inside buffers whose other bytes are
finite, NaN and huge in turn (tests/_hostile_gemm.py), the workspace's bounds, determinism and a captured graph.  What the
tables reach under the plan is asserted on the CPU
(tests/test_gemm_skinny_host.py::test_case_tables_reach_the_seams)."""
import pytest
import torch

import _gemm_check as gc
import _hostile_gemm as hg
import _skinny_cases as sk

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
ACTS = sk.ACTS
FILL = -3.0e4  # guard fill: no output of these cases comes near it
NAN = float("nan")


def _ops():
    from mio import ops
    return ops


def _rand(shape, dtype, scale=1.0, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(shape, device=DEV, generator=g) * scale).to(dtype)


def _operands(dtype, M, N, K, bias=True, res=False, seed=0, ldx=None, gate=False, bias_gate=True):
    """The construction of tests/test_gpu_gemm_matrix.py: x ~ N(0, 1) (row stride ldx, in a buffer that ends with the last row),
    w scaled by K^-1/2, bias 0.5."""
    if ldx is None or ldx == K:
        x = _rand((M, K), dtype, seed=seed)
    else:
        buf = torch.empty((M - 1) * ldx + K, dtype=dtype, device=DEV)
        x = buf.as_strided((M, K), (ldx, 1))
        x.copy_(_rand((M, K), dtype, seed=seed))
    w = _rand((N, K), dtype, K ** -0.5, seed + 1)
    b = _rand((N,), dtype, 0.5, seed + 2) if bias else None
    r = _rand((M, N), dtype, 1.0, seed + 3) if res else None
    wg = _rand((N, K), dtype, K ** -0.5, seed + 4) if gate else None
    bg = _rand((N,), dtype, 0.5, seed + 5) if (gate and bias_gate) else None
    return x, w, b, r, wg, bg


def _judge(y, ref, dtype, what, guard=None):
    """gc.check under the bars of (dtype, "t128"); the measured statistics go to gc.STATS as the row (dtype, "skinny")."""
    st = gc.check(y, ref, dtype, "skinny", guard=guard, fill=FILL, bars=gc.BARS[(dtype, "t128")], what=what)
    rec = gc.STATS.setdefault((dtype, "skinny"), {"not_rn": 0.0, "worst": 0.0, "mean": 0.0, "frag": 0.0, "n": 0})
    for name in ("not_rn", "worst", "mean", "frag"):
        rec[name] = max(rec[name], st[name])
    rec["n"] += 1
    return st


def _launch(dtype, c, x, w, b, r, wg, bg):
    """One ops.gemm_skinny call of case c on these operands (any legal strides), the whole output checked; the plan splits K or
    not as the case says."""
    ops = _ops()
    assert (ops.gemm_skinny_splits(c.M, c.N, c.K, c.act) > 1) == c.split, (c.what, ops.gemm_skinny_splits(c.M, c.N, c.K, c.act))
    kw = {}
    if r is not None:
        kw["residual"] = r
        if c.ldr is not None:  # the residual as a view of wider rows
            wide = torch.full((c.M, c.ldr), 7.0, dtype=dtype, device=DEV)
            wide[:, :c.N] = r
            kw["residual"] = wide[:, :c.N]
    if c.glu:
        kw.update(w_gate=wg, bias_gate=bg)
    buf = None
    if c.guard:  # the output as a view inside a buffer filled with FILL: one row and 16 columns on either side
        buf = torch.full((c.M + 2, (c.N + 32 + 7) // 8 * 8), FILL, dtype=dtype, device=DEV)  # (row stride a multiple of 8)
        kw["out"] = buf[1:c.M + 1, 16:c.N + 16]
    y = ops.gemm_skinny(x, w, b, c.act, **kw)
    _judge(y, gc.reference(x, w, b, c.act, wg, bg, r, device=DEV), dtype, c.what, guard=buf)
    return y


def _skinny(dtype, c):
    """Case c on operands of its own."""
    return _launch(dtype, c, *_operands(dtype, c.M, c.N, c.K, c.bias, c.res, c.seed, c.ldx, c.glu, c.bias_gate))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M", [c.M for c in sk.ROW_FRAGMENTS])
def test_row_fragments(dtype, M):
    """1 .. 4 row fragments, full and ragged; x is a buffer that ends with its last row."""
    for c in sk.ROW_FRAGMENTS:
        if c.M == M:
            _skinny(dtype, c)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,K,bias,split", [(c.M, c.N, c.K, c.bias, c.split) for c in sk.K_TAILS_AND_SPLITS])
def test_k_tails_and_splits(dtype, M, N, K, bias, split):
    """K below one step, K % 32 != 0 behind many steps, and the split: K >= 1024 runs both launches, K <= 40 one."""
    for c in sk.K_TAILS_AND_SPLITS:
        if (c.M, c.N, c.K, c.bias, c.split) == (M, N, K, bias, split):
            _skinny(dtype, c)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [c.N for c in sk.N_EDGES])
def test_n_edges(dtype, N):
    """One column, part of a 4-column group, part of a 16-row weight fragment, more than one workgroup, through the first
    kernel's epilogue: K 264 is one slice, so no partials are written (test_n_edges_split runs these edges with partials).  The
    output is a guarded view whose rows are a multiple of 8 elements apart."""
    for c in sk.N_EDGES:
        if c.N == N:
            _skinny(dtype, c)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("act", ["silu", "swiglu"])
def test_n_edges_split(dtype, act):
    """The same edges with several slices: fp32 partials in rows of N % 4 != 0 elements, which both kernels then write and read
    element by element instead of 16 bytes at a time -- N 1, part of a fragment, one short of a workgroup's 64 columns, a second
    workgroup of 7 columns, many workgroups.  The output is a guarded view."""
    for c in sk.N_EDGES_SPLIT:
        if c.act == act:
            assert c.N % 4 != 0 and c.split
            _skinny(dtype, c)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K,split", [(40, False), (1032, True)])
@pytest.mark.parametrize("act", ACTS)
def test_every_activation(dtype, act, K, split):
    """Each activation through the first kernel's epilogue (one slice) and through the reduction's (several): with bias and a
    residual, and with neither; SwiGLU with and without the gate's bias."""
    calls = [c for c in sk.EVERY_ACTIVATION if (c.act, c.K, c.split) == (act, K, split)]
    assert len(calls) == (3 if act == "swiglu" else 2)
    for c in calls:
        _skinny(dtype, c)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K,split", [(c.K, c.split) for c in sk.STRIDES])
def test_strides(dtype, K, split):
    """x rows K + 8 apart, the output a guarded view (one row and 16 columns either side), the residual rows wider than N."""
    for c in sk.STRIDES:
        if (c.K, c.split) == (K, split):
            _skinny(dtype, c)


# ---- three and more chunks per slice -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def deep_weights():
    """(dtype, N, K) -> (w, w_gate, bias, bias_gate): one weight pair per dtype and table, built on first use, shared by the cases
    (which take column prefixes of it) and never written."""
    made = {}

    def get(dtype, N, K):
        if (dtype, N, K) not in made:
            made[(dtype, N, K)] = (_rand((N, K), dtype, K ** -0.5, 11), _rand((N, K), dtype, K ** -0.5, 12),
                                   _rand((N,), dtype, 0.5, 13), _rand((N,), dtype, 0.5, 14))
        return made[(dtype, N, K)]

    yield get
    made.clear()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("table", ["unsplit", "split"])
def test_deep_pipeline(dtype, table, deep_weights):
    """Slices of 3, 4 and 5 chunks: the reload of the first register set, the rewrite of an LDS buffer one barrier after its
    last read, and the exits at an odd and at an even chunk count, for plain (gelu, bias, residual) and SwiGLU (both biases,
    residual) at every count of row fragments.  unsplit: N 32776, one slice whatever the split aims for.  split: N 8200, four
    slices of unequal chunk counts.  The K of a table are column prefixes of one weight, so ldw != K in all but the longest."""
    cases = sk.DEEP_UNSPLIT if table == "unsplit" else sk.DEEP_SPLIT
    N, ldw = cases[0].N, max(c.K for c in cases)
    w, wg, b, bg = deep_weights(dtype, N, ldw)
    for c in cases:
        assert c.N == N and c.res and c.bias and c.bias_gate
        x = _rand((c.M, c.K), dtype, seed=c.seed)
        r = _rand((c.M, N), dtype, 1.0, c.seed + 3)
        _launch(dtype, c, x, w[:, :c.K], b, r, wg[:, :c.K] if c.glu else None, bg if c.glu else None)


@pytest.mark.parametrize("dtype", DTYPES)
def test_swiglu_fragments(dtype):
    """SwiGLU (two accumulators per row fragment: the instances with the most registers) at 1 .. 4 row fragments, through the
    first kernel's epilogue and through the reduction's, with both biases and the residual and with none of them."""
    assert {c.mf for c in sk.SWIGLU_FRAGMENTS} == {1, 2, 3, 4}
    for c in sk.SWIGLU_FRAGMENTS:
        _skinny(dtype, c)


def _poisoned(dtype, c, ldw, ldw_gate):
    """Case c with every operand a view inside a larger buffer (tests/_hostile_gemm.Embedded): x is the first M rows and K columns
    of [64, ldx], w and w_gate the first K columns of [N + 2, ldw] behind one guard row, the residual the first N columns of
    [M + 1, ldr], the biases 8 elements into [N + 16], the output one row and 16 columns into its buffer.  Returns {name: Embedded}."""
    x, w, b, r, wg, bg = _operands(dtype, c.M, c.N, c.K, c.bias, c.res, c.seed, None, c.glu, c.bias_gate)
    e = {"x": hg.Embedded(x, (64, c.ldx)), "w": hg.Embedded(w, (c.N + 2, ldw), (1, 0), seed=1),
         "r": hg.Embedded(r, (c.M + 1, c.ldr), seed=2),
         "y": hg.Embedded(None, (c.M + 2, (c.N + 32 + 7) // 8 * 8), (1, 16), out_shape=(c.M, c.N), dtype=dtype, device=DEV)}
    if b is not None:
        e["b"] = hg.Embedded(b, (c.N + 16,), (8,), seed=3)
    if c.glu:
        e["wg"] = hg.Embedded(wg, (c.N + 2, ldw_gate), (1, 0), seed=4)
        if bg is not None:
            e["bg"] = hg.Embedded(bg, (c.N + 16,), (8,), seed=5)
    return e


def _poisoned_launch(e, c, out=True):
    v = lambda n: e[n].view if n in e else None  # noqa: E731
    return _ops().gemm_skinny(v("x"), v("w"), v("b"), c.act, w_gate=v("wg"), bias_gate=v("bg"), residual=v("r"),
                              out=v("y") if out else None)


@pytest.mark.parametrize("dtype", DTYPES)
def test_poisoned_paddings(dtype):
    """Nothing next to the operands reaches the arithmetic: x columns K .. ldx and x rows M .. 63 (the rows the kernel pads the
    last fragment with), w and w_gate columns K .. ldw and the rows around them, residual columns N .. ldr and the row behind
    it, the elements around the biases and the output's guard hold, in three launches at the same addresses, finite randn
    (benign), NaN (0xFF bytes) and +-finfo.max / 8 (huge: fmaxf and v_max drop a NaN operand, a huge one they keep), with one
    slice and with several (whose last ends in a step of 8 k), at M 37 and M 5, plain and SwiGLU.  The benign launch is judged
    against the fp64 reference; the NaN and the huge launch must equal it bit for bit; after each, every byte the launch does
    not own is what it was."""
    ops = _ops()
    for c in sk.POISONED:
        ldw = c.K + sk.POISONED_LDW_PAD
        e = _poisoned(dtype, c, ldw, ldw)
        for n in ("x", "w", "r") + (("wg",) if c.glu else ()):  # the views go to the launch as they are: no copy drops the poison
            t = e[n].view
            assert ops._rows16(t) is t and not t.is_contiguous()
        assert (ops.gemm_skinny_splits(c.M, c.N, c.K, c.act) > 1) == c.split, c.what
        got = {}
        for fill in hg.FILLS:
            for t in e.values():
                t.fill(fill)
            y = _poisoned_launch(e, c)
            torch.cuda.synchronize()
            assert y.data_ptr() == e["y"].view.data_ptr()
            for n, t in e.items():
                assert t.untouched(), f"{c.what} fill {fill}: bytes of {n} that the launch does not own were overwritten"
            got[fill] = y.clone()
        v = lambda n: e[n].value if n in e else None  # noqa: E731
        _judge(got["benign"], gc.reference(v("x"), v("w"), v("b"), c.act, v("wg"), v("bg"), v("r"), device=DEV), dtype,
               "poisoned " + c.what)
        for fill in ("nan", "huge"):
            d = got[fill].view(torch.int16) != got["benign"].view(torch.int16)
            assert not bool(d.any()), (f"{c.what} fill {fill}: {int(d.sum())} output elements differ from the benign launch, "
                                       f"first at (row, column) {tuple(d.nonzero()[0].tolist())}")
    # w and w_gate at different row strides: the kernel has one ldw, so ops.gemm_skinny hands it contiguous copies of both
    c = [c for c in sk.POISONED if c.glu and c.split][0]
    e = _poisoned(dtype, c, c.K + 16, c.K + 8)
    for t in e.values():
        t.fill("nan")
    assert e["w"].view.stride(0) != e["wg"].view.stride(0)
    y = _poisoned_launch(e, c, out=False)
    v = lambda n: e[n].value if n in e else None  # noqa: E731
    _judge(y, gc.reference(v("x"), v("w"), v("b"), c.act, v("wg"), v("bg"), v("r"), device=DEV), dtype, "two weight strides " + c.what)


@pytest.mark.parametrize("dtype", DTYPES)
def test_k_zero(dtype):
    """Through the C ABI: K 0 is an empty sum, y = act(bias) (+ residual) [SwiGLU: silu(bias_gate) * bias], from the first
    kernel's epilogue with no chunk run.  x and w are NaN-filled and never read.  gc.reference does not take an [M, 0] x (it
    reshapes to (-1, K)), so the same formula is evaluated here: the pre-activation value is the bias, its bound that of a sum
    of one term, and everything behind it is gc._finish as in gc.reference."""
    from mio import _lib
    ops, lib = _ops(), _lib.lib
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    for c in sk.K_ZERO:
        M, N, a = c.M, c.N, ops._ACT[c.act]
        assert c.K == 0 and lib.mio_gemm_skinny_splits(M, N, 0, a) == 1 and lib.mio_gemm_skinny_workspace_bytes(M, N, 0, a) == 0
        _, _, b, r, _, bg = _operands(dtype, M, N, 8, c.bias, c.res, c.seed, None, c.glu, c.bias_gate)
        x, w = (torch.full((rows, 8), NAN, dtype=dtype, device=DEV) for rows in (M, N))
        wg = torch.full((N, 8), NAN, dtype=dtype, device=DEV) if c.glu else None
        y = torch.full((M, N), FILL, dtype=dtype, device=DEV)
        rc = lib.mio_gemm_skinny(p(x), p(w), p(b), p(wg), p(bg), p(r), p(y), None, M, N, 0, 8, 8, N, N, a, ops._dtype_id(x),
                                 torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.mio_last_error().decode()
        torch.cuda.synchronize()
        f = lambda t: t.to(torch.float64).expand(M, N)  # noqa: E731
        gam = gc._gamma(1)
        zg, tzg = (f(bg), gam * f(bg).abs()) if c.glu else (None, None)
        ref = gc.Ref(*gc._finish(f(b), gam * f(b).abs(), c.act, zg, tzg, None, r.to(torch.float64)), 0)
        _judge(y, ref, dtype, c.what)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("act", ["none", "swiglu"])
def test_workspace_hygiene(dtype, act):
    """Through the C ABI: a workspace of exactly mio_gemm_skinny_workspace_bytes, pre-filled with NaN, inside a larger NaN buffer.
    The output is finite and correct, and no byte outside the workspace changes."""
    from mio import _lib
    ops, lib = _ops(), _lib.lib
    (c,) = [c for c in sk.WORKSPACE if c.act == act]
    M, N, K = c.M, c.N, c.K
    a = ops._ACT[act]
    gate = act == "swiglu"
    x, w, b, r, wg, bg = _operands(dtype, M, N, K, res=True, gate=gate, seed=c.seed)
    nbytes = lib.mio_gemm_skinny_workspace_bytes(M, N, K, a)
    splits = lib.mio_gemm_skinny_splits(M, N, K, a)
    assert splits > 1 and nbytes == splits * M * N * 4 * (2 if gate else 1)
    pad = 1024  # floats either side
    big = torch.full((nbytes // 4 + 2 * pad,), float("nan"), dtype=torch.float32, device=DEV)
    before = big.view(torch.int32).clone()
    ws = big[pad:pad + nbytes // 4]
    y = torch.empty(M, N, dtype=dtype, device=DEV)
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    rc = lib.mio_gemm_skinny(p(x), p(w), p(b), p(wg), p(bg), p(r), p(y), p(ws), M, N, K, K, K, N, N, a, ops._dtype_id(x),
                             torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.mio_last_error().decode()
    torch.cuda.synchronize()
    _judge(y, gc.reference(x, w, b, act, wg, bg, r, device=DEV), dtype, f"ws {act}")
    after = big.view(torch.int32)
    assert torch.equal(after[:pad], before[:pad]) and torch.equal(after[-pad:], before[-pad:])
    assert bool(torch.isfinite(ws).all())  # every partial the reduction reads was written


@pytest.mark.parametrize("dtype", DTYPES)
def test_deterministic_and_graph(dtype):
    """Two calls with the same inputs give the same bytes (no atomics, no arrival order) -- at two chunks per slice and at slices
    of three and four -- and a call captured in a graph -- one stream, no parallel branches -- and replayed once gives the eager
    bytes: the launch neither allocates nor synchronises beyond the workspace ops.gemm_skinny takes from torch's allocator."""
    ops = _ops()
    for c in sk.DETERMINISTIC:
        x, w, b, r, _, _ = _operands(dtype, c.M, c.N, c.K, res=True, seed=c.seed)
        assert ops.gemm_skinny_splits(c.M, c.N, c.K, c.act) > 1
        y1 = ops.gemm_skinny(x, w, b, c.act, residual=r)
        y2 = ops.gemm_skinny(x, w, b, c.act, residual=r)
        torch.cuda.synchronize()
        assert torch.equal(y1.view(torch.int16), y2.view(torch.int16)), c.what
    c = sk.DETERMINISTIC[0]
    x, w, b, r, _, _ = _operands(dtype, c.M, c.N, c.K, res=True, seed=c.seed)
    y1 = ops.gemm_skinny(x, w, b, "gelu", residual=r)
    out = torch.zeros_like(y1)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.gemm_skinny(x, w, b, "gelu", residual=r, out=out)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    out.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.gemm_skinny(x, w, b, "gelu", residual=r, out=out)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), y1.view(torch.int16))

"""The decode-step GEMM on weight-only FP8 (ops.gemm_skinny_w8 / mio_gemm_skinny_w8, 1 <= M <= 64; e4m3fn weight bytes, one fp32
scale per output column) and its quantiser (ops.quantize_weight_w8) in bf16 and fp16, against the fp64 reference of
tests/_w8_check.py evaluated on the very bytes and scales the kernel reads.  The shapes are the tables of tests/_w8_cases.py, the
smallest that reach each seam; what they reach under the plan is asserted on the CPU
(tests/test_gemm_skinny_w8_host.py::test_case_tables_reach_the_seams).

The scales make a misplaced scale fail: s[n] differs on every column and is no power of two, the gate's scales differ from the
up weight's, and the ZERO_SCALE cases carry zeros in a few columns."""
import pytest
import torch

import _hostile_gemm as hg
import _w8_cases as wc
import _w8_check as w8c

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
FP8 = torch.float8_e4m3fn
FILL = -3.0e4  # guard fill: no output of these cases comes near it
NAN = float("nan")


def _ops():
    from mio import ops
    return ops


def _rand(shape, dtype, scale=1.0, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(shape, device=DEV, generator=g) * scale).to(dtype)


def _bytes(rows, K, seed, ld=None, pad=0x7f):
    """[rows, K] e4m3fn spread over the format's range (N(0, 64^2) clamped to +-448), as a view of rows ld bytes apart whose
    padding columns hold `pad` (0x7f: NaN)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    q = (torch.randn(rows, K, device=DEV, generator=g) * 64.0).clamp(-448.0, 448.0).to(FP8)
    if ld is None or ld == K:
        return q
    buf = torch.full((rows, ld), pad, dtype=torch.uint8, device=DEV).view(FP8)
    buf[:, :K] = q
    return buf[:, :K]


def _scales(rows, K, phase, zero=False):
    """fp32 [rows]: K^-1/2 / 64 (so that s q is about N(0, 1 / K)) times a factor in [1, 1.37) that differs on every column and
    is no power of two; `phase` shifts the sequence (the gate's differs from the up weight's)."""
    n = torch.arange(rows, device=DEV, dtype=torch.float64)
    s = (max(K, 1) ** -0.5 / 64.0) * (1.0 + 0.37 * torch.frac((n + phase) * 0.6180339887))
    s = s.to(torch.float32)
    if zero:
        s[3:6] = 0.0
    return s


def _operands(dtype, c, ldx=None):
    """x ~ N(0, 1) (row stride ldx, in a buffer that ends with the last row), the weights' bytes and scales, bias 0.5, residual."""
    K = c.K
    if ldx is None or ldx == K:
        x = _rand((c.M, K), dtype, seed=c.seed)
    else:
        buf = torch.empty((c.M - 1) * ldx + K, dtype=dtype, device=DEV)
        x = buf.as_strided((c.M, K), (ldx, 1))
        x.copy_(_rand((c.M, K), dtype, seed=c.seed))
    rows = c.rows or c.N
    q, s = _bytes(rows, K, c.seed + 1, c.ldw)[:c.N], _scales(rows, K, 0.0, c.zero_scale)[:c.N]
    b = _rand((c.N,), dtype, 0.5, c.seed + 2) if c.bias else None
    r = _rand((c.M, c.N), dtype, 1.0, c.seed + 3) if c.res else None
    qg = _bytes(rows, K, c.seed + 4, c.ldw)[:c.N] if c.glu else None
    sg = _scales(rows, K, 0.25, c.zero_scale)[:c.N] * 1.23 if c.glu else None
    bg = _rand((c.N,), dtype, 0.5, c.seed + 5) if (c.glu and c.bias_gate) else None
    return x, q, s, b, r, qg, sg, bg


def _launch(dtype, c, x, q, s, b, r, qg, sg, bg):
    """One ops.gemm_skinny_w8 call of case c on these operands (any legal strides), the whole output checked; the plan splits K
    or not as the case says."""
    ops = _ops()
    assert (ops.gemm_skinny_w8_splits(c.M, c.N, c.K, c.act) > 1) == c.split, (c.what, ops.gemm_skinny_w8_splits(c.M, c.N, c.K, c.act))
    kw = {}
    if r is not None:
        kw["residual"] = r
        if c.ldr is not None:  # the residual as a view of wider rows
            wide = torch.full((c.M, c.ldr), 7.0, dtype=dtype, device=DEV)
            wide[:, :c.N] = r
            kw["residual"] = wide[:, :c.N]
    if c.glu:
        kw.update(w8_gate=qg, w_scale_gate=sg, bias_gate=bg)
    buf = None
    if c.guard:  # the output as a view inside a buffer filled with FILL: one row and 16 columns on either side
        buf = torch.full((c.M + 2, (c.N + 32 + 7) // 8 * 8), FILL, dtype=dtype, device=DEV)
        kw["out"] = buf[1:c.M + 1, 16:c.N + 16]
    y = ops.gemm_skinny_w8(x, q, s, b, c.act, **kw)
    w8c.judge(y, w8c.reference_w8(x, q, s, b, c.act, qg, sg, bg, r, device=DEV), dtype, c.what, guard=buf, fill=FILL)
    return y


def _w8(dtype, c):
    """Case c on operands of its own."""
    ops = _ops()
    x, q, s, b, r, qg, sg, bg = _operands(dtype, c, c.ldx)
    if c.ldw is not None or c.rows is not None:  # the views go to the launch as they are
        assert ops._w8_ok(q, "w8") is q and (qg is None or ops._w8_ok(qg, "w8_gate") is qg)
        assert ops._w8_scale(s, c.N, "w_scale").data_ptr() == s.data_ptr()
    return _launch(dtype, c, x, q, s, b, r, qg, sg, bg)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M", [c.M for c in wc.ROW_FRAGMENTS])
def test_row_fragments(dtype, M):
    """1 .. 4 row fragments, full and ragged, K below one step; x is a buffer that ends with its last row."""
    for c in wc.ROW_FRAGMENTS:
        if c.M == M:
            _w8(dtype, c)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [c.K for c in wc.K_TAILS_AND_SPLITS])
def test_k_tails_and_splits(dtype, K):
    """One 16-byte piece of K, and K % 64 in {16, 32, 48} behind many steps with several slices."""
    for c in wc.K_TAILS_AND_SPLITS:
        if c.K == K:
            _w8(dtype, c)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [c.N for c in wc.N_EDGES])
def test_n_edges(dtype, N):
    """One column, part of a 4-column group, part of a 16-row weight fragment, more than one workgroup, through the first
    kernel's epilogue (one slice).  The output is a guarded view."""
    for c in wc.N_EDGES:
        if c.N == N:
            _w8(dtype, c)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("act", ["silu", "swiglu"])
def test_n_edges_split(dtype, act):
    """The same edges with several slices: fp32 partials in rows of N % 4 != 0 elements, written and read element by element."""
    for c in wc.N_EDGES_SPLIT:
        if c.act == act:
            assert c.N % 4 != 0 and c.split
            _w8(dtype, c)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K,split", [(48, False), (1040, True)])
@pytest.mark.parametrize("act", wc.ACTS)
def test_every_activation(dtype, act, K, split):
    """Each activation through the first kernel's epilogue (one slice) and through the reduction's (several): with bias and a
    residual, and with neither; SwiGLU with and without the gate's bias."""
    calls = [c for c in wc.EVERY_ACTIVATION if (c.act, c.K, c.split) == (act, K, split)]
    assert len(calls) == (3 if act == "swiglu" else 2)
    for c in calls:
        _w8(dtype, c)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("table", ["STRIDES", "ROW_SLICE", "ZERO_SCALE"])
def test_strides_slices_zero_scales(dtype, table):
    """STRIDES: x rows K + 8 apart, weight rows K + 16 bytes apart, the output a guarded view, the residual rows wider than N.
    ROW_SLICE: the first 40 of 72 rows of a weight and of its scale vector, as views.  ZERO_SCALE: zero scales in columns 3 .. 5
    (the reference gives act(bias) (+ residual) there; a scale read from a neighbour column fails)."""
    for c in wc.TABLES[table]:
        _w8(dtype, c)


# ---- past the ring's depth ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def deep_weights():
    """(N, K) -> (w8, w8_gate, scale, scale_gate): one weight pair per table, built on first use, shared by the dtypes and cases
    (which take column prefixes of it) and never written."""
    made = {}

    def get(N, K):
        if (N, K) not in made:
            made[(N, K)] = (_bytes(N, K, 11), _bytes(N, K, 12), _scales(N, K, 0.0), _scales(N, K, 0.25) * 1.23)
        return made[(N, K)]

    yield get
    made.clear()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("table", ["unsplit", "split"])
def test_deep_pipeline(dtype, table, deep_weights):
    """Slices of more chunks than the register ring is deep: depth + 1, + 2 and + 3 in one slice (N 32776), and several slices
    of unequal chunk counts (N 8200), for plain (gelu, bias, residual) and SwiGLU (both biases, residual) at every count of row
    fragments.  The K of a table are column prefixes of one weight, so ldw != K in all but the longest."""
    cases = wc.DEEP_UNSPLIT if table == "unsplit" else wc.DEEP_SPLIT
    N, ldw = cases[0].N, max(c.K for c in cases)
    q, qg, s, sg = deep_weights(N, ldw)
    b, bg = _rand((N,), dtype, 0.5, 13), _rand((N,), dtype, 0.5, 14)
    for c in cases:
        assert c.N == N and c.res and c.bias and c.bias_gate
        x = _rand((c.M, c.K), dtype, seed=c.seed)
        r = _rand((c.M, N), dtype, 1.0, c.seed + 3)
        f = (ldw / c.K) ** 0.5  # (the scales were laid out for ldw columns)
        _launch(dtype, c, x, q[:, :c.K], s * f, b, r, qg[:, :c.K] if c.glu else None, sg * f if c.glu else None,
                bg if c.glu else None)


def _poisoned(dtype, c):
    """Case c with every operand a view inside a larger buffer (tests/_hostile_gemm.Embedded): x is the first M rows and K columns
    of [64, ldx], w8 and w8_gate the first K bytes of the rows of [N + 2, ldw] behind one guard row, the scales and biases 8
    elements into [N + 16], the residual the first N columns of [M + 1, ldr], the output one row and 16 columns into its buffer.
    Returns {name: Embedded}."""
    x, q, s, b, r, qg, sg, bg = _operands(dtype, c)
    q, qg = q.contiguous(), (qg.contiguous() if c.glu else None)
    e = {"x": hg.Embedded(x, (64, c.ldx)), "w8": hg.Embedded(q, (c.N + 2, c.ldw), (1, 0), seed=1),
         "s": hg.Embedded(s, (c.N + 16,), (8,), seed=2), "r": hg.Embedded(r, (c.M + 1, c.ldr), seed=3),
         "y": hg.Embedded(None, (c.M + 2, (c.N + 32 + 7) // 8 * 8), (1, 16), out_shape=(c.M, c.N), dtype=dtype, device=DEV)}
    if b is not None:
        e["b"] = hg.Embedded(b, (c.N + 16,), (8,), seed=4)
    if c.glu:
        e["w8g"] = hg.Embedded(qg, (c.N + 2, c.ldw), (1, 0), seed=5)
        e["sg"] = hg.Embedded(sg, (c.N + 16,), (8,), seed=6)
        if bg is not None:
            e["bg"] = hg.Embedded(bg, (c.N + 16,), (8,), seed=7)
    return e


@pytest.mark.parametrize("dtype", DTYPES)
def test_poisoned_paddings(dtype):
    """Nothing next to the operands reaches the arithmetic: x columns K .. ldx and x rows M .. 63, the weights' bytes in columns
    K .. ldw and in the rows around them, the scales and biases in front of element 0 and at and past N, residual columns
    N .. ldr and the row behind it, and the output's guard hold, in three launches at the same addresses, finite values (benign),
    NaN (0xFF bytes: NaN in e4m3fn too) and huge values (+-finfo.max / 8, 1e30 in the scales, +-448 in the weight bytes:
    fmaxf and v_max drop a NaN operand, a huge one they keep), with one slice and with several, at M 37 and M 5, plain and
    SwiGLU.  The benign launch is judged against the fp64 reference; the NaN and the huge launch must equal it bit for bit;
    after each, every byte the launch does not own is what it was."""
    ops = _ops()
    for c in wc.POISONED:
        e = _poisoned(dtype, c)
        v = lambda n: e[n].view if n in e else None  # noqa: E731
        for n in ("w8",) + (("w8g",) if c.glu else ()):
            t = v(n)
            assert ops._w8_ok(t, "w8") is t and not t.is_contiguous()
        for n in ("x", "r"):
            t = v(n)
            assert ops._rows16(t) is t and not t.is_contiguous()
        for n in ("s",) + (("sg",) if c.glu else ()):  # (the scales go to the launch where they lie: no clone drops the poison)
            t = v(n)
            assert ops._w8_scale(t, c.N, n) is t
        assert (ops.gemm_skinny_w8_splits(c.M, c.N, c.K, c.act) > 1) == c.split, c.what
        got = {}
        for fill in hg.FILLS:
            for t in e.values():
                t.fill(fill)
            y = ops.gemm_skinny_w8(v("x"), v("w8"), v("s"), v("b"), c.act, w8_gate=v("w8g"), w_scale_gate=v("sg"),
                                   bias_gate=v("bg"), residual=v("r"), out=v("y"))
            torch.cuda.synchronize()
            assert y.data_ptr() == v("y").data_ptr()
            for n, t in e.items():
                assert t.untouched(), f"{c.what} fill {fill}: bytes of {n} that the launch does not own were overwritten"
            got[fill] = y.clone()
        o = lambda n: e[n].value if n in e else None  # noqa: E731
        w8c.judge(got["benign"], w8c.reference_w8(o("x"), o("w8"), o("s"), o("b"), c.act, o("w8g"), o("sg"), o("bg"), o("r"),
                                                  device=DEV), dtype, "poisoned " + c.what)
        for fill in ("nan", "huge"):
            d = got[fill].view(torch.int16) != got["benign"].view(torch.int16)
            assert not bool(d.any()), (f"{c.what} fill {fill}: {int(d.sum())} output elements differ from the benign launch, "
                                       f"first at (row, column) {tuple(d.nonzero()[0].tolist())}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_k_zero(dtype):
    """Through the C ABI: K 0 is an empty sum, y = act(bias) (+ residual) [SwiGLU: silu(bias_gate) * bias], from the first
    kernel's epilogue with no chunk run.  x and the weights are poison and never read."""
    from mio import _lib
    ops, lib = _ops(), _lib.lib
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    for c in wc.K_ZERO:
        M, N, a = c.M, c.N, ops._ACT[c.act]
        assert c.K == 0 and lib.mio_gemm_skinny_w8_splits(M, N, 0, a) == 1 and lib.mio_gemm_skinny_w8_workspace_bytes(M, N, 0, a) == 0
        _, _, s, b, r, _, sg, bg = _operands(dtype, c)
        x = torch.full((M, 16), NAN, dtype=dtype, device=DEV)
        q, qg = (torch.full((N, 16), 0x7f, dtype=torch.uint8, device=DEV).view(FP8) for _ in range(2))
        y = torch.full((M, N), FILL, dtype=dtype, device=DEV)
        rc = lib.mio_gemm_skinny_w8(p(x), p(q), p(s), p(b), p(qg) if c.glu else None, p(sg), p(bg), p(r), p(y), None, M, N, 0, 16,
                                    16, N, N, a, ops._dtype_id(x), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.mio_last_error().decode()
        torch.cuda.synchronize()
        ref = w8c.reference_w8(x[:, :0], q[:, :0], s, b, c.act, qg[:, :0] if c.glu else None, sg, bg, r, device=DEV)
        w8c.judge(y, ref, dtype, c.what)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("act", ["none", "swiglu"])
def test_workspace_hygiene(dtype, act):
    """Through the C ABI: a workspace of exactly mio_gemm_skinny_w8_workspace_bytes, pre-filled with NaN, inside a larger NaN
    buffer.  The output is finite and correct, and no byte outside the workspace changes."""
    from mio import _lib
    ops, lib = _ops(), _lib.lib
    (c,) = [c for c in wc.WORKSPACE if c.act == act]
    M, N, K, a = c.M, c.N, c.K, ops._ACT[act]
    x, q, s, b, r, qg, sg, bg = _operands(dtype, c)
    nbytes = lib.mio_gemm_skinny_w8_workspace_bytes(M, N, K, a)
    splits = lib.mio_gemm_skinny_w8_splits(M, N, K, a)
    assert splits > 1 and nbytes == splits * M * N * 4 * (2 if c.glu else 1)
    pad = 1024  # floats either side
    big = torch.full((nbytes // 4 + 2 * pad,), NAN, dtype=torch.float32, device=DEV)
    before = big.view(torch.int32).clone()
    ws = big[pad:pad + nbytes // 4]
    y = torch.empty(M, N, dtype=dtype, device=DEV)
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    rc = lib.mio_gemm_skinny_w8(p(x), p(q), p(s), p(b), p(qg), p(sg), p(bg), p(r), p(y), p(ws), M, N, K, K, K, N, N, a,
                                ops._dtype_id(x), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.mio_last_error().decode()
    torch.cuda.synchronize()
    w8c.judge(y, w8c.reference_w8(x, q, s, b, act, qg, sg, bg, r, device=DEV), dtype, f"ws {act}")
    after = big.view(torch.int32)
    assert torch.equal(after[:pad], before[:pad]) and torch.equal(after[-pad:], before[-pad:])
    assert bool(torch.isfinite(ws).all())  # every partial the reduction reads was written


@pytest.mark.parametrize("dtype", DTYPES)
def test_deterministic_and_graph(dtype):
    """Two calls with the same inputs give the same bytes (no atomics, no arrival order), and a call captured in a graph -- one
    stream, no parallel branches -- and replayed once gives the eager bytes."""
    ops = _ops()
    for c in wc.DETERMINISTIC:
        x, q, s, b, r, _, _, _ = _operands(dtype, c)
        assert ops.gemm_skinny_w8_splits(c.M, c.N, c.K, c.act) > 1
        y1 = ops.gemm_skinny_w8(x, q, s, b, c.act, residual=r)
        y2 = ops.gemm_skinny_w8(x, q, s, b, c.act, residual=r)
        torch.cuda.synchronize()
        assert torch.equal(y1.view(torch.int16), y2.view(torch.int16)), c.what
    c = wc.DETERMINISTIC[0]
    x, q, s, b, r, _, _, _ = _operands(dtype, c)
    y1 = ops.gemm_skinny_w8(x, q, s, b, "gelu", residual=r)
    out = torch.zeros_like(y1)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        ops.gemm_skinny_w8(x, q, s, b, "gelu", residual=r, out=out)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(st)
    out.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.gemm_skinny_w8(x, q, s, b, "gelu", residual=r, out=out)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), y1.view(torch.int16))


def test_dtype_refusals():
    """Wrong dtypes are a ValueError that names float8_e4m3fn, as the KV-cache ops'; a per-tensor scale is expanded."""
    ops = _ops()
    c = wc.ROW_FRAGMENTS[1]
    x, q, s, b, r, _, _, _ = _operands(torch.bfloat16, c)
    for bad in (q.view(torch.uint8), q.view(torch.float8_e5m2), q.to(torch.bfloat16)):
        with pytest.raises(ValueError, match="float8_e4m3fn"):
            ops.gemm_skinny_w8(x, bad, s)
    with pytest.raises(ValueError, match="float8_e4m3fn"):
        ops.gemm_skinny_w8(x, q, s.double())
    with pytest.raises(ValueError, match="gate weights"):
        ops.gemm_skinny_w8(x, q, s, activation="swiglu", w8_gate=q)
    one = torch.full((1,), 2.0 ** -7, dtype=torch.float32, device=DEV)
    y = ops.gemm_skinny_w8(x, q, one, b, "gelu", residual=r)
    w8c.judge(y, w8c.reference_w8(x, q, one.expand(c.N).contiguous(), b, "gelu", residual=r, device=DEV), torch.bfloat16, "one scale")


# ---- the quantiser --------------------------------------------------------------------------------------------------------------
def _quant_expect(w):
    """(bytes, scale) of the stated formula, evaluated by torch in fp32 on the CPU (IEEE division and multiplication, the cast's
    round to nearest even): a = max |w| over the row's non-NaN elements, scale = a / 448 (1 where a == 0),
    w8 = (w.float() * (1 / scale)).clamp(-448, 448).to(float8_e4m3fn)."""
    wf = w.detach().cpu().float()
    a = torch.where(torch.isnan(wf), torch.zeros_like(wf), wf.abs()).amax(dim=1)
    scale = torch.where(a == 0, torch.ones_like(a), a / torch.tensor(448.0))
    inv = torch.ones_like(scale) / scale
    q = (wf * inv[:, None]).clamp(-448.0, 448.0).to(FP8)
    return q.view(torch.uint8), scale


@pytest.mark.parametrize("dtype", DTYPES)
def test_quantize_weight(dtype):
    """w8 and scale bit-equal to the formula evaluated by torch; an all-zero row (scale 1, bytes 0); a NaN element (0x7f or 0xff,
    the row's scale from the rest); a strided source; N 1 and N 73."""
    ops = _ops()
    for N, K, ldw in wc.QUANT:
        w = _rand((N, ldw or K), dtype, K ** -0.5, seed=N + K)[:, :K]
        if N > 2:
            w[1].zero_()
            w[2, 5] = NAN
            w[2, K - 1] = -NAN
            w[N - 1, 0] = 3.0  # (the row's maximum by far: most of the row rounds into the subnormal range of e4m3)
        assert w.is_contiguous() == (ldw is None)
        q, s = ops.quantize_weight_w8(w)
        torch.cuda.synchronize()
        assert q.dtype == FP8 and tuple(q.shape) == (N, K) and s.dtype == torch.float32 and tuple(s.shape) == (N,)
        eq, es = _quant_expect(w)
        got = q.cpu().view(torch.uint8)
        assert torch.equal(s.cpu().view(torch.int32), es.view(torch.int32)), (N, K)
        nan = torch.isnan(w.cpu().float())
        assert torch.equal(got[~nan], eq[~nan]), (N, K, int((got != eq).sum()))
        if N > 2:
            assert bool((s[1] == 1.0).item()) and bool((got[1] == 0).all())
            assert int(nan[2].sum()) == 2 and set(got[2][nan[2]].tolist()) <= {0x7f, 0xff}
            assert bool(torch.isfinite(s[2]).item()) and s[2].item() > 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_round_trip(dtype):
    """gemm_skinny_w8(x, *quantize_weight_w8(w)) against reference_w8 on the quantiser's own outputs, one slice and several."""
    ops = _ops()
    for M, N, K in ((5, 72, 48), (21, 200, 1040)):
        x, w = _rand((M, K), dtype, seed=M), _rand((N, K), dtype, K ** -0.5, seed=N)
        b, r = _rand((N,), dtype, 0.5, seed=K), _rand((M, N), dtype, seed=K + 1)
        q, s = ops.quantize_weight_w8(w)
        y = ops.gemm_skinny_w8(x, q, s, b, "gelu", residual=r)
        w8c.judge(y, w8c.reference_w8(x, q, s, b, "gelu", residual=r, device=DEV), dtype, f"round trip {M}x{N}x{K}")

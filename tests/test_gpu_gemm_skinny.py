"""The decode-step GEMM (ops.gemm_skinny / mio_gemm_skinny, 1 <= M <= 64) in bf16 and fp16 against the fp64 reference of
tests/_gemm_check.py, under the statistical bars of the route these shapes take in ops.gemm_bias_act (t128) -- the element bound
holds for any summation order, the split of K included.  The shapes are the smallest that reach each seam: every count of row
fragments, K tails and K below one step, one slice and several (asserted through ops.gemm_skinny_splits, so both kernels'
epilogues are known to have run), N down to one column and past a workgroup's 64, every activation, strides, the workspace's
bounds, determinism and a captured graph."""
import pytest
import torch

import _gemm_check as gc

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
ACTS = ["none", "gelu", "gelu_erf", "relu", "silu", "swiglu"]
FILL = -3.0e4  # guard fill: no output of these cases comes near it


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


def _skinny(dtype, M, N, K, act="none", bias=True, res=False, ldx=None, guard=False, bias_gate=True, ldr=None, split=None,
            seed=0, what=""):
    """One ops.gemm_skinny call, the whole output checked.  split: True / False asserts that the plan does / does not split K."""
    ops = _ops()
    gate = act == "swiglu"
    x, w, b, r, wg, bg = _operands(dtype, M, N, K, bias, res, seed, ldx, gate, bias_gate)
    if split is not None:
        assert (ops.gemm_skinny_splits(M, N, K, act) > 1) == split, (what, ops.gemm_skinny_splits(M, N, K, act))
    kw = {}
    if res:
        kw["residual"] = r
        if ldr is not None:  # the residual as a view of wider rows
            wide = torch.full((M, ldr), 7.0, dtype=dtype, device=DEV)
            wide[:, :N] = r
            kw["residual"] = wide[:, :N]
    if gate:
        kw.update(w_gate=wg, bias_gate=bg)
    buf = None
    if guard:  # the output as a view inside a buffer filled with FILL: one row and 16 columns on either side
        buf = torch.full((M + 2, (N + 32 + 7) // 8 * 8), FILL, dtype=dtype, device=DEV)  # (row stride a multiple of 8)
        kw["out"] = buf[1:M + 1, 16:N + 16]
    y = ops.gemm_skinny(x, w, b, act, **kw)
    ref = gc.reference(x, w, b, act, wg, bg, r, device=DEV)
    gc.check(y, ref, dtype, "skinny", guard=buf, fill=FILL, bars=gc.BARS[(dtype, "t128")], what=what)
    return y


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M", [1, 5, 16, 17, 33, 48, 64])
def test_row_fragments(dtype, M):
    """1 .. 4 row fragments, full and ragged; x is a buffer that ends with its last row."""
    _skinny(dtype, M, 72, 40, "gelu", res=True, split=False, seed=M, what=f"M {M}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,K,bias,split", [(37, 72, 8, True, False), (37, 72, 4104, False, True), (64, 264, 1024, True, True),
                                              (3, 8, 2056, True, True)])
def test_k_tails_and_splits(dtype, M, N, K, bias, split):
    """K below one step, K % 32 != 0 behind many steps, and the split: K >= 1024 runs both launches, K <= 40 one."""
    _skinny(dtype, M, N, K, bias=bias, res=True, split=split, seed=K, what=f"{M}x{N}x{K}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [1, 8, 15, 72, 1000])
def test_n_edges(dtype, N):
    """One column, part of a 4-column group, part of a 16-row weight fragment, more than one workgroup; no multiple of 4 in the
    partials' rows at N 1 and 15.  The output is a guarded view whose rows are a multiple of 8 elements apart."""
    _skinny(dtype, 17, N, 264, "silu", guard=True, seed=N, what=f"N {N}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K,split", [(40, False), (1032, True)])
@pytest.mark.parametrize("act", ACTS)
def test_every_activation(dtype, act, K, split):
    """Each activation through the first kernel's epilogue (one slice) and through the reduction's (several): with bias and a
    residual, and with neither; SwiGLU with and without the gate's bias."""
    _skinny(dtype, 21, 72, K, act, bias=True, res=True, split=split, seed=1, what=f"{act} K {K}")
    _skinny(dtype, 21, 72, K, act, bias=False, res=False, bias_gate=False, split=split, seed=2, what=f"{act} K {K} bare")
    if act == "swiglu":
        _skinny(dtype, 21, 72, K, act, bias=False, res=True, bias_gate=True, split=split, seed=3, what=f"{act} K {K} gate bias")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K,split", [(40, False), (1032, True)])
def test_strides(dtype, K, split):
    """x rows K + 8 apart, the output a guarded view (one row and 16 columns either side), the residual rows wider than N."""
    _skinny(dtype, 37, 72, K, "gelu", res=True, ldx=K + 8, guard=True, ldr=88, split=split, seed=K, what=f"strides K {K}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("act", ["none", "swiglu"])
def test_workspace_hygiene(dtype, act):
    """Through the C ABI: a workspace of exactly mio_gemm_skinny_workspace_bytes, pre-filled with NaN, inside a larger NaN buffer.
    The output is finite and correct, and no byte outside the workspace changes."""
    from mio import _lib
    ops, lib = _ops(), _lib.lib
    M, N, K = 19, 136, 1032
    a = ops._ACT[act]
    gate = act == "swiglu"
    x, w, b, r, wg, bg = _operands(dtype, M, N, K, res=True, gate=gate, seed=9)
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
    gc.check(y, gc.reference(x, w, b, act, wg, bg, r, device=DEV), dtype, "skinny", bars=gc.BARS[(dtype, "t128")], what=f"ws {act}")
    after = big.view(torch.int32)
    assert torch.equal(after[:pad], before[:pad]) and torch.equal(after[-pad:], before[-pad:])
    assert bool(torch.isfinite(ws).all())  # every partial the reduction reads was written


@pytest.mark.parametrize("dtype", DTYPES)
def test_deterministic_and_graph(dtype):
    """Two calls with the same inputs give the same bytes (no atomics, no arrival order), and a call captured in a graph --
    one stream, no parallel branches -- and replayed once gives the eager bytes: the launch neither allocates nor synchronises
    beyond the workspace ops.gemm_skinny takes from torch's allocator."""
    ops = _ops()
    M, N, K = 33, 200, 2056
    x, w, b, r, _, _ = _operands(dtype, M, N, K, res=True, seed=4)
    assert ops.gemm_skinny_splits(M, N, K, "gelu") > 1
    y1 = ops.gemm_skinny(x, w, b, "gelu", residual=r)
    y2 = ops.gemm_skinny(x, w, b, "gelu", residual=r)
    torch.cuda.synchronize()
    assert torch.equal(y1.view(torch.int16), y2.view(torch.int16))
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

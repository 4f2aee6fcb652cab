"""The mixture-of-experts path for tall inputs (ops.moe_route_prefill / moe_up_prefill / moe_down_prefill / moe_mlp_prefill and
MoEMLP with MoEConfig(grouped_prefill=True)) against the fp64 restatement of tests/_moe_check.py, stage by stage from the bytes
each launch read, under the bounds and bars the decode path is judged by.  Shapes sit at the seams of the 128 x 128 x 64 tile
(SwiGLU: 64 up columns and their gate columns): partial and full row tiles, an idle expert, a K tail below one chunk and three
chunks plus a tail, ragged and exact column tiles."""
import pytest
import torch

import _moe_cases as cs
import _moe_check as mc

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
FILL = -3.0e4  # guard fill: no output of these cases comes near it
NAN = float("nan")
BM = 128


def _ops():
    from mio import ops
    return ops


def _rand(shape, dtype, scale=1.0, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(shape, device=DEV, generator=g) * scale).to(dtype)


def _strided(value, shape):
    """value as the leading view of a NaN-filled buffer of `shape`: wider rows, more rows (per expert)."""
    buf = torch.full(shape, NAN, dtype=value.dtype, device=DEV)
    idx = tuple(slice(0, n) for n in value.shape)
    buf[idx] = value
    return buf[idx]


def _guarded(rows, N, dtype):
    """An output view inside a buffer filled with FILL: one row and 16 columns on either side."""
    buf = torch.full((rows + 2, (N + 32 + 7) // 8 * 8), FILL, dtype=dtype, device=DEV)
    return buf, buf[1:rows + 1, 16:N + 16]


def _permuted_logits(T, E, dtype, seed):
    """Rows that are permutations of i / 16 - 8, i < E: distinct, exact in bf16, inside [T, E + 24] whose padding is NaN."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(T, E, generator=g).argsort(1).float() / 16 - 8
    return _strided(x.to(dtype).to(DEV), (T, E + 24))


def _check_route(route, logits, k, renorm, what):
    """The five arrays by mc.check_route; the tile map by equality with the one the reference offsets give."""
    ref = mc.route_reference(logits, k, renorm)
    mc.check_route(ref, *route[:5], what=what)
    E, T = ref.num_experts, logits.shape[0]
    n = (ref.offsets.diff() + BM - 1) // BM
    te = torch.repeat_interleave(torch.arange(E), n)
    tr = ref.offsets[:-1][te] + (torch.arange(te.numel()) - (n.cumsum(0) - n)[te]) * BM
    nt = int(route.num_tiles)
    assert nt == te.numel() <= route.tile_expert.numel() == _ops().moe_prefill_max_tiles(T, k, E) == T * k // BM + min(E, T * k), what
    assert torch.equal(route.tile_expert[:nt].cpu().long(), te) and torch.equal(route.tile_row0[:nt].cpu().long(), tr), what
    return ref


@pytest.mark.parametrize("E", [3, 8, 65, 256])
@pytest.mark.parametrize("T", [65, 200, 1000])
def test_route(T, E):
    """top_k 1, 2 and 8 (k <= E), logits in bf16 and fp32, renormalised and not; row stride > E with NaN behind every row."""
    for k in (k for k in (1, 2, 8) if k <= E):
        for i, ldtype in enumerate((torch.bfloat16, torch.float32)):
            logits = _permuted_logits(T, E, ldtype, seed=T + E + k)
            route = _ops().moe_route_prefill(logits, k, renormalize=bool(i))
            assert route.top_k == k and route.num_experts == E
            _check_route(route, logits, k, bool(i), f"T {T} E {E} k {k} {ldtype}")


@pytest.mark.parametrize("kind", ["ties", "one_expert"])
def test_route_special_rows(kind):
    """ties: all-equal rows, the k-th and (k+1)-th logit equal, NaN / +inf / -inf entries, rows with no finite logit.
    one_expert: every token prefers expert 5, so it has T rows: several full tiles and a partial one."""
    T, E, k = 300, 8, 2
    x = _permuted_logits(T, E, torch.float32, 7)
    if kind == "ties":
        x[0::7] = 1.25
        x[1::7, :3] = 9.0
        x[2::7, 0], x[2::7, 3], x[2::7, E - 1] = float("inf"), NAN, -float("inf")
        x[3::7] = NAN
        x[4::7] = -float("inf")
    else:
        x[:, 5] = 20.0
    route = _ops().moe_route_prefill(x, k)
    ref = _check_route(route, x, k, True, kind)
    if kind == "ties":
        assert route.ids[3].tolist() == [0, 1] and not bool(route.weights[3::7].view(torch.int32).any())
    else:
        assert int(ref.offsets[6] - ref.offsets[5]) == T and int(route.num_tiles) >= 3


# ---- up and down, stage by stage -----------------------------------------------------------------------------------------------------
def _choice(name):
    """(T, k, E, logits) of a routing at the row seams.  partial: 130 rows over 8 experts, every tile partial.  full: each of 2
    experts gets all 200 rows, a full tile and a partial one.  exact: expert 0 gets exactly 128 rows, expert 1 none."""
    if name == "partial":
        return 65, 2, 8, _permuted_logits(65, 8, torch.float32, 1)
    if name == "full":
        return 200, 2, 2, _permuted_logits(200, 2, torch.float32, 2)
    t = torch.arange(200)
    choice = torch.where(t < 128, 0, 2 + t % 2)[:, None]
    return 200, 1, 4, cs.logits_for(choice, 4).to(DEV)


SHAPES = [(72, 136, "swiglu", True), (200, 256, "gelu", False), (200, 136, "swiglu", False), (72, 256, "gelu", True)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d,I,act,bias", SHAPES)
@pytest.mark.parametrize("routing", ["partial", "full", "exact"])
def test_up_and_down(routing, d, I, act, bias, dtype):
    """Each stage from the bytes it read.  Rows, weight rows and experts further apart than they are long, the gaps NaN; the
    weight and bias slabs of experts without a row NaN; h rows and workspace elements past T k NaN; outputs guarded views."""
    ops = _ops()
    T, k, E, logits = _choice(routing)
    route = ops.moe_route_prefill(logits, k)
    idle = (route.expert_offsets.diff() == 0).nonzero().flatten()
    assert (routing == "exact") == (idle.numel() > 0)
    glu = act == "swiglu"

    def weights(N, K, seed):
        w = _strided(_rand((E, N, K), dtype, K ** -0.5, seed), (E, N + 1, K + 16))
        b = _rand((E, N), dtype, 0.5, seed + 1) if bias else None
        w[idle] = NAN
        if bias:
            b[idle] = NAN
        return w, b

    what = f"{routing} d {d} I {I} {act} bias {bias}"
    x = _strided(_rand((T, d), dtype, seed=3), (T, d + 8))
    wu, bu = weights(I, d, 10)
    wg, bg = weights(I, d, 20) if glu else (None, None)
    buf, out = _guarded(T * k, I, dtype)
    h = ops.moe_up_prefill(x, route, wu, act, wg, bu, bg, out=out)
    assert h.data_ptr() == out.data_ptr()
    mc.check_up(h, mc.up_reference(x, route, wu, act, wg, bu, bg, device=DEV), dtype, "up " + what, guard=buf, fill=FILL)

    h = _strided(_rand((T * k, I), dtype, seed=4), (T * k + 3, I + 8))
    wd, bd = weights(d, I, 30)
    res = _rand((T, d + 8), dtype, seed=5)[:, :d] if bias else None
    ws = torch.full((T * k * d + 64,), NAN, device=DEV)
    buf, out = _guarded(T, d, dtype)
    y = ops.moe_down_prefill(h, route, wd, bd, res, out=out, workspace=ws)
    mc.check_down(y, mc.down_reference(h, route, wd, bd, res, device=DEV), dtype, "down " + what, guard=buf, fill=FILL)
    assert bool(torch.isnan(ws[T * k * d:]).all()) and bool(torch.isfinite(ws[:T * k * d]).all())


# ---- the whole path, reruns, graph ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_whole_path_and_module(dtype):
    """ops.moe_mlp_prefill and MoEMLP(grouped_prefill=True) at T 200, E 8, k 2, d 200, I 136 against the composed reference on the
    module's own router logits; the op and the module agree bit for bit, and a second run gives the same bits."""
    from mio.kernels.mlp import MoEConfig, MoEMLP
    ops = _ops()
    T, E, k, d, I = 200, 8, 2, 200, 136
    torch.manual_seed(E)
    m = MoEMLP(d, I, E, k, MoEConfig(dtype=dtype, grouped_prefill=True)).to(DEV)
    with torch.no_grad():
        m.router.weight.mul_(8.0)  # logits a few units apart
    x, res = _rand((T, d), dtype, seed=1), _rand((T, d), dtype, seed=2)
    logits = m._router_logits(x, dtype)
    cast = lambda p: p.detach().to(dtype)  # noqa: E731
    _, ref = mc.composed_reference(x, logits, k, True, cast(m.w_up), cast(m.w_down), "swiglu", cast(m.w_gate), residual=res, device=DEV)
    y = m(x, res)
    mc.check_down(y, ref, dtype, "module")
    route = ops.moe_route_prefill(logits, k)
    y2 = ops.moe_mlp_prefill(x, route, cast(m.w_up), cast(m.w_down), "swiglu", cast(m.w_gate), residual=res)
    mc.check_down(y2, ref, dtype, "moe_mlp_prefill")
    assert torch.equal(y.view(torch.int16), y2.view(torch.int16)) and torch.equal(m(x, res).view(torch.int16), y.view(torch.int16))


def test_graph_replays_under_new_routing():
    """Route and MLP captured on one stream at a routing with 8 tiles (50 rows for each of 8 experts); the logits are then
    overwritten so that every token goes to experts 1 and 3 (200 rows each, 4 tiles).  Each of several replays passes the checker
    for the routing at hand and equals the eager result bit for bit: the grid is sized by the bound, the map is device data."""
    ops = _ops()
    dtype, T, E, k, d, I = torch.bfloat16, 200, 8, 2, 72, 136
    x = _rand((T, d), dtype, seed=1)
    wu, wg, wd = (_rand(s, dtype, s[2] ** -0.5, 1 + j) for j, s in enumerate([(E, I, d), (E, I, d), (E, d, I)], 1))
    t = torch.arange(T)
    first = cs.logits_for(torch.stack([t % E, (t + 1) % E], 1), E).to(DEV)
    second = cs.logits_for(torch.tensor([1, 3]).expand(T, k).contiguous(), E).to(DEV)
    logits = first.clone()
    route = ops.moe_route_prefill(logits, k)
    out = torch.zeros(T, d, dtype=dtype, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up on the capture stream
        ops.moe_mlp_prefill(x, ops.moe_route_prefill(logits, k, out=route), wu, wd, "swiglu", wg, out=out)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.moe_mlp_prefill(x, ops.moe_route_prefill(logits, k, out=route), wu, wd, "swiglu", wg, out=out)
    tiles = []
    for want in (second, first, second):
        logits.copy_(want)
        out.fill_(NAN)
        g.replay()
        torch.cuda.synchronize()
        _check_route(route, want, k, True, "replay")
        tiles.append(int(route.num_tiles))
        _, ref = mc.composed_reference(x, want, k, True, wu, wd, "swiglu", wg, device=DEV)
        mc.check_down(out, ref, dtype, "replay")
        eager = ops.moe_mlp_prefill(x, ops.moe_route_prefill(want, k), wu, wd, "swiglu", wg)
        assert torch.equal(out.view(torch.int16), eager.view(torch.int16))
    assert tiles == [4, 8, 4]


def test_refusals():
    """T 8193, k > E, K % 8 != 0 and a missing workspace are refused with the entry point named; T == 0 returns empty results;
    the decode router still refuses 65 tokens."""
    from mio import _lib
    ops, lib = _ops(), _lib.lib
    A = 0x1000  # a dummy aligned address: every refusal comes before any launch
    with pytest.raises(ValueError, match="8192"):
        ops.moe_route_prefill(torch.zeros(8193, 8, device=DEV), 2)
    with pytest.raises(ValueError, match="top_k"):
        ops.moe_route_prefill(torch.zeros(70, 4, device=DEV), 5)
    assert lib.mio_moe_prefill_route(A, 8, A, A, A, A, A, A, A, A, 8193, 8, 2, 1, 2, None) < 0
    assert "mio_moe_prefill_route: T must be at most 8192" in lib.mio_last_error().decode()
    assert lib.mio_moe_prefill_up(A, A, None, A, None, A, A, A, A, A, A, 70, 2, 8, 64, 68, 72, 72, 64 * 72, 64, 5, 0, None) < 0
    assert "mio_moe_prefill_up: K must be a multiple of 8" in lib.mio_last_error().decode()
    assert lib.mio_moe_prefill_down(A, A, None, A, A, A, A, A, A, A, None, A, None, 70, 2, 8, 64, 72, 72, 72, 64 * 72, 64, 0, 0, None) < 0
    assert "mio_moe_prefill_down: workspace required" in lib.mio_last_error().decode()
    empty = ops.moe_route_prefill(torch.zeros(0, 8, device=DEV), 2)
    assert int(empty.num_tiles) == 0 and not bool(empty.expert_offsets.any())
    w = torch.zeros(8, 16, 8, dtype=torch.bfloat16, device=DEV)
    y = ops.moe_mlp_prefill(torch.zeros(0, 8, dtype=torch.bfloat16, device=DEV), empty, w, w.transpose(1, 2).contiguous(), "gelu")
    assert tuple(y.shape) == (0, 8)
    with pytest.raises(ValueError, match="decode steps only"):
        ops.moe_route(torch.zeros(65, 8, device=DEV), 2)

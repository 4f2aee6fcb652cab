"""The mixture-of-experts path for tall inputs (ops.moe_route_prefill / moe_up_prefill / moe_down_prefill / moe_mlp_prefill and
MoEMLP with MoEConfig(grouped_prefill=True)) against the fp64 restatement of tests/_moe_check.py, stage by stage from the bytes
each launch read, under the bounds and bars the decode path is judged by.  Shapes sit at the seams of the 128 x 128 x 64 tile
(SwiGLU: 64 up columns and their gate columns): partial and full row tiles, an idle expert, a K tail below one chunk and three
chunks plus a tail, ragged and exact column tiles.

The last two sections hold the three paths (decode on 16-bit experts, decode on FP8 experts, prefill) to what their shared route,
up and down cores promise: refusals under the name of the op that was called, every copy the cores make on the way to a launch,
and MoEMLP's one chunk loop at its seams, bit for bit."""
import pytest
import torch

import _moe_cases as cs
import _moe_check as mc
import test_gpu_moe_w8 as w8t  # (the FP8 path's weights and fp64 references)

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


# ---- the three paths through the one route, up and down core -------------------------------------------------------------------------
# path -> (route op, up op, down op, the route op of the other class)
PATHS = {"decode": ("moe_route", "moe_up", "moe_down", "moe_route_prefill"),
         "decode_w8": ("moe_route", "moe_up_w8", "moe_down_w8", "moe_route_prefill"),
         "prefill": ("moe_route_prefill", "moe_up_prefill", "moe_down_prefill", "moe_route")}


def _weight(path, E, N, K, dtype, seed, strided=True):
    """A stacked weight as the path's ops take it: (w,) 16-bit, (w8, scale) on the FP8 path; strided: rows 16 wider, a spare row."""
    if path == "decode_w8":
        q, s = w8t._quant(E, N, K, dtype, seed)
        return (q if strided else q.contiguous(), s)
    w = _rand((E, N, K), dtype, K ** -0.5, seed)
    return (_strided(w, (E, N + 1, K + 16)) if strided else w,)


def _up(path, x, route, w, act, g=None, **kw):
    """The path's up op on w (and the gate g), each as _weight made it."""
    if path == "decode_w8":
        return _ops().moe_up_w8(x, route, *w, act, *(g or (None, None)), **kw)
    return getattr(_ops(), PATHS[path][1])(x, route, *w, act, *(g or (None,)), **kw)


def _down(path, h, route, w, **kw):
    return getattr(_ops(), PATHS[path][2])(h, route, *w, **kw)


def _judge_up(path, h, x, route, w, act, g, dtype, what):
    if path == "decode_w8":
        w8t.w8c.judge(h, w8t._up_ref(x, route, *w, act, *(g or (None, None))), dtype, what)
    else:
        mc.check_up(h, mc.up_reference(x, route, *w, act, *(g or (None,)), device=DEV), dtype, what)


def _judge_down(path, y, h, route, w, res, dtype, what):
    eff = w8t._eff(*w) if path == "decode_w8" else w[0]
    mc.check_down(y, mc.down_reference(h, route, eff, None, res, device=DEV), dtype, what)


@pytest.mark.parametrize("path", sorted(PATHS))
def test_refusals_name_their_op(path):
    """T 3, E 4, k 2, d 16, I 16.  What the one core refuses it refuses under the name of the public op that was called, as a
    ValueError: the ops layer's own, raised before the entry point is called (whose refusal would be a RuntimeError).  The two
    SwiGLU messages carry no op name, as before."""
    ops = _ops()
    route_op, up_op, down_op, other_route_op = PATHS[path]
    T, E, k, d, I, dtype = 3, 4, 2, 16, 16, torch.bfloat16
    w8 = path == "decode_w8"
    logits = _permuted_logits(T, E, torch.float32, 1)
    route, other = getattr(ops, route_op)(logits, k), getattr(ops, other_route_op)(logits, k)
    kind = type(route).__name__
    x, h = _rand((T, d), dtype, seed=1), _rand((T * k, I), dtype, seed=2)
    wu, wg, wd = (_weight(path, E, *s, dtype, i) for i, s in enumerate([(I, d), (I, d), (d, I)]))
    gate = "w8_gate and s_gate belong" if w8 else "w_gate belongs"
    up_name, down_name = ("w8_up", "w8_down") if w8 else ("w_up", "w_down")
    wrong = (lambda w: (_rand(w[0].shape, dtype, seed=9), *w[1:])) if w8 else (lambda w: (w[0].to(torch.float16),))
    dtype_text = "must be torch.float8_e4m3fn" if w8 else "must have the activation dtype"
    nan_rows = lambda rows, n: torch.full((rows, n), NAN, dtype=dtype, device=DEV)  # noqa: E731
    refused = [
        (rf"^{up_op}: route must be a {kind} ", lambda: _up(path, x, other, wu, "swiglu", wg)),
        (rf"^{down_op}: route must be a {kind} ", lambda: _down(path, h, other, wd)),
        (rf"^{up_op}: x has 4 rows, the route 3 tokens", lambda: _up(path, _rand((T + 1, d), dtype), route, wu, "swiglu", wg)),
        (rf"^{down_op}: h must be \[T k = 6, I\]", lambda: _down(path, h[:5], route, wd)),
        (rf"^{up_op}: {gate} to act='swiglu'$", lambda: _up(path, x, route, wu, "gelu", wg)),
        (r"^SwiGLU activation requires gate weights" + (" and their scales$" if w8 else "$"), lambda: _up(path, x, route, wu, "swiglu")),
        (rf"^{up_op}: {up_name} {dtype_text}", lambda: _up(path, x, route, wrong(wu), "gelu")),
        (rf"^{down_op}: {down_name} {dtype_text}", lambda: _down(path, h, route, wrong(wd))),
        (rf"^{up_op}: out must be \[6, 16\] ", lambda: _up(path, x, route, wu, "gelu", out=nan_rows(T * k + 1, I))),
        (rf"^{up_op}: out must be \[6, 16\] .* multiple of 8", lambda: _up(path, x, route, wu, "gelu", out=nan_rows(T * k, I + 4)[:, :I])),
        (rf"^{down_op}: out must be \[3, 16\] ", lambda: _down(path, h, route, wd, out=nan_rows(T, d + 8))),
        (rf"^{down_op}: out must be \[3, 16\] .* multiple of 8", lambda: _down(path, h, route, wd, out=nan_rows(T, d + 4)[:, :d])),
    ]
    if w8:  # the scaled form also refuses a gate without its scales, and the reverse
        refused += [(r"^SwiGLU activation requires gate weights and their scales$", lambda: _up(path, x, route, wu, "swiglu", (wg[0], None))),
                    (rf"^{up_op}: {gate} to act='swiglu'$", lambda: _up(path, x, route, wu, "gelu", (None, wg[1])))]
    out = nan_rows(T, d)
    if path == "prefill":
        need = ops.lib.mio_moe_prefill_down_workspace_bytes(T, k, E, d, I) // 4
        assert need >= T * k * d
        ws = torch.zeros(need + 4, device=DEV)
        text = rf"^{down_op}: workspace must be a contiguous, 16-byte aligned fp32 tensor of at least {need} elements"
        refused += [(text, lambda: _down(path, h, route, wd, out=out, workspace=ws[:need - 1])),
                    (text, lambda: _down(path, h, route, wd, out=out, workspace=ws[1:need + 1]))]
    for text, call in refused:
        with pytest.raises(ValueError, match=text):
            call()
    assert bool(torch.isnan(out).all())  # (nothing was written behind a refusal)
    _down(path, h, route, wd, out=out)   # and the same call, unrefused, writes it
    assert bool(torch.isfinite(out).all())


@pytest.mark.parametrize("route_op", ["moe_route", "moe_route_prefill"])
def test_route_fixups(route_op):
    """Logits the launch cannot take as they are, each judged against the reference routing of the values handed in: contiguous at
    a storage offset of one element (contiguous() returns them as they are: cloned), rows 24 apart at such an offset (copied), one
    row expanded to T (row stride 0 < E: copied), a single row out of a strided buffer (its stride is not consulted), no row."""
    route = getattr(_ops(), route_op)
    T, E, k = 5, 8, 2
    base = _permuted_logits(T, E, torch.float32, 3)
    off = torch.zeros(T * E + 1, device=DEV)[1:].view(T, E).copy_(base)
    wide = torch.full((T * (E + 24) + 1,), NAN, device=DEV)[1:].view(T, E + 24)[:, :E].copy_(base)
    row = base[2:3].expand(T, E)
    one = base[4:5]
    assert off.is_contiguous() and off.data_ptr() % 16 == 4 and wide.data_ptr() % 16 == 4 and wide.stride(0) == E + 24
    assert row.stride(0) == 0 and one.stride(0) == E + 24 and one.data_ptr() % 16 == 0
    for what, logits in (("offset", off), ("offset, wide rows", wide), ("expanded", row), ("one row", one)):
        got = route(logits, k)
        mc.check_route(mc.route_reference(logits, k, True), *got[:5], what=f"{route_op} {what}")
    empty = route(base[:0], k)
    assert tuple(empty.ids.shape) == (0, k) and not bool(empty.expert_offsets.any())


@pytest.mark.parametrize("path", sorted(PATHS))
def test_up_down_fixups(path):
    """Operands that take each copy the cores make, judged by the checkers against fp64, at E 4, k 2, K 16, N 20: a gate that is
    contiguous under an up weight with padded rows (up is then copied too: one pair of strides goes to the launch); a contiguous
    residual of 20 columns (T 3: copied to rows 24 apart; T 1: taken as it is, at the single-row stride); h and y of one row; T 0."""
    ops = _ops()
    E, k, K, N, dtype = 4, 2, 16, 20, torch.bfloat16
    wu, wg, wd = _weight(path, E, N, K, dtype, 1), _weight(path, E, N, K, dtype, 2, strided=False), _weight(path, E, N, K, dtype, 3)
    assert wu[0].stride() != wg[0].stride() and wg[0].is_contiguous()
    for T in (3, 1, 0):
        kk = 1 if T == 1 else k
        route = getattr(ops, PATHS[path][0])(_permuted_logits(T, E, torch.float32, 5), kk)
        x, h, res = _rand((T, K), dtype, seed=6), _rand((T * kk, K), dtype, seed=7), _rand((T, N), dtype, seed=8)
        assert res.is_contiguous()
        hu = _up(path, x, route, wu, "swiglu", wg)
        y = _down(path, h, route, wd, residual=res)
        assert tuple(hu.shape) == (T * kk, N) and tuple(y.shape) == (T, N)
        if T:
            assert hu.stride(0) == 24 and y.stride(0) == 24
            _judge_up(path, hu, x, route, wu, "swiglu", wg, dtype, f"{path} up T {T}")
            _judge_down(path, y, h, route, wd, res, dtype, f"{path} down T {T}")


# ---- the module's one chunk loop -------------------------------------------------------------------------------------------------------
def _module(**config):
    from mio.kernels.mlp import MoEConfig, MoEMLP
    torch.manual_seed(4)
    m = MoEMLP(32, 48, 4, 2, MoEConfig(**config)).to(DEV)
    with torch.no_grad():
        m.router.weight.mul_(8.0)  # logits a few units apart
    return m


def _by_hand(m, x, res, bounds, path):
    """The path's ops on the row ranges `bounds` of x, with the module's router logits and the weight copies it reads."""
    ops, dt = _ops(), m.config.dtype
    if path == "decode_w8":
        up, down, gate = (m._cast.get_experts_w8(p, dt) for p in (m.w_up, m.w_down, m.w_gate))
    else:
        up, down, gate = ((p.detach().to(dt),) for p in (m.w_up, m.w_down, m.w_gate))
    parts = []
    for lo, hi in bounds:
        route = getattr(ops, PATHS[path][0])(m._router_logits(x[lo:hi], dt), m.top_k, m.config.renormalize)
        parts.append(_down(path, _up(path, x[lo:hi], route, up, "swiglu", gate), route, down, residual=res[lo:hi]))
    return torch.cat(parts)


@pytest.mark.parametrize("path", sorted(PATHS))
def test_module_at_the_chunk_seam(path):
    """E 4, k 2, d 32, I 48, bf16, a residual, T 70: forward is the path's ops on rows [0, 64) and [64, 70), bit for bit -- on the
    prefill path one call on all 70 rows."""
    m = _module(expert_weights_fp8=path == "decode_w8", grouped_prefill=path == "prefill")
    x, res = _rand((70, 32), torch.bfloat16, seed=1), _rand((70, 32), torch.bfloat16, seed=2)
    want = _by_hand(m, x, res, [(0, 70)] if path == "prefill" else [(0, 64), (64, 70)], path)
    assert torch.equal(m(x, res).view(torch.int16), want.view(torch.int16))


def test_module_prefill_tail_stays_on_the_prefill_ops(monkeypatch):
    """T 8200 under grouped_prefill: rows [0, 8192) and the 8-row tail [8192, 8200) both go through the prefill ops (the path is
    chosen on the whole T), and forward is those two calls, bit for bit."""
    ops = _ops()
    m = _module(grouped_prefill=True)
    x, res = _rand((8200, 32), torch.bfloat16, seed=1), _rand((8200, 32), torch.bfloat16, seed=2)
    want = _by_hand(m, x, res, [(0, 8192), (8192, 8200)], "prefill")
    routed = []

    def noting(name, op):
        def route(logits, *args, **kwargs):
            routed.append((name, logits.shape[0]))
            return op(logits, *args, **kwargs)
        return route

    for name in ("moe_route", "moe_route_prefill"):
        monkeypatch.setattr(ops, name, noting(name, getattr(ops, name)))
    got = m(x, res)
    assert routed == [("moe_route_prefill", 8192), ("moe_route_prefill", 8)]
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))

"""The mixture-of-experts decode step on weight-only FP8 expert weights (ops.moe_up_w8 / moe_down_w8 / moe_mlp_w8,
MoEConfig.expert_weights_fp8) in bf16 and fp16.  The fp64 references read the very bytes and scales the kernels read (the effective
weight is widen(w8) * scale): up per expert by _w8_check.reference_w8 under _w8_check.BARS, down by _moe_check.down_reference."""
import pytest
import torch

import _gemm_check as gc
import _moe_cases as cs
import _moe_check as mc
import _w8_check as w8c
from test_gpu_moe import DEV, DTYPES, FILL, _guarded, _ops, _p, _rand  # (FILL: the guard fill, which no output here comes near)

pytestmark = pytest.mark.gpu
PAD = 0x7F  # e4m3fn NaN: the byte behind every weight row and every expert
_bits = lambda t: t.view(torch.int16)  # noqa: E731
_eff = lambda q, s: w8c.widen(q, DEV) * s.to(torch.float64)[:, :, None]  # noqa: E731  (the effective weight, fp64)


def _quant(E, N, K, dtype, seed, pad=PAD):
    """(w8 [E, N, K] leading a buffer [E, N + 1, K + 16] of `pad` bytes: ldw > K, expert_stride > N ldw; scale [E, N], three columns 0)."""
    q, s = _ops().quantize_expert_weights_w8(_rand((E, N, K), dtype, K ** -0.5, seed))
    buf = torch.full((E, N + 1, K + 16), pad, dtype=torch.uint8, device=DEV)
    buf[:, :N, :K] = q.view(torch.uint8)
    s[:, [0, min(5, N - 1), N - 1]] = 0.0
    return buf.view(w8c.FP8)[:, :N, :K], s


def _route(T, k, E, first, seed=0):
    """Every token picks k of the first `first` experts (the others stay idle); "zero": every token picks expert 0."""
    g = torch.Generator().manual_seed(seed)
    choice = torch.zeros(T, 1, dtype=torch.int64) if first == "zero" else torch.stack([torch.randperm(first, generator=g)[:k] for _ in range(T)])
    route = _ops().moe_route(cs.logits_for(choice, E).to(DEV), k)
    assert torch.equal(route.ids.cpu().long(), choice)
    return route


def _up_ref(x, route, q, s, act, qg=None, sg=None, b=None, bg=None):
    """fp64 h [T k, N] by sorted position: _w8_check.reference_w8 per expert on the gathered rows."""
    off, srt = route.expert_offsets.tolist(), route.sorted_rows.long()
    y = torch.zeros(srt.numel(), q.shape[1], dtype=torch.float64, device=DEV)
    tol = torch.zeros_like(y)
    for e in range(route.num_experts):
        lo, hi = off[e], off[e + 1]
        if hi > lo:
            of_e = [None if t is None else t[e] for t in (b, qg, sg, bg)]
            r = w8c.reference_w8(x[srt[lo:hi] // route.top_k], q[e], s[e], of_e[0], act, *of_e[1:], device=DEV)
            y[lo:hi], tol[lo:hi] = r.y, r.tol
    return gc.Ref(y, tol, q.shape[2])


# what, T, k, E, N, K, act, bias, several slices, experts chosen from (the split aims at 512 workgroups: 256 aimed experts never split)
CASES = [
    ("T 1, K 48 below one step", 1, 1, 8, 70, 48, "gelu", True, False, 8),
    ("T 1, K 80 ragged last step", 1, 2, 8, 72, 80, "swiglu", False, False, 8),
    ("17 rows on expert 0: two fragments, one slice", 17, 1, 4, 70, 80, "swiglu", True, False, "zero"),
    ("17 rows on expert 0: eight slices, partials element by element", 17, 1, 4, 70, 1040, "silu", False, True, "zero"),
    ("T 64 over E 128, 28 idle, two slices", 64, 8, 128, 72, 1040, "swiglu", True, True, 100),
    ("K 1040 plain: 5 chunks on the depth-3 ring", 64, 8, 256, 70, 1040, "none", True, False, 256),
    ("K 656 SwiGLU: 6 chunks on the depth-4 ring", 64, 8, 256, 72, 656, "swiglu", False, False, 256),
    # the scaled branch of the shared down finish with b_down, a residual and N % 4 != 0 at once over several slices
    ("T 3, N 15: bias and ragged columns across two slices", 3, 2, 4, 15, 144, "gelu", True, True, 4),
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", CASES, ids=[c[0].replace(" ", "-") for c in CASES])
def test_up_down_against_fp64(c, dtype):
    """Up from x, then down from an h of its own (h [T k, K]: up's N 70 / 72 cannot be a K, a multiple of 16), both on the case's (N, K),
    whole outputs inside guard-filled buffers; weights in 0x7f-filled buffers, three scale columns exactly 0, down with a residual."""
    what, T, k, E, N, K, act, bias, split, first = c
    ops, glu = _ops(), act == "swiglu"
    route = _route(T, k, E, first, seed=K)
    assert (ops.moe_up_w8_splits(T, k, E, N, K, act) > 1) == split and (ops.moe_down_w8_splits(T, k, E, N, K) > 1) == split
    x, hin = _rand((T, K), dtype, seed=1), _rand((T * k, K), dtype, seed=2)
    (q, s), (qg, sg) = _quant(E, N, K, dtype, 3), (_quant(E, N, K, dtype, 4) if glu else (None, None))
    assert q.stride(1) > K and q.stride(0) > N * q.stride(1) and int((s == 0).sum()) == 3 * E
    b = _rand((E, N), dtype, 0.5, 5) if bias else None
    bg = _rand((E, N), dtype, 0.5, 6) if bias and glu else None
    buf, out = _guarded(T * k, N, dtype)
    h = ops.moe_up_w8(x, route, q, s, act, qg, sg, b, bg, out=out)
    w8c.judge(h, _up_ref(x, route, q, s, act, qg, sg, b, bg), dtype, "up " + what, guard=buf, fill=FILL)
    r = _rand((T, (N + 7) // 8 * 8), dtype, 1.0, 7)[:, :N]
    buf, out = _guarded(T, N, dtype)
    y = ops.moe_down_w8(hin, route, q, s, b, r, out=out)
    mc.check_down(y, mc.down_reference(hin, route, _eff(q, s), b, r, device=DEV), dtype, "down " + what, guard=buf, fill=FILL)


# T -> (a K of one slice, a K of several): the slice is at least 16 T k, in steps of 64 (64, 320 and 1024 k)
ONE_EXPERT_K = {1: (48, 336), 17: (48, 976), 64: (48, 3088)}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", sorted(ONE_EXPERT_K))
def test_one_expert_is_the_decode_gemm_w8(dtype, T):
    """E = 1, top_k = 1: the route is the identity with weights exactly 1.0f and the plan is mio_gemm_skinny_w8's, so up (SwiGLU, gelu)
    and down (bias, residual) equal ops.gemm_skinny_w8 bit for bit.  N 70 and 72, one slice and several.  (One row of N 70 is left to
    test_up_down_against_fp64: ops.gemm_skinny_w8 hands the launch a one-row view's stride, N, which is refused.)"""
    ops = _ops()
    route = ops.moe_route(torch.zeros(T, 1, device=DEV), 1)
    seen = set()
    for N in ((72,) if T == 1 else (70, 72)):
        for K in ONE_EXPERT_K[T]:
            x = _rand((T, K), dtype, seed=K + T)
            (q, s), (qg, sg) = _quant(1, N, K, dtype, 1), _quant(1, N, K, dtype, 2)
            b, bg = _rand((1, N), dtype, 0.5, 3), _rand((1, N), dtype, 0.5, 4)
            r = _rand((T, (N + 7) // 8 * 8), dtype, 1.0, 5)[:, :N]
            for act in ("swiglu", "gelu"):
                n = ops.gemm_skinny_w8_splits(T, N, K, act)
                assert ops.moe_up_w8_splits(T, 1, 1, N, K, act) == n, (T, N, K, act)
                seen.add(n > 1)
                g = (qg, sg, bg) if act == "swiglu" else (None, None, None)
                want = ops.gemm_skinny_w8(x, q[0], s[0], b[0], act, *(None if t is None else t[0] for t in g))
                got = ops.moe_up_w8(x, route, q, s, act, g[0], g[1], b, g[2])
                assert torch.equal(_bits(got), _bits(want)), f"up T {T} N {N} K {K} {act} {dtype}"
            assert ops.moe_down_w8_splits(T, 1, 1, N, K) == ops.gemm_skinny_w8_splits(T, N, K, "none")
            want = ops.gemm_skinny_w8(x, q[0], s[0], b[0], "none", residual=r)
            assert torch.equal(_bits(ops.moe_down_w8(x, route, q, s, b, r)), _bits(want)), f"down T {T} N {N} K {K} {dtype}"
    assert seen == {False, True}


@pytest.mark.parametrize("dtype", DTYPES)
def test_hostile_memory(dtype):
    """One routing over 5 of 8 experts, through the C ABI, clean and hostile: the idle experts' weight bytes 0x7f and their scales
    and biases NaN, every row and expert padding byte 0x7f, the h rows >= T k NaN, both workspaces NaN.  The same bits in h and y."""
    from mio import _lib
    lib, ops = _lib.lib, _ops()
    T, k, E, d, I = 5, 2, 8, 1040, 80
    route = _route(T, k, E, 5, seed=9)
    idle = torch.diff(route.expert_offsets) == 0
    assert int(idle.sum()) == 3 and ops.moe_up_w8_splits(T, k, E, I, d) > 1
    x, res = _rand((T, d), dtype, seed=1), _rand((T, d), dtype, seed=2)
    st, dt, got = torch.cuda.current_stream().cuda_stream, ops._dtype_id(x), []
    for hostile in (False, True):
        nan = float("nan") if hostile else 0.0
        ws = [torch.full((max(n // 4, 4),), nan, device=DEV) for n in (lib.mio_moe_up_w8_workspace_bytes(T, k, E, I, d, 5),
                                                                      lib.mio_moe_down_w8_workspace_bytes(T, k, E, d, I))]
        (qu, su, bu), (qg, sg, bg), (qd, sd, bd) = w = [_quant(E, N, K, dtype, seed, PAD if hostile else 0) + (_rand((E, N), dtype, 0.5, seed + 10),)
                                                        for seed, (N, K) in enumerate([(I, d), (I, d), (d, I)])]
        for q, s, b in (w if hostile else []):
            q.view(torch.uint8)[idle] = PAD
            s[idle], b[idle] = nan, nan
        h, y = torch.full((T * k + 3, I), nan, dtype=dtype, device=DEV), torch.empty(T, d, dtype=dtype, device=DEV)
        rc = lib.mio_moe_up_w8(_p(x), _p(qu), _p(su), _p(bu), _p(qg), _p(sg), _p(bg), _p(route.expert_offsets), _p(route.sorted_rows), _p(h),
                               _p(ws[0]), T, k, E, I, d, d, qu.stride(1), qu.stride(0), I, 5, dt, st)
        assert rc == 0, lib.mio_last_error().decode()
        rc = lib.mio_moe_down_w8(_p(h), _p(qd), _p(sd), _p(bd), _p(route.ids), _p(route.weights), _p(route.expert_offsets), _p(route.row_pos),
                                 _p(res), _p(y), _p(ws[1]), T, k, E, d, I, I, qd.stride(1), qd.stride(0), d, d, dt, st)
        assert rc == 0, lib.mio_last_error().decode()
        got.append((h[:T * k].clone(), y))
    (h0, y0), (h1, y1) = got
    assert bool(torch.isfinite(h0).all()) and bool(torch.isfinite(y0).all()) and bool(y0.float().abs().max() > 0)
    assert torch.equal(_bits(h0), _bits(h1)) and torch.equal(_bits(y0), _bits(y1))


@pytest.mark.parametrize("dtype", DTYPES)
def test_reruns_and_graph_replay(dtype):
    """Back-to-back launches write the same bytes; route + moe_mlp_w8 captured on one stream replays under a new routing (the logits
    overwritten in place) to the bits of an eager call: the plan consults no device value."""
    ops = _ops()
    T, k, E, d, I = 5, 2, 8, 1040, 80
    x = _rand((T, d), dtype, seed=1)
    (qu, su), (qg, sg), (qd, sd) = _quant(E, I, d, dtype, 1), _quant(E, I, d, dtype, 2), _quant(E, d, I, dtype, 3)
    first = _rand((T, E), dtype, 2.0, 4)
    second = first.roll(3, 1).contiguous()
    assert not torch.equal(ops.moe_route(first, k).ids, ops.moe_route(second, k).ids)
    run = lambda route, out=None: ops.moe_mlp_w8(x, route, qu, su, qd, sd, "swiglu", qg, sg, out=out)  # noqa: E731
    a, b = run(ops.moe_route(first, k)), run(ops.moe_route(first, k))
    assert torch.equal(_bits(a), _bits(b)) and bool(torch.isfinite(a).all())
    logits, out = first.clone(), torch.zeros(T, d, dtype=dtype, device=DEV)
    route = ops.moe_route(logits, k)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up on the capture stream
        run(ops.moe_route(logits, k, out=route), out)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run(ops.moe_route(logits, k, out=route), out)
    for want in (second, first, second):
        logits.copy_(want)
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(out), _bits(run(ops.moe_route(want, k))))


@pytest.mark.parametrize("dtype", DTYPES)
def test_module_fp8_experts(dtype):
    """MoEMLP with expert_weights_fp8 at T 5 and T 70 (two row chunks) against the fp64 chain on the effective weights of the copies
    the module made; after an in-place update of w_down the next forward reads a fresh copy."""
    from mio.kernels.mlp import MoEConfig, MoEMLP
    torch.manual_seed(3)
    m = MoEMLP(272, 144, 8, 2, MoEConfig(dtype=dtype, expert_weights_fp8=True)).to(DEV)
    with torch.no_grad():
        m.router.weight.mul_(8.0)  # logits a few units apart

    def judge(x, res, what):
        y = m(x, res)
        logits = torch.cat([m._router_logits(x[lo:lo + 64], dtype) for lo in range(0, x.shape[0], 64)])
        up, gate, down = (_eff(*m._cast.get_experts_w8(p, dtype)) for p in (m.w_up, m.w_gate, m.w_down))
        mc.check_down(y, mc.composed_reference(x, logits, 2, True, up, down, "swiglu", gate, residual=res, device=DEV)[1], dtype, what)
        return y

    for T in (5, 70):
        judge(_rand((T, 272), dtype, seed=T), _rand((T, 272), dtype, seed=T + 1), f"fp8 module T {T}")
    x = _rand((5, 272), dtype, seed=5)
    y0, s0 = judge(x, None, "before the update").clone(), m._cast.get_experts_w8(m.w_down, dtype)[1].clone()
    with torch.no_grad():
        m.w_down.mul_(-2.0)
    y1 = judge(x, None, "after the update")
    assert torch.equal(m._cast.get_experts_w8(m.w_down, dtype)[1], 2 * s0) and not torch.equal(y1, y0)
    with pytest.raises(ValueError):
        MoEMLP(264, 144, 8, 2, MoEConfig(expert_weights_fp8=True))


@pytest.mark.parametrize("dtype", DTYPES)
def test_quantize_expert_weights(dtype):
    w = _rand((5, 70, 48), dtype, 0.3, 1)
    w[1, 3] = 0.0  # an all-zero row: scale 1.0
    q, s = _ops().quantize_expert_weights_w8(w)
    assert q.dtype == w8c.FP8 and tuple(q.shape) == (5, 70, 48) and s.dtype == torch.float32 and tuple(s.shape) == (5, 70)
    for e in range(5):
        qe, se = _ops().quantize_weight_w8(w[e])
        assert torch.equal(q[e].view(torch.uint8), qe.view(torch.uint8)) and torch.equal(s[e], se)

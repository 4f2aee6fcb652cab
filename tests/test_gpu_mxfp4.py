"""MXFP4 weights (e2m1 nibbles, two per byte; one e8m0 scale byte per 32 k) on the decode-step GEMM (ops.gemm_skinny_w4), its
quantiser (ops.quantize_weight_mxfp4), the MoE decode step (ops.moe_up_w4 / moe_down_w4 / moe_mlp_w4) and the module
(MoEConfig.expert_weights_mxfp4, MoEMLP.load_mxfp4_experts).  The fp64 reference widens the very bytes the kernels read with a
16-entry table and 2.0 ** (b - 127), independent of the project's code; every product e2m1 x 2^e x bf16 is exact in fp32, so the
element bound is the summation's, gamma_K (|x||deq|^T), plus 2^-24 |z| where a bias is added, and the bars are the 16-bit decode
GEMM's (the summation is the same code).  Scale bytes are drawn per block from 107 .. 147: a wrong block-to-scale pairing or
exponent bias moves results by powers of two.  A SwiGLU gate's are drawn from 117 .. 123, which keeps silu's argument within a
few units: silu(z) for z << 0 has the condition number |z|, which the element bound allows for and the bars, measured on
pre-activations of order 1, do not."""
import pytest
import torch

import _gemm_check as gc
import _moe_check as mc
from test_gpu_moe import DEV, FILL, _guarded, _ops, _rand
from test_gpu_moe_w8 import _route

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
BARS = gc.BARS[(BF16, "t128")]
E2M1 = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
_bits = lambda t: t.view(torch.int16)  # noqa: E731


def deq(w4, s):
    """fp64 [..., N, K] of bytes [..., N, K / 2] and scale bytes [..., N, K / 32]: element 2 i in the low nibble of byte i."""
    table = torch.tensor(E2M1 + [-v for v in E2M1], dtype=torch.float64, device=w4.device)
    nib = torch.stack([w4 & 15, w4 >> 4], dim=-1).flatten(-2).long()
    return table[nib] * (2.0 ** (s.double() - 127.0)).repeat_interleave(32, dim=-1)


def reference(x, w4, s, bias=None, act="none", w4g=None, sg=None, bg=None, res=None):
    xf = x.double()
    ax, gam = xf.abs(), gc._gamma(x.shape[-1])

    def pre(q, sc, b):
        wf = deq(q, sc)
        z, tz = xf @ wf.t(), gam * (ax @ wf.abs().t())
        return (z, tz) if b is None else (z + b.double(), tz + gc.EPS32 * (z + b.double()).abs())

    z, tz = pre(w4, s, bias)
    zg, tzg = pre(w4g, sg, bg) if act == "swiglu" else (None, None)
    y, tol = gc._finish(z, tz, act, zg, tzg, None, None if res is None else res.double())
    return gc.Ref(y, tol, x.shape[-1])


GATE = (117, 124)


def _weight(lead, K, seed, ldw=None, lds=None, pad=0xFF, scales=(107, 148)):
    """(w4 [*lead, K / 2], scales [*lead, K / 32]): uniform nibbles, scale bytes 107 .. 147 (GATE: 117 .. 123); with ldw / lds as
    views of rows that many bytes apart whose padding holds `pad`."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    bufq = torch.full((*lead, ldw or K // 2), pad, dtype=torch.uint8, device=DEV)
    bufs = torch.full((*lead, lds or (K // 32 + 3) // 4 * 4), pad, dtype=torch.uint8, device=DEV)
    q, s = bufq[..., :K // 2], bufs[..., :K // 32]
    q.copy_(torch.randint(0, 256, (*lead, K // 2), device=DEV, generator=g, dtype=torch.uint8))
    s.copy_(torch.randint(*scales, (*lead, K // 32), device=DEV, generator=g, dtype=torch.uint8))
    return q, s


def _deep_k(act):
    from mio import _lib
    a = _ops()._ACT[act]
    return (_lib.lib.mio_gemm_skinny_w4_depth(a) + 2) * _lib.lib.mio_gemm_skinny_w4_chunk_k(a) + 32


# M, N, K (or "deep": depth + 2 chunks and a block), act, bias, residual, the plan splits K
GEMM = [(1, 72, 32, "none", False, False, False), (17, 71, 96, "gelu", True, True, False), (64, 1, 160, "swiglu", True, False, False),
        (17, 72, 416, "swiglu", True, True, False), (64, 71, 416, "none", True, True, False), (1, 72, 160, "gelu", False, True, False),
        (64, 72, "deep", "gelu", True, True, False), (64, 71, "deep", "swiglu", False, True, False),
        (17, 72, 2080, "gelu", True, True, True), (5, 71, 1056, "swiglu", True, False, True), (1, 72, 2880, "none", False, False, True)]


@pytest.mark.parametrize("M,N,K,act,bias,res,split", GEMM)
def test_gemm_against_fp64(M, N, K, act, bias, res, split):
    ops, glu = _ops(), act == "swiglu"
    K = _deep_k(act) if K == "deep" else K
    assert (ops.gemm_skinny_w4_splits(M, N, K, act) > 1) == split
    x = _rand((M, K), BF16, seed=K)
    (q, s), (qg, sg) = _weight((N,), K, 1), (_weight((N,), K, 2, scales=GATE) if glu else (None, None))
    b = _rand((N,), BF16, 0.5, 3) if bias else None
    bg = _rand((N,), BF16, 0.5, 4) if bias and glu else None
    r = _rand((M, (N + 7) // 8 * 8), BF16, 1.0, 5)[:, :N] if res else None  # (rows a multiple of 8 elements apart)
    y = ops.gemm_skinny_w4(x, q, s, b, act, qg, sg, bg, r)
    gc.check(y, reference(x, q, s, b, act, qg, sg, bg, r), BF16, "skinny_w4", bars=BARS, what=f"{M}x{N}x{K} {act}")
    if split and not glu:
        assert torch.equal(_bits(ops.gemm_skinny_w4(x, q, s, b, act, residual=r)), _bits(y))  # (no atomics, no arrival order)


def test_gate_scales_over_the_full_range():
    """A SwiGLU gate with scale bytes 107 .. 147 like the up weight's, judged by the element bound alone (module docstring: the
    bars do not allow for silu's condition number at z << 0), one slice and several."""
    ops, N = _ops(), 72
    for M, K in ((17, 416), (5, 1056)):
        x, (q, s), (qg, sg) = _rand((M, K), BF16, seed=K), _weight((N,), K, 1), _weight((N,), K, 2)
        y = ops.gemm_skinny_w4(x, q, s, None, "swiglu", qg, sg)
        gc.check(y, reference(x, q, s, None, "swiglu", qg, sg), BF16, "skinny_w4", bars=False, what=f"wide gate {M}x{N}x{K}")


@pytest.mark.parametrize("act,K", [("gelu", 416), ("swiglu", 2080)])
def test_gemm_in_hostile_memory(act, K):
    """Every operand a view inside a hostile buffer: ldw > K / 2 and lds > K / 32 with 0xff padding (scale 0xff: NaN), the weight and
    scale rows around the N rows 0xff, x rows and columns around the view NaN, the output inside a guard."""
    ops, glu, M, N = _ops(), act == "swiglu", 17, 71
    ldw, lds = K // 2 + 32, (K // 32 + 7) // 4 * 4

    def weight(seed, scales=(107, 148)):
        q, s = _weight((N + 2,), K, seed, ldw, lds, scales=scales)
        q[0], q[-1], s[0], s[-1] = 0xFF, 0xFF, 0xFF, 0xFF
        q, s = q[1:N + 1], s[1:N + 1]
        assert ops._w4_ok(q, "w4") is q and ops._block_scales(s, (N,), K // 32, "s") is s
        return q, s

    (q, s), (qg, sg) = weight(1), (weight(2, GATE) if glu else (None, None))
    xbuf = torch.full((64, K + 8), float("nan"), dtype=BF16, device=DEV)
    x = xbuf[:M, :K]
    x.copy_(_rand((M, K), BF16, seed=7))
    b, r = _rand((N,), BF16, 0.5, 3), _rand((M, N + 9), BF16, 1.0, 5)[:, :N]
    buf, out = _guarded(M, N, BF16)
    y = ops.gemm_skinny_w4(x, q, s, b, act, qg, sg, None, r, out=out)
    gc.check(y, reference(x, q, s, b, act, qg, sg, None, r), BF16, "skinny_w4", guard=buf, fill=FILL, bars=BARS, what=f"hostile {act}")


def _quant_expect(w):
    """The stated rule in plain torch on the CPU: (bytes [N, K / 2], scale bytes [N, K / 32])."""
    N, K = w.shape
    wf = w.detach().cpu().double().reshape(N, K // 32, 32)
    a = torch.where(torch.isnan(wf), torch.zeros_like(wf), wf.abs()).amax(-1)
    e = (torch.frexp(a)[1].double() - 1.0 - 2.0).clamp(-127, 127)  # floor(log2 a) - 2; frexp: a = m 2^ex, m in [0.5, 1)
    e = torch.where(torch.isinf(a), torch.full_like(e, 127.0), torch.where(a == 0, torch.zeros_like(e), e))
    t = torch.ldexp(wf, -e[..., None].to(torch.int32))
    at = torch.where(torch.isnan(t), torch.zeros_like(t), t.abs()).clamp(max=6.0)
    grid, code = torch.tensor(E2M1, dtype=torch.float64), torch.arange(8)
    dist = (at[..., None] - grid).abs()
    tied = dist == dist.amin(-1, keepdim=True)
    pick = torch.where(tied, (code & 1).double(), torch.full_like(dist, 2.0)).argmin(-1)  # of two nearest codes the even one
    nib = (pick + 8 * torch.signbit(wf).long()).reshape(N, K // 2, 2)
    return (nib[..., 0] | (nib[..., 1] << 4)).to(torch.uint8), (e + 127).to(torch.uint8)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_quantize_weight(dtype):
    """Bit-equal to the rule: an all-zero block; blocks whose maximum is exactly +-2^j (j = -3, 0, 5: scale bytes 122, 125, 130)
    and just below 2^j (one bf16 ulp under 1 and under 32: 124, 129), every other element of those blocks under 0.9 x 2^j; the
    ties 2.5 -> 2, 5 -> 4, 0.25 -> 0 (under a block maximum of 5: e = 0); values that saturate (7.5, -7 -> +-6); a NaN, both
    Infs; a strided source."""
    N, K = 6, 96
    w = _rand((N, K + 8), dtype, 1.0, 1)[:, :K]
    assert not w.is_contiguous()
    w[0, 32:64] = 0.0
    w[1, :32] = w[1, :32].clamp(-0.9, 0.9)
    w[1, 3], w[1, 40], w[1, 64:96] = 2.0 ** -3, -(2.0 ** 5) * (1 - 2.0 ** -8), w[1, 64:96].clamp(-3, 3)
    w[2, :32] = torch.tensor([4.0, 2.5, -2.5, 5.0, -5.0, 0.25, -0.25, 0.75, 1.25, 1.75, 3.5, 0.24] + [0.0] * 20, dtype=dtype)
    w[2, 32:64] = torch.tensor([7.5, -7.0, 6.0, 5.5] + [1.0] * 28, dtype=dtype)
    w[3, 5], w[3, 40], w[3, 70] = float("nan"), float("inf"), float("-inf")
    below = 1 - 2.0 ** -8
    for row, maxima in ((4, (2.0 ** -3, -1.0, 2.0 ** 5)), (5, (below, -32.0 * below, 1.0))):
        for b, m in enumerate(maxima):  # the block at 32 b: everything under 0.9 |m| but one element, which is m
            w[row, 32 * b:32 * b + 32] = w[row, 32 * b:32 * b + 32].clamp(-0.9 * abs(m), 0.9 * abs(m))
            w[row, 32 * b + 7 + b] = m
    q, s = _ops().quantize_weight_mxfp4(w)
    assert q.dtype == torch.uint8 and tuple(q.shape) == (N, K // 2) and s.dtype == torch.uint8 and tuple(s.shape) == (N, K // 32)
    eq, es = _quant_expect(w)
    assert torch.equal(s.cpu(), es), (s.cpu(), es)
    assert torch.equal(q.cpu(), eq), int((q.cpu() != eq).sum())
    assert s[0, 1].item() == 127 and int(q[0, 16:32].sum()) == 0 and es[3, 1].item() == 254
    assert es[4].tolist() == [122, 125, 130] and es[5].tolist() == [124, 129, 125]


# ---- the MoE decode step ------------------------------------------------------------------------------------------------------------
E_, K_, D_, I_ = 8, 2, 160, 96  # experts, top_k, d, I: a tail on both GEMMs (160 = 128 + 32, 96 < 128)


@pytest.fixture(scope="module")
def experts():
    """(up, gate, down) of (w4, scales), each expert's rows and scale rows followed by 0xff padding; shared, never written."""
    return [_weight((E_, N), K, seed, K // 2 + 16, (K // 32 + 7) // 4 * 4, scales=GATE if seed == 1 else (107, 148))
            for seed, (N, K) in enumerate([(I_, D_), (I_, D_), (D_, I_)])]


@pytest.mark.parametrize("T", [1, 5, 64])
def test_moe_against_fp64(T, experts):
    ops = _ops()
    (qu, su), (qg, sg), (qd, sd) = experts
    route = _route(T, K_, E_, E_, seed=T)
    x = _rand((T, D_), BF16, seed=T)
    buf, out = _guarded(T * K_, I_, BF16)
    h = ops.moe_up_w4(x, route, qu, su, "swiglu", qg, sg, out=out)
    mc.check_up(h, mc.up_reference(x, route, deq(qu, su), "swiglu", deq(qg, sg), device=DEV), BF16, f"up T {T}", guard=buf, fill=FILL)
    hin, r = _rand((T * K_, I_), BF16, seed=T + 1), _rand((T, D_), BF16, seed=T + 2)
    buf, out = _guarded(T, D_, BF16)
    y = ops.moe_down_w4(hin, route, qd, sd, None, r, out=out)
    mc.check_down(y, mc.down_reference(hin, route, deq(qd, sd), None, r, device=DEV), BF16, f"down T {T}", guard=buf, fill=FILL)


def test_moe_idle_experts_are_not_read(experts):
    """5 of 8 experts routed; the idle experts' weight and scale bytes 0xff (NaN scales): the same finite bits."""
    ops, T = _ops(), 5
    route = _route(T, K_, E_, 5, seed=9)
    idle = torch.diff(route.expert_offsets) == 0
    assert int(idle.sum()) == 3
    x, got = _rand((T, D_), BF16, seed=1), []
    for hostile in (False, True):
        w = [(q.clone(), s.clone()) for q, s in experts]
        for q, s in (w if hostile else []):
            q[idle], s[idle] = 0xFF, 0xFF
        (qu, su), (qg, sg), (qd, sd) = w
        got.append(ops.moe_mlp_w4(x, route, qu, su, qd, sd, "swiglu", qg, sg))
    assert bool(torch.isfinite(got[0]).all()) and bool(got[0].float().abs().max() > 0) and torch.equal(_bits(got[0]), _bits(got[1]))


@pytest.mark.parametrize("K", [160, 1056])
def test_one_expert_is_the_decode_gemm(K):
    """E = 1, top_k = 1: up (SwiGLU, gelu) and down (bias, residual) equal ops.gemm_skinny_w4 bit for bit, one slice and several."""
    ops, T, N = _ops(), 5, 72
    route = ops.moe_route(torch.zeros(T, 1, device=DEV), 1)
    x, b, r = _rand((T, K), BF16, seed=K), _rand((1, N), BF16, 0.5, 3), _rand((T, N), BF16, 1.0, 5)  # (N 72: rows of 8 k)
    (q, s), (qg, sg) = _weight((1, N), K, 1), _weight((1, N), K, 2, scales=GATE)
    assert (ops.gemm_skinny_w4_splits(T, N, K, "gelu") > 1) == (K > 160)
    for act, g in (("swiglu", (qg, sg)), ("gelu", (None, None))):
        assert ops.moe_up_w4_splits(T, 1, 1, N, K, act) == ops.gemm_skinny_w4_splits(T, N, K, act)
        want = ops.gemm_skinny_w4(x, q[0], s[0], b[0], act, *(None if t is None else t[0] for t in g))
        assert torch.equal(_bits(ops.moe_up_w4(x, route, q, s, act, g[0], g[1], b)), _bits(want)), act
    want = ops.gemm_skinny_w4(x, q[0], s[0], b[0], "none", residual=r)
    assert torch.equal(_bits(ops.moe_down_w4(x, route, q, s, b, r)), _bits(want))


def test_moe_graph_replays(experts):
    """moe_mlp_w4 captured on one stream and replayed three times gives the eager call's bits each time."""
    ops, T = _ops(), 5
    (qu, su), (qg, sg), (qd, sd) = experts
    route, x = _route(T, K_, E_, E_, seed=3), _rand((T, D_), BF16, seed=3)
    run = lambda out=None: ops.moe_mlp_w4(x, route, qu, su, qd, sd, "swiglu", qg, sg, out=out)  # noqa: E731
    want, out = run(), torch.zeros(T, D_, dtype=BF16, device=DEV)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):  # warm-up on the capture stream
        run(out)
    torch.cuda.current_stream().wait_stream(st)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run(out)
    for _ in range(3):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(out), _bits(want))


def test_module():
    """MoEMLP with expert_weights_mxfp4 equals ops.moe_mlp_w4 on quantize_expert_weights_mxfp4 of its parameters, to the bit; a
    module that loaded those bytes, the blocks as [E, N, K / 32, 16], gives the same output and holds no 16-bit expert weights."""
    from mio.kernels.mlp import MoEConfig, MoEMLP
    ops = _ops()
    torch.manual_seed(3)
    m = MoEMLP(D_, I_, E_, K_, MoEConfig(expert_weights_mxfp4=True)).to(DEV)
    x = _rand((5, D_), BF16, seed=5)
    y = m(x)
    (qu, su), (qg, sg), (qd, sd) = (ops.quantize_expert_weights_mxfp4(p.detach().to(BF16)) for p in (m.w_up, m.w_gate, m.w_down))
    route = ops.moe_route(m._router_logits(x, BF16), K_, True)
    assert torch.equal(_bits(y), _bits(ops.moe_mlp_w4(x, route, qu, su, qd, sd, "swiglu", qg, sg))) and bool(y.float().abs().max() > 0)
    m2 = MoEMLP(D_, I_, E_, K_, MoEConfig()).to(DEV)
    m2.router.load_state_dict(m.router.state_dict())
    m2.load_mxfp4_experts(qu.view(E_, I_, D_ // 32, 16), su, qg.view(E_, I_, D_ // 32, 16), sg, qd.view(E_, D_, I_ // 32, 16), sd)
    assert m2.w_up is None and torch.equal(_bits(m2(x)), _bits(y)) and not any("mxfp4" in k for k in m2.state_dict())
    m2 = m2.to("cpu").to(DEV)  # (the loaded bytes are buffers: they move with the module)
    assert m2.mxfp4_w4_up.is_cuda and torch.equal(_bits(m2(x)), _bits(y))
    with pytest.raises(ValueError, match="MXFP4 expert bytes"):
        m2.load_from_expert_state_dict({})
    with pytest.raises(ValueError):
        MoEMLP(D_, I_, E_, K_, MoEConfig(expert_weights_mxfp4=True, expert_weights_fp8=True))

"""MXFP4 expert weights on the mixture-of-experts path for tall inputs (ops.moe_up_prefill_w4 / moe_down_prefill_w4 /
moe_mlp_prefill_w4, and MoEMLP after load_mxfp4_experts with MoEConfig(grouped_prefill=True)).  Stage by stage against the fp64
restatement of tests/_moe_check.py on the dequantisation tests/test_gpu_mxfp4.py defines (a 16-entry table and 2.0 ** (b - 127),
independent of the project's code), under the checker's own bounds and bars; and bit for bit against the 16-bit tiled kernel on
the bf16 dequantisation, which the exact widening and the unchanged order of the 32-k steps promise.  d 160 and I 96: up's K is
two chunks of 64 and one MX block, its SwiGLU column tiles are 64 + 32; down's K is a chunk and a block, its N 160 a ragged second
column tile.  Scale bytes are test_gpu_mxfp4._weight's 107 .. 147 (a gate's: GATE), where e2m1 x 2^e is exact in bf16."""
import pytest
import torch

import _moe_check as mc
from test_gpu_moe_prefill import DEV, FILL, _choice, _guarded, _ops, _rand
from test_gpu_mxfp4 import GATE, _bits, _weight, deq

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
D_, I_ = 160, 96


def _experts(E, N, K, seed, scales=(107, 148)):
    """(w4 [E, N, K / 2], scales [E, N, K / 32]) as views with 0xff behind every row (ldw, lds) and behind every expert (a spare row)."""
    q, s = _weight((E, N + 1), K, seed, K // 2 + 16, (K // 32 + 7) // 4 * 4, scales=scales)
    q[:, N], s[:, N] = 0xFF, 0xFF
    return q[:, :N], s[:, :N]


def _all_experts(E):
    return _experts(E, I_, D_, 1), _experts(E, I_, D_, 2, GATE), _experts(E, D_, I_, 3)


@pytest.mark.parametrize("routing", ["partial", "full", "exact"])
def test_up_and_down_against_fp64(routing):
    """Each stage from the bytes it read: SwiGLU up into a guarded h, down with bias and residual into a guarded y."""
    ops = _ops()
    T, k, E, logits = _choice(routing)
    route = ops.moe_route_prefill(logits, k)
    (qu, su), (qg, sg), (qd, sd) = _all_experts(E)
    x = _rand((T, D_), BF16, seed=3)
    buf, out = _guarded(T * k, I_, BF16)
    h = ops.moe_up_prefill_w4(x, route, qu, su, "swiglu", qg, sg, out=out)
    mc.check_up(h, mc.up_reference(x, route, deq(qu, su), "swiglu", deq(qg, sg), device=DEV), BF16, f"up {routing}", guard=buf, fill=FILL)
    hin, bd, res = _rand((T * k, I_), BF16, seed=4), _rand((E, D_), BF16, 0.5, 5), _rand((T, D_), BF16, seed=6)
    buf, out = _guarded(T, D_, BF16)
    y = ops.moe_down_prefill_w4(hin, route, qd, sd, bd, res, out=out)
    mc.check_down(y, mc.down_reference(hin, route, deq(qd, sd), bd, res, device=DEV), BF16, f"down {routing}", guard=buf, fill=FILL)


def test_one_block_plain():
    """K 32: a single MX block, half a chunk; no gate, a bias, N 72 a partial column tile.  The activation is "none": with scale
    bytes over 107 .. 147 the pre-activations span 2^-20 .. 2^20, and the checker's bars, measured on pre-activations of order 1,
    do not allow for gelu's condition number at z << 0 (test_gpu_mxfp4's docstring says the same of silu); gelu on these weights
    is held to the 16-bit kernel's bits below."""
    ops = _ops()
    T, k, E, logits = _choice("partial")
    route = ops.moe_route_prefill(logits, k)
    (q, s), x, b = _experts(E, 72, 32, 7), _rand((T, 32), BF16, seed=8), _rand((E, 72), BF16, 0.5, 9)
    buf, out = _guarded(T * k, 72, BF16)
    h = ops.moe_up_prefill_w4(x, route, q, s, "none", b_up=b, out=out)
    mc.check_up(h, mc.up_reference(x, route, deq(q, s), "none", None, b, device=DEV), BF16, "K 32", guard=buf, fill=FILL)


def test_bit_equal_to_the_16_bit_tiled_kernel():
    """On the `full` routing: SwiGLU up, plain up with a bias and down with a residual equal moe_up_prefill / moe_down_prefill on
    deq(...) in bf16, which pins the staging map, the nibble order and the scale indexing at once."""
    ops = _ops()
    T, k, E, logits = _choice("full")
    route = ops.moe_route_prefill(logits, k)
    (qu, su), (qg, sg), (qd, sd) = _all_experts(E)
    wu, wg, wd = (deq(q, s).to(BF16) for q, s in ((qu, su), (qg, sg), (qd, sd)))
    x, hin = _rand((T, D_), BF16, seed=3), _rand((T * k, I_), BF16, seed=4)
    b, res = _rand((E, I_), BF16, 0.5, 5), _rand((T, D_), BF16, seed=6)
    pairs = [(ops.moe_up_prefill_w4(x, route, qu, su, "swiglu", qg, sg), ops.moe_up_prefill(x, route, wu, "swiglu", wg)),
             (ops.moe_up_prefill_w4(x, route, qu, su, "gelu", b_up=b), ops.moe_up_prefill(x, route, wu, "gelu", b_up=b)),
             (ops.moe_down_prefill_w4(hin, route, qd, sd, residual=res), ops.moe_down_prefill(hin, route, wd, residual=res))]
    for i, (got, want) in enumerate(pairs):
        assert bool(want.float().abs().max() > 0) and torch.equal(_bits(got), _bits(want)), i


def test_idle_experts_are_not_read():
    """The `exact` routing leaves expert 1 without a row; its nibbles and scale bytes 0xff (NaN scales): the same finite bits."""
    ops = _ops()
    T, k, E, logits = _choice("exact")
    route = ops.moe_route_prefill(logits, k)
    idle = route.expert_offsets.diff() == 0
    assert int(idle.sum()) == 1
    x, got = _rand((T, D_), BF16, seed=1), []
    for hostile in (False, True):
        w = [(q.clone(), s.clone()) for q, s in _all_experts(E)]
        for q, s in (w if hostile else []):
            q[idle], s[idle] = 0xFF, 0xFF
        (qu, su), (qg, sg), (qd, sd) = w
        got.append(ops.moe_mlp_prefill_w4(x, route, qu, su, qd, sd, "swiglu", qg, sg))
    assert bool(torch.isfinite(got[0]).all()) and bool(got[0].float().abs().max() > 0) and torch.equal(_bits(got[0]), _bits(got[1]))


def test_graph_replays_under_new_routing():
    """moe_route_prefill + moe_mlp_prefill_w4 captured once; the logits are rewritten in place between replays (8 experts with 50
    rows each, then experts 1 and 3 with 200 each), and every replay equals the eager call on the logits at hand."""
    import _moe_cases as cs
    ops = _ops()
    T, E, k = 200, 8, 2
    (qu, su), (qg, sg), (qd, sd) = _all_experts(E)
    x, t = _rand((T, D_), BF16, seed=1), torch.arange(T)
    first = cs.logits_for(torch.stack([t % E, (t + 1) % E], 1), E).to(DEV)
    second = cs.logits_for(torch.tensor([1, 3]).expand(T, k).contiguous(), E).to(DEV)
    logits = first.clone()
    route, out = ops.moe_route_prefill(logits, k), torch.zeros(T, D_, dtype=BF16, device=DEV)
    run = lambda: ops.moe_mlp_prefill_w4(x, ops.moe_route_prefill(logits, k, out=route), qu, su, qd, sd, "swiglu", qg, sg, out=out)  # noqa: E731
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):  # warm-up on the capture stream
        run()
    torch.cuda.current_stream().wait_stream(st)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    for want in (second, first, second):
        logits.copy_(want)
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        eager = ops.moe_mlp_prefill_w4(x, ops.moe_route_prefill(want, k), qu, su, qd, sd, "swiglu", qg, sg)
        assert bool(torch.isfinite(out).all()) and torch.equal(_bits(out), _bits(eager))


def test_module_prefill_on_loaded_bytes():
    """MoEMLP(grouped_prefill=True) after load_mxfp4_experts: T 200 is moe_route_prefill + moe_mlp_prefill_w4 on the loaded bytes,
    T 5 is moe_route + moe_mlp_w4 as before, both to the bit."""
    from mio.kernels.mlp import MoEConfig, MoEMLP
    ops = _ops()
    E, k = 8, 2
    torch.manual_seed(3)
    m = MoEMLP(D_, I_, E, k, MoEConfig(grouped_prefill=True)).to(DEV)
    (qu, su), (qg, sg), (qd, sd) = (_weight((E, I_), D_, 1), _weight((E, I_), D_, 2, scales=GATE), _weight((E, D_), I_, 3))
    m.load_mxfp4_experts(qu, su, qg, sg, qd, sd)
    for T, route_op, mlp_op in ((200, ops.moe_route_prefill, ops.moe_mlp_prefill_w4), (5, ops.moe_route, ops.moe_mlp_w4)):
        x = _rand((T, D_), BF16, seed=T)
        want = mlp_op(x, route_op(m._router_logits(x, BF16), k, True), qu, su, qd, sd, "swiglu", qg, sg)
        assert bool(want.float().abs().max() > 0) and torch.equal(_bits(m(x)), _bits(want)), T

"""The host side of the mixture-of-experts decode step, without a GPU: the C ABI's symbols and refusals, the plan of
csrc/moe_plan.h through its host queries, what the GPU case tables of tests/_moe_cases.py reach under that plan, the module's
weight loader and the tie / degenerate-row semantics of the fp64 restatement."""
import math
import os
import re

import pytest
import torch

import _moe_cases as cs
import _moe_check as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["mio_moe_route", "mio_moe_up_splits", "mio_moe_up_workspace_bytes", "mio_moe_down_splits", "mio_moe_down_workspace_bytes",
           "mio_moe_up", "mio_moe_down"]
A = 0x1000  # a dummy 16-byte aligned address: every refusal comes before any launch, nothing is dereferenced


def _lib():
    from mio import _lib
    return _lib


def _err():
    return _lib().lib.mio_last_error().decode()


def test_symbols_declared_and_bound():
    lib = _lib()
    header = open(os.path.join(ROOT, "include", "mio_hip.h")).read()
    for s in SYMBOLS:
        assert re.search(r"\b%s\(" % s, header), f"{s} is not declared in include/mio_hip.h"
        assert s in lib.EXPORTS and hasattr(lib.lib, s)
    assert lib.lib.mio_version() == 106
    from mio import ops
    from mio.kernels.mlp import MoEConfig, MoEMLP  # noqa: F401
    for name in ("moe_route", "moe_up", "moe_down", "moe_mlp", "MoERoute", "moe_up_splits", "moe_down_splits"):
        assert hasattr(ops, name)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def _route(**kw):
    a = dict(logits=A, ld=8, ids=A, weights=A, offsets=A, sorted_rows=A, row_pos=A, T=4, E=8, k=2, renorm=1, dtype=0)
    a.update(kw)
    return _lib().lib.mio_moe_route(a["logits"], a["ld"], a["ids"], a["weights"], a["offsets"], a["sorted_rows"], a["row_pos"], a["T"],
                                    a["E"], a["k"], a["renorm"], a["dtype"], None)


def _up(**kw):
    a = dict(x=A, w=A, b=None, wg=A, bg=None, off=A, srt=A, h=A, ws=A, T=4, k=2, E=8, I=72, d=1032, ldx=1032, ldw=1032,
             es=72 * 1032, ldh=72, act=5, dtype=0)
    a.update(kw)
    return _lib().lib.mio_moe_up(a["x"], a["w"], a["b"], a["wg"], a["bg"], a["off"], a["srt"], a["h"], a["ws"], a["T"], a["k"], a["E"],
                                 a["I"], a["d"], a["ldx"], a["ldw"], a["es"], a["ldh"], a["act"], a["dtype"], None)


def _down(**kw):
    a = dict(h=A, w=A, b=None, ids=A, wts=A, off=A, pos=A, res=None, y=A, ws=A, T=4, k=2, E=8, d=40, I=72, ldh=72, ldw=72, es=40 * 72,
             ldy=40, ldr=40, dtype=0)
    a.update(kw)
    return _lib().lib.mio_moe_down(a["h"], a["w"], a["b"], a["ids"], a["wts"], a["off"], a["pos"], a["res"], a["y"], a["ws"], a["T"],
                                   a["k"], a["E"], a["d"], a["I"], a["ldh"], a["ldw"], a["es"], a["ldy"], a["ldr"], a["dtype"], None)


REFUSALS = [
    (_route, dict(T=65), "decode steps only"), (_route, dict(E=0), "E must be"), (_route, dict(E=257, ld=257), "E must be"),
    (_route, dict(k=0), "top_k"), (_route, dict(k=9, E=16, ld=16), "top_k"), (_route, dict(k=4, E=3), "top_k"),
    (_route, dict(ld=7), "ld < E"), (_route, dict(dtype=3), "dtype"), (_route, dict(logits=A + 2), "aligned"),
    (_route, dict(ids=A + 2), "aligned"), (_route, dict(row_pos=None), "null"), (_route, dict(T=-1), "negative"),
    (_up, dict(T=65), "decode steps only"), (_up, dict(E=300), "E must be"), (_up, dict(k=9), "top_k"), (_up, dict(d=1036, ldx=1040, ldw=1040), "K must be a multiple of 8"),
    (_up, dict(ldw=1024), "row stride smaller"), (_up, dict(ldw=1036), "multiples of 8"), (_up, dict(ldx=1028), "multiples of 8"),
    (_up, dict(ldh=64), "row stride smaller"), (_up, dict(es=72 * 1032 - 8), "expert_stride"), (_up, dict(es=72 * 1032 + 4), "multiples of 8"),
    (_up, dict(x=A + 8), "aligned"), (_up, dict(w=A + 2), "aligned"), (_up, dict(srt=A + 2), "aligned"), (_up, dict(wg=None), "w_gate"),
    (_up, dict(act=0), "w_gate"), (_up, dict(act=0, wg=None, bg=A), "b_gate"), (_up, dict(ws=None), "workspace required"),
    (_up, dict(dtype=2), "dtype"), (_up, dict(act=6), "activation"), (_up, dict(h=None), "non-null"),
    (_down, dict(T=65), "decode steps only"), (_down, dict(E=0), "E must be"), (_down, dict(k=3, E=2), "top_k"),
    (_down, dict(I=76, ldh=80, ldw=80, es=40 * 80), "K must be a multiple of 8"), (_down, dict(ldw=64), "row stride smaller"),
    (_down, dict(ldy=36), "multiples of 8"), (_down, dict(ldy=32), "row stride smaller"), (_down, dict(res=A, ldr=32), "ldr"),
    (_down, dict(res=A, ldr=44), "ldr"), (_down, dict(es=40 * 72 - 8), "expert_stride"), (_down, dict(y=A + 4), "aligned"),
    (_down, dict(wts=A + 1), "aligned"), (_down, dict(ws=None), "workspace required"), (_down, dict(dtype=2), "dtype"),
    (_down, dict(ids=None), "non-null"),
]


@pytest.mark.parametrize("i", range(len(REFUSALS)))
def test_refusals_before_any_launch(i):
    """Every refusal of include/mio_hip.h through the C ABI with dummy aligned pointers: < 0 and a message that names the entry
    point and the reason; nothing is launched, so no GPU is needed."""
    fn, kw, text = REFUSALS[i]
    assert fn(**kw) < 0, (fn.__name__, kw)
    name = {"_route": "mio_moe_route", "_up": "mio_moe_up", "_down": "mio_moe_down"}[fn.__name__]
    assert _err().startswith(name + ":") and text in _err(), (kw, _err())


def test_empty_calls_and_queries():
    lib = _lib().lib
    assert _route(T=0, logits=None, ids=None, weights=None, offsets=None, sorted_rows=None, row_pos=None) == 0
    assert _up(T=0, x=None, h=None, off=None, srt=None, ws=None) == 0
    assert _down(T=0, h=None, y=None, ids=None, wts=None, off=None, pos=None, ws=None) == 0
    assert lib.mio_moe_up_splits(65, 2, 8, 72, 40, 5) < 0 and "decode steps only" in _err()
    assert lib.mio_moe_down_splits(4, 2, 8, 72, 36) < 0 and "multiple of 8" in _err()
    assert lib.mio_moe_up_workspace_bytes(4, 9, 8, 72, 40, 5) == 0 and "top_k" in _err()
    assert lib.mio_moe_down_workspace_bytes(4, 2, 0, 72, 40) == 0 and "E must be" in _err()
    from mio import ops
    with pytest.raises(ValueError):
        ops.moe_up_splits(65, 2, 8, 72, 40)
    with pytest.raises(ValueError):
        ops.moe_route(torch.zeros(4, 8), 2)  # a CPU tensor: there is no fallback


# ---- the plan ----------------------------------------------------------------------------------------------------------------------
SWEEP = [(T, k, E, N) for T in (1, 4, 17, 64) for k, E in ((1, 1), (2, 8), (4, 60), (8, 128), (8, 256), (1, 256))
         for N in (1, 72, 136, 1000, 14336)]


@pytest.mark.parametrize("act", [0, 5])
def test_plan_properties(act):
    """Over a sweep of (T, k, E, N, K, act): slices of whole 32-k steps, none empty, covering [0, K), lengths at most one step apart,
    the count never falling as K grows, the slice at least the stated minimum (8 x the mean rows per aimed expert), and the
    workspace bytes the stated formulas.  The plan reads no device value: the queries take sizes only."""
    lib = _lib().lib
    for T, k, E, N in SWEEP:
        aimed = max(1, min(E, T * k))
        min_len = max(32, (8 * -(-T * k // aimed) + 31) // 32 * 32)
        last = 0
        for K in (0, 8, 32, 40, 64, 264, 1032, 2048, 4096, 14336):
            ns = lib.mio_moe_up_splits(T, k, E, N, K, act)
            assert ns >= 1 and ns == lib.mio_moe_down_splits(T, k, E, N, K), (T, k, E, N, K)
            assert ns >= last, f"the split count fell as K grew: {(T, k, E, N, K)} {ns} < {last}"
            last = ns
            sl = cs.slices(K, ns)
            assert sl[0][0] == 0 and sl[-1][1] == K and all(a[1] == b[0] for a, b in zip(sl, sl[1:]))
            if K:
                assert all(e > b and b % 32 == 0 for b, e in sl) and all(e % 32 == 0 for _, e in sl[:-1])
                steps = [-(-(e - b) // 32) for b, e in sl]
                assert max(steps) - min(steps) <= 1
            if ns > 1:
                assert K // ns >= min_len - 31 and ns <= -(-512 // (aimed * -(-N // 64))), (T, k, E, N, K, ns)
            glu = 2 if act == 5 else 1
            assert lib.mio_moe_up_workspace_bytes(T, k, E, N, K, act) == (0 if ns == 1 else ns * T * k * N * 4 * glu)
            assert lib.mio_moe_down_workspace_bytes(T, k, E, N, K) == ns * T * k * N * 4


def test_case_tables_reach_the_seams():
    """What tests/test_gpu_moe.py relies on, asserted here so that a retune of the plan fails on the CPU: every case's split /
    unsplit claim and chunk count, one slice and several per activation, slices of 3, 4 and >= 5 chunks plain and SwiGLU, partial
    rows with N % 4 != 0, K % 32 == 8 and K 8, every required count of rows per expert, and an idle expert in every hostile case."""
    from mio import ops
    lib = _lib().lib
    for name, table in cs.ALL_TABLES.items():
        for c in table:
            ns = lib.mio_moe_up_splits(c.T, c.k, c.E, c.N, c.K, ops._ACT[c.act])
            assert ns >= 1, (name, c.what, _err())
            if name != "ROWS":
                assert (ns > 1) == c.split, (name, c.what, ns)
            if c.chunks is not None:
                assert cs.max_chunks(c.K, ns, c.glu) == c.chunks, (c.what, ns, cs.max_chunks(c.K, ns, c.glu))
    for act in cs.ACTS:
        assert {c.split for c in cs.EVERY_ACTIVATION if c.act == act} == {True, False}
    for glu in (False, True):
        assert {min(c.chunks, 5) for c in cs.DEEP if c.glu == glu} == {3, 4, 5}
        assert any(c.chunks >= 5 for c in cs.DEEP_UNSPLIT if c.glu == glu)
    assert all(c.K <= cs.DEEP_LDW for c in cs.DEEP) and any(c.K < cs.DEEP_LDW for c in cs.DEEP)  # prefixes: ldw > K
    assert {c.N for c in cs.N_EDGES} == {1, 15, 72, 1000} and any(c.N % 4 and c.split for c in cs.N_EDGES)
    assert any(c.K % 32 == 8 and c.split for c in cs.N_EDGES) and any(c.K == 8 for c in cs.N_EDGES)
    counts = torch.bincount(cs.mixed_choice().reshape(-1), minlength=cs.MIXED["E"]).tolist()
    assert tuple(counts) == cs.MIXED_COUNTS and {0, 1, 15, 16, 17, 33, 64} <= set(counts)
    for c in cs.ROWS + cs.HOSTILE + cs.N_EDGES + cs.EVERY_ACTIVATION + cs.DOWN_OPTIONS:
        ch = cs.choice_of(c)
        assert ch.shape == (c.T, c.k) and (c.k == 1 or bool((ch.sort(1).values.diff(dim=1) > 0).all())), c.what  # distinct experts
    for c in cs.HOSTILE:
        assert len(set(cs.choice_of(c).reshape(-1).tolist())) < c.E, f"hostile case {c.what} has no idle expert"
    assert {(c.routing, c.T, c.E) for c in cs.ROWS} >= {("mixed", 64, 10), ("same", 64, 8), ("random", 1, 256)}
    # the routing the logits builder writes is the routing asked for
    ch = cs.mixed_choice()
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        assert torch.equal(mc.route_reference(cs.logits_for(ch, 10, dtype), 3, True).ids, ch)


def test_hostile_fill_reaches_the_idle_experts():
    """The hostile-memory test's operands, built on the CPU: after fill() and poison_idle() every element of the idle experts'
    weights and biases holds NaN (0xFF bytes) or +-finfo.max / 8, the active experts hold the value, the padding around the view is
    poisoned too, and untouched() holds against the retaken snapshot.  Embedded.fill() alone leaves the idle experts' finite
    values in place: that is asserted as well, so the step cannot silently become redundant or be dropped."""
    import _hostile_gemm as hg
    for c in cs.HOSTILE:
        active = torch.zeros(c.E, dtype=torch.bool)
        active[cs.choice_of(c).reshape(-1)] = True
        assert bool(active.any()) and not bool(active.all())
        own = lambda shape: torch.arange(int(torch.tensor(shape).prod())).view(shape)[active].reshape(-1)  # noqa: E731
        for dtype in (torch.bfloat16, torch.float16):
            N, K = 24, 16
            w = hg.Embedded(torch.randn(c.E, N, K).to(dtype), (c.E, N + 1, K + 16), seed=1, own_index=own((c.E, N, K)))
            b = hg.Embedded(torch.randn(c.E, N).to(dtype), (c.E + 2, N), (1, 0), seed=2, own_index=own((c.E, N)))
            for fill in hg.FILLS:
                for t in (w, b):
                    t.fill(fill)
                    if fill != "benign":
                        assert not cs.idle_is_hostile(t, active, fill)   # fill() alone: the idle experts keep their finite values
                    idle = cs.poison_idle(t, active, fill)
                    assert cs.idle_is_hostile(t, active, fill), (c.what, fill, dtype)
                    assert int(idle.sum()) == int((~active).sum()) * t.value[0].numel()
                    assert t.untouched()
                    outside = torch.ones_like(t.owned)
                    outside[t.idx] = False
                    pad = t.buf[outside].float()
                    if fill == "nan":
                        assert bool(torch.isnan(pad).all())
                    elif fill == "huge":
                        assert bool((pad.abs() == float(torch.finfo(dtype).max / 8)).all())
                    hg.bits(t.buf.view(-1))[0] ^= 1  # and a changed bit is seen
                    assert not t.untouched()


# ---- the module's loader -------------------------------------------------------------------------------------------------------------
def test_load_from_expert_state_dict_round_trips():
    from mio.kernels.mlp import MoEConfig, MoEMLP
    E, d, I = 4, 16, 24
    g = torch.Generator().manual_seed(0)
    sd = {"model.layers.0.block_sparse_moe.gate.weight": torch.randn(E, d, generator=g)}
    for e in range(E):
        for n, shape in (("w1", (I, d)), ("w3", (I, d)), ("w2", (d, I))):
            sd[f"model.layers.0.block_sparse_moe.experts.{e}.{n}.weight"] = torch.randn(*shape, generator=g)
    m = MoEMLP(d, I, E, 2)
    v0 = m.w_down._version
    m.load_from_expert_state_dict(sd, prefix="model.layers.0.block_sparse_moe.")
    assert m.w_down._version > v0  # an in-place update: the cast cache sees it
    assert torch.equal(m.router.weight, sd["model.layers.0.block_sparse_moe.gate.weight"])
    for e in range(E):
        pre = f"model.layers.0.block_sparse_moe.experts.{e}."
        assert torch.equal(m.w_gate[e], sd[pre + "w1.weight"]) and torch.equal(m.w_up[e], sd[pre + "w3.weight"])
        assert torch.equal(m.w_down[e], sd[pre + "w2.weight"])
    assert tuple(m.w_up.shape) == (E, I, d) and tuple(m.w_down.shape) == (E, d, I)
    # another key layout, and a module without a gate
    q = {"mlp.gate.weight": sd["model.layers.0.block_sparse_moe.gate.weight"]}
    for e in range(E):
        q[f"mlp.experts.{e}.up_proj.weight"] = sd[f"model.layers.0.block_sparse_moe.experts.{e}.w3.weight"]
        q[f"mlp.experts.{e}.down_proj.weight"] = sd[f"model.layers.0.block_sparse_moe.experts.{e}.w2.weight"]
    m2 = MoEMLP(d, I, E, 2, MoEConfig(activation="gelu", renormalize=False))
    assert m2.w_gate is None
    m2.load_from_expert_state_dict(q, prefix="mlp.", names=("gate_proj", "up_proj", "down_proj"))
    assert torch.equal(m2.w_up, m.w_up) and torch.equal(m2.w_down, m.w_down)
    with pytest.raises(ValueError):
        MoEMLP(d, I + 8, E, 2).load_from_expert_state_dict(sd, prefix="model.layers.0.block_sparse_moe.")
    with pytest.raises(KeyError):
        m.load_from_expert_state_dict(sd, prefix="nowhere.")
    with pytest.raises(ValueError):
        MoEMLP(d, I, 4, 5)
    with pytest.raises(ValueError):
        m(torch.zeros(2, d))  # a CPU tensor: there is no fallback


# ---- the semantics, on the fp64 restatement -----------------------------------------------------------------------------------------
def test_ties_and_degenerate_rows():
    inf, nan = math.inf, math.nan
    x = torch.tensor([[1.0, 1.0, 1.0, 1.0],        # all equal: the lowest indices
                      [0.0, 2.0, 2.0, 2.0],        # a tie straddling the k-th place
                      [nan, nan, nan, nan],        # no finite logit
                      [-inf, -inf, -inf, -inf],
                      [nan, 3.0, -inf, 3.0],       # NaN counts as -inf
                      [inf, 1.0, inf, 0.0],        # +inf: the largest finite fp32, ties by index
                      [-0.0, 0.0, -1.0, -2.0]])    # -0 == +0: a tie
    for renorm in (True, False):
        r = mc.route_reference(x, 2, renorm)
        assert r.ids.tolist() == [[0, 1], [1, 2], [0, 1], [0, 1], [1, 3], [0, 2], [0, 1]]
        assert bool((r.weights[2:4] == 0).all()) and bool((r.allow[2:4] == 0).all()) and bool(torch.isfinite(r.weights).all())
        assert torch.allclose(r.weights[0], torch.full((2,), 0.5 if renorm else 0.25, dtype=torch.float64))
        assert torch.allclose(r.weights[5], torch.full((2,), 0.5, dtype=torch.float64))  # exp(1 - FLT_MAX) = 0
        assert torch.allclose(r.weights[4], torch.full((2,), 0.5, dtype=torch.float64))
        if renorm:
            assert torch.allclose(r.weights[[0, 1, 4, 5, 6]].sum(1), torch.ones(5, dtype=torch.float64))
    r = mc.route_reference(x, 2, True)
    assert r.offsets.tolist() == [0, 5, 11, 13, 14] and r.offsets[-1] == x.shape[0] * 2
    assert r.sorted_rows.tolist() == [0, 4, 6, 10, 12, 1, 2, 5, 7, 8, 13, 3, 11, 9]
    assert torch.equal(r.sorted_rows[r.row_pos], torch.arange(14))
    one = mc.route_reference(torch.tensor([[nan]]), 1, True)   # E 1: the single expert, weight 0 on a degenerate row
    assert one.ids.tolist() == [[0]] and one.weights.tolist() == [[0.0]]
    assert mc.route_reference(torch.tensor([[-3.0]]), 1, False).weights.tolist() == [[1.0]]

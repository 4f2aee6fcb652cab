"""CPU tests of the parallel-layer checker (tests/_parallel_check.py): the placement maps; the loopback against full attention in
fp64 and, bit for bit, against real gloo ranks; the routes of every case of tests/test_gpu_parallel_rows.py; the tensor-parallel
form of _module_check.model; and every planted fault refused by the judgement at the case shapes in both dtypes.

The planted faults run at the cases' own S, H and D with fewer batches (ring: B = 1 of 2; modules: 3 of hd64's 63 sequences), so
that the fp64 reference and model stay within seconds on the CPU; a fault's size per row does not depend on the batch count."""
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import _cpu_local
import _module_check as mc
import _parallel_check as pc

BF, FP = mc.BF, mc.FP
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = pytest.mark.parametrize("dtype", [BF, FP], ids=["bf16", "fp16"])


# ---- placement -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sp", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("zigzag", [False, True], ids=["contiguous", "zigzag"])
def test_positions_are_a_bijection_and_match_the_product(sp, zigzag):
    from mio.parallelism.sequence_parallel import zigzag_shard, zigzag_unshard
    Sl = 12
    S = sp * Sl
    pos = [pc.positions(r, sp, Sl, zigzag) for r in range(sp)]
    assert torch.equal(torch.cat(pos).sort().values, torch.arange(S))
    for r in range(sp):
        rr, ll = pc.local_of(pos[r], sp, Sl, zigzag)
        assert torch.equal(rr, torch.full((Sl,), r)) and torch.equal(ll, torch.arange(Sl))
    rr, ll = pc.local_of(torch.arange(S), sp, Sl, zigzag)
    assert all(int(pos[int(a)][int(b)]) == i for i, (a, b) in enumerate(zip(rr, ll)))
    x = torch.arange(2 * S * 3, dtype=torch.float32).view(2, S, 3)
    shards = [pc.shard(x, r, sp, zigzag) for r in range(sp)]
    for r in range(sp):
        want = zigzag_shard(x, r, sp, 1) if zigzag else x[:, r * Sl:(r + 1) * Sl]
        assert torch.equal(shards[r], want)
    assert torch.equal(pc.place(shards, sp, zigzag), x)
    if zigzag:
        assert torch.equal(zigzag_unshard(shards, sp, 1), x)


# ---- loopback against full attention -------------------------------------------------------------------------------------------
def _fp64_carry():
    """A steps() hook that gives the stand-in kernel an fp64 shadow of every carry buffer.  The product's carry is fp32
    (ring_attention allocates it), which alone costs 1e-7; what this test measures is the transport and the schedule."""
    shadow = {}

    def hook(i, q, k, v, kw, launch):
        for name in ("o_acc", "lse"):
            t = kw[name]
            if id(t) not in shadow:
                shadow[id(t)] = (t, t.double())
            kw[name] = shadow[id(t)][1]
    return hook


LOOP_FORMS = [("noncausal", False, False, False), ("causal", True, False, False), ("zigzag", True, True, False),
              ("mask", False, False, True)]


@pytest.mark.parametrize("sp", [2, 3, 4, 8])
@pytest.mark.parametrize("exchange", ["mesh", "ring"])
@pytest.mark.parametrize("form,causal,zigzag,mask", LOOP_FORMS, ids=[f[0] for f in LOOP_FORMS])
def test_loopback_reproduces_full_attention(monkeypatch, sp, exchange, form, causal, zigzag, mask):
    _cpu_local.install(monkeypatch)
    g = torch.Generator().manual_seed(sp * 10 + len(form))
    B, H, Hkv, D, Sl = 2, 4, 2, 8, 16
    S = sp * Sl
    Sk = S if causal else sp * 10
    q = torch.randn(B, S, H, D, generator=g, dtype=torch.float64) * 2.0
    k, v = (torch.randn(B, Sk, Hkv, D, generator=g, dtype=torch.float64) for _ in range(2))
    add = None
    if mask:
        add = torch.randn(B, 1, S, Sk, generator=g, dtype=torch.float64)
        add[1, :, :, Sk - 7:] = float("-inf")
    ref, lse = pc.ring_reference(q, k, v, causal=causal, additive_mask=add)
    assert torch.isfinite(lse).all()
    for layout in ("bshd", "bhsd"):
        out, recs = pc.run_ring(q, k, v, sp, layout=layout, causal=causal, zigzag=zigzag, exchange=exchange, additive_mask=add,
                                route=False, hook=lambda r: _fp64_carry())
        assert out.dtype == torch.float64 and (out - ref).abs().max().item() < 1e-12, (layout, (out - ref).abs().max().item())
        assert all(len(c) >= 1 for c in recs) and all(sum(s["write_out"] for s in c) == (2 if zigzag else 1) for c in recs)
        if not causal:
            assert all(len(c) == sp for c in recs)


# ---- loopback against gloo -----------------------------------------------------------------------------------------------------
GLOO_FORMS = [("mesh", False, False, False, "bshd"), ("ring", True, False, False, "bhsd"), ("mesh", True, True, False, "bhsd"),
              ("ring", True, True, False, "bshd"), ("ring", False, False, True, "bshd"), ("mesh", False, False, True, "bhsd")]


def _gloo_inputs(sp, i):
    g = torch.Generator().manual_seed(100 * sp + i)
    B, H, D, S = 2, 2, 8, 16 * sp
    q, k, v = (torch.randn(B, S, H, D, generator=g) for _ in range(3))
    return q, k, v, torch.randn(B, 1, S, S, generator=g)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _gloo_worker(rank, world, port, outdir):
    for p in (ROOT, os.path.join(ROOT, "ml-inference-optimizer_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    torch.set_grad_enabled(False)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from mio.parallelism.sequence_parallel import ring_attention
        _cpu_local.install()
        pairs = [dist.new_group([0, 1]), dist.new_group([2, 3])]
        result = {}
        for sp, group, r in ((4, None, rank), (2, pairs[rank // 2], rank % 2)):
            for i, (exchange, causal, zigzag, mask, layout) in enumerate(GLOO_FORMS):
                q, k, v, add = _gloo_inputs(sp, i)
                loc = [pc.shard(t, r, sp, zigzag) for t in (q, k, v)]
                loc = [(t.permute(0, 2, 1, 3) if layout == "bhsd" else t).contiguous() for t in loc]
                addl = pc.shard(add, r, sp, zigzag, dim=2).contiguous() if mask else None
                result[(sp, i, r)] = ring_attention(*loc, group, layout=layout, causal=causal, zigzag=zigzag, exchange=exchange,
                                                    additive_mask=addl)
        torch.save(result, os.path.join(outdir, f"rank{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_loopback_equals_gloo_bit_for_bit(monkeypatch, tmp_path):
    """One spawn of four gloo ranks: sp = 4 on the world, sp = 2 on the pairs (0, 1) and (2, 3).  The loopback with the same
    stand-in kernels gives the same bytes: it is a transport and nothing else."""
    mp.spawn(_gloo_worker, args=(4, _free_port(), str(tmp_path)), nprocs=4, join=True)
    got = [torch.load(os.path.join(str(tmp_path), f"rank{r}.pt")) for r in range(4)]
    _cpu_local.install(monkeypatch)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)   # as the ranks ran
    try:
        _compare_with_loopback(got)
    finally:
        torch.set_num_threads(threads)


def _compare_with_loopback(got):
    for sp in (4, 2):
        for i, (exchange, causal, zigzag, mask, layout) in enumerate(GLOO_FORMS):
            q, k, v, add = _gloo_inputs(sp, i)
            out, _ = pc.run_ring(q, k, v, sp, layout=layout, causal=causal, zigzag=zigzag, exchange=exchange,
                                 additive_mask=add if mask else None, route=False)
            for rank in range(4):
                r = rank if sp == 4 else rank % 2
                theirs = got[rank][(sp, i, r)]
                theirs = theirs.permute(0, 2, 1, 3) if layout == "bhsd" else theirs
                assert torch.equal(theirs, pc.shard(out, r, sp, zigzag)), (sp, GLOO_FORMS[i], rank)


# ---- the ring case table -------------------------------------------------------------------------------------------------------
def _null_step(q, k, v, **kw):
    return kw.get("out")


def test_ring_table_covers_what_the_issue_lists():
    cs = pc.RING_CASES
    assert len({c["name"] for c in cs}) == len(cs) and 20 < len(cs) < 60
    assert {c["sp"] for c in cs} == {2, 3, 4, 8} and {c["D"] for c in cs} == {64, 80, 128}
    assert {(c["H"], c["Hkv"]) for c in cs} == {(4, 4), (4, 2)} and {c["layout"] for c in cs} == {"bshd", "bhsd"}
    assert {c["route"] for c in cs} == {"fwd3", "fwd1", "fwd1_add", "fwd5_kpre_carry"}
    kinds = {"noncausal": lambda c: c["form"] == "noncausal" and c["Skl"] == c["Sl"],
             "cross": lambda c: c["form"] == "noncausal" and (c["Sl"], c["Skl"]) == (200, 136),
             "causal": lambda c: c["form"] == "causal", "zigzag": lambda c: c["form"] == "zigzag",
             "mask": lambda c: c["form"] == "mask"}
    for name, is_ in kinds.items():   # every placement and form at sp >= 3 and at both head-dim classes
        mine = [c for c in cs if is_(c)]
        assert any(c["sp"] >= 3 and c["D"] <= 64 for c in mine) and any(c["sp"] >= 3 and c["D"] == 128 for c in mine), name
    for form in ("kpre_noncausal", "kpre_causal", "kpre_zigzag"):
        assert any(c["form"] == form and c["sp"] >= 3 for c in cs), form
    for Sl, zz in ((200, False), (100, False), (272, True), (128, True)):
        assert any(c["Sl"] == Sl and c["zigzag"] == zz for c in cs)


@pytest.mark.parametrize("name", [c["name"] for c in pc.RING_CASES])
def test_ring_case_routes_and_live_rows(monkeypatch, name):
    """Every launch of every rank takes the route the table states (ops.fa3_route reads shapes and strides only), under both
    exchanges; and every row of the case has a finite reference lse, so the judgement exempts none."""
    from mio.parallelism import _local
    monkeypatch.setattr(_local, "attention_step", _null_step)
    c = pc.ring_case(name)
    for dtype in (BF, FP):
        q, k, v, add = pc.ring_inputs(c, dtype)
        per_exchange = []
        for exchange in ("mesh", "ring"):
            _, recs = pc.run_ring(q, k, v, c["sp"], exchange=exchange, additive_mask=add, **pc.ring_kwargs(c))
            for r, calls in enumerate(recs):
                assert calls and all(s["route"] == c["route"] for s in calls), (name, r, [s["route"] for s in calls])
                assert all(s["Sq"] == c["seg"] for s in calls)
            per_exchange.append(recs)
        assert per_exchange[0] == per_exchange[1], "mesh and ring exchanges issue different launches"
        if not c["causal"]:
            assert all(len(calls) == c["sp"] for calls in per_exchange[0])
        _, lse = pc.ring_reference(q, k, v, causal=c["causal"], additive_mask=add, k_prescaled=c["kpre"])
        assert torch.isfinite(lse).all(), name


def test_real_launches_see_what_the_cpu_schedules_saw(monkeypatch):
    """At sp >= 3 the table's launches include a third ring step, a query segment that finishes before the last step and two
    zig-zag segments that finish at different steps."""
    from mio.parallelism import _local
    monkeypatch.setattr(_local, "attention_step", _null_step)
    c = pc.ring_case("causal_sp4_h4kv2_d64_bshd_s200")
    q, k, v, _ = pc.ring_inputs(c, BF, B=1)
    _, recs = pc.run_ring(q, k, v, 4, exchange="mesh", **pc.ring_kwargs(c))
    assert [len(r) for r in recs] == [1, 2, 3, 4]
    assert all(r[-1]["write_out"] and not any(s["write_out"] for s in r[:-1]) for r in recs)
    c = pc.ring_case("zigzag_sp4_h4kv4_d128_bshd_s272")
    q, k, v, _ = pc.ring_inputs(c, BF, B=1)
    _, recs = pc.run_ring(q, k, v, 4, exchange="ring", **pc.ring_kwargs(c))
    for r, calls in enumerate(recs):
        fin = [i for i, s in enumerate(calls) if s["write_out"]]
        assert len(fin) == 2
        if r > 0:   # the first segment (block r) sees its last key r steps in; the second (block 7 - r) at the last step
            assert fin[0] < fin[1] == len(calls) - 1 and calls[fin[0]]["q_offset"] == r * 136


# ---- the module case table -----------------------------------------------------------------------------------------------------
def _gemm(M, N, K, dtype, residual=False, activation="none", col_scale=False):
    from mio import ops
    x, w = torch.empty(M, K, dtype=dtype), torch.empty(N, K, dtype=dtype)
    kw = {}
    if ops.blocked_weight_ok(M, N, K, activation):
        kw["w_blocked"] = torch.empty((N + 255) // 256 * 256 * K, dtype=dtype)
    if residual:
        kw["residual"] = torch.empty(M, N, dtype=dtype)
    if col_scale:
        assert ops.col_scale_ok(M, N, K, activation)
        kw["col_scale"] = (0, 128, 1.0)
    return "gemm:" + ops.gemm_route(x, w, None, activation, **kw) + ("+cs" if col_scale else "")


def _planned_routes(c, rank, dtype, monkeypatch, tiles_below=0):
    """The routes of a module case's launches on `rank`, from the shapes the modules hand to the kernels (mio/parallelism
    tensor_parallel.py and sequence_parallel.py), tiles_below row tiles of 256 below the case's rows."""
    from mio import ops
    from mio._nn import attention_plan
    from mio.parallelism import _local
    B, S = pc.module_shape(c)
    M = B * S - 256 * tiles_below
    d, H, D = pc.D_MODEL, pc.HEADS, pc.D_MODEL // pc.HEADS
    kind = c["module"]
    if kind in ("tp_mlp", "sp_mlp"):
        tp = pc.WORLD if kind == "tp_mlp" else 1
        out = [_gemm(M, pc.TP_I // tp, d, dtype, activation=c["spec"]["act"])]
        if kind == "sp_mlp":
            return out + [_gemm(M, d, pc.TP_I, dtype, residual=True)]
        K2 = pc.TP_I // tp
    elif kind == "tp_attn":
        assert tiles_below == 0 or B * S > 4096
        n = d // pc.WORLD
        Hl = H // pc.WORLD
        plan = attention_plan(B, S, S, Hl, Hl, D, (M, 3 * n, d), (n, 2 * n), 3 * n, mask=False)
        out = [_gemm(M, 3 * n, d, dtype, col_scale=plan.kpre)]
        qkv = torch.empty(B, S, 3 * n, dtype=dtype)
        q, k, v = (qkv[..., i * n:(i + 1) * n].view(B, S, Hl, D) for i in range(3))
        out.append("attn:" + ops.fa3_route(q, k, v, layout="bshd", causal=True, **({"k_prescaled": True} if plan.kpre else {})))
        K2 = n
    else:
        Sq = S // (2 if c["zigzag"] else 1)
        kpre = False
        if c["mode"] == "ring":
            kpre = attention_plan(B, Sq, Sq, H, H, D, (M, d, d), (0, d), d, mask=False, carry=True).kpre
        out = [_gemm(M, d, d, dtype), _gemm(M, d, d, dtype, col_scale=kpre), _gemm(M, d, d, dtype)]
        if tiles_below:
            return out
        q, k, v = (torch.empty(B, S * pc.WORLD, H, D, dtype=dtype) for _ in range(3))
        if c["mode"] == "ring":
            monkeypatch.setattr(_local, "attention_step", _null_step)
            _, recs = pc.run_ring(q, k, v, pc.WORLD, causal=c["spec"]["causal"], zigzag=c["zigzag"], exchange=c["exchange"],
                                  k_prescaled=kpre)
            out += ["attn:" + s["route"] for s in recs[rank]]
        elif c["mode"] == "full":
            out.append("attn:" + ops.fa3_route(q[:, :S], k, v, layout="bshd", causal=True, q_offset=rank * S, k_offset=0))
        else:
            out.append("attn:" + ops.fa3_route(q[:, :S], k[:, :S], v[:, :S], layout="bshd", causal=c["spec"]["causal"]))
        return out + [_gemm(M, d, d, dtype, residual=True)]
    nch = max(1, min(c["chunks"], M // 256 if M >= 512 else 1))   # RowParallelLinear.forward
    bounds = [(i * M) // nch for i in range(nch + 1)]
    return out + [_gemm(bounds[i + 1] - bounds[i], d, K2, dtype, residual=c["residual"] and rank == 0) for i in range(nch)]


@pytest.mark.parametrize("name", [c["name"] for c in pc.MODULE_CASES])
def test_module_case_routes_stand_and_fall_a_tile_below(monkeypatch, name):
    c = pc.module_case(name)
    B, S = pc.module_shape(c)
    big = c["shape"] != "small"
    assert (B * S) % 256 != 0
    for dtype in (BF, FP):
        for rank in range(pc.WORLD):
            got = tuple(_planned_routes(c, rank, dtype, monkeypatch))
            assert got == c["routes"][rank], f"{name} rank {rank}: planned {got}, the table says {c['routes'][rank]}"
    if "n_chunks" in c:
        assert len([r for r in c["routes"][0] if r.startswith("gemm:")]) == 1 + c["n_chunks"]
        assert c["chunks"] == 1 or (B * S // c["n_chunks"]) % 256 != 0, "the chunk bounds must be no multiples of 256"
    if big:   # one row tile below, the narrowest GEMM of the shape (the whole out-projection / fc2) has left the 256-tile kernels
        from mio import ops
        K2 = pc.D_MODEL // pc.WORLD if c["module"] == "tp_attn" else pc.TP_I // pc.WORLD if c["module"] == "tp_mlp" else pc.D_MODEL
        assert ops.blocked_weight_ok(B * S, pc.D_MODEL, K2) and not ops.blocked_weight_ok(B * S - 256, pc.D_MODEL, K2)
        assert _gemm(B * S, pc.D_MODEL, K2, BF).startswith("gemm:p8w") and _gemm(B * S - 256, pc.D_MODEL, K2, BF) == "gemm:t128"
    else:
        assert all(r in ("gemm:t128", "attn:fwd5") for r in c["routes"][0])


def test_module_table_covers_what_the_issue_lists():
    cs = pc.MODULE_CASES
    assert len({c["name"] for c in cs}) == len(cs)
    tpa = [c for c in cs if c["module"] == "tp_attn"]
    assert {c["shape"] for c in tpa} == {"small", "hd64"} and {c["chunks"] for c in tpa} == {1, 3}
    assert {c["residual"] for c in tpa} == {True, False} and all(c["spec"]["causal"] for c in tpa)
    tpm = [c for c in cs if c["module"] == "tp_mlp"]
    assert {c["spec"]["act"] for c in tpm} == {"gelu", "silu"} and {c["shape"] for c in tpm} == {"small", "hd64"}
    assert all(c["spec"]["I"] == 2048 and c["residual"] and c["norm"] for c in tpm)
    spa = [c for c in cs if c["module"] == "sp_attn"]
    rings = {(c["exchange"], c["zigzag"]) for c in spa if c["mode"] == "ring"}
    assert rings == {("mesh", False), ("ring", True)}
    assert {c["mode"] for c in spa} == {"ring", "full", "local"} and sum(c["module"] == "sp_mlp" for c in cs) == 1
    assert next(c for c in spa if c["zigzag"])["spec"]["kpre"]
    assert {c["spawn"] for c in cs} == set(pc.SPAWNS) and 2 * len(pc.SPAWNS) <= 8


# ---- the tensor-parallel form of the model -------------------------------------------------------------------------------------
_TRUTH: dict = {}
HOST_B = {"small": 2, "hd64": 3, "sp": 2}


def _truth(name, dtype):
    """Inputs, fp64 reference and clean model of a module case at HOST_B batches: computed once, left unchanged."""
    key = (name, dtype)
    if key not in _TRUTH:
        c = pc.module_case(name)
        P, n, x = pc.module_inputs(c, dtype, B=HOST_B[c["shape"]])
        ref, model = pc.module_truth(c, P, n, x, dtype)
        _TRUTH[key] = dict(c=c, P=P, n=n, x=x, ref=ref, model=model)
    return _TRUTH[key]


@pytest.mark.parametrize("name", ["tp_attn_small_chunks3_full", "tp_mlp_small_gelu_chunks3"])
def test_tp_default_is_todays_model_and_tp2_is_the_same_function(name):
    """tp = 1 takes the statements the model had before it knew of tp (one product, one store): the same bits with and without
    the argument.  Without rounding the tp = 2 form is the tp = 1 function; with it, it differs (two more stores per row)."""
    t = _truth(name, BF)
    c, kw = t["c"], dict(norm=t["n"], residual=True)
    one = mc.model(c["spec"], t["P"], t["x"], dtype=BF, **kw)
    assert torch.equal(one, mc.model(c["spec"], t["P"], t["x"], dtype=BF, tp=1, **kw))
    A = mc._Arith(BF, None)
    h = torch.randn(40, 64, dtype=torch.float64)
    w, b, res = (torch.randn(*shape, dtype=torch.float64) for shape in ((32, 64), (32,), (40, 32)))
    assert torch.equal(mc._row_parallel(A, h, w, b, res, 1)[0], mc.rn16(h @ w.t() + b + res, BF))
    assert torch.equal(mc._row_parallel(A, h, w, b, res, 2)[0],
                       mc.rn16(mc.rn16(h[:, :32] @ w[:, :32].t() + b + res, BF) + mc.rn16(h[:, 32:] @ w[:, 32:].t(), BF), BF))
    ref2 = mc.reference(c["spec"], t["P"], t["x"], tp=2, **kw)
    assert mc.row_errors(ref2, t["ref"]).max().item() < 1e-12
    assert not torch.equal(one, t["model"])
    with pytest.raises(ValueError):
        mc.model(c["spec"], t["P"], t["x"], dtype=BF, defect="tp_bias_every_rank", **kw)


@DTYPES
@pytest.mark.parametrize("name", [c["name"] for c in pc.MODULE_CASES if c["shape"] != "hd64" or c["chunks"] == 3])
def test_module_model_passes_its_bars(name, dtype):
    t = _truth(name, dtype)
    S = t["x"].shape[1]
    mc.judge(t["model"], t["ref"], t["model"], dtype, S, "host", what=name, record=False)
    st = mc.measure(t["model"], t["ref"], dtype, S)
    assert 0.2 < st["mean"] < 3.0 and st["worst"] < 6.0, st


# ---- planted faults ------------------------------------------------------------------------------------------------------------
TP_PLANTED = [("tp_bias_every_rank", "tp_attn_small_chunks3_full"), ("tp_bias_every_rank", "tp_attn_hd64_chunks3_full"),
              ("tp_bias_every_rank", "tp_mlp_small_gelu_chunks3"), ("tp_residual_every_rank", "tp_attn_small_chunks3_full"),
              ("tp_residual_every_rank", "tp_attn_hd64_chunks3_full"), ("tp_residual_every_rank", "tp_mlp_hd64_gelu_chunks3"),
              ("tp_chunk_unreduced", "tp_attn_small_chunks3_full"), ("tp_chunk_unreduced", "tp_attn_hd64_chunks3_full"),
              ("tp_chunk_unreduced", "tp_mlp_hd64_gelu_chunks3"), ("tp_k_from_rank0", "tp_attn_small_chunks3_full"),
              ("tp_k_from_rank0", "tp_attn_hd64_chunks3_full")]


@DTYPES
@pytest.mark.parametrize("defect,name", TP_PLANTED)
def test_planted_tp_fault_fails_judge(defect, name, dtype):
    t = _truth(name, dtype)
    c = t["c"]
    bad = pc.module_truth(c, t["P"], t["n"], t["x"], dtype, defect=defect)[1]
    assert not torch.equal(bad, t["model"])
    rel, accepted = mc.old_aggregate(bad, t["model"])
    print(f"\n{defect} in {name} {dtype}: old whole-tensor statistic {rel:.2e} ({'ACCEPTED' if accepted else 'refused'} at 3e-3)")
    with pytest.raises(AssertionError):
        mc.judge(bad, t["ref"], t["model"], dtype, t["x"].shape[1], "host", what=defect, record=False)


def test_every_tp_fault_is_planted():
    assert {d for d, _ in TP_PLANTED} == set(mc.TP_DEFECTS)


@DTYPES
def test_zigzag_rows_judged_at_contiguous_positions_fail(dtype):
    """The position map matters: a zig-zag rank's rows pass against the reference rows at positions() and fail against the rows
    a contiguous placement would give it."""
    t = _truth("sp_attn_ring_ring_zigzag", dtype)
    Sl = pc.SP_LOCAL
    for r in range(pc.WORLD):
        y = pc.shard(t["model"], r, pc.WORLD, True)
        good = [pc.shard(t[k_], r, pc.WORLD, True) for k_ in ("ref", "model")]
        mc.judge(y, good[0], good[1], dtype, Sl, "host", record=False)
        wrong = [pc.shard(t[k_], r, pc.WORLD, False) for k_ in ("ref", "model")]
        with pytest.raises(AssertionError):
            mc.judge(y, wrong[0], wrong[1], dtype, Sl, "host", record=False)


def _ring_truth(name, dtype):
    key = ("ring", name, dtype)
    if key not in _TRUTH:
        c = pc.ring_case(name)
        q, k, v, add = pc.ring_inputs(c, dtype, B=1)
        kw = dict(causal=c["causal"], additive_mask=add, k_prescaled=c["kpre"])
        _TRUTH[key] = dict(c=c, q=q, k=k, v=v, add=add, ref=pc.ring_reference(q, k, v, **kw)[0],
                           model=pc.ring_model(q, k, v, dtype=dtype, **kw))
    return _TRUTH[key]


def _f_next_offset(t, r):
    def hook(i, q, k, v, kw, launch):
        if i >= 1:
            kw["k_offset"] += t["c"]["Skl"]
    return hook


def _f_q_offset(t, r):
    def hook(i, q, k, v, kw, launch):
        if q.storage_offset() != 0:   # the second zig-zag segment
            kw["q_offset"] += 1
    return hook


def _f_no_carry(t, r):
    def hook(i, q, k, v, kw, launch):
        if i == 1:
            kw["carry_in"] = False
    return hook


def _f_local_mask(t, r):
    c = t["c"]
    mine = pc.shard(t["add"], r, c["sp"], False, dim=2)

    def hook(i, q, k, v, kw, launch):
        kw["additive_mask"] = mine[..., :kw["additive_mask"].shape[-1]]
    return hook


def _f_twice(t, r):
    def hook(i, q, k, v, kw, launch):
        if i == 0:
            launch(q, k, v, **kw)
            kw["carry_in"] = True
    return hook


RING_PLANTED = {
    "a shard attended at the next origin's k_offset": ("causal_sp3_h4kv4_d64_bhsd_s200", _f_next_offset),
    "the second zig-zag segment's q_offset one too large": ("zigzag_sp3_h4kv2_d128_bhsd_s272", _f_q_offset),
    "carry_in false at step 1": ("noncausal_sp3_h4kv2_d128_bhsd_s200", _f_no_carry),
    "the additive-mask slice taken at local columns": ("mask_sp3_h4kv2_d128_bhsd_s100", _f_local_mask),
    "the local shard counted twice": ("noncausal_sp4_h4kv4_d80_bshd_s200", _f_twice),
}


@DTYPES
@pytest.mark.parametrize("fault", sorted(RING_PLANTED))
def test_planted_ring_fault_fails_judge(monkeypatch, fault, dtype):
    """The product's ring_attention on the loopback with the stand-in kernels (an fp64 attention rounded once to the dtype): the
    clean run passes the judgement, the run with one launch altered does not."""
    _cpu_local.install(monkeypatch)
    name, make = RING_PLANTED[fault]
    t = _ring_truth(name, dtype)
    c = t["c"]
    def run(hook):
        return pc.run_ring(t["q"], t["k"], t["v"], c["sp"], additive_mask=t["add"], exchange="mesh", hook=hook, **pc.ring_kwargs(c))[0]

    clean = run(None)
    pc.judge_ring(clean, t["ref"], t["model"], dtype, c["seg"], "host", what=name, record=False)
    bad = run(lambda r: make(t, r))
    assert not torch.equal(bad, clean), f"{fault}: the planted fault changed nothing"
    with pytest.raises(AssertionError):
        pc.judge_ring(bad, t["ref"], t["model"], dtype, c["seg"], "host", what=fault, record=False)


@DTYPES
@pytest.mark.parametrize("name", ["kpre_zigzag_sp4_h4kv2_d64_bhsd_s272", "zigzag_sp4_h4kv4_d64_bshd_s128",
                                  "mask_sp4_h4kv4_d64_bshd_s200k136"])
def test_ring_model_passes_its_bars(name, dtype):
    """The ring's model against the reference: P and the context are its two roundings, so a row is off by less than 2 u."""
    t = _ring_truth(name, dtype)
    pc.judge_ring(t["model"], t["ref"], t["model"], dtype, t["c"]["seg"], "host", what=name, record=False)
    st = pc.ring_measure(t["model"], t["ref"], dtype, t["c"]["seg"])
    assert 0.2 < st["mean"] < 1.0 and st["worst"] < 2.0 and st["seq"] < 1.5 * st["mean"], st

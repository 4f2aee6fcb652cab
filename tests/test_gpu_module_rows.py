"""Every planned route of the module layer, judged row by row against fp64 (tests/_module_check.py: the reference, the rounding
model the bars come from, judge(), the case table).  Each case asserts the route of its GEMM and attention launches with the
recorder of tests/_module_trace.py -- a case that silently falls back fails -- then judges every sub-layer on its actual input:
worst row, mean, worst 256-row tile and worst sequence, and a ResidualStream's row statistics against its own rows.
test_prepared_copies_follow_parameter_updates changes parameters in place after a first forward (copy_, load_state_dict) and
judges the second forward against the reference of the new parameters: the CastCache keys must reach every prepared copy
(blocked, concatenated, folded, interleaved)."""
import pytest
import torch
import torch.nn as nn

import _module_check as mc
from _module_trace import PREP, record

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, FP = mc.BF, mc.FP
PREC = {BF: "bf16", FP: "fp16"}
IDS = [f"{n}-{PREC[dt]}" for n, dt in mc.case_ids()]


# ---- building the modules from the table's parameters --------------------------------------------------------------------------
def _put(module: nn.Module, P: dict, prefix: str = "") -> None:
    with torch.no_grad():
        for name, t in P.items():
            module.get_parameter(prefix + name).copy_(t)


def _norm_module(n: dict, d: int, dtype, cls=None) -> nn.Module:
    cls = cls or (nn.LayerNorm if n["kind"] == "layernorm" else nn.RMSNorm)
    m = cls(d).to(DEV, dtype)
    _put(m, {k: n[k] for k in ("weight", "bias") if k in n})
    assert mc.norm_eps(n["kind"], m.eps, dtype) == n["eps"]
    return m


def _attn_module(spec, d, dtype, storage):
    from mio.kernels.attention.flash_attention import FlashAttentionConfig, FlashAttentionLayer, FlashSelfAttention
    cfg = FlashAttentionConfig(precision=PREC[dtype], causal=spec["causal"], normalize_query=bool(spec.get("normq")),
                               rotary_dim=spec.get("rotary", 0), window_size=spec.get("window") or (-1, -1))
    cls = FlashSelfAttention if spec["kind"] == "self" else FlashAttentionLayer
    return cls(d, spec["H"], cfg, num_kv_heads=spec["Hkv"]).to(DEV, storage).eval()


def _mlp_module(spec, d, dtype, storage):
    from mio.kernels.mlp.fused_mlp import FusedMLP, FusedMLPConfig, FusedTransformerMLP
    if spec["act"] == "gelu_erf":   # the plain FusedMLP's "gelu" is the erf form
        return FusedMLP(d, spec["I"], FusedMLPConfig(precision=PREC[dtype], activation_fn="gelu")).to(DEV, storage).eval(), ""
    m = FusedTransformerMLP(d, spec["I"], spec["act"], FusedMLPConfig(precision=PREC[dtype]))
    return m.to(DEV, storage).eval(), "mlp."


def _routes(calls):
    """(the case table's route words of the launches that have a route, norm kernel launches) of a record."""
    out, norms = [], 0
    for r in calls:
        fn, a = r["fn"], r["args"]
        if fn in ("layernorm", "rmsnorm"):
            norms += 1
        elif fn in ("gemm_bias_act", "gemm_ln"):
            out.append(f"gemm:{r['route']}" + ("+cs" if a["col_scale"] is not None else ""))
        elif fn == "fused_mlp":
            rt = r["route"]
            out.append(f"mlp:{rt['path']}/{rt['stage1']}/{rt['stage2']}")
        elif fn == "fa3_fwd":
            name = str(r["route"])
            assert not name.startswith("refused"), name
            assert ("kpre" in name) == bool(a["k_prescaled"]) and name.endswith("oblk") == bool(a["out_blocked"]), (name, a)
            out.append("attn:" + ("kpre" if a["k_prescaled"] else "plain") + ("+oblk" if a["out_blocked"] else ""))
    return tuple(out), norms


def _assert_routes(c, calls):
    got, norms = _routes([r for r in calls if r["fn"] not in PREP])
    assert got == c["routes"], f"{c['name']}: launches took {got}, the table says {c['routes']}"
    assert norms == c["norms"], f"{c['name']}: {norms} norm launches, the table says {c['norms']}"


def _rows(t):
    """A module output as [B, S, d] rows: a ResidualStream by its dense() copy."""
    return t.dense() if hasattr(t, "dense") else t


def _judge_stream(s, what):
    Bc, Sc, _ = s.shape
    mc.judge_stats(s.stats[:, :Bc * Sc], s.dense(), what)


# ---- one case: build, run, judge -----------------------------------------------------------------------------------------------
def _build(c, dtype, seed_shift=0):
    """The case's parameters (CPU, storage dtype), inputs and modules (on the device)."""
    d, H, Bc, Sc = mc.SHAPES[c["shape"]]
    storage = c.get("storage", dtype)
    g = torch.Generator().manual_seed(mc.seed_of(c["name"], dtype) + seed_shift)
    st = dict(c=c, dtype=dtype, storage=storage, d=d, B=Bc, S=Sc, x=mc.draw_rows(Bc, Sc, d, g, storage))
    kind = c["module"]
    if kind in ("self", "layer"):
        st["P"] = mc.draw_params(c["spec"], d, g, storage)
        st["n"] = mc.draw_norm(c["norm"], d, g, storage) if c["norm"] else None
        st["m"] = _attn_module(c["spec"], d, dtype, storage)
        _put(st["m"], st["P"])
        st["nm"] = _norm_module(st["n"], d, storage) if st["n"] else None
        st["keep"] = mc.keep_mask(Bc, Sc) if c.get("mask") else None
    elif kind == "mlp":
        st["P"] = mc.draw_params(c["spec"], d, g, storage)
        st["n"] = mc.draw_norm(c["norm"], d, g, storage) if c["norm"] else None
        st["m"], st["prefix"] = _mlp_module(c["spec"], d, dtype, storage)
        _put(st["m"], st["P"], st["prefix"])
        st["nm"] = _norm_module(st["n"], d, storage) if st["n"] else None
        if c["stream"]:   # the attention sub-layer that produces the first stream (outside the record, not judged here)
            asp = mc.attn_spec(kpre=True)
            st["a"] = _attn_module(asp, d, dtype, storage)
            _put(st["a"], mc.draw_params(asp, d, g, storage))
            st["an"] = _norm_module(mc.draw_norm(c["norm"], d, g, storage), d, storage)
    else:
        from mio.synthetic import Block, CrossBlock, FusedLayerNorm, FusedRMSNorm
        ncls = FusedLayerNorm if c["norm"] == "layernorm" else FusedRMSNorm
        st["blocks"] = []
        for _ in range(2 if kind == "chain" else 1):
            b = dict(Pa=mc.draw_params(c["spec"], d, g, storage), Pm=mc.draw_params(c["mlp"], d, g, storage),
                     n1=mc.draw_norm(c["norm"], d, g, storage), n2=mc.draw_norm(c["norm"], d, g, storage))
            if kind == "cross_block":
                m = CrossBlock(d, H, c["mlp"]["I"], PREC[dtype], c["mlp"]["act"])
            else:
                m = Block(d, H, c["mlp"]["I"], c["spec"]["causal"], PREC[dtype], c["mlp"]["act"], c["norm"])
            m = m.to(DEV, storage).eval()
            assert isinstance(m.ln_1, ncls) and isinstance(m.ln_2, ncls)
            _put(m.attn, b["Pa"])
            _put(m.mlp, b["Pm"], "mlp.")
            for ln, n in ((m.ln_1, b["n1"]), (m.ln_2, b["n2"])):
                _put(ln, {k: n[k] for k in ("weight", "bias") if k in n})
                assert mc.norm_eps(n["kind"], ln.eps, storage) == n["eps"]
            b["m"] = m
            st["blocks"].append(b)
        if kind == "cross_block":
            st["ctx"] = mc.draw_rows(Bc, Sc, d, g, storage)
    return st


def _check(y, x, spec, P, st, family, what, **kw):
    """Judge the rows y of one sub-layer call on its actual input rows x."""
    ref = mc.reference(spec, P, x, device=DEV, **{k: v for k, v in kw.items() if k != "fold"})
    mod = mc.model(spec, P, x, dtype=st["dtype"], device=DEV, **kw)
    return mc.judge(_rows(y), ref, mod, st["dtype"], st["S"], family, what=what)


@torch.no_grad()
def _run(st):
    c, kind, fam = st["c"], st["c"]["module"], st["c"]["family"]
    x = st["x"].to(DEV)
    name = c["name"]
    if kind in ("self", "layer"):
        m, nm, n, keep = st["m"], st["nm"], st["n"], st["keep"]
        kw = dict(norm=n, keep=keep)
        mask = None if keep is None else keep.to(DEV)
        if c["stream"] is None:
            with record() as calls:
                y = m(x, mask, residual=x, pre_norm=nm) if kind == "self" else m(x, mask, residual=x)
            _assert_routes(c, calls)
            _check(y, x, c["spec"], st["P"], st, fam, name, **kw)
            return
        with record() as calls:
            s = m(x, residual=x, pre_norm=nm, stream_out=True)
            y = m(s, residual=s, pre_norm=nm)
        _assert_routes(c, calls)
        _check(s, x, c["spec"], st["P"], st, fam + "_out", name + " (stream out)", **kw)
        _judge_stream(s, name)
        _check(y, s.dense(), c["spec"], st["P"], st, fam + "_in", name + " (stream in)", fold=True, **kw)
    elif kind == "mlp":
        m, nm, n = st["m"], st["nm"], st["n"]
        if not c["stream"]:
            with record() as calls:
                y = m(x, residual=x, pre_norm=nm)
            _assert_routes(c, calls)
            _check(y, x, c["spec"], st["P"], st, fam, name, norm=n)
            return
        s0 = st["a"](x, residual=x, pre_norm=st["an"], stream_out=True)
        with record() as calls:
            s1 = m(s0, residual=s0, pre_norm=nm, stream_out=True)
            y = m(s1, residual=s1, pre_norm=nm)
        _assert_routes(c, calls)
        _check(s1, s0.dense(), c["spec"], st["P"], st, fam + "_out", name + " (stream out)", norm=n, fold=True)
        _judge_stream(s1, name)
        _check(y, s1.dense(), c["spec"], st["P"], st, fam + "_in", name + " (stream in)", norm=n, fold=True)
    else:
        seen, hooks = [], []
        for b in st["blocks"]:   # the attention sub-layer's output of each block, as the block hands it to its MLP
            hooks.append(b["m"].attn.register_forward_hook(lambda _m, _i, o: seen.append(o)))
        extra = (st["ctx"].to(DEV),) if kind == "cross_block" else ()
        akw = dict(context=st.get("ctx"))
        try:
            with record() as calls:
                h, outs = x, []
                for i, b in enumerate(st["blocks"]):
                    h = b["m"](h, *extra, stream_out=i + 1 < len(st["blocks"]), fold=c["fold"])
                    outs.append(h)
        finally:
            for hk in hooks:
                hk.remove()
        _assert_routes(c, calls)
        fold, spec, mlp = c["fold"], c["spec"], c["mlp"]
        # every sub-layer on its actual input; a block's first sub-layer folds its norm only behind a stream
        for i, (b, a) in enumerate(zip(st["blocks"], seen)):
            inp = x if i == 0 else outs[i - 1]
            tag = f"{name} block {i}"
            assert hasattr(a, "dense") == fold, f"{tag}: the attention sub-layer's output is {'not ' if fold else ''}a stream"
            _check(a, _rows(inp), spec, b["Pa"], st, fam + "_attn", tag + " attention", norm=b["n1"], fold=hasattr(inp, "dense"),
                   **akw)
            if fold:
                _judge_stream(a, tag + " attention")
            _check(outs[i], _rows(a), mlp, b["Pm"], st, fam + "_mlp", tag + " mlp", norm=b["n2"], fold=fold)
            if hasattr(outs[i], "dense"):   # the stream between two blocks
                _judge_stream(outs[i], tag + " mlp")
        if kind == "chain":
            # two blocks end to end: the reference chain in fp64 (nothing rounded), the model chain as the yardstick
            r = mo = x
            for i, b in enumerate(st["blocks"]):
                r = mc.reference(spec, b["Pa"], r, norm=b["n1"], device=DEV)
                r = mc.reference(mlp, b["Pm"], r, norm=b["n2"], device=DEV)
                mo = mc.model(spec, b["Pa"], mo, dtype=st["dtype"], norm=b["n1"], fold=i > 0, device=DEV)
                mo = mc.model(mlp, b["Pm"], mo, dtype=st["dtype"], norm=b["n2"], fold=True, device=DEV)
            mc.judge(h, r, mo, st["dtype"], st["S"], fam, what=name + " (chain against chain)")


@pytest.mark.parametrize("name,dtype", mc.case_ids(), ids=IDS)
def test_route_rows(name, dtype):
    _run(_build(mc.case(name), dtype))


# ---- freshness of the prepared weight copies ---------------------------------------------------------------------------------
def _update(dst: dict, module: nn.Module, new: dict, names, prefix="", how="copy_"):
    """Parameters `names` of module take new's values in place (copy_ or load_state_dict); dst, the table of what the module
    now holds, follows."""
    with torch.no_grad():
        if how == "copy_":
            for k in names:
                module.get_parameter(prefix + k).copy_(new[k])
        else:
            module.load_state_dict({k: new[k].to(DEV) for k in names})
    for k in names:
        dst[k] = new[k]


@pytest.mark.parametrize("dtype", [BF, FP], ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", ["block_fold", "mlp_swiglu_large", "mlp_swiglu_stream_rms"])
def test_prepared_copies_follow_parameter_updates(name, dtype):
    """A first forward prepares every copy; then parameters change in place and the second forward is judged against the
    reference of the NEW parameters.  The head-dim-64 Block (blocked fused projection, folded fc1 behind ln_2, blocked
    out-projection) and the SwiGLU MLP in its blocked form (interleaved gate / up) and its stream form (folded + interleaved)."""
    st = _build(mc.case(name), dtype)
    new = _build(mc.case(name), dtype, seed_shift=1)
    _run(st)
    if name == "block_fold":
        b, nb = st["blocks"][0], new["blocks"][0]
        m = b["m"]
        _update(b["Pa"], m.attn, nb["Pa"], ["qkv_proj.weight"])                                    # copy_ on a projection weight
        _update(b["n2"], m.ln_2, nb["n2"], ["weight", "bias"])                                     # on a norm's gamma and beta
        o = {"weight": nb["Pa"]["o_proj.weight"], "bias": nb["Pa"]["o_proj.bias"]}
        _update({}, m.attn.o_proj, o, ["weight", "bias"], how="load_state_dict")                   # load_state_dict on the out-projection
        b["Pa"]["o_proj.weight"], b["Pa"]["o_proj.bias"] = o["weight"], o["bias"]
    else:
        _update(st["P"], st["m"], new["P"], ["fc1_gate.weight"], prefix=st["prefix"])              # copy_ on the gate weight
        if st["n"] is not None:
            _update(st["n"], st["nm"], new["n"], ["weight"])                                       # and on the folded norm's gamma
    _run(st)

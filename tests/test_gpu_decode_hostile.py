"""Paged decode in hostile memory (tests/_hostile_decode.py): mio_fa3_decode_paged, mio_fa3_decode_paged_window and
mio_fa3_decode_paged_kv8, the three routes, both cache kinds, windowed and not.

test_decode_hostile launches each case of the table through the C ABI on operands embedded in guarded buffers, asserts the
route first, and is judged by _hostile_decode.judge: the launches with every not-owned byte NaN, then huge -- the
workspace included -- equal to the benign launch bit for bit in every owned byte of o; the same after a launch with longer
contexts left its partial states in the workspace; the same for three sequences and one kv head with their neighbours
poisoned; guards and inputs untouched after each launch; the benign launch within the unchanged _decode_check bars.  All
launches of a case run in the same device buffers at the same addresses.

test_decode_graph_replay captures one cache write followed by one decode and replays it over six states changed in place:
q, the new k / v, context_lengths, block_tables, the caches and (fp8) the scales.  Each replay is judged against fp64 of its
state and must equal, bit for bit, an eager C-ABI launch on the same state with a fresh all-NaN workspace.

One run on the MI355X: 52 tests (46 judgements, 6 graph tests) in 18.8 s of wall time, the slowest
(rows-kv16-wide, block size 256) 2.0 s, most of it the CPU drawing buffers and computing the fp64 reference.  Found: nothing -- every
route gave the benign launch's bits under both fills, after a stale workspace and with poisoned neighbours, and wrote no byte it
does not own; no kernel was changed.
"""
import pytest
import torch

import _decode_check as dc
import _hostile_decode as hd

pytestmark = pytest.mark.gpu

DEV = "cuda"


class GpuRun:
    """run(built, bufs) of _hostile_decode.judge on the GPU: the buffers of a case live at fixed device addresses; every
    launch copies the given bytes in (the workspace as well: it is the launch's to find), launches once and copies every
    buffer back."""

    def __init__(self):
        self.dev = {}

    def __call__(self, built, bufs):
        from mio import _lib
        for name, t in bufs.items():
            if name not in self.dev:
                self.dev[name] = t.to(DEV)
            else:
                self.dev[name].copy_(t)
        query, qargs, fn, args = hd.launch_args(built, self.dev)
        r = query(*qargs)
        assert r >= 0 and _lib.DECODE_ROUTES[r] == built.case.route, (built.case.name, r)
        _lib.check(fn(*args, torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return {name: t.cpu() for name, t in self.dev.items()}


@pytest.mark.parametrize("case", hd.CASES, ids=lambda c: f"{c.name}-{str(c.dtype).split('.')[-1]}")
def test_decode_hostile(case):
    hd.judge(GpuRun(), hd.build(case))


# ---- one captured graph over changing states ---------------------------------------------------------------------------
_GRAPH = {  # route -> (kv16 geometry, fp8 geometry): B, H, Hkv, D; one query row (the cache write takes one token)
    "head": ((12, 4, 2, 80), (12, 4, 2, 80)), "rows": ((16, 2, 2, 64), (16, 4, 4, 64)), "gqa": ((12, 4, 2, 64), (12, 4, 2, 64)),
}
_BS, _MSL, _LEFT = 16, 1100, 301
_CTX0 = [1099, 0, 16, 127, 300, 513, 77, 640, 33, 950, 45, 255, 200, 700, 64, 150]   # lengths after the first write


def _states(B, kv8):
    """(contexts after the write, (k_scale, v_scale) lists) of the six states."""
    s0 = _CTX0[:B]
    up = lambda cs: [c + 1 if c < _MSL else c for c in cs]
    s1 = up(s0)                       # 0 -> 1; 16 -> 17 starts a new page; 127 -> 128
    s2 = up(s1)                       # 128 -> 129 crosses a multiple of 128 keys; 1100 is the longest the plan allows
    s3 = [1] + s2[1:]                 # the longest context's slot goes to a 1-key sequence
    s4 = s3[5:] + s3[:5]              # the table rows permuted (every state draws new physical blocks as well)
    s5 = up(s4)
    assert s0[1] == 0 and s1[1] == 1 and s0[2] % _BS == 0 and s1[3] == 128 and s2[3] == 129 and s2[0] == _MSL
    assert s3[0] == 1 and sorted(s4) == sorted(s3) and s4 != s3
    a = ([0.9, 5.0 / 416.0, 1.7], [1.3, 16.0 / 416.0, 0.47])
    b = ([0.9, 6.5 / 416.0, 1.7], [1.3, 11.0 / 416.0, 0.47])   # the tested layer's scales changed
    unit = ([1.0, 1.0], [1.0, 1.0])
    return [(s, (b if i >= 4 else a) if kv8 else unit) for i, s in enumerate((s0, s1, s2, s3, s4, s5))]


@pytest.mark.parametrize("kv8", [False, True], ids=["kv16", "fp8"])
@pytest.mark.parametrize("route", ["head", "rows", "gqa"])
def test_decode_graph_replay(route, kv8):
    from mio import _lib, ops
    lib = _lib.lib
    B, H, Hkv, D = _GRAPH[route][kv8]
    left = _LEFT if (("head", "rows", "gqa").index(route) + kv8) % 2 == 0 else -1
    dtype = dc.FP if kv8 else dc.BF
    cache_dtype = dc.F8 if kv8 else dtype
    L, bs, msl = (3 if kv8 else 2), _BS, _MSL
    max_blocks = (msl + bs - 1) // bs + 1
    gen = torch.Generator().manual_seed(1000 + 10 * ("head", "rows", "gqa").index(route) + kv8)

    # the states, on the CPU: the cache image with the slot the write will fill still NaN, and the fp64 reference of the
    # cache after the write
    states = []
    for ctxs, (ks, vs) in _states(B, kv8):
        def fill(b, n):   # 16-bit values, so that the last key is what the write is handed
            return tuple(torch.randn(n, Hkv, D, generator=gen).to(dtype).float() for _ in range(2))
        q = (torch.randn(B, H, 1, D, generator=gen) * 1.5).to(dtype)
        kc, vc, bt, _ = dc.hostile_cache(ctxs, block_size=bs, Hkv=Hkv, D=D, L=L, layer=dc.LAYER, cache_dtype=cache_dtype,
                                         gen=gen, max_blocks=max_blocks, fill=fill, k_scale=ks[dc.LAYER],
                                         v_scale=vs[dc.LAYER])
        ctx = torch.tensor(ctxs, dtype=torch.int32)
        kw = dict(left=left, k_scale=ks[dc.LAYER], v_scale=vs[dc.LAYER])
        ref, lse = dc.reference(q, kc, vc, bt, ctx, bs, dc.LAYER, **kw)
        model_o = dc.model(q, kc, vc, bt, ctx, bs, dc.LAYER, dtype=dtype, p16=route == "gqa", **kw)
        k_new = torch.full((B, 1, Hkv, D), float("nan"), dtype=dtype)
        v_new = torch.full((B, 1, Hkv, D), float("nan"), dtype=dtype)
        nan_slot = dc.nan_cache((Hkv, D), cache_dtype)
        for b, n in enumerate(ctxs):
            if n == 0:
                continue
            blk, slot = int(bt[b, (n - 1) // bs]), (n - 1) % bs
            if kv8:   # what the cache holds there, widened exactly: the write quantises it back to the same byte
                k_new[b, 0], v_new[b, 0] = ((c[blk, dc.LAYER, slot].float() * s[dc.LAYER]).to(dtype) for c, s in ((kc, ks), (vc, vs)))
                assert torch.equal(dc.quantise(k_new[b, 0].float(), ks[dc.LAYER]).view(torch.uint8),
                                   kc[blk, dc.LAYER, slot].view(torch.uint8)), "the new key does not round back to its byte"
            else:
                k_new[b, 0], v_new[b, 0] = kc[blk, dc.LAYER, slot], vc[blk, dc.LAYER, slot]
            kc[blk, dc.LAYER, slot] = nan_slot
            vc[blk, dc.LAYER, slot] = nan_slot
        states.append(dict(q=q, kc=kc, vc=vc, bt=bt, ctx=ctx, ks=ks, vs=vs, k_new=k_new, v_new=v_new, ref=ref, lse=lse,
                           model_o=model_o, ctxs=ctxs))
    nb = max(s["kc"].shape[0] for s in states)

    def pad(t):
        return torch.cat([hd.bits(t), hd.bits(dc.nan_cache((nb - t.shape[0],) + tuple(t.shape[1:]), cache_dtype))]).view(t.dtype)

    # the device tensors of the capture: every replay finds them at these addresses
    s0 = states[0]
    d = {k: s0[k].to(DEV) for k in ("q", "bt", "ctx", "k_new", "v_new")}
    d["kc"], d["vc"] = pad(s0["kc"]).to(DEV), pad(s0["vc"]).to(DEV)
    out = torch.full((B, H, 1, D), float("nan"), dtype=dtype, device=DEV)
    sc = {}
    if kv8:
        sc = dict(k_scale=torch.tensor(s0["ks"], dtype=torch.float32, device=DEV),
                  v_scale=torch.tensor(s0["vs"], dtype=torch.float32, device=DEV))

    def load(s):
        for k in ("q", "bt", "ctx", "k_new", "v_new"):
            d[k].copy_(s[k])
        d["kc"].copy_(pad(s["kc"]))
        d["vc"].copy_(pad(s["vc"]))
        if kv8:
            sc["k_scale"].copy_(torch.tensor(s["ks"], dtype=torch.float32))
            sc["v_scale"].copy_(torch.tensor(s["vs"], dtype=torch.float32))
        out.fill_(float("nan"))

    def step():
        ops.reshape_and_cache(d["k_new"], d["v_new"], d["kc"], d["vc"], d["bt"], d["ctx"], bs, dc.LAYER, **sc)
        ops.paged_attention_forward(d["q"], out, d["kc"], d["vc"], d["bt"], d["ctx"], bs, msl, dc.LAYER,
                                    window_size=(left, -1), **sc)

    assert ops.paged_attention_route(d["q"], out, d["kc"], d["vc"], d["bt"], d["ctx"], bs, msl, dc.LAYER,
                                     window_size=(left, -1), **sc) == route
    step()   # warm-up outside the capture (one-time kernel attributes)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    nbytes = lib.mio_fa3_decode_workspace_bytes(B, H, 1, D, msl)
    eager = torch.empty_like(out)
    fam = (dtype, route, "fp8" if kv8 else "kv16")
    for i, s in enumerate(states):
        load(s)
        graph.replay()
        torch.cuda.synchronize()
        what = f"graph-{route}-{fam[2]} state {i} (contexts {s['ctxs']})"
        dc.check(out, s["ref"], s["lse"], dtype, fam, s["model_o"], what, win=left >= 0)
        # the same state (the caches as the replay's write left them) through the C ABI with a fresh all-NaN workspace
        eager.fill_(float("nan"))
        work = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
        args, dt, is8, keep = ops._decode_args(d["q"], eager, d["kc"], d["vc"], d["bt"], d["ctx"], bs, msl, dc.LAYER, None,
                                               sc.get("k_scale"), sc.get("v_scale"))
        stream = ops._stream()
        if is8:
            rc = lib.mio_fa3_decode_paged_kv8(*args, left, dt, work.data_ptr(), stream)
        elif left >= 0:
            rc = lib.mio_fa3_decode_paged_window(*args, left, -1, dt, work.data_ptr(), stream)
        else:
            rc = lib.mio_fa3_decode_paged(*args, dt, work.data_ptr(), stream)
        assert rc == 0, lib.mio_last_error().decode()
        torch.cuda.synchronize()
        del keep
        assert torch.equal(hd.bits(out), hd.bits(eager)), f"{what}: the replay differs from the eager launch"

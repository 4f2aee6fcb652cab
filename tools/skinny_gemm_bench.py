#!/usr/bin/env python3
"""Decode-step GEMM timings on the GPU: ops.gemm_skinny (both launches where the plan splits K) against ops.gemm_bias_act with the
same arguments -- the route such a call takes without the kernel -- in one process, the two legs alternated and the comparison
repeated (--repeats, default 3; the spread of a leg over its repeats is what a difference has to exceed).

A decode step reads every layer's weights once, far more than the 256 MiB Infinity Cache holds, so each leg walks a ring of
weight copies of at least --ring-mib (default 640) in all: every call streams its weight from HBM, as in a step.  --ring-mib 0
times one resident copy instead (what a microbenchmark on one tensor would see).  The calls of one walk are captured into a graph
on one stream and the graph is replayed, so the time per call is kernel time plus the boundary between dependent launches, without
the host's enqueue cost; device events around the replays.

    M in {1, 4, 8, 16, 32, 64} x (N, K) in {(3072, 1024), (1024, 1024), (4096, 1024), (1024, 4096), (6144, 4096), (4096, 4096),
    (4096, 14336)}, plus SwiGLU (14336, 4096)

Prints one JSON line per (M, N, K): microseconds per call of both legs (best repeat, and all), weight bytes / time in TB/s, the
ratio skinny / parent, the plan's split count, the parent's route and what mio_gemm_skinny_ok says.

    python tools/skinny_gemm_bench.py [--m 1,4,8,16,32,64] [--repeats 3] [--replays 5] [--ring-mib 640] [--dtype bf16]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ml-inference-optimizer_amd")):
    sys.path.insert(0, p)
from mio import ops  # noqa: E402

DEV = "cuda"
SHAPES = [(3072, 1024, "none"), (1024, 1024, "none"), (4096, 1024, "none"), (1024, 4096, "none"), (6144, 4096, "none"),
          (4096, 4096, "none"), (4096, 14336, "none"), (14336, 4096, "swiglu")]


def graph_of(fn, calls):
    """fn(i) for i in range(calls), captured on one stream."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for i in range(min(calls, 3)):  # warm-up: code objects, the allocator
            fn(i)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(calls):
            fn(i)
    return g


def timed(g, calls, replays):
    """Microseconds per call over `replays` replays of the graph (device events), after one untimed replay."""
    g.replay()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(replays):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / (replays * calls)


def bench(Ms, N, K, act, dt, ring_bytes, repeats, replays):
    """One (N, K): the ring of weights is built once and every M runs on it."""
    glu = act == "swiglu"
    wbytes = N * K * 2 * (2 if glu else 1)
    ring = max(1, -(-ring_bytes // wbytes))
    calls = ring * max(1, -(-64 // ring))  # whole walks of the ring, 64 calls at least
    g = torch.Generator(device=DEV).manual_seed(N + K)
    rnd = lambda *shape, scale=1.0: (torch.randn(*shape, device=DEV, generator=g) * scale).to(dt)  # noqa: E731
    ws = [rnd(N, K, scale=K ** -0.5) for _ in range(ring)]
    wgs = [rnd(N, K, scale=K ** -0.5) for _ in range(ring)] if glu else [None] * ring
    b = rnd(N, scale=0.5)
    for M in Ms:
        x, r = rnd(M, K), rnd(M, N)
        kw = (lambda i: dict(w_gate=wgs[i % ring])) if glu else (lambda i: dict(residual=r))
        legs = {"skinny": lambda i: ops.gemm_skinny(x, ws[i % ring], b, act, **kw(i)),
                "parent": lambda i: ops.gemm_bias_act(x, ws[i % ring], b, act, **kw(i))}
        ya, yb = legs["skinny"](0).float(), legs["parent"](0).float()
        diff = ((ya - yb).abs().mean() / yb.abs().mean()).item()
        graphs = {k: graph_of(fn, calls) for k, fn in legs.items()}
        us = {k: [] for k in legs}
        for _ in range(repeats):
            for k in legs:
                us[k].append(timed(graphs[k], calls, replays))
        best = {k: min(v) for k, v in us.items()}
        rec = {"M": M, "N": N, "K": K, "act": act, "dtype": str(dt).split(".")[-1], "ring": ring, "calls": calls,
               "splits": ops.gemm_skinny_splits(M, N, K, act), "parent_route": ops.gemm_route(x, ws[0], b, act, **kw(0)),
               "skinny_us": round(best["skinny"], 2), "parent_us": round(best["parent"], 2),
               "ratio": round(best["skinny"] / best["parent"], 3),
               "skinny_TBps": round(wbytes / best["skinny"] / 1e6, 3), "parent_TBps": round(wbytes / best["parent"] / 1e6, 3),
               "skinny_us_all": [round(t, 2) for t in us["skinny"]], "parent_us_all": [round(t, 2) for t in us["parent"]],
               "ok": ops.gemm_skinny_ok(M, N, K, act), "mean_rel_diff": float(f"{diff:.2e}")}
        print(json.dumps(rec), flush=True)
        del graphs
    del ws, wgs
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--m", default="1,4,8,16,32,64")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--replays", type=int, default=5)
    ap.add_argument("--ring-mib", type=int, default=640, help="weight copies walked per leg, in MiB (0: one resident copy)")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--shapes", default="", help="N,K[,act];... instead of the sweep's shapes")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("skinny_gemm_bench.py measures on the GPU: none found")
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float16
    shapes = SHAPES
    if a.shapes:
        shapes = [(int(t[0]), int(t[1]), t[2] if len(t) > 2 else "none") for t in (s.split(",") for s in a.shapes.split(";"))]
    for N, K, act in shapes:
        bench([int(m) for m in a.m.split(",")], N, K, act, dt, a.ring_mib << 20, a.repeats, a.replays)


if __name__ == "__main__":
    main()

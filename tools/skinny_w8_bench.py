#!/usr/bin/env python3
"""Decode-step GEMM timings on weight-only FP8: ops.gemm_skinny_w8 on the quantised weight against the two routes the same call
takes on the 16-bit weight -- ops.gemm_skinny and ops.gemm_bias_act -- in one process, the three legs alternated and the
comparison repeated (--repeats, default 3; the spread of a leg over its repeats is what a difference has to exceed).  The method
is tools/skinny_gemm_bench.py's: each leg walks a ring of weight copies of at least --ring-mib (default 640, more than the 256 MiB
Infinity Cache) in its own storage form, so every call streams its weight from HBM as in a decode step; the calls of one walk are
captured into a graph on one stream and the graph is replayed; device events around the replays.

    M in {1, 4, 8, 16, 32, 64} x (N, K) in {(3072, 1024), (1024, 1024), (4096, 1024), (1024, 4096), (6144, 4096), (4096, 4096),
    (4096, 14336)}, plus SwiGLU (14336, 4096)

Prints one JSON line per (M, N, K): microseconds per call of the three legs (best repeat, and all), weight bytes / time in TB/s
(each leg on the bytes of its own form), the ratio w8 / min(skinny, parent), the plans' split counts, the kernel's chunk and
depth, and what mio_gemm_skinny_w8_ok says; --table adds the rows of profiles/skinny_gemm_w8.md at the end.

    python tools/skinny_w8_bench.py [--m 1,4,8,16,32,64] [--repeats 3] [--replays 5] [--ring-mib 640] [--dtype bf16] [--table]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ml-inference-optimizer_amd")):
    sys.path.insert(0, p)
from mio import _lib, ops  # noqa: E402
from tools.skinny_gemm_bench import SHAPES, graph_of, timed  # noqa: E402

DEV = "cuda"
LEGS = ("w8", "skinny", "parent")


def bench(Ms, N, K, act, dt, ring_bytes, repeats, replays):
    """One (N, K): the rings of weights are built once and every M runs on them."""
    glu = act == "swiglu"
    nw = 2 if glu else 1
    ring16 = max(1, -(-ring_bytes // (N * K * 2 * nw)))
    ring8 = max(1, -(-ring_bytes // (N * K * nw)))
    calls = ring8 * max(1, -(-64 // ring8))  # whole walks of the longer ring, 64 calls at least
    g = torch.Generator(device=DEV).manual_seed(N + K)
    rnd = lambda *shape, scale=1.0: (torch.randn(*shape, device=DEV, generator=g) * scale).to(dt)  # noqa: E731
    ws = [rnd(N, K, scale=K ** -0.5) for _ in range(ring16)]
    wgs = [rnd(N, K, scale=K ** -0.5) for _ in range(ring16)] if glu else [None] * ring16
    q8 = [ops.quantize_weight_w8(ws[i % ring16]) for i in range(ring8)]  # (copies past ring16 repeat a weight: other addresses)
    g8 = [ops.quantize_weight_w8(wgs[i % ring16]) for i in range(ring8)] if glu else [(None, None)] * ring8
    b = rnd(N, scale=0.5)
    a = ops._ACT[act]
    out = []
    for M in Ms:
        x, r = rnd(M, K), rnd(M, N)
        kw = (lambda i: dict(w_gate=wgs[i % ring16])) if glu else (lambda i: dict(residual=r))
        kw8 = (lambda i: dict(w8_gate=g8[i % ring8][0], w_scale_gate=g8[i % ring8][1])) if glu else (lambda i: dict(residual=r))
        legs = {"w8": lambda i: ops.gemm_skinny_w8(x, q8[i % ring8][0], q8[i % ring8][1], b, act, **kw8(i)),
                "skinny": lambda i: ops.gemm_skinny(x, ws[i % ring16], b, act, **kw(i)),
                "parent": lambda i: ops.gemm_bias_act(x, ws[i % ring16], b, act, **kw(i))}
        ya, yb = legs["w8"](0).float(), legs["skinny"](0).float()
        diff = ((ya - yb).norm() / yb.norm()).item()  # (the format's own error: the quantised weight against the 16-bit one)
        graphs = {k: graph_of(legs[k], calls) for k in LEGS}
        us = {k: [] for k in LEGS}
        for _ in range(repeats):
            for k in LEGS:
                us[k].append(timed(graphs[k], calls, replays))
        best = {k: min(v) for k, v in us.items()}
        other = min(best["skinny"], best["parent"])
        rec = {"M": M, "N": N, "K": K, "act": act, "dtype": str(dt).split(".")[-1], "ring8": ring8, "ring16": ring16, "calls": calls,
               "chunk_k": _lib.lib.mio_gemm_skinny_w8_chunk_k(a), "depth": _lib.lib.mio_gemm_skinny_w8_depth(a),
               "splits_w8": ops.gemm_skinny_w8_splits(M, N, K, act), "splits_16": ops.gemm_skinny_splits(M, N, K, act),
               "w8_us": round(best["w8"], 2), "skinny_us": round(best["skinny"], 2), "parent_us": round(best["parent"], 2),
               "ratio": round(best["w8"] / other, 3), "ratio_skinny": round(best["w8"] / best["skinny"], 3),
               "w8_TBps": round(N * K * nw / best["w8"] / 1e6, 3), "skinny_TBps": round(N * K * 2 * nw / best["skinny"] / 1e6, 3),
               "spread": {k: round(max(v) / min(v) - 1.0, 3) for k, v in us.items()},
               "w8_us_all": [round(t, 2) for t in us["w8"]], "skinny_us_all": [round(t, 2) for t in us["skinny"]],
               "parent_us_all": [round(t, 2) for t in us["parent"]], "ok": ops.gemm_skinny_w8_ok(M, N, K, act),
               "normwise_diff_vs_16bit": float(f"{diff:.2e}")}
        print(json.dumps(rec), flush=True)
        out.append(rec)
        del graphs
    del ws, wgs, q8, g8
    torch.cuda.empty_cache()
    return out


def table(recs):
    """The rows of profiles/skinny_gemm_w8.md."""
    print("| N x K | act | M | splits w8 / 16 | w8 us | skinny us | parent us | w8 TB/s | skinny TB/s | w8 / min | spread w8 / skinny / parent |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for r in recs:
        sp = r["spread"]
        print(f"| {r['N']} x {r['K']} | {r['act']} | {r['M']} | {r['splits_w8']} / {r['splits_16']} | {r['w8_us']} | {r['skinny_us']} | "
              f"{r['parent_us']} | {r['w8_TBps']} | {r['skinny_TBps']} | {r['ratio']} | "
              f"{sp['w8'] * 100:.1f} % / {sp['skinny'] * 100:.1f} % / {sp['parent'] * 100:.1f} % |")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--m", default="1,4,8,16,32,64")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--replays", type=int, default=5)
    ap.add_argument("--ring-mib", type=int, default=640, help="weight copies walked per leg, in MiB (0: one resident copy)")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--shapes", default="", help="N,K[,act];... instead of the sweep's shapes")
    ap.add_argument("--table", action="store_true", help="print the markdown rows of the profile after the JSON lines")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("skinny_w8_bench.py measures on the GPU: none found")
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float16
    shapes = SHAPES
    if a.shapes:
        shapes = [(int(t[0]), int(t[1]), t[2] if len(t) > 2 else "none") for t in (s.split(",") for s in a.shapes.split(";"))]
    recs = []
    for N, K, act in shapes:
        recs += bench([int(m) for m in a.m.split(",")], N, K, act, dt, a.ring_mib << 20, a.repeats, a.replays)
    if a.table:
        table(recs)


if __name__ == "__main__":
    main()

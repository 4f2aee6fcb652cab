#!/usr/bin/env python3
"""Decode-step GEMM timings on MXFP4 weights: ops.gemm_skinny_w4 on the quantised weight against ops.gemm_skinny_w8 on the e4m3fn
copy and ops.gemm_skinny on the 16-bit weight itself, in one process, the three legs alternated and the comparison repeated
(--repeats, default 3; the spread of a leg over its repeats is what a difference has to exceed).  The method is
tools/skinny_w8_bench.py's: each leg walks a ring of weight copies of at least --ring-mib (default 640, more than the 256 MiB
Infinity Cache) in its own storage form, so every call streams its weight from HBM; the calls of one walk are captured into a
graph on one stream and the graph is replayed; device events around the replays.

    M in {1, 4, 16, 64} x (N, K) in {(4096, 4096), (6144, 4096), (4096, 14336)}, plus SwiGLU (14336, 4096)

Prints one JSON line per (M, N, K): microseconds per call of the three legs (best repeat, and all), weight bytes / time in TB/s
(each leg on the bytes of its own form, the block scales counted), the ratio w4 / min(w8, skinny), the plans' split counts, the
kernel's chunk and depth, and what mio_gemm_skinny_w4_ok says; --table adds the rows of profiles/skinny_gemm_w4.md at the end.

    python tools/skinny_w4_bench.py [--m 1,4,16,64] [--repeats 3] [--replays 5] [--ring-mib 640] [--table]
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
from tools.skinny_gemm_bench import graph_of, timed  # noqa: E402

DEV, DT = "cuda", torch.bfloat16
LEGS = ("w4", "w8", "skinny")
SHAPES = [(4096, 4096, "none"), (6144, 4096, "none"), (4096, 14336, "none"), (14336, 4096, "swiglu")]


def bench(Ms, N, K, act, ring_bytes, repeats, replays):
    """One (N, K): the rings of weights are built once and every M runs on them."""
    glu = act == "swiglu"
    nw = 2 if glu else 1
    ring16, ring8, ring4 = (max(1, -(-ring_bytes // int(N * K * b * nw))) for b in (2, 1, 0.5))
    calls = ring4 * max(1, -(-64 // ring4))  # whole walks of the longest ring, 64 calls at least
    g = torch.Generator(device=DEV).manual_seed(N + K)
    rnd = lambda *shape, scale=1.0: (torch.randn(*shape, device=DEV, generator=g) * scale).to(DT)  # noqa: E731
    ws = [rnd(N, K, scale=K ** -0.5) for _ in range(ring16)]
    wgs = [rnd(N, K, scale=K ** -0.5) for _ in range(ring16)] if glu else [None] * ring16
    q8 = [ops.quantize_weight_w8(ws[i % ring16]) for i in range(ring8)]  # (copies past ring16 repeat a weight: other addresses)
    g8 = [ops.quantize_weight_w8(wgs[i % ring16]) for i in range(ring8)] if glu else [(None, None)] * ring8
    q4 = [ops.quantize_weight_mxfp4(ws[i % ring16]) for i in range(ring4)]
    g4 = [ops.quantize_weight_mxfp4(wgs[i % ring16]) for i in range(ring4)] if glu else [(None, None)] * ring4
    b = rnd(N, scale=0.5)
    a = ops._ACT[act]
    out = []
    for M in Ms:
        x, r = rnd(M, K), rnd(M, N)
        res = {} if glu else dict(residual=r)
        legs = {"w4": lambda i: ops.gemm_skinny_w4(x, *q4[i % ring4], b, act, *g4[i % ring4], **res),
                "w8": lambda i: ops.gemm_skinny_w8(x, *q8[i % ring8], b, act, *g8[i % ring8], **res),
                "skinny": lambda i: ops.gemm_skinny(x, ws[i % ring16], b, act, wgs[i % ring16], **res)}
        ya, yb = legs["w4"](0).float(), legs["skinny"](0).float()
        diff = ((ya - yb).norm() / yb.norm()).item()  # (the format's own error: the quantised weight against the 16-bit one)
        graphs = {k: graph_of(legs[k], calls) for k in LEGS}
        us = {k: [] for k in LEGS}
        for _ in range(repeats):
            for k in LEGS:
                us[k].append(timed(graphs[k], calls, replays))
        best = {k: min(v) for k, v in us.items()}
        other = min(best["w8"], best["skinny"])
        rec = {"M": M, "N": N, "K": K, "act": act, "rings": [ring4, ring8, ring16], "calls": calls,
               "chunk_k": _lib.lib.mio_gemm_skinny_w4_chunk_k(a), "depth": _lib.lib.mio_gemm_skinny_w4_depth(a),
               "splits": [ops.gemm_skinny_w4_splits(M, N, K, act), ops.gemm_skinny_w8_splits(M, N, K, act), ops.gemm_skinny_splits(M, N, K, act)],
               "w4_us": round(best["w4"], 2), "w8_us": round(best["w8"], 2), "skinny_us": round(best["skinny"], 2),
               "ratio": round(best["w4"] / other, 3), "ratio_w8": round(best["w4"] / best["w8"], 3),
               "w4_TBps": round(N * K * nw * (0.5 + 1 / 32) / best["w4"] / 1e6, 3), "w8_TBps": round(N * K * nw / best["w8"] / 1e6, 3),
               "skinny_TBps": round(N * K * 2 * nw / best["skinny"] / 1e6, 3),
               "spread": {k: round(max(v) / min(v) - 1.0, 3) for k, v in us.items()},
               "us_all": {k: [round(t, 2) for t in v] for k, v in us.items()}, "ok": ops.gemm_skinny_w4_ok(M, N, K, act),
               "normwise_diff_vs_16bit": float(f"{diff:.2e}")}
        print(json.dumps(rec), flush=True)
        out.append(rec)
        del graphs
    del ws, wgs, q8, g8, q4, g4
    torch.cuda.empty_cache()
    return out


def table(recs):
    """The rows of profiles/skinny_gemm_w4.md; a row in bold where the MXFP4 leg loses to the faster alternative."""
    print("| N x K | act | M | splits w4 / w8 / 16 | w4 us | w8 us | skinny us | w4 TB/s | w8 TB/s | skinny TB/s | w4 / min | w4 / w8 | spread w4 / w8 / skinny |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in recs:
        sp, m = r["spread"], "**" if r["ratio"] > 1.0 else ""
        print(f"| {r['N']} x {r['K']} | {r['act']} | {r['M']} | {' / '.join(map(str, r['splits']))} | {r['w4_us']} | {r['w8_us']} | "
              f"{r['skinny_us']} | {r['w4_TBps']} | {r['w8_TBps']} | {r['skinny_TBps']} | {m}{r['ratio']}{m} | {r['ratio_w8']} | "
              f"{sp['w4'] * 100:.1f} % / {sp['w8'] * 100:.1f} % / {sp['skinny'] * 100:.1f} % |")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--m", default="1,4,16,64")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--replays", type=int, default=5)
    ap.add_argument("--ring-mib", type=int, default=640, help="weight copies walked per leg, in MiB")
    ap.add_argument("--shapes", default="", help="N,K[,act];... instead of the sweep's shapes")
    ap.add_argument("--table", action="store_true", help="print the markdown rows of the profile after the JSON lines")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("skinny_w4_bench.py measures on the GPU: none found")
    shapes = SHAPES
    if a.shapes:
        shapes = [(int(t[0]), int(t[1]), t[2] if len(t) > 2 else "none") for t in (s.split(",") for s in a.shapes.split(";"))]
    recs = []
    for N, K, act in shapes:
        recs += bench([int(m) for m in a.m.split(",")], N, K, act, a.ring_mib << 20, a.repeats, a.replays)
    if a.table:
        table(recs)


if __name__ == "__main__":
    main()

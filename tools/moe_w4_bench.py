#!/usr/bin/env python3
"""MXFP4 expert weights against FP8 expert weights on the mixture-of-experts decode step, on the GPU, on the method of
tools/moe_w8_bench.py: two legs in one process, alternated and repeated (--repeats, default 3; the spread of a leg over its
repeats is what a difference has to exceed), each captured into a graph and replayed:

  w8    ops.moe_route + ops.moe_mlp_w8 on ops.quantize_expert_weights_w8 of a bf16 weight: the yardstick
  w4    ops.moe_route + ops.moe_mlp_w4 on ops.quantize_expert_weights_mxfp4 of the very same weight

bf16 SwiGLU, the same logits and so the same routing on both sides.  Each leg walks a ring of weight copies as long as the
HALF-BYTE active experts need to add up to at least --ring-mib (default 640), so that the MXFP4 leg streams its experts from HBM
too.  The 16-bit weights are dropped once quantised.

    Mixtral-8x7B  E 8 / k 2 / d 4096 / I 14336      Qwen3-30B-A3B  E 128 / k 8 / d 2048 / I 768      T in {1, 4, 16, 64}

Prints one JSON line per (shape, T): microseconds per step of each leg (best repeat, and all), the ratio w4 / w8, the bytes of the
active experts' weights and scales over the time for each leg (TB/s), the plans' split counts; then the same as a markdown table,
a row in bold where the MXFP4 leg loses.

    python tools/moe_w4_bench.py [--t 1,4,16,64] [--shapes mixtral,qwen3] [--repeats 3] [--replays 3] [--ring-mib 640]
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
from moe_bench import graph_of, timed  # noqa: E402

DEV = "cuda"
DT = torch.bfloat16
SHAPES = {"mixtral": (8, 2, 4096, 14336), "qwen3": (128, 8, 2048, 768)}


def bench(name, Ts, ring_bytes, repeats, replays):
    E, k, d, I = SHAPES[name]
    g = torch.Generator(device=DEV).manual_seed(E + d)
    rnd = lambda *s, scale=1.0: (torch.randn(*s, device=DEV, generator=g) * scale).to(DT)  # noqa: E731
    rings, recs = [], []
    for T in Ts:
        x = rnd(T, d)
        logits = rnd(T, E, scale=2.0)
        route = ops.moe_route(logits, k)
        torch.cuda.synchronize()
        counts = torch.diff(route.expert_offsets).tolist()
        active = sum(1 for n in counts if n)
        bytes8, bytes4 = active * (3 * d * I + (2 * I + d) * 4), active * 3 * d * I * 17 // 32
        ring = max(1, -(-ring_bytes // bytes4))
        while len(rings) < ring:  # the ring grows to the longest one asked for and is shared
            entry = []
            for n, kk in ((I, d), (I, d), (d, I)):
                w = rnd(E, n, kk, scale=kk ** -0.5)
                entry.append((ops.quantize_expert_weights_w8(w), ops.quantize_expert_weights_mxfp4(w)))
                del w
            rings.append(entry)
        calls = ring * max(1, -(-8 // ring))

        def w8(i):
            (qu, su), (qg, sg), (qd, sd) = (t[0] for t in rings[i % ring])
            return ops.moe_mlp_w8(x, ops.moe_route(logits, k, out=route), qu, su, qd, sd, "swiglu", qg, sg)

        def w4(i):
            (qu, su), (qg, sg), (qd, sd) = (t[1] for t in rings[i % ring])
            return ops.moe_mlp_w4(x, ops.moe_route(logits, k, out=route), qu, su, qd, sd, "swiglu", qg, sg)

        ya, yb = w8(0).float(), w4(0).float()
        diff = ((ya - yb).abs().mean() / ya.abs().mean()).item()
        graphs = {"w8": graph_of(w8, calls), "w4": graph_of(w4, calls)}
        us = {n: [] for n in graphs}
        for _ in range(repeats):
            for n, gr in graphs.items():
                us[n].append(timed(gr.replay, calls, replays))
        best = {n: min(v) for n, v in us.items()}
        rec = {"shape": name, "E": E, "k": k, "d": d, "I": I, "T": T, "active_experts": active, "max_rows": max(counts), "ring": ring,
               "calls": calls, "splits_w8": [ops.moe_up_w8_splits(T, k, E, I, d), ops.moe_down_w8_splits(T, k, E, d, I)],
               "splits_w4": [ops.moe_up_w4_splits(T, k, E, I, d), ops.moe_down_w4_splits(T, k, E, d, I)],
               "w8_us": round(best["w8"], 1), "w4_us": round(best["w4"], 1), "w4_over_w8": round(best["w4"] / best["w8"], 3),
               "w8_TBps": round(bytes8 / best["w8"] / 1e6, 3), "w4_TBps": round(bytes4 / best["w4"] / 1e6, 3),
               "w8_us_all": [round(t, 1) for t in us["w8"]], "w4_us_all": [round(t, 1) for t in us["w4"]],
               "mean_rel_diff_w4_vs_w8": float(f"{diff:.2e}")}
        print(json.dumps(rec), flush=True)
        recs.append(rec)
        del graphs
    del rings
    torch.cuda.empty_cache()
    return recs


def table(recs):
    out = ["| shape | T | active experts | splits w8 (up, down) | splits w4 | w8 us | w4 us | w4 / w8 | w8 TB/s | w4 TB/s |",
           "|---|---|---|---|---|---|---|---|---|---|"]
    for r in recs:
        cells = [r["shape"], r["T"], r["active_experts"], r["splits_w8"], r["splits_w4"], r["w8_us"], r["w4_us"], r["w4_over_w8"],
                 r["w8_TBps"], r["w4_TBps"]]
        mark = "**" if r["w4_over_w8"] > 1.0 else ""
        out.append("| " + " | ".join(f"{mark}{c}{mark}" for c in cells) + " |")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--t", default="1,4,16,64")
    ap.add_argument("--shapes", default="mixtral,qwen3")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--replays", type=int, default=3)
    ap.add_argument("--ring-mib", type=int, default=640, help="half-byte active experts' weight bytes walked per leg, in MiB")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("moe_w4_bench.py measures on the GPU: none found")
    recs = []
    for name in a.shapes.split(","):
        recs += bench(name, [int(t) for t in a.t.split(",")], a.ring_mib << 20, a.repeats, a.replays)
    print(table(recs))


if __name__ == "__main__":
    main()

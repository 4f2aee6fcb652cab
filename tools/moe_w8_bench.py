#!/usr/bin/env python3
"""FP8 expert weights against 16-bit expert weights on the mixture-of-experts decode step, on the GPU, on the method of
tools/moe_bench.py: two legs in one process, alternated and repeated (--repeats, default 3; the spread of a leg over its repeats
is what a difference has to exceed), each captured into a graph and replayed:

  w16   ops.moe_route + ops.moe_mlp on the bf16 expert weights: the existing path, the yardstick
  w8    ops.moe_route + ops.moe_mlp_w8 on ops.quantize_expert_weights_w8 of the very same weights

bf16 SwiGLU, the same logits and so the same routing on both sides.  A decode step reads every layer's weights once, far more than
the 256 MiB Infinity Cache holds, so each leg walks a ring of weight copies; the ring is as long as the ONE-BYTE active experts
need to add up to at least --ring-mib (default 640), so that the FP8 leg streams its experts from HBM too.

    Mixtral-8x7B  E 8 / k 2 / d 4096 / I 14336      Qwen3-30B-A3B  E 128 / k 8 / d 2048 / I 768      T in {1, 4, 16, 64}

Prints one JSON line per (shape, T): microseconds per step of each leg (best repeat, and all), the ratio w8 / w16, the bytes of
the active experts' weights over the time for each leg (TB/s; the one-byte rate counts one byte per weight element plus the
scales), the plans' split counts; then the same as a markdown table, a row in bold where the FP8 leg loses.

    python tools/moe_w8_bench.py [--t 1,4,16,64] [--shapes mixtral,qwen3] [--repeats 3] [--replays 3] [--ring-mib 640]
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
    rings, recs = {}, []
    for T in Ts:
        x = rnd(T, d)
        logits = rnd(T, E, scale=2.0)
        route = ops.moe_route(logits, k)
        torch.cuda.synchronize()
        counts = torch.diff(route.expert_offsets).tolist()
        active = sum(1 for n in counts if n)
        bytes16, bytes8 = active * 3 * d * I * 2, active * (3 * d * I + (2 * I + d) * 4)
        ring = max(1, -(-ring_bytes // bytes8))
        while len(rings) < ring:  # the ring grows to the longest one asked for and is shared
            w = (rnd(E, I, d, scale=d ** -0.5), rnd(E, I, d, scale=d ** -0.5), rnd(E, d, I, scale=I ** -0.5))
            rings[len(rings)] = (w, tuple(ops.quantize_expert_weights_w8(t) for t in w))
        calls = ring * max(1, -(-8 // ring))

        def w16(i):
            wu, wg, wd = rings[i % ring][0]
            return ops.moe_mlp(x, ops.moe_route(logits, k, out=route), wu, wd, "swiglu", wg)

        def w8(i):
            (qu, su), (qg, sg), (qd, sd) = rings[i % ring][1]
            return ops.moe_mlp_w8(x, ops.moe_route(logits, k, out=route), qu, su, qd, sd, "swiglu", qg, sg)

        ya, yb = w16(0).float(), w8(0).float()
        diff = ((ya - yb).abs().mean() / ya.abs().mean()).item()
        graphs = {"w16": graph_of(w16, calls), "w8": graph_of(w8, calls)}
        us = {n: [] for n in graphs}
        for _ in range(repeats):
            for n, gr in graphs.items():
                us[n].append(timed(gr.replay, calls, replays))
        best = {n: min(v) for n, v in us.items()}
        rec = {"shape": name, "E": E, "k": k, "d": d, "I": I, "T": T, "active_experts": active, "max_rows": max(counts), "ring": ring,
               "calls": calls, "splits_w16": [ops.moe_up_splits(T, k, E, I, d), ops.moe_down_splits(T, k, E, d, I)],
               "splits_w8": [ops.moe_up_w8_splits(T, k, E, I, d), ops.moe_down_w8_splits(T, k, E, d, I)],
               "w16_us": round(best["w16"], 1), "w8_us": round(best["w8"], 1), "w8_over_w16": round(best["w8"] / best["w16"], 3),
               "w16_TBps": round(bytes16 / best["w16"] / 1e6, 3), "w8_TBps": round(bytes8 / best["w8"] / 1e6, 3),
               "w16_us_all": [round(t, 1) for t in us["w16"]], "w8_us_all": [round(t, 1) for t in us["w8"]],
               "mean_rel_diff_w8_vs_w16": float(f"{diff:.2e}")}
        print(json.dumps(rec), flush=True)
        recs.append(rec)
        del graphs
    del rings
    torch.cuda.empty_cache()
    return recs


def table(recs):
    out = ["| shape | T | active experts | splits w16 (up, down) | splits w8 | w16 us | w8 us | w8 / w16 | w16 TB/s | w8 TB/s (one byte) |",
           "|---|---|---|---|---|---|---|---|---|---|"]
    for r in recs:
        cells = [r["shape"], r["T"], r["active_experts"], r["splits_w16"], r["splits_w8"], r["w16_us"], r["w8_us"], r["w8_over_w16"],
                 r["w16_TBps"], r["w8_TBps"]]
        mark = "**" if r["w8_over_w16"] > 1.0 else ""
        out.append("| " + " | ".join(f"{mark}{c}{mark}" for c in cells) + " |")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--t", default="1,4,16,64")
    ap.add_argument("--shapes", default="mixtral,qwen3")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--replays", type=int, default=3)
    ap.add_argument("--ring-mib", type=int, default=640, help="one-byte active experts' weight bytes walked per leg, in MiB")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("moe_w8_bench.py measures on the GPU: none found")
    recs = []
    for name in a.shapes.split(","):
        recs += bench(name, [int(t) for t in a.t.split(",")], a.ring_mib << 20, a.repeats, a.replays)
    print(table(recs))


if __name__ == "__main__":
    main()

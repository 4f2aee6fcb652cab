#!/usr/bin/env python3
"""Mixture-of-experts prefill timings on the GPU (bf16, SwiGLU), three legs in one process, alternated and repeated (--repeats,
default 3; the spread of a leg over its repeats is what a difference has to exceed):

  ours     ops.moe_route_prefill + ops.moe_mlp_prefill: one routing, one pass over the active experts' weights; captured into a
           graph and replayed.  Its three stages (route, up, down) are also timed on their own, each in a graph of its own
  chunked  what MoEMLP.forward does without grouped_prefill: ops.moe_route + ops.moe_mlp in row chunks of 64, every chunk streaming
           its experts' weights again; captured into a graph
  torch    the torch-op chain of tools/moe_bench.py (softmax, topk, per expert nonzero / index_select / F.linear x3 /
           index_add_): it reads the routing back to the host, so it runs eager, host time included

    Mixtral-8x7B  E 8 / k 2 / d 4096 / I 14336      Qwen3-30B-A3B  E 128 / k 8 / d 2048 / I 768      narrow  E 64 / k 8 / d 2048 / I 1024
    T in {128, 512, 2048, 8192};  routing: random logits

One set of expert weights per shape (0.8 to 2.8 GB, several times the 256 MiB Infinity Cache).  Times are device events around
graph replays (torch: around eager calls) after an untimed run: call times, not profiler kernel times.  Prints one JSON line per
(shape, T): microseconds of each leg (best repeat, and all), the up GEMM's rate (6 T k d I flops over its time), the active experts'
weight bytes over the whole step's time, and the mean relative difference of ours from the torch chain.

    python tools/moe_prefill_bench.py [--t 128,512,2048,8192] [--shapes mixtral,qwen3,narrow] [--repeats 3] [--replays 3]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ml-inference-optimizer_amd"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
from mio import ops  # noqa: E402
from moe_bench import DEV, DT, SHAPES, graph_of, timed, torch_chain  # noqa: E402


def bench(name, Ts, repeats, replays):
    E, k, d, I = SHAPES[name]
    g = torch.Generator(device=DEV).manual_seed(E + d)
    rnd = lambda *s, scale=1.0: (torch.randn(*s, device=DEV, generator=g) * scale).to(DT)  # noqa: E731
    wu, wg, wd = rnd(E, I, d, scale=d ** -0.5), rnd(E, I, d, scale=d ** -0.5), rnd(E, d, I, scale=I ** -0.5)
    for T in Ts:
        x, logits = rnd(T, d), rnd(T, E, scale=2.0)
        route = ops.moe_route_prefill(logits, k)
        h = ops.moe_up_prefill(x, route, wu, "swiglu", wg)
        ws = torch.empty(T * k * d, dtype=torch.float32, device=DEV)
        y = torch.empty(T, d, dtype=DT, device=DEV)
        torch.cuda.synchronize()
        counts = torch.diff(route.expert_offsets).tolist()
        active = sum(1 for n in counts if n)

        def ours(_):
            r = ops.moe_route_prefill(logits, k, out=route)
            return ops.moe_down_prefill(ops.moe_up_prefill(x, r, wu, "swiglu", wg, out=h), r, wd, out=y, workspace=ws)

        def chunked(_):
            for lo in range(0, T, ops.MOE_MAX_TOKENS):
                xc = x[lo:lo + ops.MOE_MAX_TOKENS]
                ops.moe_mlp(xc, ops.moe_route(logits[lo:lo + ops.MOE_MAX_TOKENS], k), wu, wd, "swiglu", wg, out=y[lo:lo + ops.MOE_MAX_TOKENS])

        ya, yb = ours(0).float(), torch_chain(x, logits, k, wu, wg, wd).float()
        diff = ((ya - yb).abs().mean() / yb.abs().mean()).item()
        stages = {"route": lambda _: ops.moe_route_prefill(logits, k, out=route),
                  "up": lambda _: ops.moe_up_prefill(x, route, wu, "swiglu", wg, out=h),
                  "down": lambda _: ops.moe_down_prefill(h, route, wd, out=y, workspace=ws)}
        graphs = {n: graph_of(f, 1) for n, f in {"ours": ours, "chunked": chunked, **stages}.items()}
        runs = {n: gr.replay for n, gr in graphs.items()}
        runs["torch"] = lambda: torch_chain(x, logits, k, wu, wg, wd)
        us = {n: [] for n in runs}
        for _ in range(repeats):
            for n, run in runs.items():
                us[n].append(timed(run, 1, replays))
        best = {n: min(v) for n, v in us.items()}
        rec = {"shape": name, "E": E, "k": k, "d": d, "I": I, "T": T, "active_experts": active, "max_rows": max(counts),
               "tiles": int(route.num_tiles), "max_tiles": ops.moe_prefill_max_tiles(T, k, E),
               "active_weight_MiB": round(active * 3 * d * I * 2 / 2 ** 20, 1)}
        for n in runs:
            rec[f"{n}_us"] = round(best[n], 1)
            rec[f"{n}_us_all"] = [round(t, 1) for t in us[n]]
        rec["up_TFLOPs"] = round(4.0 * T * k * d * I / best["up"] / 1e6, 1)   # two GEMMs of 2 T k d I flops
        rec["down_TFLOPs"] = round(2.0 * T * k * d * I / best["down"] / 1e6, 1)
        rec["ours_weight_TBps"] = round(active * 3 * d * I * 2 / best["ours"] / 1e6, 3)
        rec["ours_over_chunked"] = round(best["ours"] / best["chunked"], 3)
        rec["ours_over_torch"] = round(best["ours"] / best["torch"], 3)
        rec["mean_rel_diff_vs_torch"] = float(f"{diff:.2e}")
        print(json.dumps(rec), flush=True)
        del graphs, runs
    del wu, wg, wd
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--t", default="128,512,2048,8192")
    ap.add_argument("--shapes", default="mixtral,qwen3,narrow")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--replays", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("moe_prefill_bench.py measures on the GPU: none found")
    for name in a.shapes.split(","):
        bench(name, [int(t) for t in a.t.split(",")], a.repeats, a.replays)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Mixture-of-experts decode-step timings on the GPU, three legs in one process, alternated and repeated (--repeats, default 3; the
spread of a leg over its repeats is what a difference has to exceed):

  ours    ops.moe_route + ops.moe_up + ops.moe_down: the routing stays on the device, captured into a graph and replayed
  torch   the torch-op chain a user has today: softmax, topk, then per expert nonzero / index_select / F.linear (x3, SwiGLU) /
          index_add_.  It reads the routing back to the host, so it cannot be captured: eager, host time included
  skinny  for reference only: the SAME active experts as separate ops.gemm_skinny calls (SwiGLU up, then down) on rows gathered
          in advance, the ids known on the host beforehand -- the per-expert kernel's own rate without grouping, without the
          router, the gather and the combine; captured into a graph

A decode step reads every layer's weights once, far more than the 256 MiB Infinity Cache holds, so each leg walks a ring of
weight copies whose ACTIVE experts add up to at least --ring-mib (default 640): every call streams its experts from HBM.

    Mixtral-8x7B  E 8 / k 2 / d 4096 / I 14336      Qwen3-30B-A3B  E 128 / k 8 / d 2048 / I 768      narrow  E 64 / k 8 / d 2048 / I 1024
    T in {1, 4, 16, 64};  routing: random logits, and skewed (all tokens pick the same experts)

Prints one JSON line per (shape, T, routing): microseconds per step of each leg (best repeat, and all), the bytes of the active
experts' weights over the time (TB/s), the number of active experts and the plan's split counts.

    python tools/moe_bench.py [--t 1,4,16,64] [--shapes mixtral,qwen3,narrow] [--repeats 3] [--replays 3] [--ring-mib 640]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ml-inference-optimizer_amd")):
    sys.path.insert(0, p)
from mio import ops  # noqa: E402

DEV = "cuda"
DT = torch.bfloat16
SHAPES = {"mixtral": (8, 2, 4096, 14336), "qwen3": (128, 8, 2048, 768), "narrow": (64, 8, 2048, 1024)}


def graph_of(fn, calls):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for i in range(min(calls, 2)):
            fn(i)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(calls):
            fn(i)
    return g


def timed(run, calls, replays):
    """Microseconds per call over `replays` runs (device events around them), after one untimed run."""
    run()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(replays):
        run()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / (replays * calls)


def torch_chain(x, logits, k, wu, wg, wd):
    """What a user writes without the kernels: host read-backs (nonzero) every expert, a summation order that is not fixed."""
    p = torch.softmax(logits.float(), -1)
    w, ids = torch.topk(p, k, -1)
    w = (w / w.sum(-1, keepdim=True)).to(x.dtype)
    y = torch.zeros_like(x)
    for e in range(wu.shape[0]):
        t, j = (ids == e).nonzero(as_tuple=True)
        if t.numel() == 0:
            continue
        xe = x.index_select(0, t)
        he = F.silu(F.linear(xe, wg[e])) * F.linear(xe, wu[e])
        y.index_add_(0, t, F.linear(he, wd[e]) * w[t, j, None])
    return y


def bench(name, Ts, ring_bytes, repeats, replays):
    E, k, d, I = SHAPES[name]
    per_expert = 3 * d * I * 2
    g = torch.Generator(device=DEV).manual_seed(E + d)
    rnd = lambda *s, scale=1.0: (torch.randn(*s, device=DEV, generator=g) * scale).to(DT)  # noqa: E731
    rings = {}
    for T in Ts:
        for routing in ("random", "skewed"):
            x = rnd(T, d)
            logits = rnd(T, E, scale=2.0)
            if routing == "skewed":
                logits = logits[:1].expand(T, E).contiguous()
            route = ops.moe_route(logits, k)
            torch.cuda.synchronize()
            counts = torch.diff(route.expert_offsets).tolist()
            active = [e for e, n in enumerate(counts) if n]
            abytes = len(active) * per_expert
            ring = max(1, -(-ring_bytes // abytes))
            while len(rings) < ring:  # the ring grows to the longest one asked for and is shared
                rings[len(rings)] = (rnd(E, I, d, scale=d ** -0.5), rnd(E, I, d, scale=d ** -0.5), rnd(E, d, I, scale=I ** -0.5))
            calls = ring * max(1, -(-8 // ring))

            def ours(i):
                wu, wg, wd = rings[i % ring]
                r = ops.moe_route(logits, k, out=route)
                return ops.moe_down(ops.moe_up(x, r, wu, "swiglu", wg), r, wd)

            rows = {e: (route.sorted_rows[int(route.expert_offsets[e]):int(route.expert_offsets[e + 1])] // k).long() for e in active}
            xs = {e: x.index_select(0, rows[e]) for e in active}

            def skinny(i):
                wu, wg, wd = rings[i % ring]
                for e in active:
                    ops.gemm_skinny(ops.gemm_skinny(xs[e], wu[e], None, "swiglu", w_gate=wg[e]), wd[e])

            def chain():
                for i in range(calls):
                    torch_chain(x, logits, k, *rings[i % ring])

            ya, yb = ours(0).float(), torch_chain(x, logits, k, *rings[0]).float()
            diff = ((ya - yb).abs().mean() / yb.abs().mean()).item()
            graphs = {"ours": graph_of(ours, calls), "skinny": graph_of(skinny, calls)}
            runs = {"ours": graphs["ours"].replay, "torch": chain, "skinny": graphs["skinny"].replay}
            us = {n: [] for n in runs}
            for _ in range(repeats):
                for n, run in runs.items():
                    us[n].append(timed(run, calls, replays))
            best = {n: min(v) for n, v in us.items()}
            rec = {"shape": name, "E": E, "k": k, "d": d, "I": I, "T": T, "routing": routing, "active_experts": len(active),
                   "max_rows": max(counts), "ring": ring, "calls": calls, "up_splits": ops.moe_up_splits(T, k, E, I, d, "swiglu"),
                   "down_splits": ops.moe_down_splits(T, k, E, d, I), "active_MiB": round(abytes / 2 ** 20, 1)}
            for n in runs:
                rec[f"{n}_us"] = round(best[n], 1)
                rec[f"{n}_TBps"] = round(abytes / best[n] / 1e6, 3)
                rec[f"{n}_us_all"] = [round(t, 1) for t in us[n]]
            rec["ours_over_torch"] = round(best["ours"] / best["torch"], 3)
            rec["ours_over_skinny"] = round(best["ours"] / best["skinny"], 3)
            rec["mean_rel_diff_vs_torch"] = float(f"{diff:.2e}")
            print(json.dumps(rec), flush=True)
            del graphs
    del rings
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--t", default="1,4,16,64")
    ap.add_argument("--shapes", default="mixtral,qwen3,narrow")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--replays", type=int, default=3)
    ap.add_argument("--ring-mib", type=int, default=640, help="active experts' weight bytes walked per leg, in MiB")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("moe_bench.py measures on the GPU: none found")
    for name in a.shapes.split(","):
        bench(name, [int(t) for t in a.t.split(",")], a.ring_mib << 20, a.repeats, a.replays)


if __name__ == "__main__":
    main()

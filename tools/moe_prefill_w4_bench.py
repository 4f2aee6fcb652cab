#!/usr/bin/env python3
"""Mixture-of-experts prefill timings on MXFP4 expert weights on the GPU (bf16 activations, SwiGLU), three legs in one process,
alternated and repeated (--repeats, default 3; the spread of a leg over its repeats is what a difference has to exceed):

  ours     ops.moe_route_prefill + ops.moe_mlp_prefill_w4: one routing, one pass over the active experts' MXFP4 bytes; captured
           into a graph and replayed.  Its up and down stages are also timed on their own, each in a graph of its own
  chunked  what MoEMLP.forward did on loaded MXFP4 bytes before the tiled kernel: ops.moe_route + ops.moe_mlp_w4 in row chunks of
           64, every chunk streaming its experts' bytes again; captured into a graph
  bf16     ops.moe_route_prefill + ops.moe_mlp_prefill on the bf16 dequantisation of the same bytes: the 16-bit tiled kernel, four
           times the weight bytes and no conversions; captured into a graph.  ours equals it bit for bit, which is asserted

    Mixtral-8x7B  E 8 / k 2 / d 4096 / I 14336     Qwen3-30B-A3B  E 128 / k 8 / d 2048 / I 768     gpt-oss-like  E 32 / k 4 / d = I = 2880
    T in {128, 512, 2048, 8192};  routing: random logits, the routing of tools/moe_prefill_bench.py

Weights are random nibbles with scale bytes 117 .. 123.  Times are device events around graph replays after an untimed run: call
times, not profiler kernel times.  Prints one JSON line per (shape, T): microseconds of each leg (best repeat, and all), the up and
down GEMMs' rates, the active experts' MXFP4 bytes over the whole step's time, and ours over each of the other two.

    python tools/moe_prefill_w4_bench.py [--t 128,512,2048,8192] [--shapes mixtral,qwen3,gptoss] [--repeats 3] [--replays 3]
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
from moe_bench import DEV, DT, SHAPES, graph_of, timed  # noqa: E402

W4_SHAPES = {"mixtral": SHAPES["mixtral"], "qwen3": SHAPES["qwen3"], "gptoss": (32, 4, 2880, 2880)}
E2M1 = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]


def mxfp4(E, N, K, g):
    """(nibbles [E, N, K / 2], scale bytes [E, N, K / 32], the bf16 dequantisation [E, N, K]), the last made an expert at a time."""
    q = torch.randint(0, 256, (E, N, K // 2), device=DEV, generator=g, dtype=torch.uint8)
    # (scale rows padded to 4 bytes: the strides the kernels take, so no call copies them)
    s = torch.empty(E, N, (K // 32 + 3) // 4 * 4, device=DEV, dtype=torch.uint8)[..., :K // 32]
    s.copy_(torch.randint(117, 124, (E, N, K // 32), device=DEV, generator=g, dtype=torch.uint8))
    table = torch.tensor(E2M1 + [-v for v in E2M1], dtype=torch.float32, device=DEV)
    w = torch.empty(E, N, K, dtype=DT, device=DEV)
    for e in range(E):
        nib = torch.stack([q[e] & 15, q[e] >> 4], dim=-1).flatten(-2).long()
        w[e] = (table[nib] * torch.exp2(s[e].float() - 127.0).repeat_interleave(32, dim=-1)).to(DT)
    return q, s, w


def bench(name, Ts, repeats, replays):
    E, k, d, I = W4_SHAPES[name]
    g = torch.Generator(device=DEV).manual_seed(E + d)
    (qu, su, wu), (qg, sg, wg), (qd, sd, wd) = mxfp4(E, I, d, g), mxfp4(E, I, d, g), mxfp4(E, d, I, g)
    for T in Ts:
        x = torch.randn(T, d, device=DEV, generator=g).to(DT)
        logits = (torch.randn(T, E, device=DEV, generator=g) * 2.0).to(DT)
        route = ops.moe_route_prefill(logits, k)
        h = ops.moe_up_prefill_w4(x, route, qu, su, "swiglu", qg, sg)
        ws = torch.empty(T * k * d, dtype=torch.float32, device=DEV)
        y = torch.empty(T, d, dtype=DT, device=DEV)
        torch.cuda.synchronize()
        counts = torch.diff(route.expert_offsets).tolist()
        active = sum(1 for n in counts if n)

        def ours(_):
            r = ops.moe_route_prefill(logits, k, out=route)
            return ops.moe_down_prefill_w4(ops.moe_up_prefill_w4(x, r, qu, su, "swiglu", qg, sg, out=h), r, qd, sd, out=y, workspace=ws)

        def chunked(_):
            for lo in range(0, T, ops.MOE_MAX_TOKENS):
                hi = lo + ops.MOE_MAX_TOKENS
                ops.moe_mlp_w4(x[lo:hi], ops.moe_route(logits[lo:hi], k), qu, su, qd, sd, "swiglu", qg, sg, out=y[lo:hi])

        def bf16(_):
            r = ops.moe_route_prefill(logits, k, out=route)
            return ops.moe_down_prefill(ops.moe_up_prefill(x, r, wu, "swiglu", wg, out=h), r, wd, out=y, workspace=ws)

        ya = ours(0).clone()
        assert torch.equal(ya.view(torch.int16), bf16(0).view(torch.int16)), "ours differs from the 16-bit kernel on the dequantisation"
        stages = {"up": lambda _: ops.moe_up_prefill_w4(x, route, qu, su, "swiglu", qg, sg, out=h),
                  "down": lambda _: ops.moe_down_prefill_w4(h, route, qd, sd, out=y, workspace=ws)}
        graphs = {n: graph_of(f, 1) for n, f in {"ours": ours, "chunked": chunked, "bf16": bf16, **stages}.items()}
        us = {n: [] for n in graphs}
        for _ in range(repeats):
            for n, gr in graphs.items():
                us[n].append(timed(gr.replay, 1, replays))
        best = {n: min(v) for n, v in us.items()}
        w4_bytes = active * 3 * d * I * (0.5 + 1.0 / 32)
        rec = {"shape": name, "E": E, "k": k, "d": d, "I": I, "T": T, "active_experts": active, "max_rows": max(counts),
               "tiles": int(route.num_tiles), "active_w4_MiB": round(w4_bytes / 2 ** 20, 1)}
        for n in graphs:
            rec[f"{n}_us"] = round(best[n], 1)
            rec[f"{n}_us_all"] = [round(t, 1) for t in us[n]]
        rec["up_TFLOPs"] = round(4.0 * T * k * d * I / best["up"] / 1e6, 1)   # two GEMMs of 2 T k d I flops
        rec["down_TFLOPs"] = round(2.0 * T * k * d * I / best["down"] / 1e6, 1)
        rec["ours_w4_TBps"] = round(w4_bytes / best["ours"] / 1e6, 3)
        rec["ours_over_chunked"] = round(best["ours"] / best["chunked"], 3)
        rec["ours_over_bf16"] = round(best["ours"] / best["bf16"], 3)
        print(json.dumps(rec), flush=True)
        del graphs
    del qu, su, wu, qg, sg, wg, qd, sd, wd
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--t", default="128,512,2048,8192")
    ap.add_argument("--shapes", default="mixtral,qwen3,gptoss")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--replays", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("moe_prefill_w4_bench.py measures on the GPU: none found")
    for name in a.shapes.split(","):
        bench(name, [int(t) for t in a.t.split(",")], a.repeats, a.replays)


if __name__ == "__main__":
    main()

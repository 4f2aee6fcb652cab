#!/usr/bin/env python3
"""Kernel times of on-device token sampling (ops.sample_tokens, one launch) against the torch-op chain a user runs without it:
sort of each row, softmax, cumsum, masks, renormalisation, multinomial.  Also the LM-head GEMM (ops.gemm_skinny, d = 4096) that
produces the logits at the same (B, V), so the sampler's share of a decode step can be read off.

Cases: B in {1, 8, 64} x V in {32000, 50257, 128256, 262144} x {bf16, fp32} logits x filter sets {off, top-k 50, top-p 0.95, all
three (top-k 50, top-p 0.95, min-p 0.02)}, temperature 0.8, logits N(0, 2.5^2).  Every variant is captured in a graph of REPS
back-to-back steps and the replays are timed with events after a sustained warm-up (tools/kbench.py: timeit), so the figures are
device times, not Python's launch overhead.  A chain that cannot be captured is timed eagerly and marked so.
Needs a GPU; prints progress on stderr and one JSON line on stdout."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ml-inference-optimizer_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

REPS = 10
BATCHES = (1, 8, 64)
VOCABS = (32000, 50257, 128256, 262144)
DTYPES = ("bf16", "fp32")
FILTERS = {"off": {}, "top_k": dict(top_k=50), "top_p": dict(top_p=0.95), "all": dict(top_k=50, top_p=0.95, min_p=0.02)}
TEMPERATURE = 0.8
D_MODEL = 4096


def torch_chain(logits, temperature, top_k=None, top_p=None, min_p=None):
    """The same semantics with torch ops (a full sort of each row): what the one launch replaces."""
    x = logits.float() / temperature
    vals, idx = torch.sort(x, dim=-1, descending=True, stable=True)
    if top_k is not None:
        vals[:, top_k:] = float("-inf")
    probs = torch.softmax(vals, dim=-1)
    if top_p is not None:
        before = torch.cumsum(probs, dim=-1) - probs
        probs = probs.masked_fill(before >= top_p, 0.0)
    if min_p is not None:
        probs = probs.masked_fill(probs < min_p * probs[:, :1], 0.0)
    probs = probs / probs.sum(-1, keepdim=True)
    pick = torch.multinomial(probs, 1)
    return idx.gather(1, pick).squeeze(1)


def graph_time(step, iters, sustain):
    """(seconds per step, captured): REPS steps in one graph where the step can be captured, else eager."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    try:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(REPS):
                step()
        fn, n, captured = graph.replay, REPS, True
    except Exception:  # noqa: BLE001  (an op of the chain that synchronises)
        torch.cuda.synchronize()
        fn, n, captured = step, 1, False
    return kbench.timeit(fn, iters, sustain_s=sustain) / n, captured


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--sustain", type=float, default=0.2, help="seconds of warm-up (and at least as much timed) per figure")
    ap.add_argument("--batches", default=",".join(map(str, BATCHES)))
    ap.add_argument("--vocabs", default=",".join(map(str, VOCABS)))
    ap.add_argument("--no-gemm", action="store_true")
    a = ap.parse_args()
    global torch, kbench
    import torch
    import kbench
    from mio import ops
    if not torch.cuda.is_available():
        print("sampling_bench needs a GPU", file=sys.stderr)
        return 1
    dev = "cuda"
    out = {"temperature": TEMPERATURE, "reps_per_graph": REPS, "cases": {}, "lm_head": {}}
    g = torch.Generator(device=dev).manual_seed(1)
    for V in map(int, a.vocabs.split(",")):
        w = None if a.no_gemm else (torch.randn(V, D_MODEL, device=dev, generator=g) * 0.02).to(torch.bfloat16)
        for B in map(int, a.batches.split(",")):
            if w is not None:
                h = torch.randn(B, D_MODEL, device=dev, generator=g).to(torch.bfloat16)
                y = torch.empty(B, V, device=dev, dtype=torch.bfloat16)
                try:
                    t, _ = graph_time(lambda: ops.gemm_skinny(h, w, out=y), a.iters, a.sustain)
                    out["lm_head"][f"B{B}-V{V}"] = round(t * 1e6, 2)
                    print(f"lm head gemm_skinny B {B} V {V} d {D_MODEL}: {t * 1e6:.2f} us", file=sys.stderr, flush=True)
                except (ValueError, RuntimeError) as e:  # a shape the decode GEMM does not take
                    out["lm_head"][f"B{B}-V{V}"] = f"not measured: {str(e)[:120]}"
                    print(f"lm head gemm_skinny B {B} V {V}: {e}", file=sys.stderr, flush=True)
            base = torch.randn(B, V, device=dev, generator=g) * 2.5
            u = torch.rand(B, device=dev, generator=g)
            T = torch.full((B,), TEMPERATURE, device=dev)
            for dt in DTYPES:
                x = base.to(torch.bfloat16 if dt == "bf16" else torch.float32)
                for name, f in FILTERS.items():
                    # device tensors for the parameters, as a serving loop holds them: nothing but the one launch is timed
                    kw = {k: torch.full((B,), v, device=dev, dtype=torch.int32 if k == "top_k" else torch.float32)
                          for k, v in f.items()}
                    t_k, _ = graph_time(lambda: ops.sample_tokens(x, T, u=u, **kw), a.iters, a.sustain)
                    t_c, cap = graph_time(lambda: torch_chain(x, TEMPERATURE, **f), a.iters, a.sustain)
                    key = f"B{B}-V{V}-{dt}-{name}"
                    out["cases"][key] = dict(kernel_us=round(t_k * 1e6, 2), chain_us=round(t_c * 1e6, 2),
                                             chain_over_kernel=round(t_c / t_k, 2), chain_captured=cap)
                    print(f"{key}: kernel {t_k * 1e6:.2f} us | torch chain {t_c * 1e6:.2f} us"
                          f"{'' if cap else ' (eager)'} | chain / kernel {t_c / t_k:.2f}", file=sys.stderr, flush=True)
        del w
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())

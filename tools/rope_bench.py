#!/usr/bin/env python3
"""Kernel times of the rotary cache write (ops.rope_and_cache_varlen) against the chain it replaces: rotation of q and k by
torch elementwise ops (fp32 maths, rounded to 16 bits), then ops.reshape_and_cache_varlen.

Both variants are captured in a CUDA graph of REPS back-to-back steps and the replays are timed with HIP events after a
warm-up (tools/kbench.py's timeit), so the figures are the kernels' times, not Python's launch overhead -- which would
otherwise dominate the chain's dozen small launches.  The chain gets its positions precomputed outside the timed region.
Shapes: 16 x 512 new tokens (a prefill chunk) and 64 x 1 (a decode step), each after 4096 cached tokens, block size 16, at
H 32 / Hkv 8 / D 128 and H 16 / Hkv 16 / D 64, rot_dim = D, neox pairing, bf16 inputs; caches bf16 and fp8 (e4m3fn).
Bytes counted are what the operation must move: q, k, v read and q_out written at 16 bits, K and V written at the cache's
width; TB/s = those bytes / time, for both variants.
Every case runs in a child process of its own under a time limit; the first failure ends the run.  Prints one JSON line."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ml-inference-optimizer_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SHAPES = {"prefill": (16, 512), "decode": (64, 1)}          # sequences x new tokens per sequence
HEADS = {"gqa128": (32, 8, 128), "mha64": (16, 16, 64)}     # H, Hkv, D
CACHES = ("bf16", "fp8")
CACHED, BS, REPS = 4096, 16, 20
CASES = [f"{s}-{h}-{c}" for s in SHAPES for h in HEADS for c in CACHES]


def _torch_rotate(x, c, s):
    """neox rotation of x [T, heads, D] by c / s [T, 1, D / 2] fp32, as a user writes it with torch ops."""
    h = x.shape[-1] // 2
    x1, x2 = x[..., :h].float(), x[..., h:].float()
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1).to(x.dtype)


def _graph_time(step, iters):
    """Seconds per step: REPS steps captured in one graph, replays timed."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(REPS):
            step()
    return timeit(graph.replay, iters) / REPS


def run_case(name, iters):
    shape, heads, kind = name.split("-")
    B, n = SHAPES[shape]
    H, Hkv, D = HEADS[heads]
    dev, dt = "cuda", torch.bfloat16
    T = B * n
    maxb = (CACHED + n + BS - 1) // BS
    nb = B * maxb
    g = torch.Generator(device=dev).manual_seed(1)
    bt = torch.randperm(nb, device=dev, generator=g).view(B, maxb).to(torch.int32)
    cl = torch.full((B,), CACHED + n, dtype=torch.int32, device=dev)
    cu = torch.arange(0, T + 1, n, dtype=torch.int32, device=dev)
    qkv = torch.randn(T, (H + 2 * Hkv) * D, device=dev, dtype=dt, generator=g)
    q = qkv[:, :H * D].view(T, H, D)
    k = qkv[:, H * D:(H + Hkv) * D].view(T, Hkv, D)
    v = qkv[:, (H + Hkv) * D:].view(T, Hkv, D)
    cdt = dt if kind == "bf16" else torch.float8_e4m3fn
    kc = torch.zeros(nb, 1, BS, Hkv, D, device=dev, dtype=cdt)
    vc = torch.zeros(nb, 1, BS, Hkv, D, device=dev, dtype=cdt)
    kw = {} if kind == "bf16" else dict(k_scale=torch.ones(1, device=dev), v_scale=torch.ones(1, device=dev))
    cos, sin = ops.rope_tables(8192, D, device=dev)
    q_out = torch.empty(T, H, D, device=dev, dtype=dt)
    pos = (CACHED + torch.arange(n, device=dev)).repeat(B)   # the chain's positions, outside the timed region

    def fused():
        ops.rope_and_cache_varlen(q, k, v, kc, vc, bt, cu, cl, BS, 0, cos, sin, q_out=q_out, **kw)

    def chain():
        c, s = cos[pos][:, None, :], sin[pos][:, None, :]
        q_out.copy_(_torch_rotate(q, c, s))
        ops.reshape_and_cache_varlen(_torch_rotate(k, c, s), v, kc, vc, bt, cu, cl, BS, 0, **kw)

    nbytes = T * (2 * H * D * 2 + 2 * Hkv * D * (2 + kc.element_size()))
    res = dict(B=B, new=n, H=H, Hkv=Hkv, D=D, cache=kind, bytes=nbytes)
    for what, step in (("fused", fused), ("chain", chain)):
        t = _graph_time(step, iters)
        res[what] = dict(us=round(t * 1e6, 2), tb_s=round(nbytes / t / 1e12, 3))
    res["chain_over_fused"] = round(res["chain"]["us"] / res["fused"]["us"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--timeout", type=int, default=120, help="seconds per case")
    ap.add_argument("--case", help="run this one case in this process (what the parent starts)")
    a = ap.parse_args()
    if a.case:
        global torch, ops, timeit
        import torch
        from mio import ops
        from kbench import timeit
        print(json.dumps(run_case(a.case, a.iters)), flush=True)
        return 0
    out = {}
    for name in a.cases.split(","):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--iters", str(a.iters)],
                               capture_output=True, text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            print(f"{name}: no result within {a.timeout} s; stopping", file=sys.stderr, flush=True)
            return 1
        if r.returncode != 0:
            print(f"{name}: exit status {r.returncode}; stopping\n{r.stderr[-2000:]}", file=sys.stderr, flush=True)
            return 1
        out[name] = json.loads(r.stdout.strip().splitlines()[-1])
        f, c = out[name]["fused"], out[name]["chain"]
        print(f"{name}: fused {f['us']} us {f['tb_s']} TB/s | chain {c['us']} us {c['tb_s']} TB/s | chain / fused "
              f"{out[name]['chain_over_fused']}", file=sys.stderr, flush=True)
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())

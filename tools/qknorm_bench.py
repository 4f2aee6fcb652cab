#!/usr/bin/env python3
"""Kernel times of the QK-norm rotary cache write (ops.qknorm_rope_and_cache_varlen) against
  (a) chain: the per-head RMSNorm of q and k as torch ops (fp32 maths, rounded to 16 bits), then ops.rope_and_cache_varlen --
      what a user runs without the fused write;
  (b) rope: ops.rope_and_cache_varlen alone on the same tensors -- the kernel without the norm, moving the same bytes; the
      ratio fused / rope is what the statistic (the lane groups, the butterfly, the weight loads) costs.

The cases, the graph capture of REPS back-to-back steps and the timing of the replays are tools/rope_bench.py's, so the figures
are the kernels' times, not Python's launch overhead.  Shapes: 16 x 512 new tokens (a prefill chunk) and 64 x 1 (a decode
step), each after 4096 cached tokens, block size 16, at H 32 / Hkv 8 / D 128 and H 16 / Hkv 16 / D 64, rot_dim = D, neox
pairing, bf16 inputs; caches bf16 and fp8 (e4m3fn).  Bytes counted are what the operation must move: q, k, v read and q_out
written at 16 bits, K and V written at the cache's width.
Every case runs in a child process of its own under a time limit; the first failure ends the run.  Prints one JSON line."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ml-inference-optimizer_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from rope_bench import BS, CACHED, CASES, HEADS, SHAPES  # noqa: E402  (the same cases)

EPS = 1e-6
VARIANTS = ("fused", "chain", "rope")


def _torch_rms(x, w):
    """per-head RMSNorm of x [T, heads, D] as a user writes it with torch ops"""
    xf = x.float()
    return (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + EPS) * w.float()).to(x.dtype)


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
    wq = (0.5 + torch.rand(D, device=dev, generator=g)).to(dt)
    wk = (0.5 + torch.rand(D, device=dev, generator=g)).to(dt)
    cdt = dt if kind == "bf16" else torch.float8_e4m3fn
    kc = torch.zeros(nb, 1, BS, Hkv, D, device=dev, dtype=cdt)
    vc = torch.zeros(nb, 1, BS, Hkv, D, device=dev, dtype=cdt)
    kw = {} if kind == "bf16" else dict(k_scale=torch.ones(1, device=dev), v_scale=torch.ones(1, device=dev))
    cos, sin = ops.rope_tables(8192, D, device=dev)
    q_out = torch.empty(T, H, D, device=dev, dtype=dt)

    def fused():
        ops.qknorm_rope_and_cache_varlen(q, k, v, kc, vc, bt, cu, cl, BS, 0, cos, sin, wq, wk, eps=EPS, q_out=q_out, **kw)

    def chain():
        ops.rope_and_cache_varlen(_torch_rms(q, wq), _torch_rms(k, wk), v, kc, vc, bt, cu, cl, BS, 0, cos, sin, q_out=q_out, **kw)

    def rope():
        ops.rope_and_cache_varlen(q, k, v, kc, vc, bt, cu, cl, BS, 0, cos, sin, q_out=q_out, **kw)

    nbytes = T * (2 * H * D * 2 + 2 * Hkv * D * (2 + kc.element_size()))
    res = dict(B=B, new=n, H=H, Hkv=Hkv, D=D, cache=kind, bytes=nbytes)
    for what, step in zip(VARIANTS, (fused, chain, rope)):
        t = _graph_time(step, iters)
        res[what] = dict(us=round(t * 1e6, 2), tb_s=round(nbytes / t / 1e12, 3))
    res["chain_over_fused"] = round(res["chain"]["us"] / res["fused"]["us"], 2)
    res["fused_over_rope"] = round(res["fused"]["us"] / res["rope"]["us"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--timeout", type=int, default=120, help="seconds per case")
    ap.add_argument("--case", help="run this one case in this process (what the parent starts)")
    a = ap.parse_args()
    if a.case:
        global torch, ops, _graph_time
        import torch
        from mio import ops
        import rope_bench
        import kbench
        rope_bench.torch, rope_bench.timeit = torch, kbench.timeit  # the globals its _graph_time reads
        _graph_time = rope_bench._graph_time
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
        o = out[name]
        print(f"{name}: fused {o['fused']['us']} us {o['fused']['tb_s']} TB/s | chain {o['chain']['us']} us | rope "
              f"{o['rope']['us']} us | chain / fused {o['chain_over_fused']} | fused / rope {o['fused_over_rope']}",
              file=sys.stderr, flush=True)
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())

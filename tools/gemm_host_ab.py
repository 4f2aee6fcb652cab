#!/usr/bin/env python3
"""Host-path timings of the GEMM / fused-MLP wrappers, for A/B runs of two builds of this tree (profiles/gemm_host_ab.md).
Prints one JSON line.
  --what small   gemm_bias_act at M = 64, N = K = 256 and fused_mlp at [1, 64, 256], I = 1024 (kbench.timeit, us per call):
                 launches so short that the host path is the larger share of a call
  --what route   10^5 mio_gemm_route calls through ctypes at the benchmark's fc1 shape (us per call; needs no GPU)"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ml-inference-optimizer_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def small():
    import torch
    from kbench import timeit
    from mio import ops
    dev, dt = "cuda", torch.bfloat16
    torch.manual_seed(0)
    M, d, I = 64, 256, 1024
    x = torch.randn(M, d, device=dev, dtype=dt)
    w = (torch.randn(d, d, device=dev) * 0.02).to(dt)
    b = torch.zeros(d, device=dev, dtype=dt)
    out = torch.empty(M, d, device=dev, dtype=dt)
    w1 = (torch.randn(I, d, device=dev) * 0.02).to(dt)
    w2 = (torch.randn(d, I, device=dev) * 0.02).to(dt)
    b1 = torch.zeros(I, device=dev, dtype=dt)
    xs = x.view(1, M, d)
    return {"gemm_bias_act_64x256x256_us": timeit(lambda: ops.gemm_bias_act(x, w, b, "none", out=out)) * 1e6,
            "fused_mlp_1x64x256_I1024_us": timeit(lambda: ops.fused_mlp(xs, w1, b1, w2, b, "gelu")) * 1e6}


def route(n=100000):
    from mio import _lib
    f = _lib.lib.mio_gemm_route
    M, N, K = 8 * 4096, 4096, 1024
    t0 = time.perf_counter()
    for _ in range(n):
        r = f(M, N, K, K, K, N, 0, _lib.ACT_GELU_TANH, 0, _lib.W_BLOCKED, 0, 0)
    t = time.perf_counter() - t0
    assert _lib.GEMM_ROUTES[r] == "p8w"
    return {"mio_gemm_route_c2_fc1_us": t / n * 1e6}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("small", "route"), default="small")
    a = ap.parse_args()
    print(json.dumps({k: round(v, 3) for k, v in (small() if a.what == "small" else route()).items()}))

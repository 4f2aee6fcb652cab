#!/usr/bin/env python3
"""Kernel times of the packed variable-length attention forward (ops.flash_attention_varlen), HIP events with warm-up as in
tools/kbench.py, random bf16 data.  Useful FLOP = 4 * D * H * (visible query-key pairs) of the real tokens only; the share
of the dense bf16 MFMA peak (2500 TFLOP/s, bench.py) is printed beside it.
  (a) a ragged batch (16 sequences, lengths uniform in 512 .. 4096, H 16, causal, D 64 and D 128): the varlen path against
      the same batch padded to the longest sequence through ops.flash_attention(mask=keep) (route fwd1_keep);
  (b) a uniform 8 x 4096 batch: the varlen path against the dense ops.fa3_fwd launch (route fwd5 / fwd3).
Prints one line per measurement."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ml-inference-optimizer_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mio import ops  # noqa: E402
from kbench import timeit  # noqa: E402

PEAK_TFLOPS = 2500.0


def useful_flops(lens, H, D, causal):
    pairs = sum(n * (n + 1) // 2 if causal else n * n for n in lens)
    return 4.0 * D * H * pairs


def report(name, t, fl):
    print(f"{name}: {t * 1e3:.3f} ms  {fl / t / 1e12:.1f} TFLOP/s useful  {fl / t / 1e12 / PEAK_TFLOPS:.3f} of MFMA peak",
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    dev, dt, H = "cuda", torch.bfloat16, 16
    g = torch.Generator().manual_seed(a.seed)
    lens = torch.randint(512, 4097, (16,), generator=g).tolist()
    print(f"(a) ragged batch, lengths {lens}", flush=True)
    for D in (64, 128):
        B, S, T = len(lens), max(lens), sum(lens)
        cu = torch.tensor([0] + torch.cumsum(torch.tensor(lens), 0).tolist(), dtype=torch.int32, device=dev)
        q, k, v = (torch.randn(T, H, D, device=dev, dtype=dt) for _ in range(3))
        route = ops.fa3_varlen_route(q, k, v, cu, cu, S, S, causal=True)
        out = torch.empty_like(q)
        t = timeit(lambda: ops.flash_attention_varlen(q, k, v, cu, cu, S, S, causal=True, out=out), a.iters)
        fl = useful_flops(lens, H, D, True)
        report(f"  D{D} varlen ({route})", t, fl)
        keep = torch.zeros(B, S, dtype=torch.bool, device=dev)
        for b, n in enumerate(lens):
            keep[b, :n] = True
        qp, kp, vp = (torch.randn(B, S, H, D, device=dev, dtype=dt) for _ in range(3))
        km = keep[:, None, None, :].to(torch.uint8)
        droute = ops.fa3_route(qp, kp, vp, causal=True, keep_mask=km)
        outp = torch.empty_like(qp)
        tp = timeit(lambda: ops.fa3_fwd(qp, kp, vp, causal=True, keep_mask=km, out=outp), a.iters)
        report(f"  D{D} padded + keep-mask ({droute})", tp, fl)
        print(f"  D{D} varlen speed-up over the keep-mask path: {tp / t:.2f}x", flush=True)
        del q, k, v, qp, kp, vp, out, outp
    print("(b) uniform 8 x 4096", flush=True)
    B, S = 8, 4096
    for D in (64, 128):
        for causal in (True, False):
            qd, kd, vd = (torch.randn(B, S, H, D, device=dev, dtype=dt) for _ in range(3))
            q, k, v = (x.view(B * S, H, D) for x in (qd, kd, vd))
            cu = torch.arange(0, B * S + 1, S, dtype=torch.int32, device=dev)
            fl = useful_flops([S] * B, H, D, causal)
            out = torch.empty_like(q)
            outd = torch.empty_like(qd)
            route = ops.fa3_varlen_route(q, k, v, cu, cu, S, S, causal=causal)
            droute = ops.fa3_route(qd, kd, vd, causal=causal)
            # interleaved: dense, varlen, dense, varlen
            td, tv = [], []
            for _ in range(2):
                td.append(timeit(lambda: ops.fa3_fwd(qd, kd, vd, causal=causal, out=outd), a.iters))
                tv.append(timeit(lambda: ops.flash_attention_varlen(q, k, v, cu, cu, S, S, causal=causal, out=out), a.iters))
            report(f"  D{D} causal={causal} dense ({droute})", min(td), fl)
            report(f"  D{D} causal={causal} varlen ({route})", min(tv), fl)
            print(f"  D{D} causal={causal} varlen / dense time: {min(tv) / min(td):.3f}", flush=True)
            del qd, kd, vd, out, outd


if __name__ == "__main__":
    main()

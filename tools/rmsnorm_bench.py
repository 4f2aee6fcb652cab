#!/usr/bin/env python3
"""RMSNorm timings on the GPU, device events around queued launches, every shape warmed up, the variants of a comparison
alternated inside one process and the whole comparison repeated (--repeats, default 3: the widest minus the narrowest LayerNorm
time of a shape over the repeats is the spread a difference has to exceed):
  rows   ops.rmsnorm against ops.layernorm and against the chain of torch ops an RMSNorm is without a kernel, at [32768, 1024],
         [32768, 4096] and [8192, 8192] (the last is past LayerNorm's 4096 columns: RMSNorm and the chain only), plain and with
         residual + stored sum; bytes are what the algorithm has to move (x [+ residual] in, y [+ sum] out), TB/s from them;
  gemm   the folded consumer GEMM, LayerNorm form against RMS form, at the c2_qkv_ln_fold and c2_fc1_ln_fold shapes of
         tests/test_gemm_route_host.py (the same kernel: the RMS form differs by one select per row);
  block  synthetic.Block(norm="rms", activation="swiglu"), d 1024 / I 2048 / B 8 / S 4096, both RMSNorms folded into the GEMMs
         against fold=False (every RMSNorm as its own kernel).
Prints one JSON line per measurement.

    python tools/rmsnorm_bench.py [--what rows,gemm,block] [--repeats 3] [--iters 200]
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
from mio.synthetic import Block  # noqa: E402

DT = torch.bfloat16
DEV = "cuda"


def timed(fn, iters, warmup=5):
    """Mean milliseconds of fn() over `iters` queued calls (device events)."""
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def alternate(variants, repeats, iters):
    """{name: [ms per repeat]}: in every repeat each variant is timed once, in turn."""
    out = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():
            out[k].append(timed(fn, iters))
    return out


def torch_chain(x, w, eps, residual=None, alpha=1.0):
    """RMSNorm as torch elementwise ops (the LLaMA module's forward): the sum, then fp32 variance, rsqrt, two products."""
    s = x if residual is None else x + alpha * residual
    f = s.float()
    y = (f * torch.rsqrt(f.pow(2).mean(-1, keepdim=True) + eps)).to(x.dtype) * w
    return y, s


def report(what, shape, form, ms, nbytes=None, **extra):
    rec = {"what": what, "shape": shape, "form": form}
    for k, v in ms.items():
        rec[k + "_ms"] = [round(t, 4) for t in v]
        if nbytes is not None:
            rec[k + "_TBps"] = round(nbytes / (min(v) * 1e-3) / 1e12, 3)
    if nbytes is not None:
        rec["bytes"] = nbytes
    rec.update(extra)
    print(json.dumps(rec), flush=True)


def bench_rows(repeats, iters):
    for rows, cols in ((32768, 1024), (32768, 4096), (8192, 8192)):
        x = torch.randn(rows, cols, device=DEV, dtype=DT)
        r = torch.randn(rows, cols, device=DEV, dtype=DT)
        w = (1 + 0.1 * torch.randn(cols, device=DEV)).to(DT)
        b = (0.1 * torch.randn(cols, device=DEV)).to(DT)
        for form in ("plain", "residual_sum"):
            res = form == "residual_sum"
            kw = dict(residual=r, residual_alpha=0.5, return_sum=True) if res else {}
            v = {"rmsnorm": lambda: ops.rmsnorm(x, w, 1e-6, **kw)}
            if cols <= 4096:
                v["layernorm"] = lambda: ops.layernorm(x, w, b, 1e-5, **kw)
            v["torch_chain"] = lambda: torch_chain(x, w, 1e-6, r if res else None, 0.5)
            ms = alternate(v, repeats, iters)
            extra = {}
            if "layernorm" in ms:
                extra["layernorm_spread_ms"] = round(max(ms["layernorm"]) - min(ms["layernorm"]), 4)
            extra["chain_over_rmsnorm"] = round(min(ms["torch_chain"]) / min(ms["rmsnorm"]), 2)
            report("rows", [rows, cols], form, ms, nbytes=rows * cols * 2 * (4 if res else 2), **extra)


def bench_gemm(repeats, iters):
    M, K = 8 * 4096, 1024
    x0 = torch.randn(M, K, device=DEV, dtype=DT)
    r0 = (torch.randn(M, K, device=DEV) + 0.3).to(DT)
    wp = (torch.randn(K, K, device=DEV) * 0.03).to(DT)
    stream, st = ops.gemm_ln(x0, ops.block_weight(wp), None, M=M, N=K, K=K, residual=r0, out_blocked=True, stats_out=True)
    gam = (1 + 0.1 * torch.randn(K, device=DEV)).to(DT)
    bet = (0.1 * torch.randn(K, device=DEV)).to(DT)
    for name, N, act in (("c2_qkv_ln_fold", 3072, "none"), ("c2_fc1_ln_fold", 4096, "gelu")):
        wc = (torch.randn(N, K, device=DEV) * 0.03).to(DT)
        bc = (torch.randn(N, device=DEV) * 0.05).to(DT)
        wl, bl = ops.ln_fold_weight(wc, gam, bet, bc)
        wr, br = ops.rms_fold_weight(wc, gam, bc)
        kw = dict(M=M, N=N, K=K, activation=act, x_blocked=True, ln_stats=st)
        ms = alternate({"layernorm_fold": lambda: ops.gemm_ln(stream, wl, bl, eps=1e-5, **kw),
                        "rms_fold": lambda: ops.gemm_ln(stream, wr, br, eps=1e-6, norm="rms", **kw)}, repeats, iters)
        report("gemm", [M, N, K], name, ms,
               layernorm_fold_spread_ms=round(max(ms["layernorm_fold"]) - min(ms["layernorm_fold"]), 4),
               TFLOPs_rms=round(2.0 * M * N * K / (min(ms["rms_fold"]) * 1e-3) / 1e12, 1))


def bench_block(repeats, iters):
    d, H, I, B, S = 1024, 16, 2048, 8, 4096
    torch.manual_seed(0)
    blk = Block(d, H, I, causal=True, precision="bf16", activation="swiglu", norm="rms").to(DEV, DT).eval()
    with torch.no_grad():
        for p_ in blk.parameters():
            p_.copy_(torch.randn_like(p_) * 0.03)
        blk.ln_1.weight.add_(1.0)
        blk.ln_2.weight.add_(1.0)
        x = torch.randn(B, S, d, device=DEV, dtype=DT) + 0.3
        assert blk.stream_ok(B, S, DT)
        ms = alternate({"folded": lambda: blk(x), "unfolded": lambda: blk(x, fold=False)}, repeats, max(10, iters // 10))
        a, b = blk(x).float(), blk(x, fold=False).float()
    report("block", [B, S, d, I], "rms_swiglu", ms, unfolded_over_folded=round(min(ms["unfolded"]) / min(ms["folded"]), 4),
           mean_rel_diff=float(f"{((a - b).abs().mean() / b.abs().mean()).item():.3e}"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--what", default="rows,gemm,block")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=200, help="queued calls per timing (block: a tenth)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rmsnorm_bench.py measures on the GPU: none found")
    for what in a.what.split(","):
        {"rows": bench_rows, "gemm": bench_gemm, "block": bench_block}[what](a.repeats, a.iters)


if __name__ == "__main__":
    main()

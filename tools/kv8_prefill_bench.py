#!/usr/bin/env python3
"""Kernel times of the attention forward over an fp8 (e4m3fn) paged KV cache (ops.flash_attention_varlen_paged with
k_scale / v_scale) against the same launch over a bf16 cache and against the workaround it replaces: dequantise and gather
each sequence's pages into contiguous bf16 K / V, then ops.flash_attention_varlen.  HIP events with warm-up as in
tools/kbench.py; random data, pages randomly permuted, a 2-layer cache read at layer 1, block_size 64; fp8 and bf16 runs
alternate on the same device (min of two rounds each).
  chunked prefill, 16 x (4096 cached + 512 new), causal: H 16 / Hkv 16 / D 64 and H 32 / Hkv 8 / D 128;
  full prefill, 8 x 4096, causal, H 16, D 64 and D 128;
  windowed chunked prefill, 16 x (4096 + 512), window (1024, 0), H 16, D 64.
Prints one line per case: fp8 paged, bf16 paged, dequantise-gather + varlen (ms), fp8 / bf16 and the speed-up over the
workaround.  For per-kernel times run it under rocprofv3 --kernel-trace --stats."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ml-inference-optimizer_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mio import ops  # noqa: E402
from kbench import timeit  # noqa: E402

DEV, DT, L, LAYER, BS = "cuda", torch.bfloat16, 2, 1, 64
F8 = torch.float8_e4m3fn


def cu_of(lens):
    return torch.tensor([0] + torch.cumsum(torch.tensor(lens), 0).tolist(), dtype=torch.int32, device=DEV)


def caches(lens, Hkv, D, g):
    """bf16 caches, their fp8 quantisation (per-layer scales) and a table of permuted pages."""
    npg = [(n + BS - 1) // BS for n in lens]
    nb = sum(npg)
    perm = torch.randperm(nb, generator=g)
    bt = torch.zeros(len(lens), max(npg), dtype=torch.int32)
    o = 0
    for b, n in enumerate(npg):
        bt[b, :n] = perm[o:o + n].to(torch.int32)
        o += n
    kc = torch.randn(nb, L, BS, Hkv, D, device=DEV, dtype=DT)
    vc = torch.randn(nb, L, BS, Hkv, D, device=DEV, dtype=DT)
    ks = torch.full((L,), 4.0 / 448, device=DEV)
    vs = torch.full((L,), 4.0 / 448, device=DEV)
    k8 = (kc.float() / ks.view(1, L, 1, 1, 1)).clamp(-448, 448).to(F8)
    v8 = (vc.float() / vs.view(1, L, 1, 1, 1)).clamp(-448, 448).to(F8)
    return kc, vc, k8, v8, ks, vs, bt.to(DEV)


def deq_gather(k8, v8, ks, vs, bt, lens):
    ks_, vs_ = [], []
    for b, n in enumerate(lens):
        pg = bt[b, :(n + BS - 1) // BS].long()
        ks_.append(k8[pg, LAYER].reshape(-1, k8.shape[-2], k8.shape[-1])[:n])
        vs_.append(v8[pg, LAYER].reshape(-1, v8.shape[-2], v8.shape[-1])[:n])
    k = (torch.cat(ks_).float() * ks[LAYER]).to(DT)
    v = (torch.cat(vs_).float() * vs[LAYER]).to(DT)
    return k, v


def case(name, lens_q, lens_k, H, Hkv, D, window, iters, g):
    kc, vc, k8, v8, ks, vs, bt = caches(lens_k, Hkv, D, g)
    cuq, cuk = cu_of(lens_q), cu_of(lens_k)
    mq, mk = max(lens_q), max(lens_k)
    used = torch.tensor(lens_k, dtype=torch.int32, device=DEV)
    q = torch.randn(sum(lens_q), H, D, device=DEV, dtype=DT)
    out = torch.empty_like(q)
    kw = dict(layer_idx=LAYER, causal=True, window_size=window, out=out)
    route = ops.fa3_paged_route(q, k8, v8, bt, cuq, used, mq, mk, layer_idx=LAYER, causal=True, window_size=window,
                                k_scale=ks, v_scale=vs)

    def fp8():
        ops.flash_attention_varlen_paged(q, k8, v8, bt, cuq, used, mq, mk, k_scale=ks, v_scale=vs, **kw)

    def bf16():
        ops.flash_attention_varlen_paged(q, kc, vc, bt, cuq, used, mq, mk, **kw)

    def workaround():
        k, v = deq_gather(k8, v8, ks, vs, bt, lens_k)
        ops.flash_attention_varlen(q, k, v, cuq, cuk, mq, mk, causal=True, window_size=window, out=out)

    t8, t16, tw = [], [], []
    for _ in range(2):  # interleaved
        t8.append(timeit(fp8, iters))
        t16.append(timeit(bf16, iters))
        tw.append(timeit(workaround, iters))
    a, b, c = min(t8), min(t16), min(tw)
    print(f"  {name} ({route}): fp8 paged {a * 1e3:.3f} ms, bf16 paged {b * 1e3:.3f} ms, dequantise-gather + varlen "
          f"{c * 1e3:.3f} ms; fp8 / bf16 {a / b:.3f}, workaround / fp8 {c / a:.2f}x", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    g = torch.Generator().manual_seed(a.seed)
    ctx, chunk = 4096, 512
    print("chunked prefill, 16 x (4096 cached + 512 new), causal", flush=True)
    case("H16 D64", [chunk] * 16, [ctx + chunk] * 16, 16, 16, 64, (-1, -1), a.iters, g)
    case("H32/8 D128", [chunk] * 16, [ctx + chunk] * 16, 32, 8, 128, (-1, -1), a.iters, g)
    print("full prefill, 8 x 4096, causal", flush=True)
    case("H16 D64", [4096] * 8, [4096] * 8, 16, 16, 64, (-1, -1), a.iters, g)
    case("H16 D128", [4096] * 8, [4096] * 8, 16, 16, 128, (-1, -1), a.iters, g)
    print("windowed chunked prefill, 16 x (4096 + 512), window (1024, 0)", flush=True)
    case("H16 D64 w1024", [chunk] * 16, [ctx + chunk] * 16, 16, 16, 64, (1024, 0), a.iters, g)


if __name__ == "__main__":
    main()

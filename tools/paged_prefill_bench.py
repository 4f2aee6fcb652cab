#!/usr/bin/env python3
"""Kernel times of the attention forward over the paged KV cache (ops.flash_attention_varlen_paged) and of the many-token
cache write (ops.reshape_and_cache_varlen); HIP events with warm-up as in tools/kbench.py, random bf16 data, H 16, Hkv 16,
pages randomly permuted, a 2-layer cache read at layer 1.
  (a) full prefill, uniform 8 x 4096, causal, D 64 / 128, block_size 64 / 256: the paged kernel against
      ops.flash_attention_varlen on contiguous K / V (the cost of the page lookups);
  (b) chunked prefill, 16 sequences of 4096 cached tokens plus a 512-token chunk, causal: the paged kernel against
      gathering each sequence's pages into contiguous K / V and running ops.flash_attention_varlen;
  (c) reshape_and_cache_varlen bandwidth (bytes read + written per second) for 16 x 512 new tokens.
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

DEV, DT, H, HKV, L, LAYER = "cuda", torch.bfloat16, 16, 16, 2, 1


def cu_of(lens):
    return torch.tensor([0] + torch.cumsum(torch.tensor(lens), 0).tolist(), dtype=torch.int32, device=DEV)


def paged(lens, bs, D, g):
    """(k_cache, v_cache, block_tables) holding len(lens) sequences of lens[b] keys on permuted pages."""
    npg = [(n + bs - 1) // bs for n in lens]
    nb = sum(npg)
    perm = torch.randperm(nb, generator=g)
    bt = torch.zeros(len(lens), max(npg), dtype=torch.int32)
    o = 0
    for b, n in enumerate(npg):
        bt[b, :n] = perm[o:o + n].to(torch.int32)
        o += n
    kc = torch.randn(nb, L, bs, HKV, D, device=DEV, dtype=DT)
    vc = torch.randn(nb, L, bs, HKV, D, device=DEV, dtype=DT)
    return kc, vc, bt.to(DEV)


def gather(kc, vc, bt, lens):
    bs = kc.shape[2]
    ks, vs = [], []
    for b, n in enumerate(lens):
        pg = bt[b, :(n + bs - 1) // bs].long()
        ks.append(kc[pg, LAYER].reshape(-1, HKV, kc.shape[-1])[:n])
        vs.append(vc[pg, LAYER].reshape(-1, HKV, vc.shape[-1])[:n])
    return torch.cat(ks), torch.cat(vs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    g = torch.Generator().manual_seed(a.seed)

    print("(a) full prefill, uniform 8 x 4096, causal", flush=True)
    B, S = 8, 4096
    lens = [S] * B
    cu = cu_of(lens)
    for D in (64, 128):
        for bs in (64, 256):
            kc, vc, bt = paged(lens, bs, D, g)
            k, v = gather(kc, vc, bt, lens)
            q = torch.randn(B * S, H, D, device=DEV, dtype=DT)
            used = torch.tensor(lens, dtype=torch.int32, device=DEV)
            out = torch.empty_like(q)
            route = ops.fa3_paged_route(q, kc, vc, bt, cu, used, S, S, layer_idx=LAYER, causal=True)
            tc, tp = [], []
            for _ in range(2):  # interleaved: contiguous, paged, contiguous, paged
                tc.append(timeit(lambda: ops.flash_attention_varlen(q, k, v, cu, cu, S, S, causal=True, out=out), a.iters))
                tp.append(timeit(lambda: ops.flash_attention_varlen_paged(q, kc, vc, bt, cu, used, S, S, layer_idx=LAYER,
                                                                          causal=True, out=out), a.iters))
            print(f"  D{D} bs{bs} ({route}): contiguous varlen {min(tc) * 1e3:.3f} ms, paged {min(tp) * 1e3:.3f} ms, "
                  f"paged / contiguous {min(tp) / min(tc):.3f}", flush=True)
            del kc, vc, k, v, q, out

    print("(b) chunked prefill, 16 x (4096 cached + 512 new), causal", flush=True)
    B, ctx, chunk = 16, 4096, 512
    lens = [ctx + chunk] * B
    cuq = cu_of([chunk] * B)
    for D in (64, 128):
        for bs in (64, 256):
            kc, vc, bt = paged(lens, bs, D, g)
            q = torch.randn(B * chunk, H, D, device=DEV, dtype=DT)
            used = torch.tensor(lens, dtype=torch.int32, device=DEV)
            cuk = cu_of(lens)
            out = torch.empty_like(q)
            route = ops.fa3_paged_route(q, kc, vc, bt, cuq, used, chunk, ctx + chunk, layer_idx=LAYER, causal=True)

            def via_gather():
                k, v = gather(kc, vc, bt, lens)
                ops.flash_attention_varlen(q, k, v, cuq, cuk, chunk, ctx + chunk, causal=True, out=out)

            tg, tp = [], []
            for _ in range(2):
                tg.append(timeit(via_gather, a.iters))
                tp.append(timeit(lambda: ops.flash_attention_varlen_paged(q, kc, vc, bt, cuq, used, chunk, ctx + chunk,
                                                                          layer_idx=LAYER, causal=True, out=out),
                                 a.iters))
            print(f"  D{D} bs{bs} ({route}): gather + varlen {min(tg) * 1e3:.3f} ms, paged {min(tp) * 1e3:.3f} ms, "
                  f"speed-up {min(tg) / min(tp):.2f}x", flush=True)
            del kc, vc, q, out

    print("(c) reshape_and_cache_varlen, 16 x 512 new tokens after 4096 cached", flush=True)
    for D in (64, 128):
        for bs in (64, 256):
            kc, vc, bt = paged(lens, bs, D, g)
            T = B * chunk
            kn = torch.randn(T, HKV, D, device=DEV, dtype=DT)
            vn = torch.randn(T, HKV, D, device=DEV, dtype=DT)
            cl = torch.tensor(lens, dtype=torch.int32, device=DEV)
            t = timeit(lambda: ops.reshape_and_cache_varlen(kn, vn, kc, vc, bt, cuq, cl, bs, LAYER), a.iters)
            nbytes = 4 * kn.numel() * kn.element_size()  # K and V, read once and written once
            print(f"  D{D} bs{bs}: {t * 1e6:.1f} us, {nbytes / t / 1e9:.0f} GB/s", flush=True)
            del kc, vc, kn, vn


if __name__ == "__main__":
    main()

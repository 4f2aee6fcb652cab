#!/usr/bin/env python3
"""Kernel times of paged decode over a bf16 and an fp8 (e4m3fn) KV cache on the same shapes, HIP events with warm-up as in
tools/kbench.py.  The launches are queued through the C entry points with arguments prepared once (the checks of
ops.paged_attention_forward done outside the timed loop), so small cache-resident cases time the kernels, not Python.
Bytes counted are the K and V rows a launch must read (the window's keys only, for a window); TB/s = those bytes / time.
Cases (q_len 1):
  a      H 16 / Hkv 16 / D 64,  B 64, ctx 4096,  block 16   route rows
  b      H 32 / Hkv 4  / D 128, B 64, ctx 4096,  block 16   route gqa
  c      H 32 / Hkv 8  / D 128, B 8,  ctx 32768, block 64   route gqa
  d      H 16 / Hkv 16 / D 64,  B 8,  ctx 4096,  block 16   route head (cache resident in the Infinity Cache)
  b_win  case b at ctx 32768 with window_size (4095, -1)     route gqa
Cache writes: the one-token write (B 64, Hkv 8, D 128) and the varlen write (32768 tokens, Hkv 8, D 128), bf16 and fp8;
GB/s counts the 16-bit K/V read and the cache bytes written.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ml-inference-optimizer_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mio import _lib, ops  # noqa: E402
from kbench import timeit  # noqa: E402

F8 = torch.float8_e4m3fn
CASES = {  # name: (H, Hkv, D, B, ctx, block_size, window_left)
    "a": (16, 16, 64, 64, 4096, 16, -1),
    "b": (32, 4, 128, 64, 4096, 16, -1),
    "c": (32, 8, 128, 8, 32768, 64, -1),
    "d": (16, 16, 64, 8, 4096, 16, -1),
    "b_win": (32, 4, 128, 64, 32768, 16, 4095),
}


def _decode_fn(q, o, kc, vc, bt, cl, bs, ctx, left, ks=None, vs=None):
    """(route, a no-argument launcher) for one decode over these tensors."""
    kw = {} if ks is None else dict(k_scale=ks, v_scale=vs)
    route = ops.paged_attention_route(q, o, kc, vc, bt, cl, bs, ctx, 0, window_size=(left, -1), **kw)
    args, dt, kv8, keep = ops._decode_args(q, o, kc, vc, bt, cl, bs, ctx, 0, None, ks, vs)
    B, H, ql, D = q.shape
    work = torch.empty(_lib.lib.mio_fa3_decode_workspace_bytes(B, H, ql, D, ctx), dtype=torch.uint8, device=q.device)
    st = torch.cuda.current_stream().cuda_stream
    lib = _lib.lib
    if kv8:
        fn = lambda: lib.mio_fa3_decode_paged_kv8(*args, left, dt, work.data_ptr(), st)  # noqa: E731
    elif left < 0:
        fn = lambda: lib.mio_fa3_decode_paged(*args, dt, work.data_ptr(), st)  # noqa: E731
    else:
        fn = lambda: lib.mio_fa3_decode_paged_window(*args, left, -1, dt, work.data_ptr(), st)  # noqa: E731
    assert fn() == 0, lib.mio_last_error()
    fn.keep = (keep, work)
    return route, fn


def decode_case(name, iters):
    H, Hkv, D, B, ctx, bs, left = CASES[name]
    dev = "cuda"
    maxb = (ctx + bs - 1) // bs
    nb = B * maxb
    g = torch.Generator(device=dev).manual_seed(1)
    bt = torch.randperm(nb, device=dev, generator=g).view(B, maxb).to(torch.int32)
    cl = torch.full((B,), ctx, dtype=torch.int32, device=dev)
    q = torch.randn(B, H, 1, D, device=dev, dtype=torch.bfloat16, generator=g)
    o = torch.empty_like(q)
    keys = min(ctx, left + 1) if left >= 0 else ctx
    res = dict(shape=dict(B=B, H=H, Hkv=Hkv, D=D, ctx=ctx, block_size=bs, window_left=left))
    for kind in ("bf16", "fp8"):
        kc = torch.randn(nb, 1, bs, Hkv, D, device=dev, dtype=torch.bfloat16, generator=g)
        vc = torch.randn(nb, 1, bs, Hkv, D, device=dev, dtype=torch.bfloat16, generator=g)
        ks = vs = None
        if kind == "fp8":
            kc, vc = kc.to(F8), vc.to(F8)
            ks = torch.ones(1, dtype=torch.float32, device=dev)
            vs = torch.ones(1, dtype=torch.float32, device=dev)
        route, fn = _decode_fn(q, o, kc, vc, bt, cl, bs, ctx, left, ks, vs)
        t = timeit(fn, iters)
        nbytes = 2 * B * keys * Hkv * D * kc.element_size()
        res[kind] = dict(route=route, us=round(t * 1e6, 2), tb_s=round(nbytes / t / 1e12, 3))
        del kc, vc, fn
        torch.cuda.empty_cache()
    res["fp8_over_bf16_time"] = round(res["fp8"]["us"] / res["bf16"]["us"], 3)
    print(f"{name}: bf16 {res['bf16']['route']} {res['bf16']['us']} us {res['bf16']['tb_s']} TB/s | fp8 "
          f"{res['fp8']['route']} {res['fp8']['us']} us {res['fp8']['tb_s']} TB/s | ratio {res['fp8_over_bf16_time']}",
          file=sys.stderr, flush=True)
    return res


def write_rates(iters):
    """GB/s of the one-token and the varlen cache writes, bf16 and fp8 caches (Hkv 8, D 128, block 16)."""
    dev, Hkv, D, bs = "cuda", 8, 128, 16
    out = {}
    st = torch.cuda.current_stream().cuda_stream
    lib = _lib.lib
    one = torch.ones(1, dtype=torch.float32, device=dev)
    for form, B, T in (("one_token", 64, 64), ("varlen", 64, 32768)):
        per = T // B
        maxb = (per + 4096 + bs - 1) // bs
        nb = B * maxb
        bt = torch.randperm(nb, device=dev).view(B, maxb).to(torch.int32)
        cl = torch.full((B,), 4096 + per, dtype=torch.int32, device=dev)
        cu = torch.arange(0, T + 1, per, dtype=torch.int32, device=dev)
        k = torch.randn(T, Hkv, D, device=dev, dtype=torch.bfloat16)
        v = torch.randn(T, Hkv, D, device=dev, dtype=torch.bfloat16)
        for kind in ("bf16", "fp8"):
            cdt = torch.bfloat16 if kind == "bf16" else F8
            kc = torch.zeros(nb, 1, bs, Hkv, D, device=dev, dtype=cdt)
            vc = torch.zeros(nb, 1, bs, Hkv, D, device=dev, dtype=cdt)
            if form == "one_token":
                ks_ = (C.c_int64 * 2)(Hkv * D, D)
                p = (k.data_ptr(), v.data_ptr(), kc.data_ptr(), vc.data_ptr())
                if kind == "fp8":
                    fn = lambda: lib.mio_reshape_and_cache_kv8(*p, one.data_ptr(), one.data_ptr(), bt.data_ptr(),  # noqa
                                                               cl.data_ptr(), ks_, ks_, B, Hkv, D, 1, 0, bs, maxb, 0, st)
                else:
                    fn = lambda: lib.mio_reshape_and_cache(*p, bt.data_ptr(), cl.data_ptr(), ks_, ks_, B, Hkv, D, 1, 0,  # noqa
                                                           bs, maxb, 0, st)
            else:
                ks_ = (C.c_int64 * 2)(Hkv * D, D)
                p = (k.data_ptr(), v.data_ptr(), kc.data_ptr(), vc.data_ptr())
                if kind == "fp8":
                    fn = lambda: lib.mio_reshape_and_cache_varlen_kv8(  # noqa: E731
                        *p, one.data_ptr(), one.data_ptr(), bt.data_ptr(), cu.data_ptr(), cl.data_ptr(), ks_, ks_, B,
                        T, Hkv, D, nb, 1, 0, bs, maxb, 0, st)
                else:
                    fn = lambda: lib.mio_reshape_and_cache_varlen(  # noqa: E731
                        *p, bt.data_ptr(), cu.data_ptr(), cl.data_ptr(), ks_, ks_, B, T, Hkv, D, nb, 1, 0, bs, maxb, 0,
                        st)
            assert fn() == 0, lib.mio_last_error()
            t = timeit(fn, iters)
            toks = B if form == "one_token" else T
            nbytes = toks * 2 * Hkv * D * (2 + kc.element_size())  # K and V: 16-bit read + cache bytes written
            out[f"{form}_{kind}"] = dict(tokens=toks, us=round(t * 1e6, 2), gb_s=round(nbytes / t / 1e9, 1))
            print(f"write {form} {kind}: {t * 1e6:.2f} us, {nbytes / t / 1e9:.1f} GB/s", file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--cases", default=",".join(CASES))
    a = ap.parse_args()
    res = {"decode": {}, "device": torch.cuda.get_device_name()}
    for name in a.cases.split(","):
        res["decode"][name] = decode_case(name, a.iters)
    res["write"] = write_rates(a.iters)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Timings of the FP8 x FP8 GEMM for tall inputs (ops.gemm_f8) against the route the same call takes on the 16-bit weight
(ops.gemm_bias_act as mio._nn.linear calls it: the blocked weight where ops.blocked_weight_ok says so), in one process, by device
events, the legs alternated after a warm-up and the comparison repeated (--repeats, default 3; the spread of a leg over its repeats
is what a difference has to exceed).  Three forms:

    gemm      ops.gemm_f8 alone on quantised operands           | against the 16-bit GEMM
    q+gemm    ops.quantize_rows_f8 + ops.gemm_f8 (ops.gemm_w8a8) | against the same 16-bit GEMM: what mio_gemm_f8_ok is derived from
    mlp       a whole FusedMLP with gemm_fp8 (the advice forced on) and without

    GEMMs: M 32768 x (N, K) in {(3072, 1024), (1024, 1024), (4096, 1024), (1024, 4096)} (QKV, out-proj, fc1 with gelu, fc2 with the
    residual); SwiGLU fc1 (4096, 1024) at M 32768 and (14336, 4096) at M 8192, the 16-bit leg on the row-major gate / up weights.
    MLPs:  gelu and SwiGLU d 1024 / I 4096 at M 32768; SwiGLU d 4096 / I 14336 at M 8192.

Prints one JSON line per case: microseconds per call (best repeat, and all), TFLOP/s from 2 M N K (SwiGLU: 4 M N K), the route
names, the ratio new / old, the share of the nominal fp8 peak with the bound named (the larger of FLOPs / 5.0 PFLOP/s -- twice the
2.5 PFLOP/s bf16 figure of DESIGN.md section 4 -- and bytes / 8 TB/s, over the measured time), and what ops.gemm_f8_ok says;
--table adds the rows of profiles/gemm_f8.md.  --format-error prints the format's own error instead (normwise difference of
gemm_w8a8 from the fp64 product of the 16-bit inputs, N(0, 1) activations, N(0, K^-1/2) weights, K 1024 and 4096).

    python tools/gemm_f8_bench.py [--repeats 3] [--calls 20] [--dtype bf16] [--skip-mlp] [--table] [--format-error]
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

DEV = "cuda"
PEAK_F8, PEAK_HBM = 5.0e15, 8.0e12
GEMMS = [(32768, 3072, 1024, "none", False), (32768, 1024, 1024, "none", True), (32768, 4096, 1024, "gelu", False),
         (32768, 1024, 4096, "none", True), (32768, 4096, 1024, "swiglu", False), (8192, 14336, 4096, "swiglu", False)]
MLPS = [("FusedMLPGeluTanh", 32768, 1024, 4096), ("FusedMLPSwiGLU", 32768, 1024, 4096), ("FusedMLPSwiGLU", 8192, 4096, 14336)]


def timed(fn, calls):
    """Microseconds per call of fn over `calls` calls between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def compare(legs, repeats, calls):
    """legs: name -> callable.  Warm every leg up, then alternate them `repeats` times; name -> list of microseconds."""
    for fn in legs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in legs}
    for _ in range(repeats):
        for k, fn in legs.items():
            us[k].append(timed(fn, calls))
    return us


def bench_gemm(M, N, K, act, res, dt, repeats, calls):
    g = torch.Generator(device=DEV).manual_seed(N + K)
    rnd = lambda *shape, scale=1.0: (torch.randn(*shape, device=DEV, generator=g) * scale).to(dt)  # noqa: E731
    glu = act == "swiglu"
    x, w, b = rnd(M, K), rnd(N, K, scale=K ** -0.5), rnd(N, scale=0.5)
    wg = rnd(N, K, scale=K ** -0.5) if glu else None
    r = rnd(M, N) if res else None
    wb = ops.block_weight(w) if (not glu and K % 32 == 0 and ops.blocked_weight_ok(M, N, K, act)) else None
    (w8, ws), (g8, gs) = ops.quantize_weight_w8(w), (ops.quantize_weight_w8(wg) if glu else (None, None))
    x8, xs = ops.quantize_rows_f8(x)
    y16, y8 = torch.empty(M, N, dtype=dt, device=DEV), torch.empty(M, N, dtype=dt, device=DEV)
    kw16 = dict(w_gate=wg, residual=r, out=y16, w_blocked=wb)
    legs = {"old": lambda: ops.gemm_bias_act(x, w, b, act, **kw16),
            "gemm": lambda: ops.gemm_f8(x8, xs, w8, ws, b, act, g8, gs, None, r, y8, dt),
            "q+gemm": lambda: ops.gemm_w8a8(x, w8, ws, b, act, g8, gs, None, r, y8)}
    us = compare(legs, repeats, calls)
    best = {k: min(v) for k, v in us.items()}
    diff = ((y8.float() - y16.float()).norm() / y16.float().norm()).item()
    flops = 2.0 * M * N * K * (2 if glu else 1)
    nbytes = M * K + N * K * (2 if glu else 1) + 2 * M * N * (2 if res else 1)
    t_flop, t_byte = flops / PEAK_F8, nbytes / PEAK_HBM
    rec = {"form": "gemm", "M": M, "N": N, "K": K, "act": act, "residual": res, "dtype": str(dt).split(".")[-1],
           "route_old": ops.gemm_route(x, w, b, act, **{k: v for k, v in kw16.items() if v is not None}),
           "route_f8": ops.gemm_f8_route(M, N, K, act),
           "old_us": round(best["old"], 1), "gemm_us": round(best["gemm"], 1), "qgemm_us": round(best["q+gemm"], 1),
           "old_TFLOPs": round(flops / best["old"] / 1e6, 1), "gemm_TFLOPs": round(flops / best["gemm"] / 1e6, 1),
           "qgemm_TFLOPs": round(flops / best["q+gemm"] / 1e6, 1),
           "ratio_gemm": round(best["gemm"] / best["old"], 3), "ratio_qgemm": round(best["q+gemm"] / best["old"], 3),
           "gemm_share_of_peak": round(max(t_flop, t_byte) * 1e6 / best["gemm"], 3), "bound": "fp8 MFMA" if t_flop >= t_byte else "HBM",
           "spread": {k: round(max(v) / min(v) - 1.0, 3) for k, v in us.items()},
           "us_all": {k: [round(t, 1) for t in v] for k, v in us.items()},
           "admit_at_0.9": best["q+gemm"] <= 0.9 * best["old"], "ok": ops.gemm_f8_ok(M, N, K, act),
           "normwise_diff_vs_16bit": float(f"{diff:.2e}")}
    print(json.dumps(rec), flush=True)
    return rec


def bench_mlp(kind, M, d, I, dt, repeats, calls):
    from mio.kernels import mlp
    torch.manual_seed(d + I)
    mods = {k: getattr(mlp, kind)(d, I, mlp.FusedMLPConfig(precision="bf16" if dt == torch.bfloat16 else "fp16", gemm_fp8=k == "fp8"))
            .to(DEV, dt) for k in ("old", "fp8")}
    mods["fp8"].load_state_dict(mods["old"].state_dict())
    x = torch.randn(1, M, d, device=DEV, dtype=dt)
    advised = ops.gemm_f8_ok
    forced = lambda *a: True  # noqa: E731  (the route is measured whatever the advice table says)

    def fp8():
        ops.gemm_f8_ok = forced
        try:
            return mods["fp8"](x, residual=x)
        finally:
            ops.gemm_f8_ok = advised

    with torch.no_grad():
        us = compare({"old": lambda: mods["old"](x, residual=x), "fp8": fp8}, repeats, calls)
        ya, yb = fp8().float(), mods["old"](x, residual=x).float()
    best = {k: min(v) for k, v in us.items()}
    flops = 2.0 * M * d * I * (3 if kind == "FusedMLPSwiGLU" else 2)
    rec = {"form": "mlp", "module": kind, "M": M, "d": d, "I": I, "dtype": str(dt).split(".")[-1], "old_us": round(best["old"], 1),
           "fp8_us": round(best["fp8"], 1), "old_TFLOPs": round(flops / best["old"] / 1e6, 1), "fp8_TFLOPs": round(flops / best["fp8"] / 1e6, 1),
           "ratio": round(best["fp8"] / best["old"], 3), "spread": {k: round(max(v) / min(v) - 1.0, 3) for k, v in us.items()},
           "us_all": {k: [round(t, 1) for t in v] for k, v in us.items()},
           "normwise_diff_vs_16bit": float(f"{((ya - yb).norm() / yb.norm()).item():.2e}")}
    print(json.dumps(rec), flush=True)
    return rec


def format_error(dt):
    """The format's own error, not the kernel's: gemm_w8a8 against the fp64 product of the 16-bit inputs."""
    for K in (1024, 4096):
        g = torch.Generator(device=DEV).manual_seed(K)
        x = torch.randn(1024, K, device=DEV, generator=g).to(dt)
        w = (torch.randn(1024, K, device=DEV, generator=g) * K ** -0.5).to(dt)
        ref = x.double() @ w.double().t()
        y8, y16 = ops.gemm_w8a8(x, *ops.quantize_weight_w8(w)).double(), ops.gemm_bias_act(x, w).double()
        print(json.dumps({"form": "format_error", "K": K, "dtype": str(dt).split(".")[-1],
                          "w8a8_normwise": float(f"{((y8 - ref).norm() / ref.norm()).item():.3e}"),
                          "16bit_normwise": float(f"{((y16 - ref).norm() / ref.norm()).item():.3e}")}), flush=True)


def table(recs):
    """The rows of profiles/gemm_f8.md."""
    print("| M x N x K | act | old route | old us (TFLOP/s) | gemm_f8 us (TFLOP/s) | quantiser + gemm_f8 us | gemm / old | q+gemm / old | "
          "share of fp8 peak (bound) | spread old / gemm / q+gemm |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for r in (r for r in recs if r["form"] == "gemm"):
        sp = r["spread"]
        print(f"| {r['M']} x {r['N']} x {r['K']} | {r['act']}{' + residual' if r['residual'] else ''} | {r['route_old']} | {r['old_us']} "
              f"({r['old_TFLOPs']}) | {r['gemm_us']} ({r['gemm_TFLOPs']}) | {r['qgemm_us']} | {r['ratio_gemm']} | {r['ratio_qgemm']} | "
              f"{r['gemm_share_of_peak']} ({r['bound']}) | {sp['old'] * 100:.1f} % / {sp['gemm'] * 100:.1f} % / {sp['q+gemm'] * 100:.1f} % |")
    print("\n| module | M, d, I | 16-bit us (TFLOP/s) | gemm_fp8 us (TFLOP/s) | fp8 / 16-bit | normwise difference |")
    print("|---|---|---|---|---|---|")
    for r in (r for r in recs if r["form"] == "mlp"):
        print(f"| {r['module']} | {r['M']}, {r['d']}, {r['I']} | {r['old_us']} ({r['old_TFLOPs']}) | {r['fp8_us']} ({r['fp8_TFLOPs']}) | "
              f"{r['ratio']} | {r['normwise_diff_vs_16bit']} |")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--skip-mlp", action="store_true")
    ap.add_argument("--table", action="store_true", help="print the markdown rows of the profile after the JSON lines")
    ap.add_argument("--format-error", action="store_true", help="print the format's own error rows and nothing else")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gemm_f8_bench.py measures on the GPU: none found")
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float16
    if a.format_error:
        return format_error(dt)
    recs = [bench_gemm(*c, dt, max(3, a.repeats), a.calls) for c in GEMMS]
    if not a.skip_mlp:
        recs += [bench_mlp(*c, dt, max(3, a.repeats), a.calls) for c in MLPS]
    if a.table:
        table(recs)


if __name__ == "__main__":
    main()

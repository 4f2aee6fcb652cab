"""Per-rank compute used by the parallel wrappers: the HIP kernels.

The distributed schedules (tensor-parallel sharding + all-reduce, ring / mesh K-V exchange + (o, lse)
carry) are backend-agnostic; what runs on each rank between two communication steps goes through the
functions below.  In the product they are the HIP kernels and nothing else.  The CPU (gloo)
schedule tests replace linear, attention_step and layernorm (the three launches) with checker implementations to exercise the
communication logic without a GPU (tests/test_parallel_gloo.py, tests/_cpu_local.py).

Nothing here remembers anything, and the one question asked here is ops.blocked_weight_ok (cached_linear): whether K leaves its
projection pre-scaled is _nn.attention_plan's answer, asked by the attention modules, and the blocked, concatenated and cast
parameter copies live in the _nn.CastCache of the module that owns the parameters and die with it."""
from __future__ import annotations

import torch

from .. import ops


def linear(x, weight, bias=None, activation="none", residual=None, out=None, col_scale=None, w_blocked=None):
    """One launch of F.linear (+ activation, + residual) on the MFMA GEMM; w_blocked: the weight in the blocked layout, given
    where the size runs the 256x256-tile kernels.  col_scale = (lo, hi, value): see ops.gemm_bias_act."""
    return ops.gemm_bias_act(x, weight, bias, activation, residual=residual, out=out, w_blocked=w_blocked, col_scale=col_scale)


def cached_linear(cache, x, weight, bias=None, activation="none", residual=None, out=None, col_scale=None, parts=None):
    """linear() with, at sizes that run the 256x256-tile kernels, the blocked weight from the calling module's CastCache (repacked
    once per parameter version).  parts: the parameters `weight` is the row-concatenation of (CastCache.get_cat), where it is
    not a parameter itself.  col_scale: the col_scale of _nn.attention_plan."""
    N, K = weight.shape
    M = x.numel() // K
    kw = {}
    if K % 32 == 0 and ops.blocked_weight_ok(M, N, K, activation):
        dt = weight.dtype
        kw["w_blocked"] = cache.get_blocked(weight, dt) if parts is None else cache.get_cat(parts, dt, blocked=True)
    return linear(x, weight, bias, activation, residual, out, col_scale, **kw)


def attention_step(q, k, v, **kw):
    """One kernel launch of tiled attention with optional (o_acc, lse) carry; see ops.fa3_fwd."""
    return ops.fa3_fwd(q, k, v, **kw)


def layernorm(x, weight, bias=None, eps=1e-5):
    """Row LayerNorm; weight and bias in x's dtype."""
    return ops.layernorm(x, weight, bias, eps)


def prenorm(x, pre_norm, cache):
    """pre_norm(x) for the tensor- and sequence-parallel sub-layers, which keep LayerNorm only (the pre-LN block's `module(ln(x))`
    when a converted block is called with pre_norm=); its parameters in x's dtype come from the calling module's CastCache."""
    if not isinstance(pre_norm, torch.nn.LayerNorm):
        raise TypeError(f"the tensor- and sequence-parallel sub-layers take an nn.LayerNorm as pre_norm only (an RMSNorm runs in "
                        f"front of them, or in the single-device modules), got {type(pre_norm).__name__}")
    w, b = pre_norm.weight, pre_norm.bias
    if w.dtype != x.dtype:
        w, b = cache.get(w, x.dtype), cache.get(b, x.dtype)
    return layernorm(x, w, b, pre_norm.eps)

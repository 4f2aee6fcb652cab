"""Functional entry points of the hot path: thin argument checking + one C-ABI call each.

These mirror the reference's functional launch wrappers (same positional/keyword signatures,
same exception types for the same conditions):
  flash_attention           <- triton_flash_attention        (kernels/triton/flash_attention_kernels.py:1150-1358)
  flash_attention_varlen       packed variable-length attention (cu_seqlens; not in the reference), with unpad_input /
                               pad_input for padded batches under a [B, S] keep-mask
  ring_attention_forward    <- triton_ring_attention_forward (kernels/triton/attention_kernels.py:909-1005)
  fused_mlp                 <- triton_fused_mlp              (kernels/triton/mlp_kernels.py:648-756)
  layernorm                 <- triton_layernorm              (kernels/triton/layernorm_kernels.py:191-276)
  rmsnorm / rms_fold_weight    RMSNorm rows (not a reference kernel: LLaMA-class blocks), and the weight of a projection behind one
                               for gemm_ln(..., norm="rms")
  paged_attention_forward   <- triton_paged_attention_forward(kernels/triton/attention_kernels.py:1206-1311)
  reshape_and_cache         <- triton_reshape_and_cache      (kernels/triton/attention_kernels.py:1314-1407)
  rope_tables / apply_rotary / rope_and_cache_varlen
                               rotary position embedding (not a reference kernel: its LLaMA path rotates K in PyTorch before
                               caching it, baseline/model_utils.py): the fp32 angle tables, the standalone rotation of the dense
                               path, and the rotation fused into the varlen paged-cache write (16-bit and fp8 caches)
  sample_tokens / sampling_probs
                               token sampling (not a reference kernel: its facade promises .generate()): [B, V] logits to token
                               ids in one launch -- greedy, temperature, top-k, top-p, min-p per row from device tensors
  moe_route / moe_up / moe_down / moe_mlp
                               mixture-of-experts MLP of a decode step (not a reference kernel: its models are dense): the router
                               (top-k of a softmax over all experts, routed rows grouped by expert, all on the device) and the
                               grouped up / down GEMMs over stacked expert weights with the combine
There is no fallback path: a non-zero return from the library raises RuntimeError.
"""
from __future__ import annotations

import os

import ctypes as C
import math
import operator
import types
from typing import NamedTuple, Optional, Tuple

import torch

from . import _lib
from ._lib import lib, check

_ACT = {
    "none": _lib.ACT_NONE,
    "gelu": _lib.ACT_GELU_TANH,       # the Triton kernel's GELU is the tanh form (mlp_kernels.py:144-161)
    "gelu_tanh": _lib.ACT_GELU_TANH,
    "gelu_new": _lib.ACT_GELU_TANH,
    "gelu_erf": _lib.ACT_GELU_ERF,
    "relu": _lib.ACT_RELU,
    "silu": _lib.ACT_SILU,
    "swish": _lib.ACT_SILU,
    "swiglu": _lib.ACT_SWIGLU,
}


def _dtype_id(t: torch.Tensor) -> int:
    if t.dtype == torch.bfloat16:
        return _lib.MIO_BF16
    if t.dtype == torch.float16:
        return _lib.MIO_FP16
    raise ValueError(f"HIP kernels compute in bf16 or fp16, got {t.dtype}")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _need_cuda(*ts: Optional[torch.Tensor]) -> None:
    for t in ts:
        if t is not None and not t.is_cuda:
            raise ValueError("HIP kernels require input tensors to be on a CUDA (ROCm) device.")


def _vec_ok(t: Optional[torch.Tensor], n: int, dtype: torch.dtype, what: str) -> None:
    """A per-column operand (bias, LayerNorm weight): 1-D, contiguous, n elements, the activations' dtype and device.
    The kernels read n elements of the activation dtype from the raw pointer, so anything else would be misread."""
    if t is None:
        return
    if not t.is_cuda:
        raise ValueError("HIP kernels require input tensors to be on a CUDA (ROCm) device.")
    if t.dim() != 1 or t.numel() != n or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous 1-D tensor of {n} elements, got shape {tuple(t.shape)}")
    if t.dtype != dtype:
        raise ValueError(f"{what} must have the activation dtype {dtype}, got {t.dtype}")


def _res_ok(r: Optional[torch.Tensor], numel: int, dtype: torch.dtype) -> None:
    if r is None:
        return
    if not r.is_cuda:
        raise ValueError("HIP kernels require input tensors to be on a CUDA (ROCm) device.")
    if r.dtype != dtype:
        raise ValueError(f"residual must have the activation dtype {dtype}, got {r.dtype}")
    if r.numel() != numel:
        raise ValueError(f"residual has {r.numel()} elements, the output has {numel}")


def _rows16(t: torch.Tensor) -> torch.Tensor:
    """Make the last dim contiguous and every other stride a multiple of 8 elements."""
    if t.stride(-1) != 1 or any(s % 8 for s in t.stride()[:-1]) or t.data_ptr() % 16:
        return t.contiguous()
    return t


# ------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------
def _qkv_dtype(q, k, v, names="q, k, v") -> int:
    """The dtype id of q, which k and v must share."""
    if k.dtype != q.dtype or v.dtype != q.dtype:
        raise ValueError(f"{names} must have the same dtype")
    return _dtype_id(q)


def _check_heads(H: int, Hkv: int, D: int) -> None:
    if H % Hkv != 0:
        raise ValueError(f"num_heads {H} must be a multiple of num_kv_heads {Hkv}")
    if D % 8 != 0 or D > 128:
        raise ValueError(f"head_dim must be a multiple of 8 and <= 128, got {D}")


def _softmax_scale(D: int, softmax_scale: Optional[float]) -> float:
    scale = (1.0 / math.sqrt(D)) if softmax_scale is None else float(softmax_scale)
    if not (scale > 0.0):
        raise ValueError("softmax_scale must be positive")
    return scale


def _out_like(q: torch.Tensor, out: Optional[torch.Tensor]) -> torch.Tensor:
    if out is None:
        return torch.empty_like(q, memory_format=torch.contiguous_format)
    if out.shape != q.shape or out.dtype != q.dtype or out.stride(-1) != 1:
        raise ValueError("out must match q in shape/dtype with a contiguous last dim")
    return out


def _packed_lse(q: torch.Tensor, return_lse: bool) -> Optional[torch.Tensor]:
    """The packed forms' lse, fp32 [H, total_q] for q [total_q, H, D], when return_lse."""
    return torch.empty(q.shape[1], q.shape[0], dtype=torch.float32, device=q.device) if return_lse else None


def _fill_null(p, fields, addr: int) -> None:
    """torch gives empty tensors a null address; nothing is read or written through them (include/mio_hip.h): use addr."""
    for f in fields:
        if not getattr(p, f):
            setattr(p, f, addr)


def _route(query, p, window, names, *scales) -> str:
    """The route name of a *_route_window query (window (-1, -1): exactly the query without one); scales: the fp8 form's."""
    r = query(C.byref(p), *scales, window[0], window[1])
    if r < 0:
        raise RuntimeError(lib.mio_last_error().decode("utf-8", "replace"))
    return names[r]


def _launch(fwd, p, window, out, lse, return_lse: bool, *scales):
    """A *_window launch (as _route), queued on the current stream; RuntimeError on failure."""
    check(fwd(C.byref(p), *scales, window[0], window[1], _stream()))
    return (out, lse) if return_lse else out


_WINDOW_MAX = (1 << 31) - 1  # the C ABI's int32: larger values would arrive truncated


def _window(window_size, causal: bool = False):
    """window_size = (left, right) checked (flash-attn's convention): two ints, each -1 (unbounded) or in
    [0, 2^31 - 1]; causal allows right -1 or 0 (causal is right = 0).  Returns (left, right); ValueError otherwise."""
    try:
        left, right = (operator.index(w) for w in window_size)
    except (TypeError, ValueError):
        raise ValueError(f"window_size must be a pair of ints (left, right), got {window_size!r}") from None
    if not (-1 <= left <= _WINDOW_MAX and -1 <= right <= _WINDOW_MAX):
        raise ValueError(f"window_size values must be -1 (unbounded) or in [0, 2^31 - 1], got {tuple(window_size)}")
    if causal and right > 0:
        raise ValueError(f"causal attention has window_size[1] = 0: give -1 or 0, got {right}")
    return left, right


def _dense_window(window_size, causal=False, keep_mask=None, additive_mask=None, o_acc=None, carry_in=False,
                  k_prescaled=False, out_blocked=False, **_):
    """The window of a dense launch, with the combinations the windowed kernels do not take refused."""
    w = _window(window_size, causal)
    if w != (-1, -1):
        if keep_mask is not None or additive_mask is not None:
            raise ValueError("window_size cannot be combined with a mask")
        if o_acc is not None or carry_in:
            raise ValueError("window_size cannot be combined with the ring carry (o_acc / carry_in)")
        if k_prescaled or out_blocked:
            raise ValueError("window_size cannot be combined with k_prescaled / out_blocked")
    return w


def fa3_fwd(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    *,
    layout: str = "bshd",
    causal: bool = False,
    softmax_scale: Optional[float] = None,
    keep_mask: Optional[torch.Tensor] = None,
    additive_mask: Optional[torch.Tensor] = None,
    return_lse: bool = False,
    out: Optional[torch.Tensor] = None,
    o_acc: Optional[torch.Tensor] = None,
    lse: Optional[torch.Tensor] = None,
    carry_in: bool = False,
    write_out: bool = True,
    q_offset: int = 0,
    k_offset: int = 0,
    k_prescaled: bool = False,
    out_blocked: bool = False,
    window_size=(-1, -1),
):
    """One launch of the tiled attention kernel.

    layout "bshd": q [B,Sq,H,D], k/v [B,Sk,Hkv,D] (flash); "bhsd": head-major (ring, a9).
    keep_mask / additive_mask: 4-D, broadcastable to [B,H,Sq,Sk] (size-1 dims broadcast).
    Ring carry: o_acc fp32 [B,Sq,H,D] + lse fp32 [B,H,Sq]; carry_in continues from that state.
    k_prescaled: k already holds K * softmax_scale * log2(e), scaled in fp32 before its rounding to 16 bits
    (gemm_bias_act(col_scale=...)); only where fa3_k_prescaled_ok() says so -- ValueError otherwise.
    out_blocked (k_prescaled launches, layout "bshd", where fa3_o_blocked_ok() says so): the output is returned as a
    [ceil(B*Sq/256)*256, H*D] tensor in the blocked activation layout (include/mio_hip.h) for a following
    gemm_bias_act(..., x_blocked_shape=(B, Sq, H*D)) -- the output projection then fetches contiguous K-tiles.
    window_size = (left, right): sliding window (flash-attn's convention, -1 = unbounded): query i sees key j iff
    i + q_offset - k_offset - left <= j <= i + q_offset - k_offset + right; not with masks, the ring carry, k_prescaled
    or out_blocked (ValueError).  (-1, -1) is the launch without a window.
    Returns out (same layout as q) or (out, lse) if return_lse.
    """
    w = _dense_window(window_size, causal, keep_mask=keep_mask, additive_mask=additive_mask, o_acc=o_acc,
                      carry_in=carry_in, k_prescaled=k_prescaled, out_blocked=out_blocked)
    _need_cuda(q, k, v)
    p, out, lse, _keep = _fa3_params(q, k, v, layout=layout, causal=causal, softmax_scale=softmax_scale,
                                     keep_mask=keep_mask, additive_mask=additive_mask, return_lse=return_lse, out=out,
                                     o_acc=o_acc, lse=lse, carry_in=carry_in, write_out=write_out, q_offset=q_offset,
                                     k_offset=k_offset, k_prescaled=k_prescaled, out_blocked=out_blocked)
    return _launch(lib.mio_fa3_fwd_window, p, w, out, lse, return_lse)


def fa3_route(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, **kwargs) -> str:
    """The kernel fa3_fwd(q, k, v, **kwargs) would launch (mio_fa3_route; a name of _lib.FA3_ROUTES), without launching.
    Takes fa3_fwd's arguments; tensors may live on any device (only their shapes, strides and addresses are read).
    Arguments fa3_fwd refuses raise the same ValueError / RuntimeError."""
    window_size = kwargs.pop("window_size", (-1, -1))
    w = _dense_window(window_size, **kwargs)
    p, _out, _lse, _keep = _fa3_params(q, k, v, **kwargs)
    return _route(lib.mio_fa3_route_window, p, w, _lib.FA3_ROUTES)


def _fa3_params(q, k, v, *, layout="bshd", causal=False, softmax_scale=None, keep_mask=None, additive_mask=None,
                return_lse=False, out=None, o_acc=None, lse=None, carry_in=False, write_out=True, q_offset=0, k_offset=0,
                k_prescaled=False, out_blocked=False):
    """fa3_fwd's argument checks and mio_fa3_fwd_params_t; returns (params, out, lse, keep): out / lse are allocated here
    when not given, and keep holds every other tensor the params point into (q / k / v / mask as converted here), which
    must stay alive until the launch is queued."""
    if q.dim() != 4 or k.dim() != 4 or v.dim() != 4:
        raise ValueError(f"Expected 4D tensors for q, k, v but got shapes: q={q.shape}, k={k.shape}, v={v.shape}")
    if layout not in ("bshd", "bhsd"):
        raise ValueError(f"unknown layout {layout}")
    dt = _qkv_dtype(q, k, v)
    q, k, v = _rows16(q), _rows16(k), _rows16(v)
    si, hi = (1, 2) if layout == "bshd" else (2, 1)
    B, Sq, H, D = q.shape[0], q.shape[si], q.shape[hi], q.shape[3]
    Sk, Hkv = k.shape[si], k.shape[hi]
    if k.shape[0] != B or v.shape != k.shape or k.shape[3] != D:
        raise ValueError(f"incompatible q/k/v shapes: q={q.shape}, k={k.shape}, v={v.shape}")
    _check_heads(H, Hkv, D)
    scale = _softmax_scale(D, softmax_scale)
    if keep_mask is not None and additive_mask is not None:
        raise ValueError("give either keep_mask or additive_mask, not both")

    p = _lib.FaParams()
    if out_blocked:
        if layout != "bshd" or not write_out or out is not None or not k_prescaled:
            raise ValueError("out_blocked needs layout 'bshd', k_prescaled, write_out and no out= tensor")
        out = torch.empty((B * Sq + 255) // 256 * 256, H * D, dtype=q.dtype, device=q.device)
    elif write_out:
        out = _out_like(q, out)
    else:
        out = None
        if o_acc is None:
            raise ValueError("write_out=False needs o_acc")
    if o_acc is not None:
        if o_acc.dtype != torch.float32 or tuple(o_acc.shape) != (B, Sq, H, D) or not o_acc.is_contiguous():
            raise ValueError("o_acc must be contiguous fp32 [B,Sq,H,D]")
        if lse is None:
            raise ValueError("o_acc needs an lse buffer")
    if (return_lse or o_acc is not None) and lse is None:
        lse = torch.empty(B, H, Sq, dtype=torch.float32, device=q.device)
    if lse is not None and (lse.dtype != torch.float32 or tuple(lse.shape) != (B, H, Sq) or not lse.is_contiguous()):
        raise ValueError("lse must be contiguous fp32 [B,H,Sq]")
    if carry_in and o_acc is None:
        raise ValueError("carry_in needs o_acc and lse")

    mask, kind = None, _lib.MASK_NONE
    if keep_mask is not None:
        mask, kind = keep_mask, _lib.MASK_KEEP_U8
        if mask.dtype != torch.uint8:
            mask = (mask != 0).to(torch.uint8)
    elif additive_mask is not None:
        mask, kind = additive_mask.to(torch.float32), _lib.MASK_ADD_F32
    if mask is not None:
        if q.is_cuda:
            _need_cuda(mask)
        if mask.dim() != 4:
            raise ValueError(f"Unsupported mask shape: {tuple(mask.shape)}")
        for dim, full in zip(mask.shape, (B, H, Sq, Sk)):
            if dim not in (1, full):
                raise ValueError(f"mask shape {tuple(mask.shape)} does not broadcast to {(B, H, Sq, Sk)}")
        for i in range(4):
            p.mask_stride[i] = 0 if mask.shape[i] == 1 else mask.stride(i)

    def _st(dst, t):
        dst[0], dst[1], dst[2] = t.stride(0), t.stride(si), t.stride(hi)

    _st(p.q_stride, q)
    _st(p.k_stride, k)
    _st(p.v_stride, v)
    if out is not None and not out_blocked:
        _st(p.o_stride, out)
    p.q, p.k, p.v = q.data_ptr(), k.data_ptr(), v.data_ptr()
    p.o, p.lse, p.o_acc, p.mask = _ptr(out), _ptr(lse), _ptr(o_acc), _ptr(mask)
    if Sk == 0:  # torch gives empty tensors a null address; no key (or mask entry) is read then (include/mio_hip.h)
        p.k = p.v = p.q
        if mask is not None:
            p.mask = p.q
    p.B, p.Sq, p.Sk, p.H, p.Hkv, p.D = B, Sq, Sk, H, Hkv, D
    p.dtype, p.causal, p.mask_kind, p.carry_in = dt, int(bool(causal)), kind, int(bool(carry_in))
    p.q_offset, p.k_offset, p.softmax_scale = int(q_offset), int(k_offset), scale
    if k_prescaled:
        if not lib.mio_fa3_k_prescaled_ok(C.byref(p)):
            raise ValueError("k_prescaled is only supported for head_dim <= 96 (<= 64 with the (o_acc, lse) carry), no mask, "
                             "Sq > 128")
        p.k_prescaled = 1
    if out_blocked:
        if not lib.mio_fa3_o_blocked_ok(C.byref(p)):
            raise ValueError("out_blocked is only supported for k_prescaled launches without carry, head_dim <= 64, "
                             "(H * D) % 32 == 0")
        p.o_blocked = 1
    return p, out, lse, (q, k, v, mask)


def fa3_k_prescaled_ok(B: int, Sq: int, Sk: int, H: int, D: int, k_row_stride: int, v_row_stride: int,
                       carry: bool = False) -> bool:
    """True iff fa3_fwd(..., k_prescaled=True) is available for a launch of this geometry without a mask (carry: with the
    (o_acc, lse) ring carry)."""
    return (D <= (64 if carry else 96) and Sq > 128 and Sk > 0 and Sk * k_row_stride * 2 < (1 << 32)
            and Sk * v_row_stride * 2 < (1 << 32))


def fa3_o_blocked_ok(B: int, Sq: int, Sk: int, H: int, D: int, k_row_stride: int, v_row_stride: int) -> bool:
    """True iff fa3_fwd(..., k_prescaled=True, out_blocked=True) is available for this geometry."""
    return (not NO_BLOCKED_X and fa3_k_prescaled_ok(B, Sq, Sk, H, D, k_row_stride, v_row_stride) and D <= 64
            and (H * D) % 32 == 0)


def _canon_mask4(mask: torch.Tensor) -> torch.Tensor:
    """[B,S] / [B,1,S] / [B,S,S] / 4-D -> 4-D, as flash_attention_kernels.py:1232-1250."""
    if mask.dim() == 2:
        return mask[:, None, None, :]
    if mask.dim() == 3:
        return mask[:, :, None, :] if mask.shape[1] == 1 else mask[:, None, :, :]
    if mask.dim() == 4:
        return mask
    raise ValueError(f"Unsupported mask shape: {mask.shape}")


def flash_attention(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    mask: Optional[torch.Tensor] = None,
    causal: bool = False,
    softmax_scale: Optional[float] = None,
    dropout_p: float = 0.0,
    return_softmax: bool = False,
    block_size: int = 128,
    *,
    window_size=(-1, -1),
):
    """Drop-in for triton_flash_attention (flash_attention_kernels.py:1150-1358), q/k/v [B,S,H,D].

    mask: keep-mask (nonzero = attend; masked scores := -1e9, :257-273) of shape [B,S], [B,1,S],
    [B,S,S] or 4-D.  block_size is accepted for signature compatibility; the HIP kernel's tile
    (128 queries x 64 keys) is fixed.  return_softmax / dropout_p > 0 are not computed by the
    fused kernel: NotImplementedError (the reference's autograd path punts the same way, :1044-1046).
    window_size = (left, right): sliding window as in fa3_fwd (not together with mask).
    """
    if q.dim() != 4 or k.dim() != 4 or v.dim() != 4:
        raise ValueError(f"Expected 4D tensors for q, k, v but got shapes: q={q.shape}, k={k.shape}, v={v.shape}")
    if return_softmax:
        raise NotImplementedError("return_softmax=True is not supported by the fused HIP kernel")
    if dropout_p and dropout_p > 0.0:
        raise NotImplementedError("attention dropout (training) is not supported by the inference kernel")
    keep = None
    if mask is not None:
        keep = _canon_mask4(mask.to(q.device))
    if tuple(window_size) == (-1, -1):
        return fa3_fwd(q, k, v, layout="bshd", causal=causal, softmax_scale=softmax_scale, keep_mask=keep)
    return fa3_fwd(q, k, v, layout="bshd", causal=causal, softmax_scale=softmax_scale, keep_mask=keep,
                   window_size=window_size)


def _varlen_params(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, causal=False, softmax_scale=None,
                   return_lse=False, out=None):
    """flash_attention_varlen's argument checks and mio_fa3_varlen_params_t; returns (params, out, lse, keep) as
    _fa3_params does.  Reads no device memory."""
    if q.dim() != 3 or k.dim() != 3 or v.dim() != 3:
        raise ValueError(f"Expected 3D tensors [tokens, heads, head_dim] for q, k, v but got shapes: q={q.shape}, "
                         f"k={k.shape}, v={v.shape}")
    dt = _qkv_dtype(q, k, v)
    for name, cu in (("cu_seqlens_q", cu_seqlens_q), ("cu_seqlens_k", cu_seqlens_k)):
        if cu.dtype != torch.int32 or cu.dim() != 1 or cu.numel() < 1 or not cu.is_contiguous():
            raise ValueError(f"{name} must be a contiguous 1-D int32 tensor of B+1 offsets")
        if cu.device != q.device:
            raise ValueError(f"{name} must be on the device of q")
    if cu_seqlens_k.numel() != cu_seqlens_q.numel():
        raise ValueError("cu_seqlens_q and cu_seqlens_k must have the same length (B+1)")
    q, k, v = _rows16(q), _rows16(k), _rows16(v)
    Tq, H, D = q.shape
    Tk, Hkv = k.shape[0], k.shape[1]
    if v.shape != k.shape or k.shape[2] != D:
        raise ValueError(f"incompatible q/k/v shapes: q={q.shape}, k={k.shape}, v={v.shape}")
    _check_heads(H, Hkv, D)
    scale = _softmax_scale(D, softmax_scale)
    out = _out_like(q, out)
    lse = _packed_lse(q, return_lse)

    p = _lib.FaVarlenParams()
    for dst, t in ((p.q_stride, q), (p.k_stride, k), (p.v_stride, v), (p.o_stride, out)):
        dst[0], dst[1] = t.stride(0), t.stride(1)
    p.q, p.k, p.v, p.o, p.lse = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), _ptr(lse)
    _fill_null(p, ("q", "k", "v", "o"), cu_seqlens_q.data_ptr())
    p.cu_seqlens_q, p.cu_seqlens_k = cu_seqlens_q.data_ptr(), cu_seqlens_k.data_ptr()
    p.B, p.total_q, p.total_k = cu_seqlens_q.numel() - 1, Tq, Tk
    p.max_seqlen_q, p.max_seqlen_k = int(max_seqlen_q), int(max_seqlen_k)
    p.H, p.Hkv, p.D = H, Hkv, D
    p.dtype, p.causal, p.softmax_scale = dt, int(bool(causal)), scale
    return p, out, lse, (q, k, v, cu_seqlens_q, cu_seqlens_k)


def flash_attention_varlen(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    cu_seqlens_q: torch.Tensor,
    cu_seqlens_k: torch.Tensor,
    max_seqlen_q: int,
    max_seqlen_k: int,
    causal: bool = False,
    softmax_scale: Optional[float] = None,
    return_lse: bool = False,
    out: Optional[torch.Tensor] = None,
    *,
    window_size=(-1, -1),
):
    """Packed variable-length attention forward (the form of flash-attn's flash_attn_varlen_func), mio_fa3_fwd_varlen.

    q [total_q, H, D], k / v [total_k, Hkv, D] (bf16 / fp16; k / v may be strided views into a fused QKV buffer);
    cu_seqlens_q / cu_seqlens_k: int32 [B+1] offsets on q's device -- sequence b is rows cu_seqlens_q[b] .. [b+1]-1 of q
    and cu_seqlens_k[b] .. [b+1]-1 of k / v.  max_seqlen_q / max_seqlen_k bound every sequence's length (longer ones are
    cut there).  causal is bottom-right aligned per sequence: query i sees key j iff j <= i + Lk - Lq.  Rows with no
    visible key get 0 (lse -inf).  Returns out [total_q, H, D] or (out, lse fp32 [H, total_q]) if return_lse.
    Queued on the current stream with no host sync (graph-capturable): the offsets are never read on the host.
    window_size = (left, right): sliding window, bottom-right per sequence: query i also needs
    i + Lk - Lq - left <= j <= i + Lk - Lq + right (-1 = unbounded; causal is right = 0).
    """
    w = _window(window_size, causal)
    _need_cuda(q, k, v, cu_seqlens_q, cu_seqlens_k)
    p, out, lse, _keep = _varlen_params(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, causal=causal,
                                        softmax_scale=softmax_scale, return_lse=return_lse, out=out)
    return _launch(lib.mio_fa3_fwd_varlen_window, p, w, out, lse, return_lse)


def fa3_varlen_route(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cu_seqlens_q: torch.Tensor,
                     cu_seqlens_k: torch.Tensor, max_seqlen_q: int, max_seqlen_k: int, **kwargs) -> str:
    """The kernel flash_attention_varlen(...) would launch (mio_fa3_varlen_route): "empty", "fwd5" or "fwd3", without
    launching.  Tensors may live on any device; arguments flash_attention_varlen refuses raise the same errors."""
    w = _window(kwargs.pop("window_size", (-1, -1)), kwargs.get("causal", False))
    p, _out, _lse, _keep = _varlen_params(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, **kwargs)
    return _route(lib.mio_fa3_varlen_route_window, p, w, _lib.FA3_VARLEN_ROUTES)


def unpad_input(x: torch.Tensor, keep: torch.Tensor):
    """x [B, S, ...] and a keep-mask [B, S] (nonzero = a real token, any left / right padding) -> (x_packed [total, ...],
    indices [total] int64 into the flattened [B*S], cu_seqlens int32 [B+1], max_seqlen int).  Syncs with the host (the
    packed size and max_seqlen are read back)."""
    if keep.dim() != 2 or x.shape[:2] != keep.shape:
        raise ValueError(f"keep must be [B, S] matching x's first two dims, got x={tuple(x.shape)}, keep={tuple(keep.shape)}")
    keep = keep.to(x.device) != 0
    lens = keep.sum(dim=1, dtype=torch.int32)
    indices = torch.nonzero(keep.flatten(), as_tuple=False).flatten()
    cu = torch.zeros(keep.shape[0] + 1, dtype=torch.int32, device=x.device)
    cu[1:] = torch.cumsum(lens, dim=0, dtype=torch.int32)
    max_seqlen = int(lens.max().item()) if lens.numel() else 0
    return x.reshape(-1, *x.shape[2:])[indices], indices, cu, max_seqlen


def pad_input(x_packed: torch.Tensor, indices: torch.Tensor, B: int, S: int) -> torch.Tensor:
    """Inverse of unpad_input: [total, ...] -> [B, S, ...] with zeros at the padding positions."""
    out = torch.zeros(B * S, *x_packed.shape[1:], dtype=x_packed.dtype, device=x_packed.device)
    out[indices] = x_packed
    return out.view(B, S, *x_packed.shape[1:])


def ring_attention_forward(
    query: torch.Tensor, key: torch.Tensor, value: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
    k_prescaled: bool = False,
) -> torch.Tensor:
    """Drop-in for triton_ring_attention_forward (attention_kernels.py:909-1005; fallback :1520-1591):
    q/k/v [B,H,S,D] head-major, additive mask [B,1|H,Sq,Sk]; returns [B,Sq,H*D].
    k_prescaled (not in the reference): see fa3_fwd."""
    if query.dim() != 4:
        raise ValueError(f"Expected 4D tensors, got {query.shape}")
    B, H, Sq, D = query.shape
    out = torch.empty(B, Sq, H, D, dtype=query.dtype, device=query.device)
    # write straight into the [B,Sq,H*D] result: give the kernel a head-major VIEW of it
    fa3_fwd(query, key, value, layout="bhsd", additive_mask=attention_mask, out=out.permute(0, 2, 1, 3),
            k_prescaled=k_prescaled)
    return out.view(B, Sq, H * D)


def attn_merge(o_a, lse_a, o_b, lse_b, out: Optional[torch.Tensor] = None):
    """(o_a, lse_a) <- merge((o_a, lse_a), (o_b, lse_b)); fp32 states [B,Sq,H,D] / [B,H,Sq]."""
    _need_cuda(o_a, lse_a, o_b, lse_b)
    B, Sq, H, D = o_a.shape
    for t in (o_a, o_b, lse_a, lse_b):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("merge states must be contiguous fp32")
    dt = _lib.MIO_BF16 if out is None else _dtype_id(out)
    if out is not None and (tuple(out.shape) != (B, Sq, H, D) or not out.is_contiguous()):
        raise ValueError("out must be contiguous [B,Sq,H,D]")
    check(lib.mio_attn_merge(o_a.data_ptr(), lse_a.data_ptr(), o_b.data_ptr(), lse_b.data_ptr(), _ptr(out),
                             B, Sq, H, D, dt, _stream()))
    return o_a, lse_a


# ------------------------------------------------------------------------------------------------
# GEMM / FusedMLP / LayerNorm
# ------------------------------------------------------------------------------------------------
_NO_BLOCKED_W = os.environ.get("MIO_NO_BLOCKED_W", "0") == "1"
NO_BLOCKED_X = os.environ.get("MIO_NO_BLOCKED_X", "0") == "1"  # A/B runs: LayerNorm keeps writing the plain layout


def block_weight(w: torch.Tensor) -> torch.Tensor:
    """One-time repack of a Linear weight [N, K] (K % 32 == 0) into the blocked layout of include/mio_hip.h
    (contiguous 16 KiB K-tiles): returns a [ceil(N/256)*256, K] tensor holding the blocked bytes."""
    _need_cuda(w)
    if w.dim() != 2 or w.shape[1] % 32 != 0:
        raise ValueError(f"block_weight needs a 2-D weight with K % 32 == 0, got {tuple(w.shape)}")
    w = _rows16(w)
    N, K = w.shape
    wb = torch.empty((N + 255) // 256 * 256, K, dtype=w.dtype, device=w.device)
    assert wb.numel() * wb.element_size() == lib.mio_weight_blocked_bytes(N, K)
    check(lib.mio_weight_block(w.data_ptr(), w.stride(0), wb.data_ptr(), N, K, _dtype_id(w), _stream()))
    return wb


def block_weight_glu(w_gate: torch.Tensor, w_up: torch.Tensor) -> torch.Tensor:
    """One-time repack of the SwiGLU gate / up weights [I, K] (K % 32 == 0) into ONE blocked weight whose 256-row tiles
    interleave 32 gate rows and the 32 up rows of the same output columns per wave slice (include/mio_hip.h):
    returns a [ceil(I/128)*256, K] tensor.  fused_mlp(..., activation="swiglu", fc1_blocked=<this>)."""
    _need_cuda(w_gate, w_up)
    if w_gate.dim() != 2 or w_gate.shape != w_up.shape or w_gate.shape[1] % 32 != 0 or w_gate.dtype != w_up.dtype:
        raise ValueError(f"block_weight_glu needs two 2-D weights of one shape and dtype with K % 32 == 0, got "
                         f"{tuple(w_gate.shape)} / {tuple(w_up.shape)}")
    w_gate, w_up = _rows16(w_gate), _rows16(w_up)
    if w_gate.stride(0) != w_up.stride(0):
        w_gate, w_up = w_gate.contiguous(), w_up.contiguous()
    I, K = w_gate.shape
    wb = torch.empty((I + 127) // 128 * 256, K, dtype=w_gate.dtype, device=w_gate.device)
    assert wb.numel() * wb.element_size() == lib.mio_weight_blocked_glu_bytes(I, K)
    check(lib.mio_weight_block_glu(w_gate.data_ptr(), w_up.data_ptr(), w_gate.stride(0), wb.data_ptr(), I, K,
                                   _dtype_id(w_gate), _stream()))
    return wb


def blocked_weight_ok(M: int, N: int, K: int, activation: str = "none") -> bool:
    """True iff a GEMM of this shape runs a kernel that takes blocked weights (w_blocked= below).
    MIO_NO_BLOCKED_W=1 (A/B runs) keeps the modules on the plain weights."""
    return not _NO_BLOCKED_W and bool(lib.mio_gemm_blocked_weight_ok(M, N, K, _ACT.get(activation, _lib.ACT_NONE)))


def fused_mlp_blocked_weight_ok(M: int, d: int, I: int, activation: str) -> bool:
    """True iff ops.fused_mlp at this shape takes blocked fc1 / fc2 weights (fc1_blocked= / fc2_blocked=)."""
    return not _NO_BLOCKED_W and bool(lib.mio_fused_mlp_blocked_weight_ok(M, d, I, _ACT.get(activation, _lib.ACT_NONE)))


def col_scale_ok(M: int, N: int, K: int, activation: str = "none") -> bool:
    """True iff gemm_bias_act(..., col_scale=) is available for this shape (the persistent 256x256-tile kernel runs it)."""
    return not _NO_BLOCKED_W and bool(lib.mio_gemm_col_scale_ok(M, N, K, _ACT.get(activation, _lib.ACT_NONE)))


def _gemm_route(M, N, K, ldx, ldw, ldy, ldr, act, residual: bool, w_layout, fold_in=False, stats_out=False) -> str:
    r = lib.mio_gemm_route(M, N, K, ldx, ldw, ldy, ldr, act, int(residual), w_layout, int(fold_in), int(stats_out))
    if r < 0:
        raise ValueError(lib.mio_last_error().decode("utf-8", "replace"))
    return _lib.GEMM_ROUTES[r]


def _gemm_args(x, w, act, residual=None, out=None, w_blocked=None, x_blocked_shape=None, col_scale=None, **_):
    """A gemm_bias_act call as the launch and gemm_route both read it: (entry, M, N, K, lead, x2, ldx, w2, ldw, ldy, r2, ldr).
    entry names the C entry point: "cs" (mio_gemm_bias_act_bw_cs), "bw" (mio_gemm_bias_act_bw) or "plain" (mio_gemm_bias_act);
    lead is the output's leading shape, x2 / w2 / r2 the operands as 2-D views whose rows the kernels take (copies only where
    _rows16 must make one).  Host-only: shapes and strides, no data, no allocation, so tensors may live on any device."""
    K, N = x.shape[-1], w.shape[0]
    if x_blocked_shape is not None:
        # x is layernorm(..., out_blocked=True) of a tensor of shape x_blocked_shape: blocked activation layout
        lead, x2, ldx = tuple(x_blocked_shape[:-1]), x, K
    else:
        lead, x2 = tuple(x.shape[:-1]), _rows16(x.reshape(-1, K))
        ldx = x2.stride(0)
    M = int(math.prod(lead))
    if residual is not None and residual.numel() != M * N:
        raise ValueError(f"residual has {residual.numel()} elements, the output has {M * N}")
    r2 = None if residual is None else _rows16(residual.reshape(-1, N))
    ldr = 0 if r2 is None else r2.stride(0)
    ldy = N if out is None else out.view(-1, N).stride(0)
    if col_scale is not None:
        entry = "cs"
    elif x_blocked_shape is not None:
        entry = "bw"
    else:  # a row-major x takes the blocked weight where mio_gemm_bias_act_bw takes the call (mio_gemm_route refuses it otherwise)
        bw = w_blocked is not None and M > 0 and \
            lib.mio_gemm_route(M, N, K, ldx, K, ldy, ldr, act, int(r2 is not None), _lib.W_BLOCKED, 0, 0) >= 0
        entry = "bw" if bw else "plain"
    w2 = _rows16(w) if entry == "plain" else w_blocked  # (a blocked weight counts with its row length K)
    return entry, M, N, K, lead, x2, ldx, w2, w2.stride(0) if entry == "plain" else K, ldy, r2, ldr


def gemm_route(x, w, bias=None, activation: str = "none", **kwargs) -> str:
    """The kernel (a name of mio._lib.GEMM_ROUTES) that gemm_bias_act(x, w, bias, activation, **kwargs) -- or, with the
    keyword-only M / N / K of that signature, gemm_ln(x, w, bias, **kwargs) -- launches.  Host-only (mio_gemm_route): it reads
    shapes, strides and which operands are given, never the data.  ValueError where the call would be refused."""
    if activation not in _ACT:
        raise ValueError(f"Unsupported activation function: {activation}")
    act = _ACT[activation]
    if "M" in kwargs:  # gemm_ln (norm=: both norms run the same routes)
        _norm_ok(kwargs.get("norm", "layernorm"), kwargs.get("ln_stats") is not None)
        M, N, K = int(kwargs["M"]), int(kwargs["N"]), int(kwargs["K"])
        _x2, ldx, r2, ldr = _gemm_ln_args(x, **kwargs)
        return _gemm_route(M, N, K, ldx, K, N, ldr, act, r2 is not None,
                           _lib.W_GLU if act == _lib.ACT_SWIGLU else _lib.W_BLOCKED,
                           kwargs.get("ln_stats") is not None, bool(kwargs.get("stats_out", False)))
    unknown = set(kwargs) - {"w_gate", "bias_gate", "residual", "out", "w_blocked", "x_blocked_shape", "col_scale"}
    if unknown:
        raise TypeError(f"gemm_route: unexpected arguments {sorted(unknown)}")
    entry, M, N, K, _lead, _x2, ldx, _w2, ldw, ldy, r2, ldr = _gemm_args(x, w, act, **kwargs)
    return _gemm_route(M, N, K, ldx, ldw, ldy, ldr, act, r2 is not None, _lib.W_PLAIN if entry == "plain" else _lib.W_BLOCKED)


def gemm_bias_act(x, w, bias=None, activation: str = "none", w_gate=None, bias_gate=None, residual=None, out=None,
                  w_blocked=None, x_blocked_shape=None, col_scale=None):
    """y = act(x @ w^T + bias) (+ residual); x [..., K], w [N, K].  F.linear with a fused epilogue.
    col_scale = (lo, hi, value): output columns [lo, hi) are multiplied by value in fp32 before the rounding to the
    storage dtype (lo, hi multiples of 128; needs w_blocked, no residual, and col_scale_ok())."""
    _need_cuda(x, w)
    if activation not in _ACT:
        raise ValueError(f"Unsupported activation function: {activation}")
    act = _ACT[activation]
    dt = _dtype_id(x)
    if w.dtype != x.dtype:
        raise ValueError("x and w must have the same dtype")
    if w.shape[1] != x.shape[-1]:
        raise ValueError(f"weight shape {tuple(w.shape)} does not match input features {x.shape[-1]}")
    N, K = w.shape
    _vec_ok(bias, N, x.dtype, "bias")
    if act == _lib.ACT_SWIGLU:
        _vec_ok(bias_gate, N, x.dtype, "bias_gate")
    if w_blocked is not None:
        # the blocked copy travels as a raw pointer: a stale repack (other dtype / device / shape) must not get that far
        if w_blocked.dtype != x.dtype or w_blocked.device != x.device:
            raise ValueError("w_blocked must have x's dtype and device (repack after converting the module)")
        if w_blocked.numel() != (N + 255) // 256 * 256 * K or not w_blocked.is_contiguous():
            raise ValueError(f"w_blocked has {w_blocked.numel()} elements, expected ceil(N/256)*256*K = {(N + 255) // 256 * 256 * K}")
    entry, M, N, K, lead, x2, ldx, w2, ldw, _ldy, r2, ldr = _gemm_args(x, w, act, residual, out, w_blocked, x_blocked_shape, col_scale)
    _res_ok(residual, M * N, x.dtype)
    if entry == "cs":
        lo, hi, val = int(col_scale[0]), int(col_scale[1]), float(col_scale[2])
        if w_blocked is None or residual is not None or not lib.mio_gemm_col_scale_ok(M, N, K, act):
            raise ValueError("col_scale needs a blocked weight, no residual and a shape with col_scale_ok()")
        if lo % 128 or hi % 128 or not (0 <= lo <= hi <= N):
            raise ValueError(f"col_scale range [{lo}, {hi}) must be multiples of 128 inside [0, {N}]")
    elif x_blocked_shape is not None:
        if w_blocked is None or act == _lib.ACT_SWIGLU or not lib.mio_gemm_blocked_weight_ok(M, N, K, act):
            raise ValueError("a blocked activation operand needs a blocked weight and a shape with blocked_weight_ok()")
    elif act == _lib.ACT_SWIGLU and w_gate is None:
        raise ValueError("SwiGLU activation requires gate weights")
    if out is None:
        out = torch.empty(*lead, N, dtype=x.dtype, device=x.device)
    y2 = out.view(-1, N)
    xb = int(x_blocked_shape is not None)
    if entry == "cs":
        check(lib.mio_gemm_bias_act_bw_cs(x2.data_ptr(), w2.data_ptr(), _ptr(bias), y2.data_ptr(), M, N, K, ldx, y2.stride(0),
                                          act, dt, xb, lo, hi, val, _stream()))
    elif entry == "bw":
        check(lib.mio_gemm_bias_act_bw(x2.data_ptr(), w2.data_ptr(), _ptr(bias), _ptr(r2), y2.data_ptr(), M, N, K, ldx,
                                       y2.stride(0), ldr, act, dt, xb, _stream()))
    else:
        w_gate, bias_gate = (_rows16(w_gate), bias_gate) if act == _lib.ACT_SWIGLU else (None, None)
        check(lib.mio_gemm_bias_act(x2.data_ptr(), w2.data_ptr(), _ptr(bias), _ptr(w_gate), _ptr(bias_gate), _ptr(r2),
                                    y2.data_ptr(), M, N, K, ldx, ldw, y2.stride(0), ldr, act, dt, _stream()))
    return out


# ---- the decode-step GEMM (1 <= M <= 64 rows, the weight streamed once from its row-major copy): mio_gemm_skinny on 16-bit weights,
# mio_gemm_skinny_w8 on e4m3fn weight bytes with one fp32 scale per output column ------------------------------------------------
_W8 = torch.float8_e4m3fn


def _skinny_ok(name: str, M: int, N: int, K: int, activation: str) -> bool:
    return activation in _ACT and bool(getattr(lib, f"mio_{name}_ok")(M, N, K, _ACT[activation]))


def _skinny_splits(name: str, M: int, N: int, K: int, activation: str) -> int:
    if activation not in _ACT:
        raise ValueError(f"Unsupported activation function: {activation}")
    n = getattr(lib, f"mio_{name}_splits")(M, N, K, _ACT[activation])
    if n < 0:
        raise ValueError(lib.mio_last_error().decode("utf-8", "replace"))
    return n


def _skinny(fn, ws_bytes, tall: str, x, N: int, K: int, ldw: int, w_ptrs, g_ptrs, bias, activation: str, bias_gate, residual, out):
    """What gemm_skinny and gemm_skinny_w8 do around their weight operands, which the caller has checked.  fn / ws_bytes: the
    C launch and its workspace query; ldw: the row stride of the weight [N, K] (and of the gate); w_ptrs / g_ptrs: the addresses
    of the weight and of the gate with what goes with them, as fn takes them between x and bias and between bias and bias_gate."""
    if activation not in _ACT:
        raise ValueError(f"Unsupported activation function: {activation}")
    act = _ACT[activation]
    dt = _dtype_id(x)
    _vec_ok(bias, N, x.dtype, "bias")
    if act == _lib.ACT_SWIGLU:
        _vec_ok(bias_gate, N, x.dtype, "bias_gate")
    else:
        bias_gate = None
    lead, x2 = tuple(x.shape[:-1]), _rows16(x.reshape(-1, K))
    M = x2.shape[0]
    if M > 64:  # (fn is mio_<the op's name>)
        raise ValueError(f"{fn.__name__[4:]} takes at most 64 rows, got {M} ({tall})")
    _res_ok(residual, M * N, x.dtype)
    r2 = None if residual is None else _rows16(residual.reshape(-1, N))
    if out is None:  # (rows of N % 8 != 0 columns: a view of rows padded to the stride the kernel's 8-byte stores need)
        out = torch.empty(*lead, (N + 7) // 8 * 8, dtype=x.dtype, device=x.device)[..., :N]
    y2 = out.view(-1, N)
    nbytes = ws_bytes(M, N, K, act)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device) if nbytes else None
    check(fn(x2.data_ptr(), *w_ptrs, _ptr(bias), *g_ptrs, _ptr(bias_gate), _ptr(r2), y2.data_ptr(), _ptr(ws), M, N, K, x2.stride(0),
             ldw, y2.stride(0), 0 if r2 is None else r2.stride(0), act, dt, _stream()))
    return out


def gemm_skinny_ok(M: int, N: int, K: int, activation: str = "none") -> bool:
    """True iff gemm_skinny is legal at this shape AND the measured better choice over gemm_bias_act (profiles/skinny_gemm.md).
    Advice for the module layer: gemm_skinny itself runs every legal shape."""
    return _skinny_ok("gemm_skinny", M, N, K, activation)


def gemm_skinny_splits(M: int, N: int, K: int, activation: str = "none") -> int:
    """The slices of K a gemm_skinny call of this shape runs (1: one launch, no workspace).  Host-only; ValueError where the
    call would be refused."""
    return _skinny_splits("gemm_skinny", M, N, K, activation)


def gemm_skinny(x, w, bias=None, activation: str = "none", w_gate=None, bias_gate=None, residual=None, out=None):
    """gemm_bias_act for at most 64 rows (x [..., K] with prod(...) <= 64, w [N, K], any N): y = act(x @ w^T + bias) (+ residual)
    on the weight-streaming kernel.  Allocates the split workspace only when the plan splits K."""
    _need_cuda(x, w)
    if w.dtype != x.dtype:
        raise ValueError("x and w must have the same dtype")
    if w.shape[1] != x.shape[-1]:
        raise ValueError(f"weight shape {tuple(w.shape)} does not match input features {x.shape[-1]}")
    w2, g2 = _rows16(w), None
    if activation == "swiglu":
        if w_gate is None:
            raise ValueError("SwiGLU activation requires gate weights")
        if w_gate.shape != w.shape or w_gate.dtype != w.dtype:
            raise ValueError("w_gate must have w's shape and dtype")
        _need_cuda(w_gate)
        g2 = _rows16(w_gate)
        if g2.stride(0) != w2.stride(0):
            g2, w2 = g2.contiguous(), w2.contiguous()
    N, K = w2.shape
    return _skinny(lib.mio_gemm_skinny, lib.mio_gemm_skinny_workspace_bytes, "gemm_bias_act runs taller calls", x, N, K, w2.stride(0),
                   (w2.data_ptr(),), (_ptr(g2),), bias, activation, bias_gate, residual, out)


def gemm_skinny_w8_ok(M: int, N: int, K: int, activation: str = "none") -> bool:
    """True iff gemm_skinny_w8 is legal at this shape AND measured at most 0.9 x the time of the faster of gemm_skinny and
    gemm_bias_act on the 16-bit weight (profiles/skinny_gemm_w8.md).  Advice for the module layer: gemm_skinny_w8 itself runs
    every legal shape."""
    return _skinny_ok("gemm_skinny_w8", M, N, K, activation)


def gemm_skinny_w8_splits(M: int, N: int, K: int, activation: str = "none") -> int:
    """The slices of K a gemm_skinny_w8 call of this shape runs (1: one launch, no workspace).  Host-only; ValueError where the
    call would be refused."""
    return _skinny_splits("gemm_skinny_w8", M, N, K, activation)


def quantize_weight_w8(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """One-time preparation of a bf16 / fp16 weight [N, K] (K % 16 == 0) for gemm_skinny_w8: (w8 [N, K] torch.float8_e4m3fn,
    scale [N] fp32) with scale[n] = max |w[n, :]| / 448 (1.0 for an all-zero row, NaN elements ignored) and
    w8 = e4m3(clamp(w * (1 / scale), -448, 448)), so that w8 * scale[:, None] is w to within the format's rounding."""
    _need_cuda(w)
    dt = _dtype_id(w)
    if w.dim() != 2:
        raise ValueError(f"quantize_weight_w8 takes a 2-D weight [N, K], got shape {tuple(w.shape)}")
    N, K = w.shape
    if K % 16 != 0:
        raise ValueError(f"quantize_weight_w8: K must be a multiple of 16, got {K}")
    w2 = _rows16(w)
    w8 = torch.empty(N, K, dtype=_W8, device=w.device)
    scale = torch.empty(N, dtype=torch.float32, device=w.device)
    check(lib.mio_weight_quant_w8(w2.data_ptr(), w2.stride(0), w8.data_ptr(), K, scale.data_ptr(), N, K, dt, _stream()))
    return w8, scale


def _w8_ok(t: torch.Tensor, what: str) -> torch.Tensor:
    """An fp8 weight operand: 2-D torch.float8_e4m3fn on the device (not e5m2, e4m3fnuz or an integer type); returned with unit
    column stride and rows a multiple of 16 bytes apart at a 16-byte aligned address (a row slice stays a view)."""
    if t.dtype != _W8:
        raise ValueError(f"{what} must be torch.float8_e4m3fn (OCP e4m3), got {t.dtype}")
    _need_cuda(t)
    if t.dim() != 2:
        raise ValueError(f"{what} must be a 2-D weight [N, K], got shape {tuple(t.shape)}")
    if t.stride(1) != 1 or t.stride(0) % 16 or t.data_ptr() % 16:
        return t.contiguous()
    return t


def _w8_scale(s: torch.Tensor, N: int, what: str) -> torch.Tensor:
    """The fp32 scales of an fp8 weight as [N]: one per output column, or a one-element tensor (a per-tensor scale) expanded."""
    if s is None or s.dtype != torch.float32:
        raise ValueError(f"{what} must be an fp32 tensor (the scales of a torch.float8_e4m3fn weight), got "
                         f"{None if s is None else s.dtype}")
    _need_cuda(s)
    if s.numel() == 1 and N != 1:
        return s.reshape(1).expand(N).contiguous()
    if s.dim() != 1 or s.numel() != N:
        raise ValueError(f"{what} must have {N} elements (one per output column) or one, got shape {tuple(s.shape)}")
    return s if s.is_contiguous() and s.data_ptr() % 16 == 0 else s.clone(memory_format=torch.contiguous_format)


def gemm_skinny_w8(x, w8, w_scale, bias=None, activation: str = "none", w8_gate=None, w_scale_gate=None, bias_gate=None,
                   residual=None, out=None):
    """gemm_skinny on a weight-only FP8 weight (x [..., K] bf16 / fp16 with prod(...) <= 64; w8 [N, K] torch.float8_e4m3fn,
    K % 16 == 0; w_scale fp32 [N] or one element): y = act(w_scale * (x @ w8^T) + bias) (+ residual), SwiGLU with w8_gate /
    w_scale_gate / bias_gate.  Row slices of w8 and w_scale are legal operands.  Allocates the split workspace only when the plan
    splits K."""
    _need_cuda(x)
    w2 = _w8_ok(w8, "w8")
    if w2.shape[1] != x.shape[-1]:
        raise ValueError(f"weight shape {tuple(w2.shape)} does not match input features {x.shape[-1]}")
    N, K = w2.shape
    if K % 16 != 0:
        raise ValueError(f"gemm_skinny_w8: K must be a multiple of 16, got {K}")
    s2 = _w8_scale(w_scale, N, "w_scale")
    g2 = sg2 = None
    if activation == "swiglu":
        if w8_gate is None or w_scale_gate is None:
            raise ValueError("SwiGLU activation requires gate weights and their scales")
        g2 = _w8_ok(w8_gate, "w8_gate")
        if g2.shape != w2.shape:
            raise ValueError("w8_gate must have w8's shape")
        sg2 = _w8_scale(w_scale_gate, N, "w_scale_gate")
        if g2.stride(0) != w2.stride(0):
            g2, w2 = g2.contiguous(), w2.contiguous()
    return _skinny(lib.mio_gemm_skinny_w8, lib.mio_gemm_skinny_w8_workspace_bytes, "fp8 weights are read by the decode-step kernel only",
                   x, N, K, w2.stride(0), (w2.data_ptr(), s2.data_ptr()), (_ptr(g2), _ptr(sg2)), bias, activation, bias_gate,
                   residual, out)


# ---- LayerNorm folded into the GEMMs on either side of it (mio_gemm_ln_bw; reference fused_layernorm_qkv.py:37-420) ------------
def gemm_ln_ok(M: int, N: int, K: int, activation: str = "none", fold_in: bool = False, stats_out: bool = False) -> bool:
    """True iff gemm_ln(...) runs this shape: fold_in = the projection behind a LayerNorm (ln_stats given),
    stats_out = the residual GEMM that also writes the row statistics of its output."""
    return not _NO_BLOCKED_W and bool(lib.mio_gemm_ln_ok(M, N, K, _ACT.get(activation, _lib.ACT_NONE), int(fold_in), int(stats_out)))


def ln_fold_weight(w: torch.Tensor, gamma: torch.Tensor, beta: Optional[torch.Tensor], bias: Optional[torch.Tensor],
                   blocked: bool = True):
    """One-time preparation of a projection that sits behind a LayerNorm(gamma, beta): returns
    (blocked weight = gamma-scaled rows with their mean over k subtracted, bias' [N] = bias + w @ beta).  With the rows centred
    x @ w'^T equals (x - mean(x)) @ (gamma * w)^T, so gemm_ln's read-out only multiplies by rstd and adds bias'.
    blocked=False returns the row-major [N, K] weight instead (the SwiGLU pair goes through block_weight_glu afterwards)."""
    _need_cuda(w, gamma)
    dt = _dtype_id(w)
    N, K = w.shape
    _vec_ok(gamma, K, w.dtype, "gamma")
    _vec_ok(beta, K, w.dtype, "beta")
    _vec_ok(bias, N, w.dtype, "bias")
    w = _rows16(w)
    ws = torch.empty(N, K, dtype=w.dtype, device=w.device)
    bout = torch.empty(N, dtype=w.dtype, device=w.device)
    check(lib.mio_ln_fold_weight(w.data_ptr(), w.stride(0), gamma.data_ptr(), _ptr(beta), _ptr(bias), ws.data_ptr(),
                                 bout.data_ptr(), N, K, dt, _stream()))
    return (block_weight(ws) if blocked else ws), bout


def rms_fold_weight(w: torch.Tensor, gamma: torch.Tensor, bias: Optional[torch.Tensor] = None, blocked: bool = True):
    """One-time preparation of a projection that sits behind an RMSNorm(gamma): returns (weight = w * gamma, the product taken in
    fp32 and rounded once; bias unchanged).  There is no mean, so nothing is centred, and no beta, so nothing is folded into the
    bias: gemm_ln(..., norm="rms")'s read-out multiplies by rstd and adds bias.  blocked=True returns block_weight of the [N, K]
    product, blocked=False the row-major weight (the SwiGLU pair goes through block_weight_glu afterwards).  Preparation, not
    hot path: torch ops."""
    _need_cuda(w, gamma)
    _dtype_id(w)
    if w.dim() != 2:
        raise ValueError(f"rms_fold_weight needs a 2-D weight, got {tuple(w.shape)}")
    N, K = w.shape
    _vec_ok(gamma, K, w.dtype, "gamma")
    _vec_ok(bias, N, w.dtype, "bias")
    ws = (w.float() * gamma.float()).to(w.dtype)
    return (block_weight(ws) if blocked else ws), bias


_NORMS = ("layernorm", "rms")


def _norm_ok(norm: str, fold: bool) -> bool:
    """gemm_ln's norm=: True for the RMS form, which is the consumer form only."""
    if norm not in _NORMS:
        raise ValueError(f"norm must be one of {_NORMS}, got {norm!r}")
    if norm == "rms" and not fold:
        raise ValueError("gemm_ln: norm='rms' is the consumer form (give ln_stats)")
    return norm == "rms"


def ln_stats_shape(M: int, width: int):
    return ((width + 255) // 256, (M + 255) // 256 * 256, 2)


def ln_stats_for_launch(ln_stats: torch.Tensor, M: int) -> torch.Tensor:
    """The statistics as gemm_ln's consumer launch reads them: up to 8 slots as they are; more (a stream wider than 2048 columns)
    summed in equal groups of consecutive slots (mio_ln_stats_reduce) down to the largest divisor of the count that the
    kernel's LDS region holds."""
    slots = ln_stats.shape[0]
    if slots <= 8:
        return ln_stats
    out_slots = max(s_ for s_ in range(1, 9) if slots % s_ == 0)
    red = torch.empty((out_slots,) + tuple(ln_stats.shape[1:]), dtype=torch.float32, device=ln_stats.device)
    check(lib.mio_ln_stats_reduce(ln_stats.data_ptr(), slots, red.data_ptr(), out_slots, M, _stream()))
    return red


def _gemm_ln_args(x, M, N, K, x_blocked=False, residual=None, res_blocked=False, **_):
    """gemm_ln's x and residual as mio_gemm_ln_bw and mio_gemm_route take them: (x2, ldx, r2, ldr).  Host-only."""
    M, N, K = int(M), int(N), int(K)

    def _operand(t, cols, blocked, what):
        if t.dtype != x.dtype or t.device != x.device:
            raise ValueError(f"{what} must have x's dtype and device")
        if blocked:
            if t.numel() != (M + 255) // 256 * 256 * cols or not t.is_contiguous():
                raise ValueError(f"{what}: a blocked operand has ceil(M/256)*256 x {cols} contiguous elements")
            return t, cols
        t2 = _rows16(t.reshape(-1, cols))
        if t2.shape[0] != M:
            raise ValueError(f"{what}: expected [{M}, {cols}]")
        return t2, t2.stride(0)

    return _operand(x, K, x_blocked, "x") + ((None, 0) if residual is None else _operand(residual, N, res_blocked, "residual"))


def gemm_ln(x: torch.Tensor, w_blocked: torch.Tensor, bias: Optional[torch.Tensor], *, M: int, N: int, K: int,
            activation: str = "none", x_blocked: bool = False, residual: Optional[torch.Tensor] = None,
            res_blocked: bool = False, out_blocked: bool = False, ln_stats: Optional[torch.Tensor] = None,
            eps: float = 1e-5, stats_out: bool = False, col_scale=None, bias_gate: Optional[torch.Tensor] = None,
            norm: str = "layernorm"):
    """y = act(LN?(x) @ w^T + bias) (+ residual) on the 256-tile kernels with the LayerNorm folded in (module docstring of
    include/mio_hip.h, "LayerNorm folded into the GEMMs on either side of it").  Operands are [M, *] row-major 2-D tensors or,
    where the *_blocked flag says so, [ceil(M/256)*256, *] tensors in the blocked activation layout.
      ln_stats:           x is the raw residual stream, w_blocked / bias come from ln_fold_weight(...), ln_stats from the GEMM
                          that wrote x (stats_out=True);
      stats_out=True:     also returns the (sum, sum of squares) statistics of the rounded output rows;
      norm="rms":         the norm behind ln_stats is an RMSNorm (mio_gemm_rms_bw): w_blocked / bias come from
                          rms_fold_weight(...), the statistics from the same producer (their sums are not used).
    Returns (y, stats) -- stats is None unless stats_out."""
    rms = _norm_ok(norm, ln_stats is not None)
    _need_cuda(x, w_blocked)
    if activation not in _ACT:
        raise ValueError(f"Unsupported activation function: {activation}")
    act, dt = _ACT[activation], _dtype_id(x)
    glu = act == _lib.ACT_SWIGLU  # w_blocked = block_weight_glu(gate', up'), bias = up bias, bias_gate = gate bias, N = I
    if bias_gate is not None and not glu:
        raise ValueError("bias_gate belongs to activation='swiglu'")
    fold = ln_stats is not None
    if stats_out and residual is None:
        raise ValueError("gemm_ln: stats_out is the residual epilogue's form (give the residual)")
    if fold and residual is not None:
        raise ValueError("gemm_ln: the consumer form (ln_stats) takes no residual")
    if glu and residual is not None:
        raise ValueError("gemm_ln: the gated stage takes no residual")
    if not lib.mio_gemm_ln_ok(M, N, K, act, int(fold), int(stats_out)):
        raise ValueError("gemm_ln: this shape / activation does not take the folded kernels (gemm_ln_ok)")
    mp = (M + 255) // 256 * 256
    x2, ldx, r2, ldr = _gemm_ln_args(x, M, N, K, x_blocked, residual, res_blocked)
    wn = (N + 127) // 128 * 256 * K if glu else (N + 255) // 256 * 256 * K
    if w_blocked.dtype != x.dtype or w_blocked.device != x.device or not w_blocked.is_contiguous() or w_blocked.numel() != wn:
        raise ValueError(f"w_blocked: expected {wn} contiguous elements of x's dtype on its device (swiglu: block_weight_glu)")
    _vec_ok(bias, N, x.dtype, "bias")
    _vec_ok(bias_gate, N, x.dtype, "bias_gate")
    slots = 0
    if fold:
        want = ln_stats_shape(M, K)
        if ln_stats.dtype != torch.float32 or tuple(ln_stats.shape) != want or not ln_stats.is_contiguous() or ln_stats.device != x.device:
            raise ValueError(f"ln_stats: expected a contiguous fp32 tensor of shape {want}")
        ln_stats = ln_stats_for_launch(ln_stats, M)
        slots = ln_stats.shape[0]
    lo = hi = 0
    val = 1.0
    if col_scale is not None:
        lo, hi, val = int(col_scale[0]), int(col_scale[1]), float(col_scale[2])
        if residual is not None or lo % 128 or hi % 128 or not (0 <= lo <= hi <= N):
            raise ValueError(f"col_scale range [{lo}, {hi}) must be multiples of 128 inside [0, {N}], without a residual")
    y = torch.empty(mp if out_blocked else M, N, dtype=x.dtype, device=x.device)
    st = torch.empty(ln_stats_shape(M, N), dtype=torch.float32, device=x.device) if stats_out else None
    flags = (1 if x_blocked else 0) | (2 if out_blocked else 0) | (4 if (res_blocked and residual is not None) else 0)
    entry = lib.mio_gemm_rms_bw if rms else lib.mio_gemm_ln_bw
    check(entry(x2.data_ptr(), w_blocked.data_ptr(), _ptr(bias), _ptr(bias_gate), _ptr(r2), y.data_ptr(), M, N, K, ldx, N, ldr,
                act, dt, flags, _ptr(ln_stats), slots, float(eps), _ptr(st), lo, hi, val, _stream()))
    return y, st


def _blocked_sizes_ok(fc1_blocked, fc2_blocked, x, d, I, act):
    """The blocked copies travel as raw pointers: refuse a stale repack (other dtype / device / shape)."""
    n1 = (I + 127) // 128 * 256 * d if act == _lib.ACT_SWIGLU else (I + 255) // 256 * 256 * d
    n2 = (d + 255) // 256 * 256 * I
    for t, n, what in ((fc1_blocked, n1, "fc1_blocked"), (fc2_blocked, n2, "fc2_blocked")):
        if t.dtype != x.dtype or t.device != x.device or t.numel() != n or not t.is_contiguous():
            raise ValueError(f"{what}: expected {n} contiguous elements of the input's dtype on its device "
                             f"(swiglu: block_weight_glu(gate, up)); repack after converting the module")


def _mlp_args(hidden_states, fc1_weight, act, fc1_blocked=None, fc2_blocked=None, x_blocked_shape=None):
    """A fused_mlp call as the launch and fused_mlp_route both read it: (shape, M, d, I, bw, blocked).  shape is the logical
    [..., d] shape of the input (x_blocked_shape: hidden_states is layernorm(..., out_blocked=True) of such a tensor, in the
    blocked activation layout), bw says that the blocked-weight entry points take the call (else mio_fused_mlp_fwd), and
    blocked that both stages run on the 256x256-tile kernels: the rule of gemm_api.hip fused_mlp_impl, SwiGLU only with its
    interleaved blocked weight.  Host-only."""
    shape = tuple(hidden_states.shape if x_blocked_shape is None else x_blocked_shape)
    M, d, I = int(math.prod(shape[:-1])), shape[-1], fc1_weight.shape[0]
    ok = bool(lib.mio_fused_mlp_blocked_weight_ok(M, d, I, act))
    bw = ok and fc1_blocked is not None and fc2_blocked is not None
    if x_blocked_shape is not None and not bw:
        raise ValueError("a blocked activation operand needs blocked weights and fused_mlp_blocked_weight_ok()")
    return shape, M, d, I, bw, ok and (bw or act != _lib.ACT_SWIGLU)


def fused_mlp_route(hidden_states, fc1_weight, fc1_bias=None, fc2_weight=None, fc2_bias=None, activation: str = "gelu",
                    fc1_gate_weight=None, fc1_gate_bias=None, residual=None, fc1_blocked=None, fc2_blocked=None,
                    x_blocked_shape=None) -> dict:
    """How fused_mlp(...) with these arguments runs (host-only): {"path": "blocked" (both stages on the 256x256-tile kernels,
    the intermediate in the blocked layout) or "two_launch" (two gemm_bias_act launches, row-major intermediate),
    "stage1": route, "stage2": route} with route names of mio._lib.GEMM_ROUTES."""
    if activation not in _ACT or _ACT[activation] == _lib.ACT_NONE:
        raise ValueError(f"Unsupported activation function: {activation}")
    act = _ACT[activation]
    _shape, M, d, I, bw, blocked = _mlp_args(hidden_states, fc1_weight, act, fc1_blocked, fc2_blocked, x_blocked_shape)
    w2 = _lib.W_BLOCKED if blocked and bw else _lib.W_PLAIN
    w1 = _lib.W_GLU if blocked and act == _lib.ACT_SWIGLU else w2
    return {"path": "blocked" if blocked else "two_launch",
            "stage1": _gemm_route(M, I, d, d, d, I, 0, act, False, w1),
            "stage2": _gemm_route(M, d, I, I, I, d, d, _lib.ACT_NONE, residual is not None, w2)}


def fused_mlp(
    hidden_states: torch.Tensor,
    fc1_weight: torch.Tensor,
    fc1_bias: Optional[torch.Tensor],
    fc2_weight: torch.Tensor,
    fc2_bias: Optional[torch.Tensor],
    activation: str = "gelu",
    fc1_gate_weight: Optional[torch.Tensor] = None,
    fc1_gate_bias: Optional[torch.Tensor] = None,
    residual: Optional[torch.Tensor] = None,
    fc1_blocked: Optional[torch.Tensor] = None,
    fc2_blocked: Optional[torch.Tensor] = None,
    x_blocked_shape=None,
) -> torch.Tensor:
    """Drop-in for triton_fused_mlp (mlp_kernels.py:648-756): fc2(act(fc1(x))), hidden [B,S,d].
    "gelu" is the tanh form like the Triton kernel (:144-161); "gelu_erf" is pytorch_fused_mlp's (:782-783)."""
    xb = x_blocked_shape is not None
    if not xb and hidden_states.dim() != 3:
        raise ValueError(f"Expected 3D input tensor, got shape: {hidden_states.shape}")
    _need_cuda(hidden_states)
    if activation not in _ACT or _ACT[activation] == _lib.ACT_NONE:
        raise ValueError(f"Unsupported activation function: {activation}")
    act = _ACT[activation]
    glu = act == _lib.ACT_SWIGLU
    if glu and not xb and fc1_gate_weight is None:
        raise ValueError("SwiGLU activation requires gate weights")
    dt, dtype = _dtype_id(hidden_states), hidden_states.dtype
    shape, M, d, I, bw, _blocked = _mlp_args(hidden_states, fc1_weight, act, fc1_blocked, fc2_blocked, x_blocked_shape)
    x2 = hidden_states
    if not xb:
        if fc1_weight.shape[1] != d or tuple(fc2_weight.shape) != (d, I):
            raise ValueError("fc1/fc2 weight shapes do not match hidden size")
        x2 = _rows16(hidden_states.reshape(-1, d))
        if x2.stride(0) != d:
            x2 = x2.contiguous()
    _vec_ok(fc1_bias, I, dtype, "fc1_bias")
    _vec_ok(fc2_bias, d, dtype, "fc2_bias")
    gate_w, gate_b = (fc1_gate_weight, fc1_gate_bias) if glu else (None, None)
    _vec_ok(gate_b, I, dtype, "fc1_gate_bias")
    _res_ok(residual, M * d, dtype)
    if not xb:  # (a blocked input comes with blocked weights: the plain ones are not read)
        for w_ in (fc1_weight, fc2_weight) + ((gate_w,) if glu else ()):
            if w_.dtype != dtype or not w_.is_contiguous():
                raise ValueError("weights must be contiguous and of the input dtype")
    if bw:
        _blocked_sizes_ok(fc1_blocked, fc2_blocked, hidden_states, d, I, act)
    out = torch.empty(shape, dtype=dtype, device=hidden_states.device)
    # workspace in whole 256-row blocks (mio_fused_mlp_workspace_bytes): the intermediate may use a blocked layout
    work = torch.empty((M + 255) // 256 * 256, I, dtype=dtype, device=hidden_states.device)
    r2 = None if residual is None else residual.reshape(-1, d)
    if r2 is not None and not r2.is_contiguous():
        r2 = r2.contiguous()
    tail = (_ptr(r2), out.data_ptr(), work.data_ptr(), M, d, I)
    if bw and glu:
        check(lib.mio_fused_mlp_glu_fwd_bw(x2.data_ptr(), fc1_blocked.data_ptr(), _ptr(fc1_bias), _ptr(gate_b),
                                           fc2_blocked.data_ptr(), _ptr(fc2_bias), *tail, dt, int(xb), _stream()))
    elif bw:
        check(lib.mio_fused_mlp_fwd_bw(x2.data_ptr(), fc1_blocked.data_ptr(), _ptr(fc1_bias), fc2_blocked.data_ptr(),
                                       _ptr(fc2_bias), *tail, act, dt, int(xb), _stream()))
    else:
        check(lib.mio_fused_mlp_fwd(x2.data_ptr(), fc1_weight.data_ptr(), _ptr(fc1_bias), _ptr(gate_w), _ptr(gate_b),
                                    fc2_weight.data_ptr(), _ptr(fc2_bias), *tail, act, dt, _stream()))
    return out


RMSNORM_MAX_COLS = 8192


def _row_norm(kind: str, x, weight, bias, eps, residual, residual_alpha, return_sum: bool, out_blocked: bool):
    """layernorm / rmsnorm (kind "layernorm" / "rmsnorm"): the checks, the operands as contiguous rows, the outputs, one launch."""
    rms = kind == "rmsnorm"
    _need_cuda(x, weight)
    dt = _dtype_id(x)
    cols = x.shape[-1]
    if rms and cols > RMSNORM_MAX_COLS:
        raise ValueError(f"rmsnorm takes up to {RMSNORM_MAX_COLS} columns, got {cols}")
    _vec_ok(weight, cols, x.dtype, f"{kind} weight")
    if not rms:
        _vec_ok(bias, cols, x.dtype, "layernorm bias")
    _res_ok(residual, x.numel(), x.dtype)
    x2 = x.reshape(-1, cols)
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    r2 = None
    if residual is not None:
        r2 = residual.reshape(-1, cols)
        if not r2.is_contiguous():
            r2 = r2.contiguous()
    s = torch.empty_like(x2) if (return_sum and r2 is not None) else None
    if out_blocked:
        if cols % 32 != 0:
            raise ValueError("out_blocked needs cols % 32 == 0")
        y = torch.empty((x2.shape[0] + 255) // 256 * 256, cols, dtype=x.dtype, device=x.device)
    else:
        y = torch.empty_like(x2)
    tail = (y.data_ptr(), _ptr(s), x2.shape[0], cols, float(eps), float(residual_alpha), dt)
    if rms:
        check(lib.mio_rmsnorm_fwd(x2.data_ptr(), _ptr(r2), weight.data_ptr(), *tail, int(out_blocked), _stream()))
    else:
        entry = lib.mio_layernorm_fwd_bx if out_blocked else lib.mio_layernorm_fwd
        check(entry(x2.data_ptr(), _ptr(r2), weight.data_ptr(), _ptr(bias), *tail, _stream()))
    if not out_blocked:
        y = y.view(x.shape)
    if return_sum:
        return y, (s.view(x.shape) if s is not None else x)
    return y


def layernorm(x, weight, bias=None, eps: float = 1e-5, residual=None, residual_alpha: float = 1.0,
              return_sum: bool = False, out_blocked: bool = False):
    """Drop-in for triton_layernorm (layernorm_kernels.py:191-276): optional x + alpha*residual first.
    out_blocked: y is returned as a [ceil(rows/256)*256, cols] tensor in the blocked activation layout
    (include/mio_hip.h) for a following gemm_bias_act / fused_mlp with x_blocked_shape=x.shape."""
    return _row_norm("layernorm", x, weight, bias, eps, residual, residual_alpha, return_sum, out_blocked)


def rmsnorm(x, weight, eps: float = 1e-6, residual=None, residual_alpha: float = 1.0, return_sum: bool = False,
            out_blocked: bool = False):
    """RMSNorm over the last dim (torch.nn.functional.rms_norm with a weight): y = s * rsqrt(mean(s^2) + eps) * weight, s = x or
    x + alpha*residual (return_sum: rounded, returned, and y is RMSNorm of the returned tensor exactly).  Arguments and return
    shapes as layernorm; up to 8192 columns."""
    return _row_norm("rmsnorm", x, weight, None, eps, residual, residual_alpha, return_sum, out_blocked)


# ------------------------------------------------------------------------------------------------
# paged decode
# ------------------------------------------------------------------------------------------------
def _i32_dev(t: torch.Tensor, name: str, dim: int, what: str, device) -> None:
    if t.dtype != torch.int32 or t.dim() != dim or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {dim}-D int32 tensor {what}")
    if t.device != device:
        raise ValueError(f"{name} must be on the device of q")


def _paged_params(q, k_cache, v_cache, block_tables, cu_seqlens_q, seqused_k, max_seqlen_q, max_seqlen_k, layer_idx=0,
                  causal=False, softmax_scale=None, return_lse=False, out=None):
    """flash_attention_varlen_paged's argument checks and mio_fa3_paged_params_t for a 16-bit cache; returns (params,
    out, lse, keep) as _varlen_params does.  Reads no device memory."""
    p, out, lse, keep, _scales = _paged_args(q, k_cache, v_cache, block_tables, cu_seqlens_q, seqused_k, max_seqlen_q,
                                             max_seqlen_k, layer_idx, causal, softmax_scale, return_lse, out)
    return p, out, lse, keep


def _paged_args(q, k_cache, v_cache, block_tables, cu_seqlens_q, seqused_k, max_seqlen_q, max_seqlen_k, layer_idx=0,
                causal=False, softmax_scale=None, return_lse=False, out=None, k_scale=None, v_scale=None):
    """_paged_params for either cache: also returns the scale addresses of an fp8 (float8_e4m3fn) cache (None for a
    16-bit one), checked as paged decode checks them (_kv8_kind, _kv_scales)."""
    if q.dim() != 3:
        raise ValueError(f"Expected a 3D tensor [tokens, heads, head_dim] for q but got shape {q.shape}")
    if k_cache.dim() != 5 or v_cache.shape != k_cache.shape:
        raise ValueError("caches must be [num_blocks, num_layers, block_size, num_kv_heads, head_dim] with equal shapes")
    scales = None
    if k_cache.element_size() == 1 or v_cache.element_size() == 1 or k_scale is not None or v_scale is not None:
        _kv8_kind(k_cache, v_cache)
        scales = _kv_scales(k_cache.dtype, k_scale, v_scale, k_cache.shape[1], layer_idx, k_cache.device,
                            "flash_attention_varlen_paged")
        if v_cache.dtype != k_cache.dtype:
            raise ValueError("k_cache and v_cache must share a dtype")
        dt = _dtype_id(q)
        if q.shape[-1] % 16 != 0:
            raise ValueError(f"an fp8 KV cache needs head_dim to be a multiple of 16, got head_dim {q.shape[-1]}")
    else:
        dt = _qkv_dtype(q, k_cache, v_cache, "q, k_cache, v_cache")
    if not (k_cache.is_contiguous() and v_cache.is_contiguous()):
        raise ValueError("caches must be contiguous")
    _i32_dev(cu_seqlens_q, "cu_seqlens_q", 1, "of B+1 offsets", q.device)
    if cu_seqlens_q.numel() < 1:
        raise ValueError("cu_seqlens_q must be a contiguous 1-D int32 tensor of B+1 offsets")
    B = cu_seqlens_q.numel() - 1
    _i32_dev(seqused_k, "seqused_k", 1, "of B key counts", q.device)
    _i32_dev(block_tables, "block_tables", 2, "[B, max_blocks_per_seq]", q.device)
    if seqused_k.numel() != B or block_tables.shape[0] != B:
        raise ValueError(f"seqused_k and block_tables must have B = {B} rows (cu_seqlens_q has B+1 entries)")
    q = _rows16(q)
    Tq, H, D = q.shape
    nb, L, bs, Hkv, Dc = k_cache.shape
    if Dc != D:
        raise ValueError(f"incompatible q/cache shapes: q={q.shape}, k_cache={k_cache.shape}")
    _check_heads(H, Hkv, D)
    if bs % 64 != 0:
        raise ValueError(f"block_size must be a multiple of 64 for the paged attention kernels, got {bs}")
    if not 0 <= int(layer_idx) < L:
        raise ValueError(f"layer_idx {layer_idx} out of range for a {L}-layer cache")
    scale = _softmax_scale(D, softmax_scale)
    out = _out_like(q, out)
    lse = _packed_lse(q, return_lse)

    p = _lib.FaPagedParams()
    for dst, t in ((p.q_stride, q), (p.o_stride, out)):
        dst[0], dst[1] = t.stride(0), t.stride(1)
    p.q, p.k_cache, p.v_cache, p.o, p.lse = q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), out.data_ptr(), _ptr(lse)
    _fill_null(p, ("q", "k_cache", "v_cache", "o"), cu_seqlens_q.data_ptr())
    p.cu_seqlens_q, p.seqused_k, p.block_tables = cu_seqlens_q.data_ptr(), seqused_k.data_ptr(), block_tables.data_ptr()
    p.B, p.total_q = B, Tq
    p.max_seqlen_q, p.max_seqlen_k = int(max_seqlen_q), int(max_seqlen_k)
    p.H, p.Hkv, p.D = H, Hkv, D
    p.num_blocks, p.num_layers, p.layer_idx, p.block_size = nb, L, int(layer_idx), bs
    p.max_blocks_per_seq = block_tables.shape[1]
    p.dtype, p.causal, p.softmax_scale = dt, int(bool(causal)), scale
    return p, out, lse, (q, k_cache, v_cache, block_tables, cu_seqlens_q, seqused_k, k_scale, v_scale), scales


def flash_attention_varlen_paged(
    q: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    block_tables: torch.Tensor,
    cu_seqlens_q: torch.Tensor,
    seqused_k: torch.Tensor,
    max_seqlen_q: int,
    max_seqlen_k: int,
    layer_idx: int = 0,
    causal: bool = False,
    softmax_scale: Optional[float] = None,
    return_lse: bool = False,
    out: Optional[torch.Tensor] = None,
    *,
    window_size=(-1, -1),
    k_scale: Optional[torch.Tensor] = None,
    v_scale: Optional[torch.Tensor] = None,
):
    """Packed variable-length attention forward over the paged KV cache (chunked prefill), mio_fa3_fwd_paged.

    q [total_q, H, D] packed by cu_seqlens_q (int32 [B+1]) as in flash_attention_varlen.  k_cache / v_cache
    [num_blocks, num_layers, block_size, Hkv, D] contiguous (PagedKVCache's layout), read at layer_idx; block_size must
    be a multiple of 64.  Sequence b attends keys 0 .. min(seqused_k[b], max_seqlen_k) - 1, key j in page
    block_tables[b, j // block_size] (int32 [B, max_blocks_per_seq]) at slot j % block_size.  causal is bottom-right
    aligned: query i of a sequence sees key j iff j <= i + Lk - Lq.  Rows with no visible key get 0 (lse -inf).
    Returns out [total_q, H, D] or (out, lse fp32 [H, total_q]) if return_lse.  Queued on the current stream with no host
    sync (graph-capturable): the offsets and tables are never read on the host.
    window_size = (left, right): sliding window as in flash_attention_varlen; only the pages inside each query block's
    window are read.
    FP8 cache: k_cache / v_cache torch.float8_e4m3fn (q / out bf16 or fp16, head_dim a multiple of 16) with k_scale /
    v_scale, fp32 device tensors of 1 or num_layers elements (PagedKVCache.get_kv_scales()): attention over
    K = k_cache * k_scale, V = v_cache * v_scale (mio_fa3_fwd_paged_kv8), everything else as above.  The scales are read
    on the device, never on the host.
    """
    w = _window(window_size, causal)
    _need_cuda(q, k_cache, v_cache, block_tables, cu_seqlens_q, seqused_k)
    p, out, lse, _keep, scales = _paged_args(q, k_cache, v_cache, block_tables, cu_seqlens_q, seqused_k, max_seqlen_q,
                                             max_seqlen_k, layer_idx=layer_idx, causal=causal,
                                             softmax_scale=softmax_scale, return_lse=return_lse, out=out,
                                             k_scale=k_scale, v_scale=v_scale)
    if scales is not None:
        return _launch(lib.mio_fa3_fwd_paged_kv8, p, w, out, lse, return_lse, *scales)
    return _launch(lib.mio_fa3_fwd_paged_window, p, w, out, lse, return_lse)


def fa3_paged_route(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, block_tables: torch.Tensor,
                    cu_seqlens_q: torch.Tensor, seqused_k: torch.Tensor, max_seqlen_q: int, max_seqlen_k: int,
                    **kwargs) -> str:
    """The kernel flash_attention_varlen_paged(...) would launch (mio_fa3_paged_route): "empty", "fwd5" or "fwd3",
    without launching.  Tensors may live on any device; arguments flash_attention_varlen_paged refuses raise the same
    errors."""
    w = _window(kwargs.pop("window_size", (-1, -1)), kwargs.get("causal", False))
    p, _out, _lse, _keep, scales = _paged_args(q, k_cache, v_cache, block_tables, cu_seqlens_q, seqused_k, max_seqlen_q,
                                               max_seqlen_k, **kwargs)
    if scales is not None:
        return _route(lib.mio_fa3_paged_kv8_route, p, w, _lib.FA3_PAGED_ROUTES, *scales)
    return _route(lib.mio_fa3_paged_route_window, p, w, _lib.FA3_PAGED_ROUTES)


def _decode_window(window_size) -> int:
    """The left bound of a decode window_size = (left, right): each -1 (unbounded) or >= 0, and right must be -1 (a
    decode row sees every cached key up to its own position).  Raises ValueError otherwise."""
    left, right = _window(window_size)
    if right != -1:
        raise ValueError(f"paged decode takes no right window: window_size[1] must be -1, got {right}")
    return left


# the fp8 KV cache: OCP e4m3fn only (MI300's e4m3fnuz is another encoding)
_KV8 = torch.float8_e4m3fn


def _kv8_kind(k_cache, v_cache) -> None:
    """One-byte caches must be float8_e4m3fn (not e5m2, e4m3fnuz or an integer type): ValueError otherwise."""
    for c in (k_cache, v_cache):
        if c.element_size() == 1 and c.dtype != _KV8:
            raise ValueError(f"an 8-bit KV cache must be torch.float8_e4m3fn (OCP e4m3), got {c.dtype}")


def _kv_scales(cache_dtype, k_scale, v_scale, L: int, layer_idx: int, device, who: str):
    """None for a 16-bit cache (which takes no scales); for a float8_e4m3fn cache, the device addresses of the fp32
    scales the kernels read for layer_idx (1 element shared by all layers, or num_layers elements).  ValueError for any
    other cache dtype or scale misuse."""
    if cache_dtype in (torch.bfloat16, torch.float16):
        if k_scale is not None or v_scale is not None:
            raise ValueError(f"{who}: k_scale / v_scale apply to an fp8 (float8_e4m3fn) cache only, got a "
                             f"{cache_dtype} cache")
        return None
    if cache_dtype != _KV8:
        raise ValueError(f"{who}: the KV cache must be bf16, fp16 or float8_e4m3fn, got {cache_dtype}")
    if k_scale is None or v_scale is None:
        raise ValueError(f"{who}: an fp8 (float8_e4m3fn) cache requires k_scale and v_scale")
    ptrs = []
    for name, s in (("k_scale", k_scale), ("v_scale", v_scale)):
        if not isinstance(s, torch.Tensor) or s.dtype != torch.float32 or not s.is_contiguous():
            raise ValueError(f"{who}: {name} must be a contiguous float32 tensor")
        if s.numel() not in (1, L):
            raise ValueError(f"{who}: {name} must hold 1 or num_layers = {L} elements, got {s.numel()}")
        if s.device != device:
            raise ValueError(f"{who}: {name} must be on the device of the cache")
        if s.numel() > 1 and not 0 <= int(layer_idx) < L:
            raise ValueError(f"{who}: layer_idx {layer_idx} out of range for a {L}-layer cache")
        ptrs.append(s.data_ptr() + (4 * int(layer_idx) if s.numel() > 1 else 0))
    return tuple(ptrs)


def _decode_args(query, output, k_cache, v_cache, block_tables, context_lengths, block_size, max_seq_len, layer_idx,
                 scale, k_scale=None, v_scale=None):
    """The checked arguments of mio_fa3_decode_paged(_window / _kv8) up to the window, the scale addresses (None for a
    16-bit cache) and the tensors they point into."""
    _need_cuda(query, output, k_cache, v_cache, block_tables, context_lengths)
    if query.dim() != 4 or output.shape != query.shape:
        raise ValueError("query/output must be [B,H,q_len,D] with equal shapes")
    if k_cache.dim() != 5 or v_cache.shape != k_cache.shape:
        raise ValueError("caches must be [num_blocks, num_layers, block_size, num_kv_heads, head_dim]")
    dt = _dtype_id(query)
    _kv8_kind(k_cache, v_cache)
    if output.dtype != query.dtype or v_cache.dtype != k_cache.dtype:
        raise ValueError("query, output and caches must share a dtype")
    if k_cache.dtype != _KV8 and k_cache.dtype != query.dtype:
        raise ValueError("query, output and caches must share a dtype")
    if not (k_cache.is_contiguous() and v_cache.is_contiguous()):
        raise ValueError("caches must be contiguous")
    B, H, q_len, D = query.shape
    nb, L, bs, Hkv, Dc = k_cache.shape
    if bs != block_size or Dc != D:
        raise ValueError("cache geometry does not match block_size/head_dim")
    scales = _kv_scales(k_cache.dtype, k_scale, v_scale, L, layer_idx, k_cache.device, "paged_attention_forward")
    if scales is not None and D % 16 != 0:
        raise ValueError(f"an fp8 KV cache needs head_dim to be a multiple of 16, got head_dim {D}")
    q = _rows16(query)
    if output.stride(-1) != 1:
        raise ValueError("output last dim must be contiguous")
    bt = block_tables.to(torch.int32).contiguous()
    cl = context_lengths.to(torch.int32).contiguous()
    sc = (1.0 / math.sqrt(D)) if scale is None else float(scale)
    qs = (C.c_int64 * 3)(q.stride(0), q.stride(1), q.stride(2))
    os_ = (C.c_int64 * 3)(output.stride(0), output.stride(1), output.stride(2))
    if scales is None:
        args = (q.data_ptr(), output.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), bt.data_ptr(), cl.data_ptr(),
                qs, os_, B, H, Hkv, q_len, D, L, int(layer_idx), bs, bt.shape[1], int(max_seq_len), sc)
    else:
        args = (q.data_ptr(), output.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), *scales, bt.data_ptr(),
                cl.data_ptr(), qs, os_, B, H, Hkv, q_len, D, L, int(layer_idx), bs, bt.shape[1], int(max_seq_len), sc)
    return args, dt, scales is not None, (q, bt, cl, k_scale, v_scale)


def paged_attention_forward(query, output, k_cache, v_cache, block_tables, context_lengths, block_size: int,
                            max_seq_len: int, layer_idx: int, scale: Optional[float] = None, *,
                            window_size=(-1, -1), k_scale=None, v_scale=None) -> torch.Tensor:
    """Drop-in for triton_paged_attention_forward (attention_kernels.py:1206-1311).
    query/output [B,H,q_len,D] (output caller-preallocated, :1208,1286); caches
    [num_blocks, L, block_size, Hkv, D]; block_tables [B,max_blocks] int32; context_lengths [B] int32.

    window_size = (left, -1): sliding-window decode (flash-attn's convention): row qi of q_len sees the cached keys
    j < ctx with j >= ctx - q_len + qi - left; only the window's keys are read.  (-1, -1) (the default) is the
    unwindowed launch exactly.

    FP8 cache: k_cache / v_cache torch.float8_e4m3fn (query / output bf16 or fp16, head_dim a multiple of 16) with
    k_scale / v_scale, fp32 device tensors of 1 or num_layers elements: attention over K = k_cache * k_scale,
    V = v_cache * v_scale (mio_fa3_decode_paged_kv8).  The scales are read on the device, never on the host."""
    left = _decode_window(window_size)
    args, dt, kv8, keep = _decode_args(query, output, k_cache, v_cache, block_tables, context_lengths, block_size,
                                       max_seq_len, layer_idx, scale, k_scale, v_scale)
    B, H, q_len, D = query.shape
    nbytes = lib.mio_fa3_decode_workspace_bytes(B, H, q_len, D, int(max_seq_len))
    work = torch.empty(nbytes, dtype=torch.uint8, device=query.device)
    if kv8:
        check(lib.mio_fa3_decode_paged_kv8(*args, left, dt, work.data_ptr(), _stream()))
    elif left < 0:
        check(lib.mio_fa3_decode_paged(*args, dt, work.data_ptr(), _stream()))
    else:
        check(lib.mio_fa3_decode_paged_window(*args, left, -1, dt, work.data_ptr(), _stream()))
    del keep
    return output


def paged_attention_route(query, output, k_cache, v_cache, block_tables, context_lengths, block_size: int,
                          max_seq_len: int, layer_idx: int, scale: Optional[float] = None, *,
                          window_size=(-1, -1), k_scale=None, v_scale=None) -> str:
    """The decode kernel paged_attention_forward takes for these arguments ("head", "rows" or "gqa",
    mio_fa3_decode_window_route / mio_fa3_decode_kv8_route); nothing is launched."""
    left = _decode_window(window_size)
    args, dt, kv8, keep = _decode_args(query, output, k_cache, v_cache, block_tables, context_lengths, block_size,
                                       max_seq_len, layer_idx, scale, k_scale, v_scale)
    if kv8:
        r = lib.mio_fa3_decode_kv8_route(*args, left, dt, None, None)
    else:
        r = lib.mio_fa3_decode_window_route(*args, left, -1, dt, None, None)
    del keep
    if r < 0:
        check(r)
    return _lib.DECODE_ROUTES[r]


def _write_caches(key, value, k_cache, v_cache, layer_idx, k_scale, v_scale, who):
    """The cache checks the cache writes share: value shares key's dtype; the caches are 5-D, equal, contiguous,
    and either of key's dtype or float8_e4m3fn with scales.  Returns the scale addresses (None for a 16-bit cache)."""
    if value.dtype != key.dtype:
        raise ValueError("key, value and caches must share a dtype")
    _kv8_kind(k_cache, v_cache)
    if k_cache.dim() != 5 or v_cache.shape != k_cache.shape:
        raise ValueError("caches must be [num_blocks, num_layers, block_size, num_kv_heads, head_dim] with equal shapes")
    if v_cache.dtype != k_cache.dtype or (k_cache.dtype != _KV8 and k_cache.dtype != key.dtype):
        raise ValueError("key, value and caches must share a dtype")
    if not (k_cache.is_contiguous() and v_cache.is_contiguous()):
        raise ValueError("caches must be contiguous")
    scales = _kv_scales(k_cache.dtype, k_scale, v_scale, k_cache.shape[1], layer_idx, k_cache.device, who)
    if scales is not None and key.shape[-1] % 16 != 0:
        raise ValueError(f"an fp8 KV cache needs head_dim to be a multiple of 16, got head_dim {key.shape[-1]}")
    return scales


def _cache_write_args(key, value, k_cache, v_cache, block_tables, context_lengths, block_size, layer_idx, k_scale, v_scale,
                      who, cu_seqlens_new=None, q=None):
    """The argument checks the three cache writes share and what they pass to the library; host only (shapes, strides,
    dtypes and addresses: the tensors may live on any device, the public functions call _need_cuda first).
    cu_seqlens_new None: the single-token form, key / value [B, 1, Hkv, D], block_tables / context_lengths converted to
    int32.  Otherwise the varlen forms: key / value [total_new, Hkv, D], strict int32 tables; q (the rotating write) is
    checked against key.  Returns a namespace: data (key, value, cache and scale addresses, in the C order), tables
    (block_tables, [cu_seqlens_new,] context_lengths), strides (k, v), B, T, Hkv, D, geom (num_blocks, num_layers, layer_idx,
    block_size, max_blocks_per_seq), dt, kv8, and keep (the tensors the addresses point into)."""
    varlen = cu_seqlens_new is not None
    if not varlen:
        if key.dim() != 4 or key.shape[1] != 1:
            raise ValueError("reshape_and_cache supports q_seq_len == 1 only (attention_kernels.py:1363-1365)")
    elif key.dim() != 3 or value.shape != key.shape:
        raise ValueError(f"key/value must be [total_new, num_kv_heads, head_dim] with equal shapes, got "
                         f"key={tuple(key.shape)}, value={tuple(value.shape)}")
    dt = _dtype_id(key)
    scales = _write_caches(key, value, k_cache, v_cache, layer_idx, k_scale, v_scale, who)
    T, Hkv, D = key.shape[0], key.shape[-2], key.shape[-1]
    if q is not None and (q.dim() != 3 or q.shape[0] != T or q.shape[2] != D or q.dtype != key.dtype):
        raise ValueError(f"q must be [total_new, num_heads, head_dim] = [{T}, H, {D}] of key's dtype, got "
                         f"{tuple(q.shape)} {q.dtype}")
    nb, L, bs, Hc, Dc = k_cache.shape
    if (Hc, Dc, bs) != (Hkv, D, block_size):
        raise ValueError("cache geometry mismatch")
    if varlen:
        if D % 8 != 0:
            raise ValueError(f"head_dim must be a multiple of 8, got {D}")
        if q is not None:
            _check_heads(q.shape[1], Hkv, D)
        if not 0 <= int(layer_idx) < L:
            raise ValueError(f"layer_idx {layer_idx} out of range for a {L}-layer cache")
        _i32_dev(cu_seqlens_new, "cu_seqlens_new", 1, "of B+1 offsets", key.device)
        if cu_seqlens_new.numel() < 1:
            raise ValueError("cu_seqlens_new must be a contiguous 1-D int32 tensor of B+1 offsets")
        B = cu_seqlens_new.numel() - 1
        _i32_dev(context_lengths, "context_lengths", 1, "of B lengths", key.device)
        _i32_dev(block_tables, "block_tables", 2, "[B, max_blocks_per_seq]", key.device)
        if context_lengths.numel() != B or block_tables.shape[0] != B:
            raise ValueError(f"context_lengths and block_tables must have B = {B} rows (cu_seqlens_new has B+1 entries)")
        tables = (block_tables, cu_seqlens_new, context_lengths)
    else:
        B = T
        tables = (block_tables.to(torch.int32).contiguous(), context_lengths.to(torch.int32).contiguous())
    key, value = _rows16(key), _rows16(value)
    strides = tuple((C.c_int64 * 2)(t.stride(0), t.stride(-2)) for t in (key, value))
    return types.SimpleNamespace(
        data=(key.data_ptr(), value.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), *(scales or ())),
        tables=tuple(t.data_ptr() for t in tables), strides=strides, B=B, T=T, Hkv=Hkv, D=D,
        geom=(nb, L, int(layer_idx), bs, tables[0].shape[1]), dt=dt, kv8=scales is not None,
        keep=(key, value, tables, k_scale, v_scale))


def reshape_and_cache(key, value, k_cache, v_cache, block_tables, context_lengths, block_size: int, layer_idx: int, *,
                      k_scale=None, v_scale=None):
    """Drop-in for triton_reshape_and_cache (attention_kernels.py:1314-1407): key/value [B,1,Hkv,D].
    The caches share key's dtype, or are torch.float8_e4m3fn with k_scale / v_scale (fp32 device tensors of 1 or
    num_layers elements): the written bytes are e4m3(clamp(x * (1 / scale), -448, 448)) (mio_reshape_and_cache_kv8)."""
    _need_cuda(key, value, k_cache, v_cache)
    w = _cache_write_args(key, value, k_cache, v_cache, block_tables, context_lengths, block_size, layer_idx, k_scale,
                          v_scale, "reshape_and_cache")
    fn = lib.mio_reshape_and_cache_kv8 if w.kv8 else lib.mio_reshape_and_cache
    check(fn(*w.data, *w.tables, *w.strides, w.B, w.Hkv, w.D, *w.geom[1:], w.dt, _stream()))


def reshape_and_cache_varlen(key, value, k_cache, v_cache, block_tables, cu_seqlens_new, context_lengths,
                             block_size: int, layer_idx: int, *, k_scale=None, v_scale=None):
    """Write many new tokens per sequence into the paged cache (mio_reshape_and_cache_varlen).

    key / value [total_new, Hkv, D] packed by cu_seqlens_new (int32 [B+1]); context_lengths (int32 [B]) holds each
    sequence's length AFTER the append, so token i of the n_b new ones goes to position context_lengths[b] - n_b + i of
    the pages in block_tables (int32 [B, max_blocks_per_seq]).  Positions that are negative or past the table row are
    skipped.  Byte-exact copies, queued on the current stream with no host sync (graph-capturable).
    FP8 cache: as reshape_and_cache, torch.float8_e4m3fn caches with k_scale / v_scale (mio_reshape_and_cache_varlen_kv8)."""
    _need_cuda(key, value, k_cache, v_cache, block_tables, cu_seqlens_new, context_lengths)
    w = _cache_write_args(key, value, k_cache, v_cache, block_tables, context_lengths, block_size, layer_idx, k_scale,
                          v_scale, "reshape_and_cache_varlen", cu_seqlens_new)
    fn = lib.mio_reshape_and_cache_varlen_kv8 if w.kv8 else lib.mio_reshape_and_cache_varlen
    check(fn(*w.data, *w.tables, *w.strides, w.B, w.T, w.Hkv, w.D, *w.geom, w.dt, _stream()))


# ------------------------------------------------------------------------------------------------
# rotary position embedding
# ------------------------------------------------------------------------------------------------
def rope_tables(max_position: int, rot_dim: int, base: float = 10000.0, device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The (cos, sin) tables of the plain rotary schedule, fp32 [max_position, rot_dim / 2]: entry (p, i) is the cosine /
    sine of p * base ** (-2 i / rot_dim), the angle computed in fp64 and cast once.  Any other schedule (scaled, YaRN,
    Llama-3) is a table of the same shape the caller builds."""
    max_position, rot_dim = operator.index(max_position), operator.index(rot_dim)
    if max_position <= 0:
        raise ValueError(f"max_position must be positive, got {max_position}")
    if rot_dim <= 0 or rot_dim % 2 != 0:
        raise ValueError(f"rot_dim must be a positive even number, got {rot_dim}")
    inv_freq = float(base) ** (-torch.arange(0, rot_dim, 2, dtype=torch.float64) / rot_dim)
    ang = torch.arange(max_position, dtype=torch.float64)[:, None] * inv_freq[None, :]
    return ang.cos().to(torch.float32).to(device), ang.sin().to(torch.float32).to(device)


def _rope_tables_ok(cos, sin, D: int, kv8: bool, interleaved: bool, device, who: str) -> Tuple[int, int]:
    """The checks of the (cos, sin) tables; returns (max_position, rot_dim)."""
    for name, t in (("cos", cos), ("sin", sin)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 2 or not t.is_contiguous():
            raise ValueError(f"{who}: {name} must be a contiguous float32 tensor [max_position, rot_dim / 2]")
        if t.device != device:
            raise ValueError(f"{who}: {name} must be on the device of the rotated tensor")
    if sin.shape != cos.shape:
        raise ValueError(f"{who}: cos and sin must have equal shapes, got {tuple(cos.shape)} and {tuple(sin.shape)}")
    max_position, rot_dim = cos.shape[0], 2 * cos.shape[1]
    if max_position < 1:
        raise ValueError(f"{who}: the tables must hold at least one position")
    if rot_dim < 16 or rot_dim % 16 != 0 or rot_dim > D:
        raise ValueError(f"{who}: rot_dim must be a multiple of 16 in [16, head_dim = {D}], got {rot_dim}")
    if kv8 and not interleaved and rot_dim % 32 != 0:
        raise ValueError(f"{who}: rot_dim must be a multiple of 32 for an fp8 cache with the neox pairing, got {rot_dim}")
    if cos.data_ptr() % 16 or sin.data_ptr() % 16:
        raise ValueError(f"{who}: cos and sin must be 16-byte aligned")
    return max_position, rot_dim


def apply_rotary(x, cos, sin, positions, *, interleaved: bool = False, out=None) -> torch.Tensor:
    """Rotary position embedding of x (mio_rope_rows): x [tokens, heads, D] with positions int32 [tokens], or
    [B, S, heads, D] with positions [B, S] or [S].  The first rot_dim = 2 * cos.shape[1] elements of every head are rotated by
    the angles cos / sin hold (fp32 [max_position, rot_dim / 2], rope_tables or the caller's schedule) for the token's
    position: y1 = x1 c - x2 s, y2 = x2 c + x1 s in fp32, rounded once; the neox pairing (i with i + rot_dim / 2) or, with
    interleaved, GPT-J's (2 i with 2 i + 1).  Elements past rot_dim are copied.  A position outside [0, max_position) gives a
    row of zeros.  out (x's shape and dtype, last dim contiguous, strides multiples of 8) may be x itself."""
    r = _rotary_rows_args("apply_rotary", x, cos, sin, positions, interleaved, out)
    check(lib.mio_rope_rows(*r.head, *r.strides, *r.sizes, _stream()))
    return r.res


def _rotary_rows_args(who: str, x, cos, sin, positions, interleaved: bool, out, weight=None):
    """The argument checks of the standalone rotary forms (apply_rotary, qk_norm_rotary) and what they pass to the library:
    head (x, out, positions, cos, sin[, weight] addresses), strides (x, out), sizes (tokens, heads, D, rot_dim, max_position,
    interleaved, dtype), res (the tensor to return) and keep (the tensors the addresses point into)."""
    if not isinstance(x, torch.Tensor) or x.dim() not in (3, 4):
        raise ValueError(f"{who}: x must be [tokens, heads, head_dim] or [B, S, heads, head_dim]")
    _need_cuda(x, cos, sin, positions, out, weight)
    dt = _dtype_id(x)
    D = x.shape[-1]
    if D % 8 != 0 or D > 128:
        raise ValueError(f"head_dim must be a multiple of 8 and <= 128, got {D}")
    max_position, rot_dim = _rope_tables_ok(cos, sin, D, False, interleaved, x.device, who)
    if weight is not None:
        _qk_weight_ok(weight, x, "weight", who)
    if not isinstance(positions, torch.Tensor) or positions.dtype != torch.int32 or positions.device != x.device:
        raise ValueError(f"{who}: positions must be an int32 tensor on the device of x")
    if out is not None and (out.shape != x.shape or out.dtype != x.dtype or out.device != x.device):
        raise ValueError(f"{who}: out must have x's shape, dtype and device")
    shape = x.shape
    if x.dim() == 4:
        B, S = shape[0], shape[1]
        if tuple(positions.shape) == (S,):
            positions = positions.expand(B, S)
        if tuple(positions.shape) != (B, S):
            raise ValueError(f"{who}: positions must be [B, S] = [{B}, {S}] or [S], got {tuple(positions.shape)}")
        positions = positions.reshape(B * S)
        # [B, S] collapse to one token axis where the strides allow it (a view of a [B, S, n] projection does)
        x3 = x.reshape(B * S, shape[2], D) if x.stride(0) == S * x.stride(1) else x.contiguous().view(B * S, shape[2], D)
        out3 = None
        if out is not None:
            if out.stride(0) != S * out.stride(1):
                raise ValueError(f"{who}: out's batch and sequence axes must collapse to one token axis")
            out3 = out.view(B * S, shape[2], D)
    else:
        if positions.dim() != 1 or positions.numel() != shape[0]:
            raise ValueError(f"{who}: positions must be [tokens] = [{shape[0]}], got {tuple(positions.shape)}")
        x3, out3 = x, out
    positions = positions.contiguous()
    x3 = _rows16(x3)
    if out3 is None:
        res = torch.empty(shape, dtype=x.dtype, device=x.device)
        out3 = res.view(x3.shape)
    else:
        res = out
        if out3.stride(-1) != 1 or any(s % 8 for s in out3.stride()[:-1]) or out3.data_ptr() % 16:
            raise ValueError(f"{who}: out needs a contiguous last dim, strides that are multiples of 8 and 16-byte alignment")
    T, Hn, _ = x3.shape
    xs = (C.c_int64 * 2)(x3.stride(0), x3.stride(1))
    os_ = (C.c_int64 * 2)(out3.stride(0), out3.stride(1))
    head = (x3.data_ptr(), out3.data_ptr(), positions.data_ptr(), cos.data_ptr(), sin.data_ptr())
    if weight is not None:
        head += (weight.data_ptr(),)
    return types.SimpleNamespace(head=head, strides=(xs, os_), res=res, keep=(x3, out3, positions),
                                 sizes=(T, Hn, D, rot_dim, max_position, int(bool(interleaved)), dt))


def _qk_weight_ok(w, x, name: str, who: str) -> None:
    """A QK-norm weight: [head_dim] of x's dtype on x's device, contiguous and 16-byte aligned."""
    D = x.shape[-1]
    if not isinstance(w, torch.Tensor) or w.dim() != 1 or w.numel() != D or w.dtype != x.dtype or w.device != x.device \
            or not w.is_contiguous():
        raise ValueError(f"{who}: {name} must be a contiguous [head_dim] = [{D}] tensor of {x.dtype} on the device of the "
                         f"normalised tensor")
    if w.data_ptr() % 16:
        raise ValueError(f"{who}: {name} must be 16-byte aligned")


def _qk_eps(eps, who: str) -> float:
    eps = float(eps)
    if not math.isfinite(eps) or eps < 0.0:
        raise ValueError(f"{who}: eps must be finite and not negative, got {eps}")
    return eps


def qk_norm_rotary(x, weight, cos, sin, positions, *, eps: float = 1e-6, interleaved: bool = False, out=None) -> torch.Tensor:
    """QK-norm and rotary position embedding of x in one pass (mio_qknorm_rope_rows): every head row of x is RMS-normalised
    over head_dim -- n = x * rsqrt(mean(x^2) + eps) * weight in fp32, the mean over the whole head_dim, not over rot_dim --
    then the first rot_dim elements of n are rotated as apply_rotary rotates and the result is rounded once (nothing is
    rounded between the norm and the rotation).  x, cos, sin, positions, interleaved and out as apply_rotary (out may be x);
    weight [head_dim] in x's dtype, on x's device, contiguous, shared by all heads (q_norm.weight for q, k_norm.weight for k).
    Gemma's (1 + w) form is the caller's concern: pass 1 + w.  A zero row gives zeros, a NaN in a head makes that head NaN, a
    position outside [0, max_position) gives a row of zeros."""
    who = "qk_norm_rotary"
    eps = _qk_eps(eps, who)
    if not isinstance(weight, torch.Tensor):
        raise ValueError(f"{who}: weight must be a [head_dim] tensor")
    r = _rotary_rows_args(who, x, cos, sin, positions, interleaved, out, weight)
    check(lib.mio_qknorm_rope_rows(*r.head, *r.strides, *r.sizes, eps, _stream()))
    return r.res


def rope_and_cache_varlen(q, key, value, k_cache, v_cache, block_tables, cu_seqlens_new, context_lengths,
                          block_size: int, layer_idx: int, cos, sin, *, positions=None, interleaved: bool = False,
                          q_out=None, k_scale=None, v_scale=None) -> torch.Tensor:
    """reshape_and_cache_varlen with rotary position embedding fused in (mio_rope_and_cache_varlen / _kv8): K is rotated on
    its way into the paged cache (rounded once, straight into the cache's format: 16 bits, or e4m3 of rot(k) / k_scale for a
    float8_e4m3fn cache), V and K's elements past rot_dim are written exactly as reshape_and_cache_varlen writes them, and
    the token's query heads q [total_new, H, D] are rotated into q_out (returned; q's shape, may be q itself; allocated when
    None).  cos / sin as apply_rotary.  A token's position is its cache position context_lengths[b] - n_b + i, or
    positions[t] (int32 [total_new]) where given -- the cache row does not depend on it.  A token outside every sequence, or
    whose position is outside [0, max_position), writes nothing to the caches and gets a q_out row of zeros.  Queued on the
    current stream with no host sync (graph-capturable)."""
    r = _rope_cache_args("rope_and_cache_varlen", q, key, value, k_cache, v_cache, block_tables, cu_seqlens_new,
                         context_lengths, block_size, layer_idx, cos, sin, positions, interleaved, q_out, k_scale, v_scale)
    fn = lib.mio_rope_and_cache_varlen_kv8 if r.kv8 else lib.mio_rope_and_cache_varlen
    check(fn(*r.head, *r.strides, *r.sizes, _stream()))
    return r.q_out


def _rope_cache_args(who, q, key, value, k_cache, v_cache, block_tables, cu_seqlens_new, context_lengths, block_size,
                     layer_idx, cos, sin, positions, interleaved, q_out, k_scale, v_scale, weights=()):
    """The argument checks of the rotating cache writes (rope_and_cache_varlen, qknorm_rope_and_cache_varlen: weights = the two
    norm weights) and what they pass to the library: head (q .. sin[, q_weight, k_weight] addresses), strides (q, q_out, k, v),
    sizes (B .. dtype), kv8, q_out and keep (the tensors the addresses point into)."""
    _need_cuda(q, key, value, k_cache, v_cache, block_tables, cu_seqlens_new, context_lengths, cos, sin, positions, q_out,
               *weights)
    w = _cache_write_args(key, value, k_cache, v_cache, block_tables, context_lengths, block_size, layer_idx, k_scale,
                          v_scale, who, cu_seqlens_new, q)
    for name, t in zip(("q_weight", "k_weight"), weights):
        _qk_weight_ok(t, key, name, who)
    T, D = w.T, w.D
    max_position, rot_dim = _rope_tables_ok(cos, sin, D, w.kv8, interleaved, key.device, who)
    if positions is not None:
        _i32_dev(positions, "positions", 1, "of total_new positions", key.device)
        if positions.numel() != T:
            raise ValueError(f"positions must hold total_new = {T} entries, got {positions.numel()}")
    if q_out is None:
        q_out = torch.empty(q.shape, dtype=q.dtype, device=q.device)
    elif q_out.shape != q.shape or q_out.dtype != q.dtype or q_out.device != q.device:
        raise ValueError(f"{who}: q_out must have q's shape, dtype and device")
    elif q_out.stride(-1) != 1 or any(s % 8 for s in q_out.stride()[:-1]) or q_out.data_ptr() % 16:
        raise ValueError(f"{who}: q_out needs a contiguous last dim, strides that are multiples of 8 and 16-byte alignment")
    q = _rows16(q)
    qs = (C.c_int64 * 2)(q.stride(0), q.stride(1))
    os_ = (C.c_int64 * 2)(q_out.stride(0), q_out.stride(1))
    head = (q.data_ptr(), q_out.data_ptr(), *w.data, *w.tables, _ptr(positions), cos.data_ptr(), sin.data_ptr(),
            *(t.data_ptr() for t in weights))
    return types.SimpleNamespace(
        head=head, strides=(qs, os_, *w.strides), kv8=w.kv8, q_out=q_out, keep=(q, w.keep),
        sizes=(w.B, T, q.shape[1], w.Hkv, D, rot_dim, max_position, int(bool(interleaved)), *w.geom, w.dt))


def qknorm_rope_and_cache_varlen(q, key, value, k_cache, v_cache, block_tables, cu_seqlens_new, context_lengths,
                                 block_size: int, layer_idx: int, cos, sin, q_weight, k_weight, *, eps: float = 1e-6,
                                 positions=None, interleaved: bool = False, q_out=None, k_scale=None,
                                 v_scale=None) -> torch.Tensor:
    """rope_and_cache_varlen with QK-norm fused in (mio_qknorm_rope_and_cache_varlen / _kv8): every query head of q and every
    key head of key is RMS-normalised over head_dim -- n = x * rsqrt(mean(x^2) + eps) * weight in fp32, the mean over the
    whole head_dim, not over rot_dim; q_weight / k_weight [head_dim] in q's dtype, contiguous, shared by all heads of their
    kind -- then rotated as rope_and_cache_varlen rotates and rounded ONCE into the stored format: q into q_out (returned;
    may be q; allocated when None), K into the paged cache (16 bits, or e4m3 of y / k_scale for a float8_e4m3fn cache).
    Nothing is rounded between the norm and the rotation.  V is untouched: its bytes are reshape_and_cache_varlen's.  Every
    other argument, the token placement and the skipping rules as rope_and_cache_varlen: a token outside every sequence, or
    whose position is outside [0, max_position), writes nothing to the caches and gets a q_out row of zeros.  q_out is
    bit-equal to qk_norm_rotary(q, q_weight, ...).  Gemma's (1 + w) form is the caller's concern: pass 1 + w.  A zero row
    gives zeros; a NaN in a head makes that head NaN.  Queued on the current stream with no host sync (graph-capturable)."""
    who = "qknorm_rope_and_cache_varlen"
    eps = _qk_eps(eps, who)
    for name, t in (("q_weight", q_weight), ("k_weight", k_weight)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{who}: {name} must be a [head_dim] tensor")
    r = _rope_cache_args(who, q, key, value, k_cache, v_cache, block_tables, cu_seqlens_new, context_lengths, block_size,
                         layer_idx, cos, sin, positions, interleaved, q_out, k_scale, v_scale, (q_weight, k_weight))
    fn = lib.mio_qknorm_rope_and_cache_varlen_kv8 if r.kv8 else lib.mio_qknorm_rope_and_cache_varlen
    check(fn(*r.head, *r.strides, *r.sizes, eps, _stream()))
    return r.q_out


# ------------------------------------------------------------------------------------------------
# token sampling
# ------------------------------------------------------------------------------------------------
SAMPLE_MAX_VOCAB = 1 << 20
_SAMPLE_DTYPES = {torch.bfloat16: _lib.MIO_BF16, torch.float16: _lib.MIO_FP16, torch.float32: _lib.MIO_FP32}


def _sample_param(v, B: int, dtype: torch.dtype, name: str, who: str, device, required: bool = False):
    """A per-row parameter as a device tensor [B] of dtype: a tensor is checked, a Python scalar is broadcast with torch.full
    (no synchronisation), None stays None (the filter is off for every row)."""
    if v is None:
        if required:
            raise ValueError(f"{who}: {name} is required")
        return None
    if isinstance(v, torch.Tensor):
        if not v.is_cuda:
            raise ValueError("HIP kernels require input tensors to be on a CUDA (ROCm) device.")
        if v.dtype != dtype or v.dim() != 1 or v.numel() != B or not v.is_contiguous():
            raise ValueError(f"{who}: {name} must be a contiguous {dtype} tensor of {B} elements, got {v.dtype} "
                             f"{tuple(v.shape)}")
        return v
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise ValueError(f"{who}: {name} must be a number or a tensor, got {type(v).__name__}")
    if dtype == torch.int32:
        if isinstance(v, float) and v != int(v):
            raise ValueError(f"{who}: {name} must be an integer, got {v}")
        v = max(-1, min(int(v), 2 ** 31 - 1))
    return torch.full((B,), v, dtype=dtype, device=device)


def _sample(who: str, logits, temperature, top_k, top_p, min_p, u, generator, tokens: bool, kept: bool, probs: bool):
    if not isinstance(logits, torch.Tensor):
        raise ValueError(f"{who}: logits must be a tensor")
    _need_cuda(logits)
    if logits.dtype not in _SAMPLE_DTYPES:
        raise ValueError(f"{who}: logits must be bf16, fp16 or fp32, got {logits.dtype}")
    if logits.dim() < 1:
        raise ValueError(f"{who}: logits must be [..., V]")
    V = logits.shape[-1]
    if not 1 <= V <= SAMPLE_MAX_VOCAB:
        raise ValueError(f"{who}: the vocabulary must be 1 .. {SAMPLE_MAX_VOCAB} tokens, got {V}")
    if logits.stride(-1) != 1 and V > 1:
        raise ValueError(f"{who}: logits must have last-dim stride 1")
    lead = logits.shape[:-1]
    x = logits if logits.dim() == 2 else logits.reshape(-1, V)
    if x.stride(-1) != 1 and V > 1:
        x = x.contiguous()
    B = x.shape[0]
    ld = x.stride(0) if B > 1 else V
    if ld < V or x.data_ptr() % 16:
        x = x.contiguous()
        ld = V
    dev = x.device
    T = _sample_param(temperature, B, torch.float32, "temperature", who, dev, required=True)
    k = _sample_param(top_k, B, torch.int32, "top_k", who, dev)
    p = _sample_param(top_p, B, torch.float32, "top_p", who, dev)
    q = _sample_param(min_p, B, torch.float32, "min_p", who, dev)
    if tokens:
        if u is None:
            u = torch.rand(B, generator=generator, device=dev, dtype=torch.float32)
        elif generator is not None:
            raise ValueError(f"{who}: give u or generator, not both")
        else:
            u = _sample_param(u, B, torch.float32, "u", who, dev)
    tok = torch.empty(B, dtype=torch.int64, device=dev) if tokens else None
    kep = torch.empty(B, dtype=torch.int32, device=dev) if kept else None
    pr = torch.empty(B, V, dtype=torch.float32, device=dev) if probs else None
    if B > 0:  # an empty batch has no addresses to hand over
        check(lib.mio_sample_tokens(x.data_ptr(), ld, T.data_ptr(), _ptr(k), _ptr(p), _ptr(q), _ptr(u) if tokens else None,
                                    _ptr(tok), _ptr(kep), _ptr(pr), V, B, V, _SAMPLE_DTYPES[x.dtype], _stream()))
    return (None if tok is None else tok.view(lead), None if kep is None else kep.view(lead),
            None if pr is None else pr.view(*lead, V))


def sample_tokens(logits, temperature, top_k=None, top_p=None, min_p=None, *, u=None, generator=None,
                  return_kept: bool = False, return_probs: bool = False):
    """One token id per row of logits [B, V] (or [..., V], flattened; bf16, fp16 or fp32, last-dim stride 1) in one launch
    (mio_sample_tokens; the semantics are stated in include/mio_hip.h): greedy where temperature <= 0, else temperature
    sampling restricted by top-k, then top-p over the renormalised top-k set, then min-p, drawn with the uniform u[b] in
    [0, 1) by an index-ordered CDF search.  Ties are ordered by token index; a NaN logit counts as -inf.

    temperature, top_p, min_p, u: fp32 device tensors [B] or Python scalars; top_k: int32 [B] or an int.  A scalar becomes a
    device tensor with torch.full, a None filter is off; nothing synchronises, so the call can be captured in a graph (pass
    tensors then, and update them in place: see mio.sampling.Sampler).  u=None draws torch.rand(B, generator=generator) on the
    device.  Returns tokens (int64, logits.shape[:-1]; -1 for a row with no finite logit), followed by kept (int32, the size
    of the filtered set) when return_kept and probs (fp32 [..., V], the filtered distribution, exactly 0 outside the kept
    set) when return_probs.  ValueError for CPU tensors, wrong dtypes or shapes, a strided last dim; RuntimeError with the
    library's message on a refusal."""
    tok, kep, pr = _sample("sample_tokens", logits, temperature, top_k, top_p, min_p, u, generator, True, bool(return_kept),
                           bool(return_probs))
    if not return_kept and not return_probs:
        return tok
    return (tok,) + ((kep,) if return_kept else ()) + ((pr,) if return_probs else ())


def sampling_probs(logits, temperature, top_k=None, top_p=None, min_p=None):
    """The filtered distribution sample_tokens draws from, fp32 [..., V]: w_i / Z on the kept set, exactly 0 elsewhere, one-hot
    on a greedy row, all zero on a row with no finite logit.  The arguments of sample_tokens without u: nothing is drawn."""
    return _sample("sampling_probs", logits, temperature, top_k, top_p, min_p, None, None, False, False, True)[2]


# ------------------------------------------------------------------------------------------------
# mixture-of-experts MLP for decode steps: router, grouped up projection, grouped down projection + combine
# ------------------------------------------------------------------------------------------------
MOE_MAX_TOKENS, MOE_MAX_EXPERTS, MOE_MAX_TOP_K = 64, 256, 8


class MoERoute(NamedTuple):
    """What moe_route decides, all device tensors (semantics: include/mio_hip.h): ids int32 [T, k] and weights fp32 [T, k] per
    token; expert_offsets int32 [E + 1], sorted_rows int32 [T k] and row_pos int32 [T k], the routed rows r = t k + j grouped by
    expert in ascending r and the inverse of that permutation."""
    ids: torch.Tensor
    weights: torch.Tensor
    expert_offsets: torch.Tensor
    sorted_rows: torch.Tensor
    row_pos: torch.Tensor
    top_k: int
    num_experts: int


def _moe_route_ok(route, who: str, device) -> Tuple[int, int, int]:
    """(T, k, E) of a MoERoute whose tensors are what the kernels take from raw pointers."""
    if not isinstance(route, MoERoute):
        raise ValueError(f"{who}: route must be a MoERoute (ops.moe_route)")
    T, k, E = route.ids.shape[0], route.top_k, route.num_experts
    want = (("ids", route.ids, torch.int32, (T, k)), ("weights", route.weights, torch.float32, (T, k)),
            ("expert_offsets", route.expert_offsets, torch.int32, (E + 1,)), ("sorted_rows", route.sorted_rows, torch.int32, (T * k,)),
            ("row_pos", route.row_pos, torch.int32, (T * k,)))
    for name, t, dtype, shape in want:
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != device:
            raise ValueError(f"{who}: route.{name} must be a tensor on the activations' device")
        if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"{who}: route.{name} must be a contiguous {dtype} tensor of shape {shape}, got {t.dtype} {tuple(t.shape)}")
    return T, k, E


def moe_route(router_logits, top_k: int, renormalize: bool = True, out: Optional[MoERoute] = None) -> MoERoute:
    """Route T <= 64 tokens over E <= 256 experts in one launch (mio_moe_route): router_logits [T, E] (or [..., E], flattened; bf16,
    fp16 or fp32, last-dim stride 1) -> the top_k experts of every token in the sampler's order (ties to the lowest index, NaN as
    -inf), their softmax-over-all-experts weights (renormalize: divided by their sum), and the routed rows grouped by expert.
    out: a MoERoute of the same (T, top_k, E) to write into (a captured step reuses its buffers).  T == 0 launches nothing and
    zeroes expert_offsets (out's too).  Nothing is read back to the host."""
    who = "moe_route"
    if not isinstance(router_logits, torch.Tensor):
        raise ValueError(f"{who}: router_logits must be a tensor")
    _need_cuda(router_logits)
    if router_logits.dtype not in _SAMPLE_DTYPES:
        raise ValueError(f"{who}: router_logits must be bf16, fp16 or fp32, got {router_logits.dtype}")
    if router_logits.dim() < 1:
        raise ValueError(f"{who}: router_logits must be [..., E]")
    E = router_logits.shape[-1]
    k = operator.index(top_k)
    if not 1 <= E <= MOE_MAX_EXPERTS:
        raise ValueError(f"{who}: 1 .. {MOE_MAX_EXPERTS} experts, got {E}")
    if not 1 <= k <= min(E, MOE_MAX_TOP_K):
        raise ValueError(f"{who}: top_k must be in [1, min(E, {MOE_MAX_TOP_K})], got {k}")
    x = router_logits if router_logits.dim() == 2 else router_logits.reshape(-1, E)
    if x.stride(-1) != 1 and E > 1:
        x = x.contiguous()
    T = x.shape[0]
    if T > MOE_MAX_TOKENS:
        raise ValueError(f"{who} takes at most {MOE_MAX_TOKENS} tokens (decode steps only), got {T}")
    ld = x.stride(0) if T > 1 else E
    if ld < E or x.data_ptr() % 16:
        x, ld = x.contiguous(), E
        if x.data_ptr() % 16:  # (already contiguous at a storage offset off 16 bytes: contiguous() returned it as it was)
            x = x.clone()
    dev = x.device
    if out is None:
        i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)  # noqa: E731
        out = MoERoute(i32(T, k), torch.empty(T, k, dtype=torch.float32, device=dev), i32(E + 1), i32(T * k), i32(T * k), k, E)
    elif _moe_route_ok(out, who, dev) != (T, k, E):
        raise ValueError(f"{who}: out was made for another (T, top_k, E)")
    if T == 0:  # (nothing is launched: the offsets of an empty routing are zeros, in the caller's buffer as in ours)
        out.expert_offsets.zero_()
    else:
        check(lib.mio_moe_route(x.data_ptr(), ld, out.ids.data_ptr(), out.weights.data_ptr(), out.expert_offsets.data_ptr(),
                                out.sorted_rows.data_ptr(), out.row_pos.data_ptr(), T, E, k, 1 if renormalize else 0,
                                _SAMPLE_DTYPES[x.dtype], _stream()))
    return out


def _moe_act(activation: str) -> int:
    if activation not in _ACT:
        raise ValueError(f"Unsupported activation function: {activation}")
    return _ACT[activation]


def moe_up_splits(T: int, top_k: int, E: int, I: int, d: int, activation: str = "swiglu") -> int:
    """The slices of K = d a moe_up call of this shape runs (1: one launch, no workspace).  Host-only; ValueError where the call
    would be refused."""
    n = lib.mio_moe_up_splits(T, top_k, E, I, d, _moe_act(activation))
    if n < 0:
        raise ValueError(lib.mio_last_error().decode("utf-8", "replace"))
    return n


def moe_down_splits(T: int, top_k: int, E: int, d: int, I: int) -> int:
    """The slices of K = I a moe_down call of this shape runs.  Host-only; ValueError where the call would be refused."""
    n = lib.mio_moe_down_splits(T, top_k, E, d, I)
    if n < 0:
        raise ValueError(lib.mio_last_error().decode("utf-8", "replace"))
    return n


def _moe_weight(w, E: int, dtype, name: str, who: str, like=None) -> torch.Tensor:
    """A stacked expert weight [E, N, K] as the kernels take it: last-dim stride 1, row and expert strides multiples of 8, 16-byte
    aligned (a copy otherwise); like: the weight it must share shape and strides with (the SwiGLU gate and up)."""
    if not isinstance(w, torch.Tensor) or w.dim() != 3 or w.shape[0] != E:
        raise ValueError(f"{who}: {name} must be a stacked expert weight [E = {E}, N, K]")
    _need_cuda(w)
    if w.dtype != dtype:
        raise ValueError(f"{who}: {name} must have the activation dtype {dtype}, got {w.dtype}")
    N, K = w.shape[1:]
    ok = (w.stride(2) == 1 and w.stride(1) % 8 == 0 and w.stride(1) >= K and w.stride(0) % 8 == 0
          and w.stride(0) >= (N - 1) * w.stride(1) + K and w.data_ptr() % 16 == 0)
    if not ok or (like is not None and w.stride() != like.stride()):
        w = w.contiguous()
    return w


def _moe_bias(b, E: int, N: int, dtype, name: str, who: str):
    if b is None:
        return None
    _need_cuda(b)
    if b.dtype != dtype or tuple(b.shape) != (E, N):
        raise ValueError(f"{who}: {name} must be a {dtype} tensor of shape ({E}, {N}), got {b.dtype} {tuple(b.shape)}")
    return b if b.is_contiguous() and b.data_ptr() % 16 == 0 else b.contiguous().clone()


def _pad8(n: int) -> int:
    return (n + 7) // 8 * 8


def _ld(t: torch.Tensor, n: int) -> int:
    """The row stride of t [rows, n] as the launch takes it (a single row has no stride to speak of)."""
    return t.stride(0) if t.shape[0] > 1 else _pad8(n)


def moe_up(x, route: MoERoute, w_up, act: str = "swiglu", w_gate=None, b_up=None, b_gate=None, out=None):
    """The grouped up projection (mio_moe_up): x [T, d], w_up (and w_gate for swiglu) [E, I, d] -> h [T k, I] BY SORTED POSITION:
    row p is act(x[t] w_up[e]^T + b_up[e]) (swiglu: silu(x[t] w_gate[e]^T + b_gate[e]) * that) for the expert e and the token
    t = sorted_rows[p] // k of position p.  One launch over all experts (two when the plan splits K); experts without a routed
    row are not read.  out: h to write into, [T k, I], row stride a multiple of 8."""
    who = "moe_up"
    _need_cuda(x)
    a = _moe_act(act)
    dt = _dtype_id(x)
    if x.dim() != 2:
        raise ValueError(f"{who}: x must be [T, d], got {tuple(x.shape)}")
    T, k, E = _moe_route_ok(route, who, x.device)
    if x.shape[0] != T:
        raise ValueError(f"{who}: x has {x.shape[0]} rows, the route {T} tokens")
    glu = a == _lib.ACT_SWIGLU
    if glu != (w_gate is not None):
        raise ValueError("SwiGLU activation requires gate weights" if glu else f"{who}: w_gate belongs to act='swiglu'")
    w = _moe_weight(w_up, E, x.dtype, "w_up", who)
    I, d = w.shape[1:]
    if x.shape[1] != d:
        raise ValueError(f"{who}: weight shape {tuple(w.shape)} does not match input features {x.shape[1]}")
    g = None
    if glu:
        if w_gate.shape != w_up.shape:
            raise ValueError(f"{who}: w_gate must have w_up's shape")
        g = _moe_weight(w_gate, E, x.dtype, "w_gate", who, like=w)
        if g.stride() != w.stride():
            w = w.contiguous()
    bu = _moe_bias(b_up, E, I, x.dtype, "b_up", who)
    bg = _moe_bias(b_gate, E, I, x.dtype, "b_gate", who) if glu else None
    x2 = _rows16(x)
    if out is None:
        out = torch.empty(T * k, _pad8(I), dtype=x.dtype, device=x.device)[:, :I]
    elif tuple(out.shape) != (T * k, I) or out.dtype != x.dtype or (I > 1 and out.stride(1) != 1) or out.stride(0) % 8:
        raise ValueError(f"{who}: out must be [{T * k}, {I}] {x.dtype} with a row stride that is a multiple of 8")
    if T == 0:
        return out
    nbytes = lib.mio_moe_up_workspace_bytes(T, k, E, I, d, a)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device) if nbytes else None
    check(lib.mio_moe_up(x2.data_ptr(), w.data_ptr(), _ptr(bu), _ptr(g), _ptr(bg), route.expert_offsets.data_ptr(),
                         route.sorted_rows.data_ptr(), out.data_ptr(), _ptr(ws), T, k, E, I, d, _ld(x2, d), w.stride(1), w.stride(0),
                         _ld(out, I), a, dt, _stream()))
    return out


def moe_down(h, route: MoERoute, w_down, b_down=None, residual=None, out=None):
    """The grouped down projection and the combine (mio_moe_down): h [T k, I] by sorted position (moe_up's output), w_down
    [E, d, I] -> y [T, d] = sum_j weights[t, j] (h[row_pos[t k + j]] w_down[e]^T + b_down[e]) (+ residual[t]), e = ids[t, j]: the
    slots summed in fp32 in slot order and rounded once.  residual [T, d] is also where a shared expert's output goes in."""
    who = "moe_down"
    _need_cuda(h)
    dt = _dtype_id(h)
    T, k, E = _moe_route_ok(route, who, h.device)
    if h.dim() != 2 or h.shape[0] != T * k:
        raise ValueError(f"{who}: h must be [T k = {T * k}, I], got {tuple(h.shape)}")
    w = _moe_weight(w_down, E, h.dtype, "w_down", who)
    d, I = w.shape[1:]
    if h.shape[1] != I:
        raise ValueError(f"{who}: weight shape {tuple(w.shape)} does not match h's {h.shape[1]} features")
    bd = _moe_bias(b_down, E, d, h.dtype, "b_down", who)
    h2 = _rows16(h)
    _res_ok(residual, T * d, h.dtype)
    r2 = None if residual is None else _rows16(residual.reshape(T, d))
    if r2 is not None and T > 1 and r2.stride(0) % 8:  # (d % 8 != 0, contiguous: rows at the stride the kernel's loads are laid out for)
        r2 = torch.empty(T, _pad8(d), dtype=h.dtype, device=h.device)[:, :d].copy_(r2)
    if out is None:
        out = torch.empty(T, _pad8(d), dtype=h.dtype, device=h.device)[:, :d]
    elif tuple(out.shape) != (T, d) or out.dtype != h.dtype or (d > 1 and out.stride(1) != 1) or out.stride(0) % 8:
        raise ValueError(f"{who}: out must be [{T}, {d}] {h.dtype} with a row stride that is a multiple of 8")
    if T == 0:
        return out
    nbytes = lib.mio_moe_down_workspace_bytes(T, k, E, d, I)
    ws = torch.empty(max(nbytes // 4, 4), dtype=torch.float32, device=h.device)
    check(lib.mio_moe_down(h2.data_ptr(), w.data_ptr(), _ptr(bd), route.ids.data_ptr(), route.weights.data_ptr(),
                           route.expert_offsets.data_ptr(), route.row_pos.data_ptr(), _ptr(r2), out.data_ptr(), ws.data_ptr(), T, k, E, d,
                           I, _ld(h2, I), w.stride(1), w.stride(0), _ld(out, d), 0 if r2 is None else _ld(r2, d), dt, _stream()))
    return out


def moe_mlp(x, route: MoERoute, w_up, w_down, act: str = "swiglu", w_gate=None, b_up=None, b_gate=None, b_down=None,
            residual=None, out=None):
    """The experts' MLP of a decode step under a routing: moe_up, then moe_down.  x [T, d] (T <= 64), w_up / w_gate [E, I, d],
    w_down [E, d, I], biases [E, I] / [E, d].  h and both workspaces come from torch's allocator; nothing synchronises, so the
    call can be captured in a graph."""
    return moe_down(moe_up(x, route, w_up, act, w_gate, b_up, b_gate), route, w_down, b_down, residual, out)


# ------------------------------------------------------------------------------------------------
# composed entry points: QKV projection + attention + out-projection, LayerNorm + QKV projection
# ------------------------------------------------------------------------------------------------
def fused_attention(hidden_states: torch.Tensor, qkv_weight: torch.Tensor, qkv_bias: Optional[torch.Tensor],
                    out_weight: torch.Tensor, out_bias: Optional[torch.Tensor], mask: Optional[torch.Tensor] = None,
                    causal: bool = False, num_heads: int = 8, head_dim: Optional[int] = None, dropout_p: float = 0.0,
                    softmax_scale: Optional[float] = None, block_size: int = 128) -> torch.Tensor:
    """Drop-in for triton_fused_attention (flash_attention_kernels.py:1361-1530): hidden [B,S,d],
    qkv_weight [3d,d], out_weight [d,d].  Three launches (QKV GEMM, tiled attention reading q/k/v as strided views
    of the QKV result, out-projection GEMM); nothing is copied in between."""
    if hidden_states.dim() != 3:
        raise ValueError(f"Expected 3D input tensor, got shape: {hidden_states.shape}")
    B, S, d = hidden_states.shape
    D = head_dim if head_dim is not None else d // num_heads
    if num_heads * D != d or qkv_weight.shape[0] != 3 * d:
        raise ValueError(f"hidden_size {d} does not match num_heads {num_heads} x head_dim {D} / qkv_weight "
                         f"{tuple(qkv_weight.shape)}")
    qkv = gemm_bias_act(hidden_states, qkv_weight, qkv_bias).view(B, S, 3, num_heads, D)
    ctx = flash_attention(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], mask=mask, causal=causal,
                          softmax_scale=softmax_scale, dropout_p=dropout_p, block_size=block_size)
    return gemm_bias_act(ctx.view(B, S, d), out_weight, out_bias)


def _infer_heads(hidden_size: int, num_heads: int) -> int:
    if num_heads:
        return num_heads
    for hs in (64, 80, 128):  # fused_layernorm_qkv.py:653-663
        if hidden_size % hs == 0:
            return hidden_size // hs
    return max(1, hidden_size // 64)


def fused_layernorm_qkv(hidden_states, layernorm_weight, layernorm_bias, query_weight, key_weight, value_weight,
                        query_bias=None, key_bias=None, value_bias=None, eps: float = 1e-5, num_heads: int = 0,
                        num_kv_heads: Optional[int] = None):
    """Drop-in for triton_fused_layernorm_qkv / pytorch_fused_layernorm_qkv (fused_layernorm_qkv.py:422-700):
    returns (q [B,S,H,Dh], k [B,S,Hkv,Dkv], v [B,S,Hkv,Dkv]).

    Two kernel kinds: the row-wise LayerNorm (HBM-bound, ~3 % of a layer at the benchmark shape) and the MFMA GEMM
    whose operand tiles are moved global -> LDS by DMA; normalising inside that GEMM would put every activation
    tile through registers and the vector ALU, which costs the matrix pipeline more than the one [B,S,d] round
    trip it saves."""
    if hidden_states.dim() != 3:
        raise ValueError(f"Expected 3D input tensor, got shape: {hidden_states.shape}")
    B, S, d = hidden_states.shape
    H = _infer_heads(d, num_heads)
    Hkv = H if num_kv_heads is None else num_kv_heads
    xn = layernorm(hidden_states, layernorm_weight, layernorm_bias, eps)
    q = gemm_bias_act(xn, query_weight, query_bias)
    k = gemm_bias_act(xn, key_weight, key_bias)
    v = gemm_bias_act(xn, value_weight, value_bias)
    return (q.view(B, S, H, q.shape[-1] // H), k.view(B, S, Hkv, k.shape[-1] // Hkv),
            v.view(B, S, Hkv, v.shape[-1] // Hkv))


def flash_compatible_wrapper(hidden_states, layernorm_weight, layernorm_bias, qkv_weight, qkv_bias=None,
                             eps: float = 1e-5, num_heads: int = 0, num_kv_heads: Optional[int] = None):
    """fused_layernorm_qkv.py:1073-1116: combined [3d,d] QKV weight -> ONE GEMM; q/k/v are strided views of it."""
    if hidden_states.dim() != 3:
        raise ValueError(f"Expected 3D input tensor, got shape: {hidden_states.shape}")
    B, S, d = hidden_states.shape
    H = _infer_heads(d, num_heads)
    Hkv = H if num_kv_heads is None else num_kv_heads
    xn = layernorm(hidden_states, layernorm_weight, layernorm_bias, eps)
    qkv = gemm_bias_act(xn, qkv_weight, qkv_bias)
    q, k, v = qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:]
    return q.view(B, S, H, d // H), k.view(B, S, Hkv, d // Hkv), v.view(B, S, Hkv, d // Hkv)


def ring_compatible_wrapper(hidden_states, layernorm_weight, layernorm_bias, q_weight, k_weight, v_weight,
                            q_bias=None, k_bias=None, v_bias=None, eps: float = 1e-5, num_heads: int = 0,
                            num_kv_heads: Optional[int] = None):
    """fused_layernorm_qkv.py:1118-1161: as fused_layernorm_qkv, head-major [B,H,S,Dh] views for ring attention."""
    q, k, v = fused_layernorm_qkv(hidden_states, layernorm_weight, layernorm_bias, q_weight, k_weight, v_weight,
                                  q_bias, k_bias, v_bias, eps, num_heads, num_kv_heads)
    return q.permute(0, 2, 1, 3), k.permute(0, 2, 1, 3), v.permute(0, 2, 1, 3)


# reference-name aliases (drop-in for code written against the Triton wrappers)
triton_flash_attention = flash_attention
triton_ring_attention_forward = ring_attention_forward
triton_fused_mlp = fused_mlp
triton_layernorm = layernorm
triton_paged_attention_forward = paged_attention_forward
triton_reshape_and_cache = reshape_and_cache
triton_fused_attention = fused_attention
triton_fused_layernorm_qkv = fused_layernorm_qkv

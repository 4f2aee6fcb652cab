"""FlashAttention-3 operator surface on the HIP kernels.

Mirrors reference kernels/attention/flash_attention.py: FlashAttentionConfig (:53-104),
FlashAttention3 (:107-471), FlashAttentionLayer (:474-659), FlashSelfAttention (:662-949),
ModelConverter (:952-1168) -- same constructor/forward signatures, parameter names and error
behaviour.  The reference module cannot be imported and its PyTorch body returns
zeros (F4); the semantics implemented here are the ones its kernel math and self-checks define:
exact softmax attention, causal / keep-mask fill of -1e9, output cast back to the input dtype.
One launch of mio_fa3_fwd per call; the projections run on the MFMA GEMM.  No PyTorch path.
"""
from __future__ import annotations

import copy
from dataclasses import dataclass
from typing import Any, Optional, Set, Tuple, Union

import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import ops
from ..._nn import (CastCache, ResidualStream, apply_norm, as_dtype, attention_plan, compute_dtype, decode_route, folded_linear,
                    linear, prenorm_linear, residual_linear, routed_linear, stream_preconditions)


@dataclass
class FlashAttentionConfig:
    """Fields as reference flash_attention.py:53-80."""
    block_size: int = 128
    causal: bool = False
    softmax_scale: Optional[float] = None
    dropout_p: float = 0.0
    return_softmax: bool = False
    use_triton: bool = True        # kept for signature compatibility; the HIP kernel is always used
    memory_efficient: bool = True
    precision: str = "fp16"
    normalize_query: bool = False
    fp8_ortho_matrix: Optional[torch.Tensor] = None
    # sliding window (flash-attn's window_size = (left, right), -1 = unbounded): prefill through ops.flash_attention,
    # decode through ops.paged_attention_forward with (left, -1); windowed modules take the plain attention path
    window_size: Tuple[int, int] = (-1, -1)
    # rotary position embedding in FlashAttentionLayer / FlashSelfAttention: the first rotary_dim elements of every q and k head
    # are rotated (0: off, the layers run exactly as without these fields); the plain schedule base ** (-2 i / rotary_dim) over
    # positions [0, max_position); neox pairing, or GPT-J's with rotary_interleaved.  A position outside the table gives a zero row.
    rotary_dim: int = 0
    rotary_base: float = 10000.0
    rotary_interleaved: bool = False
    max_position: int = 8192
    # decode steps (the paged branch, "block_tables" in kwargs): the q / qkv projection and o_proj run on the decode-step GEMM
    # (ops.gemm_skinny) where ops.gemm_skinny_ok advises it; off: every call as before
    decode_gemm: bool = False
    # the same calls on weight-only FP8 copies of the weights (e4m3fn bytes, one fp32 scale per output channel, quantised once
    # per parameter version; ops.gemm_skinny_w8) where ops.gemm_skinny_w8_ok advises it; a call it does not advise runs as
    # decode_gemm says.  Activations, the output and every other call stay 16-bit: a storage form, not precision="fp8".
    decode_gemm_fp8: bool = False
    # QK-norm (Qwen3, Gemma 3): every q and k head is RMS-normalised over head_dim with a learned [head_dim] weight
    # (q_norm.weight / k_norm.weight, ones at construction) between the projection and the rotation, fused into the rotation
    # (ops.qk_norm_rotary) and rounded once.  Needs rotary_dim > 0; off: no new submodules, the layers run exactly as before.
    # Gemma's (1 + w) form: store 1 + w in the weights.
    qk_norm: bool = False
    qk_norm_eps: float = 1e-6

    @property
    def allowed_precisions(self) -> Set[str]:
        return {"fp16", "bf16", "fp32", "fp8"}

    def __post_init__(self):
        if self.precision not in self.allowed_precisions:
            raise ValueError(f"Unsupported precision mode: {self.precision}. Allowed: {self.allowed_precisions}")
        if self.precision == "fp8":
            # the reference gates FP8 to Hopper (CC >= 9.0) and raises RuntimeError elsewhere (:89-100)
            raise RuntimeError("FP8 precision requires Hopper architecture in the reference and is not "
                               "implemented by the gfx950 HIP path.")


class FlashAttention3(nn.Module):
    """q/k/v [B,S,H,D] -> [B,S,H,D]  (reference :107-471)."""

    def __init__(self, config: Optional[FlashAttentionConfig] = None):
        super().__init__()
        self.config = config or FlashAttentionConfig()
        self.supports_backward = False  # inference kernels only

    def forward(self, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                mask: Optional[torch.Tensor] = None) -> Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]:
        if q.dim() != 4 or k.dim() != 4 or v.dim() != 4:
            raise ValueError(f"Expected 4D tensors for q, k, v but got shapes: q={q.shape}, k={k.shape}, v={v.shape}")
        if not q.is_cuda:
            raise ValueError("HIP kernels require input tensors to be on a CUDA (ROCm) device.")
        cfg = self.config
        _refuse(cfg, self.training)
        orig_dtype = q.dtype
        dt = compute_dtype(cfg.precision, q)
        if q.dtype != dt:
            q, k, v = q.to(dt), k.to(dt), v.to(dt)
        if cfg.normalize_query:
            q = F.normalize(q, dim=-1)
        out = ops.flash_attention(q, k, v, mask=mask, causal=cfg.causal, softmax_scale=cfg.softmax_scale,
                                  dropout_p=0.0, return_softmax=False, block_size=cfg.block_size,
                                  **_window_kw(cfg))
        return as_dtype(out, orig_dtype)


def _refuse(cfg, training: bool) -> None:
    """What no attention kernel of this package computes: the softmax matrix, dropout."""
    if cfg.return_softmax:
        raise NotImplementedError("return_softmax=True is not supported by the fused kernel")
    if training and cfg.dropout_p > 0.0:
        raise NotImplementedError("attention dropout (training) is not supported by the inference kernel")


def _window_kw(cfg) -> dict:
    """window_size for ops.flash_attention when the config sets one (nothing otherwise: the unwindowed call exactly)."""
    return {} if tuple(cfg.window_size) == (-1, -1) else {"window_size": tuple(cfg.window_size)}


def _decode_window_kw(cfg) -> dict:
    """The config's window for ops.paged_attention_forward: a decode row has no key right of itself (right -1)."""
    if tuple(cfg.window_size) == (-1, -1):
        return {}
    left, right = cfg.window_size
    return {"window_size": (left, -1 if right in (-1, 0) else right)}


def _windowed(cfg) -> bool:
    return tuple(cfg.window_size) != (-1, -1)


_PAGED_KEYS = ("physical_kv_cache_k", "physical_kv_cache_v", "block_tables", "context_lengths",
               "kv_cache_block_size", "max_seq_len", "layer_idx")


def _paged_args(kwargs, who: str):
    vals = [kwargs.get(k) for k in _PAGED_KEYS]
    if any(v is None for v in vals):
        raise ValueError(f"Missing required arguments for PagedAttention in {who} forward pass.")
    return vals


class _HeadNorm(nn.Module):
    """The learned weight [head_dim] of a per-head RMSNorm (q_norm / k_norm of a layer with qk_norm).  It only holds the
    parameter: the norm itself runs fused into the rotation (ops.qk_norm_rotary, ops.qknorm_rope_and_cache_varlen)."""

    def __init__(self, head_dim: int):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(head_dim))


class _AttentionBase(nn.Module):
    def _setup(self, hidden_size, num_attention_heads, config, num_kv_heads):
        self.hidden_size = hidden_size
        self.num_attention_heads = num_attention_heads
        self.num_kv_heads = num_kv_heads if num_kv_heads is not None else num_attention_heads
        self.head_dim = hidden_size // num_attention_heads
        self.config = config or FlashAttentionConfig()
        if hidden_size % num_attention_heads != 0:
            raise ValueError(f"hidden_size {hidden_size} must be divisible by num_attention_heads {num_attention_heads}")
        if hidden_size % self.num_kv_heads != 0:
            raise ValueError(f"hidden_size {hidden_size} must be divisible by num_kv_heads {self.num_kv_heads}")
        self._cast = CastCache()
        rd = self.config.rotary_dim
        if rd and (rd < 0 or rd % 16 != 0 or rd > self.head_dim):
            raise ValueError(f"rotary_dim must be 0 (off) or a multiple of 16 up to head_dim {self.head_dim}, got {rd}")
        self._rope_key, self._rope_tabs = None, None  # plain attributes: the tables are derived, not state
        if self.config.qk_norm and not rd:
            raise ValueError("qk_norm=True needs rotary_dim > 0: the norm is fused into the rotation, a norm-only path is not built")

    def _setup_qk_norm(self):
        """q_norm / k_norm ([head_dim] weights, ones) where the config asks for QK-norm; nothing otherwise.  Called after the
        projections are made, so their initialisation draws what it drew before."""
        if self.config.qk_norm:
            self.q_norm = _HeadNorm(self.head_dim)
            self.k_norm = _HeadNorm(self.head_dim)

    def _rope_tables(self, device):
        """(cos, sin) of the config's schedule on device: built once, and again when max_position (or the schedule) changes."""
        cfg = self.config
        key = (torch.device(device), int(cfg.max_position), int(cfg.rotary_dim), float(cfg.rotary_base))
        if self._rope_key != key:
            self._rope_tabs = ops.rope_tables(cfg.max_position, cfg.rotary_dim, cfg.rotary_base, device=device)
            self._rope_key = key
        return self._rope_tabs

    def _rotate(self, t, positions, norm=None):
        """t [B,S,heads,D] (a fresh projection result or a view of one) rotated in place at positions int32 [B,S] or [S]; with
        QK-norm on, normalised by `norm` (q_norm or k_norm: its weight in t's dtype, cast again when it changes) in the same
        pass."""
        cos, sin = self._rope_tables(t.device)
        if self.config.qk_norm:
            return ops.qk_norm_rotary(t, self._cast.get(norm.weight, t.dtype), cos, sin, positions,
                                      eps=self.config.qk_norm_eps, interleaved=self.config.rotary_interleaved, out=t)
        return ops.apply_rotary(t, cos, sin, positions, interleaved=self.config.rotary_interleaved, out=t)

    def _dense_positions(self, kwargs, S, device):
        """The dense path's positions: the position_ids kwarg ([B,S] or [S]), else 0 .. S-1."""
        ids = kwargs.get("position_ids")
        if ids is not None:
            return ids.to(device=device, dtype=torch.int32)
        if S > self.config.max_position:
            raise ValueError(f"sequence length {S} exceeds the rotary tables' max_position {self.config.max_position}")
        return torch.arange(S, dtype=torch.int32, device=device)

    def _paged(self, q2d, B, q_len, dt, kwargs, who, residual=None):
        """q [B,q_len,H*D] already projected; attention over the paged cache, then o_proj
        (reference :572-621: K/V are NOT recomputed, they are read from the cache).  An fp8 cache takes the k_scale /
        v_scale kwargs next to physical_kv_cache_k / _v."""
        k_cache, v_cache, bt, cl, bs, max_seq_len, layer_idx = _paged_args(kwargs, who)
        k_scale, v_scale = kwargs.get("k_scale"), kwargs.get("v_scale")
        if k_cache.dtype == torch.float8_e4m3fn and (k_scale is None or v_scale is None):
            raise ValueError(f"{who}: an fp8 (float8_e4m3fn) KV cache needs k_scale and v_scale "
                             "(PagedKVCache.get_kv_scales())")
        scales = {} if k_scale is None and v_scale is None else {"k_scale": k_scale, "v_scale": v_scale}
        q = q2d.view(B, q_len, self.num_attention_heads, self.head_dim)
        if self.config.rotary_dim > 0:
            # row i of sequence b sits at position context_lengths[b] - q_len + i (the keys were rotated when they were cached:
            # ops.rope_and_cache_varlen); computed on the device, nothing is read back
            pos = kwargs.get("position_ids")
            if pos is None:
                pos = (cl.to(device=q.device, dtype=torch.int32).view(B, 1) - q_len
                       + torch.arange(q_len, dtype=torch.int32, device=q.device).view(1, q_len))
            else:
                pos = pos.to(device=q.device, dtype=torch.int32)
            # with qk_norm the keys were also normalised on their way into the cache (ops.qknorm_rope_and_cache_varlen with
            # k_norm.weight); q is normalised here, in the same pass as its rotation
            q = self._rotate(q, pos, getattr(self, "q_norm", None))
        q = q.permute(0, 2, 1, 3)
        out = torch.empty(B, q_len, self.num_attention_heads, self.head_dim, dtype=dt, device=q2d.device)
        ops.paged_attention_forward(q, out.permute(0, 2, 1, 3), k_cache, v_cache, bt, cl, bs, max_seq_len, layer_idx,
                                    **_decode_window_kw(self.config), **scales)
        return linear(out.view(B, q_len, self.hidden_size), self.o_proj, self._cast, dt, residual=residual,
                      skinny=self.config.decode_gemm, skinny_w8=self.config.decode_gemm_fp8)

    def _plan(self, B, S, k_proj, k_cols, kv_stride, o_proj, mask: bool):
        """mio._nn.attention_plan of a dense self-attention call of this module (Sq = Sk = S) under its config."""
        cfg = self.config
        return attention_plan(B, S, S, self.num_attention_heads, self.num_kv_heads, self.head_dim, k_proj, k_cols, kv_stride,
                              o_proj, softmax_scale=cfg.softmax_scale, mask=mask, normalize_query=cfg.normalize_query,
                              return_softmax=cfg.return_softmax, windowed=_windowed(cfg), rotary=cfg.rotary_dim > 0)

    def _context(self, q, k, v, plan, attention_mask, kwargs):
        """Projected q [B,S,H,D] / k / v [B,S,Hkv,D] (views of the projection results) -> the attention result: rotary in place,
        then the pre-scaled-K kernel where the plan says so (k then holds K * softmax_scale * log2(e), scaled in fp32 by the
        projection's epilogue and rounded once; with plan.out_blocked the result comes in the out-projection's blocked
        activation layout), else the plain path.  [B,S,H,D], or blocked [ceil(B*S/256)*256, H*D]."""
        cfg = self.config
        if cfg.rotary_dim > 0:
            pos = self._dense_positions(kwargs, q.shape[1], q.device)
            q = self._rotate(q, pos, getattr(self, "q_norm", None))
            k = self._rotate(k, pos, getattr(self, "k_norm", None))
        if plan.kpre:
            return ops.fa3_fwd(q, k, v, causal=cfg.causal, k_prescaled=True, out_blocked=plan.out_blocked)
        if cfg.normalize_query:
            q = F.normalize(q, dim=-1)
        return ops.flash_attention(q, k, v, mask=attention_mask, causal=cfg.causal,
                                   softmax_scale=cfg.softmax_scale, block_size=cfg.block_size, **_window_kw(cfg))


class FlashAttentionLayer(_AttentionBase):
    """Separate q/k/v/o projections + FlashAttention3 (reference :474-659)."""

    def __init__(self, hidden_size: int, num_attention_heads: int, config: Optional[FlashAttentionConfig] = None,
                 num_kv_heads: Optional[int] = None):
        super().__init__()
        self._setup(hidden_size, num_attention_heads, config, num_kv_heads)
        self.q_proj = nn.Linear(hidden_size, hidden_size)
        self.k_proj = nn.Linear(hidden_size, self.num_kv_heads * self.head_dim)
        self.v_proj = nn.Linear(hidden_size, self.num_kv_heads * self.head_dim)
        self.o_proj = nn.Linear(hidden_size, hidden_size)
        self.flash_attention = FlashAttention3(self.config)
        self._init_weights()
        self._setup_qk_norm()

    def _init_weights(self):
        for lin in (self.q_proj, self.k_proj, self.v_proj, self.o_proj):  # N(0, 0.02), zero bias (:531-542)
            nn.init.normal_(lin.weight, mean=0.0, std=0.02)
            nn.init.zeros_(lin.bias)

    def forward(self, hidden_states: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
                residual: Optional[torch.Tensor] = None, **kwargs: Any) -> torch.Tensor:
        if hidden_states.dim() != 3:
            raise ValueError(f"Expected 3D input tensor, got shape: {hidden_states.shape}")
        if not hidden_states.is_cuda:
            raise ValueError("HIP kernels require input tensors to be on a CUDA (ROCm) device.")
        B, S, _ = hidden_states.shape
        in_dtype = hidden_states.dtype
        dt = compute_dtype(self.config.precision, hidden_states)
        x, r, c = as_dtype(hidden_states, dt), as_dtype(residual, dt), self._cast
        if "block_tables" in kwargs:
            q2d = linear(x, self.q_proj, c, dt, skinny=self.config.decode_gemm, skinny_w8=self.config.decode_gemm_fp8)
            return as_dtype(self._paged(q2d, B, S, dt, kwargs, "FlashAttentionLayer", r), in_dtype)
        _refuse(self.config, self.training)
        # K is the whole output of k_proj; q / k / v are tensors of their own and the context stays row-major (no o_proj shape)
        kv_dim = self.num_kv_heads * self.head_dim
        plan = self._plan(B, S, (B * S, kv_dim, self.k_proj.in_features), (0, kv_dim), kv_dim, None, attention_mask is not None)
        q = linear(x, self.q_proj, c, dt).view(B, S, self.num_attention_heads, self.head_dim)
        k = linear(x, self.k_proj, c, dt, col_scale=plan.col_scale).view(B, S, self.num_kv_heads, self.head_dim)
        v = linear(x, self.v_proj, c, dt).view(B, S, self.num_kv_heads, self.head_dim)
        ctx = self._context(q, k, v, plan, attention_mask, kwargs).view(B, S, self.hidden_size)
        return as_dtype(linear(ctx, self.o_proj, c, dt, residual=r), in_dtype)


class FlashSelfAttention(_AttentionBase):
    """Fused qkv projection [d, d + 2*Hkv*Dh] + FlashAttention3 (reference :662-949).  GQA is handled
    inside the kernel (kv head = h // (H/Hkv)), not by repeat_interleave (:894-912)."""

    def __init__(self, hidden_size: int, num_attention_heads: int, config: Optional[FlashAttentionConfig] = None,
                 num_kv_heads: Optional[int] = None):
        super().__init__()
        self._setup(hidden_size, num_attention_heads, config, num_kv_heads)
        kv_dim = self.num_kv_heads * self.head_dim
        self.qkv_proj = nn.Linear(hidden_size, hidden_size + 2 * kv_dim)
        self.o_proj = nn.Linear(hidden_size, hidden_size)
        self.flash_attention = FlashAttention3(self.config)
        self._init_weights()
        self._setup_qk_norm()

    def _init_weights(self):
        for lin in (self.qkv_proj, self.o_proj):
            nn.init.normal_(lin.weight, mean=0.0, std=0.02)
            nn.init.zeros_(lin.bias)

    def stream_ok(self, B: int, S: int, dtype: torch.dtype, pre_norm: Optional[nn.Module]) -> bool:
        """True iff forward(...) can take / return the residual stream as a ResidualStream at this size: the folded GEMMs on both
        projections (ops.gemm_ln_ok); the attention between them is whatever forward() would run (pre-scaled K + blocked output
        where the kernels take the head dim, else the plain tiled kernel and a row-major context)."""
        cfg = self.config
        d, q_dim, kv_dim = self.qkv_proj.in_features, self.hidden_size, self.num_kv_heads * self.head_dim
        n_tot, M = q_dim + 2 * kv_dim, B * S
        if not stream_preconditions(dtype, pre_norm, cfg.precision, d) or self.o_proj.out_features != d or q_dim != d:
            return False
        if _windowed(cfg) or cfg.rotary_dim > 0:  # forward() takes these on the ordinary route only
            return False
        if cfg.normalize_query or cfg.return_softmax or (self.training and cfg.dropout_p > 0.0):
            return False
        return (ops.blocked_weight_ok(M, n_tot, d) and ops.gemm_ln_ok(M, n_tot, d, "none", fold_in=True)
                and ops.gemm_ln_ok(M, d, q_dim, "none", stats_out=True))

    def forward(self, hidden_states: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
                residual: Optional[torch.Tensor] = None, pre_norm: Optional[nn.Module] = None,
                stream_out: bool = False, **kwargs: Any) -> torch.Tensor:
        """pre_norm (not in the reference): a LayerNorm or RMSNorm (mio._nn.norm_kind) to apply to hidden_states first -- the
        pre-LN block's `attn(ln(x))` in one call, which lets the norm hand its output to the QKV GEMM in the blocked layout.
        hidden_states may be a ResidualStream (mio._nn) and stream_out=True returns one, where stream_ok() says so: the
        residual is then the stream itself (`x + attn(ln(x))`) and the LayerNorm is folded into the GEMMs (ops.gemm_ln)."""
        stream = isinstance(hidden_states, ResidualStream) or stream_out
        c, cfg = self._cast, self.config
        if stream:  # runs in the stream's dtype (stream_ok): nothing is cast, the residual is the input itself
            B, S, _ = hidden_states.shape
            if attention_mask is not None or kwargs or (residual is not None and residual is not hidden_states) or \
                    not self.stream_ok(B, S, hidden_states.dtype, pre_norm):
                raise ValueError("the ResidualStream form needs pre_norm, residual = the input itself, no mask / paged arguments "
                                 "and a size with stream_ok()")
            x = r = hidden_states
            in_dtype = dt = hidden_states.dtype
        else:
            if hidden_states.dim() != 3:
                raise ValueError(f"Expected 3D input tensor, got shape: {hidden_states.shape}")
            if not hidden_states.is_cuda:
                raise ValueError("HIP kernels require input tensors to be on a CUDA (ROCm) device.")
            B, S, _ = hidden_states.shape
            in_dtype = hidden_states.dtype
            dt = compute_dtype(cfg.precision, hidden_states)
            x, r = as_dtype(hidden_states, dt), as_dtype(residual, dt)
        q_dim, kv_dim = self.hidden_size, self.num_kv_heads * self.head_dim
        if "block_tables" in kwargs:
            if pre_norm is not None:
                x = apply_norm(x, pre_norm, c, dt)
            # only the query slice of the fused projection is needed on the paged path (:572-621)
            route = decode_route([(B * S, q_dim, self.qkv_proj.in_features, "none")], cfg.decode_gemm, cfg.decode_gemm_fp8)
            q2d = routed_linear(route, x, self.qkv_proj, c, dt, rows=q_dim)
            return as_dtype(self._paged(q2d, B, S, dt, kwargs, "FlashSelfAttention", r), in_dtype)
        _refuse(cfg, self.training)
        # [B,S,q_dim+2*kv_dim]; q / k / v are strided views of it, K its columns [q_dim, q_dim + kv_dim)
        n_tot, d = q_dim + 2 * kv_dim, self.qkv_proj.in_features
        plan = self._plan(B, S, (B * S, n_tot, d), (q_dim, q_dim + kv_dim), n_tot, (B * S, self.o_proj.out_features, q_dim),
                          attention_mask is not None)
        if isinstance(x, ResidualStream):
            qkv = folded_linear(x, pre_norm, self.qkv_proj, c, col_scale=plan.col_scale).view(B, S, n_tot)
        elif pre_norm is None:
            qkv = linear(x, self.qkv_proj, c, dt, col_scale=plan.col_scale)
        else:
            qkv = prenorm_linear(x, pre_norm, self.qkv_proj, c, dt, col_scale=plan.col_scale)
        q = qkv[:, :, :q_dim].view(B, S, self.num_attention_heads, self.head_dim)
        k = qkv[:, :, q_dim:q_dim + kv_dim].view(B, S, self.num_kv_heads, self.head_dim)
        v = qkv[:, :, q_dim + kv_dim:].view(B, S, self.num_kv_heads, self.head_dim)
        ctx = self._context(q, k, v, plan, attention_mask, kwargs)
        if stream:
            return residual_linear(ctx if plan.out_blocked else ctx.reshape(B * S, q_dim), self.o_proj, c, x,
                                   x_blocked=plan.out_blocked, stream_out=stream_out)
        if plan.out_blocked:
            out = linear(ctx, self.o_proj, c, dt, residual=r, x_blocked_shape=(B, S, q_dim))
        else:
            out = linear(ctx.view(B, S, q_dim), self.o_proj, c, dt, residual=r)
        return as_dtype(out, in_dtype)


def _lin_weight(lin: nn.Module) -> torch.Tensor:
    return lin.weight.t() if type(lin).__name__ == "Conv1D" else lin.weight


def _copy_linear(dst: nn.Linear, src: nn.Module, rows: Optional[slice] = None) -> None:
    with torch.no_grad():
        w = _lin_weight(src)
        b = getattr(src, "bias", None)
        if rows is not None:
            w = w[rows]
            b = None if b is None else b[rows]
        dst.weight.copy_(w)
        if b is not None:
            dst.bias.copy_(b)
        else:
            dst.bias.zero_()


class ModelConverter:
    """Find attention modules and replace them with FlashAttentionLayer / FlashSelfAttention
    (reference :952-1168).  Detection = the reference's class-name set (:1033-1044) or attribute
    sniffing (:1048-1059); additionally HF GPT-2's c_attn/c_proj Conv1D layout is converted WITH its
    weights (the reference matches GPT2Attention by name but copies nothing -> random replacement)."""

    _NAMES = {"MultiHeadAttention", "BertSelfAttention", "T5Attention", "GPT2Attention", "LlamaAttention",
              "MistralAttention", "CLIPAttention", "OPTAttention", "RobertaAttention", "FalconAttention"}

    def __init__(self, config: Optional[FlashAttentionConfig] = None):
        self.config = config or FlashAttentionConfig()
        self.replacements = 0

    def convert_model(self, model: nn.Module) -> nn.Module:
        return self._find_and_replace_attention(model)

    def _find_and_replace_attention(self, module: nn.Module) -> nn.Module:
        for name, sub in list(module.named_children()):
            if isinstance(sub, (FlashAttentionLayer, FlashSelfAttention)):
                continue
            if self._is_attention_module(sub) and self._convertible(sub):
                setattr(module, name, self._create_flash_replacement(sub))
                self.replacements += 1
            else:
                self._find_and_replace_attention(sub)
        return module

    def _is_attention_module(self, module: nn.Module) -> bool:
        if type(module).__name__ in self._NAMES:
            return True
        has_qkv = hasattr(module, "q_proj") and hasattr(module, "k_proj") and hasattr(module, "v_proj")
        has_out = hasattr(module, "out_proj") or hasattr(module, "o_proj")
        has_heads = hasattr(module, "num_heads") or hasattr(module, "num_attention_heads")
        if has_qkv and has_out and has_heads:
            return True
        has_fused = hasattr(module, "qkv_proj") or hasattr(module, "qkv")
        return bool(has_fused and has_out and has_heads)

    @staticmethod
    def _convertible(module: nn.Module) -> bool:
        """A name match whose projections we cannot locate is left alone rather than replaced by a
        randomly initialised layer."""
        sep = all(hasattr(module, n) for n in ("q_proj", "k_proj", "v_proj"))
        fused = hasattr(module, "qkv_proj") or hasattr(module, "qkv") or hasattr(module, "c_attn")
        out = any(hasattr(module, n) for n in ("o_proj", "out_proj", "c_proj"))
        return (sep or fused) and out

    def _create_flash_replacement(self, module: nn.Module) -> nn.Module:
        sep = all(hasattr(module, n) for n in ("q_proj", "k_proj", "v_proj"))
        if hasattr(module, "num_attention_heads"):
            H = module.num_attention_heads
        elif hasattr(module, "num_heads"):
            H = module.num_heads
        else:
            H = 8
        Hkv = getattr(module, "num_kv_heads", None) or getattr(module, "num_key_value_heads", None)
        if hasattr(module, "hidden_size"):
            d = module.hidden_size
        elif hasattr(module, "embed_dim"):
            d = module.embed_dim
        elif sep:
            d = _lin_weight(module.q_proj).shape[0]
        elif hasattr(module, "c_attn"):
            d = _lin_weight(module.c_attn).shape[1]
        else:
            d = 512
        cfg = copy.copy(self.config)
        if getattr(module, "is_causal", None) is True or getattr(module, "causal", None) is True:
            cfg.causal = True
        out_name = next(n for n in ("o_proj", "out_proj", "c_proj") if hasattr(module, n))
        ref_p = next(module.parameters(), None)
        if sep:
            kv_rows = _lin_weight(module.k_proj).shape[0]
            if Hkv is None:
                Hkv = kv_rows // (d // H)
            rep = FlashAttentionLayer(d, H, cfg, num_kv_heads=Hkv)
            if ref_p is not None:
                rep = rep.to(device=ref_p.device, dtype=ref_p.dtype)
            for n in ("q_proj", "k_proj", "v_proj"):
                _copy_linear(getattr(rep, n), getattr(module, n))
        else:
            qkv_name = next(n for n in ("qkv_proj", "qkv", "c_attn") if hasattr(module, n))
            rows = _lin_weight(getattr(module, qkv_name)).shape[0]
            if Hkv is None:
                Hkv = (rows - d) // 2 // (d // H)
            rep = FlashSelfAttention(d, H, cfg, num_kv_heads=Hkv)
            if ref_p is not None:
                rep = rep.to(device=ref_p.device, dtype=ref_p.dtype)
            _copy_linear(rep.qkv_proj, getattr(module, qkv_name))
        _copy_linear(rep.o_proj, getattr(module, out_name))
        if cfg.qk_norm:  # the source's per-head norm weights, where it has them in this shape; anything else is left alone
            for n in ("q_norm", "k_norm"):
                w = getattr(getattr(module, n, None), "weight", None)
                if isinstance(w, torch.Tensor) and tuple(w.shape) == (rep.head_dim,):
                    with torch.no_grad():
                        getattr(rep, n).weight.copy_(w)
        rep.train(module.training)
        return rep

    @staticmethod
    def convert_mask(attention_mask: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
        """Reference :1144-1168."""
        if attention_mask is None:
            return None
        if attention_mask.dim() == 2:
            attention_mask = attention_mask.unsqueeze(1).unsqueeze(2)
        elif attention_mask.dim() == 3 and attention_mask.shape[1] == 1:
            attention_mask = attention_mask.unsqueeze(2)
        return attention_mask.bool()

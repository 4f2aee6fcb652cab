"""Small host-side helpers shared by the nn.Module wrappers (precision casting, Linear via the HIP GEMM)."""
from __future__ import annotations

import math
from typing import Dict, NamedTuple, Optional, Tuple

import torch
import torch.nn as nn

from . import ops

_PRECISION = {"fp16": torch.float16, "bf16": torch.bfloat16}


def compute_dtype(precision: str, x: torch.Tensor) -> torch.dtype:
    """dtype the HIP kernels run in for a module configured with `precision`.

    The reference casts to `config.precision` before its Triton launch
    (flash_attention.py:176-198, fused_mlp.py:106-123).  fp16/bf16 map directly; "fp32" means
    "keep the tensor's dtype" there, which the MFMA kernels cannot do: a 16-bit input is used as
    is, an fp32 input raises (no silent down-cast of an fp32-configured module)."""
    if precision in _PRECISION:
        return _PRECISION[precision]
    if precision == "fp32":
        if x.dtype in (torch.float16, torch.bfloat16):
            return x.dtype
        raise RuntimeError("precision='fp32' with fp32 tensors is not supported by the MFMA kernels; "
                           "configure precision='bf16' or 'fp16'")
    if precision == "fp8":
        raise RuntimeError("FP8 precision is not supported by the HIP path (the reference gates it to "
                           "Hopper, flash_attention.py:89-100)")
    raise ValueError(f"Unsupported precision mode: {precision}")


def as_dtype(t: Optional[torch.Tensor], dtype: torch.dtype) -> Optional[torch.Tensor]:
    """t in dtype (t itself where it already is; None stays None): the cast into the compute dtype and the cast back."""
    return t if t is None or t.dtype == dtype else t.to(dtype)


def norm_kind(norm: nn.Module, dtype: Optional[torch.dtype] = None) -> Tuple[str, float]:
    """(kind, effective eps) of a norm module the wrappers take as pre_norm: "layernorm" for nn.LayerNorm, "rms" for nn.RMSNorm
    (whose eps=None means torch.finfo(dtype).eps of the activations, as torch's own module resolves it); TypeError for anything
    else.  The kind is the norm= of ops.gemm_ln / ops.gemm_route."""
    if isinstance(norm, nn.LayerNorm):
        return "layernorm", float(norm.eps)
    if isinstance(norm, nn.RMSNorm):
        if norm.eps is not None:
            return "rms", float(norm.eps)
        if dtype is None:
            raise ValueError("an RMSNorm with eps=None takes its eps from the activation dtype: give dtype")
        return "rms", float(torch.finfo(dtype).eps)
    raise TypeError(f"pre_norm must be an nn.LayerNorm or an nn.RMSNorm, got {type(norm).__name__}")


def _versions(*ps: Optional[torch.Tensor]) -> Tuple:
    return tuple((None if t is None else (t.data_ptr(), t._version)) for t in ps)


class CastCache:
    """Caches parameter copies in the compute dtype, keyed on (data_ptr, _version, dtype), so a module
    whose parameters are stored in another dtype does not re-cast them on every forward; and what is prepared from those
    copies once per version of the parameters involved (blocked and norm-folded weights)."""

    def __init__(self):
        self._c: Dict[object, Tuple[Tuple, object]] = {}

    def _memo(self, slot, key: Tuple, make):
        """The value kept in `slot` if it was made under `key`, else make() (kept from now on)."""
        hit = self._c.get(slot)
        if hit is not None and hit[0] == key:
            return hit[1]
        t = make()
        self._c[slot] = (key, t)
        return t

    def get(self, p: Optional[torch.Tensor], dtype: torch.dtype) -> Optional[torch.Tensor]:
        if p is None:
            return None
        if p.dtype == dtype and p.is_contiguous():
            return p.detach()
        return self._memo(id(p), (p.data_ptr(), p._version, dtype, p.device), lambda: p.detach().to(dtype).contiguous())

    def get_blocked(self, p: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
        """The parameter in the blocked weight layout (ops.block_weight), repacked when its version changes."""
        return self._memo(("b", id(p)), (p.data_ptr(), p._version, dtype, p.device, "blocked"),
                          lambda: ops.block_weight(self.get(p, dtype)))

    def get_w8(self, p: torch.Tensor, dtype: torch.dtype) -> Tuple[torch.Tensor, torch.Tensor]:
        """The parameter as weight-only FP8 (ops.quantize_weight_w8 of its copy in dtype): (w8 [N, K] float8_e4m3fn, scale [N]
        fp32), quantised again when its version changes."""
        return self._memo(("w8", id(p)), (p.data_ptr(), p._version, dtype, p.device, "w8"),
                          lambda: ops.quantize_weight_w8(self.get(p, dtype)))

    def get_row_padded(self, p: torch.Tensor, dtype: torch.dtype, multiple: int) -> torch.Tensor:
        """The 2-D parameter in dtype with zero rows appended up to the next multiple of `multiple` rows (itself where it has that
        many already), made again when its version changes."""
        w = self.get(p, dtype)
        pad = -w.shape[0] % multiple
        if pad == 0:
            return w
        return self._memo(("rp", id(p), multiple), (p.data_ptr(), p._version, dtype, p.device, "row_padded"),
                          lambda: torch.cat([w, w.new_zeros(pad, w.shape[1])]))

    def get_cat(self, ps: Tuple[Optional[torch.Tensor], ...], dtype: torch.dtype, blocked: bool = False) -> Optional[torch.Tensor]:
        """The row-concatenation of the parameters ps in dtype (None where they are: biases that are not there), or with blocked
        that weight in the blocked layout; made again when one of them changes."""
        if ps[0] is None:
            return None
        key = _versions(*ps) + (dtype, ps[0].device)
        if blocked:
            return self._memo(("cb",) + tuple(map(id, ps)), key, lambda: ops.block_weight(self.get_cat(ps, dtype)))
        return self._memo(("c",) + tuple(map(id, ps)), key, lambda: torch.cat([self.get(p, dtype) for p in ps], dim=0).contiguous())

    def get_blocked_glu(self, gate: torch.Tensor, up: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
        """The SwiGLU gate / up parameters as ONE interleaved blocked weight (ops.block_weight_glu), repacked when either changes."""
        return self._memo(("g", id(gate), id(up)),
                          (gate.data_ptr(), gate._version, up.data_ptr(), up._version, dtype, gate.device, "blocked_glu"),
                          lambda: ops.block_weight_glu(self.get(gate, dtype), self.get(up, dtype)))

    def _fold(self, lin: nn.Linear, ln: nn.Module, kind: str, dtype: torch.dtype, blocked: bool = True):
        """ops.ln_fold_weight / ops.rms_fold_weight of the projection `lin` behind the norm `ln` of that kind."""
        w, lw, b = self.get(lin.weight, dtype), self.get(ln.weight, dtype), self.get(lin.bias, dtype)
        if kind == "rms":
            return ops.rms_fold_weight(w, lw, b, blocked=blocked)
        return ops.ln_fold_weight(w, lw, self.get(ln.bias, dtype), b, blocked=blocked)

    def get_ln_folded(self, lin: nn.Linear, ln: nn.Module, dtype: torch.dtype):
        """The projection `lin` behind the norm `ln`, prepared once per version of the parameters involved.  LayerNorm: (blocked
        gamma-scaled, row-centred weight, beta-folded bias) (ops.ln_fold_weight); RMSNorm: (blocked gamma-scaled weight, bias)
        (ops.rms_fold_weight).  The kind is part of the key and the slot: one Linear behind two kinds of norm keeps two folds."""
        kind = norm_kind(ln, dtype)[0]
        ps = (lin.weight, lin.bias, ln.weight) + ((ln.bias,) if kind == "layernorm" else ())
        return self._memo(("f", kind, id(lin.weight), id(ln.weight)), _versions(*ps) + (dtype, lin.weight.device, "ln_fold", kind),
                          lambda: self._fold(lin, ln, kind, dtype))

    def get_ln_folded_glu(self, gate: nn.Linear, up: nn.Linear, ln: nn.Module, dtype: torch.dtype):
        """The SwiGLU pair behind the norm `ln` (LayerNorm or RMSNorm, as get_ln_folded): (interleaved blocked weight of the two
        folded weights, up bias', gate bias')."""
        kind = norm_kind(ln, dtype)[0]
        ps = (gate.weight, gate.bias, up.weight, up.bias, ln.weight) + ((ln.bias,) if kind == "layernorm" else ())

        def make():
            (wg, bg), (wu, bu) = self._fold(gate, ln, kind, dtype, blocked=False), self._fold(up, ln, kind, dtype, blocked=False)
            return ops.block_weight_glu(wg, wu), bu, bg

        return self._memo(("fg", kind, id(gate.weight), id(up.weight), id(ln.weight)),
                          _versions(*ps) + (dtype, up.weight.device, "ln_fold_glu", kind), make)


def apply_norm(x: torch.Tensor, norm: nn.Module, cache: "CastCache", dtype: torch.dtype, out_blocked: bool = False) -> torch.Tensor:
    """norm(x) on the row kernel of the module's kind (an RMSNorm has no bias: none is read)."""
    kind, eps = norm_kind(norm, x.dtype)
    if kind == "rms":
        return ops.rmsnorm(x, cache.get(norm.weight, dtype), eps, out_blocked=out_blocked)
    return ops.layernorm(x, cache.get(norm.weight, dtype), cache.get(norm.bias, dtype), eps, out_blocked=out_blocked)


class ResidualStream:
    """The residual stream between two sub-layers as the folded kernels hand it on (ops.gemm_ln): `blocked` is the
    [ceil(M/256)*256, d] tensor in the blocked activation layout, `stats` the (sum, sum of squares) row statistics its
    producer wrote beside it ([d/256, ceil(M/256)*256, 2] fp32), `shape` the logical (B, S, d).  A sub-layer that takes a
    ResidualStream normalises inside its first GEMM's read-out and reads the residual from `blocked`; no LayerNorm launch."""
    __slots__ = ("blocked", "stats", "shape")

    def __init__(self, blocked: torch.Tensor, stats: torch.Tensor, shape: Tuple[int, int, int]):
        self.blocked, self.stats, self.shape = blocked, stats, tuple(shape)

    @property
    def dtype(self):
        return self.blocked.dtype

    @property
    def device(self):
        return self.blocked.device

    def dense(self) -> torch.Tensor:
        """Row-major [B, S, d] copy (tests / debugging: a strided view copied by torch, not a kernel of this package)."""
        B, S, d = self.shape
        mp = self.blocked.shape[0]
        return self.blocked.view(mp // 256, d // 32, 256, 32).permute(0, 2, 1, 3).reshape(mp, d)[:B * S].reshape(B, S, d)


def decode_route(calls, skinny: bool, skinny_w8: bool) -> Optional[str]:
    """The decode-step route of the GEMMs calls = [(M, N, K, activation), ...] that run as a group, under the modules' decode_gemm
    (skinny) and decode_gemm_fp8 (skinny_w8) options: "w8" (ops.gemm_skinny_w8 on the weights' FP8 copies) if that option is on
    and ops.gemm_skinny_w8_ok advises every call, else "skinny" (ops.gemm_skinny) if that one is on and ops.gemm_skinny_ok advises
    every call, else None.  An option that is off asks nothing."""
    if skinny_w8 and all(ops.gemm_skinny_w8_ok(*c) for c in calls):
        return "w8"
    if skinny and all(ops.gemm_skinny_ok(*c) for c in calls):
        return "skinny"
    return None


def routed_linear(route: Optional[str], x: torch.Tensor, lin: nn.Linear, cache: "CastCache", dtype: torch.dtype,
                  activation: str = "none", gate: Optional[nn.Linear] = None, rows: Optional[int] = None,
                  residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """lin(x) (+ activation; gate: the SwiGLU gate projection; + residual) of a row-major x on the route decode_route decided,
    None being ops.gemm_bias_act on the row-major weight.  rows: only the first `rows` output features of lin (the query rows
    of a fused qkv projection).  "w8" reads CastCache.get_w8's copies (a sliced projection is quantised whole, once: rows are
    independent), the others the 16-bit copies."""
    bias = cache.get(lin.bias, dtype)
    bias = None if bias is None else bias[:rows].contiguous()
    gb = None if gate is None else cache.get(gate.bias, dtype)
    if route == "w8":
        w8, scale = cache.get_w8(lin.weight, dtype)
        g8, gs = (None, None) if gate is None else cache.get_w8(gate.weight, dtype)
        return ops.gemm_skinny_w8(x, w8[:rows], scale[:rows], bias, activation, g8, gs, gb, residual)
    gemm = ops.gemm_skinny if route == "skinny" else ops.gemm_bias_act
    gw = None if gate is None else cache.get(gate.weight, dtype)
    return gemm(x, cache.get(lin.weight, dtype)[:rows], bias, activation, gw, gb, residual)


def linear(x: torch.Tensor, lin: nn.Linear, cache: CastCache, dtype: torch.dtype, activation: str = "none",
           residual: Optional[torch.Tensor] = None, col_scale=None, x_blocked_shape=None, skinny: bool = False,
           skinny_w8: bool = False) -> torch.Tensor:
    """F.linear(x, W, b) (+ activation, + residual) on the MFMA GEMM.  At sizes that run the 256x256-tile kernels the
    weight is handed over in the blocked layout (repacked once per parameter version, cached next to the cast copy).
    skinny / skinny_w8 (the modules' decode_gemm / decode_gemm_fp8 options): a row-major x without a column scale goes to the
    decode-step GEMM decode_route picks, if it picks one."""
    N, K = lin.weight.shape
    M = x.numel() // K if x_blocked_shape is None else int(math.prod(x_blocked_shape[:-1]))
    if x_blocked_shape is None and col_scale is None:
        route = decode_route([(M, N, K, activation)], skinny, skinny_w8)
        if route is not None:
            return routed_linear(route, x, lin, cache, dtype, activation, residual=residual)
    w = cache.get(lin.weight, dtype)
    wb = cache.get_blocked(lin.weight, dtype) if (K % 32 == 0 and ops.blocked_weight_ok(M, N, K, activation)) else None
    return ops.gemm_bias_act(x, w, cache.get(lin.bias, dtype), activation, residual=residual, w_blocked=wb,
                             col_scale=col_scale, x_blocked_shape=x_blocked_shape)


def prenorm_linear(x: torch.Tensor, ln: nn.Module, lin: nn.Linear, cache: CastCache, dtype: torch.dtype,
                   activation: str = "none", residual: Optional[torch.Tensor] = None, col_scale=None) -> torch.Tensor:
    """lin(ln(x)) (+ activation, + residual), ln a LayerNorm or an RMSNorm (norm_kind).  At sizes that run the 256x256-tile
    kernels the norm writes its output in the blocked activation layout, so the GEMM's K-tile fetches are contiguous on both
    operands."""
    w = cache.get(lin.weight, dtype)
    N, K = w.shape
    M = x.numel() // K
    if K % 32 == 0 and not ops.NO_BLOCKED_X and ops.blocked_weight_ok(M, N, K, activation):
        xb = apply_norm(x, ln, cache, dtype, out_blocked=True)
        return ops.gemm_bias_act(xb, w, cache.get(lin.bias, dtype), activation, residual=residual,
                                 w_blocked=cache.get_blocked(lin.weight, dtype), x_blocked_shape=tuple(x.shape),
                                 col_scale=col_scale)
    return linear(apply_norm(x, ln, cache, dtype), lin, cache, dtype, activation, residual, col_scale=col_scale)


# ---- the attention plan: may K leave its projection pre-scaled, may the context be written blocked ---------------------------
LOG2E = 1.4426950408889634  # the attention kernels work in base 2: a pre-scaled K holds K * softmax_scale * log2(e)


class AttentionPlan(NamedTuple):
    kpre: bool                                     # ops.fa3_fwd(k_prescaled=True) on a K the projection scaled
    col_scale: Optional[Tuple[int, int, float]]    # the col_scale= of the projection that produces K (None: unscaled)
    out_blocked: bool                              # ops.fa3_fwd(out_blocked=True): the context in the out-projection's blocked layout


def attention_plan(B: int, Sq: int, Sk: int, H: int, Hkv: int, D: int, k_proj: Tuple[int, int, int], k_cols: Tuple[int, int],
                   kv_stride: int, o_proj: Optional[Tuple[int, int, int]] = None, *, softmax_scale: Optional[float] = None,
                   mask: bool = False, normalize_query: bool = False, return_softmax: bool = False, windowed: bool = False,
                   rotary: bool = False, carry: bool = False) -> AttentionPlan:
    """The one statement of both decisions, from sizes and flags alone (no tensors).  k_proj = (rows, N, K) is the GEMM that
    produces K, in columns k_cols = [lo, hi) of its output; kv_stride the row stride of K and V as the attention kernel reads
    them; o_proj = (rows, N, K) the output projection that would read a blocked context (None: the caller has no use for one).
    carry: the launch runs with the (o_acc, lse) ring carry.  Hkv belongs to the launch's geometry; no term reads it today.

    K may be pre-scaled iff
      * the call is one the pre-scaled-K kernels take and the plain path does not have to run: no mask, no window (neither
        kernel family takes a pre-scaled K), no normalize_query, no return_softmax, no rotary (the rotation comes before any
        scaling of K);
      * lo and hi are multiples of 128, the column granularity of the GEMM's scaled read-out;
      * the attention kernel takes it: ops.fa3_k_prescaled_ok (head dim, Sq > 128, 32-bit K / V offsets);
      * the projection runs the persistent 256-tile kernel: ops.col_scale_ok.  mio_gemm_col_scale_ok (gemm_api.hip:41-43)
        already implies the blocked weight (mio_gemm_blocked_weight_ok is its first term) and K % 32 == 0 (K % 64 == 0), and
        the Python query honours MIO_NO_BLOCKED_W: nobody needs to ask those again.
    The context may be written blocked iff K is pre-scaled (the only kernels with that epilogue), the output projection takes
    blocked operands (ops.blocked_weight_ok; the stream form's producer asked ops.gemm_ln_ok in stream_ok(), and mio_gemm_ln_ok
    implies it, gemm_api.hip:67) and ops.fa3_o_blocked_ok says so (no carry, D <= 64, (H * D) % 32 == 0, MIO_NO_BLOCKED_X)."""
    lo, hi = k_cols
    kpre = (not (mask or normalize_query or return_softmax or windowed or rotary) and lo % 128 == 0 and hi % 128 == 0
            and ops.fa3_k_prescaled_ok(B, Sq, Sk, H, D, kv_stride, kv_stride, carry) and ops.col_scale_ok(*k_proj))
    if not kpre:
        return AttentionPlan(False, None, False)
    scale = softmax_scale if softmax_scale is not None else 1.0 / math.sqrt(D)
    out_blocked = (o_proj is not None and not carry and ops.blocked_weight_ok(*o_proj)
                   and ops.fa3_o_blocked_ok(B, Sq, Sk, H, D, kv_stride, kv_stride))
    return AttentionPlan(True, (lo, hi, scale * LOG2E), out_blocked)


# ---- the residual stream between sub-layers: preconditions, consumer, producer -----------------------------------------------
def stream_preconditions(dtype: torch.dtype, pre_norm: Optional[nn.Module], precision: str, d: int) -> bool:
    """The part of stream_ok() every sub-layer shares: a 16-bit stream, a pre_norm of a known kind (TypeError otherwise) with a
    weight over exactly the stream's width d, blocked activations not switched off (MIO_NO_BLOCKED_X), and a module whose
    compute dtype is the stream's (the stream form does not cast)."""
    if dtype not in (torch.float16, torch.bfloat16) or pre_norm is None or pre_norm.weight is None or ops.NO_BLOCKED_X:
        return False
    norm_kind(pre_norm, dtype)
    return compute_dtype(precision, torch.empty(0, dtype=dtype)) == dtype and tuple(pre_norm.normalized_shape) == (d,)


def folded_linear(s: ResidualStream, ln: nn.Module, lin: nn.Linear, cache: CastCache, activation: str = "none", col_scale=None,
                  gate: Optional[nn.Linear] = None, out_blocked: bool = False) -> torch.Tensor:
    """The stream's consumer: lin(ln(s)) (+ activation; gate: the SwiGLU pair) with the norm in the GEMM's read-out, from the
    raw blocked stream and its row statistics (ops.gemm_ln with the weights of CastCache.get_ln_folded).  Returns [B*S, N]
    rows, or with out_blocked the blocked layout for the next GEMM."""
    dt = s.dtype
    if gate is None:
        (w, b), bg = cache.get_ln_folded(lin, ln, dt), None
    else:
        w, b, bg = cache.get_ln_folded_glu(gate, lin, ln, dt)
    kind, eps = norm_kind(ln, dt)
    B, S, d = s.shape
    return ops.gemm_ln(s.blocked, w, b, M=B * S, N=lin.out_features, K=d, activation=activation, x_blocked=True,
                       out_blocked=out_blocked, ln_stats=s.stats, eps=eps, col_scale=col_scale, bias_gate=bg, norm=kind)[0]


def residual_linear(x: torch.Tensor, lin: nn.Linear, cache: CastCache, res, x_blocked: bool = False, stream_out: bool = False):
    """The stream's producer: res + lin(x), res the sub-layer's input (a ResidualStream, read blocked, or a [B, S, d] tensor), x
    [B*S, K] rows or (x_blocked) the blocked layout.  Writes the next ResidualStream (blocked + row statistics, stream_out) or a
    plain [B, S, d] tensor."""
    B, S, d = res.shape
    M, dt, blocked = B * S, res.dtype, isinstance(res, ResidualStream)
    y, st = ops.gemm_ln(x, cache.get_blocked(lin.weight, dt), cache.get(lin.bias, dt), M=M, N=d, K=lin.in_features,
                        x_blocked=x_blocked, residual=res.blocked if blocked else res.reshape(M, d), res_blocked=blocked,
                        out_blocked=stream_out, stats_out=stream_out)
    return ResidualStream(y, st, (B, S, d)) if stream_out else y.view(B, S, d)

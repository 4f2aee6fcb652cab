"""Mixture-of-experts MLP on the HIP kernels, for decode steps and for tall inputs (not a reference module: its models are dense).

MoEMLP replaces the MLP of a Mixtral / Qwen-MoE / OLMoE class block: a router (one linear layer to E logits per token), the
top_k experts of every token, and the weighted sum of those experts' MLPs.  forward() is the router GEMM, ops.moe_route and
ops.moe_mlp (the grouped up projection, then the grouped down projection with the combine): four to six launches whatever E is,
the routing device data from start to end, so a step can be captured in a graph.  MoEConfig selects the FP8 copies of the expert
weights (ops.moe_mlp_w8) or, for more than 64 rows, the tiled path (ops.moe_route_prefill, ops.moe_mlp_prefill; on loaded MXFP4 bytes
ops.moe_mlp_prefill_w4).  There is no
PyTorch path: CPU tensors raise ValueError as the other modules do.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional, Sequence

import torch
import torch.nn as nn

from ... import ops
from ..._nn import CastCache, as_dtype


@dataclass
class MoEConfig:
    """activation: "swiglu" (gate and up weights) or one of none / gelu / gelu_erf / relu / silu (up weight only).  renormalize: the
    top_k softmax weights divided by their sum (Mixtral, Qwen3-MoE: True; OLMoE, Qwen2-MoE: False).  dtype: the compute dtype.
    grouped_prefill: inputs of more than 64 rows run the tiled grouped GEMMs (ops.moe_route_prefill, ops.moe_mlp_prefill): one
    routing and one pass over the active experts' weights per 8192 rows, in place of the decode path in row chunks of 64.  Off
    by default: forward is then what it was, to the bit.
    expert_weights_fp8: the decode kernels (T <= 64 and the row-chunk path) read weight-only FP8 copies of w_up, w_gate and w_down
    (ops.quantize_expert_weights_w8: e4m3fn bytes, one fp32 scale per expert and output channel, made once per version of a
    parameter) through ops.moe_mlp_w8: half the weight bytes per step.  hidden_size and intermediate_size must then be multiples
    of 16.  The router GEMM stays 16-bit, and so does grouped_prefill, which keeps reading the 16-bit weights.  Off by default:
    forward is then what it was, to the bit.  Whether it pays at a shape is the caller's to measure (profiles/moe_w8.md).
    expert_weights_mxfp4: the same with MXFP4 copies (ops.quantize_expert_weights_mxfp4: e2m1 nibbles, one e8m0 scale byte per 32
    k) through ops.moe_mlp_w4: a quarter of the 16-bit weight bytes plus 1/32 for the scales per step.  Exclusive with
    expert_weights_fp8; hidden_size and intermediate_size must be multiples of 32; dtype must be bf16.  The router GEMM and
    grouped_prefill stay 16-bit: the module holds the 16-bit parameters, and its tall inputs read them.  A module whose experts
    were loaded as MXFP4 bytes (MoEMLP.load_mxfp4_experts) holds nothing else, and its grouped_prefill runs the tiled grouped
    GEMMs on those bytes (ops.moe_mlp_prefill_w4, profiles/moe_prefill_w4.md).  Off by default (profiles/moe_w4.md)."""
    activation: str = "swiglu"
    renormalize: bool = True
    dtype: torch.dtype = torch.bfloat16
    grouped_prefill: bool = False
    expert_weights_fp8: bool = False
    expert_weights_mxfp4: bool = False


_MXFP4_NAMES = ("w4_up", "s_up", "w4_down", "s_down", "w4_gate", "s_gate")  # ops.moe_mlp_w4's names for the loaded bytes


class MoEMLP(nn.Module):
    """y[t] = sum_j w[t, j] * expert_{ids[t, j]}(x[t]) (+ residual[t]) with (ids, w) = top_k of softmax(router(x[t])).

    Parameters: router.weight [E, d]; w_up [E, I, d], w_gate [E, I, d] (swiglu only), w_down [E, d, I], stacked per expert; no
    biases.  A parameter stored in another dtype than config.dtype is cast once per version (CastCache), so an in-place update is
    seen by the next forward.  With config.expert_weights_fp8 the decode kernels read weight-only FP8 copies of the three stacked
    expert weights (e4m3fn bytes and fp32 scales [E, N]), quantised from the compute-dtype copies once per version in the same
    way; the parameters themselves stay as they are stored."""

    def __init__(self, hidden_size: int, intermediate_size: int, num_experts: int, top_k: int, config: Optional[MoEConfig] = None):
        super().__init__()
        self.config = config or MoEConfig()
        if not 1 <= num_experts <= ops.MOE_MAX_EXPERTS:
            raise ValueError(f"num_experts must be in [1, {ops.MOE_MAX_EXPERTS}], got {num_experts}")
        if not 1 <= top_k <= min(num_experts, ops.MOE_MAX_TOP_K):
            raise ValueError(f"top_k must be in [1, min(num_experts, {ops.MOE_MAX_TOP_K})], got {top_k}")
        if self.config.activation not in ops._ACT:
            raise ValueError(f"Unsupported activation function: {self.config.activation}")
        if self.config.expert_weights_fp8 and (hidden_size % 16 or intermediate_size % 16):
            raise ValueError(f"expert_weights_fp8 needs hidden_size and intermediate_size to be multiples of 16 (the FP8 kernels' "
                             f"16-byte weight loads), got {hidden_size} and {intermediate_size}")
        if self.config.expert_weights_mxfp4:
            if self.config.expert_weights_fp8:
                raise ValueError("expert_weights_mxfp4 and expert_weights_fp8 are exclusive")
            if hidden_size % 32 or intermediate_size % 32:
                raise ValueError(f"expert_weights_mxfp4 needs hidden_size and intermediate_size to be multiples of 32 (whole MX "
                                 f"blocks), got {hidden_size} and {intermediate_size}")
            if self.config.dtype != torch.bfloat16:
                raise ValueError("expert_weights_mxfp4 needs dtype bf16: e2m1 x 2^e is not exact in fp16 outside a narrow exponent range")
        self._mxfp4 = False  # load_mxfp4_experts: pre-quantised bytes, held as buffers, stand in place of the 16-bit expert parameters
        self.hidden_size, self.intermediate_size = hidden_size, intermediate_size
        self.num_experts, self.top_k = num_experts, top_k
        self.router = nn.Linear(hidden_size, num_experts, bias=False)
        E, I, d = num_experts, intermediate_size, hidden_size

        def stacked(n, k):
            w = torch.empty(E, n, k)
            nn.init.uniform_(w, -k ** -0.5, k ** -0.5)  # nn.Linear's range
            return nn.Parameter(w)

        self.w_up = stacked(I, d)
        if self.config.activation == "swiglu":
            self.w_gate = stacked(I, d)
        else:
            self.register_parameter("w_gate", None)
        self.w_down = stacked(d, I)
        self._cast = CastCache()

    def _router_logits(self, x: torch.Tensor, dt: torch.dtype) -> torch.Tensor:
        """router(x) [T, E]: the decode-step GEMM where ops.gemm_skinny_ok advises it (at most 64 rows), else ops.gemm_bias_act.
        Where E is no multiple of 8 the GEMM runs on a copy of the router weight with zero rows up to the next multiple (made once
        per version of the parameter), so its output rows keep the 16-byte stride both GEMMs write at; the logits are the
        first E columns of that, which ops.moe_route takes by its row stride."""
        E = self.num_experts
        w = self._cast.get_row_padded(self.router.weight, dt, 8)
        gemm = ops.gemm_skinny if ops.gemm_skinny_ok(x.shape[0], w.shape[0], w.shape[1], "none") else ops.gemm_bias_act
        return gemm(x, w)[:, :E]

    def forward(self, hidden_states: torch.Tensor, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
        """hidden_states [..., d] (flattened to [T, d]); residual of the same shape is added inside the combine's one rounding.
        T <= 64 is one routing and one pass over the active experts' weights.  T > 64 runs the same path in row chunks of 64: correct,
        without host synchronisation, but every chunk streams its experts' weights again -- unless config.grouped_prefill is on:
        then T > 64 is one router GEMM, one ops.moe_route_prefill and one ops.moe_mlp_prefill per 8192 rows.  With
        config.expert_weights_fp8 the decode path (T <= 64 and the row chunks) reads the FP8 copies of the expert weights; the
        grouped prefill path reads the 16-bit weights -- or, after load_mxfp4_experts, the loaded bytes through
        ops.moe_mlp_prefill_w4."""
        if not hidden_states.is_cuda:
            raise ValueError("Input tensor must be on a CUDA device for the HIP kernels")
        d = self.hidden_size
        if hidden_states.shape[-1] != d:
            raise ValueError(f"Expected hidden size {d}, got shape: {tuple(hidden_states.shape)}")
        if residual is not None and residual.shape != hidden_states.shape:
            raise ValueError("residual must have the shape of hidden_states")
        in_dtype, dt, c = hidden_states.dtype, self.config.dtype, self._cast
        x = as_dtype(hidden_states, dt).reshape(-1, d)
        r = None if residual is None else as_dtype(residual, dt).reshape(-1, d)
        T = x.shape[0]
        out = ops.empty_rows8(T, d, dt, x.device)
        # the path, chosen once on the whole T (a short last chunk of a tall input stays on the prefill ops): its chunk length,
        # its route and MLP ops, and the weights under the names that MLP op takes them by
        prefill = self.config.grouped_prefill and T > ops.MOE_MAX_TOKENS
        if self._mxfp4 or (self.config.expert_weights_mxfp4 and not prefill):
            # (loaded MXFP4 bytes are the only expert weights there are: their tall inputs run the tiled path on those bytes)
            chunk, route_op, mlp_op = ((ops.MOE_PREFILL_MAX_TOKENS, ops.moe_route_prefill, ops.moe_mlp_prefill_w4) if prefill
                                       else (ops.MOE_MAX_TOKENS, ops.moe_route, ops.moe_mlp_w4))
            if dt != torch.bfloat16:
                raise ValueError("MXFP4 expert weights need dtype bf16")
            if self._mxfp4:
                weights = {name: getattr(self, "mxfp4_" + name) for name in _MXFP4_NAMES}
            else:
                (q_up, s_up), (q_down, s_down) = c.get_experts_mxfp4(self.w_up, dt), c.get_experts_mxfp4(self.w_down, dt)
                q_gate, s_gate = c.get_experts_mxfp4(self.w_gate, dt) if self.w_gate is not None else (None, None)
                weights = dict(w4_up=q_up, s_up=s_up, w4_down=q_down, s_down=s_down, w4_gate=q_gate, s_gate=s_gate)
        elif self.config.expert_weights_fp8 and not prefill:
            chunk, route_op, mlp_op = ops.MOE_MAX_TOKENS, ops.moe_route, ops.moe_mlp_w8
            (q_up, s_up), (q_down, s_down) = c.get_experts_w8(self.w_up, dt), c.get_experts_w8(self.w_down, dt)
            q_gate, s_gate = c.get_experts_w8(self.w_gate, dt) if self.w_gate is not None else (None, None)
            weights = dict(w8_up=q_up, s_up=s_up, w8_down=q_down, s_down=s_down, w8_gate=q_gate, s_gate=s_gate)
        else:
            chunk, route_op, mlp_op = ((ops.MOE_PREFILL_MAX_TOKENS, ops.moe_route_prefill, ops.moe_mlp_prefill) if prefill
                                       else (ops.MOE_MAX_TOKENS, ops.moe_route, ops.moe_mlp))
            weights = dict(w_up=c.get(self.w_up, dt), w_down=c.get(self.w_down, dt),
                           w_gate=c.get(self.w_gate, dt) if self.w_gate is not None else None)
        for lo in range(0, T, chunk):
            hi = min(T, lo + chunk)
            xc = x[lo:hi]
            route = route_op(self._router_logits(xc, dt), self.top_k, self.config.renormalize)
            mlp_op(xc, route, act=self.config.activation, **weights, residual=None if r is None else r[lo:hi], out=out[lo:hi])
        return as_dtype(out.reshape(*hidden_states.shape[:-1], d), in_dtype)

    def load_mxfp4_experts(self, blocks_up, scales_up, blocks_gate, scales_gate, blocks_down, scales_down) -> None:
        """Take pre-quantised MXFP4 expert weights as they are: blocks uint8 [E, N, K / 2] (or [E, N, K / 32, 16], taken by view),
        e2m1 nibbles with element 2 i in the low nibble of byte i, and scales uint8 e8m0 [E, N, K / 32]; N, K = I, d for up and
        gate, d, I for down; the gate pair is None where the activation is not swiglu.  The module then holds no 16-bit expert
        weights (w_up, w_gate and w_down become None): T <= 64 is the decode path on these bytes (ops.moe_mlp_w4); T > 64 goes
        through it in row chunks of 64, or with config.grouped_prefill through the tiled path on the same bytes
        (ops.moe_route_prefill, ops.moe_mlp_prefill_w4) per 8192 rows; config.dtype must be bf16.  The tensors are kept, not copied, where the kernels can take them as they lie, as
        non-persistent buffers mxfp4_w4_up, mxfp4_s_up, ...: module.to(device) moves them, state_dict() does not hold them (a
        checkpoint of such a module is the bytes it was loaded from), and load_from_expert_state_dict is refused afterwards."""
        E, I, d = self.num_experts, self.intermediate_size, self.hidden_size
        if d % 32 or I % 32 or self.config.dtype != torch.bfloat16:
            raise ValueError("MXFP4 expert weights need hidden_size and intermediate_size to be multiples of 32 and dtype bf16")
        if (blocks_gate is not None) != (self.config.activation == "swiglu") or (blocks_gate is None) != (scales_gate is None):
            raise ValueError("the gate blocks and scales are given together, with activation 'swiglu' only")

        def take(blocks, scales, N, K, name):
            if blocks is None:
                return None, None
            if blocks.dim() == 4 and tuple(blocks.shape) == (E, N, K // 32, 16):
                blocks = blocks.reshape(E, N, K // 2)
            if tuple(blocks.shape) != (E, N, K // 2) or tuple(scales.shape) != (E, N, K // 32):
                raise ValueError(f"{name}: expected blocks {(E, N, K // 2)} (or {(E, N, K // 32, 16)}) and scales {(E, N, K // 32)}, got "
                                 f"{tuple(blocks.shape)} and {tuple(scales.shape)}")
            return ops._as_bytes(blocks, name + " blocks"), ops._moe_scales(ops._MOE_DECODE_W4, scales, E, N, K, name + " scales", "load_mxfp4_experts")

        (q_up, s_up), (q_gate, s_gate), (q_down, s_down) = (take(blocks_up, scales_up, I, d, "up"), take(blocks_gate, scales_gate, I, d, "gate"),
                                                            take(blocks_down, scales_down, d, I, "down"))
        for name, t in zip(_MXFP4_NAMES, (q_up, s_up, q_down, s_down, q_gate, s_gate)):
            self.register_buffer("mxfp4_" + name, t, persistent=False)
        self._mxfp4 = True
        self.w_up = self.w_gate = self.w_down = None

    def load_from_expert_state_dict(self, state_dict: Dict[str, torch.Tensor], prefix: str = "", gate: str = "gate.weight",
                                    expert: str = "experts.{e}", names: Sequence[str] = ("w1", "w3", "w2")) -> None:
        """Stack per-expert weights into this module's parameters.  Keys: {prefix}{gate} is the router [E, d]; expert e's
        projections are {prefix}{expert.format(e=e)}.{name}.weight with names = (gate projection [I, d], up projection [I, d],
        down projection [d, I]).  The defaults are HF Mixtral's layout (block_sparse_moe.gate, experts.N.w1 / w3 / w2); Qwen-MoE
        is gate="gate.weight", names=("gate_proj", "up_proj", "down_proj").  Without a gate weight (activation != "swiglu") the
        first name is not read.  KeyError for a missing key, ValueError for a wrong shape."""
        if self._mxfp4:
            raise ValueError("this module holds MXFP4 expert bytes (load_mxfp4_experts) and no 16-bit expert parameters to load into")
        n_gate, n_up, n_down = names

        def take(key, shape):
            t = state_dict[key]
            if tuple(t.shape) != tuple(shape):
                raise ValueError(f"{key} has shape {tuple(t.shape)}, expected {tuple(shape)}")
            return t

        E, I, d = self.num_experts, self.intermediate_size, self.hidden_size
        with torch.no_grad():
            self.router.weight.copy_(take(f"{prefix}{gate}", (E, d)))
            for e in range(E):
                base = f"{prefix}{expert.format(e=e)}."
                self.w_up[e].copy_(take(f"{base}{n_up}.weight", (I, d)))
                self.w_down[e].copy_(take(f"{base}{n_down}.weight", (d, I)))
                if self.w_gate is not None:
                    self.w_gate[e].copy_(take(f"{base}{n_gate}.weight", (I, d)))

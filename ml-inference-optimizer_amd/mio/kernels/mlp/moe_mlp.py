"""Mixture-of-experts MLP for decode steps on the HIP kernels (not a reference module: its models are dense).

MoEMLP replaces the MLP of a Mixtral / Qwen-MoE / OLMoE class block: a router (one linear layer to E logits per token), the
top_k experts of every token, and the weighted sum of those experts' MLPs.  forward() is the router GEMM, ops.moe_route and
ops.moe_mlp (the grouped up projection, then the grouped down projection with the combine): four to six launches whatever E is,
the routing device data from start to end, so a step can be captured in a graph.  There is no PyTorch path: CPU tensors raise
ValueError as the other modules do.
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
    top_k softmax weights divided by their sum (Mixtral, Qwen3-MoE: True; OLMoE, Qwen2-MoE: False).  dtype: the compute dtype."""
    activation: str = "swiglu"
    renormalize: bool = True
    dtype: torch.dtype = torch.bfloat16


class MoEMLP(nn.Module):
    """y[t] = sum_j w[t, j] * expert_{ids[t, j]}(x[t]) (+ residual[t]) with (ids, w) = top_k of softmax(router(x[t])).

    Parameters: router.weight [E, d]; w_up [E, I, d], w_gate [E, I, d] (swiglu only), w_down [E, d, I], stacked per expert; no
    biases.  A parameter stored in another dtype than config.dtype is cast once per version (CastCache), so an in-place update is
    seen by the next forward."""

    def __init__(self, hidden_size: int, intermediate_size: int, num_experts: int, top_k: int, config: Optional[MoEConfig] = None):
        super().__init__()
        self.config = config or MoEConfig()
        if not 1 <= num_experts <= ops.MOE_MAX_EXPERTS:
            raise ValueError(f"num_experts must be in [1, {ops.MOE_MAX_EXPERTS}], got {num_experts}")
        if not 1 <= top_k <= min(num_experts, ops.MOE_MAX_TOP_K):
            raise ValueError(f"top_k must be in [1, min(num_experts, {ops.MOE_MAX_TOP_K})], got {top_k}")
        if self.config.activation not in ops._ACT:
            raise ValueError(f"Unsupported activation function: {self.config.activation}")
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
        """router(x) [T, E] for at most 64 rows: the decode-step GEMM where ops.gemm_skinny_ok advises it, else ops.gemm_bias_act.
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
        without host synchronisation, but every chunk streams its experts' weights again -- a prefill-grade grouped GEMM is out of
        scope."""
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
        w_up, w_down = c.get(self.w_up, dt), c.get(self.w_down, dt)
        w_gate = c.get(self.w_gate, dt) if self.w_gate is not None else None
        out = torch.empty(T, ops._pad8(d), dtype=dt, device=x.device)[:, :d]
        for lo in range(0, T, ops.MOE_MAX_TOKENS):
            hi = min(T, lo + ops.MOE_MAX_TOKENS)
            xc = x[lo:hi]
            route = ops.moe_route(self._router_logits(xc, dt), self.top_k, self.config.renormalize)
            ops.moe_mlp(xc, route, w_up, w_down, self.config.activation, w_gate, residual=None if r is None else r[lo:hi],
                        out=out[lo:hi])
        return as_dtype(out.reshape(*hidden_states.shape[:-1], d), in_dtype)

    def load_from_expert_state_dict(self, state_dict: Dict[str, torch.Tensor], prefix: str = "", gate: str = "gate.weight",
                                    expert: str = "experts.{e}", names: Sequence[str] = ("w1", "w3", "w2")) -> None:
        """Stack per-expert weights into this module's parameters.  Keys: {prefix}{gate} is the router [E, d]; expert e's
        projections are {prefix}{expert.format(e=e)}.{name}.weight with names = (gate projection [I, d], up projection [I, d],
        down projection [d, I]).  The defaults are HF Mixtral's layout (block_sparse_moe.gate, experts.N.w1 / w3 / w2); Qwen-MoE
        is gate="gate.weight", names=("gate_proj", "up_proj", "down_proj").  Without a gate weight (activation != "swiglu") the
        first name is not read.  KeyError for a missing key, ValueError for a wrong shape."""
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

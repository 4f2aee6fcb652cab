"""Megatron-style tensor parallelism on the HIP GEMM/attention kernels + RCCL all-reduce.

Mirrors reference parallelism/tensor_parallel.py: TensorParallelConfig (:16-85), ColumnParallelLinear
(:88-204), RowParallelLinear (:207-327, the all-reduce at :302), TensorParallelMLP (:330-400),
TensorParallelAttention (:403-614), ModelParallelConverter (:617-815).

Differences that are deliberate: converted blocks COPY the original weights (the
reference's are randomly initialised), the all-reduce runs on the tensor-parallel GROUP (the reference
uses WORLD), and RowParallelLinear overlaps it with compute: the row-parallel GEMM is cut into row chunks
and chunk i's all-reduce (RCCL's own stream) runs under chunk i+1's GEMM -- a TP pair on MI355X is
bound by one ~153 GB/s xGMI link, so a 64 MiB activation costs about as much as the GEMM that made it.
"""
from __future__ import annotations

import copy
import math
from typing import Callable, List, Optional, Tuple, Union

import torch
import torch.nn as nn
import torch.nn.functional as F

from .._nn import CastCache, attention_plan
from . import _local
from . import communication as comm
from .parallel_utils import attention_projections, divide, set_tensor_model_parallel_attributes, split_tensor_along_dim


class TensorParallelConfig:
    """Fields as reference :16-63; get_tp_group() returns the real group (a placeholder there, :65-75)."""

    def __init__(self, world_size: int = 1, tp_size: int = 1, dp_size: Optional[int] = None, parallel_dim: int = -1,
                 gather_output: bool = True, recompute_activation: bool = False,
                 communication_dtype: torch.dtype = torch.float16, sequence_parallel: bool = False,
                 gradient_accumulation_steps: int = 1, use_cpu_initialization: bool = False,
                 overlap_chunks: int = 4):
        self.world_size = world_size
        self.tp_size = tp_size
        if dp_size is None:
            assert world_size % tp_size == 0, "World size must be divisible by tensor parallel size"
            self.dp_size = world_size // tp_size
        else:
            self.dp_size = dp_size
            assert world_size == tp_size * dp_size, "World size must equal tp_size * dp_size"
        self.parallel_dim = parallel_dim
        self.gather_output = gather_output
        self.recompute_activation = recompute_activation
        self.communication_dtype = communication_dtype
        self.sequence_parallel = sequence_parallel
        self.gradient_accumulation_steps = gradient_accumulation_steps
        self.use_cpu_initialization = use_cpu_initialization
        self.overlap_chunks = overlap_chunks  # row chunks of the GEMM -> all-reduce pipeline (1 = no overlap)

    def get_tp_group(self):
        if self.tp_size == 1 or not torch.distributed.is_initialized():
            return None
        return comm.setup_device_groups(self.world_size, self.tp_size)

    def get_dp_group(self):
        return None

    def tp_rank(self) -> int:
        """Rank inside the tensor-parallel group (the group is asked: adjacent ranks by default, the registered mesh
        group after parallel_utils.initialize_parallel_groups)."""
        if self.tp_size == 1 or not torch.distributed.is_initialized():
            return 0
        g = self.get_tp_group()
        return torch.distributed.get_rank(g) if g is not None else comm.get_rank() % self.tp_size


class ColumnParallelLinear(nn.Module):
    """weight [out/tp, in] (reference :88-204)."""

    def __init__(self, in_features: int, out_features: int, bias: bool = True,
                 config: Optional[TensorParallelConfig] = None, gather_output: Optional[bool] = None, stride: int = 1,
                 skip_bias_add: bool = False):
        super().__init__()
        self.config = config or TensorParallelConfig()
        self.in_features, self.out_features = in_features, out_features
        self.output_size_per_partition = divide(out_features, self.config.tp_size)
        self.weight = nn.Parameter(torch.empty(self.output_size_per_partition, in_features))
        self.bias = nn.Parameter(torch.empty(self.output_size_per_partition)) if bias else None
        self.reset_parameters()
        set_tensor_model_parallel_attributes(self.weight, True, 0, stride)
        if self.bias is not None:
            set_tensor_model_parallel_attributes(self.bias, True, 0, stride)
        self.gather_output = gather_output if gather_output is not None else self.config.gather_output
        self.skip_bias_add = skip_bias_add
        self.activation = "none"  # fused epilogue when followed by an activation (TensorParallelMLP)
        self._cast = CastCache()

    def reset_parameters(self):
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if self.bias is not None:
            bound = 1 / math.sqrt(self.in_features)
            nn.init.uniform_(self.bias, -bound, bound)

    def forward(self, input: torch.Tensor):
        fuse_bias = self.bias is not None and not self.skip_bias_add
        out = _local.cached_linear(self._cast, input, self.weight, self.bias if fuse_bias else None, self.activation)
        if self.gather_output and self.config.tp_size > 1:
            out = comm.all_gather(out, dim=-1, group=self.config.get_tp_group())
        if self.bias is not None and self.skip_bias_add:
            return out, self.bias
        return out

    def get_master_weight(self) -> torch.Tensor:
        if self.config.tp_size == 1:
            return self.weight
        return comm.all_gather(self.weight.detach(), dim=0, group=self.config.get_tp_group())


class RowParallelLinear(nn.Module):
    """weight [out, in/tp]; all-reduce SUM after the local GEMM, bias added once (reference :207-327)."""

    def __init__(self, in_features: int, out_features: int, bias: bool = True,
                 config: Optional[TensorParallelConfig] = None, input_is_parallel: bool = False, stride: int = 1,
                 skip_bias_add: bool = False):
        super().__init__()
        self.config = config or TensorParallelConfig()
        self.in_features, self.out_features = in_features, out_features
        self.input_size_per_partition = divide(in_features, self.config.tp_size)
        self.weight = nn.Parameter(torch.empty(out_features, self.input_size_per_partition))
        self.bias = nn.Parameter(torch.empty(out_features)) if bias else None
        self.reset_parameters()
        set_tensor_model_parallel_attributes(self.weight, True, 1, stride)
        if self.bias is not None:
            set_tensor_model_parallel_attributes(self.bias, False, 0, 1)
        self.input_is_parallel = input_is_parallel
        self.skip_bias_add = skip_bias_add
        self._cast = CastCache()

    def reset_parameters(self):
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if self.bias is not None:
            bound = 1 / math.sqrt(self.in_features) / self.config.tp_size
            nn.init.uniform_(self.bias, -bound, bound)

    def forward(self, input: torch.Tensor, residual: Optional[torch.Tensor] = None):
        cfg = self.config
        tp = cfg.tp_size
        rank = cfg.tp_rank()
        if not self.input_is_parallel and tp > 1:
            input = split_tensor_along_dim(input, dim=-1, num_partitions=tp)[rank]
        # bias (+ residual) enter the sum exactly once: fused into rank 0's GEMM epilogue (reference adds
        # the bias after the reduce, :304-308 -- same value, one pass over the activation fewer)
        add_here = (rank == 0)
        bias = self.bias if (self.bias is not None and not self.skip_bias_add and add_here) else None
        res = residual if add_here else None
        if not torch.distributed.is_initialized() or (tp == 1 and not comm.FORCE_SINGLE_RANK_COLLECTIVES):
            out = _local.cached_linear(self._cast, input, self.weight, bias, "none", res)
        else:
            group = cfg.get_tp_group()
            x2 = input.reshape(-1, input.shape[-1])
            r2 = None if res is None else res.reshape(-1, self.out_features)
            M = x2.shape[0]
            n = max(1, min(cfg.overlap_chunks, M // 256 if M >= 512 else 1))
            out2 = torch.empty(M, self.out_features, dtype=input.dtype, device=input.device)
            bounds = [(i * M) // n for i in range(n + 1)]
            works = []
            for i in range(n):
                a, b = bounds[i], bounds[i + 1]
                _local.cached_linear(self._cast, x2[a:b], self.weight, bias, "none", None if r2 is None else r2[a:b], out=out2[a:b])
                works.append(torch.distributed.all_reduce(out2[a:b], group=group, async_op=True))
            for w in works:
                w.wait()  # stream-level wait on GPU; the host does not block
            out = out2.view(*input.shape[:-1], self.out_features)
        if self.bias is not None and self.skip_bias_add:
            return out, self.bias
        return out

    def get_master_weight(self) -> torch.Tensor:
        if self.config.tp_size == 1:
            return self.weight
        return comm.all_gather(self.weight.detach(), dim=1, group=self.config.get_tp_group())


_ACT_NAMES = {F.gelu: "gelu_erf", F.relu: "relu", F.silu: "silu"}


class TensorParallelMLP(nn.Module):
    """Column-parallel fc1 (+ fused activation) -> row-parallel fc2 (+ all-reduce) (reference :330-400)."""

    def __init__(self, hidden_size: int, intermediate_size: int, config: Optional[TensorParallelConfig] = None,
                 activation: Union[Callable, str] = F.gelu):
        super().__init__()
        self.config = config or TensorParallelConfig()
        self.dense_h_to_4h = ColumnParallelLinear(hidden_size, intermediate_size, bias=True, config=self.config,
                                                  gather_output=False)
        self.dense_4h_to_h = RowParallelLinear(intermediate_size, hidden_size, bias=True, config=self.config,
                                               input_is_parallel=True)
        self.activation = activation
        if isinstance(activation, str):
            self.dense_h_to_4h.activation = activation
        elif activation in _ACT_NAMES:
            self.dense_h_to_4h.activation = _ACT_NAMES[activation]
        else:
            raise ValueError("activation must be F.gelu / F.relu / F.silu or a kernel activation name")

    def forward(self, hidden_states: torch.Tensor, residual: Optional[torch.Tensor] = None,
                pre_norm: Optional[nn.LayerNorm] = None) -> torch.Tensor:
        """pre_norm (not in the reference): the pre-LN block's `mlp(ln(x))` in one call, as FusedMLP.forward takes it."""
        if pre_norm is not None:
            hidden_states = _local.prenorm(hidden_states, pre_norm, self.dense_h_to_4h._cast)
        return self.dense_4h_to_h(self.dense_h_to_4h(hidden_states), residual=residual)


class TensorParallelAttention(nn.Module):
    """H/tp local heads: column-parallel q/k/v, tiled attention, row-parallel out-proj (reference :403-614).
    The three projections keep the reference's parameter names (query / key / value) but run as ONE GEMM on the
    concatenated local weight [3 * H/tp * D, hidden] (k + v only for cross attention): at tp = 4 a single projection is
    N = 256 -- one tile column, which cannot fill 256 CUs -- and the activation is read once instead of three times.
    The reference's `self.key = self.value = self.query` aliasing (:480-483) is not reproduced."""

    def __init__(self, hidden_size: int, num_attention_heads: int, config: Optional[TensorParallelConfig] = None,
                 attention_dropout: float = 0.0, head_dim: Optional[int] = None, is_cross_attention: bool = False,
                 causal: bool = False):
        super().__init__()
        self.config = config or TensorParallelConfig()
        tp = self.config.tp_size
        self.hidden_size, self.num_attention_heads = hidden_size, num_attention_heads
        self.is_cross_attention = is_cross_attention
        self.num_heads_per_partition = divide(num_attention_heads, tp)
        self.head_dim = head_dim if head_dim is not None else hidden_size // num_attention_heads
        self.attention_head_size = self.head_dim
        all_head = num_attention_heads * self.head_dim
        self.query = ColumnParallelLinear(hidden_size, all_head, config=self.config, gather_output=False)
        self.key = ColumnParallelLinear(hidden_size, all_head, config=self.config, gather_output=False)
        self.value = ColumnParallelLinear(hidden_size, all_head, config=self.config, gather_output=False)
        self.output = RowParallelLinear(all_head, hidden_size, config=self.config, input_is_parallel=True)
        self.causal = causal
        if attention_dropout and attention_dropout > 0:
            self.dropout_p = attention_dropout
        else:
            self.dropout_p = 0.0
        self._cast = CastCache()

    def _fused_linear(self, x: torch.Tensor, lins: Tuple[ColumnParallelLinear, ...], col_scale=None) -> torch.Tensor:
        """ONE GEMM on the row-concatenation of the local projections `lins`; the concatenated weight and bias and the weight's
        blocked form are kept in this module's cache until a parameter changes."""
        ws, dt = tuple(l.weight for l in lins), lins[0].weight.dtype
        return _local.cached_linear(self._cast, x, self._cast.get_cat(ws, dt), self._cast.get_cat(tuple(l.bias for l in lins), dt),
                                    col_scale=col_scale, parts=ws)

    def forward(self, hidden_states: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
                encoder_hidden_states: Optional[torch.Tensor] = None,
                residual: Optional[torch.Tensor] = None, pre_norm: Optional[nn.LayerNorm] = None) -> torch.Tensor:
        if self.training and self.dropout_p > 0:
            raise NotImplementedError("attention dropout (training) is not supported by the inference kernel")
        if pre_norm is not None:
            hidden_states = _local.prenorm(hidden_states, pre_norm, self._cast)
        B, S, _ = hidden_states.shape
        Hl, D = self.num_heads_per_partition, self.head_dim
        kv_in = encoder_hidden_states if (self.is_cross_attention and encoder_hidden_states is not None) else hidden_states
        n = Hl * D
        Sk = kv_in.shape[1]
        kpre = False
        if kv_in is hidden_states:  # self attention: one [3 n, hidden] GEMM, q / k / v are strided views of its result
            # where both kernels can (_nn.attention_plan): the K columns [n, 2n) leave the GEMM multiplied by softmax_scale * log2(e)
            # (one rounding) and the attention launch drops its per-score multiply (ops.fa3_fwd k_prescaled)
            plan = attention_plan(B, S, S, Hl, Hl, D, (B * S, 3 * n, hidden_states.shape[-1]), (n, 2 * n), 3 * n,
                                  mask=attention_mask is not None)
            kpre = plan.kpre
            qkv = self._fused_linear(hidden_states, (self.query, self.key, self.value), plan.col_scale)
            q, k, v = (qkv[..., i * n:(i + 1) * n].view(B, S, Hl, D) for i in range(3))
        else:  # cross attention: K stays unscaled
            q = self.query(hidden_states).view(B, S, Hl, D)
            kv = self._fused_linear(kv_in, (self.key, self.value))
            k, v = (kv[..., i * n:(i + 1) * n].view(B, Sk, Hl, D) for i in range(2))
        add = None
        if attention_mask is not None:  # additive [B,1,Sq,Sk] / [B,1,1,Sk] like the reference (:560-566)
            add = attention_mask
            while add.dim() < 4:
                add = add.unsqueeze(1)
        ctx = _local.attention_step(q, k, v, layout="bshd", causal=self.causal, additive_mask=add,
                                    **({"k_prescaled": True} if kpre else {}))
        return self.output(ctx.reshape(B, S, Hl * D), residual=residual)


class ModelParallelConverter:
    """Swap Linear / MLP / attention blocks for their tensor-parallel forms, slicing and COPYING the
    original weights for this rank (reference :617-815 leaves new blocks randomly initialised)."""

    def __init__(self, config: Optional[TensorParallelConfig] = None):
        self.config = config or TensorParallelConfig()

    def convert_model(self, model: nn.Module) -> nn.Module:
        model_tp = copy.deepcopy(model)
        self._convert_module(model_tp)
        return model_tp

    # -- slicing helpers
    def _col(self, weight: torch.Tensor, bias: Optional[torch.Tensor], **kw) -> ColumnParallelLinear:
        """This rank's rows of the full [out, in] weight (and bias) as a ColumnParallelLinear."""
        tp, r = self.config.tp_size, self.config.tp_rank()
        new = ColumnParallelLinear(weight.shape[1], weight.shape[0], bias is not None, self.config, **kw)
        new = new.to(device=weight.device, dtype=weight.dtype)
        per = weight.shape[0] // tp
        with torch.no_grad():
            new.weight.copy_(weight[r * per:(r + 1) * per])
            if bias is not None:
                new.bias.copy_(bias[r * per:(r + 1) * per])
        return new

    def _row(self, lin: nn.Linear, **kw) -> RowParallelLinear:
        tp, r = self.config.tp_size, self.config.tp_rank()
        new = RowParallelLinear(lin.in_features, lin.out_features, lin.bias is not None, self.config, **kw)
        new = new.to(device=lin.weight.device, dtype=lin.weight.dtype)
        per = lin.in_features // tp
        with torch.no_grad():
            new.weight.copy_(lin.weight[:, r * per:(r + 1) * per])
            if lin.bias is not None:
                new.bias.copy_(lin.bias)
        return new

    def _convert_module(self, module: nn.Module) -> None:
        from ..kernels.mlp.fused_mlp import FusedMLP, FusedMLPSwiGLU, FusedTransformerMLP
        from ..kernels.attention.flash_attention import FlashAttentionLayer, FlashSelfAttention

        for name, child in list(module.named_children()):
            if isinstance(child, FusedTransformerMLP) and not isinstance(child.mlp, FusedMLPSwiGLU):
                setattr(module, name, self._convert_fused_mlp(child.mlp))
            elif isinstance(child, FusedMLP) and not isinstance(child, FusedMLPSwiGLU):
                setattr(module, name, self._convert_fused_mlp(child))
            elif isinstance(child, (FlashAttentionLayer, FlashSelfAttention)):
                setattr(module, name, self._convert_flash_attention(child))
            elif isinstance(child, nn.Linear):
                # name-suffix heuristic of the reference (:659-667)
                lname = name.lower()
                if any(s in lname for s in ("out_proj", "o_proj", "output", "fc2", "down_proj", "dense_4h_to_h")):
                    setattr(module, name, self._row(child, input_is_parallel=False))
                elif any(s in lname for s in ("q_proj", "k_proj", "v_proj", "query", "key", "value", "fc1", "up_proj",
                                              "gate_proj", "dense_h_to_4h")):
                    setattr(module, name, self._col(child.weight, child.bias, gather_output=True))
            else:
                self._convert_module(child)

    def _convert_fused_mlp(self, mlp) -> TensorParallelMLP:
        act = mlp._kernel_activation()
        d, I = mlp.fc1.in_features, mlp.fc1.out_features
        new = TensorParallelMLP(d, I, self.config, activation=act)
        new.dense_h_to_4h = self._col(mlp.fc1.weight, mlp.fc1.bias, gather_output=False)
        new.dense_h_to_4h.activation = act
        new.dense_4h_to_h = self._row(mlp.fc2, input_is_parallel=True)
        return new

    def _convert_flash_attention(self, att) -> TensorParallelAttention:
        qkv, o_proj = attention_projections(att, "tensor-parallel")
        new = TensorParallelAttention(att.hidden_size, att.num_attention_heads, self.config, causal=att.config.causal)
        for tgt, (w, b) in zip(("query", "key", "value"), qkv):
            setattr(new, tgt, self._col(w, b, gather_output=False))
        new.output = self._row(o_proj, input_is_parallel=True)
        return new

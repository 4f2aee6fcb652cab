"""CPU-only tests: the C-ABI library loads and exports every symbol of include/mio_hip.h, the operator
surface mirrors the reference's names/errors, converters copy weights, host-side helpers."""
import os
import re
import sys

import pytest
import torch
import torch.nn as nn

import _isa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cabi_exports_and_version_match_header():
    """Every symbol include/mio_hip.h declares is exported and bound, and the library reports the header's ABI version:
    106, the version that added mio_fa3_route."""
    from mio import _lib
    hdr = open(os.path.join(ROOT, "include", "mio_hip.h")).read()
    declared = set(re.findall(r"\b(mio_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    for name in declared:
        assert hasattr(_lib.lib, name), name
    assert int(re.search(r"#define MIO_VERSION (\d+)", hdr).group(1)) == 106
    assert _lib.lib.mio_version() == 106
    assert _lib.lib.mio_last_error() is not None  # callable without a GPU


def test_layernorm_fold_eligibility_without_gpu():
    """mio_gemm_ln_ok / mio_ln_stats_bytes are host functions: the shapes of the benchmark stacks take the folded kernels, the
    shapes outside their limits do not (K % 256, more than 8 statistic slots, too few tiles, activations without an instantiation),
    and mio_gemm_ln_bw refuses bad argument combinations before any launch."""
    from mio import _lib
    lib = _lib.lib
    NONE, GELU_TANH, RELU, SWIGLU = _lib.ACT_NONE, 1, _lib.ACT_RELU, _lib.ACT_SWIGLU
    M = 8 * 4096
    assert lib.mio_gemm_ln_ok(M, 3072, 1024, NONE, 1, 0) == 1          # C2 QKV behind ln_1
    assert lib.mio_gemm_ln_ok(M, 4096, 1024, GELU_TANH, 1, 0) == 1     # C2 fc1 behind ln_2
    assert lib.mio_gemm_ln_ok(M, 1024, 1024, NONE, 0, 1) == 1 and lib.mio_gemm_ln_ok(M, 1024, 4096, NONE, 0, 1) == 1  # out-proj, fc2
    assert lib.mio_gemm_ln_ok(M, 5120, 1280, GELU_TANH, 1, 0) == 1 and lib.mio_gemm_ln_ok(M, 1280, 5120, NONE, 0, 1) == 1  # C5
    assert lib.mio_gemm_ln_ok(M, 4096, 1024, SWIGLU, 1, 0) == 1 and lib.mio_gemm_ln_ok(M, 4096, 1024, SWIGLU, 0, 1) == 0
    assert lib.mio_gemm_ln_ok(M, 3072, 1024 + 64, NONE, 1, 0) == 0     # K % 256
    assert lib.mio_gemm_ln_ok(M, 3072, 4096, NONE, 1, 0) == 1          # 16 statistic slots: through mio_ln_stats_reduce
    assert lib.mio_gemm_ln_ok(M, 1024 + 128, 1024, NONE, 0, 1) == 0    # N % 256
    assert lib.mio_gemm_ln_ok(1024, 1024, 1024, NONE, 0, 1) == 0       # 16 tiles: not a 256-tile launch
    assert lib.mio_gemm_ln_ok(M, 3072, 1024, RELU, 1, 0) == 0
    assert lib.mio_gemm_ln_ok(M, 1024, 1024, GELU_TANH, 0, 1) == 0     # statistics come from the plain residual epilogue
    assert lib.mio_ln_stats_bytes(M, 1024) == 4 * M * 8 and lib.mio_ln_stats_bytes(16500, 1280) == 5 * 16640 * 8
    one = 16  # any non-null 16-byte aligned "pointer": validation returns before anything is dereferenced
    assert lib.mio_gemm_ln_bw(one, one, None, None, None, one, M, 1024, 1024, 1024, 1024, 0, NONE, 0, 0, None, 0, 1e-5, one, 0, 0, 1.0, None) != 0
    assert b"residual" in lib.mio_last_error()                         # stats_out without a residual
    assert lib.mio_gemm_ln_bw(one, one, None, None, one, one, M, 3072, 1024, 1024, 3072, 3072, NONE, 0, 0, one, 0, 1e-5, None, 0, 0, 1.0, None) != 0
    assert b"no residual" in lib.mio_last_error()                      # consumer form with a residual
    assert lib.mio_gemm_ln_bw(one, one, None, one, None, one, M, 3072, 1024, 1024, 3072, 0, NONE, 0, 0, None, 0, 1e-5, None, 0, 0, 1.0, None) != 0
    assert b"bias_gate" in lib.mio_last_error()
    assert lib.mio_gemm_ln_bw(one, one, None, None, None, one, M, 3072, 1024, 1024, 3072, 0, NONE, 0, 8, None, 0, 1e-5, None, 0, 0, 1.0, None) != 0
    assert b"flag" in lib.mio_last_error()
    assert lib.mio_gemm_ln_bw(one, one, None, None, None, one, M, 3072, 4096, 4096, 3072, 0, NONE, 0, 0, one, 0, 1e-5, None, 0, 0, 1.0, None) != 0
    assert b"mio_ln_stats_reduce" in lib.mio_last_error()               # 16 slots handed over unreduced
    assert lib.mio_ln_fold_weight(one, 16384, one, None, None, one, one, 1024, 16384, 0, None) != 0 and b"8192" in lib.mio_last_error()
    assert lib.mio_ln_stats_reduce(one, 16, one, 5, M, None) != 0


def _fa_params(*, D=64, Sq=300, Sk=300, H=4, Hkv=4, dtype=0, causal=0, mask_kind=0, row=None, vrow=None, o=True,
               o_acc=False, carry_in=0, kpre=0, oblk=0):
    """mio_fa3_fwd_params_t for a [B,S,H,D] launch with fake 16-byte aligned pointers (nothing is dereferenced)."""
    from mio import _lib
    p = _lib.FaParams()
    one = 16
    p.q = p.k = p.v = one
    p.o = one if o else None
    p.o_acc = one if o_acc else None
    p.lse = one if (o_acc or carry_in) else None
    p.mask = one if mask_kind else None
    krow = H * D if row is None else row
    for st, r in ((p.q_stride, H * D), (p.k_stride, krow), (p.v_stride, krow if vrow is None else vrow), (p.o_stride, H * D)):
        st[0], st[1], st[2] = max(Sq, Sk, 1) * r, r, D
    p.B, p.Sq, p.Sk, p.H, p.Hkv, p.D = 1, Sq, Sk, H, Hkv, D
    p.dtype, p.causal, p.mask_kind, p.carry_in = dtype, causal, mask_kind, carry_in
    p.softmax_scale, p.k_prescaled, p.o_blocked = 0.125, kpre, oblk
    return p


# (geometry, route): every boundary of fa3_pick_route (csrc/fa3_route.h); None = refused (mio_fa3_route < 0)
_ROUTE_TABLE = [
    (dict(), "fwd5"),
    (dict(Sq=129), "fwd5"),
    (dict(Sq=128), "fwd1"),
    (dict(Sq=1), "fwd1"),
    (dict(Sq=0), "empty"),
    (dict(D=8), "fwd5"),
    (dict(D=72), "fwd3"),
    (dict(D=96), "fwd3"),
    (dict(D=104), "fwd3"),
    (dict(D=128), "fwd3"),
    (dict(D=128, Sq=128), "fwd1"),
    (dict(Sk=0), "fwd1"),
    (dict(Sk=1), "fwd5"),
    (dict(D=96, Sk=0), "fwd1"),
    # 32-bit K / V span: Sk * row_stride * 2 just under / at 2^32 (either operand)
    (dict(Sk=(1 << 15) - 1, row=1 << 16), "fwd5"),
    (dict(Sk=1 << 15, row=1 << 16), "fwd1"),
    (dict(Sk=(1 << 15) - 1, row=256, vrow=1 << 16), "fwd5"),
    (dict(Sk=1 << 15, row=256, vrow=1 << 16), "fwd1"),
    (dict(D=96, Sk=1 << 15, row=1 << 16), "fwd1"),
    (dict(D=96, Sk=(1 << 15) - 1, row=1 << 16), "fwd3"),
    # k_prescaled
    (dict(kpre=1), "fwd5_kpre"),
    (dict(kpre=1, D=72), "fwd3_kpre"),
    (dict(kpre=1, D=96), "fwd3_kpre"),
    (dict(kpre=1, D=104), None),
    (dict(kpre=1, Sq=128), None),
    (dict(kpre=1, Sk=0), None),
    (dict(kpre=1, Sk=1 << 15, row=1 << 16), None),
    (dict(kpre=1, mask_kind=1), None),
    (dict(kpre=1, oblk=1), "fwd5_kpre_oblk"),
    (dict(kpre=1, oblk=1, D=40, H=4), "fwd5_kpre_oblk"),
    (dict(kpre=1, oblk=1, D=8, H=3), None),            # (H * D) % 32 != 0
    (dict(kpre=1, oblk=1, D=72), None),
    (dict(oblk=1), None),                              # o_blocked needs k_prescaled
    # the (o_acc, lse) carry
    (dict(o_acc=True), "fwd3"),
    (dict(o_acc=True, o=False), "fwd3"),
    (dict(o_acc=True, carry_in=1, kpre=1), "fwd5_kpre_carry"),
    (dict(o_acc=True, o=False, kpre=1), "fwd5_kpre_carry"),
    (dict(o_acc=True, kpre=1, D=72), None),
    (dict(o_acc=True, kpre=1, oblk=1), None),
    (dict(o_acc=True, D=128, carry_in=1), "fwd3"),
    (dict(o_acc=True, Sq=128, carry_in=1), "fwd1"),
    (dict(o_acc=True, kpre=1, Sq=128), None),
    # user masks: the sequential kernel at every Sq and head dim
    (dict(mask_kind=1), "fwd1_keep"),
    (dict(mask_kind=2), "fwd1_add"),
    (dict(mask_kind=1, Sq=64, D=128), "fwd1_keep"),
    (dict(mask_kind=2, Sq=64, D=96), "fwd1_add"),
    (dict(mask_kind=2, o_acc=True, carry_in=1), "fwd1_add"),
    (dict(mask_kind=2, Sk=0), "fwd1_add"),
    (dict(mask_kind=3), None),
]


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("causal", [0, 1])
def test_fa3_route_table_without_gpu(dtype, causal):
    """mio_fa3_route reports the kernel mio_fa3_fwd launches, through the same rule (fa3_pick_route); every route of
    mio_fa3_route_t appears in the table."""
    import ctypes as C
    from mio import _lib
    seen = set()
    for geom, want in _ROUTE_TABLE:
        r = _lib.lib.mio_fa3_route(C.byref(_fa_params(dtype=dtype, causal=causal, **geom)))
        got = _lib.FA3_ROUTES.get(r) if r >= 0 else None
        assert got == want, f"{geom}: route {got} ({r}), expected {want}"
        if r < 0:
            assert _lib.lib.mio_last_error()
        seen.add(got)
    assert seen == set(_lib.FA3_ROUTES.values()) | {None}
    # invalid arguments are refused like mio_fa3_fwd refuses them
    p = _fa_params(D=60)
    assert _lib.lib.mio_fa3_route(C.byref(p)) < 0 and b"head_dim" in _lib.lib.mio_last_error()
    assert _lib.lib.mio_fa3_route(None) < 0


def test_fa3_route_python_wrapper_without_gpu():
    """ops.fa3_route builds fa3_fwd's parameters (strides of views, mask conversion, k_prescaled / out_blocked checks)
    from tensors on any device and launches nothing."""
    from mio import ops
    q = torch.zeros(1, 300, 2, 64, dtype=torch.bfloat16)
    assert ops.fa3_route(q, q, q) == "fwd5"
    assert ops.fa3_route(q, q, q, k_prescaled=True, out_blocked=True) == "fwd5_kpre_oblk"
    assert ops.fa3_route(q[:, :128], q, q, causal=True) == "fwd1"
    assert ops.fa3_route(q, q, q, additive_mask=torch.zeros(1, 1, 300, 300)) == "fwd1_add"
    assert ops.fa3_route(q, q, q, keep_mask=torch.ones(1, 1, 1, 300, dtype=torch.bool)) == "fwd1_keep"
    acc, lse = torch.zeros(1, 300, 2, 64), torch.zeros(1, 2, 300)
    assert ops.fa3_route(q, q, q, o_acc=acc, lse=lse, write_out=False, k_prescaled=True) == "fwd5_kpre_carry"
    qkv = torch.zeros(1, 300, 3 * 2 * 96, dtype=torch.float16)  # strided views of one fused projection
    qv, kv, vv = (qkv[..., i * 192:(i + 1) * 192].view(1, 300, 2, 96) for i in range(3))
    assert ops.fa3_route(qv, kv, vv) == "fwd3" and ops.fa3_route(qv, kv, vv, k_prescaled=True) == "fwd3_kpre"
    assert ops.fa3_route(q, q[:, :0], q[:, :0]) == "fwd1"
    with pytest.raises(ValueError):
        ops.fa3_route(q, q, q, additive_mask=torch.zeros(1, 1, 300, 300), k_prescaled=True)


def test_cabi_argument_errors_without_gpu():
    """Validation happens before any launch, so bad arguments are reportable without a device."""
    import ctypes as C
    from mio import _lib
    p = _lib.FaParams()
    assert _lib.lib.mio_fa3_fwd(C.byref(p), None) != 0
    assert b"non-null" in _lib.lib.mio_last_error()
    assert _lib.lib.mio_gemm_bias_act(None, None, None, None, None, None, None, 1, 8, 8, 8, 8, 8, 8, 0, 0, None) != 0
    with pytest.raises(RuntimeError):
        _lib.check(-1)


def test_no_cpu_fallback():
    from mio import ops
    from mio.kernels.mlp import FusedTransformerMLP
    from mio.kernels.attention import FlashAttention3, FlashSelfAttention
    x = torch.randn(1, 4, 64)
    with pytest.raises(ValueError):
        FusedTransformerMLP(64, 128)(x)
    with pytest.raises(ValueError):
        FlashSelfAttention(64, 4)(x)
    q = torch.randn(1, 4, 2, 32)
    with pytest.raises(ValueError):
        FlashAttention3()(q, q, q)
    with pytest.raises(ValueError):
        ops.flash_attention(q, q, q)
    with pytest.raises(ValueError):
        FlashAttention3()(q[0], q, q)  # rank check first, like flash_attention.py:167


def test_configs_mirror_reference():
    from mio.kernels.attention import FlashAttentionConfig
    from mio.kernels.mlp import FusedMLPConfig
    from mio.parallelism import SequenceParallelConfig, TensorParallelConfig
    c = FlashAttentionConfig()
    assert (c.block_size, c.causal, c.softmax_scale, c.dropout_p, c.precision) == (128, False, None, 0.0, "fp16")
    with pytest.raises(ValueError):
        FlashAttentionConfig(precision="int8")
    with pytest.raises(RuntimeError):
        FlashAttentionConfig(precision="fp8")
    m = FusedMLPConfig()
    assert (m.activation_fn, m.dropout_prob, m.precision) == ("gelu", 0.0, "fp16")
    with pytest.raises(ValueError):
        SequenceParallelConfig(world_size=4, sp_size=3)
    with pytest.raises(ValueError):
        SequenceParallelConfig(attention_handling="striped")
    t = TensorParallelConfig(world_size=8, tp_size=2)
    assert t.dp_size == 4
    from mio.kernels.attention import FlashAttentionLayer
    with pytest.raises(ValueError):
        FlashAttentionLayer(100, 3)


def test_module_parameter_names():
    from mio.kernels.attention import FlashAttentionLayer, FlashSelfAttention
    from mio.kernels.mlp import FusedTransformerMLP
    assert set(dict(FlashAttentionLayer(64, 4, num_kv_heads=2).named_parameters())) == {
        f"{p}.{w}" for p in ("q_proj", "k_proj", "v_proj", "o_proj") for w in ("weight", "bias")}
    fs = FlashSelfAttention(64, 4, num_kv_heads=2)
    assert fs.qkv_proj.weight.shape == (64 + 2 * 2 * 16, 64)
    sw = FusedTransformerMLP(64, 128, "swiglu")
    assert {"mlp.fc1.weight", "mlp.fc1_gate.weight", "mlp.fc2.weight"} <= set(dict(sw.named_parameters()))
    assert type(FusedTransformerMLP(64, 128, "gelu").mlp).__name__ == "FusedMLPGeluTanh"
    assert type(FusedTransformerMLP(64, 128, "relu").mlp).__name__ == "FusedMLPReLU"
    assert type(FusedTransformerMLP(64, 128, "silu").mlp).__name__ == "FusedMLP"


def test_converters_copy_weights():
    from oracle.baseline_runner import PlainGPT2Stack
    from ml_inference_optimizer import Optimizer
    from mio.kernels.attention import FlashAttentionLayer
    from mio.kernels.mlp import FusedTransformerMLP
    model = PlainGPT2Stack(64, 4, 2, seed=3)
    ref = {k: v.clone() for k, v in model.state_dict().items()}
    opt = Optimizer(model)
    prof = opt.profile()
    assert prof["attention_modules"] == 2 and prof["mlp_modules"] == 2
    out = opt.optimize(use_flash_attention=True, use_fused_mlp=True, tensor_parallel_size=1, causal=True)
    blk = out.h[0]
    assert isinstance(blk.attn, FlashAttentionLayer) and isinstance(blk.mlp, FusedTransformerMLP)
    assert blk.attn.config.causal is True
    assert torch.equal(blk.attn.q_proj.weight, ref["h.0.attn.q_proj.weight"])
    assert torch.equal(blk.attn.o_proj.bias, ref["h.0.attn.o_proj.bias"])
    assert torch.equal(blk.mlp.mlp.fc1.weight, ref["h.0.mlp.linear1.weight"])
    assert torch.equal(blk.mlp.mlp.fc2.weight, ref["h.0.mlp.linear2.weight"])
    assert type(blk.mlp.mlp).__name__ == "FusedMLPGeluTanh"


def test_converter_llama_and_gpt2_layouts():
    from mio.kernels.mlp import MLPConverter
    from mio.kernels.attention import ModelConverter, FlashSelfAttention

    class LlamaMLP(nn.Module):
        def __init__(self):
            super().__init__()
            self.gate_proj = nn.Linear(32, 64, bias=False)
            self.up_proj = nn.Linear(32, 64, bias=False)
            self.down_proj = nn.Linear(64, 32, bias=False)

    class Conv1D(nn.Module):  # HF GPT-2 layout: weight [in, out]
        def __init__(self, nf, nx):
            super().__init__()
            self.weight = nn.Parameter(torch.randn(nx, nf))
            self.bias = nn.Parameter(torch.randn(nf))

    class GPT2MLP(nn.Module):
        def __init__(self):
            super().__init__()
            self.c_fc, self.c_proj, self.act = Conv1D(64, 32), Conv1D(32, 64), nn.GELU()

    class GPT2Attention(nn.Module):
        def __init__(self):
            super().__init__()
            self.c_attn, self.c_proj = Conv1D(96, 32), Conv1D(32, 32)
            self.num_heads, self.embed_dim = 4, 32

    class Holder(nn.Module):
        def __init__(self):
            super().__init__()
            self.a, self.b, self.attn = LlamaMLP(), GPT2MLP(), GPT2Attention()

    h = Holder()
    src = {k: v.clone() for k, v in h.state_dict().items()}
    MLPConverter().convert_model(h)
    assert torch.equal(h.a.mlp.fc1_gate.weight, src["a.gate_proj.weight"])
    assert torch.equal(h.a.mlp.fc1.weight, src["a.up_proj.weight"])
    assert torch.equal(h.a.mlp.fc2.weight, src["a.down_proj.weight"])
    assert h.a.mlp.fc2.bias.abs().max() == 0
    assert torch.equal(h.b.mlp.fc1.weight, src["b.c_fc.weight"].t())
    assert torch.equal(h.b.mlp.fc2.bias, src["b.c_proj.bias"])
    ModelConverter().convert_model(h)
    assert isinstance(h.attn, FlashSelfAttention) and h.attn.num_attention_heads == 4
    assert torch.equal(h.attn.qkv_proj.weight, src["attn.c_attn.weight"].t())
    assert torch.equal(h.attn.o_proj.weight, src["attn.c_proj.weight"].t())


def test_sequence_helpers():
    from mio.parallelism import partition_sequence, gather_sequence, zigzag_shard, zigzag_unshard
    x = torch.arange(2 * 16 * 3).view(2, 16, 3)
    parts = partition_sequence(x, 4)
    assert len(parts) == 4 and torch.equal(gather_sequence(parts), x)
    with pytest.raises(ValueError):
        partition_sequence(x, 5)
    shards = [zigzag_shard(x, r, 4) for r in range(4)]
    assert torch.equal(shards[0][:, :2], x[:, 0:2]) and torch.equal(shards[0][:, 2:], x[:, 14:16])
    assert torch.equal(zigzag_unshard(shards, 4), x)


def test_comm_wrappers_single_process():
    from mio.parallelism import all_reduce, all_gather, reduce_scatter, ring_exchange, get_rank, get_world_size
    t = torch.ones(3)
    assert get_rank() == 0 and get_world_size() == 1
    assert all_reduce(t) is t and all_gather(t) is t and reduce_scatter(t) is t
    assert ring_exchange(t, None)[0] is t


def test_fusion_registry_host_logic():
    """FusionRegistry API of baseline/inference.py:26-215: pattern matching, non-overlapping candidates, replacement
    inside nn.Sequential and attribute-style parents, weights carried over (module construction is host work)."""
    from mio.baseline.inference import FusionPattern, FusionRegistry, fusion_registry
    from mio.kernels.mlp.fused_mlp import FusedMLP, FusedMLPGeluTanh, FusedMLPReLU
    assert [p.name for p in fusion_registry.patterns] == ["linear_gelu_linear", "linear_relu_linear"]
    seq = nn.Sequential(nn.LayerNorm(8), nn.Linear(8, 32), nn.GELU(approximate="tanh"), nn.Linear(32, 8),
                        nn.Linear(8, 16), nn.ReLU(), nn.Linear(16, 8), nn.Linear(8, 24), nn.GELU(), nn.Linear(24, 6))
    fused = fusion_registry.fuse_modules(seq)
    kinds = [type(m).__name__ for m in fused]
    # the last triple does not map back to its input width (24 -> 6 != 8): left alone
    assert kinds == ["LayerNorm", "FusedMLPGeluTanh", "FusedMLPReLU", "Linear", "GELU", "Linear"]
    assert len(seq) == 10  # not in place by default
    assert torch.equal(fused[1].fc1.weight, seq[1].weight) and torch.equal(fused[2].fc2.bias, seq[6].bias)

    class Blk(nn.Module):
        def __init__(self):
            super().__init__()
            self.fc_in, self.act, self.fc_out = nn.Linear(8, 16), nn.GELU(), nn.Linear(16, 8)
    b = fusion_registry.fuse_modules(Blk(), inplace=True)
    assert isinstance(b.fc_in, FusedMLP) and not isinstance(b.fc_in, (FusedMLPGeluTanh, FusedMLPReLU))
    assert not hasattr(b, "act") and not hasattr(b, "fc_out")

    reg = FusionRegistry()
    reg.register_pattern(FusionPattern("pair", [nn.ReLU, nn.ReLU], lambda ms: nn.Identity()))
    assert reg.find_matching_pattern([nn.ReLU(), nn.ReLU()]).name == "pair"
    assert reg.find_matching_pattern([nn.ReLU(), nn.GELU()]) is None
    assert [type(m).__name__ for m in reg.fuse_modules(nn.Sequential(nn.ReLU(), nn.ReLU(), nn.ReLU()))] == ["Identity", "ReLU"]


def test_paged_kv_cache_allocator():
    """BlockManager / PagedKVCache semantics of baseline/inference.py:1045-1303 (host bookkeeping; cache on CPU here)."""
    from mio.baseline.inference import PagedKVCache
    pc = PagedKVCache(num_blocks=6, block_size=4, num_layers=2, num_heads=2, head_dim=8, dtype=torch.float16, device="cpu")
    k, v = pc.get_physical_caches()
    assert tuple(k.shape) == (6, 2, 4, 2, 8) and tuple(v.shape) == tuple(k.shape)
    pc.allocate_blocks_for_sequence(0, 9)           # 3 blocks
    assert len(pc.get_block_table(0)) == 3 and pc.get_sequence_length(0) == 9
    for _ in range(3):
        pc.append_token(0)                           # 10, 11, 12 -> still 3 blocks
    assert len(pc.get_block_table(0)) == 3 and pc.get_sequence_length(0) == 12
    pc.append_token(0)                               # 13 -> 4th block
    assert len(pc.get_block_table(0)) == 4
    pc.append_token(7)                               # new sequence via append
    assert pc.get_sequence_length(7) == 1 and len(pc.get_block_table(7)) == 1
    assert len(set(pc.get_block_table(0)) | set(pc.get_block_table(7))) == 5
    bt, cl, mx = pc.kernel_metadata([0, 7])
    assert bt.dtype == torch.int32 and tuple(bt.shape) == (2, 4) and cl.tolist() == [13, 1] and mx == 13
    assert bt[0].tolist() == pc.get_block_table(0) and bt[1, 0].item() == pc.get_block_table(7)[0]
    with pytest.raises(MemoryError):                 # 1 block left, 3 needed: raises and frees the sequence
        pc.allocate_blocks_for_sequence(9, 12)
    assert pc.get_sequence_length(9) == 0
    with pytest.raises(ValueError):
        pc.get_block_table(9)
    bm = pc.block_manager
    blk = pc.get_block_table(7)[0]
    bm.increase_ref_count(blk)
    pc.free_sequence(7)
    assert blk not in bm.free_blocks                 # still referenced once
    bm.free_block(blk)
    assert blk in bm.free_blocks
    pc.free_sequence(0)
    u = pc.get_memory_usage()
    assert u["free_physical_blocks"] == 6 and u["active_sequences"] == 0 and u["gpu_cache_k_shape"] == (6, 2, 4, 2, 8)


def test_ring_attention_config_and_shells():
    """RingAttentionConfig validation (ring_attention.py:65-89) and the parameter names of the module shells."""
    from mio.kernels.attention import RingAttentionConfig, RingCrossAttention, RingSelfAttention
    for bad in (dict(world_size=0), dict(chunk_size=0), dict(precision="fp8"), dict(attention_dropout=1.0)):
        with pytest.raises(ValueError):
            RingAttentionConfig(**bad)
    assert RingAttentionConfig(precision="fp16").compute_dtype == torch.float16
    with pytest.raises(ValueError):
        RingSelfAttention(30, 4, RingAttentionConfig())
    fused = RingSelfAttention(32, 4, RingAttentionConfig(fuse_qkv=True))
    split = RingSelfAttention(32, 4, RingAttentionConfig(fuse_qkv=False))
    cross = RingCrossAttention(32, 4, RingAttentionConfig())
    assert {n for n, _ in fused.named_parameters()} == {"qkv_proj.weight", "qkv_proj.bias", "out_proj.weight", "out_proj.bias"}
    names = {"q_proj.weight", "q_proj.bias", "k_proj.weight", "k_proj.bias", "v_proj.weight", "v_proj.bias",
             "out_proj.weight", "out_proj.bias"}
    assert {n for n, _ in split.named_parameters()} == names == {n for n, _ in cross.named_parameters()}
    with pytest.raises(ValueError):  # CPU tensor: no fallback
        cross(torch.zeros(1, 4, 32), torch.zeros(1, 4, 32))


@pytest.mark.parametrize("type_id,D", [(0, 64), (1, 64), (0, 96), (0, 128)])
def test_fwd3_accumulator_registers_untouched_by_compiler(tmp_path, type_id, D):
    """fa3_fwd3_kernel keeps O^T, L, Q and the ones operand in accumulator registers Fa3Map<D>::A_Q .. a255 that only
    its inline asm names.  The allocator does not know they are live between asm statements, so the build is only sound
    if no compiler-generated instruction touches them: check the ISA of every instantiation (tools/check_agpr.py)."""
    text = _isa.fa_isa(tmp_path, "fa3_fwd_inst.hip", type_id, D)
    bodies = _isa.kernels(text, "_Z15fa3_fwd3_kernel")
    assert len(bodies) >= 2, "causal and full instantiations expected"
    for body in bodies:
        _isa.check_agpr(tmp_path, body, _isa.fa3_agpr_floor(D))


def test_fwd5_two_waves_per_simd_fits_without_spills(tmp_path):
    """fa3_fwd5_kernel runs two waves per SIMD: 256 registers per wave.  It must fit them without scratch (a staggered
    variant that did not fit ran 60 % slower) -- check the ISA metadata of both dtypes' causal instantiation."""
    for type_id in (0, 1):
        text = _isa.fa_isa(tmp_path, "fa3_fwd_inst.hip", type_id, 64)
        blocks = _isa.metadata(text, r"_Z15fa3_fwd5_kernel\w+")
        assert len(blocks) >= 8, "fa3_fwd5_kernel: causal / full x {pre-scaled, plain K, ring carry, blocked output}"
        for blk in blocks:
            _isa.check_fits_256(blk)


def _inflight_load_reads(body):
    """Instructions that read (or copy) a register a global_load_dwordx4 is still filling, in a straight-line listing:
    vector-memory operations retire in order, and s_waitcnt vmcnt(N) leaves only the N most recent outstanding.  hipcc
    waits for its own loads before their first use; a hit is a load it cannot see (inline asm) used too early."""
    def regs(tok):
        m = re.fullmatch(r"v\[(\d+):(\d+)\]", tok)
        if m:
            return set(range(int(m.group(1)), int(m.group(2)) + 1))
        m = re.fullmatch(r"v(\d+)", tok)
        return {int(m.group(1))} if m else set()
    queue, hits = [], []  # destination registers of the outstanding vector-memory operations, oldest first
    for line in body:
        s = line.strip()
        if not s or s.startswith((".", ";")):
            continue
        ops = [t.rstrip(",") for t in s.split()[1:]]
        m = re.search(r"vmcnt\((\d+)\)", s) if s.startswith("s_waitcnt") else None
        if m:
            n = int(m.group(1))
            queue = queue[len(queue) - n:] if n else []
            continue
        live = set().union(*queue) if queue else set()
        if live and any(regs(t) & live for t in ops[1:]):
            hits.append(s)
        if re.match(r"(global|buffer|flat)_(load|store|atomic)", s):
            queue.append(regs(ops[0]) if "_load" in s.split()[0] else set())
    return hits


@pytest.mark.parametrize("type_id", [0, 1])
@pytest.mark.parametrize("D", [64, 96, 128])
def test_fwd1_staging_registers_not_moved_in_flight(tmp_path, type_id, D):
    """fa3_fwd_kernel stages K / V tiles with asm loads the compiler cannot see (no s_waitcnt of its own); they are sound
    only while hipcc leaves their destination registers alone until wait_loads().  At D = 128 hipcc copied them into AGPRs
    right after issue (every output of the Sq <= 128 launches wrong); that path now uses compiler-visible loads."""
    bodies = _isa.kernels(_isa.fa_isa(tmp_path, "fa3_fwd_inst.hip", type_id, D), "_Z14fa3_fwd_kernel")
    assert len(bodies) == 6  # causal x mask kind
    for body in bodies:
        hits = _inflight_load_reads(body)
        assert not hits, body[0] + "\n" + "\n".join(hits[:8])


def test_gemm8w_kernel_isa_soundness(tmp_path):
    """(a) gemm8w_kernel (the product's 256x256-tile GEMM, two waves per SIMD, compiler-managed registers): every shipped
    instantiation fits 256 registers without scratch -- a spill inside its K loop would put a vmcnt(0) in front of the
    counted waits."""
    import subprocess
    isa = _isa.device_isa(tmp_path, "gemm_inst.hip", ["GEMM_TYPE_ID=0", "MIO_DIAG"], attention=False)
    full = isa.read_text()
    blocks = _isa.metadata(full, r"_Z13gemm8w_kernel\w+Li0EEv7GemmDev")  # VAR = 0: what the product launches
    assert len(blocks) >= 9, "gemm8w_kernel: 5 plain + 4 residual instantiations (+ SwiGLU) expected"
    for blk in blocks:
        erf = "DF16bLi2E" in blk  # exact-erf GELU: erff() in the read-out may spill a few registers (slow, still correct)
        _isa.check_fits_256(blk, no_spill=not erf)
    # (b) no store whose data registers are rewritten by the very next instruction (tools/check_store_war.py: the hazard
    # behind round 3's wrong lanes -- hipcc leaves no wait state behind a buffer_store with a register soffset)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_store_war.py"), str(isa), "gemm8w_kernel", "1"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout


@pytest.mark.parametrize("n1,n2", [(64, 4), (13, 4), (4, 4), (5, 1), (1, 0), (3, 0), (12, 8), (2, 1), (7, 3), (0, 0)])
def test_fwd5_tile_stream_schedule(n1, n2):
    """Host-side model of fa3_fwd5_kernel's LDS schedule (csrc/fa3_fwd5_kernel.h): the KV tiles of the one or two causal passes
    of a workgroup are one stream of virtual tiles in 8 LDS stages; a wave meets the barrier once per two iterations (waves 0-3
    behind the QK^T half of an even iteration, waves 4-7 in front of it) and requests the next two tiles there.  Checked for
    every wave, whatever its own tile count: (a) all waves execute the same number of barriers, (b) every tile a half reads
    was requested BEFORE an earlier barrier of that wave (so its vmcnt(0) + the barrier made it visible), (c) a request never
    overwrites a stage that some wave may still read, (d) no tile past the stream's end is requested."""
    STAGES = 8
    passes = [n for n in (n1, n2) if True][: (2 if n2 > 0 else 1)]
    total = sum(passes)

    def wave_events(late, n_w_per_pass):
        """-> list of events in program order: ("sync",) | ("read", virtual_tile) ; sync = vmcnt(0) + barrier + 2 requests"""
        ev, tbase = [], 0
        for pi, n_tiles in enumerate(passes):
            n_w = min(n_w_per_pass[pi], n_tiles)
            ev.append(("pass_start", tbase, n_tiles))
            if n_w > 0:
                ev.append(("read", tbase + 0))       # K(0): scores of tile 0
                ev.append(("read", tbase + 1))       # K(1) fragments for iteration 0 (garbage if the pass has one tile)
            for t in range(n_w):
                even = (t % 2 == 0)
                if late and even:
                    ev.append(("sync",))
                ev.append(("read", tbase + t))       # V(t) fragments, requested in the QK^T half
                if (not late) and even:
                    ev.append(("sync",))
                ev.append(("read", tbase + t + 2))   # K(t+2) fragments, requested in the PV half
            for t in range(n_w, n_tiles):
                if t % 2 == 0:
                    ev.append(("sync",))
            tbase += n_tiles
        return ev

    # the shared (wave-uniform) request stream: what each sync / pass start requests
    def requests():
        out, vnext, vseen, tbase = [], 0, 0, 0    # out[k] = tiles requested at the k-th "request point"
        pts = []
        for pi, n_tiles in enumerate(passes):
            nxt = passes[pi + 1] if pi + 1 < len(passes) else 0
            first = []
            while vnext < tbase + 4:
                first.append(vnext); vnext += 1
            need_barrier = vseen < tbase + 2
            if need_barrier:
                vseen = vnext
            pts.append(("pass_start", [v for v in first if v - tbase < n_tiles + nxt], need_barrier))
            for t in range(n_tiles):
                if t % 2 == 0:
                    vseen = vnext
                    pts.append(("sync", [v for v in (vnext, vnext + 1) if v - tbase < n_tiles + nxt], True))
                    vnext += 2
            tbase += n_tiles
        return pts

    pts = requests()
    assert all(v < total for _, vs, _ in pts for v in vs), "a tile past the end of the stream is requested"          # (d)
    assert sorted(v for _, vs, _ in pts for v in vs) == list(range(total)), "every tile is requested exactly once"
    n_sync = sum(1 for kind, _, _ in pts if kind == "sync")
    waves = []
    for late in (False, True):
        for short in (0, 1, 2, 3):
            n_w = [max(0, n - short) for n in passes]
            ev = wave_events(late, n_w)
            assert sum(1 for e in ev if e[0] == "sync") == n_sync                                                    # (a)
            waves.append((late, ev))
    # replay: global order = request points in sequence; a wave's reads between its (k)th and (k+1)th barrier-like point
    for late, ev in waves:
        k = -1                      # index of the last request point this wave has passed
        visible = set()             # tiles requested before the last vmcnt(0)+barrier this wave executed
        pending = set()             # requested by this wave since
        pi = -1
        for e in ev:
            if e[0] == "pass_start":
                k += 1
                kind, vs, barrier = pts[k]
                assert kind == "pass_start"
                if barrier:
                    pending |= set(vs); visible |= pending; pending = set()
                else:
                    pending |= set(vs)
            elif e[0] == "sync":
                k += 1
                kind, vs, _ = pts[k]
                assert kind == "sync"
                visible |= pending; pending = set(vs)
            else:
                v = e[1]
                if v < total:                                                                                      # (b)
                    assert v in visible, f"late={late}: tile {v} read before a barrier made it visible"
    # (c) WAR: when tile v is requested at request point k, every wave that could still read stage v % 8's previous
    # occupant (tile v - 8) must have passed a barrier after its last read of it.  Waves are at most one barrier apart, so:
    # the last read of tile v - 8 by ANY wave happens before that wave's barrier number (k - 1) at the latest.
    order = {}
    for late, ev in waves:
        k = -1
        for e in ev:
            if e[0] in ("pass_start", "sync"):
                k += 1
            elif e[1] < total:
                order[e[1]] = max(order.get(e[1], -1), k)   # read of tile happens after request point k of that wave
    for k, (_, vs, _) in enumerate(pts):
        for v in vs:
            if v - STAGES >= 0 and (v - STAGES) in order:
                # a wave issuing request point k has passed barrier k; another wave may still be before ITS point k only if
                # point k is a barrier for it too (then it has arrived); reads recorded "after point j" with j <= k - 1 are done
                assert order[v - STAGES] <= k - 1, f"tile {v} overwrites tile {v - STAGES} that may still be read"

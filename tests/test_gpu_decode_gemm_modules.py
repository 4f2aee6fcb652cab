"""The modules' decode_gemm option: with it set, the paged branch of FlashSelfAttention / FlashAttentionLayer and the plain-tensor
path of FusedMLP run their linear layers on ops.gemm_skinny (counted through a wrapper; ops.gemm_skinny_ok is patched to say yes
at these tiny shapes, so the kernel is the one under test) and match the fp64 chain; with it off, no call reaches ops.gemm_skinny
and the output bytes are those of a module built without the field."""
import pytest
import torch
import torch.nn.functional as F

import oracle

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).abs().mean() / b.abs().mean()).item()


@pytest.fixture
def counted(monkeypatch):
    """ops.gemm_skinny behind a counting wrapper, ops.gemm_skinny_ok forced on."""
    from mio import ops
    calls = []
    real = ops.gemm_skinny

    def wrapper(*a, **k):
        calls.append(tuple(a[0].shape))
        return real(*a, **k)

    monkeypatch.setattr(ops, "gemm_skinny", wrapper)
    monkeypatch.setattr(ops, "gemm_skinny_ok", lambda M, N, K, activation="none": 1 <= M <= 64)
    return calls


def _paged_setup(cls_name, decode_gemm):
    """The set-up of tests/test_gpu_modules.py test_paged_path_through_module: B 2, q_len 1, d 128, H 4, fp16."""
    from mio.kernels import attention
    torch.manual_seed(2)
    d, H, B, bs, L, nblk = 128, 4, 2, 16, 2, 16
    D = d // H
    dt = torch.float16
    kw = {} if decode_gemm is None else {"decode_gemm": decode_gemm}
    m = getattr(attention, cls_name)(d, H, attention.FlashAttentionConfig(precision="fp16", **kw)).to(DEV, dt).eval()
    kc = torch.randn(nblk, L, bs, H, D, device=DEV, dtype=dt)
    vc = torch.randn(nblk, L, bs, H, D, device=DEV, dtype=dt)
    bt = torch.stack([torch.randperm(nblk)[:6] for _ in range(B)]).to(torch.int32).to(DEV)
    cl = torch.tensor([70, 33], dtype=torch.int32, device=DEV)
    x = torch.randn(B, 1, d, device=DEV, dtype=dt)
    paged = dict(physical_kv_cache_k=kc, physical_kv_cache_v=vc, block_tables=bt, context_lengths=cl, kv_cache_block_size=bs,
                 max_seq_len=96, layer_idx=1)
    return m, x, paged, (d, H, D, B, bs)


@pytest.mark.parametrize("cls_name", ["FlashSelfAttention", "FlashAttentionLayer"])
def test_paged_attention_modules(cls_name, counted):
    m, x, paged, (d, H, D, B, bs) = _paged_setup(cls_name, True)
    y = m(x, **paged)
    assert counted == [(B, 1, d), (B, 1, d)]  # the q (slice of the qkv) projection and o_proj: K and V come from the cache
    sd = {k_: v_.cpu().double() for k_, v_ in m.state_dict().items()}
    wq, bq = (sd["qkv_proj.weight"][:d], sd["qkv_proj.bias"][:d]) if cls_name == "FlashSelfAttention" else \
        (sd["q_proj.weight"], sd["q_proj.bias"])
    q = F.linear(x.cpu().double(), wq, bq).view(B, 1, H, D).permute(0, 2, 1, 3)
    ctx = oracle.paged_attention_forward(q, paged["physical_kv_cache_k"].cpu(), paged["physical_kv_cache_v"].cpu(),
                                         paged["block_tables"].cpu(), paged["context_lengths"].cpu(), bs, 1)
    ref = F.linear(ctx.permute(0, 2, 1, 3).reshape(B, 1, d), sd["o_proj.weight"], sd["o_proj.bias"])
    assert _rel(y, ref) < 5e-3
    # a dense call of the same module never takes the kernel: the option covers the paged branch only
    del counted[:]
    m(torch.randn(B, 40, d, device=DEV, dtype=torch.float16))
    assert counted == []


@pytest.mark.parametrize("cls_name", ["FlashSelfAttention", "FlashAttentionLayer"])
def test_paged_attention_modules_flag_off(cls_name, counted):
    """decode_gemm=False and a config built without the field: no call reaches ops.gemm_skinny, equal bytes."""
    m0, x, paged, _ = _paged_setup(cls_name, None)
    m1, x1, paged1, _ = _paged_setup(cls_name, False)
    y0, y1 = m0(x, **paged), m1(x1, **paged1)
    assert counted == []
    assert torch.equal(y0.view(torch.int16), y1.view(torch.int16))


def _mlp(act, decode_gemm):
    from mio.kernels.mlp import FusedMLPConfig, FusedTransformerMLP
    from mio.synthetic import FusedRMSNorm
    torch.manual_seed(3)
    kw = {} if decode_gemm is None else {"decode_gemm": decode_gemm}
    m = FusedTransformerMLP(128, 512, act, FusedMLPConfig(precision="fp16", **kw)).to(DEV, torch.float16).eval()
    norm = FusedRMSNorm(128, eps=1e-6).to(DEV, torch.float16)
    with torch.no_grad():
        norm.weight.copy_(1 + 0.1 * torch.randn(128))
    x = torch.randn(4, 1, 128, device=DEV, dtype=torch.float16)
    return m, norm, x


@pytest.mark.parametrize("act", ["gelu", "swiglu"])
def test_fused_mlp(act, counted):
    """B 4, S 1, d 128, I 512 with a residual and a pre_norm RMSNorm against fp64 (the norm's 16-bit output as the kernels see it
    is part of the chain judged: the tolerance is the one of test_mlp_converter_module_on_gpu)."""
    m, norm, x = _mlp(act, True)
    y = m(x, x, norm)
    assert counted == [(4, 1, 128), (4, 1, 512)]  # fc1 (activation, gate), fc2 (residual)
    sd = {k: v.cpu() for k, v in m.state_dict().items()}
    xn = F.rms_norm(x.cpu().double(), (128,), norm.weight.cpu().double(), 1e-6)
    ref = oracle.fused_mlp(xn, sd["mlp.fc1.weight"], sd["mlp.fc1.bias"], sd["mlp.fc2.weight"], sd["mlp.fc2.bias"], act,
                           sd.get("mlp.fc1_gate.weight"), sd.get("mlp.fc1_gate.bias")).double() + x.cpu().double()
    assert _rel(y, ref) < 3e-3


@pytest.mark.parametrize("act", ["gelu", "swiglu"])
def test_fused_mlp_flag_off(act, counted):
    m0, norm0, x0 = _mlp(act, None)
    m1, norm1, x1 = _mlp(act, False)
    y0, y1 = m0(x0, x0, norm0), m1(x1, x1, norm1)
    assert counted == []
    assert torch.equal(y0.view(torch.int16), y1.view(torch.int16))

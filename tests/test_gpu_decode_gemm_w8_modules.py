"""The modules' decode_gemm_fp8 option, on the set-ups of tests/test_gpu_decode_gemm_modules.py: with it set, the paged branch of
FlashSelfAttention / FlashAttentionLayer and the plain-tensor path of FusedMLP run their linear layers on ops.gemm_skinny_w8
(counted through a wrapper; ops.gemm_skinny_w8_ok is patched to say yes at these tiny shapes, so the kernel is the one under
test) with weights quantised once per parameter version, and match the fp64 chain evaluated on the DEQUANTISED weights
w8.double() * scale at that file's tolerances -- the quantisation error is the format's, not what is judged here; after an in-place
update of a weight the next call runs on re-quantised bytes and scales; with the field off or absent no call reaches the new ops
and the output bytes are those of a module built without it."""
import pytest
import torch
import torch.nn.functional as F

import oracle

pytestmark = pytest.mark.gpu
DEV = "cuda"
_REAL = {}  # ops.quantize_weight_w8 as the package has it, kept by the fixture for the reference's own use


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).abs().mean() / b.abs().mean()).item()


@pytest.fixture
def counted(monkeypatch):
    """ops.gemm_skinny_w8 and ops.quantize_weight_w8 behind counting wrappers, ops.gemm_skinny_w8_ok forced on."""
    from mio import ops
    calls, quantised = [], []
    real, real_q = ops.gemm_skinny_w8, ops.quantize_weight_w8
    _REAL["quantize"] = real_q

    def wrapper(*a, **k):
        calls.append(tuple(a[0].shape))
        return real(*a, **k)

    def wrapper_q(w):
        quantised.append(tuple(w.shape))
        return real_q(w)

    monkeypatch.setattr(ops, "gemm_skinny_w8", wrapper)
    monkeypatch.setattr(ops, "quantize_weight_w8", wrapper_q)
    monkeypatch.setattr(ops, "gemm_skinny_w8_ok", lambda M, N, K, activation="none": 1 <= M <= 64)
    return calls, quantised


@pytest.fixture
def counted_off(monkeypatch):
    """The advice forced on and both new ops replaced by failures: with the field off nobody may ask, quantise or launch."""
    from mio import ops
    calls = []
    monkeypatch.setattr(ops, "gemm_skinny_w8", lambda *a, **k: calls.append("gemm") or pytest.fail("ops.gemm_skinny_w8 called"))
    monkeypatch.setattr(ops, "quantize_weight_w8", lambda *a, **k: calls.append("quant") or pytest.fail("quantised"))
    monkeypatch.setattr(ops, "gemm_skinny_w8_ok", lambda *a, **k: calls.append("asked") or True)
    return calls


def _deq(w):
    """The weight as the kernel reads it, in fp64: w8 * scale of ops.quantize_weight_w8 (rows are quantised independently)."""
    q, s = _REAL["quantize"](w.detach().to(DEV))
    return (q.float().double() * s.double()[:, None]).cpu()


def _paged_setup(cls_name, fp8):
    """The set-up of tests/test_gpu_decode_gemm_modules.py: B 2, q_len 1, d 128, H 4, fp16."""
    from mio.kernels import attention
    torch.manual_seed(2)
    d, H, B, bs, L, nblk = 128, 4, 2, 16, 2, 16
    D = d // H
    dt = torch.float16
    kw = {} if fp8 is None else {"decode_gemm_fp8": fp8}
    m = getattr(attention, cls_name)(d, H, attention.FlashAttentionConfig(precision="fp16", **kw)).to(DEV, dt).eval()
    kc = torch.randn(nblk, L, bs, H, D, device=DEV, dtype=dt)
    vc = torch.randn(nblk, L, bs, H, D, device=DEV, dtype=dt)
    bt = torch.stack([torch.randperm(nblk)[:6] for _ in range(B)]).to(torch.int32).to(DEV)
    cl = torch.tensor([70, 33], dtype=torch.int32, device=DEV)
    x = torch.randn(B, 1, d, device=DEV, dtype=dt)
    paged = dict(physical_kv_cache_k=kc, physical_kv_cache_v=vc, block_tables=bt, context_lengths=cl, kv_cache_block_size=bs,
                 max_seq_len=96, layer_idx=1)
    return m, x, paged, (d, H, D, B, bs)


def _paged_ref(m, cls_name, x, paged, dims):
    d, H, D, B, bs = dims
    sd = {k_: v_.detach() for k_, v_ in m.state_dict().items()}
    wq, bq = (sd["qkv_proj.weight"][:d], sd["qkv_proj.bias"][:d]) if cls_name == "FlashSelfAttention" else \
        (sd["q_proj.weight"], sd["q_proj.bias"])
    q = F.linear(x.cpu().double(), _deq(wq), bq.cpu().double()).view(B, 1, H, D).permute(0, 2, 1, 3)
    ctx = oracle.paged_attention_forward(q, paged["physical_kv_cache_k"].cpu(), paged["physical_kv_cache_v"].cpu(),
                                         paged["block_tables"].cpu(), paged["context_lengths"].cpu(), bs, 1)
    return F.linear(ctx.permute(0, 2, 1, 3).reshape(B, 1, d), _deq(sd["o_proj.weight"]), sd["o_proj.bias"].cpu().double())


@pytest.mark.parametrize("cls_name", ["FlashSelfAttention", "FlashAttentionLayer"])
def test_paged_attention_modules(cls_name, counted):
    calls, quantised = counted
    m, x, paged, dims = _paged_setup(cls_name, True)
    d, B = dims[0], dims[3]
    y = m(x, **paged)
    assert calls == [(B, 1, d), (B, 1, d)]  # the q (slice of the qkv) projection and o_proj: K and V come from the cache
    assert len(quantised) == 2
    ref = _paged_ref(m, cls_name, x, paged, dims)
    assert _rel(y, ref) < 5e-3
    y_again = m(x, **paged)
    assert len(quantised) == 2 and torch.equal(y_again.view(torch.int16), y.view(torch.int16))  # the prepared copies are kept
    # an in-place update of a parameter: the next call runs on re-quantised weights
    del calls[:], quantised[:]
    with torch.no_grad():
        m.o_proj.weight.mul_(2)
    y2 = m(x, **paged)
    assert calls == [(B, 1, d), (B, 1, d)] and quantised == [tuple(m.o_proj.weight.shape)]
    ref2 = _paged_ref(m, cls_name, x, paged, dims)
    assert _rel(y2, ref2) < 5e-3 and _rel(y2, ref) > 0.1
    # a dense call of the same module never takes the kernel: the option covers the paged branch only
    del calls[:]
    m(torch.randn(B, 40, d, device=DEV, dtype=torch.float16))
    assert calls == []


@pytest.mark.parametrize("cls_name", ["FlashSelfAttention", "FlashAttentionLayer"])
def test_paged_attention_modules_flag_off(cls_name, counted_off):
    """decode_gemm_fp8=False and a config built without the field: no call reaches the new ops, equal bytes."""
    m0, x, paged, _ = _paged_setup(cls_name, None)
    m1, x1, paged1, _ = _paged_setup(cls_name, False)
    y0, y1 = m0(x, **paged), m1(x1, **paged1)
    assert counted_off == []
    assert torch.equal(y0.view(torch.int16), y1.view(torch.int16))


def _mlp(act, fp8):
    from mio.kernels.mlp import FusedMLPConfig, FusedTransformerMLP
    from mio.synthetic import FusedRMSNorm
    torch.manual_seed(3)
    kw = {} if fp8 is None else {"decode_gemm_fp8": fp8}
    m = FusedTransformerMLP(128, 512, act, FusedMLPConfig(precision="fp16", **kw)).to(DEV, torch.float16).eval()
    norm = FusedRMSNorm(128, eps=1e-6).to(DEV, torch.float16)
    with torch.no_grad():
        norm.weight.copy_(1 + 0.1 * torch.randn(128))
    x = torch.randn(4, 1, 128, device=DEV, dtype=torch.float16)
    return m, norm, x


def _mlp_ref(m, norm, x, act):
    sd = {k: v.detach() for k, v in m.state_dict().items()}
    xn = F.rms_norm(x.cpu().double(), (128,), norm.weight.cpu().double(), 1e-6)
    gate = sd.get("mlp.fc1_gate.weight")
    ref = oracle.fused_mlp(xn, _deq(sd["mlp.fc1.weight"]), sd["mlp.fc1.bias"].cpu().double(), _deq(sd["mlp.fc2.weight"]),
                           sd["mlp.fc2.bias"].cpu().double(), act, None if gate is None else _deq(gate),
                           None if gate is None else sd["mlp.fc1_gate.bias"].cpu().double())
    return ref.double() + x.cpu().double()


@pytest.mark.parametrize("act", ["gelu", "swiglu"])
def test_fused_mlp(act, counted):
    """B 4, S 1, d 128, I 512 with a residual and a pre_norm RMSNorm against fp64 on the dequantised weights."""
    calls, quantised = counted
    m, norm, x = _mlp(act, True)
    y = m(x, x, norm)
    assert calls == [(4, 1, 128), (4, 1, 512)]  # fc1 (activation, gate), fc2 (residual)
    assert len(quantised) == (3 if act == "swiglu" else 2)
    ref = _mlp_ref(m, norm, x, act)
    assert _rel(y, ref) < 3e-3
    del calls[:], quantised[:]
    with torch.no_grad():
        m.mlp.fc1.weight.mul_(2)
    y2 = m(x, x, norm)
    assert calls == [(4, 1, 128), (4, 1, 512)] and quantised == [tuple(m.mlp.fc1.weight.shape)]
    assert _rel(y2, _mlp_ref(m, norm, x, act)) < 3e-3 and _rel(y2, ref) > 1e-2


@pytest.mark.parametrize("act", ["gelu", "swiglu"])
def test_fused_mlp_flag_off(act, counted_off):
    m0, norm0, x0 = _mlp(act, None)
    m1, norm1, x1 = _mlp(act, False)
    y0, y1 = m0(x0, x0, norm0), m1(x1, x1, norm1)
    assert counted_off == []
    assert torch.equal(y0.view(torch.int16), y1.view(torch.int16))

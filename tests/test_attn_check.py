"""No-GPU self-test of tests/_attn_check.py: its reference agrees with the oracle, an fp64 result rounded to the storage
dtype passes, and the signatures of typical attention-kernel bugs, applied to the oracle's output, are rejected."""
import math

import pytest
import torch

import oracle
import _attn_check as ac
from test_gpu_kernels import _cmp

B, S, H, HKV, D = 1, 300, 4, 2, 64


def _inputs(dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, S, H, D, generator=g).to(dtype)
    k = torch.randn(B, S, HKV, D, generator=g).to(dtype)
    v = torch.randn(B, S, HKV, D, generator=g).to(dtype)
    return q, k, v


def _rejected(o, ref, dtype, lse, ref_lse):
    with pytest.raises(AssertionError):
        ac.check(o, ref, dtype, "fwd5", lse, ref_lse, "perturbed")


def test_reference_matches_oracle():
    q, k, v = _inputs(torch.bfloat16)
    for causal in (False, True):
        o, lse = ac.reference(q, k, v, causal=causal)
        ro, rlse = oracle.attention_with_lse(q, k, v, causal=causal)
        assert torch.allclose(o, ro, rtol=0, atol=1e-12) and torch.allclose(lse, rlse, rtol=0, atol=1e-12)
    # with a user mask: standard_attention's conventions (causal fill -1e9, keep-mask fill -1e9, additive added)
    keep = (torch.rand(B, 1, S, S) > 0.3).to(torch.uint8)
    add = torch.randn(B, 1, S, S, dtype=torch.float64)
    for causal in (False, True):
        o, _ = ac.reference(q, k, v, causal=causal, keep_mask=keep)
        assert torch.allclose(o, oracle.standard_attention(q, k, v, mask=keep, causal=causal), atol=1e-12)
        o, _ = ac.reference(q, k, v, causal=causal, additive_mask=add)
        assert torch.allclose(o, oracle.standard_attention(q, k, v, additive_mask=add, causal=causal), atol=1e-12)
    # head-major layout
    o, lse = ac.reference(*(t.permute(0, 2, 1, 3) for t in (q, k, v)), layout="bhsd", causal=True)
    ro, rlse = oracle.attention_with_lse(q, k, v, causal=True)
    assert torch.allclose(o, ro, atol=1e-12)


def test_reference_additive_floor():
    """-inf / finfo.min additive entries behave like the -1e30 floor: masked keys get weight 0, a fully masked row the
    uniform average of every key (never NaN)."""
    q, k, v = _inputs(torch.float16)
    for fill in (float("-inf"), torch.finfo(torch.float32).min, torch.finfo(torch.bfloat16).min):
        add = torch.zeros(B, 1, S, S)
        add[..., :40] = fill
        add[..., 7, :] = fill  # query 7 sees no key
        o, lse = ac.reference(q, k, v, additive_mask=add)
        assert torch.isfinite(o).all() and torch.isfinite(lse).all()
        ro, _ = oracle.attention_with_lse(q[:, :, :, :], k[:, 40:], v[:, 40:])
        keep_rows = [i for i in range(S) if i != 7]
        assert torch.allclose(o[:, keep_rows], ro[:, keep_rows], atol=1e-12)
        uni = v.double().repeat_interleave(H // HKV, dim=2).mean(dim=1)
        assert torch.allclose(o[:, 7], uni, atol=1e-12)
        assert torch.allclose(lse[:, :, 7], torch.full_like(lse[:, :, 7], -1e30 + math.log(S)), rtol=1e-15)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_rounded_reference_passes(dtype):
    q, k, v = _inputs(dtype)
    for causal in (False, True):
        ref, rlse = ac.reference(q, k, v, causal=causal)
        st = ac.check(ref.to(dtype), ref, dtype, "fwd5", rlse.float(), rlse, "rounded oracle")
        assert st["worst"] <= 0.5 * math.sqrt(2) and st["mean"] < 0.5


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_kernel_bug_signatures_rejected(dtype):
    q, k, v = _inputs(dtype, seed=1)
    ref, rlse = ac.reference(q, k, v, causal=True)
    good = ref.to(dtype)
    lse = rlse.float()

    # 1. one 16-row group scaled by 1 + 2^-6 (bf16) / 1 + 2^-8 (fp16): a mis-applied rescale / lane-to-row mapping
    eps = 2.0 ** -6 if dtype == torch.bfloat16 else 2.0 ** -8
    o = good.clone()
    o[:, 160:176, 1] = (o[:, 160:176, 1].double() * (1 + eps)).to(dtype)
    _rejected(o, ref, dtype, lse, rlse)
    if dtype == torch.bfloat16:  # ... which the mean / max comparator of the older tests accepts
        _cmp(o, ref, dtype, "scaled row group")

    # 2. one 64-key tile missing from one 32-row group
    keep = torch.ones(B, H, S, S, dtype=torch.uint8)
    keep[:, 2, 224:256, 64:128] = 0
    dropped, dlse = ac.reference(q, k, v, causal=True, keep_mask=keep)
    o = good.clone()
    o[:, 224:256, 2] = dropped[:, 224:256, 2].to(dtype)
    l2 = lse.clone()
    l2[:, 2, 224:256] = dlse[:, 2, 224:256].float()
    _rejected(o, ref, dtype, l2, rlse)
    _rejected(o, ref, dtype, None, rlse)

    # 3. two adjacent 8-wide D columns swapped in one row group
    o = good.clone()
    o[:, 32:48, 0, 8:16], o[:, 32:48, 0, 16:24] = good[:, 32:48, 0, 16:24], good[:, 32:48, 0, 8:16]
    _rejected(o, ref, dtype, lse, rlse)

    # 4. one extra key past the causal diagonal
    extra, xlse = ac.reference(q, k, v, causal=True, q_offset=1)
    _rejected(extra.to(dtype), ref, dtype, xlse.float(), rlse)
    _rejected(extra.to(dtype), ref, dtype, None, rlse)

    # 5. the wrong KV head for one GQA group (heads 2, 3 read kv head 0 instead of 1)
    k2, v2 = k.clone(), v.clone()
    k2[:, :, 1], v2[:, :, 1] = k[:, :, 0], v[:, :, 0]
    wrong, wlse = ac.reference(q, k2, v2, causal=True)
    o = good.clone()
    o[:, :, 2:] = wrong[:, :, 2:].to(dtype)
    _rejected(o, ref, dtype, lse, rlse)

    # non-finite values, and empty rows that are not exactly (0, -inf)
    o = good.clone()
    o[0, 5, 1, 3] = float("nan")
    _rejected(o, ref, dtype, lse, rlse)
    fut, flse = ac.reference(q, k, v, causal=True, k_offset=S - 10)  # rows 0 .. 288 see no key
    o = fut.to(dtype)
    o[0, 3, 0, 0] = 2.0 ** -20
    _rejected(o, fut, dtype, flse.float(), flse)
    fl = flse.float()
    fl[0, 0, 3] = -1e30
    _rejected(fut.to(dtype), fut, dtype, fl, flse)
    ac.check(fut.to(dtype), fut, dtype, "fwd5", flse.float(), flse, "future keys")

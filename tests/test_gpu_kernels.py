"""Parity of the HIP kernels (through the C ABI) against the CPU oracle and the golden fixtures.

Tolerances (stated per the north star's "bf16/fp16 tolerance"):
  rel_err = mean|a-b| / mean|b|  (reference ring_attention.py:1027-1029) against the oracle evaluated in
  fp64 on the same bf16/fp16 inputs and rounded to the storage dtype like the kernel output:
      fp16: rel_err < 1e-3, max|d| < 4e-3      bf16: rel_err < 3e-3, max|d| < 2e-2
  (bf16 has 8 significant bits: one ulp of an O(1) output is 7.8e-3 and rounding alone gives rel_err 1.4e-3, so the
  reference's fp32 "max|d| < 1e-3" is not representable in bf16 storage; the fp16 row is the 1e-3 bar.  The bf16 bar
  is what profiles/parity_r02.json shows at the benchmark shapes -- kernel 1.4e-3 .. 2.5e-3 against the unrounded
  fp32 chain, the reference's own bf16 chain 1.4e-3 .. 5.6e-3 on the same inputs -- with margin;
  tests/test_gpu_fullsize.py asserts kernel_err <= 1.25 x reference_bf16_err case by case.)
"""
import os

import numpy as np
import pytest
import torch

import oracle
import _decode_check as dc

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = {torch.float16: (1e-3, 4e-3), torch.bfloat16: (3e-3, 2e-2)}


def _ops():
    from mio import ops
    return ops


def _cmp(got, ref, dtype, what=""):
    ref = ref.to(dtype).float()
    got = got.float().cpu()
    rel = ((got - ref).abs().mean() / ref.abs().mean().clamp_min(1e-12)).item()
    mx = (got - ref).abs().max().item()
    rtol, atol = TOL[dtype]
    assert rel < rtol and mx < atol * max(1.0, ref.abs().max().item()), f"{what}: rel_err={rel:.3e} max={mx:.3e}"
    return rel, mx


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("B,Sq,Sk,H,Hkv,D,causal", [
    (2, 300, 300, 4, 4, 64, False),
    (2, 300, 300, 4, 4, 64, True),
    (1, 128, 128, 2, 2, 64, True),
    (1, 1, 77, 2, 2, 64, False),       # single query row
    (1, 130, 333, 2, 2, 80, False),    # C5-style cross attention, Dh = 80 (padded to 96)
    (1, 257, 257, 2, 1, 128, True),    # GQA, Dh = 128
    (1, 192, 192, 3, 3, 32, True),     # small head dim (padded to 64)
    (1, 1024, 1024, 8, 8, 64, True),   # several KV tiles + XCD remap (B*H % 8 == 0)
])
def test_fa3_fwd_vs_oracle(dtype, B, Sq, Sk, H, Hkv, D, causal):
    ops = _ops()
    torch.manual_seed(B * 1000 + Sq + D)
    q = torch.randn(B, Sq, H, D, dtype=dtype)
    k = torch.randn(B, Sk, Hkv, D, dtype=dtype)
    v = torch.randn(B, Sk, Hkv, D, dtype=dtype)
    o, lse = ops.fa3_fwd(q.to(DEV), k.to(DEV), v.to(DEV), causal=causal, return_lse=True)
    ref, rlse = oracle.attention_with_lse(q, k, v, causal=causal)
    _cmp(o, ref, dtype, "o")
    assert (lse.cpu().double() - rlse).abs().max() < 2e-3
    # public drop-in signature
    o2 = ops.flash_attention(q.to(DEV), k.to(DEV), v.to(DEV), None, causal)
    assert torch.equal(o2, o)


@pytest.mark.parametrize("Sq,Sk,causal,q_off,k_off", [
    (129, 1, False, 0, 0), (129, 63, False, 0, 0), (200, 64, False, 0, 0), (256, 65, False, 0, 0),
    (257, 130, False, 0, 0), (511, 257, False, 0, 0), (300, 700, False, 0, 0),
    (129, 129, True, 0, 0), (256, 256, True, 0, 0), (257, 257, True, 0, 0), (511, 511, True, 0, 0),
    (200, 200, True, 200, 0),    # ring step: keys entirely in the past (nothing masked)
    (200, 200, True, 0, 200),    # keys entirely in the future: every row empty (o = 0, lse = -inf)
    (256, 192, True, 64, 128),   # partial overlap, unaligned offsets
    (130, 300, True, 170, 0),    # queries are the tail of a longer sequence
])
def test_fa3_pipelined_kernel_shapes(Sq, Sk, causal, q_off, k_off):
    """Edge shapes of the software-pipelined kernel (head dim 64, Sq > 128): one-tile and ragged KV, ragged query
    blocks, waves with no visible key, causal diagonals at arbitrary offsets, grouped KV heads, B*H not a multiple
    of 8 (no XCD remap)."""
    ops = _ops()
    torch.manual_seed(Sq * 7 + Sk)
    dtype, B, H, Hkv, D = torch.float16, 1, 6, 2, 64
    q = torch.randn(B, Sq, H, D, dtype=dtype)
    k = torch.randn(B, Sk, Hkv, D, dtype=dtype)
    v = torch.randn(B, Sk, Hkv, D, dtype=dtype)
    o, lse = ops.fa3_fwd(q.to(DEV), k.to(DEV), v.to(DEV), causal=causal, q_offset=q_off, k_offset=k_off, return_lse=True)
    ref, rlse = oracle.attention_with_lse(q, k, v, causal=causal, q_offset=q_off, k_offset=k_off)
    empty = torch.isinf(rlse)                       # rows without a visible key
    assert torch.equal(torch.isinf(lse.cpu()), empty)
    assert (lse.cpu().double() - rlse)[~empty].abs().max() < 2e-3 if (~empty).any() else True
    keep = (~empty).permute(0, 2, 1)[..., None].expand_as(ref)   # [B,H,Sq] -> [B,Sq,H,D]
    if keep.any():
        _cmp(o.cpu()[keep], ref[keep], dtype, "o")
    assert (o.cpu()[~keep] == 0).all()


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D,S,H", [(64, 4096, 8), (128, 2048, 4), (80, 1536, 4)])
def test_fa3_benchmark_length(dtype, causal, D, S, H):
    """Sequence length of the benchmark (4096 = 64 KV tiles per query block: many reference moves, the 4-stage DMA
    ring wraps 16 times, heavy + light causal passes) with head dim 64 -> the software-pipelined kernel.  The CPU oracle
    cannot finish this size in seconds, so the checker is plain fp32 torch on the GPU (softmax(q k^T / sqrt(D)) v) on
    the same 16-bit inputs; lse against logsumexp.  Scores are scaled up (q * 3) so that rows really outgrow their
    running reference by more than the rescale threshold several times (the rare path that rescales the asm-owned
    accumulators).  Head dims 128 and 80 take the one-wave-per-SIMD pipelined kernel (fa3_fwd3), head dim 64 fa3_fwd5."""
    ops = _ops()
    torch.manual_seed(17)
    B = 1
    q = (torch.randn(B, S, H, D, device=DEV) * 3).to(dtype)
    k = torch.randn(B, S, H, D, device=DEV).to(dtype)
    v = torch.randn(B, S, H, D, device=DEV).to(dtype)
    o, lse = ops.fa3_fwd(q, k, v, causal=causal, return_lse=True)
    qf, kf, vf = (t.float().permute(0, 2, 1, 3) for t in (q, k, v))
    s = (qf @ kf.transpose(-1, -2)) / D ** 0.5
    if causal:
        s = s.masked_fill(torch.triu(torch.ones(S, S, device=DEV, dtype=torch.bool), 1), float("-inf"))
    ref = (torch.softmax(s, -1) @ vf).permute(0, 2, 1, 3)
    rel = ((o.float() - ref).abs().mean() / ref.abs().mean()).item()
    assert rel < TOL[dtype][0], f"rel_err={rel:.3e}"
    # the row sum is accumulated by the matrix core from the 16-bit P that also feeds P.V (numerator and denominator
    # see the same rounding): with peaked rows (few dominant keys) lse carries P's relative precision, 2^-11 / 2^-9
    assert (lse - torch.logsumexp(s, -1)).abs().max().item() < (2e-3 if dtype == torch.float16 else 6e-3)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("B,Sq,Sk,H,Hkv,D,causal,q_off,k_off", [
    (2, 300, 300, 4, 4, 64, True, 0, 0), (1, 257, 130, 6, 2, 64, False, 0, 0), (1, 511, 511, 6, 2, 64, True, 0, 0),
    (1, 256, 192, 6, 2, 64, True, 64, 128),   # partial overlap: rows that see no key stay "fresh" for the whole pass
    (1, 130, 300, 6, 2, 64, True, 170, 0), (1, 192, 192, 3, 3, 32, True, 0, 0), (1, 2048, 2048, 8, 8, 64, True, 0, 0),
    (1, 2048, 2048, 4, 4, 64, False, 0, 0),
    (1, 832, 832, 4, 4, 64, True, 0, 0),     # 13 KV tiles in the heavy pass (odd), 4 in the light one: the DMA stream crosses
    (1, 576, 576, 4, 2, 64, True, 0, 0),     # three 256-row blocks: one causal pair + the single-pass middle block
    (1, 700, 1100, 4, 4, 64, True, 400, 0),  # Sk > Sq behind an offset: every row sees > 400 keys, ragged last tile
    (1, 600, 1000, 4, 4, 48, False, 0, 0),
])
def test_fa3_k_prescaled(dtype, B, Sq, Sk, H, Hkv, D, causal, q_off, k_off):
    """k_prescaled launches (fa3_fwd5_kernel at D <= 64, fa3_fwd3_kernel KPRE above: reference through the MFMA's C
    operand, post-exp rescale test on bit 14 of the packed P words): K~ = round16(K * softmax_scale * log2 e) computed in fp32 -- what the projection's
    col_scale epilogue hands over -- against the oracle evaluated on (q, K~, v) with scores q . K~ * ln 2.  q is scaled
    up at the long sequence so that rows outgrow their reference by more than 2^(margin + 1) several times (the rare
    branch that recomputes a tile's P)."""
    import math
    ops = _ops()
    torch.manual_seed(Sq + 3 * Sk + D)
    q = (torch.randn(B, Sq, H, D) * (3 if Sq >= 2048 else 1)).to(dtype)
    kt = (torch.randn(B, Sk, Hkv, D) * (math.log2(math.e) / math.sqrt(D))).to(dtype)
    v = torch.randn(B, Sk, Hkv, D).to(dtype)
    o, lse = ops.fa3_fwd(q.to(DEV), kt.to(DEV), v.to(DEV), causal=causal, q_offset=q_off, k_offset=k_off, return_lse=True,
                         k_prescaled=True)
    ref, rlse = oracle.attention_with_lse(q, kt, v, causal=causal, q_offset=q_off, k_offset=k_off,
                                          softmax_scale=math.log(2.0))
    empty = torch.isinf(rlse)
    assert torch.equal(torch.isinf(lse.cpu()), empty)
    if (~empty).any():
        assert (lse.cpu().double() - rlse)[~empty].abs().max() < (6e-3 if dtype == torch.bfloat16 else 2e-3)
    keep = (~empty).permute(0, 2, 1)[..., None].expand_as(ref)
    if keep.any():
        _cmp(o.cpu()[keep], ref[keep], dtype, "o")
    assert (o.cpu()[~keep] == 0).all()
    with pytest.raises(ValueError):  # outside the kernel that supports it: refused, not silently ignored
        ops.fa3_fwd(q[:, :64].to(DEV), kt.to(DEV), v.to(DEV), k_prescaled=True)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_gemm_col_scale(dtype):
    """Column-scale epilogue of the persistent GEMM: columns [lo, hi) = round16(value * (x w^T + b)) -- scaled in fp32
    before the one rounding -- and every other column bit-identical to the plain launch."""
    ops = _ops()
    torch.manual_seed(13)
    M, N, K = 8192 + 40, 3072, 512
    x = torch.randn(M, K).to(dtype)
    w = (torch.randn(N, K) * 0.05).to(dtype)
    b = torch.randn(N).to(dtype)
    wb = ops.block_weight(w.to(DEV))
    assert ops.col_scale_ok(M, N, K)
    val, lo, hi = 0.18033688, 1024, 2048
    y0 = ops.gemm_bias_act(x.to(DEV), w.to(DEV), b.to(DEV), w_blocked=wb)
    y1 = ops.gemm_bias_act(x.to(DEV), w.to(DEV), b.to(DEV), w_blocked=wb, col_scale=(lo, hi, val))
    assert torch.equal(y1[:, :lo], y0[:, :lo]) and torch.equal(y1[:, hi:], y0[:, hi:])
    want = ((x.float() @ w.float().T).double() + b.double())[:, lo:hi] * val
    _cmp(y1[:, lo:hi], want, dtype, "scaled columns")
    # a single rounding: tighter than scaling the already rounded plain result
    once = (y1[:, lo:hi].float().cpu().double() - want).abs().mean()
    twice = ((y0[:, lo:hi].float() * val).to(dtype).float().cpu().double() - want).abs().mean()
    assert once < twice
    with pytest.raises(ValueError):
        ops.gemm_bias_act(x.to(DEV), w.to(DEV), b.to(DEV), w_blocked=wb, col_scale=(100, 2048, val))
    with pytest.raises(ValueError):
        ops.gemm_bias_act(x[:64].to(DEV), w.to(DEV), b.to(DEV), w_blocked=wb, col_scale=(lo, hi, val))


@pytest.mark.parametrize("case", ["d64_nomask", "d64_additive", "d64_causal", "d80_cross", "d128_causal", "d64_padding"])
def test_ring_forward_vs_golden(golden_dir, case):
    """HIP kernel vs the outputs of the reference's own ring fallback (tests/golden)."""
    ops = _ops()
    g = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(golden_dir, "ring_attention_fallback.npz")).items()}
    dtype = torch.float16
    q, k, v, o = (g[f"{case}_{n}"] for n in "qkvo")
    B, H, Sq, D = q.shape
    Sk = k.shape[2]
    mask = None
    if f"{case}_mask" in g:
        mask = g[f"{case}_mask"]
    elif "causal" in case:
        mask = torch.triu(torch.full((Sq, Sk), -1e9), diagonal=1)[None, None].expand(B, 1, Sq, Sk).contiguous()
    elif "padding" in case:
        mask = ((1.0 - g[f"{case}_keep"]) * -1e9)[:, None, None, :]
    qh, kh, vh = (t.to(dtype) for t in (q, k, v))
    out = ops.ring_attention_forward(qh.to(DEV), kh.to(DEV), vh.to(DEV), None if mask is None else mask.to(DEV))
    assert out.shape == (B, Sq, H * D)
    # golden was computed from fp32 inputs; the kernel sees fp16-rounded inputs -> compare to the oracle on the
    # rounded inputs (tight) and to the golden itself (loose, input rounding included)
    ref = oracle.ring_attention_forward(qh.float(), kh.float(), vh.float(), mask)
    _cmp(out, ref, dtype, "vs oracle")
    assert (out.float().cpu() - o).abs().max() < 2e-2
    if "padding" in case:  # the same through the keep-mask path of flash_attention
        o2 = ops.flash_attention(qh.permute(0, 2, 1, 3).to(DEV), kh.permute(0, 2, 1, 3).to(DEV),
                                 vh.permute(0, 2, 1, 3).to(DEV), g[f"{case}_keep"].to(DEV))
        _cmp(o2.reshape(B, Sq, H * D), ref, dtype, "keep-mask")


def test_fa3_masks_and_causal_with_mask():
    ops = _ops()
    torch.manual_seed(3)
    B, S, H, D = 2, 200, 2, 64
    dtype = torch.float16
    q, k, v = (torch.randn(B, S, H, D, dtype=dtype) for _ in range(3))
    keep3 = (torch.rand(B, S, S) > 0.3)
    keep3[:, :, 0] = True
    o = ops.flash_attention(q.to(DEV), k.to(DEV), v.to(DEV), keep3.to(DEV), True)
    ref = oracle.standard_attention(q, k, v, mask=keep3.float(), causal=True)
    _cmp(o, ref, dtype, "causal+mask")
    keep2 = torch.ones(B, S)
    keep2[0, 150:] = 0
    o = ops.flash_attention(q.to(DEV), k.to(DEV), v.to(DEV), keep2.to(DEV))
    _cmp(o, oracle.standard_attention(q, k, v, mask=keep2), dtype, "padding")
    # a fully masked row degenerates to the uniform average, as the -1e9 fill does in the reference
    keep0 = torch.ones(B, S)
    keep0[1, :] = 0
    o = ops.flash_attention(q.to(DEV), k.to(DEV), v.to(DEV), keep0.to(DEV))
    _cmp(o, oracle.standard_attention(q, k, v, mask=keep0), dtype, "all-masked")


def test_fa3_carry_and_merge_roundtrip():
    """Split-KV with (o, lse) carry and with the merge kernel both reproduce whole attention."""
    ops = _ops()
    torch.manual_seed(5)
    B, S, H, D = 1, 384, 4, 64
    dtype = torch.bfloat16
    q, k, v = (torch.randn(B, S, H, D, dtype=dtype, device=DEV) for _ in range(3))
    full, lse_full = ops.fa3_fwd(q, k, v, return_lse=True)
    o_acc = torch.zeros(B, S, H, D, dtype=torch.float32, device=DEV)
    lse = torch.full((B, H, S), float("-inf"), device=DEV)
    cuts = [0, 100, 228, 384]
    for i in range(3):
        ks, vs = k[:, cuts[i]:cuts[i + 1]].contiguous(), v[:, cuts[i]:cuts[i + 1]].contiguous()
        out = ops.fa3_fwd(q, ks, vs, o_acc=o_acc, lse=lse, carry_in=(i > 0), write_out=(i == 2))
    assert (out.float() - full.float()).abs().max() < 2e-2
    assert (lse - lse_full).abs().max() < 1e-3
    ref = oracle.standard_attention(q.cpu(), k.cpu(), v.cpu())
    assert (o_acc.cpu().double() - ref).abs().max() < 5e-3
    # merge kernel
    oa = torch.zeros_like(o_acc); la = torch.empty_like(lse)
    ob = torch.zeros_like(o_acc); lb = torch.empty_like(lse)
    ops.fa3_fwd(q, k[:, :200].contiguous(), v[:, :200].contiguous(), o_acc=oa, lse=la, write_out=False)
    ops.fa3_fwd(q, k[:, 200:].contiguous(), v[:, 200:].contiguous(), o_acc=ob, lse=lb, write_out=False)
    out2 = torch.empty_like(q)
    ops.attn_merge(oa, la, ob, lb, out2)
    assert (oa.cpu().double() - ref).abs().max() < 5e-3
    assert (la - lse_full).abs().max() < 1e-3
    assert (out2.float() - full.float()).abs().max() < 2e-2
    # causal with offsets: a future shard leaves the state untouched; a past shard is unmasked
    o3 = torch.zeros_like(o_acc); l3 = torch.full_like(lse, float("-inf"))
    ops.fa3_fwd(q, k, v, causal=True, q_offset=0, k_offset=4096, o_acc=o3, lse=l3, write_out=False)
    assert torch.isinf(l3).all() and o3.abs().max() == 0
    o4, l4 = ops.fa3_fwd(q, k, v, causal=True, q_offset=4096, k_offset=0, return_lse=True)
    assert (o4.float() - full.float()).abs().max() < 2e-2


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("B,S,H,Hkv,D,causal", [(2, 600, 4, 4, 64, True), (1, 1000, 6, 2, 32, False), (3, 300, 2, 2, 48, True)])
def test_fa3_blocked_output(dtype, B, S, H, Hkv, D, causal):
    """o_blocked: the same launch writes its [B*S, H*D] output in the GEMMs' blocked activation layout -- bit for bit the
    row-major result after un-blocking, and the output projection fed with it equals the one fed with the row-major tensor."""
    import math
    ops = _ops()
    torch.manual_seed(S + D)
    q = torch.randn(B, S, H, D).to(dtype).to(DEV)
    kt = (torch.randn(B, S, Hkv, D) * (math.log2(math.e) / math.sqrt(D))).to(dtype).to(DEV)
    v = torch.randn(B, S, Hkv, D).to(dtype).to(DEV)
    assert ops.fa3_o_blocked_ok(B, S, S, H, D, Hkv * D, Hkv * D)
    o = ops.fa3_fwd(q, kt, v, causal=causal, k_prescaled=True)
    ob = ops.fa3_fwd(q, kt, v, causal=causal, k_prescaled=True, out_blocked=True)
    M, N = B * S, H * D
    Mp = (M + 255) // 256 * 256
    assert tuple(ob.shape) == (Mp, N)
    un = ob.view(Mp // 256, N // 32, 256, 32).permute(0, 2, 1, 3).reshape(Mp, N)[:M]
    assert torch.equal(un, o.view(M, N))
    with pytest.raises(ValueError):  # needs a k_prescaled launch
        ops.fa3_fwd(q, kt, v, causal=causal, out_blocked=True)
    if N % 128 == 0 and ops.blocked_weight_ok(M, 256, N):
        w = (torch.randn(256, N) * 0.05).to(dtype).to(DEV)
        bias = torch.randn(256).to(dtype).to(DEV)
        res = torch.randn(B, S, 256).to(dtype).to(DEV)
        wb = ops.block_weight(w)
        y0 = ops.gemm_bias_act(o.view(B, S, N), w, bias, residual=res, w_blocked=wb)
        y1 = ops.gemm_bias_act(ob, w, bias, residual=res, w_blocked=wb, x_blocked_shape=(B, S, N))
        assert torch.equal(y0, y1)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("B,S,H,Hkv,D,causal", [(1, 640, 4, 4, 64, False), (2, 450, 4, 2, 64, True), (1, 832, 3, 3, 48, True)])
def test_fa3_k_prescaled_carry(dtype, B, S, H, Hkv, D, causal):
    """The ring form of the k_prescaled launch (fa3_fwd5_kernel CARRY): K~ / V shards visited in ring order -- the local
    (diagonal) shard first, then the past ones -- with the (o_acc fp32, lse) state carried from launch to launch, a shard in
    the future of every query dropped by the kernel (state untouched), the last launch writing the 16-bit output.  Against
    the oracle's whole attention on (q, K~, v) in base 2."""
    import math
    ops = _ops()
    torch.manual_seed(S + D + int(causal))
    q = (torch.randn(B, S, H, D) * 2).to(dtype)
    kt = (torch.randn(B, S, Hkv, D) * (math.log2(math.e) / math.sqrt(D))).to(dtype)
    v = torch.randn(B, S, Hkv, D).to(dtype)
    ref, rlse = oracle.attention_with_lse(q, kt, v, causal=causal, softmax_scale=math.log(2.0))
    qd, kd, vd = q.to(DEV), kt.to(DEV), v.to(DEV)
    assert ops.fa3_k_prescaled_ok(B, S - 2 * (S // 3), S // 3, H, D, Hkv * D, Hkv * D, carry=True)
    # queries = the LAST third of the sequence (a rank's shard), keys in three shards: own, then the two before it
    n = S // 3
    qs = qd[:, 2 * n:].contiguous()
    Sq = qs.shape[1]
    o_acc = torch.zeros(B, Sq, H, D, dtype=torch.float32, device=DEV)
    lse = torch.full((B, H, Sq), float("-inf"), device=DEV)
    out = torch.empty_like(qs)
    order = [(2 * n, S), (n, 2 * n), (0, n)]
    for i, (a, b) in enumerate(order):
        ops.fa3_fwd(qs, kd[:, a:b].contiguous(), vd[:, a:b].contiguous(), causal=causal, q_offset=2 * n if causal else 0,
                    k_offset=a if causal else 0, o_acc=o_acc, lse=lse, carry_in=(i > 0), write_out=(i == 2), out=out,
                    k_prescaled=True)
    _cmp(out.cpu(), ref[:, 2 * n:], dtype, "o")
    assert (o_acc.cpu().double() - ref[:, 2 * n:]).abs().max() < (1.5e-2 if dtype == torch.bfloat16 else 3e-3)
    assert (lse.cpu().double() - rlse[:, :, 2 * n:]).abs().max() < (6e-3 if dtype == torch.bfloat16 else 2e-3)
    if causal:  # the FIRST third as queries against the last shard: every key lies in the future, the state must not move
        q1 = qd[:, :n + 40].contiguous()
        o1 = torch.full((B, n + 40, H, D), 3.0, dtype=torch.float32, device=DEV)
        l1 = torch.full((B, H, n + 40), 0.25, device=DEV)
        ops.fa3_fwd(q1, kd[:, 2 * n:].contiguous(), vd[:, 2 * n:].contiguous(), causal=True, q_offset=0, k_offset=2 * n,
                    o_acc=o1, lse=l1, carry_in=True, write_out=False, k_prescaled=True)
        assert (o1 - 3.0).abs().max() < 1e-5 and (l1 - 0.25).abs().max() < 1e-5


ACTS = ["gelu", "gelu_erf", "relu", "silu", "swiglu"]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("B,S,d,I", [(2, 75, 64, 256), (1, 130, 96, 160), (3, 333, 256, 1024)])
def test_fused_mlp_vs_oracle(dtype, act, B, S, d, I):
    ops = _ops()
    torch.manual_seed(S + I)
    x = torch.randn(B, S, d).to(dtype)
    w1, b1 = (torch.randn(I, d) * 0.1).to(dtype), (torch.randn(I) * 0.1).to(dtype)
    w2, b2 = (torch.randn(d, I) * 0.1).to(dtype), (torch.randn(d) * 0.1).to(dtype)
    wg, bg = (torch.randn(I, d) * 0.1).to(dtype), (torch.randn(I) * 0.1).to(dtype)
    gate = (wg.to(DEV), bg.to(DEV)) if act == "swiglu" else (None, None)
    y = ops.fused_mlp(x.to(DEV), w1.to(DEV), b1.to(DEV), w2.to(DEV), b2.to(DEV), act, *gate)
    ref = oracle.fused_mlp(x, w1, b1, w2, b2, act, wg, bg)
    # the [M,I] activation is stored once in the storage dtype between the two GEMM stages (like the
    # reference's F.linear chain in bf16/fp16); allow its rounding on top of the output rounding
    ref_q = oracle.fused_mlp(x, w1, b1, w2, b2, act, wg, bg)
    rel, mx = _cmp(y, ref_q, dtype, f"mlp {act}") if False else (None, None)
    got = y.float().cpu()
    refd = ref.to(dtype).float()
    rel = ((got - refd).abs().mean() / refd.abs().mean()).item()
    assert rel < (2e-3 if dtype == torch.float16 else 5e-3), f"rel_err={rel:.3e}"


@pytest.mark.parametrize("name,act", [("gelu", "gelu"), ("swiglu", "swiglu"), ("relu", "relu"), ("silu", "silu"),
                                      ("gelu_erf", "gelu_erf")])
def test_fused_mlp_vs_golden(golden_dir, name, act):
    """HIP FusedMLP vs the outputs of the reference's FusedTransformerMLP / FusedMLP modules."""
    ops = _ops()
    g = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(golden_dir, "fused_mlp_modules.npz")).items()}
    pre = f"{name}_mlp_" if f"{name}_mlp_fc1_weight" in g else f"{name}_"
    h = lambda t: None if t is None else t.to(torch.float16).to(DEV)
    y = ops.fused_mlp(h(g[f"{name}_x"]), h(g[pre + "fc1_weight"]), h(g[pre + "fc1_bias"]), h(g[pre + "fc2_weight"]),
                      h(g[pre + "fc2_bias"]), act, h(g.get(pre + "fc1_gate_weight")), h(g.get(pre + "fc1_gate_bias")))
    ref = g[f"{name}_y"]
    rel = ((y.float().cpu() - ref).abs().mean() / ref.abs().mean()).item()
    assert rel < 3e-3, f"rel_err={rel:.3e}"  # fp16 rounding of inputs/weights/intermediate vs the fp32 module


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_gemm_edges_and_residual(dtype):
    ops = _ops()
    torch.manual_seed(11)
    for M, N, K in [(1, 8, 8), (37, 72, 40), (300, 520, 136), (513, 264, 1024), (4096, 1024, 512)]:
        x = torch.randn(M, K).to(dtype)
        w = (torch.randn(N, K) * 0.1).to(dtype)
        b = torch.randn(N).to(dtype)
        r = torch.randn(M, N).to(dtype)
        y = ops.gemm_bias_act(x.to(DEV), w.to(DEV), b.to(DEV), residual=r.to(DEV))
        ref = (x.double() @ w.double().T + b.double() + r.double())
        _cmp(y, ref, dtype, f"gemm {M}x{N}x{K}")
    # linearity (size independent property): f(x1 + x2) == f(x1) + f(x2) for the bias-free GEMM, exactly
    # representable inputs
    # (K = 64, |x| <= 2, |w| <= 1 keeps every result an integer <= 256: exact in bf16 and fp16)
    x1 = torch.randint(-2, 3, (256, 64)).to(dtype).to(DEV)
    x2 = torch.randint(-2, 3, (256, 64)).to(dtype).to(DEV)
    w = torch.randint(-1, 2, (256, 64)).to(dtype).to(DEV)
    a = ops.gemm_bias_act(x1 + x2, w).float()
    bsum = ops.gemm_bias_act(x1, w).float() + ops.gemm_bias_act(x2, w).float()
    assert torch.equal(a, bsum)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("act,res,M", [("gelu", True, 16384 + 100), ("relu", False, 16384), ("silu", True, 20000)])
def test_fused_mlp_blocked_intermediate(dtype, act, res, M):
    """FusedMLP at a size where both GEMMs run the 256x256-tile kernels: the [M, I] intermediate then lives in the
    blocked layout (one contiguous 16 KiB block per 256 rows x 32 columns) between the persistent stage-1 kernel's
    trickled stores and the stage-2 kernel's DMA loads; ragged M exercises the partly filled last row block.
    Checker: fp32 CPU matmuls on the same 16-bit inputs + the oracle's activation (too large for the fp64 oracle)."""
    ops = _ops()
    from oracle.mlp import gelu_tanh
    torch.manual_seed(9)
    d, I = 1024, 1024
    x = torch.randn(1, M, d).to(dtype)
    w1 = (torch.randn(I, d) * 0.03).to(dtype)
    b1 = (torch.randn(I) * 0.1).to(dtype)
    w2 = (torch.randn(d, I) * 0.03).to(dtype)
    b2 = (torch.randn(d) * 0.1).to(dtype)
    r = torch.randn(1, M, d).to(dtype) if res else None
    y = ops.fused_mlp(x.to(DEV), w1.to(DEV), b1.to(DEV), w2.to(DEV), b2.to(DEV), act,
                      residual=None if r is None else r.to(DEV))
    h = x[0].float() @ w1.float().T + b1.float()
    h = {"gelu": gelu_tanh, "relu": torch.relu, "silu": torch.nn.functional.silu}[act](h).to(dtype).float()
    ref = (h @ w2.float().T + b2.float()).double()
    if r is not None:
        ref = ref + r[0].double()
    rel = ((y[0].float().cpu().double() - ref).abs().mean() / ref.abs().mean()).item()
    assert rel < (2e-3 if dtype == torch.float16 else 5e-3), f"rel_err={rel:.3e}"
    assert ops.fused_mlp_blocked_weight_ok(M, d, I, act)
    y2 = ops.fused_mlp(x.to(DEV), w1.to(DEV), b1.to(DEV), w2.to(DEV), b2.to(DEV), act,
                       residual=None if r is None else r.to(DEV),
                       fc1_blocked=ops.block_weight(w1.to(DEV)), fc2_blocked=ops.block_weight(w2.to(DEV)))
    assert torch.equal(y2, y)  # blocked weights: same kernels, same arithmetic


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("M,N,K,act,res", [
    (4096 + 37, 4096 + 8, 1024, "none", False),   # gemm8w_kernel, ragged M and N, 289 tiles (2 per workgroup for some)
    (8192, 2304 + 24, 256, "gelu", False),        # 8 K-tiles, 320 tiles
    (5000, 3584, 544, "silu", False),             # 17 K-tiles (odd: the LDS stage index runs on across tiles)
    (4096 + 5, 4096, 512, "gelu_erf", False),     # erf read-out
    (4352, 4096, 288, "none", True),              # residual read-out, 9 K-tiles
    (8192 + 100, 4096, 128, "none", True),        # the minimum depth: 4 K-tiles, every K-tile is a boundary case
    (8192, 4096 + 72, 160, "gelu", False),        # 5 K-tiles
    (4352 + 3, 4096, 264, "relu", True),          # K % 32 != 0 -> generic 256x256 kernel (32x32x16)
])
def test_gemm_big_tiles(dtype, M, N, K, act, res):
    """The 256x256-tile kernels only run when a launch has >= 256 such tiles (mio gemm_inst.hip launch_act): sizes
    the numpy oracle cannot finish in seconds, so the checker here is a CPU fp32 matmul of the same 16-bit inputs
    + the oracle's activation (oracle/mlp.py), which is the reference's F.linear + activation
    (kernels/mlp/fused_mlp.py:159-176)."""
    ops = _ops()
    torch.manual_seed(5)
    x = torch.randn(M, K).to(dtype)
    w = (torch.randn(N, K) * 0.05).to(dtype)
    b = torch.randn(N).to(dtype)
    r = torch.randn(M, N).to(dtype) if res else None
    y = ops.gemm_bias_act(x.to(DEV), w.to(DEV), b.to(DEV), act, residual=None if r is None else r.to(DEV))
    from oracle.mlp import gelu_tanh
    z = (x.float() @ w.float().T).double() + b.double()
    z = {"none": lambda t: t, "gelu": gelu_tanh, "gelu_erf": torch.nn.functional.gelu, "relu": torch.relu,
         "silu": torch.nn.functional.silu}[act](z)
    if r is not None:
        z = z + r.double()
    _cmp(y, z, dtype, f"gemm {M}x{N}x{K} {act} res={res}")
    if K % 32 == 0:  # the same launch with the weight in the blocked layout: same kernel, same arithmetic -> same bits
        assert ops.blocked_weight_ok(M, N, K, act)
        wb = ops.block_weight(w.to(DEV))
        ref_blk = w.view(-1)  # layout check against the definition: wb[((n/256)*(K/32) + k/32)*256 + n%256][k%32]
        Np = (N + 255) // 256 * 256
        wp = torch.zeros(Np, K, dtype=dtype)
        wp[:N] = w
        want = wp.view(Np // 256, 256, K // 32, 32).permute(0, 2, 1, 3).reshape(Np, K)
        assert torch.equal(wb.cpu(), want)
        y2 = ops.gemm_bias_act(x.to(DEV), w.to(DEV), b.to(DEV), act, residual=None if r is None else r.to(DEV), w_blocked=wb)
        assert torch.equal(y2, y)


def test_gemm_big_tiles_exact():
    """Bit-exact integer case for the persistent kernel: x, w in {-1, 0, 1}, K = 256 keeps every dot product an
    integer of magnitude <= 256 (exact in bf16); every tile of every workgroup must match integer arithmetic, and
    rows / columns past the ragged edge must stay untouched."""
    ops = _ops()
    g = torch.Generator().manual_seed(3)
    M, N, K = 4096 + 250, 4096 + 16, 256
    x = torch.randint(-1, 2, (M, K), generator=g)
    w = torch.randint(-1, 2, (N, K), generator=g)
    out = torch.full((M + 2, N + 8), 7.0, dtype=torch.bfloat16, device=DEV)  # guard rows / columns around the view
    view = out[:M, :N]
    ops.gemm_bias_act(x.to(torch.bfloat16).to(DEV), w.to(torch.bfloat16).to(DEV), None, out=view)
    ref = (x.double() @ w.double().T)
    assert torch.equal(view.double().cpu(), ref)
    assert bool((out[M:, :] == 7).all()) and bool((out[:, N:] == 7).all())


@pytest.mark.parametrize("N,residual", [(1024 + 16, True), (3072, False)])
def test_gemm_exact_k4096(N, residual):
    """The integer case at K = 4096 (the fc2 depth): x, w in {-1, 0, 1}, dot products up to 4096 in magnitude are exact in the
    fp32 accumulators, so the 16-bit result must equal the exactly rounded integer sum (+ integer residual) bit for bit -- on
    the plain operands, with the blocked weight, and with both operands blocked (residual: one-tile kernel, else persistent)."""
    ops = _ops()
    g = torch.Generator().manual_seed(11)
    M, K = 2048 + 250, 4096
    x = torch.randint(-1, 2, (M, K), generator=g).to(torch.bfloat16)
    w = torch.randint(-1, 2, (N, K), generator=g).to(torch.bfloat16)
    r = torch.randint(-8, 9, (M, N), generator=g).to(torch.bfloat16) if residual else None
    ref = x.double() @ w.double().T
    if r is not None:
        ref = ref + r.double()
    want = ref.to(torch.bfloat16)  # round-to-nearest-even of the exact integer
    xd, wd = x.to(DEV), w.to(DEV)
    rd = None if r is None else r.to(DEV)
    y0 = ops.gemm_bias_act(xd, wd, None, residual=rd)
    assert torch.equal(y0.cpu(), want)
    if ops.blocked_weight_ok(M, N, K):
        wb = ops.block_weight(wd)
        y1 = ops.gemm_bias_act(xd, wd, None, residual=rd, w_blocked=wb)
        assert torch.equal(y1.cpu(), want)
        xb = ops.block_weight(xd)  # the blocked activation layout is the weight layout with m in the place of n
        y2 = ops.gemm_bias_act(xb, wd, None, residual=rd, w_blocked=wb, x_blocked_shape=(M, K))
        assert torch.equal(y2.cpu(), want)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_layernorm_blocked_handover(dtype):
    """LayerNorm -> GEMM hand-over in the blocked activation layout: layout exactness of mio_layernorm_fwd_bx against
    the definition, then the blocked-x GEMM and fused MLP against the plain-layout launches of the same kernels (same
    arithmetic -> same bits).  Ragged M exercises the partly filled last 256-row block."""
    ops = _ops()
    torch.manual_seed(21)
    M, d, I = 16384 + 100, 1024, 1024
    x = torch.randn(1, M, d, device=DEV).to(dtype)
    g = (1 + 0.1 * torch.randn(d, device=DEV)).to(dtype)
    be = (0.1 * torch.randn(d, device=DEV)).to(dtype)
    y = ops.layernorm(x, g, be)
    yb = ops.layernorm(x, g, be, out_blocked=True)
    Mp = (M + 255) // 256 * 256
    assert tuple(yb.shape) == (Mp, d)
    want = torch.zeros(Mp, d, dtype=dtype, device=DEV)
    want[:M] = y[0]
    want = want.view(Mp // 256, 256, d // 32, 32).permute(0, 2, 1, 3).reshape(Mp, d)
    got = yb.clone()
    got.view(Mp // 256, d // 32, 256, 32)[-1, :, M % 256:, :] = 0  # rows past M are never written
    assert torch.equal(got, want)
    w = (torch.randn(I, d, device=DEV) * 0.03).to(dtype)
    b = (torch.randn(I, device=DEV) * 0.1).to(dtype)
    r = torch.randn(1, M, I, device=DEV).to(dtype)
    wb = ops.block_weight(w)
    z_plain = ops.gemm_bias_act(y, w, b, "none", residual=r, w_blocked=wb)
    z_blk = ops.gemm_bias_act(yb, w, b, "none", residual=r, w_blocked=wb, x_blocked_shape=tuple(x.shape))
    assert torch.equal(z_blk, z_plain)
    z_plain = ops.gemm_bias_act(y, w, b, "gelu", w_blocked=wb)                      # persistent kernel
    z_blk = ops.gemm_bias_act(yb, w, b, "gelu", w_blocked=wb, x_blocked_shape=tuple(x.shape))
    assert torch.equal(z_blk, z_plain)
    w2 = (torch.randn(d, I, device=DEV) * 0.03).to(dtype)
    b2 = (torch.randn(d, device=DEV) * 0.1).to(dtype)
    w2b = ops.block_weight(w2)
    m_plain = ops.fused_mlp(y, w, b, w2, b2, "gelu", residual=x, fc1_blocked=wb, fc2_blocked=w2b)
    m_blk = ops.fused_mlp(yb, w, b, w2, b2, "gelu", residual=x, fc1_blocked=wb, fc2_blocked=w2b,
                          x_blocked_shape=tuple(x.shape))
    assert torch.equal(m_blk, m_plain)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_layernorm(golden_dir, dtype):
    ops = _ops()
    g = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(golden_dir, "layernorm.npz")).items()}
    x, r, w, b = (g[n].to(dtype) for n in "xrwb")
    y = ops.layernorm(x.to(DEV), w.to(DEV), b.to(DEV), 1e-5)
    _cmp(y, oracle.layernorm(x, w, b, 1e-5), dtype, "ln")
    y2, s2 = ops.layernorm(x.to(DEV), w.to(DEV), b.to(DEV), 1e-5, residual=r.to(DEV), residual_alpha=0.5,
                           return_sum=True)
    summed = (x.double() + 0.5 * r.double()).to(dtype)
    assert (s2.float().cpu() - summed.float()).abs().max() <= 2 * torch.finfo(dtype).eps * summed.abs().max()
    _cmp(y2, oracle.layernorm(s2.cpu(), w, b, 1e-5), dtype, "ln+res")
    for cols in (64, 768, 1280, 4096):
        xx = torch.randn(5, cols).to(dtype)
        ww = torch.randn(cols).to(dtype)
        _cmp(ops.layernorm(xx.to(DEV), ww.to(DEV)), oracle.layernorm(xx, ww), dtype, f"ln{cols}")


def _decode_rows(out, q, kc, vc, bt, ctx, bs, layer, dtype, route, what):
    """The per-row check of tests/_decode_check.py next to _cmp's whole-tensor one (which lets a defect in one long
    sequence of a mixed batch pass): bars from the fp32 model of the same inputs."""
    ref, lse = dc.reference(q, kc, vc, bt, ctx, bs, layer)
    model_o = dc.model(q, kc, vc, bt, ctx, bs, layer, dtype=dtype, p16=route == "gqa")
    dc.check(out, ref, lse, dtype, (dtype, route, "kv16"), model_o, what)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D,H,Hkv,q_len", [
    (64, 4, 4, 1), (128, 8, 2, 1), (80, 2, 2, 3),
    # whole-token-row kernel geometries: row = 2 / 4 wave-loads (H 16: the bench.py decode leg), two query positions,
    # a row of exactly one wave-load with two query heads per kv head
    (64, 16, 16, 1), (128, 16, 16, 1), (64, 8, 8, 2), (64, 16, 8, 1),
    # eight query vectors per kv head (GQA 8: H 32 / Hkv 4, and GQA 4 with two query positions)
    (128, 32, 4, 1), (64, 16, 4, 2),
    # matrix-core GQA kernel (2 .. 16 query vectors per kv head; the two rows above and (64, 8, 8, 2), (64, 16, 8, 1), (128, 8, 2, 1)
    # take it too): 16 (all MFMA columns live), 6 and 12 (not powers of two,
    # three query positions), 16 as 8 heads x 2 positions at D 64, and B 3 (fewer workgroups than CUs)
    (128, 32, 2, 1), (64, 12, 2, 1), (64, 8, 2, 3), (64, 16, 2, 2), (128, 6, 1, 1),
])
def test_paged_decode_and_cache(dtype, D, H, Hkv, q_len):
    ops = _ops()
    torch.manual_seed(D + H)
    B, bs, L, maxb = (3 if H < 8 else 18), 16, 2, 20   # B >= 16 takes the whole-token-row kernel where the geometry fits
    # the kernel each geometry takes: per head at B 3 with one query vector per key at D 64, and at D 80; whole token rows
    # at B 18 with one vector per key at D 64; the matrix core with 2 .. 16 vectors per key, or one at D 128
    route = {(64, 4, 4, 1): "head", (80, 2, 2, 3): "head", (64, 16, 16, 1): "rows"}.get((D, H, Hkv, q_len), "gqa")
    nblk = B * maxb + 4
    ctx = torch.tensor(([300, 17, 0] * 6)[:B], dtype=torch.int32)
    kc = torch.randn(nblk, L, bs, Hkv, D).to(dtype)
    vc = torch.randn(nblk, L, bs, Hkv, D).to(dtype)
    bt = torch.randperm(nblk)[:B * maxb].view(B, maxb).to(torch.int32)  # disjoint physical blocks per sequence
    q = torch.randn(B, H, q_len, D).to(dtype)
    out = torch.empty(B, H, q_len, D, dtype=dtype, device=DEV)
    kcd, vcd = kc.to(DEV), vc.to(DEV)
    assert ops.paged_attention_route(q.to(DEV), out, kcd, vcd, bt.to(DEV), ctx.to(DEV), bs, 320, 1) == route
    ops.paged_attention_forward(q.to(DEV), out, kcd, vcd, bt.to(DEV), ctx.to(DEV), bs, 320, 1)
    ref = oracle.paged_attention_forward(q, kc, vc, bt, ctx, bs, 1)
    _cmp(out, ref, dtype, "paged")
    _decode_rows(out, q, kc, vc, bt, ctx, bs, 1, dtype, route, "paged")
    assert out[2].abs().max() == 0  # empty context -> zeros (attention_kernels.py:802)
    if B > 3:
        ctx[3:] = torch.tensor([319, 256, 1, 64, 129, 255, 318, 16, 15, 33, 100, 200, 7, 303, 48][:B - 3], dtype=torch.int32)
        ops.paged_attention_forward(q.to(DEV), out, kcd, vcd, bt.to(DEV), ctx.to(DEV), bs, 320, 1)
        _cmp(out, oracle.paged_attention_forward(q, kc, vc, bt, ctx, bs, 1), dtype, "paged ragged")
        _decode_rows(out, q, kc, vc, bt, ctx, bs, 1, dtype, route, "paged ragged")
    # cache write for the next token, then decode again: must equal the oracle on the updated cache
    knew, vnew = torch.randn(B, 1, Hkv, D).to(dtype), torch.randn(B, 1, Hkv, D).to(dtype)
    ctx2 = ctx + 1
    ops.reshape_and_cache(knew.to(DEV), vnew.to(DEV), kcd, vcd, bt.to(DEV), ctx2.to(DEV), bs, 1)
    oracle.reshape_and_cache(knew, vnew, kc, vc, bt, ctx2, bs, 1)
    assert torch.equal(kcd.cpu(), kc) and torch.equal(vcd.cpu(), vc)  # byte-exact scatter
    ops.paged_attention_forward(q.to(DEV), out, kcd, vcd, bt.to(DEV), ctx2.to(DEV), bs, 320, 1)
    _cmp(out, oracle.paged_attention_forward(q, kc, vc, bt, ctx2, bs, 1), dtype, "paged+1")
    _decode_rows(out, q, kc, vc, bt, ctx2, bs, 1, dtype, route, "paged+1")


def test_paged_decode_pipelined_batches():
    """Ragged contexts long enough for several double-buffered batches and the split + reduce path; contexts that
    end inside a batch, inside a block, at a split boundary, and one empty sequence."""
    ops = _ops()
    unroll = "2"
    torch.manual_seed(7)
    dtype = torch.bfloat16
    for D, H, Hkv, route in ((64, 4, 4, "head"), (128, 4, 2, "gqa")):   # B 6: per head; two query heads per key: matrix core
        B, bs, L, maxb = 6, 16, 1, 80
        nblk = B * maxb
        ctx = torch.tensor([1280, 1023, 513, 257, 1, 0], dtype=torch.int32)
        kc = torch.randn(nblk, L, bs, Hkv, D).to(dtype)
        vc = torch.randn(nblk, L, bs, Hkv, D).to(dtype)
        bt = torch.randperm(nblk).view(B, maxb).to(torch.int32)
        q = torch.randn(B, H, 1, D).to(dtype)
        out = torch.empty(B, H, 1, D, dtype=dtype, device=DEV)
        assert ops.paged_attention_route(q.to(DEV), out, kc.to(DEV), vc.to(DEV), bt.to(DEV), ctx.to(DEV), bs, 1280, 0) == route
        ops.paged_attention_forward(q.to(DEV), out, kc.to(DEV), vc.to(DEV), bt.to(DEV), ctx.to(DEV), bs, 1280, 0)
        _cmp(out, oracle.paged_attention_forward(q, kc, vc, bt, ctx, bs, 0), dtype, f"paged U={unroll} D={D}")
        _decode_rows(out, q, kc, vc, bt, ctx, bs, 0, dtype, route, f"paged U={unroll} D={D}")
        assert out[5].abs().max() == 0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D,H,Hkv,q_len,bs", [(128, 32, 4, 1, 16), (64, 32, 4, 1, 16), (128, 16, 1, 1, 8), (64, 10, 2, 1, 12),
                                              (128, 8, 1, 2, 1)])
def test_paged_decode_gqa_long_contexts(dtype, D, H, Hkv, q_len, bs):
    """decode_gqa_kernel over contexts of several splits and many 32-key chunks per wave: ends inside a chunk, at a chunk / 128-key /
    split boundary, one key, none; block sizes 16, 8, 12 (not a power of two) and 1; random physical blocks; layer 1 of 2."""
    ops = _ops()
    torch.manual_seed(D + H + bs)
    ctxs = [5000, 4096, 4097, 2047, 1311, 129, 128, 33, 32, 31, 1, 0]
    B, L = len(ctxs), 2
    maxb = (5000 + bs - 1) // bs + 1
    nblk = B * maxb
    ctx = torch.tensor(ctxs, dtype=torch.int32)
    kc = torch.randn(nblk, L, bs, Hkv, D).to(dtype)
    vc = torch.randn(nblk, L, bs, Hkv, D).to(dtype)
    bt = torch.randperm(nblk).view(B, maxb).to(torch.int32)
    q = (torch.randn(B, H, q_len, D) * 1.5).to(dtype)
    out = torch.full((B, H, q_len, D), float("nan"), dtype=dtype, device=DEV)
    assert ops.paged_attention_route(q.to(DEV), out, kc.to(DEV), vc.to(DEV), bt.to(DEV), ctx.to(DEV), bs, 5000, 1) == "gqa"
    ops.paged_attention_forward(q.to(DEV), out, kc.to(DEV), vc.to(DEV), bt.to(DEV), ctx.to(DEV), bs, 5000, 1)
    _cmp(out, oracle.paged_attention_forward(q, kc, vc, bt, ctx, bs, 1), dtype, f"gqa decode D={D} H={H}/{Hkv} q_len={q_len} bs={bs}")
    _decode_rows(out, q, kc, vc, bt, ctx, bs, 1, dtype, "gqa", f"gqa decode D={D} H={H}/{Hkv} q_len={q_len} bs={bs}")
    assert out[-1].abs().max() == 0
    # a strided (non-contiguous in H) output tensor still lands in the right rows
    big = torch.zeros(B, H, q_len, 2 * D, dtype=dtype, device=DEV)
    view = big[..., :D]
    ops.paged_attention_forward(q.to(DEV), view, kc.to(DEV), vc.to(DEV), bt.to(DEV), ctx.to(DEV), bs, 5000, 1)
    assert torch.equal(view, out) and big[..., D:].abs().max() == 0


def _unblock(t, M, N):
    """Blocked activation layout [ceil(M/256), N/32, 256, 32] -> row-major [M, N]."""
    mp = (M + 255) // 256 * 256
    return t.view(mp // 256, N // 32, 256, 32).permute(0, 2, 1, 3).reshape(mp, N)[:M]


def _block(t):
    M, N = t.shape
    mp = (M + 255) // 256 * 256
    pad = torch.zeros(mp, N, dtype=t.dtype, device=t.device)
    pad[:M] = t
    return pad.view(mp // 256, 256, N // 32, 32).permute(0, 2, 1, 3).contiguous().view(mp, N)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("act", ["none", "gelu"])
def test_gemm_ln_fold(dtype, act):
    """LayerNorm folded into the GEMMs on either side of it (mio_gemm_ln_bw): the residual GEMM writes its output blocked +
    the rows' (sum, sum of squares); the projection behind the LayerNorm runs on the raw stream with gamma-scaled weights.
    M 16 500 (ragged last row tile), d 1024 (4 statistic slots), against the oracle's LayerNorm -> linear and, where the
    arithmetic is the same, bit for bit against the unfused kernels."""
    ops = _ops()
    torch.manual_seed(11)
    M, d, N2 = 16500, 1024, 2048
    assert ops.gemm_ln_ok(M, d, d, "none", stats_out=True) and ops.gemm_ln_ok(M, N2, d, act, fold_in=True)
    x0 = torch.randn(M, d).to(dtype)
    r0 = (torch.randn(M, d) * 2 + 1.0).to(dtype)   # a residual stream whose row mean is half its deviation
    wp = (torch.randn(d, d) * 0.03).to(dtype)
    bp = (torch.randn(d) * 0.1).to(dtype)
    gamma, beta = (1 + 0.2 * torch.randn(d)).to(dtype), (0.1 * torch.randn(d)).to(dtype)
    wc = (torch.randn(N2, d) * 0.03).to(dtype)
    bc = (torch.randn(N2) * 0.1).to(dtype)
    x0d, r0d, wpd, bpd, gd, btd, wcd, bcd = (t.to(DEV) for t in (x0, r0, wp, bp, gamma, beta, wc, bc))
    wpb = ops.block_weight(wpd)
    # -- producer: y = x0 wp^T + bp + r0, blocked, + statistics
    yb, st = ops.gemm_ln(x0d, wpb, bpd, M=M, N=d, K=d, residual=r0d, out_blocked=True, stats_out=True)
    y_plain = ops.gemm_bias_act(x0d, wpd, bpd, residual=r0d, w_blocked=wpb)
    y = _unblock(yb, M, d)
    assert torch.equal(y, y_plain)
    assert tuple(st.shape) == (d // 256, (M + 255) // 256 * 256, 2)
    yf = y.float().view(M, d // 256, 256)
    want_s, want_q = yf.sum(-1).t(), (yf * yf).sum(-1).t()
    assert torch.allclose(st[:, :M, 0], want_s, rtol=1e-4, atol=1e-3) and torch.allclose(st[:, :M, 1], want_q, rtol=1e-4, atol=1e-3)
    yb2, st2 = ops.gemm_ln(x0d, wpb, bpd, M=M, N=d, K=d, residual=r0d, out_blocked=True, stats_out=True)
    assert torch.equal(st2[:, :M], st[:, :M]) and torch.equal(_unblock(yb2, M, d), y)   # deterministic (rows past M are never written)
    # -- consumer: z = act(LN(y) wc^T + bc) on the raw blocked stream
    wfb, bfold = ops.ln_fold_weight(wcd, gd, btd, bcd)
    zb, none = ops.gemm_ln(yb, wfb, bfold, M=M, N=N2, K=d, activation=act, x_blocked=True, out_blocked=True,
                           ln_stats=st, eps=1e-5)
    assert none is None
    z = _unblock(zb, M, N2)
    rows = torch.cat([torch.arange(0, M, 61), torch.tensor([255, 256, 16383, 16384, M - 1])])
    yc = y[rows].cpu()
    ln = oracle.layernorm(yc, gamma, beta, 1e-5)          # fp64 LayerNorm of the stored stream (not rounded to 16 bits)
    want = ln.double() @ wc.double().t() + bc.double()
    if act == "gelu":
        want = torch.nn.functional.gelu(want, approximate="tanh")
    _cmp(z[rows], want, dtype, f"ln-fold consumer {act}")
    # the same through row-major operands (x row-major, y row-major)
    z2, _ = ops.gemm_ln(y, wfb, bfold, M=M, N=N2, K=d, activation=act, ln_stats=st)
    assert torch.equal(z2, z)
    # column scale on the folded read-out (the K columns of a QKV projection)
    z3, _ = ops.gemm_ln(yb, wfb, bfold, M=M, N=N2, K=d, activation=act, x_blocked=True, ln_stats=st,
                        col_scale=(1024, 2048, 0.25))
    assert torch.equal(z3[:, :1024], z[:, :1024])
    _cmp(z3[rows][:, 1024:], want[:, 1024:] * 0.25, dtype, "ln-fold consumer + col_scale")
    # -- a second residual GEMM reading the BLOCKED stream as its residual, row-major output, no statistics
    w2 = (torch.randn(d, N2) * 0.02).to(dtype).to(DEV)
    w2b = ops.block_weight(w2)
    o_blk, _ = ops.gemm_ln(zb, w2b, bpd, M=M, N=d, K=N2, x_blocked=True, residual=yb, res_blocked=True)
    o_plain = ops.gemm_bias_act(z, w2, bpd, residual=y, w_blocked=w2b)
    assert torch.equal(o_blk, o_plain)


@pytest.mark.parametrize("mean_over_std", [1.0, 4.0])
def test_gemm_ln_fold_stream_with_large_mean(mean_over_std):
    """The centred-weight form must not care about the stream's mean: mio_ln_fold_weight picks rounding directions so that every
    prepared weight row sums to zero within an ulp or two (plain rounding leaves ~9 ulp, and the output then carries mean(x) times
    that: 2.8e-3 / 7.1e-3 at |mean| = 1x / 4x the deviation).  Streams whose row mean is 1x and 4x their deviation, bf16, against
    the oracle, beside the LayerNorm kernel + GEMM on the same data (2.3e-3)."""
    _fold_stream_with_large_mean(torch.bfloat16, mean_over_std)


@pytest.mark.parametrize("mean_over_std", [1.0, 4.0])
def test_gemm_ln_fold_stream_with_large_mean_fp16(mean_over_std):
    """The same in fp16 (ulp 2^-10 of the row's largest element; the mean relative error stays under the fold tests' fp16 bar)."""
    _fold_stream_with_large_mean(torch.float16, mean_over_std)


def _fold_stream_with_large_mean(dtype, mean_over_std):
    ops = _ops()
    torch.manual_seed(31)
    ulp_rel = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}[dtype]
    M, d, N2 = 16384, 1024, 1024
    x0 = torch.randn(M, d).to(dtype)
    r0 = (torch.randn(M, d) * 2 + 2.2 * mean_over_std).to(dtype)
    wp, bp = (torch.randn(d, d) * 0.03).to(dtype), (torch.randn(d) * 0.1).to(dtype)
    gamma, beta = (1 + 0.2 * torch.randn(d)).to(dtype), (0.1 * torch.randn(d)).to(dtype)
    wc, bc = (torch.randn(N2, d) * 0.03).to(dtype), (torch.randn(N2) * 0.1).to(dtype)
    dv = lambda t: t.to(DEV)
    yb, st = ops.gemm_ln(dv(x0), ops.block_weight(dv(wp)), dv(bp), M=M, N=d, K=d, residual=dv(r0), out_blocked=True, stats_out=True)
    wfb, bfold = ops.ln_fold_weight(dv(wc), dv(gamma), dv(beta), dv(bc))
    # the prepared rows sum to zero within an ulp or two of their largest element (plain rounding leaves ~ sqrt(K / 12) = 9 ulp)
    ws, _ = ops.ln_fold_weight(dv(wc), dv(gamma), dv(beta), dv(bc), blocked=False)
    ulp = ws.float().abs().amax(1) * ulp_rel
    assert (ws.float().sum(1).abs() <= 2 * ulp).all(), (ws.float().sum(1).abs() / ulp).max().item()
    if dtype == torch.bfloat16:
        exact = wc.float() * gamma.float()
        exact = exact - exact.mean(1, keepdim=True)
        assert ((ws.float().cpu() - exact).abs() <= exact.abs() * ulp_rel + 1e-30).all()   # every element still a neighbour of its exact value
    else:
        # fp16: the spacing is 2^-24 below 2^-14, and an element near zero is smaller than the kernel's fp32 error of the row mean
        # (K + 1 roundings of one fp32 ulp on mean|w gamma|): both are part of "a neighbour" here (tests/test_gpu_gemm_matrix.py
        # test_ln_fold_weight_rows has the exact form)
        exact = wc.double() * gamma.double()
        slack = (d + 1) * 2.0 ** -23 * exact.abs().mean(1, keepdim=True)
        exact = exact - exact.mean(1, keepdim=True)
        assert ((ws.double().cpu() - exact).abs() <= (exact.abs() * ulp_rel).clamp_min(2.0 ** -24) + slack).all()
    z, _ = ops.gemm_ln(yb, wfb, bfold, M=M, N=N2, K=d, x_blocked=True, ln_stats=st)
    rows = torch.arange(0, M, 127)
    y = _unblock(yb, M, d)[rows].cpu()
    ratio = (y.float().mean(-1).abs() / y.float().std(-1)).mean().item()
    assert 0.7 * mean_over_std < ratio < 1.4 * mean_over_std, ratio
    want = oracle.layernorm(y, gamma, beta, 1e-5).double() @ wc.double().t() + bc.double()
    rel = ((z[rows].double().cpu() - want).abs().mean() / want.abs().mean()).item()
    unfused = ops.gemm_bias_act(ops.layernorm(_unblock(yb, M, d)[rows].contiguous().view(1, -1, d), dv(gamma), dv(beta)), dv(wc), dv(bc))
    rel_unfused = ((unfused[0].double().cpu() - want).abs().mean() / want.abs().mean()).item()
    print(f"|mean|/std {ratio:.2f}: folded rel_err {rel:.3e}, LayerNorm kernel + GEMM {rel_unfused:.3e}")
    assert rel < TOL[dtype][0] and rel < 1.15 * rel_unfused, (rel, rel_unfused)


def test_gemm_ln_fold_wide_stream():
    """A stream of 4096 columns (LLaMA-7B width): the producer writes 16 statistic slots, ops.gemm_ln sums them in pairs
    (mio_ln_stats_reduce) for the consumer, whose folded weight rows are 4096 long; M 4096 (256 tiles), bf16, against the oracle."""
    ops = _ops()
    torch.manual_seed(41)
    dtype = torch.bfloat16
    M, d, N2 = 4096, 4096, 4096
    assert ops.gemm_ln_ok(M, d, d, "none", stats_out=True) and ops.gemm_ln_ok(M, N2, d, "gelu", fold_in=True)
    x0 = torch.randn(M, d).to(dtype)
    r0 = (torch.randn(M, d) * 2 + 0.7).to(dtype)
    wp, bp = (torch.randn(d, d) * 0.015).to(dtype), (torch.randn(d) * 0.1).to(dtype)
    gamma, beta = (1 + 0.2 * torch.randn(d)).to(dtype), (0.1 * torch.randn(d)).to(dtype)
    wc, bc = (torch.randn(N2, d) * 0.015).to(dtype), (torch.randn(N2) * 0.1).to(dtype)
    dv = lambda t: t.to(DEV)
    yb, st = ops.gemm_ln(dv(x0), ops.block_weight(dv(wp)), dv(bp), M=M, N=d, K=d, residual=dv(r0), out_blocked=True, stats_out=True)
    assert st.shape[0] == 16
    y = _unblock(yb, M, d)
    yf = y.float().view(M, 16, 256)
    assert torch.allclose(st[:, :M, 0], yf.sum(-1).t(), rtol=1e-4, atol=1e-3) and torch.allclose(st[:, :M, 1], (yf * yf).sum(-1).t(), rtol=1e-4, atol=1e-3)
    wfb, bfold = ops.ln_fold_weight(dv(wc), dv(gamma), dv(beta), dv(bc))
    ws, _ = ops.ln_fold_weight(dv(wc), dv(gamma), dv(beta), dv(bc), blocked=False)
    assert (ws.float().sum(1).abs() <= 2 * ws.float().abs().amax(1) * 2.0 ** -7).all()
    z, _ = ops.gemm_ln(yb, wfb, bfold, M=M, N=N2, K=d, activation="gelu", x_blocked=True, ln_stats=st)
    rows = torch.arange(0, M, 37)
    want = torch.nn.functional.gelu(oracle.layernorm(y[rows].cpu(), gamma, beta, 1e-5).double() @ wc.double().t() + bc.double(), approximate="tanh")
    _cmp(z[rows], want, dtype, "ln-fold consumer, 4096-column stream")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_gemm_ln_fold_swiglu(dtype):
    """The consumer form of the LayerNorm fold on the gated stage: silu(LN(y) Wg^T + bg) * (LN(y) Wu^T + bu) with the two folded
    weights interleaved in one blocked weight, the raw blocked stream + statistics of a producer as input, against the oracle."""
    ops = _ops()
    torch.manual_seed(21)
    M, d, I = 16500, 1024, 2048
    assert ops.gemm_ln_ok(M, I, d, "swiglu", fold_in=True)
    x0 = torch.randn(M, d).to(dtype)
    r0 = (torch.randn(M, d) * 1.5 + 0.4).to(dtype)
    wp, bp = (torch.randn(d, d) * 0.03).to(dtype), (torch.randn(d) * 0.1).to(dtype)
    gamma, beta = (1 + 0.2 * torch.randn(d)).to(dtype), (0.1 * torch.randn(d)).to(dtype)
    wg, wu = ((torch.randn(I, d) * 0.03).to(dtype) for _ in range(2))
    bg, bu = ((torch.randn(I) * 0.1).to(dtype) for _ in range(2))
    dv = lambda t: t.to(DEV)
    yb, st = ops.gemm_ln(dv(x0), ops.block_weight(dv(wp)), dv(bp), M=M, N=d, K=d, residual=dv(r0), out_blocked=True, stats_out=True)
    wgf, bgf = ops.ln_fold_weight(dv(wg), dv(gamma), dv(beta), dv(bg), blocked=False)
    wuf, buf = ops.ln_fold_weight(dv(wu), dv(gamma), dv(beta), dv(bu), blocked=False)
    hb, _ = ops.gemm_ln(yb, ops.block_weight_glu(wgf, wuf), buf, M=M, N=I, K=d, activation="swiglu", x_blocked=True, out_blocked=True,
                        ln_stats=st, bias_gate=bgf)
    h = _unblock(hb, M, I)
    rows = torch.cat([torch.arange(0, M, 67), torch.tensor([255, 256, 16383, 16384, M - 1])])
    ln = oracle.layernorm(_unblock(yb, M, d)[rows].cpu(), gamma, beta, 1e-5).double()
    want = torch.nn.functional.silu(ln @ wg.double().t() + bg.double()) * (ln @ wu.double().t() + bu.double())
    _cmp(h[rows], want, dtype, "ln-fold consumer swiglu")


def test_errors_raise_before_launch():
    ops = _ops()
    q = torch.randn(1, 8, 2, 64, dtype=torch.float16, device=DEV)
    with pytest.raises(ValueError):
        ops.flash_attention(q[0], q, q)
    with pytest.raises(ValueError):
        ops.flash_attention(q.cpu(), q.cpu(), q.cpu())
    with pytest.raises(NotImplementedError):
        ops.flash_attention(q, q, q, return_softmax=True)
    with pytest.raises(ValueError):
        ops.fused_mlp(q[0], q, None, q, None)
    x = torch.randn(1, 4, 64, dtype=torch.float16, device=DEV)
    w1 = torch.randn(128, 64, dtype=torch.float16, device=DEV)
    w2 = torch.randn(64, 128, dtype=torch.float16, device=DEV)
    with pytest.raises(ValueError):
        ops.fused_mlp(x, w1, None, w2, None, "swiglu")
    with pytest.raises(ValueError):
        ops.fused_mlp(x, w1, None, w2, None, "tanh")
    with pytest.raises(ValueError):
        ops.flash_attention(q.float(), q.float(), q.float())
    # per-column operands and residuals are read through raw pointers: dtype / length / contiguity are checked first
    xl = torch.randn(2, 8, 64, dtype=torch.bfloat16, device=DEV)
    wl = torch.ones(64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError):
        ops.layernorm(xl, wl.float())                      # fp32 nn.LayerNorm weight with bf16 activations
    with pytest.raises(ValueError):
        ops.layernorm(xl, wl[:32])                         # shorter than cols: would be an out-of-bounds device read
    with pytest.raises(ValueError):
        ops.layernorm(xl, torch.ones(128, dtype=torch.bfloat16, device=DEV)[::2])  # not contiguous
    with pytest.raises(ValueError):
        ops.layernorm(xl, wl, wl.float())
    with pytest.raises(ValueError):
        ops.layernorm(xl, wl, residual=xl.float())
    wg = torch.randn(32, 64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError):
        ops.gemm_bias_act(xl, wg, torch.zeros(32, device=DEV))               # fp32 bias
    with pytest.raises(ValueError):
        ops.gemm_bias_act(xl, wg, torch.zeros(16, dtype=torch.bfloat16, device=DEV))  # short bias
    with pytest.raises(ValueError):
        ops.gemm_bias_act(xl, wg, residual=torch.zeros(2, 8, 32, device=DEV))  # fp32 residual
    w1b = torch.randn(128, 64, dtype=torch.bfloat16, device=DEV)
    w2b = torch.randn(64, 128, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError):
        ops.fused_mlp(xl, w1b, torch.zeros(128, device=DEV), w2b, None)      # fp32 fc1 bias
    with pytest.raises(ValueError):
        ops.fused_mlp(xl, w1b, None, w2b, torch.zeros(32, dtype=torch.bfloat16, device=DEV))  # short fc2 bias
    with pytest.raises(ValueError):
        ops.fused_mlp(xl, w1b, None, w2b, None, residual=xl.float())
    # the folded GEMM entry point: operands travel as raw pointers, every shape / dtype / flag combination is checked first
    Mf, df = 16384, 1024
    xf = torch.zeros(Mf, df, dtype=torch.bfloat16, device=DEV)
    wf = ops.block_weight(torch.zeros(df, df, dtype=torch.bfloat16, device=DEV))
    stf = torch.zeros(ops.ln_stats_shape(Mf, df), dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError):
        ops.gemm_ln(xf, wf, None, M=Mf, N=df, K=df, stats_out=True)                       # the producer form is the residual epilogue
    with pytest.raises(ValueError):
        ops.gemm_ln(xf, wf, None, M=Mf, N=df, K=df, ln_stats=stf, residual=xf)            # the consumer form takes no residual
    with pytest.raises(ValueError):
        ops.gemm_ln(xf, wf, None, M=Mf, N=df, K=df, ln_stats=stf[:, :256])                # statistics of another row count
    with pytest.raises(ValueError):
        ops.gemm_ln(xf, wf, None, M=Mf, N=df, K=df, ln_stats=stf.double())                # fp64 statistics
    with pytest.raises(ValueError):
        ops.gemm_ln(xf[:256], wf, None, M=Mf, N=df, K=df, x_blocked=True)                 # a blocked operand of the wrong size
    with pytest.raises(ValueError):
        ops.gemm_ln(xf, wf[:512], None, M=Mf, N=df, K=df)                                 # a truncated blocked weight
    with pytest.raises(ValueError):
        ops.gemm_ln(xf, wf, None, M=Mf, N=df, K=df, residual=xf, col_scale=(0, 128, 2.0))  # column scale with a residual
    with pytest.raises(ValueError):
        ops.gemm_ln(xf, wf, None, M=Mf, N=df, K=df, bias_gate=torch.zeros(df, dtype=torch.bfloat16, device=DEV))  # gate bias without swiglu
    with pytest.raises(ValueError):
        ops.gemm_ln(xf[:1000], wf, None, M=1000, N=df, K=df)                              # too few tiles for the folded kernels
    assert not ops.gemm_ln_ok(Mf, df, 1280 + 64, "none", fold_in=True)                   # K % 256 != 0
    assert not ops.gemm_ln_ok(Mf, df, df, "relu", fold_in=True)                          # activations without a folded instantiation


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_fused_mlp_swiglu_blocked_glu_weight(dtype):
    """SwiGLU on the 256-tile kernels (interleaved gate / up blocked weight, ops.block_weight_glu) at a shape with a ragged
    last row tile (M = 8200), one missing bias and a residual; against the oracle and the plain dual-B path."""
    ops = _ops()
    M, d, I = 8200, 2048, 2048
    assert ops.fused_mlp_blocked_weight_ok(M, d, I, "swiglu")
    torch.manual_seed(5)
    x = torch.randn(1, M, d).to(dtype)
    r = torch.randn(1, M, d).to(dtype)
    wu, wg, w2 = ((torch.randn(*s) * 0.03).to(dtype) for s in ((I, d), (I, d), (d, I)))
    bu, b2 = (torch.randn(I) * 0.1).to(dtype), (torch.randn(d) * 0.1).to(dtype)
    rows = torch.cat([torch.arange(0, M, 97), torch.tensor([255, 256, 8191, 8192, M - 1])])
    want = oracle.fused_mlp(x[0, rows], wu, bu, w2, b2, "swiglu", wg, None, residual=r[0, rows])
    xd, rd, wud, wgd, w2d, bud, b2d = (t.to(DEV) for t in (x, r, wu, wg, w2, bu, b2))
    y = ops.fused_mlp(xd, wud, bud, w2d, b2d, "swiglu", wgd, None, residual=rd, fc1_blocked=ops.block_weight_glu(wgd, wud),
                      fc2_blocked=ops.block_weight(w2d))
    got, refd = y[0, rows.to(DEV)].float().cpu(), want.to(dtype).float()
    rel = ((got - refd).abs().mean() / refd.abs().mean()).item()
    assert rel < (2e-3 if dtype == torch.float16 else 5e-3), f"rel_err={rel:.3e}"  # (bars of test_fused_mlp_vs_oracle)
    y_plain = ops.fused_mlp(xd, wud, bud, w2d, b2d, "swiglu", wgd, None, residual=rd)
    tol = 2e-2 if dtype == torch.bfloat16 else 3e-3
    assert (y.float() - y_plain.float()).abs().max().item() < tol * max(1.0, y_plain.float().abs().max().item())
    with pytest.raises(ValueError):  # a plain blocked weight is not the interleaved one
        ops.fused_mlp(xd, wud, bud, w2d, b2d, "swiglu", wgd, None, fc1_blocked=ops.block_weight(wud)[:1],
                      fc2_blocked=ops.block_weight(w2d))

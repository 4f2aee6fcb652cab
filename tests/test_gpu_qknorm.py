"""QK-norm on the GPU: the per-head RMSNorm of q and k fused into the rotating paged-cache write
(ops.qknorm_rope_and_cache_varlen, 16-bit and fp8 caches), the standalone form (ops.qk_norm_rotary) and FlashSelfAttention with
qk_norm=True.

q_out and the cached K are judged by the derived interval of tests/_qknorm_check.py (zero elements outside; no measured
tolerance); V is compared byte for byte with what ops.reshape_and_cache_varlen writes; every other cache byte must keep its
poison; the fused q_out must equal the standalone form bit for bit; and against the two-step 16-bit chain (torch RMSNorm rounded
to 16 bits, then ops.rope_and_cache_varlen) the fused result's summed error against fp64 must be no larger.  The shapes are the
smallest that reach the seams of the kernel's lane groups (module docstring of csrc/qknorm_rope.hip): rows per wave that do
not divide it, ten units in a group of sixteen, partial rotation.
"""
import pytest
import torch

import _decode_check as dc
import _qknorm_check as qc
import test_gpu_rope as tr

pytestmark = pytest.mark.gpu

DEV = "cuda"
F8 = torch.float8_e4m3fn
DTYPES = [torch.bfloat16, torch.float16]
POISON8 = 0x7F  # e4m3fn NaN
EPS = 1e-6
# (H, Hkv, D, rot)
SHAPES = [(3, 1, 64, 64),    # group counts that do not divide a wave
          (4, 2, 128, 128),
          (5, 5, 80, 48),    # 16-bit cache only; 10 units per row (interleaved): idle lanes in a group of 16; partial rotation
          (2, 1, 96, 32)]


def _ops():
    from mio import ops
    return ops


def _bytes(t):
    return t.detach().cpu().contiguous().view(torch.uint8)


def _kv8_ok(D, rot, il):
    return D % 16 == 0 and (il or rot % 32 == 0)


class _Scene:
    """Packed new tokens of several sequences (new[b] tokens after cached[b] cached ones, block size 16) plus one packed token
    outside every sequence.  One block-table entry of the last sequence is -1 where it has more than one block in play: the
    tokens of that block get no cache row but still get their q.  With use_positions the rotation positions are the cache
    positions + 3, except one token whose position lies outside the table (its cache row is left alone, its q_out row is zeros).
    q / k / v are strided views of one [T, (H + 2 Hkv) D] projection result; the heads are scaled by different powers of two,
    x is not centred, and the two norm weights differ and vary with d."""

    def __init__(self, dtype, kv8, H, Hkv, D, rot, *, new, cached, use_positions, seed, L=2, layer=1, bs=16):
        g = torch.Generator().manual_seed(seed)
        self.dtype, self.kv8, self.H, self.Hkv, self.D, self.rot, self.bs, self.L, self.layer = dtype, kv8, H, Hkv, D, rot, bs, L, layer
        B = len(new)
        self.after = [c + n for c, n in zip(cached, new)]
        M = max(self.after) // bs + 1
        self.M, self.T = M, sum(new) + 1
        self.maxpos = M * bs + 8
        self.nb = B * M + 2
        self.bt = torch.randperm(self.nb, generator=g)[:B * M].view(B, M).to(torch.int32)
        if new[-1] > bs:
            self.bt[B - 1, (cached[-1] // bs) + 1] = -1
        self.cu = torch.tensor([0] + [sum(new[:i + 1]) for i in range(B)], dtype=torch.int32)
        self.cl = torch.tensor(self.after, dtype=torch.int32)
        self.seq = torch.full((self.T,), -1, dtype=torch.long)
        self.cpos = torch.zeros(self.T, dtype=torch.long)
        t = 0
        for b, n in enumerate(new):
            self.seq[t:t + n] = b
            self.cpos[t:t + n] = torch.arange(cached[b], cached[b] + n)
            t += n
        if use_positions:
            rp = self.cpos + 3
            rp[min(3, self.T - 2)] = self.maxpos + 5     # outside the table
            rp[self.T - 1] = 5                           # the stray token: still outside every sequence
            self.positions = rp.to(torch.int32)
        else:
            rp = self.cpos.clone()
            self.positions = None
        self.rpos = rp
        self.live = (self.seq >= 0) & (rp >= 0) & (rp < self.maxpos)
        blk = self.bt[self.seq.clamp_min(0), (self.cpos // bs).clamp_max(M - 1)].long()
        self.has_row = (self.seq >= 0) & (blk >= 0)
        self.blk, self.slot = blk.clamp_min(0), self.cpos % bs
        heads = H + 2 * Hkv
        scale = torch.tensor([2.0 ** -10, 2.0 ** -3, 1.0, 2.0 ** 3, 2.0 ** -6])[torch.arange(heads) % 5]
        x = (torch.randn(self.T, heads, D, generator=g) + 0.5) * scale[None, :, None]
        self.qkv = x.to(dtype).view(self.T, heads * D)
        self.wq = (0.5 + torch.rand(D, generator=g)).to(dtype)
        self.wk = (1.5 - torch.rand(D, generator=g) * torch.linspace(0.2, 1.0, D)).to(dtype)
        self.cos, self.sin = _ops().rope_tables(self.maxpos, rot, 10000.0)
        self.k_scale = [0.9, 0.043] if kv8 else None   # |k| after the norm is about 1.5 |w|: nothing saturates, nothing is tiny
        self.v_scale = [1.3, 0.02] if kv8 else None

    def views(self, buf):
        H, Hkv, D = self.H, self.Hkv, self.D
        q = buf[:, :H * D].view(self.T, H, D)
        k = buf[:, H * D:(H + Hkv) * D].view(self.T, Hkv, D)
        v = buf[:, (H + Hkv) * D:].view(self.T, Hkv, D)
        return q, k, v

    def caches(self):
        shape = (self.nb, self.L, self.bs, self.Hkv, self.D)
        if self.kv8:
            c = torch.full(shape, POISON8, dtype=torch.uint8, device=DEV).view(F8)
        else:
            c = torch.full(shape, float("nan"), dtype=self.dtype, device=DEV)
        return c, c.clone()

    def scales(self):
        if not self.kv8:
            return {}
        return dict(k_scale=torch.tensor(self.k_scale, dtype=torch.float32, device=DEV),
                    v_scale=torch.tensor(self.v_scale, dtype=torch.float32, device=DEV))


def _sum_err(y, ref):
    return (y.double() - ref).abs().sum().item()


def _run_scene(sc, il, alias):
    """One fused write of a scene and every bar of the module docstring on it."""
    ops = _ops()
    dev = lambda t: None if t is None else t.to(DEV)  # noqa: E731
    buf = sc.qkv.to(DEV)
    q, k, v = sc.views(buf)
    q_cpu, k_cpu, v_cpu = sc.views(sc.qkv)
    bt, cu, cl, cos, sin, pos = dev(sc.bt), dev(sc.cu), dev(sc.cl), dev(sc.cos), dev(sc.sin), dev(sc.positions)
    wq, wk = dev(sc.wq), dev(sc.wk)
    kc, vc = sc.caches()
    kc2, vc2 = sc.caches()
    kc3, vc3 = sc.caches()
    kw = dict(positions=pos, interleaved=il, **sc.scales())
    # before q may be overwritten in place: the plain write (V's bytes), the standalone form, the two-step chain
    ops.reshape_and_cache_varlen(k, v, kc2, vc2, bt, cu, cl, sc.bs, sc.layer, **sc.scales())
    rp = torch.where(sc.seq >= 0, sc.rpos, torch.full_like(sc.rpos, -1)).to(torch.int32).to(DEV)
    q_rows = ops.qk_norm_rotary(q, wq, cos, sin, rp, eps=EPS, interleaved=il)
    q_chain = ops.rope_and_cache_varlen(qc.rms16(q, wq, EPS), qc.rms16(k, wk, EPS), v, kc3, vc3, bt, cu, cl, sc.bs, sc.layer,
                                        cos, sin, **kw)
    torch.cuda.synchronize()
    assert torch.equal(buf.cpu(), sc.qkv)  # none of them touched its inputs
    q_out = q if alias else torch.full((sc.T, sc.H, sc.D), float("nan"), dtype=sc.dtype, device=DEV)
    got = ops.qknorm_rope_and_cache_varlen(q, k, v, kc, vc, bt, cu, cl, sc.bs, sc.layer, cos, sin, wq, wk, eps=EPS, q_out=q_out,
                                           **kw)
    torch.cuda.synchronize()
    assert got.data_ptr() == q_out.data_ptr()
    qo, live = q_out.cpu(), sc.live
    # k and v are never modified, whatever q_out aliases
    assert torch.equal(_bytes(sc.views(buf.cpu())[1]), _bytes(k_cpu)) and torch.equal(_bytes(sc.views(buf.cpu())[2]), _bytes(v_cpu))
    # ---- q_out: dead rows exactly zero, live rows inside the interval, the whole bit-equal to the standalone form
    assert not torch.isnan(qo.float()).any()
    assert int((~live).sum()) == (2 if sc.positions is not None else 1)
    assert (_bytes(qo[~live]) == 0).all()
    ref_q, dq = qc.reference(q_cpu[live], sc.wq, EPS, sc.cos, sc.sin, sc.rpos[live], il)
    out, differ = qc.outside16(qo[live], ref_q, dq, sc.dtype)
    print(f"q_out: {ref_q.numel()} elements, {out} outside the interval, {differ} differ from RN(ref)")
    assert out == 0
    assert torch.equal(_bytes(qo), _bytes(q_rows))
    # ---- caches: V's bytes are the plain write's on the written rows, every other byte of both caches keeps its poison
    kcb, vcb, vc2b = kc.cpu(), vc.cpu(), vc2.cpu()
    wr = live & sc.has_row
    blk, slot = sc.blk[wr], sc.slot[wr]
    exp_v = sc.caches()[1].cpu()
    exp_v[blk, sc.layer, slot] = vc2b[blk, sc.layer, slot]
    assert torch.equal(_bytes(vcb), _bytes(exp_v))
    krows = kcb[blk, sc.layer, slot]             # [n, Hkv, D]
    exp_k = sc.caches()[0].cpu()
    exp_k[blk, sc.layer, slot] = krows           # the written rows are judged below, not here
    assert torch.equal(_bytes(kcb), _bytes(exp_k))
    assert int(wr.sum()) >= 6 and (sc.T < 30 or int((live & ~sc.has_row).sum()) >= 8)
    ref_k, dk = qc.reference(k_cpu[wr], sc.wk, EPS, sc.cos, sc.sin, sc.rpos[wr], il)
    if sc.kv8:
        out = qc.outside8(krows, ref_k, dk, sc.k_scale[sc.layer])
        sat = int((krows.float().abs() == 448).sum())
        print(f"fp8 K: {ref_k.numel()} elements, {out} outside the interval, {sat} saturated")
        assert sat == 0
    else:
        out, differ = qc.outside16(krows, ref_k, dk, sc.dtype)
        print(f"K: {ref_k.numel()} elements, {out} outside the interval, {differ} differ from RN(ref)")
    assert out == 0
    # ---- against the two-step chain: one rounding is no worse than two
    e_f, e_c = _sum_err(qo[live], ref_q), _sum_err(q_chain.cpu()[live], ref_q)
    print(f"q summed |error|: fused {e_f:.6g}, chain {e_c:.6g}")
    assert e_f <= e_c
    crows = kc3.cpu()[blk, sc.layer, slot]
    if sc.kv8:
        inv = (torch.tensor(1.0) / torch.tensor(sc.k_scale[sc.layer])).double()
        e_f, e_c = _sum_err(krows.float(), ref_k * inv), _sum_err(crows.float(), ref_k * inv)
    else:
        e_f, e_c = _sum_err(krows, ref_k), _sum_err(crows, ref_k)
    print(f"K summed |error|: fused {e_f:.6g}, chain {e_c:.6g}")
    assert e_f <= e_c
    return qo


# every shape with both pairings over a 16-bit cache, and over an fp8 cache where its head_dim / rot_dim rules allow
FUSED_CASES = [(*s, il, kv8) for s in SHAPES for il in (False, True) for kv8 in (False, True)
               if not kv8 or _kv8_ok(s[2], s[3], il)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H,Hkv,D,rot,il,kv8", FUSED_CASES)
def test_qknorm_rope_and_cache_varlen(dtype, H, Hkv, D, rot, il, kv8):
    """Three sequences of 1, 5 and 31 new tokens after 0, 16 and 40 cached ones and a token outside every sequence; q_out
    aliasing q or separate, positions given or the cache positions."""
    i = SHAPES.index((H, Hkv, D, rot))
    for alias in (False, True):
        for use_positions in (False, True):
            sc = _Scene(dtype, kv8, H, Hkv, D, rot, new=[1, 5, 31], cached=[0, 16, 40], use_positions=use_positions,
                        seed=1000 * i + 100 * il + 10 * kv8 + 2 * alias + use_positions)
            _run_scene(sc, il, alias)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("il", [False, True])
@pytest.mark.parametrize("H,Hkv,D,rot", SHAPES)
def test_qknorm_decode_step(dtype, il, H, Hkv, D, rot):
    """A decode step: 7 sequences x 1 token (and the stray one), the same bars."""
    i = SHAPES.index((H, Hkv, D, rot))
    for kv8 in (False, True):
        if kv8 and not _kv8_ok(D, rot, il):
            continue
        sc = _Scene(dtype, kv8, H, Hkv, D, rot, new=[1] * 7, cached=[0, 15, 16, 17, 31, 40, 63], use_positions=bool(i % 2),
                    seed=77 + 10 * i + il + 2 * kv8)
        _run_scene(sc, il, alias=bool((i + il) % 2))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("il", [False, True])
def test_qknorm_special_rows_and_forms(dtype, il):
    """A zero row gives zeros and a NaN makes its own head NaN and no other, in both forms; the [B, S, heads, D] form with [S]
    and [B, S] positions agrees with the packed one; in place equals out of place."""
    ops = _ops()
    g = torch.Generator().manual_seed(11)
    B, S, Hn, D, rot, P = 2, 9, 3, 80, 48, 32
    cos, sin = (t.to(DEV) for t in ops.rope_tables(P, rot))
    w = (0.5 + torch.rand(D, generator=g)).to(dtype).to(DEV)
    wide = (torch.randn(B, S, 2 * Hn * D, generator=g) + 0.5).to(dtype)
    x_cpu = wide[:, :, Hn * D:].view(B, S, Hn, D)
    x_cpu[0, 2, 1] = 0
    x_cpu[1, 4, 0, 77] = float("nan")
    x = wide.to(DEV)[:, :, Hn * D:].view(B, S, Hn, D)  # a strided view whose batch and sequence axes collapse
    pos1 = torch.arange(S, dtype=torch.int32, device=DEV)
    y1 = ops.qk_norm_rotary(x, w, cos, sin, pos1, eps=EPS, interleaved=il)
    y2 = ops.qk_norm_rotary(x, w, cos, sin, pos1.expand(B, S).contiguous(), eps=EPS, interleaved=il)
    y3 = ops.qk_norm_rotary(x.reshape(B * S, Hn, D), w, cos, sin, pos1.repeat(B), eps=EPS, interleaved=il)
    xin = x.clone()
    assert ops.qk_norm_rotary(xin, w, cos, sin, pos1, eps=EPS, interleaved=il, out=xin).data_ptr() == xin.data_ptr()
    torch.cuda.synchronize()
    y = y1.cpu()
    assert y1.shape == x.shape and torch.equal(_bytes(y1), _bytes(y2)) and torch.equal(_bytes(y1.view(B * S, Hn, D)), _bytes(y3))
    assert torch.equal(_bytes(xin), _bytes(y1))
    assert (y[0, 2, 1] == 0).all()  # zeros of either sign: 0 * c - 0 * s is -0 where c < 0
    assert torch.isnan(y[1, 4, 0].float()).all()
    ok = torch.ones(B, S, Hn, dtype=torch.bool)
    ok[1, 4, 0] = False
    assert not torch.isnan(y[ok].float()).any()
    xr = x_cpu.reshape(B * S, Hn, D).clone()
    xr[S + 4, 0] = 0  # the reference of the NaN head is not judged
    ref, delta = qc.reference(xr, w.cpu(), EPS, cos.cpu(), sin.cpu(), pos1.repeat(B).cpu().long(), il)
    assert qc.outside16(y.view(B * S, Hn, D)[ok.view(B * S, Hn)], ref[ok.view(B * S, Hn)], delta[ok.view(B * S, Hn)], dtype)[0] == 0


def test_qknorm_ops_argument_errors():
    """Each malformed argument of the two ops functions raises ValueError before any launch."""
    ops = _ops()
    bf = torch.bfloat16
    T, H, Hkv, D, bs = 6, 4, 2, 64, 16
    q = torch.zeros(T, H, D, dtype=bf, device=DEV)
    k = torch.zeros(T, Hkv, D, dtype=bf, device=DEV)
    kc = torch.zeros(4, 1, bs, Hkv, D, dtype=bf, device=DEV)
    k8 = torch.zeros(4, 1, bs, Hkv, D, dtype=torch.uint8, device=DEV).view(F8)
    bt = torch.zeros(1, 4, dtype=torch.int32, device=DEV)
    cu = torch.tensor([0, T], dtype=torch.int32, device=DEV)
    cl = torch.tensor([T], dtype=torch.int32, device=DEV)
    cos, sin = (t.to(DEV) for t in ops.rope_tables(32, 32))
    w = torch.ones(D, dtype=bf, device=DEV)
    one = torch.ones(1, device=DEV)
    f = ops.qknorm_rope_and_cache_varlen
    assert f(q, k, k, kc, kc, bt, cu, cl, bs, 0, cos, sin, w, w).shape == q.shape
    bad_w = [w.cpu(), w.half(), w[:32], torch.ones(2 * D, dtype=bf, device=DEV)[::2], torch.ones(D + 8, dtype=bf, device=DEV)[4:D + 4]]
    for bw in bad_w:
        with pytest.raises(ValueError):
            f(q, k, k, kc, kc, bt, cu, cl, bs, 0, cos, sin, bw, w)
        with pytest.raises(ValueError):
            f(q, k, k, kc, kc, bt, cu, cl, bs, 0, cos, sin, w, bw)
        with pytest.raises(ValueError):
            ops.qk_norm_rotary(q, bw, cos, sin, torch.zeros(T, dtype=torch.int32, device=DEV))
    for kw in (dict(eps=-1.0), dict(eps=float("nan")), dict(positions=torch.zeros(T, dtype=torch.int64, device=DEV)),
               dict(q_out=torch.zeros(T, H, D, dtype=torch.float16, device=DEV)), dict(k_scale=one, v_scale=one)):
        with pytest.raises(ValueError):
            f(q, k, k, kc, kc, bt, cu, cl, bs, 0, cos, sin, w, w, **kw)
    with pytest.raises(ValueError):
        f(q, k, k, k8, k8, bt, cu, cl, bs, 0, cos, sin, w, w)   # an fp8 cache without scales
    c16, s16 = (t.to(DEV) for t in ops.rope_tables(32, 16))
    with pytest.raises(ValueError, match="multiple of 32"):
        f(q, k, k, k8, k8, bt, cu, cl, bs, 0, c16, s16, w, w, k_scale=one, v_scale=one)
    f(q, k, k, k8, k8, bt, cu, cl, bs, 0, c16, s16, w, w, k_scale=one, v_scale=one, interleaved=True)
    torch.cuda.synchronize()


# ---- modules --------------------------------------------------------------------------------------------------------
# The bar is the one tests/test_gpu_rope.py applies to the same comparison (the layer's output against the fp64 chain on the
# same 16-bit weights, worst normwise row error in units of the dtype's unit roundoff): tr.MODULE_BARS, read there, not loosened.
def _make_layer(dt, D=64, H=4, Hkv=2):
    from mio.kernels.attention import flash_attention as fa
    torch.manual_seed(17)
    cfg = fa.FlashAttentionConfig(causal=True, precision="bf16" if dt == torch.bfloat16 else "fp16", rotary_dim=D,
                                  max_position=1024, qk_norm=True, qk_norm_eps=EPS)
    layer = fa.FlashSelfAttention(H * D, H, cfg, num_kv_heads=Hkv).to(DEV).to(dt)
    with torch.no_grad():
        for p in layer.parameters():
            if p.dim() == 2:
                p.mul_(4.0)
        g = torch.Generator().manual_seed(23)   # random non-unit norm weights, q's and k's different
        layer.q_norm.weight.copy_((0.5 + torch.rand(D, generator=g)).to(dt))
        layer.k_norm.weight.copy_((1.5 - torch.rand(D, generator=g) * torch.linspace(0.2, 1.0, D)).to(dt))
    return layer.eval()


def _norm64(x, w):
    """fp64 per-head RMSNorm of x [..., D] with the 16-bit weight w (as fp64) and the fp32 eps."""
    e = float(torch.tensor(EPS, dtype=torch.float32))
    return x * (x.pow(2).mean(-1, keepdim=True) + e).rsqrt() * w


def _norm_weights(layer, dt):
    return layer.q_norm.weight.detach().to(dt).double().cpu(), layer.k_norm.weight.detach().to(dt).double().cpu()


def _module_ref_dense(layer, x):
    """fp64 chain: projections, per-head norm, rotation at 0 .. S-1, causal attention, output projection."""
    import _attn_check as ac
    wq, bq, wk, bk, wv, bv, wo, bo = tr._layer_weights(layer, x.dtype)
    nq, nk = _norm_weights(layer, x.dtype)
    B, S, d = x.shape
    H, Hkv, D = layer.num_attention_heads, layer.num_kv_heads, layer.head_dim
    xd = x.double().cpu()
    q = _norm64((xd @ wq.t() + bq).view(B, S, H, D), nq)
    k = _norm64((xd @ wk.t() + bk).view(B, S, Hkv, D), nk)
    v = (xd @ wv.t() + bv).view(B, S, Hkv, D)
    pos = torch.arange(S)
    q, k = tr._rot64(q, pos, D), tr._rot64(k, pos, D)
    o, _ = ac.reference(q, k, v, causal=True)
    return o.reshape(B, S, d) @ wo.t() + bo


@pytest.mark.parametrize("dt", DTYPES)
def test_module_dense_with_qk_norm(dt):
    D = 64
    g = torch.Generator().manual_seed(5)
    B, S = 2, 200
    x = torch.randn(B, S, 4 * D, generator=g).to(dt).to(DEV)
    layer = _make_layer(dt)
    bar = tr.MODULE_BARS[("FlashSelfAttention", dt, "dense")]
    with torch.no_grad():
        y = layer(x)
    err = tr._row_err(y, _module_ref_dense(layer, x), dt)
    print(f"MODULE FlashSelfAttention {str(dt).split('.')[-1]} dense, qk_norm: worst row error {err:.3f} u (bar {bar})")
    assert err <= bar
    # after an in-place update of q_norm.weight the next forward uses the new values
    with torch.no_grad():
        layer.q_norm.weight.mul_(1.5)
        layer.k_norm.weight.add_(0.25)
        y2 = layer(x)
    err2 = tr._row_err(y2, _module_ref_dense(layer, x), dt)
    print(f"  after the in-place weight update: {err2:.3f} u")
    assert not torch.equal(y2, y) and err2 <= bar


@pytest.mark.parametrize("dt", DTYPES)
def test_module_paged_with_qk_norm(dt):
    """The paged path: a prefill chunk written by ops.qknorm_rope_and_cache_varlen from the layer's own K / V projections and
    its k_norm weight, the chunk's last rows attending through the layer, then decode steps (one token per sequence written the
    same way, then the layer).  fp64 chain of each call: q projected, normalised and rotated at context_lengths[b] - q_len + i,
    decode attention over the cache as written, output projection."""
    ops = _ops()
    D, H, Hkv, bs = 64, 4, 2, 16
    ctxs = [37, 120, 64]
    steps = 2
    B = len(ctxs)
    g = torch.Generator().manual_seed(9)
    M = (max(ctxs) + steps) // bs + 2
    bt = torch.randperm(B * M, generator=g).view(B, M).to(torch.int32)
    layer = _make_layer(dt)
    bar = tr.MODULE_BARS[("FlashSelfAttention", dt, "paged")]
    wq, bq, wk, bk, wv, bv, wo, bo = tr._layer_weights(layer, dt)
    nq, _ = _norm_weights(layer, dt)
    kc = torch.full((B * M, 1, bs, Hkv, D), float("nan"), dtype=dt, device=DEV)
    vc = kc.clone()
    cos, sin = (t.to(DEV) for t in ops.rope_tables(1024, D))
    btd = bt.to(DEV)

    def write(hs, after):
        """append the rows hs[b] (hidden states) of every sequence; after[b]: its length afterwards"""
        kn = torch.cat([(h.double() @ wk.t() + bk) for h in hs]).to(dt).view(-1, Hkv, D).to(DEV)
        vn = torch.cat([(h.double() @ wv.t() + bv) for h in hs]).to(dt).view(-1, Hkv, D).to(DEV)
        n = [h.shape[0] for h in hs]
        cu = torch.tensor([0] + [sum(n[:i + 1]) for i in range(B)], dtype=torch.int32, device=DEV)
        cl = torch.tensor(after, dtype=torch.int32, device=DEV)
        with torch.no_grad():
            ops.qknorm_rope_and_cache_varlen(torch.zeros(kn.shape[0], H, D, dtype=dt, device=DEV), kn, vn, kc, vc, btd, cu, cl,
                                             bs, 0, cos, sin, layer.q_norm.weight.detach(), layer.k_norm.weight.detach(), eps=EPS)
        return cl

    def attend(x, lens, q_len, what):
        cl = torch.tensor(lens, dtype=torch.int32, device=DEV)
        with torch.no_grad():
            y = layer(x.to(DEV), physical_kv_cache_k=kc, physical_kv_cache_v=vc, block_tables=btd, context_lengths=cl,
                      kv_cache_block_size=bs, max_seq_len=max(lens), layer_idx=0)
        q = _norm64((x.double() @ wq.t() + bq).view(B, q_len, H, D), nq)
        q = torch.stack([tr._rot64(q[b], torch.arange(lens[b] - q_len, lens[b]), D) for b in range(B)])
        o, _ = dc.reference(q.permute(0, 2, 1, 3), kc.cpu(), vc.cpu(), bt, torch.tensor(lens), bs, 0)
        ref = o.permute(0, 2, 1, 3).reshape(B, q_len, H * D) @ wo.t() + bo
        err = tr._row_err(y, ref, dt)
        print(f"MODULE FlashSelfAttention {str(dt).split('.')[-1]} paged, qk_norm, {what}: worst row error {err:.3f} u (bar {bar})")
        assert err <= bar, what
        return y

    hs = [torch.randn(n, H * D, generator=g).to(dt) for n in ctxs]
    write(hs, ctxs)
    attend(torch.stack([h[-2:] for h in hs]), ctxs, 2, "prefill chunk")
    lens = list(ctxs)
    for t in range(steps):
        new = [torch.randn(1, H * D, generator=g).to(dt) for _ in range(B)]
        lens = [n + 1 for n in lens]
        write(new, lens)
        y = attend(torch.stack(new), lens, 1, f"decode step {t}")
    # after an in-place update of q_norm.weight the next forward uses the new values (k is in the cache as written)
    with torch.no_grad():
        layer.q_norm.weight.mul_(1.5)
    nq, _ = _norm_weights(layer, dt)
    y2 = attend(torch.stack(new), lens, 1, "after the in-place weight update")
    assert not torch.equal(y2, y)

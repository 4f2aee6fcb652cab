"""Rotary position embedding on the GPU: the rotation fused into the paged KV-cache write (ops.rope_and_cache_varlen, 16-bit
and fp8 caches), the standalone form (ops.apply_rotary) and the attention modules with rotary_dim > 0.

The rotated values are judged by the derived interval of tests/_rope_check.py (no measured tolerance); everything the fused
write does not rotate is compared byte for byte with what ops.reshape_and_cache_varlen writes from the same inputs; every
other cache byte must keep its sentinel.  One scenario (_Scene) carries the hard cases together: ragged sequences, a shared
prefix, a sequence that overruns its block-table row, packed tokens outside every sequence, rotation positions past
max_position and below 0, strided views into a fused QKV buffer, q_out aliasing q.
"""
import math

import pytest
import torch

import _attn_check as ac
import _decode_check as dc
import _rope_check as rc

pytestmark = pytest.mark.gpu

DEV = "cuda"
F8 = torch.float8_e4m3fn
DTYPES = [torch.bfloat16, torch.float16]
SENT = 0x5A
# (D, rot_dim): rot_dim is D, D / 2 for D 64 and 128, and 32 for D 96
GEOMS = [(64, 64), (64, 32), (96, 96), (96, 32), (128, 128), (128, 64)]


def _ops():
    from mio import ops
    return ops


def _bytes(t):
    return t.detach().cpu().contiguous().view(torch.uint8)


class _Scene:
    """Four sequences and two stray packed tokens.  Sequence 0 appends 37 tokens at 2 bs + 5; sequence 1 shares its first two
    pages with sequence 0 and appends 50 tokens at 2 bs; sequence 2 appends 20 tokens of which the last 7 lie past its
    block-table row (max_blocks * bs), the last 4 of those also past max_position = max_blocks * bs + 3; sequence 3 appends
    one token (a decode step) at position 10.  total_new is 2 more than cu_seqlens_new[-1]: the last two packed tokens belong
    to no sequence.  With use_positions the rotation positions are the cache positions + 3, except two tokens of sequence 0
    (max_position + 5, -1: rows the plain write fills but the rotating write must leave alone) and one of sequence 2's
    overrunning tokens, which gets a valid position (its q row is rotated although its cache row is skipped)."""

    def __init__(self, dtype, kv8, D, rot, *, H, Hkv, bs, use_positions, seed, L=2, layer=1):
        g = torch.Generator().manual_seed(seed)
        self.dtype, self.kv8, self.D, self.rot, self.H, self.Hkv, self.bs, self.L, self.layer = dtype, kv8, D, rot, H, Hkv, bs, L, layer
        M = 4 if bs == 64 else 12
        self.M = M
        new = [37, 50, 20, 1]
        start = [2 * bs + 5, 2 * bs, M * bs - 13, 10]
        self.new, self.start = new, start
        self.after = [a + n for a, n in zip(start, new)]
        self.T = sum(new) + 2
        self.maxpos = M * bs + 3
        nb = 4 * M + 2
        perm = torch.randperm(nb, generator=g)[:4 * M].view(4, M).to(torch.int32)
        perm[1, :2] = perm[0, :2]  # the shared prefix
        self.bt = perm
        self.cu = torch.tensor([0, 37, 87, 107, 108], dtype=torch.int32)
        self.cl = torch.tensor(self.after, dtype=torch.int32)
        # packed token -> (sequence, cache position); -1: outside every sequence
        self.seq = torch.full((self.T,), -1, dtype=torch.long)
        self.cpos = torch.zeros(self.T, dtype=torch.long)
        t = 0
        for b, n in enumerate(new):
            self.seq[t:t + n] = b
            self.cpos[t:t + n] = torch.arange(start[b], start[b] + n)
            t += n
        if use_positions:
            rp = self.cpos + 3
            rp[5] = self.maxpos + 5
            rp[11] = -1
            rp[87 + 15] = 40          # sequence 2, cache position M bs + 2: no cache row, a valid rotation position
            rp[self.T - 1] = 5        # a stray token: still outside every sequence
            self.positions = rp.to(torch.int32)
        else:
            rp = self.cpos.clone()
            self.positions = None
        self.rpos = rp
        self.live = (self.seq >= 0) & (rp >= 0) & (rp < self.maxpos)            # rotated (q_out row written)
        self.has_row = (self.seq >= 0) & (self.cpos < M * bs)                    # the plain write fills the row
        blk = torch.where(self.has_row, self.bt[self.seq.clamp_min(0), (self.cpos // bs).clamp_max(M - 1)].long(),
                          torch.zeros_like(self.seq))
        self.blk, self.slot = blk, self.cpos % bs
        # one fused projection result [T, (H + 2 Hkv) D]: q / k / v are strided views of it
        w = (H + 2 * Hkv) * D
        self.qkv = (torch.randn(self.T, w, generator=g) * 1.5).to(dtype)
        self.cos, self.sin = _ops().rope_tables(self.maxpos, rot, 10000.0)
        self.k_scale = [0.9, 0.011] if kv8 else None   # |k| reaches about 6: 6 / 0.011 = 545 > 448, the clamp is exercised
        self.v_scale = [1.3, 0.02] if kv8 else None
        self.nb = nb

    def views(self, buf):
        H, Hkv, D = self.H, self.Hkv, self.D
        q = buf[:, :H * D].view(self.T, H, D)
        k = buf[:, H * D:(H + Hkv) * D].view(self.T, Hkv, D)
        v = buf[:, (H + Hkv) * D:].view(self.T, Hkv, D)
        return q, k, v

    def caches(self):
        shape = (self.nb, self.L, self.bs, self.Hkv, self.D)
        if self.kv8:
            c = torch.full(shape, SENT, dtype=torch.uint8, device=DEV).view(F8)
        else:
            c = torch.full(shape, SENT, dtype=torch.uint8, device=DEV).repeat_interleave(2, -1).view(self.dtype)
        return c, c.clone()

    def scales(self):
        if not self.kv8:
            return {}
        return dict(k_scale=torch.tensor(self.k_scale, dtype=torch.float32, device=DEV),
                    v_scale=torch.tensor(self.v_scale, dtype=torch.float32, device=DEV))

    def dev(self, t):
        return None if t is None else t.to(DEV)


def _run_scene(sc, interleaved, alias):
    """The fused write of a scene and every assertion on it (rotated values, untouched bytes, zero rows); returns
    (q_out, kc, vc) on the CPU."""
    ops = _ops()
    buf = sc.qkv.to(DEV)
    q, k, v = sc.views(buf)
    q_cpu, k_cpu, v_cpu = sc.views(sc.qkv)
    kc, vc = sc.caches()
    kc2, vc2 = sc.caches()
    bt, cu, cl = sc.dev(sc.bt), sc.dev(sc.cu), sc.dev(sc.cl)
    cos, sin = sc.dev(sc.cos), sc.dev(sc.sin)
    # the plain write first (before q may be rotated in place; k and v are never modified)
    ops.reshape_and_cache_varlen(k, v, kc2, vc2, bt, cu, cl, sc.bs, sc.layer, **sc.scales())
    if alias:
        q_out = q
    else:
        q_out = torch.full((sc.T, sc.H, sc.D), float("nan"), dtype=sc.dtype, device=DEV)
    got = ops.rope_and_cache_varlen(q, k, v, kc, vc, bt, cu, cl, sc.bs, sc.layer, cos, sin, positions=sc.dev(sc.positions),
                                    interleaved=interleaved, q_out=q_out, **sc.scales())
    torch.cuda.synchronize()
    assert got.data_ptr() == q_out.data_ptr()
    qo = q_out.cpu()
    rot, D = sc.rot, sc.D
    live = sc.live
    # ---- q_out: no NaN; rows of tokens that are not rotated exactly zero; the others rotated within the interval, the rest copied
    assert not torch.isnan(qo.float()).any()
    assert (qo[~live] == 0).all() and (_bytes(qo[~live]) == 0).all()
    ref, delta = rc.reference(q_cpu[live], sc.cos, sc.sin, sc.rpos[live], interleaved)
    out, differ = rc.outside16(qo[live][..., :rot], ref, delta, sc.dtype)
    print(f"q_out: {ref.numel()} rotated elements, {out} outside the interval, {differ} differ from RN(ref)")
    assert out == 0
    assert torch.equal(_bytes(qo[live][..., rot:]), _bytes(q_cpu[live][..., rot:]))
    # ---- caches
    kcb, vcb, kc2b, vc2b = kc.cpu(), vc.cpu(), kc2.cpu(), vc2.cpu()
    wr = live & sc.has_row                       # tokens whose row the rotating write fills
    blk, slot = sc.blk[wr], sc.slot[wr]
    # V, and K past rot_dim: byte-identical to the plain write on the written rows; every other byte keeps the sentinel
    exp_v = sc.caches()[1].cpu()
    exp_v[blk, sc.layer, slot] = vc2b[blk, sc.layer, slot]
    assert torch.equal(_bytes(vcb), _bytes(exp_v))
    exp_k = sc.caches()[0].cpu()
    exp_k[blk, sc.layer, slot] = kc2b[blk, sc.layer, slot]
    krows = kcb[blk, sc.layer, slot]             # [n, Hkv, D]
    exp_k[blk, sc.layer, slot, :, :rot] = krows[..., :rot]   # the rotated part is judged below, not here
    assert torch.equal(_bytes(kcb), _bytes(exp_k))
    # every row the plain write leaves at the sentinel (and the whole other layer) is still the sentinel
    rows_plain = torch.zeros(sc.nb, sc.bs, dtype=torch.bool)
    rows_plain[sc.blk[sc.has_row], sc.slot[sc.has_row]] = True
    kview = _bytes(kcb).view(sc.nb, sc.L, sc.bs, -1)
    assert (kview[:, sc.layer][~rows_plain] == SENT).all() and (kview[:, 1 - sc.layer] == SENT).all()
    # rotated K
    ref, delta = rc.reference(k_cpu[wr], sc.cos, sc.sin, sc.rpos[wr], interleaved)
    if sc.kv8:
        out = rc.outside8(krows[..., :rot], ref, delta, sc.k_scale[sc.layer])
        sat = int((krows[..., :rot].float().abs() == 448).sum())
        print(f"fp8 K: {ref.numel()} rotated elements, {out} outside the interval, {sat} saturated")
    else:
        out, differ = rc.outside16(krows[..., :rot], ref, delta, sc.dtype)
        print(f"K: {ref.numel()} rotated elements, {out} outside the interval, {differ} differ from RN(ref)")
    assert out == 0
    assert int(wr.sum()) > 80 and int((sc.has_row & ~live).sum()) == (2 if sc.positions is not None else 0)
    return qo, kcb, vcb


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("D,rot", GEOMS)
@pytest.mark.parametrize("kv8", [False, True])
def test_rope_and_cache_varlen(dtype, interleaved, D, rot, kv8):
    i = GEOMS.index((D, rot))
    gqa = (i + interleaved) % 2 == 0
    sc = _Scene(dtype, kv8, D, rot, H=8 if gqa else 4, Hkv=2 if gqa else 4, bs=(16, 64)[(i + kv8) % 2],
                use_positions=(i + interleaved + kv8) % 2 == 1, seed=100 * i + 10 * interleaved + kv8)
    _run_scene(sc, interleaved, alias=(i + (dtype == torch.float16)) % 2 == 0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("use_positions", [False, True])
@pytest.mark.parametrize("bs", [16, 64])
@pytest.mark.parametrize("gqa", [False, True])
def test_rope_and_cache_varlen_forms(dtype, use_positions, bs, gqa):
    """positions given / not given x block size x GQA / MHA at one geometry, both cache kinds, q_out aliasing q or not."""
    for kv8 in (False, True):
        sc = _Scene(dtype, kv8, 128, 64, H=8 if gqa else 2, Hkv=2, bs=bs, use_positions=use_positions, seed=7 + bs + gqa)
        _run_scene(sc, interleaved=bool(bs == 16), alias=use_positions)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("D,rot", GEOMS)
def test_standalone_form_agrees_bit_for_bit(dtype, interleaved, D, rot):
    """apply_rotary on q and k followed by the plain write gives the fused write's q_out and 16-bit cache bit for bit.  The
    one difference is by construction: a token whose rotation position is outside the table gets no cache row from the fused
    write (the row keeps its sentinel) and a zero K row from the two-step chain."""
    ops = _ops()
    for use_positions in (False, True):
        sc = _Scene(dtype, False, D, rot, H=4, Hkv=2, bs=16, use_positions=use_positions, seed=3 + D + rot)
        qo, kcb, vcb = _run_scene(sc, interleaved, alias=False)
        buf = sc.qkv.to(DEV)
        q, k, v = sc.views(buf)
        cos, sin = sc.dev(sc.cos), sc.dev(sc.sin)
        rp = torch.where(sc.seq >= 0, sc.rpos, torch.full_like(sc.rpos, -1)).to(torch.int32).to(DEV)
        q2 = ops.apply_rotary(q, cos, sin, rp, interleaved=interleaved)
        k2 = ops.apply_rotary(k, cos, sin, rp, interleaved=interleaved)
        assert q2.data_ptr() != q.data_ptr() and torch.equal(buf.cpu(), sc.qkv)  # out of place: the inputs are intact
        kc3, vc3 = sc.caches()
        ops.reshape_and_cache_varlen(k2, v, kc3, vc3, sc.dev(sc.bt), sc.dev(sc.cu), sc.dev(sc.cl), sc.bs, sc.layer)
        torch.cuda.synchronize()
        assert torch.equal(_bytes(q2), _bytes(qo))
        k3, v3 = kc3.cpu(), vc3.cpu()
        dead = sc.has_row & ~sc.live
        same = torch.ones(sc.nb, sc.bs, dtype=torch.bool)
        same[sc.blk[dead], sc.slot[dead]] = False
        assert torch.equal(_bytes(k3[:, sc.layer][same]), _bytes(kcb[:, sc.layer][same]))
        assert torch.equal(_bytes(v3[:, sc.layer][same]), _bytes(vcb[:, sc.layer][same]))
        assert (_bytes(kcb[:, sc.layer][~same]) == SENT).all() and (k3[:, sc.layer][~same][..., :rot] == 0).all()
        # in place, and the [B, S, heads, D] form with [S] and [B, S] positions
        q_in = q.clone()
        assert ops.apply_rotary(q_in, cos, sin, rp, interleaved=interleaved, out=q_in).data_ptr() == q_in.data_ptr()
        assert torch.equal(_bytes(q_in), _bytes(qo))
    g = torch.Generator().manual_seed(D)
    B, S, Hn = 3, 50, 4
    cos, sin = (t.to(DEV) for t in ops.rope_tables(64, rot))
    wide = torch.randn(B, S, 2 * Hn * D, generator=g).to(dtype).to(DEV)
    x = wide[:, :, Hn * D:].view(B, S, Hn, D)  # a strided view whose batch and sequence axes collapse
    pos1 = torch.arange(S, dtype=torch.int32, device=DEV)
    y1 = ops.apply_rotary(x, cos, sin, pos1, interleaved=interleaved)
    y2 = ops.apply_rotary(x, cos, sin, pos1.expand(B, S).contiguous(), interleaved=interleaved)
    y3 = ops.apply_rotary(x.reshape(B * S, Hn, D), cos, sin, pos1.repeat(B), interleaved=interleaved)
    assert y1.shape == x.shape and torch.equal(y1, y2) and torch.equal(y1.view(B * S, Hn, D), y3)
    ref, delta = rc.reference(x.reshape(B * S, Hn, D).cpu(), cos.cpu(), sin.cpu(), pos1.repeat(B).cpu().long(), interleaved)
    assert rc.outside16(y3.cpu()[..., :rot], ref, delta, dtype)[0] == 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("interleaved", [False, True])
def test_fp8_key_is_rounded_once(dtype, interleaved):
    """One fixed seed: the fused fp8 K (one rounding from fp32) against the two-step K (apply_rotary to 16 bits, then the
    quantising write), both against fp64 in the scaled domain: the fused one's summed error is no larger."""
    ops = _ops()
    sc = _Scene(dtype, True, 128, 128, H=4, Hkv=4, bs=16, use_positions=False, seed=2024)
    sc.k_scale = [0.9, 0.05]   # nothing saturates: the clamp would hide rounding differences
    _, kcb, _ = _run_scene(sc, interleaved, alias=False)
    buf = sc.qkv.to(DEV)
    q, k, v = sc.views(buf)
    rp = torch.where(sc.seq >= 0, sc.rpos, torch.full_like(sc.rpos, -1)).to(torch.int32).to(DEV)
    k2 = ops.apply_rotary(k, sc.dev(sc.cos), sc.dev(sc.sin), rp, interleaved=interleaved)
    kc3, vc3 = sc.caches()
    ops.reshape_and_cache_varlen(k2, v, kc3, vc3, sc.dev(sc.bt), sc.dev(sc.cu), sc.dev(sc.cl), sc.bs, sc.layer, **sc.scales())
    torch.cuda.synchronize()
    wr = sc.live & sc.has_row
    _, k_cpu, _ = sc.views(sc.qkv)
    ref, _ = rc.reference(k_cpu[wr], sc.cos, sc.sin, sc.rpos[wr], interleaved)
    inv = (torch.tensor(1.0) / torch.tensor(sc.k_scale[sc.layer])).double()
    fused = kcb[sc.blk[wr], sc.layer, sc.slot[wr]].float().double()
    two = kc3.cpu()[sc.blk[wr], sc.layer, sc.slot[wr]].float().double()
    e1, e2 = (fused - ref * inv).abs().sum().item(), (two - ref * inv).abs().sum().item()
    print(f"summed |error| in the scaled domain over {ref.numel()} elements: fused {e1:.6f}, two-step {e2:.6f}, "
          f"{int((fused != two).sum())} bytes differ")
    assert e1 <= e2


def _ref_attention(q, k, v, left, off):
    """fp64 causal (bottom-right, offset off) attention with a left window: q [Sq,H,D], k / v [Sk,Hkv,D] fp64 ->
    (o [1,Sq,H,D], lse [1,H,Sq])."""
    Sq, H, D = q.shape
    Sk, Hkv = k.shape[0], k.shape[1]
    qd = q.double().permute(1, 0, 2)
    kd = k.repeat_interleave(H // Hkv, dim=1).permute(1, 0, 2)
    vd = v.repeat_interleave(H // Hkv, dim=1).permute(1, 0, 2)
    s = qd @ kd.transpose(-1, -2) / math.sqrt(D)
    i = torch.arange(Sq).view(Sq, 1) + off
    j = torch.arange(Sk).view(1, Sk)
    vis = j <= i
    if left >= 0:
        vis = vis & (j >= i - left)
    s = s.masked_fill(~vis, float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse.unsqueeze(-1))
    return (p @ vd).permute(1, 0, 2)[None], lse[None]


@pytest.mark.parametrize("dtype,kv8,D,left", [(torch.bfloat16, False, 128, -1), (torch.float16, False, 64, -1),
                                               (torch.bfloat16, True, 128, -1), (torch.float16, True, 64, 100),
                                               (torch.bfloat16, False, 64, 100)])
def test_chunked_prefill_then_decode_with_rotary(dtype, kv8, D, left):
    """A chunked prefill of ragged prompts (chunks of 128: rope_and_cache_varlen, then flash_attention_varlen_paged) and
    decode steps (rope_and_cache_varlen with one token per sequence, then paged_attention_forward).  Each result is judged
    against the fp64 attention of the cache contents as written and the rotated q as returned, at the unchanged bars of the
    attention kernels' families; that the cache holds the rotation of the right position is checked on the way."""
    ops = _ops()
    g = torch.Generator().manual_seed(D + kv8)
    H, Hkv, L, layer, bs, chunk, rot = 4, 2, 2, 1, 64, 128, D // 2 if kv8 else D
    prompts = [150, 333, 40]
    steps = 3
    B = len(prompts)
    M = (max(prompts) + steps + bs - 1) // bs + 1
    nb = B * M + 1
    bt = torch.randperm(nb, generator=g)[:B * M].view(B, M).to(torch.int32)
    cos, sin = ops.rope_tables(M * bs, rot)
    ks, vs = (torch.tensor(0.031).item(), torch.tensor(0.027).item()) if kv8 else (1.0, 1.0)  # the fp32 values
    if kv8:
        kc = torch.full((nb, L, bs, Hkv, D), 0x7F, dtype=torch.uint8, device=DEV).view(F8)
        scales = dict(k_scale=torch.tensor([9.0, ks], device=DEV), v_scale=torch.tensor([7.0, vs], device=DEV))
    else:
        kc = torch.full((nb, L, bs, Hkv, D), float("nan"), dtype=dtype, device=DEV)
        scales = {}
    vc = kc.clone()
    K = [torch.randn(n + steps, Hkv, D, generator=g).to(dtype) for n in prompts]
    V = [torch.randn(n + steps, Hkv, D, generator=g).to(dtype) for n in prompts]
    Q = [torch.randn(n + steps, H, D, generator=g).to(dtype) for n in prompts]
    win = {} if left < 0 else {"window_size": (left, -1)}
    btd, cosd, sind = bt.to(DEV), cos.to(DEV), sin.to(DEV)

    def cached(b, n):
        pos = torch.arange(n)
        blk, slot = bt[b, pos // bs].long(), pos % bs
        kk, vv = kc.cpu()[blk, layer, slot], vc.cpu()[blk, layer, slot]
        return kk.float().double() * ks, vv.float().double() * vs

    def append(step, done):
        cu = torch.tensor([0] + [sum(step[:i + 1]) for i in range(B)], dtype=torch.int32, device=DEV)
        cl = torch.tensor([d + n for d, n in zip(done, step)], dtype=torch.int32, device=DEV)
        cat = lambda X: torch.cat([X[s][done[s]:done[s] + step[s]] for s in range(B)]).to(DEV)  # noqa: E731
        q_rot = ops.rope_and_cache_varlen(cat(Q), cat(K), cat(V), kc, vc, btd, cu, cl, bs, layer, cosd, sind, **scales)
        return q_rot, cu, cl

    done = [0] * B
    while any(d < n for d, n in zip(done, prompts)):
        step = [min(chunk, n - d) for d, n in zip(done, prompts)]
        q_rot, cu, cl = append(step, done)
        mx = max(d + n for d, n in zip(done, step))
        route = ops.fa3_paged_route(q_rot, kc, vc, btd, cu, cl, max(step), mx, layer_idx=layer, causal=True, **win, **scales)
        o, lse = ops.flash_attention_varlen_paged(q_rot, kc, vc, btd, cu, cl, max(step), mx, layer_idx=layer, causal=True,
                                                  return_lse=True, **win, **scales)
        torch.cuda.synchronize()
        for s in range(B):
            if step[s] == 0:
                continue
            a, e = sum(step[:s]), done[s] + step[s]
            kk, vv = cached(s, e)
            ref, ref_lse = _ref_attention(q_rot[a:a + step[s]].cpu(), kk, vv, left, e - step[s])
            ac.check(o[a:a + step[s]][None].cpu(), ref, dtype, route, lse=lse[:, a:a + step[s]][None].cpu(),
                     ref_lse=ref_lse, what=f"prefill seq {s} rows {done[s]}..{e}")
        done = [d + n for d, n in zip(done, step)]
    for t in range(steps):
        q_rot, cu, cl = append([1] * B, done)
        done = [d + 1 for d in done]
        q4 = q_rot.view(B, 1, H, D).permute(0, 2, 1, 3)
        o = torch.empty(B, 1, H, D, dtype=dtype, device=DEV).permute(0, 2, 1, 3)
        mx = max(done)
        route = ops.paged_attention_route(q4, o, kc, vc, btd, cl, bs, mx, layer, **win, **scales)
        ops.paged_attention_forward(q4, o, kc, vc, btd, cl, bs, mx, layer, **win, **scales)
        torch.cuda.synchronize()
        kw = dict(left=left, k_scale=ks, v_scale=vs)
        ctx = torch.tensor(done, dtype=torch.int32)
        ref, ref_lse = dc.reference(q4.cpu(), kc.cpu(), vc.cpu(), bt, ctx, bs, layer, **kw)
        mo = dc.model(q4.cpu(), kc.cpu(), vc.cpu(), bt, ctx, bs, layer, dtype=dtype, p16=route == "gqa", **kw)
        dc.check(o, ref, ref_lse, dtype, (dtype, route, "fp8" if kv8 else "kv16"), mo, what=f"decode step {t}",
                 win=left >= 0)
    # the cache holds rot(K) of each token's own position (the attention checks above take the cache as it is)
    for s in range(B):
        n = prompts[s] + steps
        kk, _ = cached(s, n)
        ref, delta = rc.reference(K[s], cos, sin, torch.arange(n), False)
        if kv8:
            got8 = kc.cpu()[bt[s, torch.arange(n) // bs].long(), layer, torch.arange(n) % bs]
            assert rc.outside8(got8[..., :rot], ref, delta, ks) == 0
            assert torch.equal(got8[..., rot:].view(torch.uint8), dc.quantise(K[s][..., rot:], ks).view(torch.uint8))
        else:
            assert rc.outside16(kk[..., :rot].to(dtype), ref, delta, dtype)[0] == 0


@pytest.mark.parametrize("kv8", [False, True])
def test_rope_and_cache_varlen_graph_capture(kv8):
    """A torch.cuda.graph capture and replay of rope_and_cache_varlen (inputs refilled in place) reproduces the eager result."""
    ops = _ops()
    dtype = torch.bfloat16
    sc = _Scene(dtype, kv8, 128, 64, H=8, Hkv=2, bs=16, use_positions=True, seed=99)
    buf = torch.empty_like(sc.qkv, device=DEV)
    q, k, v = sc.views(buf)
    kc, vc = sc.caches()
    q_out = torch.empty(sc.T, sc.H, sc.D, dtype=dtype, device=DEV)
    bt, cu, cl, pos = sc.dev(sc.bt), sc.dev(sc.cu), sc.dev(sc.cl), sc.dev(sc.positions)
    cos, sin = sc.dev(sc.cos), sc.dev(sc.sin)
    scales = sc.scales()

    def step():
        ops.rope_and_cache_varlen(q, k, v, kc, vc, bt, cu, cl, sc.bs, sc.layer, cos, sin, positions=pos, q_out=q_out, **scales)

    def fill(seed):
        buf.copy_((torch.randn(buf.shape, generator=torch.Generator().manual_seed(seed)) * 1.5).to(dtype))

    fill(1)
    kc0, vc0 = kc.clone(), vc.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    fill(2)
    kc.copy_(kc0)
    vc.copy_(vc0)
    q_out.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    got = (q_out.clone(), kc.clone(), vc.clone())
    kc.copy_(kc0)
    vc.copy_(vc0)
    q_out.fill_(float("nan"))
    step()
    torch.cuda.synchronize()
    for a, b in zip(got, (q_out, kc, vc)):
        assert torch.equal(_bytes(a), _bytes(b))
    assert not torch.equal(_bytes(kc), _bytes(kc0))


def test_rope_ops_argument_errors():
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
    one = torch.ones(1, device=DEV)
    f = ops.rope_and_cache_varlen
    assert f(q, k, k, kc, kc, bt, cu, cl, bs, 0, cos, sin).shape == q.shape
    bad = [
        dict(q=q[:, :, :32]), dict(q=q[:5]), dict(q=q.half()), dict(q=torch.zeros(T, 3, D, dtype=bf, device=DEV)),
        dict(key=k[:, :1]), dict(k_cache=kc[:, :, :8]), dict(layer_idx=1), dict(block_size=32),
        dict(cu=cu.long()), dict(cl=torch.cat([cl, cl])), dict(bt=bt.long()),
        dict(cos=cos.cpu()), dict(cos=cos.double()), dict(cos=cos[:, :12].contiguous(), sin=sin[:, :12].contiguous()),
        dict(cos=ops.rope_tables(32, 128)[0].to(DEV), sin=ops.rope_tables(32, 128)[1].to(DEV)),
        dict(positions=torch.zeros(T, dtype=torch.int64, device=DEV)), dict(positions=torch.zeros(T - 1, dtype=torch.int32, device=DEV)),
        dict(q_out=torch.zeros(T, H, D, dtype=torch.float16, device=DEV)), dict(q_out=torch.zeros(T, H, D + 8, dtype=bf, device=DEV)[..., 4:D + 4]),
        dict(k_scale=one, v_scale=one),                       # scales with a 16-bit cache
        dict(k_cache=k8, v_cache=k8),                         # an fp8 cache without scales
    ]
    for kw in bad:
        a = dict(q=q, key=k, value=k, k_cache=kc, v_cache=kc, bt=bt, cu=cu, cl=cl, block_size=bs, layer_idx=0, cos=cos, sin=sin,
                 positions=None, q_out=None, k_scale=None, v_scale=None)
        a.update(kw)
        if "key" in kw:
            a["value"] = kw["key"]
        if "k_cache" in kw and "v_cache" not in kw:
            a["v_cache"] = kw["k_cache"]
        with pytest.raises(ValueError):
            f(a["q"], a["key"], a["value"], a["k_cache"], a["v_cache"], a["bt"], a["cu"], a["cl"], a["block_size"],
              a["layer_idx"], a["cos"], a["sin"], positions=a["positions"], q_out=a["q_out"], k_scale=a["k_scale"],
              v_scale=a["v_scale"])
    # fp8 cache, neox pairing, rot_dim 16
    c16, s16 = (t.to(DEV) for t in ops.rope_tables(32, 16))
    with pytest.raises(ValueError, match="multiple of 32"):
        f(q, k, k, k8, k8, bt, cu, cl, bs, 0, c16, s16, k_scale=one, v_scale=one)
    f(q, k, k, k8, k8, bt, cu, cl, bs, 0, c16, s16, k_scale=one, v_scale=one, interleaved=True)
    pos = torch.zeros(T, dtype=torch.int32, device=DEV)
    g = ops.apply_rotary
    assert g(q, cos, sin, pos).shape == q.shape
    for args, kw in [((q, cos, sin, pos.long()), {}), ((q, cos, sin, pos[:3]), {}), ((q.float(), cos, sin, pos), {}),
                     ((q, cos, sin[:8], pos), {}), ((q, cos, sin, pos), dict(out=q.half())),
                     ((q, cos, sin, pos), dict(out=torch.zeros(T, H, D + 8, dtype=bf, device=DEV)[..., 4:D + 4])),
                     ((q.view(2, 3, H, D), cos, sin, pos), {}), ((q[..., :60], cos, sin, pos), {})]:
        with pytest.raises(ValueError):
            g(*args, **kw)
    torch.cuda.synchronize()


# ---- modules --------------------------------------------------------------------------------------------------------
# The worst normwise row error ||y - ref|| / ||ref|| of a layer's output against the fp64 chain on the same 16-bit weights,
# in units of the dtype's unit roundoff (bf16 2^-8, fp16 2^-11).  No derived bar exists for a chain of four GEMMs and an
# attention; the bar is 2x the value one run measured on the MI355X (MODULE_BARS: measured values in the comments, with
# the same layer without rotary next to them).
MODULE_BARS = {
    # (class, dtype, path): bar                             measured with rotary / without  (the two classes draw the same
    # weights from the same seed and run the same kernels here, hence the equal figures)
    ("FlashAttentionLayer", torch.bfloat16, "dense"): 4.9,   # 2.473 / 1.698
    ("FlashAttentionLayer", torch.float16, "dense"): 5.3,    # 2.684 / 1.869
    ("FlashSelfAttention", torch.bfloat16, "dense"): 4.9,    # 2.473 / 1.698
    ("FlashSelfAttention", torch.float16, "dense"): 5.3,     # 2.684 / 1.869
    ("FlashAttentionLayer", torch.bfloat16, "paged"): 2.4,   # 1.225 / 1.006
    ("FlashAttentionLayer", torch.float16, "paged"): 3.4,    # 1.703 / 0.999
    ("FlashSelfAttention", torch.bfloat16, "paged"): 2.4,    # 1.225 / 1.006
    ("FlashSelfAttention", torch.float16, "paged"): 3.4,     # 1.703 / 0.999
}


def _rot64(x, pos, rot, base=10000.0):
    """fp64 neox rotation of x [..., S, heads, D] at pos [S] with the fp32 table entries the layer reads."""
    from mio import ops
    cos, sin = ops.rope_tables(int(pos.max()) + 1, rot, base)
    c, s = cos[pos].double()[:, None, :], sin[pos].double()[:, None, :]
    x1, x2 = x[..., :rot // 2], x[..., rot // 2:rot]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s, x[..., rot:]], -1)


def _layer_weights(layer, dt):
    """(wq, bq, wk, bk, wv, bv, wo, bo) fp64 of the layer's weights rounded to dt (what the kernels see)."""
    r = lambda t: t.detach().to(dt).double().cpu()  # noqa: E731
    if hasattr(layer, "qkv_proj"):
        w, b = r(layer.qkv_proj.weight), r(layer.qkv_proj.bias)
        qd, kvd = layer.hidden_size, layer.num_kv_heads * layer.head_dim
        parts = (w[:qd], b[:qd], w[qd:qd + kvd], b[qd:qd + kvd], w[qd + kvd:], b[qd + kvd:])
    else:
        parts = (r(layer.q_proj.weight), r(layer.q_proj.bias), r(layer.k_proj.weight), r(layer.k_proj.bias),
                 r(layer.v_proj.weight), r(layer.v_proj.bias))
    return parts + (r(layer.o_proj.weight), r(layer.o_proj.bias))


def _module_ref_dense(layer, x, rot):
    """fp64 chain: projections, rotation at 0 .. S-1 (rot 0: none), causal attention, output projection."""
    wq, bq, wk, bk, wv, bv, wo, bo = _layer_weights(layer, x.dtype)
    B, S, d = x.shape
    H, Hkv, D = layer.num_attention_heads, layer.num_kv_heads, layer.head_dim
    xd = x.double().cpu()
    q = (xd @ wq.t() + bq).view(B, S, H, D)
    k = (xd @ wk.t() + bk).view(B, S, Hkv, D)
    v = (xd @ wv.t() + bv).view(B, S, Hkv, D)
    if rot:
        pos = torch.arange(S)
        q, k = _rot64(q, pos, rot), _rot64(k, pos, rot)
    o, _ = ac.reference(q, k, v, causal=True)
    return o.reshape(B, S, d) @ wo.t() + bo


def _row_err(y, ref, dt):
    e = (y.double().cpu() - ref).norm(dim=-1) / ref.norm(dim=-1)
    return (e / ac.U[dt]).max().item()


def _make_layer(cls_name, dt, rot, D=64, H=4, Hkv=2):
    from mio.kernels.attention import flash_attention as fa
    torch.manual_seed(17)
    cfg = fa.FlashAttentionConfig(causal=True, precision="bf16" if dt == torch.bfloat16 else "fp16", rotary_dim=rot,
                                  max_position=1024)
    layer = getattr(fa, cls_name)(H * D, H, cfg, num_kv_heads=Hkv).to(DEV).to(dt)
    with torch.no_grad():  # weights large enough that the scores vary: positions matter
        for p in layer.parameters():
            if p.dim() == 2:
                p.mul_(4.0)
    return layer.eval()


def _assert_bar(key, with_rot, without):
    print(f"MODULE {key[0]} {str(key[1]).split('.')[-1]} {key[2]}: worst row error {with_rot:.3f} u with rotary, "
          f"{without:.3f} u without")
    bar = MODULE_BARS[key]
    assert bar is not None, f"no bar recorded for {key}: measured {with_rot:.3f} u (without rotary {without:.3f} u)"
    assert with_rot <= bar, f"{key}: {with_rot:.3f} u above the bar {bar}"


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("cls_name", ["FlashAttentionLayer", "FlashSelfAttention"])
def test_modules_dense_with_rotary(cls_name, dt):
    D = 64
    g = torch.Generator().manual_seed(5)
    B, S = 2, 200
    x = torch.randn(B, S, 4 * D, generator=g).to(dt).to(DEV)
    errs = {}
    for rot in (D, 0):
        layer = _make_layer(cls_name, dt, rot)
        with torch.no_grad():
            y = layer(x)
        errs[rot] = _row_err(y, _module_ref_dense(layer, x, rot), dt)
        if rot:
            # explicit position_ids equal to the default give the same bits; shifted ones do not
            ids = torch.arange(S, device=DEV)
            with torch.no_grad():
                assert torch.equal(layer(x, position_ids=ids), y)
                assert torch.equal(layer(x, position_ids=ids.expand(B, S)), y)
            # rotary leaves no state behind: the tables are rebuilt when max_position changes
            key0 = layer._rope_key
            layer.config.max_position = 2048
            with torch.no_grad():
                assert torch.equal(layer(x), y)
            assert layer._rope_key != key0 and layer._rope_tabs[0].shape[0] == 2048
    _assert_bar((cls_name, dt, "dense"), errs[D], errs[0])


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("cls_name", ["FlashAttentionLayer", "FlashSelfAttention"])
def test_modules_paged_with_rotary(cls_name, dt):
    """The paged path: the cache is filled by rope_and_cache_varlen from the layer's own K / V projections, then q_len = 2
    rows per sequence attend through the layer; fp64 chain: q projected and rotated at context_lengths[b] - q_len + i, decode
    attention over the cache as written (no causal mask among the rows, as the decode kernel defines it), output projection."""
    ops = _ops()
    D, H, Hkv, bs, q_len = 64, 4, 2, 16, 2
    ctxs = [37, 120, 64]
    B = len(ctxs)
    g = torch.Generator().manual_seed(9)
    M = max(ctxs) // bs + 2
    bt = torch.randperm(B * M, generator=g).view(B, M).to(torch.int32)
    errs = {}
    for rot in (D, 0):
        layer = _make_layer(cls_name, dt, rot)
        wq, bq, wk, bk, wv, bv, wo, bo = _layer_weights(layer, dt)
        kc = torch.full((B * M, 1, bs, Hkv, D), float("nan"), dtype=dt, device=DEV)
        vc = kc.clone()
        hs = [torch.randn(n, H * D, generator=g).to(dt) for n in ctxs]
        kn = torch.cat([(h.double() @ wk.t() + bk) for h in hs]).to(dt).view(-1, Hkv, D).to(DEV)
        vn = torch.cat([(h.double() @ wv.t() + bv) for h in hs]).to(dt).view(-1, Hkv, D).to(DEV)
        cu = torch.tensor([0] + [sum(ctxs[:i + 1]) for i in range(B)], dtype=torch.int32, device=DEV)
        cl = torch.tensor(ctxs, dtype=torch.int32, device=DEV)
        if rot:
            cos, sin = (t.to(DEV) for t in ops.rope_tables(1024, rot))
            ops.rope_and_cache_varlen(torch.zeros(kn.shape[0], H, D, dtype=dt, device=DEV), kn, vn, kc, vc, bt.to(DEV), cu, cl,
                                      bs, 0, cos, sin)
        else:
            ops.reshape_and_cache_varlen(kn, vn, kc, vc, bt.to(DEV), cu, cl, bs, 0)
        x = torch.stack([h[-q_len:] for h in hs]).to(DEV)  # the last q_len tokens of each sequence
        with torch.no_grad():
            y = layer(x, physical_kv_cache_k=kc, physical_kv_cache_v=vc, block_tables=bt.to(DEV), context_lengths=cl,
                      kv_cache_block_size=bs, max_seq_len=max(ctxs), layer_idx=0)
        q = (x.double().cpu() @ wq.t() + bq).view(B, q_len, H, D)
        if rot:
            q = torch.stack([_rot64(q[b], torch.arange(ctxs[b] - q_len, ctxs[b]), rot) for b in range(B)])
        o, _ = dc.reference(q.permute(0, 2, 1, 3), kc.cpu(), vc.cpu(), bt, torch.tensor(ctxs), bs, 0)
        ref = o.permute(0, 2, 1, 3).reshape(B, q_len, H * D) @ wo.t() + bo
        errs[rot] = _row_err(y, ref, dt)
    _assert_bar((cls_name, dt, "paged"), errs[D], errs[0])


@pytest.mark.parametrize("cls_name", ["FlashAttentionLayer", "FlashSelfAttention"])
def test_rotary_off_takes_the_same_route_bit_for_bit(cls_name, monkeypatch):
    """rotary_dim = 0: the layer runs the route it ran before rotary existed (the pre-scaled-K kernel where it applies, seen
    through the attention launches it makes) and never touches the rotary entry points; rotary on falls back to the ordinary
    route rather than refusing."""
    from mio import ops
    from mio.kernels.attention import flash_attention as fa
    dt = torch.bfloat16
    torch.manual_seed(1)
    x = torch.randn(2, 256, 512, device=DEV).to(dt)
    calls = []
    real_fwd, real_attn, real_rot = ops.fa3_fwd, ops.flash_attention, ops.apply_rotary
    monkeypatch.setattr(ops, "fa3_fwd", lambda *a, **k: (calls.append(("fa3_fwd", ops.fa3_route(*a, **k), bool(k.get("k_prescaled")))),
                                                         real_fwd(*a, **k))[1])
    monkeypatch.setattr(ops, "flash_attention", lambda *a, **k: (calls.append(("flash_attention", None)), real_attn(*a, **k))[1])
    monkeypatch.setattr(ops, "apply_rotary", lambda *a, **k: (calls.append(("apply_rotary", None)), real_rot(*a, **k))[1])
    outs, routes = [], []
    for cfg in (fa.FlashAttentionConfig(causal=True, precision="bf16"),
                fa.FlashAttentionConfig(causal=True, precision="bf16", rotary_dim=0, rotary_interleaved=True, max_position=7)):
        torch.manual_seed(2)
        layer = getattr(fa, cls_name)(512, 8, cfg, num_kv_heads=8).to(DEV).to(dt).eval()
        calls.clear()
        with torch.no_grad():
            outs.append(layer(x))
        # no rotation, and one attention launch through ops.fa3_fwd (directly, or inside ops.flash_attention), whose
        # kernel fa3_route names
        names = [c[0] for c in calls]
        assert "apply_rotary" not in names and names.count("fa3_fwd") == 1, calls
        routes.append(list(calls))
    print(f"{cls_name}: rotary off -> {routes[0]}")
    assert routes[0] == routes[1] and torch.equal(outs[0], outs[1])
    torch.manual_seed(2)
    layer = getattr(fa, cls_name)(512, 8, fa.FlashAttentionConfig(causal=True, precision="bf16", rotary_dim=64),
                                  num_kv_heads=8).to(DEV).to(dt).eval()
    calls.clear()
    with torch.no_grad():
        y = layer(x)
    assert [c[0] for c in calls][:3] == ["apply_rotary", "apply_rotary", "flash_attention"], calls
    assert not any(c[0] == "fa3_fwd" and c[2] for c in calls), calls   # never the pre-scaled-K kernel under rotary
    assert torch.isfinite(y.float()).all() and not torch.equal(y, outs[0])
    if cls_name == "FlashSelfAttention":
        assert not layer.stream_ok(2, 256, dt, torch.nn.LayerNorm(512).to(DEV).to(dt))

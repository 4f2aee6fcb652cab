"""CPU-only tests of QK-norm (the per-head RMSNorm of q and k fused into the rotary writes): the three C-ABI symbols are bound,
every host refusal returns before a launch with a message that names the function, the ops functions refuse CPU tensors and
malformed arguments, the attention layers construct as before with the feature off, every kernel of csrc/qknorm_rope.hip
compiles for gfx950 without scratch or LDS and stores 16 bytes at a time -- and the checker of tests/_qknorm_check.py is itself
checked: a plain fp32 evaluation (squares summed sequentially, and in the kernel's lane-group butterfly) lies wholly inside
its interval, and each of seven planted defects does not."""
import ctypes as C
import re

import pytest
import torch

import _isa
import _qknorm_check as qc
import _rope_check as rc

ALIGNED = 1 << 20  # a fake 16-byte aligned device address: no refusal dereferences anything
F32 = torch.float32

QKN_SYMBOLS = {  # name -> number of C arguments
    "mio_qknorm_rope_and_cache_varlen": 34,
    "mio_qknorm_rope_and_cache_varlen_kv8": 36,
    "mio_qknorm_rope_rows": 17,
}
FUSED = ["mio_qknorm_rope_and_cache_varlen", "mio_qknorm_rope_and_cache_varlen_kv8"]


def _err():
    from mio import _lib
    return _lib.lib.mio_last_error().decode()


def _cache_rc(fn, *, D=128, rot=64, maxpos=4096, il=0, dtype=0, cos=ALIGNED, sin=ALIGNED, q=ALIGNED, q_out=ALIGNED,
              positions=None, k_scale=ALIGNED, v_scale=ALIGNED, H=8, Hkv=2, B=2, total=3, layer=0, qs=None, qw=ALIGNED,
              kw=ALIGNED, eps=1e-6):
    from mio import _lib
    st_q = (C.c_int64 * 2)(*(qs or (H * D, D)))
    st_k = (C.c_int64 * 2)(Hkv * D, D)
    head = (q, q_out, ALIGNED, ALIGNED, ALIGNED, ALIGNED)
    tail = (ALIGNED, ALIGNED, ALIGNED, positions, cos, sin, qw, kw, st_q, st_q, st_k, st_k, B, total, H, Hkv, D, rot, maxpos, il,
            8, 1, layer, 16, 4, dtype, eps, None)
    if fn.endswith("kv8"):
        return getattr(_lib.lib, fn)(*head, k_scale, v_scale, *tail)
    return getattr(_lib.lib, fn)(*head, *tail)


def _rows_rc(*, D=128, rot=64, maxpos=4096, il=0, dtype=0, cos=ALIGNED, sin=ALIGNED, x=ALIGNED, out=ALIGNED,
             positions=ALIGNED, tokens=5, heads=4, xs=None, w=ALIGNED, eps=1e-6):
    from mio import _lib
    st = (C.c_int64 * 2)(*(xs or (heads * D, D)))
    return _lib.lib.mio_qknorm_rope_rows(x, out, positions, cos, sin, w, st, st, tokens, heads, D, rot, maxpos, il, dtype, eps,
                                         None)


def test_qknorm_symbols_bound():
    from mio import _lib, ops
    for name, nargs in QKN_SYMBOLS.items():
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name), name
        assert len(getattr(_lib.lib, name).argtypes) == nargs, name
    for f in ("qk_norm_rotary", "qknorm_rope_and_cache_varlen"):
        assert callable(getattr(ops, f))


@pytest.mark.parametrize("fn", FUSED)
def test_qknorm_cache_refusals_c(fn):
    # every refusal returns before a launch: nothing here reaches the fake addresses
    kv8 = fn.endswith("kv8")
    # the norm's own arguments
    assert _cache_rc(fn, qw=None) < 0 and "null norm weight (q_weight)" in _err() and fn in _err()
    assert _cache_rc(fn, kw=None) < 0 and "null norm weight (k_weight)" in _err() and fn in _err()
    assert _cache_rc(fn, qw=ALIGNED + 8) < 0 and "16-byte alignment (norm weight q_weight)" in _err() and fn in _err()
    assert _cache_rc(fn, kw=ALIGNED + 2) < 0 and "16-byte alignment (norm weight k_weight)" in _err() and fn in _err()
    for bad in (-1e-6, float("nan"), float("inf"), float("-inf")):
        assert _cache_rc(fn, eps=bad) < 0 and "eps must be finite and not negative" in _err() and fn in _err()
    # the rotating write's rules, inherited under this entry point's name
    assert _cache_rc(fn, rot=24) < 0 and "rot_dim" in _err() and "multiple of 16" in _err() and fn in _err()
    assert _cache_rc(fn, D=64, rot=128) < 0 and "rot_dim" in _err() and fn in _err()
    assert _cache_rc(fn, rot=0) < 0 and "rot_dim" in _err() and fn in _err()
    assert _cache_rc(fn, cos=None) < 0 and "null cos / sin" in _err() and fn in _err()
    assert _cache_rc(fn, maxpos=0) < 0 and "max_position" in _err() and fn in _err()
    assert _cache_rc(fn, dtype=2) < 0 and "bf16 or fp16" in _err() and fn in _err()
    assert _cache_rc(fn, q=ALIGNED + 8) < 0 and "16-byte alignment" in _err() and fn in _err()
    assert _cache_rc(fn, q_out=ALIGNED + 2) < 0 and "16-byte alignment" in _err() and fn in _err()
    assert _cache_rc(fn, cos=ALIGNED + 4) < 0 and "16-byte alignment" in _err() and fn in _err()
    assert _cache_rc(fn, positions=ALIGNED + 2) < 0 and "16-byte alignment" in _err() and fn in _err()
    assert _cache_rc(fn, q=None) < 0 and "null pointer" in _err() and fn in _err()
    assert _cache_rc(fn, qs=(8 * 128 + 4, 128)) < 0 and "16-byte alignment" in _err() and fn in _err()
    assert _cache_rc(fn, il=2) < 0 and "interleaved" in _err() and fn in _err()
    assert _cache_rc(fn, D=136, rot=64) < 0 and "head_dim" in _err() and fn in _err()
    assert _cache_rc(fn, D=12, rot=16) < 0 and "head_dim" in _err() and fn in _err()
    assert _cache_rc(fn, H=3) < 0 and "bad sizes" in _err() and fn in _err()
    assert _cache_rc(fn, layer=1) < 0 and "bad cache geometry" in _err() and fn in _err()
    if kv8:
        assert _cache_rc(fn, rot=16) < 0 and "multiple of 32" in _err() and fn in _err()
        assert _cache_rc(fn, rot=48, D=64) < 0 and "multiple of 32" in _err()
        assert _cache_rc(fn, k_scale=None) < 0 and "k_scale and v_scale are required" in _err() and fn in _err()
        assert _cache_rc(fn, D=72, rot=64) < 0 and "head_dim must be a multiple of 16" in _err()
    # nothing to do: 0 without a launch, and without looking at the data pointers or the weights -- but eps is still judged
    assert _cache_rc(fn, B=0, q=None, qw=None) == 0
    assert _cache_rc(fn, total=0, q=None, kw=None, eps=0.0) == 0
    assert _cache_rc(fn, total=0, eps=-1.0) < 0 and "eps" in _err()


def test_qknorm_rows_refusals_c():
    fn = "mio_qknorm_rope_rows"
    assert _rows_rc(w=None) < 0 and "null norm weight (weight)" in _err() and fn in _err()
    assert _rows_rc(w=ALIGNED + 8) < 0 and "16-byte alignment (norm weight weight)" in _err() and fn in _err()
    for bad in (-1e-6, float("nan"), float("inf")):
        assert _rows_rc(eps=bad) < 0 and "eps must be finite and not negative" in _err() and fn in _err()
    assert _rows_rc(rot=24) < 0 and "rot_dim" in _err() and fn in _err()
    assert _rows_rc(D=64, rot=128) < 0 and "rot_dim" in _err() and fn in _err()
    assert _rows_rc(cos=None) < 0 and "null cos / sin" in _err() and fn in _err()
    assert _rows_rc(maxpos=0) < 0 and "max_position" in _err() and fn in _err()
    assert _rows_rc(dtype=2) < 0 and "bf16 or fp16" in _err() and fn in _err()
    assert _rows_rc(x=ALIGNED + 8) < 0 and "16-byte alignment" in _err() and fn in _err()
    assert _rows_rc(out=ALIGNED + 8) < 0 and "16-byte alignment" in _err()
    assert _rows_rc(positions=None) < 0 and "null pointer" in _err() and fn in _err()
    assert _rows_rc(xs=(516, 128)) < 0 and "16-byte alignment" in _err()
    assert _rows_rc(xs=(-512, 128)) < 0 and "16-byte alignment" in _err()
    assert _rows_rc(heads=0) < 0 and "bad sizes" in _err() and fn in _err()
    assert _rows_rc(D=12, rot=16) < 0 and "head_dim" in _err()
    assert _rows_rc(D=136, rot=64) < 0 and "head_dim" in _err()
    assert _rows_rc(tokens=0, x=None, w=None) == 0


def test_qknorm_ops_errors_without_gpu():
    from mio import ops
    bf = torch.bfloat16
    cos, sin = ops.rope_tables(64, 32)
    x = torch.zeros(5, 4, 64, dtype=bf)
    w = torch.ones(64, dtype=bf)
    pos = torch.zeros(5, dtype=torch.int32)
    with pytest.raises(ValueError, match="CUDA"):
        ops.qk_norm_rotary(x, w, cos, sin, pos)
    with pytest.raises(ValueError):
        ops.qk_norm_rotary(torch.zeros(5, 64, dtype=bf), w, cos, sin, pos)  # not 3-D / 4-D
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="eps"):
            ops.qk_norm_rotary(x, w, cos, sin, pos, eps=bad)
    with pytest.raises(ValueError, match="weight"):
        ops.qk_norm_rotary(x, None, cos, sin, pos)
    k = torch.zeros(5, 2, 64, dtype=bf)
    kc = torch.zeros(4, 1, 16, 2, 64, dtype=bf)
    bt = torch.zeros(1, 4, dtype=torch.int32)
    cu = torch.tensor([0, 5], dtype=torch.int32)
    cl = torch.tensor([5], dtype=torch.int32)
    with pytest.raises(ValueError, match="CUDA"):
        ops.qknorm_rope_and_cache_varlen(x, k, k, kc, kc, bt, cu, cl, 16, 0, cos, sin, w, w)
    with pytest.raises(ValueError, match="eps"):
        ops.qknorm_rope_and_cache_varlen(x, k, k, kc, kc, bt, cu, cl, 16, 0, cos, sin, w, w, eps=-1e-3)
    with pytest.raises(ValueError, match="k_weight"):
        ops.qknorm_rope_and_cache_varlen(x, k, k, kc, kc, bt, cu, cl, 16, 0, cos, sin, w, None)
    # the weight check both functions share, on CPU tensors (it dereferences nothing)
    ops._qk_weight_ok(w, x, "weight", "f")
    for bad in (torch.ones(32, dtype=bf), torch.ones(64), torch.ones(1, 64, dtype=bf), torch.ones(128, dtype=bf)[::2], None,
                torch.ones(72, dtype=bf)[4:68]):
        with pytest.raises(ValueError, match="f: weight"):
            ops._qk_weight_ok(bad, x, "weight", "f")


# ---- the checker itself ---------------------------------------------------------------------------------------------
def _units(D, rot, il):
    """The element lists of the kernel's units of a 16-bit head row: rotated ones first, then the others."""
    half = rot // 2
    if il:
        us = [list(range(8 * u, 8 * u + 8)) for u in range(rot // 8)]
    else:
        us = [list(range(8 * u, 8 * u + 8)) + list(range(half + 8 * u, half + 8 * u + 8)) for u in range(rot // 16)]
    return us + [list(range(e, e + 8)) for e in range(rot, D, 8)]


def _sum_squares(sq, order, rot, il):
    """fp32 sum over the last dim of sq in one of two orders: "seq" element by element; "butterfly" as the kernel: every lane
    of a group of G = 2^k lanes sums its unit's squares in order, then log2 G steps of lane ^= 1, 2, 4, 8 adds."""
    D = sq.shape[-1]
    if order == "seq":
        acc = torch.zeros(sq.shape[:-1], dtype=F32)
        for d in range(D):
            acc = acc + sq[..., d]
        return acc
    us = _units(D, rot, il)
    G = 1
    while G < len(us):
        G *= 2
    lanes = torch.zeros(*sq.shape[:-1], G, dtype=F32)
    for u, idx in enumerate(us):
        acc = torch.zeros(sq.shape[:-1], dtype=F32)
        for d in idx:
            acc = acc + sq[..., d]
        lanes[..., u] = acc
    m = 1
    while m < G:
        lanes = lanes + lanes[..., torch.arange(G) ^ m]
        m *= 2
    assert (lanes == lanes[..., :1]).all()  # one statistic per row, the same bits in every lane
    return lanes[..., 0]


def _rotate32(n, cos, sin, pos, il):
    half = cos.shape[1]
    rot = 2 * half
    c, s = cos[pos][:, None, :], sin[pos][:, None, :]
    n1, n2 = (n[..., 0:rot:2], n[..., 1:rot:2]) if il else (n[..., :half], n[..., half:rot])
    y1, y2 = n1 * c - n2 * s, n2 * c + n1 * s
    y = torch.stack([y1, y2], -1).flatten(-2) if il else torch.cat([y1, y2], -1)
    return torch.cat([y, n[..., rot:]], -1)


def _eval32(x, w, eps, cos, sin, pos, il, order="seq", defect=None, w_other=None):
    """A plain fp32 evaluation of the norm and the rotation of x [T, heads, D] (fp32 result, not yet rounded), in the kernel's
    operation order; defect plants one named error."""
    D = x.shape[-1]
    half = cos.shape[1]
    rot = 2 * half
    xf = x.float()
    sq = xf * xf
    if defect == "mean over rot_dim":
        ss, cnt = _sum_squares(sq[..., :rot], "seq", rot, il), rot
    else:
        ss, cnt = _sum_squares(sq, order, rot, il), D
    if defect == "statistic of the neighbouring head":
        ss = ss.roll(1, dims=1)
    e = torch.tensor(0.0 if defect == "eps dropped" else eps, dtype=F32)
    r = torch.rsqrt(ss / torch.tensor(float(cnt), dtype=F32) + e)[..., None]
    wf = w.float()
    if defect == "weight of the partner element":
        wf = torch.cat([wf[:rot].roll(half), wf[rot:]])
    if defect == "k normalised with the q weight":
        wf = w_other.float()
    if defect == "norm after the rotation":
        return _rotate32(xf, cos, sin, pos, il) * r * wf
    n = xf * r * wf
    if defect == "n rounded to 16 bits before the rotation":
        n = n.to(x.dtype).float()
    return _rotate32(n, cos, sin, pos, il)


def _inputs(dtype, D, T=384, seed=0):
    """q and k weights that differ and vary with d; heads scaled by different powers of two (2^-10: a mean square of the size of
    eps); x not centred."""
    g = torch.Generator().manual_seed(seed)
    scale = torch.tensor([2.0 ** -10, 2.0 ** -3, 1.0, 2.0 ** 4])
    x = ((torch.randn(T, 4, D, generator=g) + 0.5) * scale[None, :, None]).to(dtype)
    wq = (0.5 + torch.rand(D, generator=g)).to(dtype)
    wk = (1.5 - torch.rand(D, generator=g) * torch.linspace(0.2, 1.0, D)).to(dtype)
    return x, wq, wk


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("D,rot", [(64, 64), (80, 48), (96, 32), (128, 128), (128, 64)])
def test_interval_holds_for_a_plain_fp32_evaluation(dtype, interleaved, D, rot):
    """The reference alone meets the zero-outside bar: a plain fp32 evaluation, its squares summed sequentially or in the
    kernel's butterfly, lies inside the interval everywhere, for the 16-bit store and (where the geometry allows) the fp8 one."""
    from mio import ops
    P, eps = 4096, 1e-6
    x, wq, _ = _inputs(dtype, D, seed=D + rot)
    cos, sin = ops.rope_tables(P, rot)
    pos = torch.randint(0, P, (x.shape[0],), generator=torch.Generator().manual_seed(1))
    ref, delta = qc.reference(x, wq, eps, cos, sin, pos, interleaved)
    ys = {order: _eval32(x, wq, eps, cos, sin, pos, interleaved, order) for order in ("seq", "butterfly")}
    for order, y in ys.items():
        out, differ = qc.outside16(y.to(dtype), ref, delta, dtype)
        assert out == 0, (order, out, differ)
        if D % 16 == 0 and (interleaved or rot % 32 == 0):
            scale = 0.37
            inv = torch.tensor(1.0) / torch.tensor(scale)
            y8 = (y * inv).clamp(-448, 448).to(rc.F8)
            assert qc.outside8(y8, ref, delta, scale) == 0, order
    # a zero row is exactly zero with a zero allowance; the reference and the rule agree
    z = torch.zeros(2, 4, D, dtype=dtype)
    zr, zd = qc.reference(z, wq, eps, cos, sin, pos[:2], interleaved)
    assert (zr == 0).all() and (zd == 0).all()
    assert (_eval32(z, wq, eps, cos, sin, pos[:2], interleaved, "butterfly") == 0).all()


DEFECTS = ["mean over rot_dim", "eps dropped", "weight of the partner element", "statistic of the neighbouring head",
           "k normalised with the q weight", "n rounded to 16 bits before the rotation", "norm after the rotation"]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("defect", DEFECTS)
def test_planted_defects_fall_outside_the_interval(dtype, interleaved, defect):
    """Each planted defect fails the check the sound evaluation passes (D 128, rot_dim 64: the mean over rot_dim differs from
    the mean over head_dim)."""
    from mio import ops
    D, rot, P, eps = 128, 64, 4096, 1e-6
    x, wq, wk = _inputs(dtype, D, seed=7)
    cos, sin = ops.rope_tables(P, rot)
    pos = torch.randint(1, P, (x.shape[0],), generator=torch.Generator().manual_seed(2))
    ref, delta = qc.reference(x, wk, eps, cos, sin, pos, interleaved)
    good = _eval32(x, wk, eps, cos, sin, pos, interleaved, "butterfly").to(dtype)
    assert qc.outside16(good, ref, delta, dtype)[0] == 0
    bad = _eval32(x, wk, eps, cos, sin, pos, interleaved, "butterfly", defect=defect, w_other=wq).to(dtype)
    out, _ = qc.outside16(bad, ref, delta, dtype)
    print(f"{defect}: {out} of {ref.numel()} elements outside")
    assert out > 0, defect
    if defect == "eps dropped":  # seen on the head whose mean square is of the size of eps, and only there
        per_head = [qc.outside16(bad[:, h], ref[:, h], delta[:, h], dtype)[0] for h in range(4)]
        assert per_head[0] > 0.5 * ref[:, 0].numel() and per_head[2] == per_head[3] == 0, per_head


# ---- modules ---------------------------------------------------------------------------------------------------------
def test_qk_norm_off_constructs_layers_as_before():
    from mio.kernels.attention.flash_attention import FlashAttentionConfig, FlashAttentionLayer, FlashSelfAttention
    cfg = FlashAttentionConfig()
    assert cfg.qk_norm is False and cfg.qk_norm_eps == 1e-6
    # the new fields come last: positional construction of the earlier fields is unchanged
    assert FlashAttentionConfig(64, True).block_size == 64 and FlashAttentionConfig(64, True).causal is True
    for cls in (FlashAttentionLayer, FlashSelfAttention):
        torch.manual_seed(3)
        a = cls(256, 4, FlashAttentionConfig(causal=True, rotary_dim=32), num_kv_heads=2)
        torch.manual_seed(3)
        b = cls(256, 4, FlashAttentionConfig(causal=True, rotary_dim=32, qk_norm=False, qk_norm_eps=1e-5), num_kv_heads=2)
        torch.manual_seed(3)
        on = cls(256, 4, FlashAttentionConfig(causal=True, rotary_dim=32, qk_norm=True), num_kv_heads=2)
        sa, sb, so = a.state_dict(), b.state_dict(), on.state_dict()
        assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)  # no new parameter or buffer
        assert not hasattr(a, "q_norm") and not hasattr(a, "k_norm")
        assert not [k for k in sa if "norm" in k]
        # on: the two [head_dim] weights, ones, and every other parameter drawn as before
        assert sorted(set(so) - set(sa)) == ["k_norm.weight", "q_norm.weight"]
        assert all(torch.equal(so[k], sa[k]) for k in sa)
        for n in ("q_norm", "k_norm"):
            w = getattr(on, n).weight
            assert isinstance(w, torch.nn.Parameter) and tuple(w.shape) == (64,) and (w == 1).all()


def test_qk_norm_needs_rotary():
    from mio.kernels.attention.flash_attention import FlashAttentionConfig, FlashAttentionLayer, FlashSelfAttention
    for cls in (FlashAttentionLayer, FlashSelfAttention):
        with pytest.raises(ValueError, match="qk_norm"):
            cls(256, 4, FlashAttentionConfig(qk_norm=True, rotary_dim=0))
        with pytest.raises(ValueError, match="qk_norm"):
            cls(256, 4, FlashAttentionConfig(qk_norm=True))
        cls(256, 4, FlashAttentionConfig(qk_norm=True, rotary_dim=64))


def test_model_converter_copies_qk_norm_weights():
    from mio.kernels.attention.flash_attention import FlashAttentionConfig, FlashAttentionLayer, ModelConverter
    nn = torch.nn

    class Norm(nn.Module):
        def __init__(self, n):
            super().__init__()
            self.weight = nn.Parameter(torch.rand(n) + 0.5)

    class SrcAttention(nn.Module):
        def __init__(self, norm_width):
            super().__init__()
            self.num_heads, self.hidden_size = 4, 256
            self.q_proj, self.k_proj, self.v_proj, self.o_proj = (nn.Linear(256, 256) for _ in range(4))
            if norm_width:
                self.q_norm, self.k_norm = Norm(norm_width), Norm(norm_width)

    class Model(nn.Module):
        def __init__(self, norm_width):
            super().__init__()
            self.attn = SrcAttention(norm_width)

    torch.manual_seed(0)
    on = FlashAttentionConfig(rotary_dim=64, qk_norm=True)
    src = Model(64)
    wq, wk = src.attn.q_norm.weight.detach().clone(), src.attn.k_norm.weight.detach().clone()
    rep = ModelConverter(on).convert_model(src).attn
    assert isinstance(rep, FlashAttentionLayer)
    assert torch.equal(rep.q_norm.weight, wq) and torch.equal(rep.k_norm.weight, wk) and not torch.equal(wq, wk)
    # a whole-hidden-size norm (OLMo-2 style) is not a per-head weight: left alone; so is a source without norms
    for width in (256, 0):
        rep = ModelConverter(on).convert_model(Model(width)).attn
        assert (rep.q_norm.weight == 1).all() and (rep.k_norm.weight == 1).all()
    # qk_norm off: nothing is copied, nothing is created
    rep = ModelConverter(FlashAttentionConfig(rotary_dim=64)).convert_model(Model(64)).attn
    assert isinstance(rep, FlashAttentionLayer) and not hasattr(rep, "q_norm")


# ---- the unit's ISA ----------------------------------------------------------------------------------------------------
# mangled-name pattern -> instantiations: bf16 / fp16, both pairings, 16-bit and fp8 cache; the rows form has no cache kind
_QKN_UNIT_KERNELS = {r"qknorm_rope_and_cache_varlen_kernel": 8, r"qknorm_rope_rows_kernel": 4}


def test_qknorm_kernels_isa(tmp_path):
    """Every kernel of csrc/qknorm_rope.hip exists, with zero scratch and zero spills (read from the metadata), uses no LDS,
    and moves data with 16-byte stores only; the write unit's kernel names are not reused."""
    text = _isa.device_isa(tmp_path, "qknorm_rope.hip", [], attention=False).read_text()
    for name, want in _QKN_UNIT_KERNELS.items():
        blks = _isa.metadata(text, rf"_Z\d+{name}\w+")
        assert len(blks) == want, name
        for blk in blks:
            _isa.check_fits_256(blk)
        assert len(_isa.kernels(text, rf"_Z\d+{name}")) == want
    total = sum(_QKN_UNIT_KERNELS.values())
    assert not _isa.metadata(text, r"_Z\d+(rope_and_cache_varlen_kernel|rope_rows_kernel|cache_write)\w+")
    lds = re.findall(r"\.group_segment_fixed_size:\s+(\d+)", text)
    assert len(lds) == total == 12 and set(lds) == {"0"}
    code = [l.split("//")[0].split(";")[0] for l in text.splitlines()]
    stores = [l for l in code if re.search(r"\b(global|flat|buffer|scratch)_store", l)]
    assert stores and all("global_store_dwordx4" in l for l in stores), [l for l in stores if "dwordx4" not in l][:4]
    assert not [l for l in code if re.search(r"\bscratch_|\bds_", l)]  # registers and DPP only: not even a ds_bpermute
    # rows, weights and tables are read 16 bytes at a time; narrower loads are the int32 lookups and the fp8 scales
    assert sum("global_load_dwordx4" in l for l in code) >= 8 * total
    narrow = [l for l in code if re.search(r"\bglobal_load_(dword|dwordx2|ushort|short|ubyte|sbyte)\b", l)]
    assert len(narrow) <= 8 * total, len(narrow)
    # the statistic: the cross-lane adds are DPP, four steps (groups of up to 16 lanes) at every place a row is computed
    assert sum("row_half_mirror" in l for l in code) >= total

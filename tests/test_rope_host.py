"""CPU-only tests of rotary position embedding: the three C-ABI symbols are bound, every host refusal returns before a launch
with a message that names the function, the ops functions refuse CPU tensors and malformed arguments, rope_tables is the
fp64 formula cast once, every kernel of csrc/cache_write.hip compiles for gfx950 without scratch and stores 16 bytes at a time,
and a config without rotary builds the attention layers as before.  The checker's own rounding (tests/_rope_check.py) is
tested against exhaustive and randomised cases."""
import ctypes as C
import math
import re

import pytest
import torch

import _isa
import _rope_check as rc

ALIGNED = 1 << 20  # a fake 16-byte aligned device address: no refusal dereferences anything

ROPE_SYMBOLS = {  # name -> number of C arguments
    "mio_rope_and_cache_varlen": 31,
    "mio_rope_and_cache_varlen_kv8": 33,
    "mio_rope_rows": 15,
}


def _err():
    from mio import _lib
    return _lib.lib.mio_last_error().decode()


def _cache_rc(fn, *, D=128, rot=64, maxpos=4096, il=0, dtype=0, cos=ALIGNED, sin=ALIGNED, q=ALIGNED, q_out=ALIGNED,
              positions=None, k_scale=ALIGNED, v_scale=ALIGNED, H=8, Hkv=2, B=2, total=3, layer=0, qs=None):
    from mio import _lib
    st_q = (C.c_int64 * 2)(*(qs or (H * D, D)))
    st_k = (C.c_int64 * 2)(Hkv * D, D)
    head = (q, q_out, ALIGNED, ALIGNED, ALIGNED, ALIGNED)
    tail = (ALIGNED, ALIGNED, ALIGNED, positions, cos, sin, st_q, st_q, st_k, st_k, B, total, H, Hkv, D, rot, maxpos, il,
            8, 1, layer, 16, 4, dtype, None)
    if fn.endswith("kv8"):
        return getattr(_lib.lib, fn)(*head, k_scale, v_scale, *tail)
    return getattr(_lib.lib, fn)(*head, *tail)


def _rows_rc(*, D=128, rot=64, maxpos=4096, il=0, dtype=0, cos=ALIGNED, sin=ALIGNED, x=ALIGNED, out=ALIGNED,
             positions=ALIGNED, tokens=5, heads=4, xs=None):
    from mio import _lib
    st = (C.c_int64 * 2)(*(xs or (heads * D, D)))
    return _lib.lib.mio_rope_rows(x, out, positions, cos, sin, st, st, tokens, heads, D, rot, maxpos, il, dtype, None)


def test_rope_symbols_bound():
    from mio import _lib, ops
    for name, nargs in ROPE_SYMBOLS.items():
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name), name
        assert len(getattr(_lib.lib, name).argtypes) == nargs, name
    assert _lib.lib.mio_version() == 106
    for f in ("rope_tables", "apply_rotary", "rope_and_cache_varlen"):
        assert callable(getattr(ops, f))


@pytest.mark.parametrize("fn", ["mio_rope_and_cache_varlen", "mio_rope_and_cache_varlen_kv8"])
def test_rope_cache_refusals_c(fn):
    # every refusal returns before a launch: nothing here reaches the fake addresses
    kv8 = fn.endswith("kv8")
    assert _cache_rc(fn, rot=24) < 0 and "rot_dim" in _err() and "multiple of 16" in _err() and fn in _err()
    assert _cache_rc(fn, D=64, rot=128) < 0 and "rot_dim" in _err() and fn in _err()
    assert _cache_rc(fn, rot=0) < 0 and "rot_dim" in _err() and fn in _err()
    assert _cache_rc(fn, cos=None) < 0 and "null cos / sin" in _err() and fn in _err()
    assert _cache_rc(fn, sin=None) < 0 and "null cos / sin" in _err() and fn in _err()
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
    assert _cache_rc(fn, H=3) < 0 and "bad sizes" in _err() and fn in _err()
    assert _cache_rc(fn, layer=1) < 0 and "bad cache geometry" in _err() and fn in _err()
    # rot_dim 16 with the neox pairing: an fp8 cache's 16-element chunk has no whole partner chunk
    if kv8:
        assert _cache_rc(fn, rot=16) < 0 and "multiple of 32" in _err() and fn in _err()
        assert _cache_rc(fn, rot=48, D=64) < 0 and "multiple of 32" in _err()
        assert _cache_rc(fn, k_scale=None) < 0 and "k_scale and v_scale are required" in _err() and fn in _err()
        assert _cache_rc(fn, D=72, rot=64) < 0 and "head_dim must be a multiple of 16" in _err()
    # nothing to do: 0 without a launch (and without looking at the data pointers)
    assert _cache_rc(fn, B=0, q=None) == 0
    assert _cache_rc(fn, total=0, q=None) == 0


def test_rope_rows_refusals_c():
    fn = "mio_rope_rows"
    assert _rows_rc(rot=24) < 0 and "rot_dim" in _err() and fn in _err()
    assert _rows_rc(D=64, rot=128) < 0 and "rot_dim" in _err() and fn in _err()
    assert _rows_rc(cos=None) < 0 and "null cos / sin" in _err() and fn in _err()
    assert _rows_rc(maxpos=0) < 0 and "max_position" in _err() and fn in _err()
    assert _rows_rc(maxpos=-3) < 0 and "max_position" in _err()
    assert _rows_rc(dtype=2) < 0 and "bf16 or fp16" in _err() and fn in _err()
    assert _rows_rc(x=ALIGNED + 8) < 0 and "16-byte alignment" in _err() and fn in _err()
    assert _rows_rc(out=ALIGNED + 8) < 0 and "16-byte alignment" in _err()
    assert _rows_rc(sin=ALIGNED + 8) < 0 and "16-byte alignment" in _err()
    assert _rows_rc(positions=None) < 0 and "null pointer" in _err() and fn in _err()
    assert _rows_rc(xs=(516, 128)) < 0 and "16-byte alignment" in _err()
    assert _rows_rc(xs=(-512, 128)) < 0 and "16-byte alignment" in _err()
    assert _rows_rc(heads=0) < 0 and "bad sizes" in _err() and fn in _err()
    assert _rows_rc(D=12, rot=16) < 0 and "head_dim" in _err()
    assert _rows_rc(tokens=0, x=None) == 0


def test_rope_tables_are_the_fp64_formula():
    from mio import ops
    for P, rot, base in ((1000, 64, 10000.0), (4096, 128, 500000.0), (17, 16, 10000.0)):
        cos, sin = ops.rope_tables(P, rot, base)
        assert cos.dtype == sin.dtype == torch.float32 and cos.shape == sin.shape == (P, rot // 2)
        assert cos.is_contiguous() and sin.is_contiguous()
        p = torch.arange(P, dtype=torch.float64)[:, None]
        i = torch.arange(rot // 2, dtype=torch.float64)[None, :]
        ang = p * base ** (-2.0 * i / rot)
        assert torch.equal(cos, torch.cos(ang).to(torch.float32))
        assert torch.equal(sin, torch.sin(ang).to(torch.float32))
    assert ops.rope_tables(8, 16)[0][0].eq(1).all() and ops.rope_tables(8, 16)[1][0].eq(0).all()
    for bad in ((0, 64), (16, 0), (16, 31), (-1, 64)):
        with pytest.raises(ValueError):
            ops.rope_tables(*bad)


def test_rope_ops_errors_without_gpu():
    from mio import ops
    bf = torch.bfloat16
    cos, sin = ops.rope_tables(64, 32)
    x = torch.zeros(5, 4, 64, dtype=bf)
    pos = torch.zeros(5, dtype=torch.int32)
    with pytest.raises(ValueError, match="CUDA"):
        ops.apply_rotary(x, cos, sin, pos)
    with pytest.raises(ValueError):
        ops.apply_rotary(torch.zeros(5, 64, dtype=bf), cos, sin, pos)  # not 3-D / 4-D
    k = torch.zeros(5, 2, 64, dtype=bf)
    kc = torch.zeros(4, 1, 16, 2, 64, dtype=bf)
    bt = torch.zeros(1, 4, dtype=torch.int32)
    cu = torch.tensor([0, 5], dtype=torch.int32)
    cl = torch.tensor([5], dtype=torch.int32)
    with pytest.raises(ValueError, match="CUDA"):
        ops.rope_and_cache_varlen(x, k, k, kc, kc, bt, cu, cl, 16, 0, cos, sin)


def test_rope_table_argument_checks():
    """The table checks both ops functions share, on CPU tensors (they dereference nothing)."""
    from mio import ops
    dev = torch.device("cpu")
    ok = ops.rope_tables(64, 32)
    assert ops._rope_tables_ok(*ok, 64, False, False, dev, "f") == (64, 32)
    assert ops._rope_tables_ok(*ok, 64, True, False, dev, "f") == (64, 32)
    assert ops._rope_tables_ok(*ops.rope_tables(64, 16), 64, True, True, dev, "f") == (64, 16)
    bad = [
        (ops.rope_tables(64, 24), 64, False, False),                        # rot_dim 24
        (ops.rope_tables(64, 128), 64, False, False),                       # rot_dim > head_dim
        (ops.rope_tables(64, 16), 64, True, False),                         # fp8 cache, neox, rot_dim 16
        ((ok[0].double(), ok[1]), 64, False, False),                        # not fp32
        ((ok[0], ok[1][:32]), 64, False, False),                            # unequal shapes
        ((ok[0].t().contiguous().t(), ok[1]), 64, False, False),            # not contiguous
        ((ok[0][0], ok[1][0]), 64, False, False),                           # 1-D
        ((ok[0][:0], ok[1][:0]), 64, False, False),                         # no position
        ((None, ok[1]), 64, False, False),
    ]
    for (cos, sin), D, kv8, il in bad:
        with pytest.raises(ValueError, match="f: "):
            ops._rope_tables_ok(cos, sin, D, kv8, il, dev, "f")


# mangled-name pattern -> instantiations: the rotating and rotation kernels (bf16 / fp16, both pairings, 16-bit and fp8 cache), the
# plain writes' fp8 forms per source dtype and their 16-bit forms once (over unsigned short: they move bits)
_WRITE_UNIT_KERNELS = {r"rope_and_cache_varlen_kernel": 8, r"rope_rows_kernel": 4, r"cache_write_kernelI\w+Lb1E": 2,
                       r"cache_write_varlen_kernelI\w+Lb1E": 2, r"cache_write_kernelItLb0E": 1, r"cache_write_varlen_kernelItLb0E": 1}


def test_rope_kernels_isa(tmp_path):
    """Every kernel of the write unit (csrc/cache_write.hip: the rotating writes, the standalone rotation and the plain cache
    writes) exists, with no scratch and no spills, moves data with 16-byte stores only and uses no LDS; the decode units'
    kernel names are not reused."""
    text = _isa.device_isa(tmp_path, "cache_write.hip", [], attention=False).read_text()
    for name, want in _WRITE_UNIT_KERNELS.items():
        blks = _isa.metadata(text, rf"_Z\d+{name}\w+")
        assert len(blks) == want, name
        for blk in blks:
            _isa.check_fits_256(blk)
        bodies = _isa.kernels(text, rf"_Z\d+{name}")
        assert len(bodies) == want
    total = sum(_WRITE_UNIT_KERNELS.values())
    assert not _isa.metadata(text, r"_Z\d+(decode_|reshape_and_cache)\w+")
    lds = re.findall(r"\.group_segment_fixed_size:\s+(\d+)", text)
    assert len(lds) == total == 18 and set(lds) == {"0"}
    code = [l.split("//")[0].split(";")[0] for l in text.splitlines()]
    stores = [l for l in code if re.search(r"\b(global|flat|buffer|scratch)_store", l)]
    assert stores and all("global_store_dwordx4" in l for l in stores), [l for l in stores if "dwordx4" not in l][:4]
    assert not [l for l in code if re.search(r"\bscratch_|\bds_(read|write|load|store)", l)]
    # the 16-bit loads and the table reads are 16 bytes wide; narrower loads are the int32 lookups and the fp8 scales
    assert sum("global_load_dwordx4" in l for l in code) >= 8 * total


def test_rotary_off_constructs_layers_as_before():
    from mio.kernels.attention.flash_attention import FlashAttentionConfig, FlashAttentionLayer, FlashSelfAttention
    cfg = FlashAttentionConfig()
    assert cfg.rotary_dim == 0 and cfg.rotary_base == 10000.0 and cfg.rotary_interleaved is False
    assert cfg.max_position > 0
    # the new fields come last: positional construction of the earlier fields is unchanged
    assert FlashAttentionConfig(64, True).block_size == 64 and FlashAttentionConfig(64, True).causal is True
    for cls in (FlashAttentionLayer, FlashSelfAttention):
        torch.manual_seed(3)
        a = cls(256, 4, FlashAttentionConfig(causal=True), num_kv_heads=2)
        torch.manual_seed(3)
        b = cls(256, 4, FlashAttentionConfig(causal=True, rotary_dim=0), num_kv_heads=2)
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)  # no new parameter or buffer
        assert not [n for n, _ in a.named_buffers()]
    with pytest.raises(ValueError):
        FlashAttentionLayer(256, 4, FlashAttentionConfig(rotary_dim=24))      # not a multiple of 16
    with pytest.raises(ValueError):
        FlashSelfAttention(256, 4, FlashAttentionConfig(rotary_dim=128))      # above head_dim 64


# ---- the checker's own rounding -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, rc.F8])
def test_rn_is_round_to_nearest_even(dtype):
    vals, _ = rc._table(dtype)
    # every representable value is a fixed point; a midpoint goes to the even neighbour; just off a midpoint to the nearer
    assert torch.equal(rc.rn(vals, dtype), vals)
    a, b = vals[:-1], vals[1:]
    mid = (a + b) / 2  # exact in fp64
    r = rc.rn(mid, dtype)
    assert ((r == a) | (r == b)).all()
    up, dn = mid + (b - a) / 1024, mid - (b - a) / 1024
    assert torch.equal(rc.rn(up, dtype), b) and torch.equal(rc.rn(dn, dtype), a)
    if dtype != rc.F8:
        # agrees with torch's cast wherever that does not round twice: fp32 inputs
        g = torch.Generator().manual_seed(1)
        x = (torch.randn(200000, generator=g) * 3).to(torch.float32)
        assert torch.equal(rc.rn(x.double(), dtype), x.to(dtype).double())
        assert torch.equal(r, mid.to(torch.float32).to(dtype).double())  # midpoints are exact in fp32: ties to even
    else:
        x = torch.linspace(-448, 448, 100001, dtype=torch.float32)
        assert torch.equal(rc.rn(x.double(), dtype), x.to(dtype).double())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("interleaved", [False, True])
def test_interval_rule_holds_for_a_plain_fp32_evaluation(dtype, interleaved):
    """A plain fp32 evaluation on the CPU lies inside the interval everywhere (the bar the GPU tests use is derived, not
    measured), while a rotation at the neighbouring position does not."""
    from mio import ops
    g = torch.Generator().manual_seed(5)
    T, Hn, D, rot, P = 4096, 4, 128, 128, 131072
    cos, sin = ops.rope_tables(P, rot)
    x = torch.randn(T, Hn, D, generator=g).to(dtype)
    pos = torch.randint(0, P, (T,), generator=g)
    ref, delta = rc.reference(x, cos, sin, pos, interleaved)
    c, s = cos[pos][:, None, :], sin[pos][:, None, :]
    xf = x.float()
    x1, x2 = (xf[..., 0::2], xf[..., 1::2]) if interleaved else (xf[..., :rot // 2], xf[..., rot // 2:])
    y1, y2 = x1 * c - x2 * s, x2 * c + x1 * s
    y = (torch.stack([y1, y2], -1).flatten(-2) if interleaved else torch.cat([y1, y2], -1)).to(dtype)
    out, differ = rc.outside16(y, ref, delta, dtype)
    assert out == 0, (out, differ)
    wrong, _ = rc.reference(x, cos, sin, (pos + 1) % P, interleaved)
    assert rc.outside16(wrong.to(torch.float32).to(dtype), ref, delta, dtype)[0] > 0.5 * y.numel()
    # the fp8 interval, same evaluation: y * inv clamped and rounded once
    scale = 0.37
    inv = torch.tensor(1.0) / torch.tensor(scale)
    y32 = torch.stack([y1, y2], -1).flatten(-2) if interleaved else torch.cat([y1, y2], -1)
    y8 = (y32 * inv).clamp(-448, 448).to(rc.F8)
    assert rc.outside8(y8, ref, delta, scale) == 0
    assert math.isclose(float(inv), 1 / scale, rel_tol=1e-6)

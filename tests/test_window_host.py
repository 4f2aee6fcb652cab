"""CPU-only tests of sliding-window paged decode (mio_fa3_decode_paged_window, mio_fa3_decode_window_route): the C-ABI
symbols are bound, the route query picks the per-head / whole-row / GQA kernel from the window span rather than max_ctx,
every refusal is reported at the C level and raised by ops before any tensor is touched, and the windowed decode kernels
compile without scratch."""
import ctypes as C
import re

import pytest
import torch

import _isa

ALIGNED = 1 << 20  # a fake 16-byte aligned device address: the route query dereferences nothing


def _route_rc(B=4, H=8, Hkv=2, q_len=1, D=128, bs=16, max_blocks=64, max_ctx=1024, left=-1, right=-1, dtype=0,
              fn="mio_fa3_decode_window_route", layers=1, layer=0):
    from mio import _lib
    qs = (C.c_int64 * 3)(H * q_len * D, q_len * D, D)
    os_ = (C.c_int64 * 3)(H * q_len * D, q_len * D, D)
    return getattr(_lib.lib, fn)(ALIGNED, ALIGNED, ALIGNED, ALIGNED, ALIGNED, ALIGNED, qs, os_, B, H, Hkv, q_len, D,
                                 layers, layer, bs, max_blocks, max_ctx, 0.125, left, right, dtype, None, None)


def _route(**kw):
    from mio import _lib
    r = _route_rc(**kw)
    return _lib.DECODE_ROUTES.get(r) if r >= 0 else None


def _err():
    from mio import _lib
    return _lib.lib.mio_last_error().decode()


def test_window_symbols_bound():
    from mio import _lib, ops
    for name in ("mio_fa3_decode_paged_window", "mio_fa3_decode_window_route"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name)
        assert len(getattr(_lib.lib, name).argtypes) == 24
    assert _lib.lib.mio_version() == 106
    assert set(_lib.DECODE_ROUTES.values()) == {"head", "rows", "gqa"}
    for f in ("paged_attention_forward", "paged_attention_route"):
        assert callable(getattr(ops, f))


# (geometry, expected kernel): each side of dec_rows_ok / dec_gqa_ok
_ROUTES = [
    (dict(B=64, H=16, Hkv=16, D=64), "rows"),           # MHA, B >= 16, whole token rows of 2 KiB
    (dict(B=64, H=16, Hkv=16, D=80), "head"),           # D not 64 / 128
    (dict(B=4, H=16, Hkv=16, D=64), "head"),            # B < 8
    (dict(B=64, H=16, Hkv=16, D=128, q_len=2), "gqa"),  # two query vectors per key
    (dict(B=64, H=32, Hkv=8, D=128), "gqa"),            # GQA 4
    (dict(B=64, H=32, Hkv=8, D=64), "gqa"),
    (dict(B=4, H=32, Hkv=8, D=80), "head"),
    (dict(B=4, H=64, Hkv=2, D=128), "head"),            # 32 query vectors per key: past the 16 MFMA columns
    (dict(B=4, H=8, Hkv=8, D=128), "gqa"),              # one vector per key at D 128
    (dict(B=4, H=8, Hkv=8, D=64), "head"),              # ... not at D 64
]


@pytest.mark.parametrize("geom,want", _ROUTES)
@pytest.mark.parametrize("left", [-1, 0, 17, 4095, 1 << 20])
def test_decode_window_route(geom, want, left):
    assert _route(max_ctx=32768, max_blocks=2048, left=left, **geom) == want


def test_decode_window_route_sees_span():
    # B 8 streams its cache from HBM at ctx 32768 (1 GiB: whole-row kernel), but a 1024-key window of it fits the
    # Infinity Cache, where the per-head kernel wins: the heuristic must see the window span
    g = dict(B=8, H=16, Hkv=16, D=64, max_ctx=32768, max_blocks=2048)
    assert _route(**g) == "rows"
    assert _route(left=1023, **g) == "head"
    assert _route(left=32767, **g) == "rows"
    # the GQA kernel needs a context of at least one key: max_ctx 0 goes to the per-head kernel either way
    g = dict(B=4, H=32, Hkv=8, D=128, max_ctx=0)
    assert _route(**g) == _route(left=0, **g) == "head"


def test_decode_window_unbounded_equals_unwindowed_route():
    # (-1, -1) and a window no shorter than max_ctx: the route of the unwindowed launch
    for geom, _ in _ROUTES:
        assert _route(max_ctx=4096, **geom) == _route(max_ctx=4096, left=4096, **geom)


@pytest.mark.parametrize("fn", ["mio_fa3_decode_window_route", "mio_fa3_decode_paged_window"])
@pytest.mark.parametrize("left,right,msg", [(-2, -1, "window values"), (0, -2, "window values"),
                                            (16, 0, "no right window"), (-1, 5, "no right window"),
                                            (100, 100, "no right window")])
def test_decode_window_refusals_c(fn, left, right, msg):
    assert _route_rc(fn=fn, left=left, right=right) < 0
    assert msg in _err() and fn in _err()


def test_decode_window_route_argument_checks():
    assert _route_rc(left=5, D=12) < 0 and "head_dim" in _err()
    assert _route_rc(left=5, layer=1) < 0 and "layer_idx" in _err()
    assert _route_rc(left=5, H=6, Hkv=4) < 0 and "bad sizes" in _err()


@pytest.mark.parametrize("ws", [(-2, -1), (0, 0), (3, 7), (-1, 0), (1.5, -1), (1, 2, 3), 5, None])
def test_decode_window_refusals_ops(ws):
    from mio import ops
    # raised before anything looks at the (CPU) tensors
    t = torch.zeros(1)
    with pytest.raises(ValueError, match="window"):
        ops.paged_attention_forward(t, t, t, t, t, t, 16, 16, 0, window_size=ws)
    with pytest.raises(ValueError, match="window"):
        ops.paged_attention_route(t, t, t, t, t, t, 16, 16, 0, window_size=ws)


def test_windowed_decode_kernels_isa(tmp_path):
    """The windowed decode kernels exist for every unwindowed one, under their own names, with no scratch; the unit holds
    decode only (the cache writes are csrc/cache_write.hip's)."""
    text = _isa.device_isa(tmp_path, "decode_paged.hip", [], attention=False).read_text()
    assert not _isa.metadata(text, r"_Z\d+(reshape_and_cache|cache_write|rope_)\w+")
    for base in ("decode_paged", "decode_rows", "decode_gqa"):
        plain = _isa.metadata(text, rf"_Z\d+{base}_kernel\w+")
        win = _isa.metadata(text, rf"_Z\d+{base}_win_kernel\w+")
        assert len(plain) == 4 and len(win) == 4, base
        for blk in win:
            assert re.search(r"\.private_segment_fixed_size:\s+0\b", blk), blk
            assert re.search(r"\.vgpr_spill_count:\s+0\b", blk), blk

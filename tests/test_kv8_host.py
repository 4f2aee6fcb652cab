"""CPU-only tests of the fp8 (e4m3fn) paged KV cache's C ABI: the new symbols are bound and the ABI version is unchanged,
the host-only route query mio_fa3_decode_kv8_route picks the named kernel for the benchmark cases, the C-level refusals
carry their messages, and every fp8 decode kernel of csrc/decode_kv8.hip compiles without scratch (the unit holds decode only)."""
import ctypes as C
import re

import pytest

import _isa

ALIGNED = 1 << 20  # a fake 16-byte aligned device address: the route query dereferences nothing

KV8_SYMBOLS = {  # name -> number of C arguments
    "mio_reshape_and_cache_kv8": 19,
    "mio_reshape_and_cache_varlen_kv8": 22,
    "mio_fa3_decode_paged_kv8": 25,
    "mio_fa3_decode_kv8_route": 25,
}


def _route_rc(B=4, H=8, Hkv=2, q_len=1, D=128, bs=16, max_blocks=64, max_ctx=1024, left=-1, dtype=0, layers=1, layer=0,
              k_scale=ALIGNED, v_scale=ALIGNED, fn="mio_fa3_decode_kv8_route"):
    from mio import _lib
    qs = (C.c_int64 * 3)(H * q_len * D, q_len * D, D)
    os_ = (C.c_int64 * 3)(H * q_len * D, q_len * D, D)
    return getattr(_lib.lib, fn)(ALIGNED, ALIGNED, ALIGNED, ALIGNED, k_scale, v_scale, ALIGNED, ALIGNED, qs, os_, B, H,
                                 Hkv, q_len, D, layers, layer, bs, max_blocks, max_ctx, 0.125, left, dtype, None, None)


def _route(**kw):
    from mio import _lib
    r = _route_rc(**kw)
    return _lib.DECODE_ROUTES.get(r) if r >= 0 else None


def _err():
    from mio import _lib
    return _lib.lib.mio_last_error().decode()


def test_kv8_symbols_bound():
    from mio import _lib, ops
    for name, nargs in KV8_SYMBOLS.items():
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name), name
        assert len(getattr(_lib.lib, name).argtypes) == nargs, name
    assert _lib.lib.mio_version() == 106
    for f in ("paged_attention_forward", "paged_attention_route", "reshape_and_cache", "reshape_and_cache_varlen"):
        assert callable(getattr(ops, f))


# the issue's benchmark cases (tools/kv8_bench.py): geometry and the kernel it must take
KV8_CASES = {
    "a": (dict(B=64, H=16, Hkv=16, D=64, max_ctx=4096, bs=16), "rows"),
    "b": (dict(B=64, H=32, Hkv=4, D=128, max_ctx=4096, bs=16), "gqa"),
    "c": (dict(B=8, H=32, Hkv=8, D=128, max_ctx=32768, bs=64), "gqa"),
    "d": (dict(B=8, H=16, Hkv=16, D=64, max_ctx=4096, bs=16), "head"),  # 64 MiB of fp8 cache: Infinity-Cache resident
    "b_win": (dict(B=64, H=32, Hkv=4, D=128, max_ctx=32768, bs=16, left=4095), "gqa"),
}


@pytest.mark.parametrize("case", sorted(KV8_CASES))
def test_kv8_route_cases(case):
    geom, want = KV8_CASES[case]
    g = dict(geom)
    g["max_blocks"] = (g["max_ctx"] + g["bs"] - 1) // g["bs"]
    assert _route(**g) == want


def test_kv8_route_rules():
    # the rows kernel counts one-byte elements: half the bytes of the 16-bit cache
    g = dict(B=8, H=16, Hkv=16, D=64, max_blocks=2048, bs=16)
    assert _route(max_ctx=8192, **g) == "head"    # 128 MiB of fp8 cache (the 16-bit cache, 256 MiB, streams: rows)
    assert _route(max_ctx=32768, **g) == "rows"   # 512 MiB
    # a head row of D / 16 16-byte chunks: Hkv 2 x D 64 is 8 chunks per token row, below the rows kernel's 16
    assert _route(B=64, H=2, Hkv=2, D=64, max_ctx=4096, max_blocks=256) == "head"
    # head dims other than 64 / 128 take the per-head kernel
    for D in (16, 32, 48, 80, 96, 112):
        assert _route(B=64, H=32, Hkv=8, D=D, max_ctx=4096, max_blocks=256) == "head", D
    # q_len > 1 at MHA: query vectors share a key -> the matrix-core kernel
    assert _route(B=64, H=16, Hkv=16, D=128, q_len=2, max_ctx=4096, max_blocks=256) == "gqa"
    # a window shrinks the span the heuristics see
    w = dict(B=8, H=16, Hkv=16, D=64, max_ctx=65536, max_blocks=4096, bs=16)
    assert _route(**w) == "rows" and _route(left=1023, **w) == "head"


@pytest.mark.parametrize("fn", ["mio_fa3_decode_kv8_route", "mio_fa3_decode_paged_kv8"])
def test_kv8_decode_refusals_c(fn):
    assert _route_rc(fn=fn, k_scale=None) < 0 and "k_scale and v_scale are required" in _err() and fn in _err()
    assert _route_rc(fn=fn, v_scale=None) < 0 and "null scale pointer" in _err()
    assert _route_rc(fn=fn, k_scale=ALIGNED + 2) < 0 and "4-byte aligned" in _err()
    for D in (8, 24, 72, 120, 136):
        assert _route_rc(fn=fn, D=D) < 0 and "head_dim" in _err() and "multiple of 16" in _err(), D
    assert _route_rc(fn=fn, dtype=2) < 0 and "dtype" in _err() and "bf16 or fp16" in _err()
    assert _route_rc(fn=fn, left=-2) < 0 and "window_left" in _err()
    assert _route_rc(fn=fn, layer=1) < 0 and "layer_idx" in _err()


def _write_rc(fn, k_scale=ALIGNED, v_scale=ALIGNED, D=128, dtype=0):
    from mio import _lib
    st = (C.c_int64 * 2)(4 * D, D)
    f = getattr(_lib.lib, fn)
    if fn == "mio_reshape_and_cache_kv8":
        return f(ALIGNED, ALIGNED, ALIGNED, ALIGNED, k_scale, v_scale, ALIGNED, ALIGNED, st, st, 2, 4, D, 1, 0, 16, 4,
                 dtype, None)
    return f(ALIGNED, ALIGNED, ALIGNED, ALIGNED, k_scale, v_scale, ALIGNED, ALIGNED, ALIGNED, st, st, 2, 3, 4, D, 8, 1,
             0, 16, 4, dtype, None)


@pytest.mark.parametrize("fn", ["mio_reshape_and_cache_kv8", "mio_reshape_and_cache_varlen_kv8"])
def test_kv8_write_refusals_c(fn):
    # every refusal returns before a launch: nothing here reaches the fake addresses
    assert _write_rc(fn, k_scale=None) < 0 and "k_scale and v_scale are required" in _err() and fn in _err()
    assert _write_rc(fn, v_scale=None) < 0 and "null scale pointer" in _err()
    assert _write_rc(fn, D=72) < 0 and "head_dim must be a multiple of 16" in _err()
    assert _write_rc(fn, dtype=2) < 0 and "bf16 or fp16" in _err()


# the fp8 cache writes (cache_write_kernel / cache_write_varlen_kernel, two instantiations each) live in csrc/cache_write.hip:
# tests/test_rope_host.py::test_rope_kernels_isa holds them to the same checks
_KV8_KERNELS = ["decode_paged_kv8_kernel", "decode_paged_kv8_win_kernel", "decode_rows_kv8_kernel",
                "decode_rows_kv8_win_kernel", "decode_gqa_kv8_kernel", "decode_gqa_kv8_win_kernel"]


def test_kv8_kernels_isa(tmp_path):
    """Every fp8 decode kernel (plain and windowed, bf16 / fp16, both head-dim forms) exists, with no scratch and no spills;
    the matrix-core form reads V^T with the 8-bit transposed LDS read; the unit defines no cache-write kernel."""
    text = _isa.device_isa(tmp_path, "decode_kv8.hip", [], attention=False).read_text()
    for name in _KV8_KERNELS:
        blks = _isa.metadata(text, rf"_Z\d+{name}\w+")
        assert len(blks) == 4, name
        for blk in blks:
            _isa.check_fits_256(blk)
    # the 16-bit decode kernels' names are not reused (the ISA test of decode_paged.hip counts them by name)
    assert not _isa.metadata(text, r"_Z\d+decode_(paged|rows|gqa)_(win_)?kernel\w+")
    assert not _isa.metadata(text, r"_Z\d+(reshape_and_cache|cache_write|rope_)\w+")  # decode only: the writes are cache_write.hip's
    starts = [m.start() for m in re.finditer(r"^_Z\d+decode_gqa_kv8_kernel\w+:", text, re.M)]
    assert len(starts) == 4
    for a in starts:
        code = text[a:text.index(".Lfunc_end", a)]  # the whole kernel (its early exits end in s_endpgm too)
        assert "ds_read_b64_tr_b8" in code and "v_mfma_f32_16x16x32_" in code
        assert re.search(r"v_cvt_scalef32_pk_(bf16|f16)_fp8", code)
        assert "scratch_" not in code

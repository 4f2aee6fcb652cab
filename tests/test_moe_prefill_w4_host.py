"""The host side of the tall-input mixture-of-experts path on MXFP4 expert weights, without a GPU: the two C-ABI symbols are
declared, exported and bound; every refusal returns before a launch under the entry point's name; the empty calls return 0; the
compiled kernels use no scratch.  Addresses are fake and aligned; nothing is dereferenced."""
import os
import re

import pytest

A = 1 << 20  # a fake 16-byte aligned device address
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"mio_moe_prefill_up_w4": 27, "mio_moe_prefill_down_w4": 28}  # name -> number of C arguments
SWIGLU, FP16 = 5, 1


def _lib():
    from mio import _lib
    return _lib


def test_symbols_declared_and_bound():
    lib = _lib()
    header = open(os.path.join(ROOT, "include", "mio_hip.h")).read()
    for name, nargs in SYMBOLS.items():
        assert re.search(rf"\bint {name}\(", header), name
        assert name in lib.EXPORTS and len(getattr(lib.lib, name).argtypes) == nargs, name
    from mio import ops
    assert all(hasattr(ops, n) for n in ("moe_up_prefill_w4", "moe_down_prefill_w4", "moe_mlp_prefill_w4"))
    assert lib.lib.mio_version() == 106


# T 200, top_k 2, E 8, I 96, d 160 with their strides: a legal pair of calls
_UP = dict(x=A, w4_up=A, s_up=A, b_up=None, w4_gate=A, s_gate=A, b_gate=None, expert_offsets=A, sorted_rows=A, tile_expert=A, tile_row0=A,
           num_tiles=A, h=A, T=200, top_k=2, E=8, I=96, d=160, ldx=160, ldw=80, expert_stride=96 * 80, lds=8, scale_expert_stride=96 * 8,
           ldh=96, act=SWIGLU, dtype=0)
_DOWN = dict(h=A, w4_down=A, s_down=A, b_down=None, ids=A, weights=A, expert_offsets=A, row_pos=A, tile_expert=A, tile_row0=A, num_tiles=A,
             residual=None, y=A, workspace=A, T=200, top_k=2, E=8, d=160, I=96, ldh=96, ldw=48, expert_stride=160 * 48, lds=4,
             scale_expert_stride=160 * 4, ldy=160, ldr=0, dtype=0)
_CALLS = {"up": ("mio_moe_prefill_up_w4", _UP), "down": ("mio_moe_prefill_down_w4", _DOWN)}


@pytest.mark.parametrize("which,fault,words", [
    ("up", dict(d=144, ldx=144), "K must be a multiple of 32"), ("down", dict(I=80, ldh=80), "K must be a multiple of 32"),
    ("up", dict(dtype=FP16), "exact"), ("down", dict(dtype=FP16), "exact"),
    ("up", dict(ldw=88), "multiples of 16 bytes"), ("up", dict(ldw=64), "smaller than row length"),
    ("up", dict(lds=4), "lds at least K / 32"), ("down", dict(lds=2), "multiples of 4 bytes"),
    ("up", dict(scale_expert_stride=96 * 8 - 4), "scale_expert_stride smaller"),
    ("up", dict(s_gate=None), "w4_gate and s_gate"), ("up", dict(w4_gate=None), "w4_gate and s_gate"),
    ("up", dict(s_up=None), "s_up"), ("down", dict(s_down=None), "s_down"), ("up", dict(s_up=A + 2), "4-byte"),
    ("up", dict(T=8193), "T must be at most 8192"), ("down", dict(T=8193), "T must be at most 8192"),
    ("up", dict(num_tiles=None), "non-null"), ("down", dict(workspace=None), "workspace required"),
])
def test_refusals(which, fault, words):
    """Each fault is the only thing wrong with a legal call."""
    lib = _lib().lib
    name, call = _CALLS[which]
    assert getattr(lib, name)(*dict(call, **fault).values(), None) != 0
    err = lib.mio_last_error().decode()
    assert err.startswith(name + ": ") and words in err, err


def test_empty_calls_return_zero():
    lib = _lib().lib
    for name, call in _CALLS.values():
        n = "I" if name.endswith("up_w4") else "d"
        for empty in (dict(T=0), {n: 0}):
            assert getattr(lib, name)(*dict(call, **empty).values(), None) == 0, lib.mio_last_error().decode()
    assert lib.mio_moe_prefill_down_w4(*dict(_DOWN, T=0, workspace=None).values(), None) == 0


def test_kernels_fit_256_vgprs_without_scratch(tmp_path):
    """The compiled unit's kernel metadata under its Makefile flags: the three instances of the grouped GEMM (up SwiGLU, up plain,
    down) use no scratch, spill nothing and stay within 256 VGPRs."""
    import _isa
    text = _isa.device_isa(tmp_path, "moe_prefill_w4.hip", [], attention=False, extra_flags=_isa.NO_PACKED_FP32_FLAGS).read_text()
    blocks = _isa.metadata(text, r"_Z26moe_prefill_w4_gemm_kernel\w+")
    assert len(blocks) == 3, len(blocks)
    for blk in blocks:
        _isa.check_fits_256(blk)

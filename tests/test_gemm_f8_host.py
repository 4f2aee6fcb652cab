"""CPU-only tests of the host side of the FP8 x FP8 GEMM, through the loaded library: the C-ABI symbols are declared and bound; every
refusal of mio_gemm_f8 returns before a launch with a message under the entry point's name; mio_gemm_f8_route names a route for
each shape of the GPU table.  Addresses are fake and 16-byte aligned; nothing is dereferenced."""
import os
import re

import pytest

A = 1 << 20  # a fake 16-byte aligned device address
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWIGLU = 5


def _lib():
    from mio import _lib
    return _lib


def test_symbols_declared_and_bound():
    lib = _lib()
    header = open(os.path.join(ROOT, "include", "mio_hip.h")).read()
    for name, nargs in {"mio_gemm_f8": 20, "mio_gemm_f8_ok": 4, "mio_gemm_f8_route": 4}.items():
        assert re.search(rf"\b(int|const char\*) {name}\(", header), name
        assert name in lib.EXPORTS and hasattr(lib.lib, name), name
        assert len(getattr(lib.lib, name).argtypes) == nargs, name


# a legal call (M 300, N 520, K 1040): every fault below is the only thing wrong with it
_G = dict(x8=A, ldx=1040, x_scale=A, w8=A, ldw=1040, w_scale=A, bias=None, w8_gate=None, w_scale_gate=None, bias_gate=None,
          residual=None, ldr=0, y=A, ldy=520, M=300, N=520, K=1040, act=0, out_dtype=0)


@pytest.mark.parametrize("fault,words", [
    (dict(K=1032, ldx=1040, ldw=1040), "K must be a multiple of 16"),
    (dict(x8=A + 8), "16-byte aligned"), (dict(w8=A + 4), "16-byte aligned"), (dict(y=A + 2), "16-byte aligned"),
    (dict(residual=A + 8, ldr=520), "16-byte aligned"), (dict(x_scale=A + 2), "4-byte aligned"), (dict(bias=A + 1), "2-byte aligned"),
    (dict(ldx=1048), "multiples of 16 bytes"), (dict(ldw=1048), "multiples of 16 bytes"), (dict(ldy=524), "multiples of 8"),
    (dict(residual=A, ldr=524), "multiples of 8"), (dict(ldx=1024), "smaller than row length"), (dict(ldy=512), "smaller than row length"),
    (dict(w8_gate=A, w_scale_gate=A), "iff act == SWIGLU"), (dict(w8_gate=A), "iff act == SWIGLU"),
    (dict(act=SWIGLU), "iff act == SWIGLU"), (dict(act=SWIGLU, w8_gate=A), "iff act == SWIGLU"), (dict(bias_gate=A), "bias_gate"),
    (dict(act=6), "unknown activation"), (dict(act=-1), "unknown activation"), (dict(out_dtype=2), "bf16 or fp16"),
    (dict(M=-1), "negative"), (dict(N=-8), "negative"), (dict(K=-16), "negative"),
    (dict(x8=None), "non-null"), (dict(x_scale=None), "non-null"), (dict(w_scale=None), "non-null"), (dict(y=None), "non-null"),
])
def test_refusals(fault, words):
    lib = _lib().lib
    assert lib.mio_gemm_f8(*dict(_G, **fault).values(), None) != 0
    err = lib.mio_last_error().decode()
    assert err.startswith("mio_gemm_f8: ") and words in err, err


def test_route_names_the_gpu_table_and_empty_calls_return():
    lib = _lib().lib
    from mio import ops
    for M, N, K in [(1, 8, 16), (16, 16, 128), (17, 24, 144), (255, 264, 384), (257, 248, 384), (300, 520, 1040), (257, 264, 400),
                    (64, 1032, 1040), (32768, 3072, 1024), (1 << 33, 8, 0)]:
        assert ops.gemm_f8_route(M, N, K) == "f8_t256x256" and ops.gemm_f8_route(M, N, K, "swiglu") == "f8_glu_t256x128"
    assert ops.gemm_f8_route(0, 8, 16) == "empty" and ops.gemm_f8_route(8, 0, 16, "gelu") == "empty"
    with pytest.raises(ValueError, match="mio_gemm_f8_route: K must be a multiple of 16"):
        ops.gemm_f8_route(300, 520, 1032)
    assert lib.mio_gemm_f8(*dict(_G, M=0, x8=None, y=None).values(), None) == 0  # an empty call launches nothing
    assert not ops.gemm_f8_ok(300, 520, 1032) and not ops.gemm_f8_ok(-1, 8, 16) and not ops.gemm_f8_ok(300, 520, 1040, "tanh")
    # the advice: the shapes profiles/gemm_f8.md measured under 0.9, and none of those that lost or were not measured
    assert ops.gemm_f8_ok(32768, 4096, 1024, "swiglu") and ops.gemm_f8_ok(8192, 14336, 4096, "swiglu")
    assert not any(ops.gemm_f8_ok(32768, N, K, a) for N, K, a in ((3072, 1024, "none"), (1024, 4096, "none"), (4096, 1024, "gelu")))
    assert not ops.gemm_f8_ok(8192, 4096, 14336) and not ops.gemm_f8_ok(32769, 4096, 1024, "swiglu")

"""CPU-only tests of the host side of the MXFP4 decode GEMM and MoE step, through the loaded library: the C-ABI symbols are
declared, exported and bound; every refusal returns before a launch under the entry point's name; the plan's slices are whole
128-k steps of at least 32 M that cover K; the advice admits nothing unmeasured.  Addresses are fake and aligned; nothing is
dereferenced."""
import ctypes as C
import os
import re

import pytest

A = 1 << 20  # a fake 16-byte aligned device address
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"mio_weight_quant_mxfp4": 10, "mio_gemm_skinny_w4_workspace_bytes": 4, "mio_gemm_skinny_w4_splits": 4,
           "mio_gemm_skinny_w4_slice": 7, "mio_gemm_skinny_w4_chunk_k": 1, "mio_gemm_skinny_w4_depth": 1, "mio_gemm_skinny_w4_ok": 4,
           "mio_gemm_skinny_w4": 21, "mio_moe_up_w4_splits": 6, "mio_moe_up_w4_workspace_bytes": 6, "mio_moe_down_w4_splits": 5,
           "mio_moe_down_w4_workspace_bytes": 5, "mio_moe_up_w4": 25, "mio_moe_down_w4": 25}  # name -> number of C arguments
SWIGLU, FP16 = 5, 1


def _lib():
    from mio import _lib
    return _lib


def _err():
    return _lib().lib.mio_last_error().decode()


def test_symbols_declared_and_bound():
    lib = _lib()
    header = open(os.path.join(ROOT, "include", "mio_hip.h")).read()
    for name, nargs in SYMBOLS.items():
        assert re.search(rf"\b(int|size_t) {name}\(", header), name
        assert name in lib.EXPORTS and hasattr(lib.lib, name), name
        assert len(getattr(lib.lib, name).argtypes) == nargs, name


# a legal call that splits K (M 4, N 1024, K 1024): every fault below is the only thing wrong with it
_G = dict(x=A, w4=A, w_scale=A, bias=None, w4_gate=None, w_scale_gate=None, bias_gate=None, residual=None, y=A, workspace=A, M=4,
          N=1024, K=1024, ldx=1024, ldw=512, lds=32, ldy=1024, ldr=0, act=0, dtype=0)


@pytest.mark.parametrize("fault,words", [
    (dict(K=1040, ldx=1040, ldw=528, lds=36), "K must be a multiple of 32"),
    (dict(dtype=FP16), "dtype must be bf16"),
    (dict(ldw=496), "ldw smaller than K / 2"), (dict(ldw=520), "ldw must be a multiple of 16 bytes"),
    (dict(lds=34), "lds must be a multiple of 4"), (dict(lds=28), "lds must be a multiple of 4 bytes and at least K / 32"),
    (dict(M=65), "at most 64"),
    (dict(act=SWIGLU, w4_gate=A), "w4_gate and w_scale_gate"), (dict(act=SWIGLU, w_scale_gate=A), "w4_gate and w_scale_gate"),
    (dict(w_scale_gate=A), "w4_gate and w_scale_gate"), (dict(act=SWIGLU), "w4_gate and w_scale_gate"),
    (dict(w_scale=None), "non-null"), (dict(w_scale=A + 2), "4-byte"), (dict(w4=A + 8), "16-byte aligned"),
    (dict(workspace=None), "workspace required"),
])
def test_gemm_refusals(fault, words):
    lib = _lib().lib
    assert lib.mio_gemm_skinny_w4_splits(_G["M"], _G["N"], _G["K"], 0) > 1  # the neighbour is a legal call that splits
    assert lib.mio_gemm_skinny_w4(*dict(_G, **fault).values(), None) != 0
    assert _err().startswith("mio_gemm_skinny_w4: ") and words in _err(), _err()


def test_fp16_refusal_says_why_and_empty_calls_return():
    lib = _lib().lib
    assert lib.mio_gemm_skinny_w4(*dict(_G, dtype=FP16).values(), None) != 0 and "exact" in _err()
    for empty in (dict(M=0), dict(N=0, ldy=8)):
        assert lib.mio_gemm_skinny_w4(*dict(_G, **empty).values(), None) == 0, _err()
    assert lib.mio_gemm_skinny_w4_splits(4, 1024, 0, 0) == 1  # K 0: an empty sum in one slice


_Q = dict(w=A, ldw=1024, w4=A, ldw4=512, scale=A, lds=32, N=64, K=1024, dtype=0)


@pytest.mark.parametrize("fault,words", [
    (dict(K=1040, ldw=1040, ldw4=528, lds=36), "multiple of 32"), (dict(dtype=2), "bf16 or fp16"), (dict(ldw=1016), "ldw must be"),
    (dict(ldw4=504), "ldw4 must be"), (dict(ldw4=496), "ldw4 must be"), (dict(lds=31), "lds must be"), (dict(scale=None), "non-null"),
    (dict(w4=A + 4), "16-byte aligned"),
])
def test_quantiser_refusals(fault, words):
    assert _lib().lib.mio_weight_quant_mxfp4(*dict(_Q, **fault).values(), None) != 0
    assert _err().startswith("mio_weight_quant_mxfp4: ") and words in _err(), _err()


# T 4, top_k 2, E 8, I 96, d 160 with their strides: a legal pair of calls
_UP = dict(x=A, w4_up=A, s_up=A, b_up=None, w4_gate=A, s_gate=A, b_gate=None, expert_offsets=A, sorted_rows=A, h=A, workspace=A, T=4,
           top_k=2, E=8, I=96, d=160, ldx=160, ldw=80, expert_stride=96 * 80, lds=8, scale_expert_stride=96 * 8, ldh=96, act=SWIGLU, dtype=0)
_DOWN = dict(h=A, w4_down=A, s_down=A, b_down=None, ids=A, weights=A, expert_offsets=A, row_pos=A, residual=None, y=A, workspace=A,
             T=4, top_k=2, E=8, d=160, I=96, ldh=96, ldw=48, expert_stride=160 * 48, lds=4, scale_expert_stride=160 * 4, ldy=160, ldr=0,
             dtype=0)


@pytest.mark.parametrize("fault,words", [
    (dict(d=144, ldx=144), "K must be a multiple of 32"), (dict(dtype=FP16), "exact"), (dict(T=65), "at most 64"),
    (dict(ldw=64), "smaller than row length"), (dict(ldw=88), "multiples of 16 bytes"),
    (dict(lds=6), "multiples of 4 bytes"), (dict(lds=4), "lds at least K / 32"), (dict(scale_expert_stride=96 * 8 - 4), "scale_expert_stride smaller"),
    (dict(s_gate=None), "w4_gate and s_gate"), (dict(w4_gate=None), "w4_gate and s_gate"), (dict(s_up=None), "s_up"),
    (dict(s_up=A + 2), "4-byte"),
])
def test_moe_up_refusals(fault, words):
    assert _lib().lib.mio_moe_up_w4(*dict(_UP, **fault).values(), None) != 0
    assert _err().startswith("mio_moe_up_w4: ") and words in _err(), _err()


@pytest.mark.parametrize("fault,words", [
    (dict(I=80, ldh=80), "K must be a multiple of 32"), (dict(dtype=FP16), "exact"), (dict(ldw=32), "smaller than row length"),
    (dict(lds=2), "multiples of 4 bytes"), (dict(scale_expert_stride=160 * 4 - 4), "scale_expert_stride smaller"),
    (dict(s_down=None), "s_down"), (dict(workspace=None), "workspace required"),
])
def test_moe_down_refusals(fault, words):
    assert _lib().lib.mio_moe_down_w4(*dict(_DOWN, **fault).values(), None) != 0
    assert _err().startswith("mio_moe_down_w4: ") and words in _err(), _err()


@pytest.mark.parametrize("M", [1, 5, 16, 37, 64])
@pytest.mark.parametrize("act", [0, SWIGLU])
def test_plan_slices(M, act):
    """Slices are whole 128-k steps (the last ends at K), each at least 32 M long where K is split, they cover [0, K) in order, the
    workspace follows the count, and the advice admits only the region profiles/skinny_gemm_w4.md lists."""
    lib = _lib().lib
    kb, ke = C.c_int32(), C.c_int32()
    for N in (1, 72, 1000, 14336):
        for K in (0, 32, 160, 2880, 4096, 14336):
            n = lib.mio_gemm_skinny_w4_splits(M, N, K, act)
            assert n >= 1 and lib.mio_gemm_skinny_w4_workspace_bytes(M, N, K, act) == (0 if n == 1 else n * M * N * 4 * (2 if act else 1))
            end = 0
            for s in range(n):
                assert lib.mio_gemm_skinny_w4_slice(M, N, K, act, s, C.byref(kb), C.byref(ke)) == 0
                assert kb.value == end and kb.value % 128 == 0 and (ke.value % 128 == 0 or ke.value == K)
                assert n == 1 or ke.value - kb.value >= 32 * M
                end = ke.value
            assert end == K
            listed = act == SWIGLU and M <= 16 and N * K >= 14336 * 4096  # (the one region of profiles/skinny_gemm_w4.md)
            assert lib.mio_gemm_skinny_w4_ok(M, N, K, act) == int(listed and K > 0)
    assert lib.mio_gemm_skinny_w4_chunk_k(act) % 128 == 0 and lib.mio_gemm_skinny_w4_depth(act) >= 2

"""CPU-only tests of the attention forward over an fp8 (e4m3fn) paged KV cache (mio_fa3_fwd_paged_kv8): the C-ABI symbols
are bound and declared, the ABI version is unchanged, the host-only route query reports the kernel family and every
refusal without a GPU, ops.fa3_paged_route takes fp8 CPU tensors, and the kernels of csrc/fa3_kv8_inst.hip pass the ISA
soundness checks of the 16-bit paged kernels."""
import ctypes as C
import os
import re

import pytest
import torch

import _isa
from test_paged_host import ALIGNED, _params

F8 = torch.float8_e4m3fn
NEW = ("mio_fa3_fwd_paged_kv8", "mio_fa3_paged_kv8_route")


def _rc(k_scale=ALIGNED, v_scale=ALIGNED, left=-1, right=-1, **kw):
    from mio import _lib
    kw.setdefault("causal", 0 if right > 0 else 1)
    return _lib.lib.mio_fa3_paged_kv8_route(C.byref(_params(**kw)), k_scale, v_scale, left, right)


def _route(**kw):
    from mio import _lib
    r = _rc(**kw)
    return _lib.FA3_PAGED_ROUTES.get(r) if r >= 0 else None


def _err():
    from mio import _lib
    return _lib.lib.mio_last_error().decode()


def test_kv8_prefill_symbols_bound_and_declared():
    from mio import _lib, ops
    header = open(os.path.join(_isa.ROOT, "include", "mio_hip.h")).read()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name)
        assert re.search(rf"\b{name}\(", header), f"{name} is not declared in mio_hip.h"
    assert _lib.lib.mio_fa3_fwd_paged_kv8.argtypes[0] == C.POINTER(_lib.FaPagedParams)
    assert len(_lib.lib.mio_fa3_fwd_paged_kv8.argtypes) == 6
    assert len(_lib.lib.mio_fa3_paged_kv8_route.argtypes) == 5
    assert _lib.lib.mio_version() == 106
    assert set(_lib.FA3_PAGED_ROUTES.values()) == {"empty", "fwd5", "fwd3"}
    assert callable(ops.flash_attention_varlen_paged)


@pytest.mark.parametrize("D", [16, 32, 48, 64, 80, 96, 112, 128])
def test_kv8_prefill_route_by_head_dim(D):
    want = "fwd5" if D <= 64 else "fwd3"
    assert _route(D=D) == want
    assert _route(D=D, left=100, right=0) == want
    assert _route(D=D, left=64, right=32, causal=0) == want
    assert _route(D=D, total_q=0) == "empty" and _route(D=D, B=0) == "empty"


@pytest.mark.parametrize("kw,msg", [
    (dict(k_scale=None), "null scale"),
    (dict(v_scale=None), "null scale"),
    (dict(k_scale=ALIGNED + 2), "4-byte aligned"),
    (dict(D=72), "multiple of 16"),
    (dict(D=40), "multiple of 16"),
    (dict(D=136), "head_dim"),
    (dict(block_size=32), "block_size"),
    (dict(block_size=96), "block_size"),
    (dict(left=-2), "window"),
    (dict(left=10, right=5, causal=1), "causal"),
    (dict(layer_idx=2), "layer_idx"),
    (dict(layer_idx=-1), "layer_idx"),
    (dict(Hkv=3, H=4), "multiple"),
    (dict(dtype=3), "dtype"),
    (dict(num_blocks=1 << 20, num_layers=64, block_size=128), "2^32"),
])
def test_kv8_prefill_refusals(kw, msg):
    """Every refusal is reported by the route query and by the launch itself, before anything is launched."""
    from mio import _lib
    assert _rc(**kw) < 0
    assert msg in _err(), _err()
    k_scale, v_scale = kw.pop("k_scale", ALIGNED), kw.pop("v_scale", ALIGNED)
    left, right = kw.pop("left", -1), kw.pop("right", -1)
    kw.setdefault("causal", 0 if right > 0 else 1)
    rc = _lib.lib.mio_fa3_fwd_paged_kv8(C.byref(_params(**kw)), k_scale, v_scale, left, right, None)
    assert rc != 0 and msg in _err(), _err()


def test_kv8_prefill_ops_route_cpu():
    """ops.fa3_paged_route on fp8 CPU tensors: the family of the head dim; the scale rules of decode."""
    from mio import ops
    bt = torch.zeros(2, 4, dtype=torch.int32)
    cu = torch.tensor([0, 100, 300], dtype=torch.int32)
    sk = torch.tensor([150, 300], dtype=torch.int32)
    one = torch.ones(1)
    for D, want in ((16, "fwd5"), (64, "fwd5"), (80, "fwd3"), (128, "fwd3")):
        q = torch.zeros(300, 4, D, dtype=torch.bfloat16)
        kc = torch.zeros(8, 2, 64, 2, D, dtype=F8)
        assert ops.fa3_paged_route(q, kc, kc, bt, cu, sk, 200, 300, k_scale=one, v_scale=one) == want
        assert ops.fa3_paged_route(q, kc, kc, bt, cu, sk, 200, 300, causal=True, window_size=(64, 0),
                                   k_scale=torch.ones(2), v_scale=torch.ones(2), layer_idx=1) == want
    q = torch.zeros(300, 4, 64, dtype=torch.float16)
    kc = torch.zeros(8, 2, 64, 2, 64, dtype=F8)
    with pytest.raises(ValueError, match="requires k_scale and v_scale"):
        ops.fa3_paged_route(q, kc, kc, bt, cu, sk, 200, 300)
    with pytest.raises(ValueError, match="num_layers"):
        ops.fa3_paged_route(q, kc, kc, bt, cu, sk, 200, 300, k_scale=torch.ones(3), v_scale=one)
    with pytest.raises(ValueError, match="float32"):
        ops.fa3_paged_route(q, kc, kc, bt, cu, sk, 200, 300, k_scale=one.double(), v_scale=one)
    with pytest.raises(ValueError, match="e4m3fn"):
        ops.fa3_paged_route(q, kc.view(torch.float8_e5m2), kc.view(torch.float8_e5m2), bt, cu, sk, 200, 300,
                            k_scale=one, v_scale=one)
    with pytest.raises(ValueError, match="e4m3fn"):
        ops.fa3_paged_route(q, kc.view(torch.uint8), kc.view(torch.uint8), bt, cu, sk, 200, 300, k_scale=one,
                            v_scale=one)
    k16 = torch.zeros(8, 2, 64, 2, 64, dtype=torch.float16)
    with pytest.raises(ValueError, match="fp8"):
        ops.fa3_paged_route(q, k16, k16, bt, cu, sk, 200, 300, k_scale=one, v_scale=one)
    assert ops.fa3_paged_route(q, k16, k16, bt, cu, sk, 200, 300) == "fwd5"  # the 16-bit path as before
    q40 = torch.zeros(300, 4, 40, dtype=torch.float16)
    k40 = torch.zeros(8, 2, 64, 2, 40, dtype=F8)
    with pytest.raises(ValueError, match="multiple of 16"):
        ops.fa3_paged_route(q40, k40, k40, bt, cu, sk, 200, 300, k_scale=one, v_scale=one)


@pytest.mark.parametrize("type_id", [0, 1])
@pytest.mark.parametrize("D", [64, 96, 128])
def test_kv8_prefill_kernels_isa(tmp_path, type_id, D):
    """Plain and windowed, causal and full: four kernels per object.  The fwd5 forms keep two waves per SIMD (no scratch,
    at most 256 VGPRs); the fwd3 forms leave the asm-owned accumulator registers alone; all widen with
    v_cvt_scalef32_pk_*_fp8."""
    text = _isa.fa_isa(tmp_path, "fa3_kv8_inst.hip", type_id, D)
    assert "scratch_" not in text
    cvt = "bf16" if type_id == 0 else "f16"
    if D == 64:
        blks = _isa.metadata(text, r"_Z\d+fa3_fwd5_paged_kv8\w*kernel\w+")
        assert len(blks) == 4
        for blk in blks:
            _isa.check_fits_256(blk)
        bodies = _isa.kernels(text, r"_Z\d+fa3_fwd5_paged_kv8")
    else:
        bodies = _isa.kernels(text, r"_Z\d+fa3_fwd3_paged_kv8")
        assert len(bodies) == 4
        for body in bodies:
            _isa.check_agpr(tmp_path, body, _isa.fa3_agpr_floor(D))
        for blk in _isa.metadata(text, r"_Z\d+fa3_fwd3_paged_kv8\w*kernel\w+"):
            assert re.search(r"\.private_segment_fixed_size:\s+0\b", blk), blk
    assert len(bodies) == 4
    assert re.search(rf"v_cvt_scalef32_pk_{cvt}_fp8", text)

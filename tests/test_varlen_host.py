"""CPU-only tests of the packed variable-length attention forward (mio_fa3_fwd_varlen): the C-ABI symbols are bound, the
route table and every refusal are reported without a GPU, the varlen kernels pass the same ISA soundness checks as the dense
pipelined kernels, and unpad_input / pad_input round-trip."""
import ctypes as C

import pytest
import torch

import _isa

ALIGNED = 1 << 20  # a fake 16-byte aligned device address: nothing is dereferenced by the route query


def _params(B=3, total_q=600, total_k=600, max_q=300, max_k=300, H=4, Hkv=4, D=64, dtype=0, causal=1, cu=True,
            tok_stride=None, head_stride=None, ptr_off=0):
    from mio import _lib
    p = _lib.FaVarlenParams()
    p.q = ALIGNED + ptr_off
    p.k, p.v, p.o = ALIGNED, ALIGNED, ALIGNED
    p.cu_seqlens_q = p.cu_seqlens_k = (ALIGNED if cu else None)
    ts = H * D if tok_stride is None else tok_stride
    hs = D if head_stride is None else head_stride
    for st in (p.q_stride, p.o_stride):
        st[0], st[1] = ts, hs
    for st in (p.k_stride, p.v_stride):
        st[0], st[1] = (Hkv * D if tok_stride is None else tok_stride), hs
    p.B, p.total_q, p.total_k, p.max_seqlen_q, p.max_seqlen_k = B, total_q, total_k, max_q, max_k
    p.H, p.Hkv, p.D, p.dtype, p.causal, p.softmax_scale = H, Hkv, D, dtype, causal, 0.125
    return p


def _route(**kw):
    from mio import _lib
    r = _lib.lib.mio_fa3_varlen_route(C.byref(_params(**kw)))
    return _lib.FA3_VARLEN_ROUTES.get(r) if r >= 0 else None


def test_varlen_symbols_bound():
    from mio import _lib, ops
    for name in ("mio_fa3_fwd_varlen", "mio_fa3_varlen_route"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name)
    assert _lib.lib.mio_fa3_varlen_route.argtypes == [C.POINTER(_lib.FaVarlenParams)]
    assert set(_lib.FA3_VARLEN_ROUTES.values()) == {"empty", "fwd5", "fwd3"}
    # the dense route table stays mio_fa3_fwd's alone
    assert set(_lib.FA3_ROUTES) == set(range(10))
    for f in ("flash_attention_varlen", "fa3_varlen_route", "unpad_input", "pad_input"):
        assert callable(getattr(ops, f))


# (geometry, expected route or None = refused, substring of the error)
_VARLEN_TABLE = [
    (dict(D=8), "fwd5", None),
    (dict(D=64), "fwd5", None),
    (dict(D=72), "fwd3", None),
    (dict(D=96), "fwd3", None),
    (dict(D=104), "fwd3", None),
    (dict(D=128), "fwd3", None),
    (dict(D=128, causal=0, dtype=1), "fwd3", None),
    (dict(total_q=0, max_q=0), "empty", None),
    (dict(B=0, cu=False), "empty", None),
    (dict(total_k=0, max_k=0), "fwd5", None),            # every sequence without keys: launched, writes the empty rows
    (dict(D=136), None, b"head_dim"),
    (dict(D=60), None, b"head_dim"),
    (dict(H=6, Hkv=4), None, b"multiple of Hkv"),
    (dict(ptr_off=8), None, b"aligned"),
    (dict(tok_stride=4 * 64 + 4), None, b"strides"),
    (dict(head_stride=68), None, b"strides"),
    (dict(tok_stride=-256), None, b"strides"),
    (dict(cu=False), None, b"cu_seqlens"),
    (dict(max_q=0), None, b"max_seqlen_q"),
    (dict(max_k=0), None, b"max_seqlen_k"),
    (dict(dtype=2), None, b"dtype"),
    (dict(B=-1), None, b"sizes"),
    # K / V rows of one sequence within 4 GiB: max_seqlen_k * token stride * 2 < 2^32
    (dict(max_k=(1 << 31) // 4096 - 1, tok_stride=4096), "fwd5", None),
    (dict(max_k=(1 << 31) // 4096, tok_stride=4096), None, b"4 GiB"),
]


@pytest.mark.parametrize("geom,want,err", _VARLEN_TABLE)
def test_varlen_route_table_without_gpu(geom, want, err):
    from mio import _lib
    got = _route(**geom)
    assert got == want, f"{geom}: route {got}, expected {want}"
    if want is None:
        assert err in _lib.lib.mio_last_error(), _lib.lib.mio_last_error()


def test_varlen_argument_errors_without_gpu():
    """mio_fa3_fwd_varlen refuses what the route query refuses, before any launch; ops raises before it calls the library."""
    from mio import _lib, ops
    assert _lib.lib.mio_fa3_fwd_varlen(None, None) != 0 and b"null" in _lib.lib.mio_last_error()
    assert _lib.lib.mio_fa3_varlen_route(None) < 0
    assert _lib.lib.mio_fa3_fwd_varlen(C.byref(_params(D=136)), None) != 0 and b"head_dim" in _lib.lib.mio_last_error()
    assert _lib.lib.mio_fa3_fwd_varlen(C.byref(_params(cu=False)), None) != 0
    # nothing to do: no launch, success
    assert _lib.lib.mio_fa3_fwd_varlen(C.byref(_params(total_q=0, max_q=0)), None) == 0
    q = torch.zeros(600, 4, 64, dtype=torch.bfloat16)
    cu = torch.tensor([0, 300, 600], dtype=torch.int32)
    assert ops.fa3_varlen_route(q, q, q, cu, cu, 300, 300, causal=True) == "fwd5"
    assert ops.fa3_varlen_route(q[:, :, :40], q[:, :1, :40], q[:, :1, :40], cu, cu, 300, 300) == "fwd5"
    qkv = torch.zeros(600, 3, 2, 96, dtype=torch.float16)  # strided views of one fused projection
    assert ops.fa3_varlen_route(qkv[:, 0], qkv[:, 1], qkv[:, 2], cu, cu, 300, 300) == "fwd3"
    assert ops.fa3_varlen_route(q[:0], q, q, cu[:1], cu[:1], 0, 300) == "empty"
    with pytest.raises(ValueError):  # CPU tensors: no fallback
        ops.flash_attention_varlen(q, q, q, cu, cu, 300, 300)
    with pytest.raises(ValueError):
        ops.fa3_varlen_route(q, q, q, cu.long(), cu, 300, 300)
    with pytest.raises(ValueError):
        ops.fa3_varlen_route(q, q, q, cu, cu[:2], 300, 300)
    with pytest.raises(ValueError):
        ops.fa3_varlen_route(q[None], q, q, cu, cu, 300, 300)
    with pytest.raises(ValueError):
        ops.fa3_varlen_route(q.float(), q.float(), q.float(), cu, cu, 300, 300)
    with pytest.raises(RuntimeError):
        ops.fa3_varlen_route(q, q, q, cu, cu, 0, 300)


@pytest.mark.parametrize("type_id", [0, 1])
def test_fwd5_varlen_fits_without_spills(tmp_path, type_id):
    """The varlen form of fa3_fwd5_kernel runs two waves per SIMD like the dense one: no scratch, at most 256 VGPRs."""
    text = _isa.fa_isa(tmp_path, "fa3_seq_inst.hip", type_id, 64)
    blocks = _isa.metadata(text, r"_Z22fa3_fwd5_varlen_kernel\w+")
    assert len(blocks) == 2, "causal and full instantiations expected"
    for blk in blocks:
        _isa.check_fits_256(blk)
    assert "scratch_" not in text


@pytest.mark.parametrize("type_id,D", [(0, 96), (1, 96), (0, 128), (1, 128)])
def test_fwd3_varlen_accumulator_registers_untouched_by_compiler(tmp_path, type_id, D):
    """The varlen form of fa3_fwd3_kernel owns the same accumulator registers (Fa3Map<D>::A_Q and up) through inline asm:
    no compiler-generated instruction may touch them (tools/check_agpr.py), and nothing spills."""
    bodies = _isa.kernels(_isa.fa_isa(tmp_path, "fa3_seq_inst.hip", type_id, D), "_Z22fa3_fwd3_varlen_kernel")
    assert len(bodies) == 2, "causal and full instantiations expected"
    for body in bodies:
        _isa.check_agpr(tmp_path, body, _isa.fa3_agpr_floor(D))


def test_unpad_pad_round_trip():
    from mio import ops
    g = torch.Generator().manual_seed(0)
    B, S = 4, 37
    x = torch.randn(B, S, 3, 8, generator=g)
    keep = torch.zeros(B, S, dtype=torch.bool)
    keep[0, 5:] = True      # left padding
    keep[1, :20] = True     # right padding
    keep[2] = True          # none
    # keep[3]: an empty sequence
    xp, idx, cu, ms = ops.unpad_input(x, keep)
    lens = keep.sum(1)
    assert xp.shape == (int(lens.sum()), 3, 8) and idx.dtype == torch.int64
    assert cu.dtype == torch.int32 and cu.tolist() == [0] + torch.cumsum(lens, 0).tolist() and ms == S
    assert torch.equal(xp, x[keep])
    y = ops.pad_input(xp, idx, B, S)
    assert torch.equal(y, torch.where(keep[..., None, None], x, torch.zeros_like(x)))
    with pytest.raises(ValueError):
        ops.unpad_input(x, keep[:, :5])

"""CPU-only tests of the attention forward over the paged KV cache (mio_fa3_fwd_paged) and of the many-token cache write
(mio_reshape_and_cache_varlen): the C-ABI symbols are bound, the route table and every refusal are reported without a GPU,
ops raises on bad arguments before it calls the library (every ValueError of the cache writes' shared argument builder by its
text), and the paged kernels pass the ISA soundness checks of the dense pipelined kernels."""
import ctypes as C

import pytest
import torch

import _isa

ALIGNED = 1 << 20  # a fake 16-byte aligned device address: nothing is dereferenced by the route query


def _params(B=3, total_q=600, max_q=300, max_k=1000, H=4, Hkv=4, D=64, dtype=0, causal=1, tables=True, num_blocks=64,
            num_layers=2, layer_idx=0, block_size=64, max_blocks=16, tok_stride=None, head_stride=None, ptr_off=0):
    from mio import _lib
    p = _lib.FaPagedParams()
    p.q = ALIGNED + ptr_off
    p.k_cache, p.v_cache, p.o = ALIGNED, ALIGNED, ALIGNED
    p.cu_seqlens_q = p.seqused_k = p.block_tables = (ALIGNED if tables else None)
    for st in (p.q_stride, p.o_stride):
        st[0], st[1] = (H * D if tok_stride is None else tok_stride), (D if head_stride is None else head_stride)
    p.B, p.total_q, p.max_seqlen_q, p.max_seqlen_k = B, total_q, max_q, max_k
    p.H, p.Hkv, p.D, p.dtype, p.causal, p.softmax_scale = H, Hkv, D, dtype, causal, 0.125
    p.num_blocks, p.num_layers, p.layer_idx, p.block_size, p.max_blocks_per_seq = (num_blocks, num_layers, layer_idx,
                                                                                 block_size, max_blocks)
    return p


def _route(**kw):
    from mio import _lib
    r = _lib.lib.mio_fa3_paged_route(C.byref(_params(**kw)))
    return _lib.FA3_PAGED_ROUTES.get(r) if r >= 0 else None


def test_paged_symbols_bound():
    from mio import _lib, ops
    for name in ("mio_fa3_fwd_paged", "mio_fa3_paged_route", "mio_reshape_and_cache_varlen"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name)
    assert _lib.lib.mio_fa3_paged_route.argtypes == [C.POINTER(_lib.FaPagedParams)]
    assert _lib.lib.mio_fa3_fwd_paged.argtypes[0] == C.POINTER(_lib.FaPagedParams)
    assert len(_lib.lib.mio_reshape_and_cache_varlen.argtypes) == 20
    assert set(_lib.FA3_PAGED_ROUTES.values()) == {"empty", "fwd5", "fwd3"}
    for f in ("flash_attention_varlen_paged", "fa3_paged_route", "reshape_and_cache_varlen"):
        assert callable(getattr(ops, f))


# (geometry, expected route or None = refused, substring of the error)
_PAGED_TABLE = [
    (dict(D=8), "fwd5", None),
    (dict(D=32), "fwd5", None),
    (dict(D=64), "fwd5", None),
    (dict(D=72), "fwd3", None),
    (dict(D=96), "fwd3", None),
    (dict(D=128), "fwd3", None),
    (dict(D=128, causal=0, dtype=1), "fwd3", None),
    (dict(H=32, Hkv=4), "fwd5", None),
    (dict(block_size=128), "fwd5", None),
    (dict(block_size=256, D=128), "fwd3", None),
    (dict(block_size=192), "fwd5", None),
    (dict(layer_idx=1), "fwd5", None),
    (dict(total_q=0, max_q=0), "empty", None),
    (dict(B=0, tables=False), "empty", None),
    (dict(max_k=0), "fwd5", None),                     # every sequence without keys: launched, writes the empty rows
    (dict(block_size=16), None, b"multiple of 64"),
    (dict(block_size=96), None, b"multiple of 64"),
    (dict(block_size=0), None, b"multiple of 64"),
    (dict(H=6, Hkv=4), None, b"multiple of Hkv"),
    (dict(D=136), None, b"head_dim"),
    (dict(D=60), None, b"head_dim"),
    (dict(layer_idx=2), None, b"layer_idx"),
    (dict(layer_idx=-1), None, b"layer_idx"),
    (dict(tables=False), None, b"block_tables"),
    (dict(num_blocks=0), None, b"cache geometry"),
    (dict(num_blocks=-3), None, b"cache geometry"),
    (dict(max_blocks=0), None, b"cache geometry"),
    (dict(dtype=2), None, b"dtype"),
    (dict(ptr_off=8), None, b"aligned"),
    (dict(tok_stride=4 * 64 + 4), None, b"strides"),
    (dict(head_stride=68), None, b"strides"),
    (dict(max_q=0), None, b"max_seqlen_q"),
    (dict(B=-1), None, b"sizes"),
    # 32-bit cache rows: num_blocks * num_layers * block_size < 2^32
    (dict(num_blocks=(1 << 31) // 64 - 1, num_layers=2), "fwd5", None),
    (dict(num_blocks=(1 << 31) // 64, num_layers=2), None, b"2^32"),
]


@pytest.mark.parametrize("geom,want,err", _PAGED_TABLE)
def test_paged_route_table_without_gpu(geom, want, err):
    from mio import _lib
    got = _route(**geom)
    assert got == want, f"{geom}: route {got}, expected {want}"
    if want is None:
        assert err in _lib.lib.mio_last_error(), _lib.lib.mio_last_error()


def _cache(nb=8, L=2, bs=64, Hkv=2, D=64, dtype=torch.bfloat16):
    return torch.zeros(nb, L, bs, Hkv, D, dtype=dtype)


def test_paged_argument_errors_without_gpu():
    """mio_fa3_fwd_paged refuses what the route query refuses, before any launch; ops raises before it calls the library."""
    from mio import _lib, ops
    assert _lib.lib.mio_fa3_fwd_paged(None, None) != 0 and b"null" in _lib.lib.mio_last_error()
    assert _lib.lib.mio_fa3_paged_route(None) < 0
    assert _lib.lib.mio_fa3_fwd_paged(C.byref(_params(block_size=32)), None) != 0
    assert b"multiple of 64" in _lib.lib.mio_last_error()
    assert _lib.lib.mio_fa3_fwd_paged(C.byref(_params(tables=False)), None) != 0
    assert _lib.lib.mio_fa3_fwd_paged(C.byref(_params(total_q=0, max_q=0)), None) == 0  # nothing to do: no launch

    q = torch.zeros(600, 4, 64, dtype=torch.bfloat16)
    kc, vc = _cache(), _cache()
    bt = torch.zeros(2, 8, dtype=torch.int32)
    cu = torch.tensor([0, 300, 600], dtype=torch.int32)
    used = torch.tensor([400, 512], dtype=torch.int32)
    assert ops.fa3_paged_route(q, kc, vc, bt, cu, used, 300, 512, causal=True) == "fwd5"
    assert ops.fa3_paged_route(q, kc, vc, bt, cu, used, 300, 512, layer_idx=1) == "fwd5"
    kc128 = _cache(bs=128, D=128, dtype=torch.float16)
    assert ops.fa3_paged_route(torch.zeros(600, 8, 128, dtype=torch.float16), kc128, kc128, bt, cu, used, 300,
                               512) == "fwd3"
    assert ops.fa3_paged_route(q[:0], kc, vc, bt[:0], cu[:1], used[:0], 0, 512) == "empty"
    with pytest.raises(ValueError):  # CPU tensors: no fallback
        ops.flash_attention_varlen_paged(q, kc, vc, bt, cu, used, 300, 512)
    with pytest.raises(ValueError, match="multiple of 64"):
        ops.fa3_paged_route(q, _cache(bs=16), _cache(bs=16), bt, cu, used, 300, 512)
    with pytest.raises(ValueError, match="layer_idx"):
        ops.fa3_paged_route(q, kc, vc, bt, cu, used, 300, 512, layer_idx=2)
    with pytest.raises(ValueError, match="multiple of num_kv_heads"):
        ops.fa3_paged_route(torch.zeros(600, 3, 64, dtype=torch.bfloat16), kc, vc, bt, cu, used, 300, 512)
    with pytest.raises(ValueError, match="head_dim"):
        ops.fa3_paged_route(q[:, :, :60], _cache(D=60), _cache(D=60), bt, cu, used, 300, 512)
    with pytest.raises(ValueError):
        ops.fa3_paged_route(q, kc, vc, bt.long(), cu, used, 300, 512)
    with pytest.raises(ValueError):
        ops.fa3_paged_route(q, kc, vc, bt, cu.long(), used, 300, 512)
    with pytest.raises(ValueError):
        ops.fa3_paged_route(q, kc, vc, bt, cu, used[:1], 300, 512)
    with pytest.raises(ValueError):
        ops.fa3_paged_route(q, kc, vc[:4], bt, cu, used, 300, 512)
    with pytest.raises(ValueError):
        ops.fa3_paged_route(q[None], kc, vc, bt, cu, used, 300, 512)
    with pytest.raises(ValueError):
        ops.fa3_paged_route(q.float(), kc.float(), vc.float(), bt, cu, used, 300, 512)
    with pytest.raises(ValueError):
        ops.fa3_paged_route(q, kc.transpose(3, 4), vc.transpose(3, 4), bt, cu, used, 300, 512)
    with pytest.raises(RuntimeError):
        ops.fa3_paged_route(q, kc, vc, bt, cu, used, 0, 512)


def test_reshape_and_cache_varlen_errors_without_gpu():
    from mio import _lib, ops
    k = torch.zeros(10, 2, 64, dtype=torch.bfloat16)
    kc, vc = _cache(), _cache()
    bt = torch.zeros(2, 8, dtype=torch.int32)
    cu = torch.tensor([0, 4, 10], dtype=torch.int32)
    cl = torch.tensor([4, 6], dtype=torch.int32)
    with pytest.raises(ValueError):  # CPU tensors: no fallback
        ops.reshape_and_cache_varlen(k, k, kc, vc, bt, cu, cl, 64, 0)
    ks = (C.c_int64 * 2)(128, 64)
    f = _lib.lib.mio_reshape_and_cache_varlen
    args = dict(B=2, T=10, Hkv=2, D=64, nb=8, L=2, layer=0, bs=64, mb=8, dt=0)

    def call(**kw):
        a = dict(args, **kw)
        return f(ALIGNED, ALIGNED, ALIGNED, ALIGNED, ALIGNED, ALIGNED, ALIGNED, ks, ks, a["B"], a["T"], a["Hkv"], a["D"],
                 a["nb"], a["L"], a["layer"], a["bs"], a["mb"], a["dt"], None)

    assert call(layer=2) != 0 and b"geometry" in _lib.lib.mio_last_error()
    assert call(nb=0) != 0 and b"geometry" in _lib.lib.mio_last_error()
    assert call(D=60) != 0 and b"sizes" in _lib.lib.mio_last_error()
    assert call(dt=3) != 0 and b"dtype" in _lib.lib.mio_last_error()
    assert call(T=0) == 0 and call(B=0) == 0  # nothing to write: no launch


def _write_tensors(dtype=torch.bfloat16, T=10, Hkv=2, D=64, cache_dtype=None, L=2, bs=64):
    """Valid CPU arguments of ops._cache_write_args for a varlen write of T tokens in 2 sequences."""
    k = torch.zeros(T, Hkv, D, dtype=dtype)
    c = torch.zeros(8, L, bs, Hkv, D, dtype=cache_dtype or dtype)
    return dict(key=k, value=k.clone(), k_cache=c, v_cache=c.clone(), block_tables=torch.zeros(2, 8, dtype=torch.int32),
                context_lengths=torch.tensor([4, 6], dtype=torch.int32), block_size=bs, layer_idx=1, k_scale=None,
                v_scale=None, who="f", cu_seqlens_new=torch.tensor([0, 4, T], dtype=torch.int32))


def test_cache_write_args_returns_the_c_arguments():
    """The host-only builder of the three cache writes on CPU tensors: addresses, strides and geometry in the C order."""
    from mio import ops
    F8 = torch.float8_e4m3fn
    a = _write_tensors()
    a["key"] = torch.zeros(10, 3 * 2 * 64, dtype=torch.bfloat16)[:, 128:256].view(10, 2, 64)  # a view of a fused projection
    w = ops._cache_write_args(**a)
    assert w.data == (a["key"].data_ptr(), a["value"].data_ptr(), a["k_cache"].data_ptr(), a["v_cache"].data_ptr())
    assert w.tables == (a["block_tables"].data_ptr(), a["cu_seqlens_new"].data_ptr(), a["context_lengths"].data_ptr())
    assert [tuple(s) for s in w.strides] == [(384, 64), (128, 64)]
    assert (w.B, w.T, w.Hkv, w.D, w.geom, w.dt, w.kv8) == (2, 10, 2, 64, (8, 2, 1, 64, 8), 0, False)
    # fp8 cache: the scale addresses of layer_idx follow the caches'
    a = _write_tensors(torch.float16, cache_dtype=F8)
    a.update(k_scale=torch.ones(2), v_scale=torch.ones(1), q=torch.zeros(10, 4, 64, dtype=torch.float16))
    w = ops._cache_write_args(**a)
    assert w.data[4:] == (a["k_scale"].data_ptr() + 4, a["v_scale"].data_ptr()) and w.kv8 and w.dt == 1
    # single-token form: [B, 1, Hkv, D], tables of any integer type converted to int32
    a = _write_tensors()
    a.update(key=a["key"][:2, None], value=a["value"][:2, None], cu_seqlens_new=None, block_tables=a["block_tables"].long())
    w = ops._cache_write_args(**a)
    assert (w.B, w.T, w.Hkv, w.D, w.geom) == (2, 2, 2, 64, (8, 2, 1, 64, 8)) and len(w.tables) == 2
    assert [tuple(s) for s in w.strides] == [(128, 64), (128, 64)] and w.keep[2][0].dtype == torch.int32


_T = _write_tensors
_F8 = torch.float8_e4m3fn
_SHARE = "key, value and caches must share a dtype"
_CU = "cu_seqlens_new must be a contiguous 1-D int32 tensor of B+1 offsets"
# (changes to the valid arguments, the ValueError's text): one case per raise of the builder and of the checks it calls
_WRITE_ERRORS = [
    (lambda a: a.update(key=a["key"][:2], value=a["value"][:2], cu_seqlens_new=None),
     "reshape_and_cache supports q_seq_len == 1 only (attention_kernels.py:1363-1365)"),
    (lambda a: a.update(key=a["key"][:2, None].expand(2, 2, 2, 64), cu_seqlens_new=None),
     "reshape_and_cache supports q_seq_len == 1 only (attention_kernels.py:1363-1365)"),
    (lambda a: a.update(value=a["value"][:9]), "key/value must be [total_new, num_kv_heads, head_dim] with equal shapes, got "
                                               "key=(10, 2, 64), value=(9, 2, 64)"),
    (lambda a: a.update(key=a["key"][0], value=a["value"][0]),
     "key/value must be [total_new, num_kv_heads, head_dim] with equal shapes, got key=(2, 64), value=(2, 64)"),
    (lambda a: a.update(key=a["key"].float(), value=a["value"].float()), "HIP kernels compute in bf16 or fp16, got torch.float32"),
    (lambda a: a.update(value=a["value"].half()), _SHARE),
    (lambda a: a.update(k_cache=a["k_cache"].to(torch.int8), v_cache=a["v_cache"].to(torch.int8)),
     "an 8-bit KV cache must be torch.float8_e4m3fn (OCP e4m3), got torch.int8"),
    (lambda a: a.update(k_cache=a["k_cache"][0], v_cache=a["v_cache"][0]),
     "caches must be [num_blocks, num_layers, block_size, num_kv_heads, head_dim] with equal shapes"),
    (lambda a: a.update(v_cache=a["v_cache"][:4]),
     "caches must be [num_blocks, num_layers, block_size, num_kv_heads, head_dim] with equal shapes"),
    (lambda a: a.update(v_cache=a["v_cache"].half()), _SHARE),
    (lambda a: a.update(k_cache=a["k_cache"].half(), v_cache=a["v_cache"].half()), _SHARE),
    (lambda a: a.update(k_cache=a["k_cache"].transpose(0, 1).contiguous().transpose(0, 1)), "caches must be contiguous"),
    (lambda a: a.update(k_scale=torch.ones(1)),
     "f: k_scale / v_scale apply to an fp8 (float8_e4m3fn) cache only, got a torch.bfloat16 cache"),
    (lambda a: a.update(_T(cache_dtype=_F8), k_scale=torch.ones(1)), "f: an fp8 (float8_e4m3fn) cache requires k_scale and v_scale"),
    (lambda a: a.update(_T(cache_dtype=_F8), k_scale=torch.ones(1), v_scale=torch.ones(1).double()),
     "f: v_scale must be a contiguous float32 tensor"),
    (lambda a: a.update(_T(cache_dtype=_F8), k_scale=1.0, v_scale=torch.ones(1)), "f: k_scale must be a contiguous float32 tensor"),
    (lambda a: a.update(_T(cache_dtype=_F8), k_scale=torch.ones(3), v_scale=torch.ones(1)),
     "f: k_scale must hold 1 or num_layers = 2 elements, got 3"),
    (lambda a: a.update(_T(cache_dtype=_F8), k_scale=torch.ones(1), v_scale=torch.ones(1, device="meta")),
     "f: v_scale must be on the device of the cache"),
    (lambda a: a.update(_T(cache_dtype=_F8), k_scale=torch.ones(2), v_scale=torch.ones(2), layer_idx=2),
     "f: layer_idx 2 out of range for a 2-layer cache"),
    (lambda a: a.update(_T(D=72, cache_dtype=_F8), k_scale=torch.ones(1), v_scale=torch.ones(1)),
     "an fp8 KV cache needs head_dim to be a multiple of 16, got head_dim 72"),
    (lambda a: a.update(q=torch.zeros(9, 4, 64, dtype=torch.bfloat16)),
     "q must be [total_new, num_heads, head_dim] = [10, H, 64] of key's dtype, got (9, 4, 64) torch.bfloat16"),
    (lambda a: a.update(q=torch.zeros(10, 4, 64, dtype=torch.float16)),
     "q must be [total_new, num_heads, head_dim] = [10, H, 64] of key's dtype, got (10, 4, 64) torch.float16"),
    (lambda a: a.update(block_size=32), "cache geometry mismatch"),
    (lambda a: a.update(key=a["key"][:, :1], value=a["value"][:, :1]), "cache geometry mismatch"),
    (lambda a: a.update(_T(D=60)), "head_dim must be a multiple of 8, got 60"),
    (lambda a: a.update(q=torch.zeros(10, 3, 64, dtype=torch.bfloat16)), "num_heads 3 must be a multiple of num_kv_heads 2"),
    (lambda a: a.update(_T(D=136), q=torch.zeros(10, 4, 136, dtype=torch.bfloat16)),
     "head_dim must be a multiple of 8 and <= 128, got 136"),
    (lambda a: a.update(layer_idx=2), "layer_idx 2 out of range for a 2-layer cache"),
    (lambda a: a.update(layer_idx=-1), "layer_idx -1 out of range for a 2-layer cache"),
    (lambda a: a.update(cu_seqlens_new=a["cu_seqlens_new"].long()), _CU),
    (lambda a: a.update(cu_seqlens_new=a["cu_seqlens_new"][None]), _CU),
    (lambda a: a.update(cu_seqlens_new=torch.zeros(6, dtype=torch.int32)[::2]), _CU),
    (lambda a: a.update(cu_seqlens_new=a["cu_seqlens_new"][:0]), _CU),
    (lambda a: a.update(cu_seqlens_new=a["cu_seqlens_new"].to("meta")), "cu_seqlens_new must be on the device of q"),
    (lambda a: a.update(context_lengths=a["context_lengths"].long()),
     "context_lengths must be a contiguous 1-D int32 tensor of B lengths"),
    (lambda a: a.update(block_tables=a["block_tables"][0]),
     "block_tables must be a contiguous 2-D int32 tensor [B, max_blocks_per_seq]"),
    (lambda a: a.update(block_tables=a["block_tables"].to("meta")), "block_tables must be on the device of q"),
    (lambda a: a.update(context_lengths=a["context_lengths"][:1]),
     "context_lengths and block_tables must have B = 2 rows (cu_seqlens_new has B+1 entries)"),
    (lambda a: a.update(block_tables=torch.zeros(3, 8, dtype=torch.int32)),
     "context_lengths and block_tables must have B = 2 rows (cu_seqlens_new has B+1 entries)"),
]


@pytest.mark.parametrize("change,text", _WRITE_ERRORS, ids=[f"{i}-{t[:28]}" for i, (_, t) in enumerate(_WRITE_ERRORS)])
def test_cache_write_args_errors(change, text):
    from mio import ops
    a = _write_tensors()
    assert ops._cache_write_args(**a).B == 2  # the neighbour is valid
    change(a)
    with pytest.raises(ValueError) as e:
        ops._cache_write_args(**a)
    assert str(e.value) == text


@pytest.mark.parametrize("type_id", [0, 1])
def test_fwd5_paged_fits_without_spills(tmp_path, type_id):
    """The paged form of fa3_fwd5_kernel runs two waves per SIMD like the dense one: no scratch, at most 256 VGPRs."""
    text = _isa.fa_isa(tmp_path, "fa3_seq_inst.hip", type_id, 64)
    blocks = _isa.metadata(text, r"_Z21fa3_fwd5_paged_kernel\w+")
    assert len(blocks) == 2, "causal and full instantiations expected"
    for blk in blocks:
        _isa.check_fits_256(blk)
    assert "scratch_" not in text


@pytest.mark.parametrize("type_id,D", [(0, 96), (1, 96), (0, 128), (1, 128)])
def test_fwd3_paged_accumulator_registers_untouched_by_compiler(tmp_path, type_id, D):
    """The paged form of fa3_fwd3_kernel owns the same accumulator registers (Fa3Map<D>::A_Q and up) through inline asm:
    no compiler-generated instruction may touch them (tools/check_agpr.py), and nothing spills."""
    bodies = _isa.kernels(_isa.fa_isa(tmp_path, "fa3_seq_inst.hip", type_id, D), "_Z21fa3_fwd3_paged_kernel")
    assert len(bodies) == 2, "causal and full instantiations expected"
    for body in bodies:
        _isa.check_agpr(tmp_path, body, _isa.fa3_agpr_floor(D))

"""CPU-only tests of token sampling (mio_sample_tokens, ops.sample_tokens / sampling_probs, mio.sampling.Sampler): the symbol
is bound with the header's argument count, every host refusal returns before a launch with a message that names the function,
the ops functions refuse CPU tensors and malformed arguments with the documented exception types, and csrc/sampling.hip
compiles for gfx950 without scratch, with integer LDS atomics only."""
import os
import re

import pytest
import torch

import _isa

ALIGNED = 1 << 20  # a fake 16-byte aligned device address: no refusal dereferences anything
FN = "mio_sample_tokens"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _err():
    from mio import _lib
    return _lib.lib.mio_last_error().decode()


def _rc(*, logits=ALIGNED, ld=None, temperature=ALIGNED, top_k=ALIGNED, top_p=ALIGNED, min_p=ALIGNED, u=ALIGNED, tokens=ALIGNED,
        kept=ALIGNED, probs=ALIGNED, ld_probs=None, B=4, V=1000, dtype=0):
    from mio import _lib
    return _lib.lib.mio_sample_tokens(logits, V if ld is None else ld, temperature, top_k, top_p, min_p, u, tokens, kept, probs,
                                      V if ld_probs is None else ld_probs, B, V, dtype, None)


def test_sampling_symbol_bound():
    from mio import _lib, ops
    assert FN in _lib.EXPORTS and hasattr(_lib.lib, FN)
    assert len(_lib.lib.mio_sample_tokens.argtypes) == 15
    header = open(os.path.join(ROOT, "include", "mio_hip.h")).read()
    decl = re.search(r"int mio_sample_tokens\(([^;]*)\);", header).group(1)
    assert len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")) == 15
    assert _lib.MIO_FP32 == 2 and "MIO_FP32 = 2" in header
    assert _lib.lib.mio_version() == 106 and "#define MIO_VERSION 106" in header  # additive: the ABI version stays
    assert callable(ops.sample_tokens) and callable(ops.sampling_probs)
    import mio
    from mio.sampling import Sampler
    assert mio.Sampler is Sampler


def test_sampling_refusals_c():
    # every refusal returns before a launch: nothing here reaches the fake addresses
    assert _rc(logits=None) < 0 and "null logits" in _err() and FN in _err()
    assert _rc(temperature=None) < 0 and "temperature" in _err() and FN in _err()
    assert _rc(u=None) < 0 and "null u" in _err() and FN in _err()
    assert _rc(tokens=None, kept=None, probs=None) < 0 and "every output is null" in _err() and FN in _err()
    for V in (0, -1, (1 << 20) + 1):
        assert _rc(V=V, ld=1 << 21, ld_probs=1 << 21) < 0 and "V must be in [1, 2^20]" in _err() and FN in _err()
    assert _rc(B=-1) < 0 and "B must not be negative" in _err() and FN in _err()
    assert _rc(ld=999) < 0 and "ld < V" in _err() and FN in _err()
    assert _rc(ld_probs=999) < 0 and "ld_probs < V" in _err() and FN in _err()
    for dtype in (3, -1, 7):
        assert _rc(dtype=dtype) < 0 and "dtype must be bf16, fp16 or fp32" in _err() and FN in _err()
    for off in (2, 4, 8):
        assert _rc(logits=ALIGNED + off) < 0 and "16-byte alignment (logits)" in _err() and FN in _err()
    assert _rc(top_k=ALIGNED + 2) < 0 and "aligned to their element size" in _err() and FN in _err()
    assert _rc(tokens=ALIGNED + 4) < 0 and "aligned to their element size" in _err()
    # ld_probs is judged only with probs_out; an empty batch is 0 without a launch and without looking at the pointers
    assert _rc(B=0, probs=None, ld_probs=0) == 0
    assert _rc(B=0, logits=None, temperature=None, u=None) == 0
    assert _rc(B=0, ld=999) < 0 and "ld < V" in _err()
    # the existing entry points still refuse the new dtype id
    from mio import _lib
    assert _lib.lib.mio_rmsnorm_fwd(ALIGNED, None, ALIGNED, ALIGNED, None, 4, 256, 1e-6, 1.0, 2, 0, None) < 0


def test_sampling_ops_errors_without_gpu():
    from mio import ops
    from mio.sampling import Sampler
    x = torch.zeros(4, 100, dtype=torch.bfloat16)
    for f in (ops.sample_tokens, ops.sampling_probs):
        with pytest.raises(ValueError, match="CUDA"):
            f(x, 1.0)
    with pytest.raises(ValueError, match="CUDA"):
        Sampler(4, "cpu")
    with pytest.raises(ValueError):
        ops.sample_tokens(None, 1.0)
    # the argument checks ahead of the launch, on meta tensors that claim to be on the device (nothing is dereferenced)
    dev = "meta"
    xm = torch.zeros(4, 100, dtype=torch.bfloat16, device=dev)
    chk = ops._sample_param
    with pytest.raises(ValueError, match="CUDA"):
        chk(torch.zeros(4), 4, torch.float32, "temperature", "f", dev)
    with pytest.raises(ValueError, match="f: temperature is required"):
        chk(None, 4, torch.float32, "temperature", "f", dev, required=True)
    assert chk(None, 4, torch.float32, "top_p", "f", dev) is None
    for bad in ("0.5", [0.5], True):
        with pytest.raises(ValueError, match="f: top_p must be a number or a tensor"):
            chk(bad, 4, torch.float32, "top_p", "f", dev)
    with pytest.raises(ValueError, match="f: top_k must be an integer"):
        chk(2.5, 4, torch.int32, "top_k", "f", dev)
    full = chk(0.8, 4, torch.float32, "temperature", "f", dev)
    assert full.shape == (4,) and full.dtype == torch.float32 and chk(50, 4, torch.int32, "top_k", "f", dev).dtype == torch.int32
    del xm


# ---- the unit's ISA ----------------------------------------------------------------------------------------------------
def test_sampling_kernels_isa(tmp_path):
    """Every instantiation of sample_tokens_kernel exists (fp32 streamed; bf16 and fp16 resident and streamed) with zero
    scratch and zero spills, within the 128 VGPRs a workgroup of 1024 threads leaves a lane; the histogram adds are integer LDS
    atomics and there is no float atomic; rows are read 16 bytes at a time."""
    text = _isa.device_isa(tmp_path, "sampling.hip", [], attention=False).read_text()
    blks = _isa.metadata(text, r"_Z\d+sample_tokens_kernel\w+")
    assert len(blks) == 5
    for blk in blks:
        _isa.check_fits_256(blk)
        assert int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1)) <= 128, blk
        assert re.search(r"\.sgpr_spill_count:\s+0\b", blk), blk
    assert text.count("global_load_dwordx4") >= 5 and not re.search(r"\bflat_(load|store|atomic)", text)
    bodies = _isa.kernels(text, r"_Z\d+sample_tokens_kernel")
    assert len(bodies) == 5
    for body in bodies:
        code = [l.split("//")[0].split(";")[0] for l in body]
        assert not [l for l in code if re.search(r"\bscratch_", l)]
        atomics = [l for l in code if re.search(r"atomic|\bds_(add|sub|min|max|pk_add|cmpst|wrxchg)", l)]
        assert atomics and all(re.search(r"\bds_add_u64\b", l) for l in atomics), atomics[:4]
        assert not [l for l in code if re.search(r"_(add|min|max)_(f32|f64|rtn_f32|rtn_f64|pk)", l) and "atomic" in l]

"""CPU-only tests of RMSNorm: the two C-ABI symbols are declared and bound, every host refusal of mio_rmsnorm_fwd and
mio_gemm_rms_bw returns before a launch with a message that starts with the entry point's own name, empty calls return 0, the ops
functions refuse CPU tensors and malformed arguments, the norm-kind helper names its kinds, apply_fused_layernorm swaps the
RMSNorm modules it knows, every row-kernel instantiation compiles without scratch, and the checker of the GPU tests
(tests/_rms_check.py) passes fp32 models of the kernels and fails wrong ones.  Addresses are fake and 16-byte aligned; nothing
is dereferenced."""
import os
import re

import pytest
import torch
import torch.nn as nn

A = 1 << 20  # a fake 16-byte aligned device address
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"mio_rmsnorm_fwd": 12, "mio_gemm_rms_bw": 23}  # name -> number of C arguments


def _lib():
    from mio import _lib
    return _lib


def _err():
    return _lib().lib.mio_last_error().decode()


def test_symbols_declared_and_bound():
    lib = _lib()
    header = open(os.path.join(ROOT, "include", "mio_hip.h")).read()
    for name, nargs in SYMBOLS.items():
        assert re.search(rf"\bint {name}\(", header), name
        assert name in lib.EXPORTS and hasattr(lib.lib, name), name
        assert len(getattr(lib.lib, name).argtypes) == nargs, name
    assert lib.lib.mio_gemm_rms_bw.argtypes == lib.lib.mio_gemm_ln_bw.argtypes
    assert lib.lib.mio_version() == 106 and "#define MIO_VERSION 106" in header


def _row(x=A, residual=None, weight=A, y=A, sum_out=None, rows=5, cols=1024, eps=1e-6, alpha=1.0, dtype=0, y_blocked=0):
    return _lib().lib.mio_rmsnorm_fwd(x, residual, weight, y, sum_out, rows, cols, eps, alpha, dtype, y_blocked, None)


@pytest.mark.parametrize("fault,words", [
    (dict(x=None), "non-null"), (dict(weight=None), "non-null"), (dict(y=None), "non-null"),
    (dict(cols=0), "positive multiple of 8"), (dict(cols=-8), "positive multiple of 8"), (dict(cols=1028), "positive multiple of 8"),
    (dict(cols=8200), "cols > 8192"),
    (dict(cols=1032, y_blocked=1), "multiple of 32"),
    (dict(dtype=2), "bf16 or fp16"),
    (dict(x=A + 8), "16-byte aligned"), (dict(residual=A + 2), "16-byte aligned"), (dict(weight=A + 4), "16-byte aligned"),
    (dict(y=A + 8), "16-byte aligned"), (dict(residual=A, sum_out=A + 8), "16-byte aligned"),
])
def test_rmsnorm_fwd_refusals(fault, words):
    assert _row(**fault) != 0
    assert _err().startswith("mio_rmsnorm_fwd: ") and words in _err(), _err()


def test_rmsnorm_fwd_empty_and_limits():
    assert _row(rows=0) == 0 and _row(rows=0, cols=8192, y_blocked=1, residual=A, sum_out=A) == 0
    # LayerNorm's own limit and words stay
    lib = _lib().lib
    assert lib.mio_layernorm_fwd(None, None, A, None, A, None, 5, 1024, 1e-5, 1.0, 0, None) != 0
    assert _err() == "mio_layernorm_fwd: x, weight, y must be non-null"
    assert lib.mio_layernorm_fwd_bx(A, None, A, None, A, None, 5, 1032, 1e-5, 1.0, 0, None) != 0
    assert _err() == "mio_layernorm_fwd_bx: cols must be a multiple of 32"


# mio_gemm_rms_bw: the consumer form at a shape every blocked-weight form takes (16 x 16 tiles of 256 x 256)
_G = dict(x=A, wb=A, bias=None, bias_gate=None, residual=None, y=A, M=4096, N=4096, K=1024, ldx=1024, ldy=4096, ldr=0, act=0,
          dtype=0, flags=0, ln_stats=A, ln_slots=0, ln_eps=1e-6, stats_out=None, cs_lo=0, cs_hi=0, cs_val=1.0)


def _gemm(entry="mio_gemm_rms_bw", **fault):
    return getattr(_lib().lib, entry)(*dict(_G, **fault).values(), None)


@pytest.mark.parametrize("fault,words", [
    (dict(ln_stats=None), "ln_stats"),
    (dict(residual=A, ldr=4096), "no residual"),
    (dict(stats_out=A), "stats_out"),
    (dict(flags=8), "unknown flag"),
    # through the shared plan, as form GEMM_LN, under this entry point's name
    (dict(x=None), ": x, wb, y must be non-null"),
    (dict(N=0), ": bad sizes"),
    (dict(dtype=2), ": dtype must be bf16 or fp16"),
    (dict(act=9), ": unknown activation"),
    (dict(bias=A + 8), ": pointers must be 16-byte aligned"),
    (dict(ln_stats=A + 8), ": pointers must be 16-byte aligned"),
    (dict(bias_gate=A), ": bias_gate belongs to the gated stage (act == SWIGLU)"),
    (dict(K=1000, ldx=1000), ": this shape / activation does not take the folded kernels (mio_gemm_ln_ok == 0)"),
    (dict(ln_slots=9), ": at most 8 statistic slots"),
    (dict(cs_lo=0, cs_hi=100), ": [cs_lo, cs_hi) must be multiples of 128"),
])
def test_gemm_rms_bw_refusals(fault, words):
    lib = _lib().lib
    assert lib.mio_gemm_ln_ok(_G["M"], _G["N"], _G["K"], 0, 1, 0) == 1  # the neighbour is a valid consumer call
    assert _gemm(**fault) != 0
    assert _err().startswith("mio_gemm_rms_bw") and words in _err(), _err()


def test_gemm_rms_bw_empty_and_ln_bw_flag_stays():
    assert _gemm(M=0) == 0 and _gemm(M=0, flags=8) == 0
    assert _gemm("mio_gemm_ln_bw", flags=8) != 0 and _err() == "mio_gemm_ln_bw: unknown flag"


def test_ops_refuse_cpu_tensors_and_malformed_arguments():
    from mio import ops
    x, w = torch.zeros(4, 64, dtype=torch.bfloat16), torch.ones(64, dtype=torch.bfloat16)
    for bad_w in (w, w.float(), torch.ones(32, dtype=torch.bfloat16), torch.ones(128, dtype=torch.bfloat16)[::2]):
        with pytest.raises(ValueError):
            ops.rmsnorm(x, bad_w)
    with pytest.raises(ValueError):
        ops.rmsnorm(x, w, residual=torch.zeros(4, 32, dtype=torch.bfloat16))
    with pytest.raises(ValueError):
        ops.rmsnorm(torch.zeros(2, 8200, dtype=torch.bfloat16), torch.ones(8200, dtype=torch.bfloat16))
    lin = torch.zeros(128, 64, dtype=torch.bfloat16)
    for bad_g in (w, w.float(), torch.ones(32, dtype=torch.bfloat16), torch.ones(128, dtype=torch.bfloat16)[::2]):
        with pytest.raises(ValueError):
            ops.rms_fold_weight(lin, bad_g)
    with pytest.raises(ValueError):
        ops.rms_fold_weight(lin, w, torch.zeros(64, dtype=torch.bfloat16))


def test_rmsnorm_argument_checks(monkeypatch):
    """The weight / residual / width checks themselves, with the device check out of the way (nothing is launched: each call is
    refused)."""
    from mio import ops
    monkeypatch.setattr(ops, "_need_cuda", lambda *ts: None)
    monkeypatch.setattr(ops, "_vec_ok", _vec_ok_any_device)
    monkeypatch.setattr(ops, "_res_ok", _res_ok_any_device)
    x, w = torch.zeros(4, 64, dtype=torch.bfloat16), torch.ones(64, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="activation dtype"):
        ops.rmsnorm(x, w.float())
    with pytest.raises(ValueError, match="64 elements"):
        ops.rmsnorm(x, torch.ones(32, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="contiguous"):
        ops.rmsnorm(x, torch.ones(128, dtype=torch.bfloat16)[::2])
    with pytest.raises(ValueError, match="residual"):
        ops.rmsnorm(x, w, residual=torch.zeros(4, 32, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="8192"):
        ops.rmsnorm(torch.zeros(2, 8200, dtype=torch.bfloat16), torch.ones(8200, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="bf16 or fp16"):
        ops.rmsnorm(x.float(), w.float())
    with pytest.raises(ValueError, match="gamma"):
        ops.rms_fold_weight(torch.zeros(128, 64, dtype=torch.bfloat16), torch.ones(32, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="bias"):
        ops.rms_fold_weight(torch.zeros(128, 64, dtype=torch.bfloat16), w, torch.zeros(64, dtype=torch.bfloat16))


def _vec_ok_any_device(t, n, dtype, what):
    if t is None:
        return
    if t.dim() != 1 or t.numel() != n or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous 1-D tensor of {n} elements, got shape {tuple(t.shape)}")
    if t.dtype != dtype:
        raise ValueError(f"{what} must have the activation dtype {dtype}, got {t.dtype}")


def _res_ok_any_device(r, numel, dtype):
    if r is not None and (r.dtype != dtype or r.numel() != numel):
        raise ValueError("residual must have the activation dtype and the input's size")


def test_gemm_ln_norm_argument():
    from mio import ops
    x, wb = torch.zeros(4096, 1024, dtype=torch.bfloat16), torch.zeros(4096, 1024, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="norm must be one of"):
        ops.gemm_ln(x, wb, None, M=4096, N=4096, K=1024, norm="x")
    with pytest.raises(ValueError, match="ln_stats"):
        ops.gemm_ln(x, wb, None, M=4096, N=4096, K=1024, norm="rms")
    with pytest.raises(ValueError, match="norm must be one of"):
        ops.gemm_route(x, wb, None, M=4096, N=4096, K=1024, norm="x")
    st = torch.zeros(ops.ln_stats_shape(4096, 1024))
    for norm in ("layernorm", "rms"):  # the same routes for both norms (host-only: shapes and which operands are given)
        assert ops.gemm_route(x, wb, None, M=4096, N=4096, K=1024, ln_stats=st, norm=norm) == "p8w_fold"
    assert ops.gemm_route(x, wb, None, M=4096, N=4096, K=1024, ln_stats=st) == "p8w_fold"


def test_norm_kind():
    from mio._nn import norm_kind
    from mio.synthetic import FusedLayerNorm, FusedRMSNorm
    assert norm_kind(nn.LayerNorm(8, eps=1e-3)) == ("layernorm", 1e-3)
    assert norm_kind(FusedLayerNorm(8)) == ("layernorm", 1e-5)
    assert norm_kind(nn.RMSNorm(8, eps=1e-6)) == ("rms", 1e-6)
    assert norm_kind(FusedRMSNorm(8, eps=1e-4), torch.float16) == ("rms", 1e-4)
    for dt in (torch.bfloat16, torch.float16):  # eps=None: the activation dtype's eps, as torch.nn.RMSNorm resolves it
        assert norm_kind(nn.RMSNorm(8), dt) == ("rms", torch.finfo(dt).eps)
    with pytest.raises(ValueError):
        norm_kind(nn.RMSNorm(8))
    for other in (nn.GroupNorm(2, 8), nn.Identity(), None):
        with pytest.raises(TypeError, match="LayerNorm"):
            norm_kind(other)


def test_folded_weight_cache_keys_hold_the_kind(monkeypatch):
    """The same Linear behind a LayerNorm and behind an RMSNorm that share one weight tensor: two folds, neither stale."""
    from mio import ops
    from mio._nn import CastCache
    calls = []
    monkeypatch.setattr(ops, "ln_fold_weight", lambda w, g, b, bias, blocked=True: calls.append("layernorm") or ("ln", bias))
    monkeypatch.setattr(ops, "rms_fold_weight", lambda w, g, bias=None, blocked=True: calls.append("rms") or ("rms", bias))
    monkeypatch.setattr(ops, "block_weight_glu", lambda g, u: (g, u))
    lin, up = nn.Linear(8, 16).bfloat16(), nn.Linear(8, 16).bfloat16()
    ln, rms = nn.LayerNorm(8).bfloat16(), nn.RMSNorm(8, eps=1e-6).bfloat16()
    rms.weight = ln.weight  # one parameter under both norms: the kind alone tells the folds apart
    c = CastCache()
    assert c.get_ln_folded(lin, ln, torch.bfloat16)[0] == "ln" and c.get_ln_folded(lin, rms, torch.bfloat16)[0] == "rms"
    assert c.get_ln_folded(lin, ln, torch.bfloat16)[0] == "ln" and c.get_ln_folded(lin, rms, torch.bfloat16)[0] == "rms"
    assert calls == ["layernorm", "rms"]
    assert c.get_ln_folded_glu(lin, up, ln, torch.bfloat16)[0] == ("ln", "ln")
    assert c.get_ln_folded_glu(lin, up, rms, torch.bfloat16)[0] == ("rms", "rms")
    assert c.get_ln_folded_glu(lin, up, ln, torch.bfloat16)[0] == ("ln", "ln")
    assert calls == ["layernorm", "rms"] + ["layernorm"] * 2 + ["rms"] * 2


class LlamaRMSNorm(nn.Module):  # the LLaMA form as transformers writes it
    def __init__(self, d, eps=1e-6):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(d))
        self.variance_epsilon = eps


class Qwen3RMSNorm(nn.Module):  # the same form with `eps`
    def __init__(self, d, eps=1e-5):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(d))
        self.eps = eps


class GemmaRMSNorm(nn.Module):  # scales by (1 + weight): not this norm
    def __init__(self, d, eps=1e-6):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(d))
        self.eps = eps


def test_apply_fused_layernorm_swaps_rmsnorm():
    from mio.optimizer import apply_fused_layernorm
    from mio.synthetic import FusedLayerNorm, FusedRMSNorm
    model = nn.Sequential()
    model.add_module("ln", nn.LayerNorm(16))
    model.add_module("rms", nn.RMSNorm(16, eps=1e-4))
    model.add_module("rms_default_eps", nn.RMSNorm(16))
    model.add_module("inner", nn.Sequential(LlamaRMSNorm(16, 1e-6), Qwen3RMSNorm(16, 1e-5), GemmaRMSNorm(16)))
    model.add_module("no_weight", nn.RMSNorm(16, elementwise_affine=False))
    model = model.to(torch.bfloat16)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(getattr(m, "weight", None), nn.Parameter):
                m.weight.copy_(torch.randn(16))
    want = {k: v.clone() for k, v in model.state_dict().items()}
    out = apply_fused_layernorm(model)
    assert type(out.ln) is FusedLayerNorm
    assert type(out.rms) is FusedRMSNorm and out.rms.eps == 1e-4
    assert type(out.rms_default_eps) is FusedRMSNorm and out.rms_default_eps.eps is None
    assert type(out.inner[0]) is FusedRMSNorm and out.inner[0].eps == 1e-6
    assert type(out.inner[1]) is FusedRMSNorm and out.inner[1].eps == 1e-5
    assert type(out.inner[2]) is GemmaRMSNorm and type(out.no_weight) is nn.RMSNorm
    got = out.state_dict()
    assert got.keys() == want.keys()
    for k, v in want.items():
        assert got[k].dtype == v.dtype and torch.equal(got[k], v), k


def test_block_takes_the_norm_kind():
    from mio.synthetic import Block, FusedLayerNorm, FusedRMSNorm, GPT2ShapedStack
    assert type(Block(64, 2, 128, True, "bf16").ln_1) is FusedLayerNorm
    b = Block(64, 2, 128, True, "bf16", activation="swiglu", norm="rms")
    assert type(b.ln_1) is FusedRMSNorm and type(b.ln_2) is FusedRMSNorm
    s = GPT2ShapedStack(64, 2, 1, 128, norm="rms")
    assert type(s.ln_f) is FusedRMSNorm and type(s.h[0].ln_2) is FusedRMSNorm
    assert type(GPT2ShapedStack(64, 2, 1, 128).ln_f) is FusedLayerNorm
    with pytest.raises(ValueError):
        Block(64, 2, 128, True, "bf16", norm="x")
    with pytest.raises(ValueError):
        FusedRMSNorm(64)(torch.zeros(2, 64))


def test_row_kernels_compile_without_scratch(tmp_path):
    """Every instantiation of the row kernel for gfx950 -- LayerNorm's 1 to 8 chunks per lane, RMSNorm's 1 to 16, both dtypes --
    has no scratch and fits 256 registers, and 16 chunks exist for RMSNorm alone."""
    import _isa
    text = _isa.device_isa(tmp_path, "rowops.hip", [], attention=False).read_text()
    blocks = _isa.metadata(text, r"_Z16layernorm_kernel\w+")
    names = sorted(re.search(r"\.name:\s+(\S+)", b).group(1) for b in blocks)
    rms, ln = [n for n in names if "ELb1EE" in n], [n for n in names if "ELb0EE" in n]
    assert len(rms) == 10 and len(ln) == 8 and len(names) == 18, names
    assert sum("Li16ELb1" in n for n in rms) == 2 and not any("Li16E" in n for n in ln), names
    for b in blocks:
        _isa.check_fits_256(b)


# ---- the checker itself (tests/_rms_check.py): an fp32 model of each kernel passes, a wrong one does not ------------------------
def _model_rows(s, w, eps, dtype, wrong=None):
    """The row kernel's operation sequence in fp32 on the CPU (sequential sums instead of the wave's tree)."""
    f = s.float()
    q = (f * f).sum(-1, keepdim=True) / s.shape[-1]
    if wrong == "variance":  # a LayerNorm-style variance instead of the second moment
        q = q - f.mean(-1, keepdim=True) ** 2
    r = torch.rsqrt(q + (0.0 if wrong == "no_eps" else eps))
    if wrong == "rstd_off":
        r = r * (1 + 2.0 ** -6)  # four bf16 ulps
    return (f * r * w.float()).to(dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("cols", [8, 520, 8192])
def test_rms_check_rows_model(dtype, cols):
    import _gemm_check as gc
    import _rms_check as rc
    g = torch.Generator().manual_seed(cols)
    scale = 10.0 ** (torch.rand(64, 1, generator=g) * 4 - 2)
    s = torch.randn(64, cols, generator=g) * scale + 0.5 * scale
    s[5] = 0
    s[17] = scale[17]
    s = s.to(dtype)
    w = (1 + 0.2 * torch.randn(cols, generator=g)).to(dtype)
    ref = rc.reference_rows(s, w, 1e-6)
    assert bool((ref.y[5] == 0).all()) and bool((ref.tol[5] == 0).all())
    bnd = gc.element_bound(ref, dtype)
    err = lambda y: (y.double() - ref.y).abs()  # noqa: E731
    y = _model_rows(s, w, 1e-6, dtype)
    assert bool((err(y) <= bnd).all()) and rc.not_rn(y, ref, dtype) < 0.01
    assert bool((err(_model_rows(s, w, 1e-6, dtype, "variance")) > bnd).any())
    assert bool((err(_model_rows(s, w, 1e-6, dtype, "rstd_off")) > bnd).any())
    tiny = (s.float() * 1e-3).to(dtype)  # rows whose second moment is near eps
    rt = rc.reference_rows(tiny, w, 1e-6)
    assert bool(((_model_rows(tiny, w, 1e-6, dtype).double() - rt.y).abs() <= gc.element_bound(rt, dtype)).all())
    assert bool(((_model_rows(tiny, w, 1e-6, dtype, "no_eps").double() - rt.y).abs() > gc.element_bound(rt, dtype)).any())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_rms_check_sum_bound_model(dtype):
    import _rms_check as rc
    g = torch.Generator().manual_seed(1)
    x, r = (torch.randn(32, 264, generator=g) * 3).to(dtype), (torch.randn(32, 264, generator=g) * 3).to(dtype)
    ref, bnd = rc.sum_bound(x, r, 0.5, dtype)
    s = (x.float() + 0.5 * r.float()).to(dtype)
    assert bool(((s.double() - ref).abs() <= bnd).all())
    up = torch.nextafter(s.float(), torch.full_like(s.float(), 1e9)).to(dtype)  # a neighbour on the 16-bit grid is outside
    up = torch.where(up == s, (s.float() * (1 + 2.0 ** -7)).to(dtype), up)
    assert bool(((up.double() - ref).abs() > bnd).any())


@pytest.mark.parametrize("act", ["none", "gelu", "swiglu"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_rms_check_fold_model(dtype, act):
    """reference_fold_rms is RMSNorm -> linear of the stream, an fp32 model of the consumer passes under the LayerNorm fold's
    bars, the sum entries do not matter, and a consumer that subtracts the mean fails."""
    import _gemm_check as gc
    import _rms_check as rc
    M, N, K = 96, 64, 512
    g = torch.Generator().manual_seed(3)
    y = (torch.randn(M, K, generator=g) * 2 + 1).to(dtype)
    gam = (1 + 0.2 * torch.randn(K, generator=g)).to(dtype)
    ws = ((torch.randn(N, K, generator=g) * K ** -0.5) * gam.float()).to(dtype)
    wg = ((torch.randn(N, K, generator=g) * K ** -0.5) * gam.float()).to(dtype)
    b, bg = (0.1 * torch.randn(N, generator=g)).to(dtype), (0.1 * torch.randn(N, generator=g)).to(dtype)
    yd = y.double().view(M, K // 256, 256)
    st = torch.stack([yd.sum(-1).t().float(), (yd * yd).sum(-1).t().float()], -1)  # [slots, M, 2]
    kw = dict(ws_gate=wg, bias_gate=bg) if act == "swiglu" else {}
    ref = rc.reference_fold_rms(y, st, ws, b, eps=1e-6, act=act, **kw)
    nan_sums = st.clone()
    nan_sums[..., 0] = float("nan")
    ref2 = rc.reference_fold_rms(y, nan_sums, ws, b, eps=1e-6, act=act, **kw)
    assert torch.equal(ref.y, ref2.y) and torch.equal(ref.tol, ref2.tol)
    if act == "none":  # RMSNorm -> linear of the stream itself
        want = torch.nn.functional.rms_norm(y.double(), (K,), None, 1e-6) @ ws.double().t() + b.double()
        assert float((ref.y - want).abs().max()) < 1e-6  # (the slot sums are rounded to fp32: 2^-24 of the second moment)

    def model(centre):
        q = st[..., 1].sum(0) / K
        if centre:
            q = q - (st[..., 0].sum(0) / K) ** 2
        r = torch.rsqrt(q + 1e-6)[:, None]
        z = (y.float() @ ws.float().t()) * r + b.float()
        if act == "swiglu":
            z = torch.nn.functional.silu((y.float() @ wg.float().t()) * r + bg.float()) * z
        elif act == "gelu":
            z = torch.nn.functional.gelu(z, approximate="tanh")
        return z.to(dtype)

    route = "p8w_glu_fold" if act == "swiglu" else "p8w_fold"
    gc.check(model(False), ref, dtype, route, bars=gc.BARS[(dtype, route)], what="fp32 model of the RMS consumer")
    with pytest.raises(AssertionError):
        gc.check(model(True), ref, dtype, route, bars=False)

"""CPU-only tests of the decode-step GEMM's host side, through the loaded library: the C-ABI symbols are declared and bound, every
refusal of mio_gemm_skinny returns before a launch with a message under the entry point's name, an empty call returns 0, the
workspace size follows the split count, the split count never falls as K grows, the slices are whole 32-k steps that cover K, and
ops.gemm_skinny checks its arguments as ops.gemm_bias_act does, and the GPU tests' case tables (tests/_skinny_cases.py) reach the
kernel's seams under the plan the library holds.  Addresses are fake and 16-byte aligned; nothing is dereferenced."""
import ctypes as C
import os
import re

import pytest
import torch

import _skinny_cases as sk

A = 1 << 20  # a fake 16-byte aligned device address
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"mio_gemm_skinny_workspace_bytes": 4, "mio_gemm_skinny_splits": 4, "mio_gemm_skinny_ok": 4, "mio_gemm_skinny": 18,
           "mio_gemm_skinny_slice": 7, "mio_gemm_skinny_chunk_k": 1}  # name -> number of C arguments
SWIGLU = 5
SHAPES = [(M, N, K) for M in (1, 5, 16, 37, 64) for N in (1, 72, 1000, 3072, 14336) for K in (8, 40, 264, 1024, 2056, 4104, 14336)]


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
    assert lib.ACT_SWIGLU == SWIGLU
    assert "F.linear" in header[header.index("The decode-step GEMM"):header.index("size_t mio_gemm_skinny_workspace_bytes")]


# a legal call that splits K (M 4, N 1024, K 1024): every fault below is the only thing wrong with it
_G = dict(x=A, w=A, bias=None, w_gate=None, bias_gate=None, residual=None, y=A, workspace=A, M=4, N=1024, K=1024, ldx=1024,
          ldw=1024, ldy=1024, ldr=0, act=0, dtype=0)


def _call(**fault):
    return _lib().lib.mio_gemm_skinny(*dict(_G, **fault).values(), None)


@pytest.mark.parametrize("fault,words", [
    (dict(M=65), "at most 64"),
    (dict(M=-1), "negative"), (dict(N=-8), "negative"), (dict(K=-8), "negative"),
    (dict(K=1028, ldx=1032, ldw=1032), "K must be a multiple of 8"),
    (dict(ldx=1028), "multiples of 8"), (dict(ldw=1028), "multiples of 8"), (dict(ldy=1028), "multiples of 8"),
    (dict(residual=A, ldr=1028), "multiples of 8"),
    (dict(ldx=1016), "smaller than row length"), (dict(ldy=1016), "smaller than row length"),
    (dict(residual=A, ldr=8), "smaller than row length"),
    (dict(x=None), "non-null"), (dict(w=None), "non-null"), (dict(y=None), "non-null"),
    (dict(x=A + 8), "16-byte aligned"), (dict(w=A + 2), "16-byte aligned"), (dict(y=A + 4), "16-byte aligned"),
    (dict(bias=A + 8), "16-byte aligned"), (dict(residual=A + 8, ldr=1024), "16-byte aligned"),
    (dict(workspace=A + 4), "16-byte aligned"), (dict(act=SWIGLU, w_gate=A + 8), "16-byte aligned"),
    (dict(act=SWIGLU), "w_gate"), (dict(w_gate=A), "w_gate"), (dict(bias_gate=A), "bias_gate"),
    (dict(act=6), "unknown activation"), (dict(act=-1), "unknown activation"),
    (dict(dtype=2), "bf16 or fp16"),
    (dict(workspace=None), "workspace required"),
])
def test_refusals(fault, words):
    lib = _lib().lib
    assert lib.mio_gemm_skinny_splits(_G["M"], _G["N"], _G["K"], 0) > 1  # the neighbour is a legal call that splits
    assert _call(**fault) != 0
    assert _err().startswith("mio_gemm_skinny: ") and words in _err(), _err()


def test_empty_and_queries_refuse():
    """M == 0 returns 0 whatever the data pointers; the host queries refuse what the launch refuses."""
    lib = _lib().lib
    assert _call(M=0) == 0 and _call(M=0, x=None, y=None, workspace=None) == 0
    for M, N, K, act, words in [(65, 8, 8, 0, "at most 64"), (-1, 8, 8, 0, "negative"), (4, 8, 12, 0, "multiple of 8"),
                                (4, 8, 8, 7, "unknown activation")]:
        assert lib.mio_gemm_skinny_splits(M, N, K, act) < 0
        assert _err().startswith("mio_gemm_skinny_splits: ") and words in _err(), _err()
        assert lib.mio_gemm_skinny_ok(M, N, K, act) == 0
        assert lib.mio_gemm_skinny_workspace_bytes(M, N, K, act) == 0
        kb, ke = C.c_int32(), C.c_int32()
        assert lib.mio_gemm_skinny_slice(M, N, K, act, 0, C.byref(kb), C.byref(ke)) < 0
    assert lib.mio_gemm_skinny_ok(0, 1024, 1024, 0) == 0


@pytest.mark.parametrize("act", [0, 1, SWIGLU])
def test_workspace_follows_splits(act):
    lib = _lib().lib
    split = 0
    for M, N, K in SHAPES:
        n = lib.mio_gemm_skinny_splits(M, N, K, act)
        assert n >= 1, (M, N, K)
        want = 0 if n == 1 else n * M * N * 4 * (2 if act == SWIGLU else 1)
        assert lib.mio_gemm_skinny_workspace_bytes(M, N, K, act) == want, (M, N, K)
        split += n > 1
    assert split > 0 and split < len(SHAPES)  # both kinds are among the shapes


def test_splits_monotone_in_k():
    lib = _lib().lib
    for M in (1, 4, 16, 17, 64):
        for N in (8, 1000, 1024, 4096, 14336):
            last = 0
            for K in range(8, 16400, 8):
                n = lib.mio_gemm_skinny_splits(M, N, K, 0)
                assert n >= last, (M, N, K, n, last)
                last = n
            assert last > 1


def test_slices_cover_k_in_whole_steps():
    """Slice s is [k_begin, k_end): they tile [0, K) in order, every begin is a multiple of 32, every length is a multiple of 32
    (the last slice ends at K, a multiple of 8), and with several slices none is shorter than 8 M: the partials written stay at
    or under 1/4 of the weight bytes read."""
    lib = _lib().lib
    for M, N, K in SHAPES + [(3, 8, 2056), (64, 264, 1024), (37, 72, 8)]:
        n = lib.mio_gemm_skinny_splits(M, N, K, 0)
        at = 0
        for s in range(n):
            kb, ke = C.c_int32(-1), C.c_int32(-1)
            assert lib.mio_gemm_skinny_slice(M, N, K, 0, s, C.byref(kb), C.byref(ke)) == 0
            assert kb.value == at and kb.value % 32 == 0 and ke.value > kb.value, (M, N, K, s)
            assert (ke.value - kb.value) % 32 == 0 or ke.value == K, (M, N, K, s)
            if n > 1:
                assert -(-(ke.value - kb.value) // 32) * 32 >= 8 * M, (M, N, K, s)
            at = ke.value
        assert at == K, (M, N, K)
        kb, ke = C.c_int32(), C.c_int32()
        assert lib.mio_gemm_skinny_slice(M, N, K, 0, n, C.byref(kb), C.byref(ke)) != 0
        assert _err().startswith("mio_gemm_skinny_slice: ")


def test_chunk_query():
    """k per chunk of the kernel's loop: 256, SwiGLU 128 (two weights in the same registers); an unknown activation is refused."""
    lib = _lib().lib
    assert [lib.mio_gemm_skinny_chunk_k(a) for a in range(SWIGLU + 1)] == [256] * SWIGLU + [128]
    for act in (-1, SWIGLU + 1):
        assert lib.mio_gemm_skinny_chunk_k(act) < 0
        assert _err() == "mio_gemm_skinny_chunk_k: unknown activation"


def _chunks(c):
    """Chunks per slice of case c under the loaded library's plan: one entry per slice."""
    lib, act = _lib().lib, sk.ACTS.index(c.act)
    n, per = lib.mio_gemm_skinny_splits(c.M, c.N, c.K, act), lib.mio_gemm_skinny_chunk_k(act)
    assert n >= 1 and per > 0, (c, _err())
    out = []
    for s in range(n):
        kb, ke = C.c_int32(), C.c_int32()
        assert lib.mio_gemm_skinny_slice(c.M, c.N, c.K, act, s, C.byref(kb), C.byref(ke)) == 0, (c, _err())
        out.append(-(-(ke.value - kb.value) // per))
    return out


def test_case_tables_reach_the_seams():
    """What tests/test_gpu_gemm_skinny.py runs, under the plan as it is now.  Every case splits K or not as its table says; the
    deep cases reach, for plain and SwiGLU and for each count of row fragments, one slice of 3, of 4 and of 5 or more chunks, and
    several slices of 3 or more chunks with unequal counts (with a full and with a ragged last row fragment, and at M 1); the
    ragged-N cases write partials (N % 4 != 0 at N 1, below 16, just under a workgroup's 64 columns and above it); SwiGLU runs at
    every count of row fragments through both epilogues, with and without its biases and residual.  A requirement nobody meets
    is reported with the chunk counts of its table's cases of that kind."""
    from mio import _lib as L
    assert [L.ACT_SWIGLU, sk.ACTS.index("swiglu")] == [SWIGLU] * 2 and sk.ACTS.index("none") == 0
    chunks = {c: _chunks(c) for t in sk.TABLES.values() for c in t}
    wrong = [(name, c.what, chunks[c]) for name, t in sk.TABLES.items() for c in t if (len(chunks[c]) > 1) != c.split]
    assert not wrong, f"the plan splits K otherwise than these cases say: {wrong}"
    missing = []

    def need(table, glu, text, pred):
        mine = [c for c in sk.TABLES[table] if c.glu == glu]
        if not any(pred(c, chunks[c]) for c in mine):
            missing.append(f"{table}: no {'SwiGLU' if glu else 'plain'} case with {text}; its cases: "
                           + ", ".join(f"{c.what} -> {chunks[c]}" for c in mine))

    def deep(ch):  # several slices, each long enough to reload a register set, of unequal chunk counts
        return len(ch) > 1 and min(ch) >= 3 and len(set(ch)) > 1

    for glu in (False, True):
        for mf in (1, 2, 3, 4):
            for n, text in ((3, "3"), (4, "4"), (5, "5 or more")):
                need("DEEP_UNSPLIT", glu, f"MF {mf}, one slice of {text} chunks",
                     lambda c, ch: c.mf == mf and len(ch) == 1 and (ch[0] == n if n < 5 else ch[0] >= 5))
            for full in (True, False):
                need("DEEP_SPLIT", glu, f"MF {mf}, a {'full' if full else 'ragged'} last fragment, slices of >= 3 chunks, unequal",
                     lambda c, ch: c.mf == mf and (c.M % 16 == 0) == full and deep(ch))
        need("DEEP_SPLIT", glu, "M 1, slices of >= 3 chunks, unequal", lambda c, ch: c.M == 1 and deep(ch))
        for lo, hi in ((3, 4), (4, 5)) if glu else ((3, 4),):  # the exits after a reload: odd and even counts side by side
            need("DEEP_SPLIT", glu, f"slices of exactly {lo} and {hi} chunks", lambda c, ch: len(ch) > 1 and set(ch) == {lo, hi})
        for text, ok in (("N 1", lambda N: N == 1), ("1 < N < 16", lambda N: 1 < N < 16), ("48 < N < 64", lambda N: 48 < N < 64),
                         ("N > 64", lambda N: N > 64)):
            need("N_EDGES_SPLIT", glu, f"several slices, N % 4 != 0, {text}", lambda c, ch: len(ch) > 1 and c.N % 4 != 0 and ok(c.N))
    for mf in (1, 2, 3, 4):
        for split in (False, True):
            for full in (True, False):
                need("SWIGLU_FRAGMENTS", True, f"MF {mf}, {'several slices' if split else 'one slice'}, "
                     f"{'both biases and the residual' if full else 'no bias, no residual'}",
                     lambda c, ch: c.mf == mf and (len(ch) > 1) == split and [c.bias, c.bias_gate, c.res] == [full] * 3)
    assert not missing, "\n".join(missing)
    # the deep tables hold nothing that is not deep, and stay within the K the borrowed statistical bars already judge here
    for c in sk.DEEP_UNSPLIT + sk.DEEP_SPLIT:
        assert min(chunks[c]) >= 3 and c.K <= 4104, (c.what, chunks[c])
    assert all(c.N == sk.DEEP_N and c.K <= sk.DEEP_LDW for c in sk.DEEP_UNSPLIT)


def test_ops_queries():
    from mio import ops
    assert ops.gemm_skinny_splits(4, 1024, 1024) == _lib().lib.mio_gemm_skinny_splits(4, 1024, 1024, 0) > 1
    assert ops.gemm_skinny_splits(37, 72, 40, "gelu") == 1
    with pytest.raises(ValueError, match="at most 64"):
        ops.gemm_skinny_splits(65, 1024, 1024)
    with pytest.raises(ValueError, match="Unsupported activation"):
        ops.gemm_skinny_splits(4, 1024, 1024, "tanh")
    assert ops.gemm_skinny_ok(65, 4096, 4096) is False and ops.gemm_skinny_ok(4, 4096, 4096, "tanh") is False
    assert ops.gemm_skinny_ok(4, 8, 8) is False  # tiny weights: two launches or one, the parent route is no slower
    # the regions of the measured sweep (profiles/skinny_gemm.md): plain activations from 1024 x 1024 weights up at every M,
    # SwiGLU for at most one row fragment from 14336 x 4096 up; nothing below the smallest weight measured
    assert all(ops.gemm_skinny_ok(M, N, K, a) for M in (1, 16, 64) for N, K in ((4096, 4096), (4096, 14336), (1024, 1024))
               for a in ("none", "gelu"))
    assert ops.gemm_skinny_ok(16, 14336, 4096, "swiglu") and not ops.gemm_skinny_ok(17, 14336, 4096, "swiglu")
    assert not ops.gemm_skinny_ok(1, 4096, 4096, "swiglu") and not ops.gemm_skinny_ok(64, 1024, 1016)


def test_ops_refuse_cpu_tensors_as_gemm_bias_act_does():
    from mio import ops
    x, w = torch.zeros(4, 64, dtype=torch.bfloat16), torch.zeros(128, 64, dtype=torch.bfloat16)
    for fn in (ops.gemm_bias_act, ops.gemm_skinny):
        with pytest.raises(ValueError, match="CUDA"):
            fn(x, w)


def test_ops_argument_checks(monkeypatch):
    """The checks themselves with the device check out of the way (each call is refused before a launch), next to
    gemm_bias_act's for the same condition: same exception type."""
    from mio import ops
    monkeypatch.setattr(ops, "_need_cuda", lambda *ts: None)
    monkeypatch.setattr(ops, "_vec_ok", _vec_ok_any_device)
    monkeypatch.setattr(ops, "_res_ok", _res_ok_any_device)
    bf = torch.bfloat16
    x, w = torch.zeros(4, 64, dtype=bf), torch.zeros(128, 64, dtype=bf)
    for fn in (ops.gemm_bias_act, ops.gemm_skinny):
        with pytest.raises(ValueError, match="Unsupported activation"):
            fn(x, w, activation="tanh")
        with pytest.raises(ValueError, match="bf16 or fp16"):
            fn(x.float(), w.float())
        with pytest.raises(ValueError, match="same dtype"):
            fn(x, w.half())
        with pytest.raises(ValueError, match="does not match input features"):
            fn(x, torch.zeros(128, 32, dtype=bf))
        with pytest.raises(ValueError, match="bias"):
            fn(x, w, torch.zeros(64, dtype=bf))
        with pytest.raises(ValueError, match="activation dtype"):
            fn(x, w, torch.zeros(128))
        with pytest.raises(ValueError, match="bias_gate"):
            fn(x, w, None, "swiglu", w_gate=w, bias_gate=torch.zeros(64, dtype=bf))
        with pytest.raises(ValueError, match="gate weights"):
            fn(x, w, None, "swiglu")
        with pytest.raises(ValueError, match="residual"):
            fn(x, w, residual=torch.zeros(4, 64, dtype=bf))
    with pytest.raises(ValueError, match="at most 64 rows"):
        ops.gemm_skinny(torch.zeros(5, 13, 64, dtype=bf), w)


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


def test_linear_takes_the_kernel_only_when_asked_and_advised(monkeypatch):
    """mio._nn.linear: skinny=True goes to ops.gemm_skinny only without a blocked x, without a column scale and where
    ops.gemm_skinny_ok holds; skinny=False never asks."""
    import torch.nn as nn
    from mio import _nn, ops
    calls = []
    monkeypatch.setattr(ops, "gemm_skinny", lambda *a, **k: calls.append("skinny") or "S")
    monkeypatch.setattr(ops, "gemm_bias_act", lambda *a, **k: calls.append("plain") or "P")
    monkeypatch.setattr(ops, "blocked_weight_ok", lambda *a: False)
    asked = []
    monkeypatch.setattr(ops, "gemm_skinny_ok", lambda M, N, K, act="none": asked.append((M, N, K, act)) or N >= 256)
    cache, x = _nn.CastCache(), torch.zeros(2, 1, 64, dtype=torch.bfloat16)
    big, small = nn.Linear(64, 256).bfloat16(), nn.Linear(64, 128).bfloat16()
    assert _nn.linear(x, big, cache, torch.bfloat16) == "P" and asked == []
    assert _nn.linear(x, big, cache, torch.bfloat16, "gelu", skinny=True) == "S" and asked == [(2, 256, 64, "gelu")]
    assert _nn.linear(x, small, cache, torch.bfloat16, skinny=True) == "P"
    assert _nn.linear(x, big, cache, torch.bfloat16, skinny=True, col_scale=(0, 128, 2.0)) == "P"
    assert _nn.linear(x, big, cache, torch.bfloat16, skinny=True, x_blocked_shape=(2, 1, 64)) == "P"
    assert calls == ["plain", "skinny", "plain", "plain", "plain"]


def test_config_fields_default_off():
    from mio.kernels.attention import FlashAttentionConfig
    from mio.kernels.mlp import FusedMLPConfig
    assert FlashAttentionConfig().decode_gemm is False and FusedMLPConfig().decode_gemm is False
    assert FlashAttentionConfig(decode_gemm=True).decode_gemm and FusedMLPConfig(decode_gemm=True).decode_gemm

"""CPU-only tests of the host side of the decode-step GEMM on weight-only FP8, through the loaded library: the C-ABI symbols are
declared, exported and bound and the ABI version stays; every refusal of mio_gemm_skinny_w8 and mio_weight_quant_w8 returns before
a launch with a message under the entry point's name; an empty call returns 0; the workspace size follows the split count, the
split count never falls as K grows, the slices are whole 64-k steps that cover K; the advice admits no illegal shape and only the
measured regions; the module layer's switch; the GPU tests' case tables (tests/_w8_cases.py) reach the kernel's seams under the
plan and the tuning values the library holds; and the compiled unit's kernels fit 256 VGPRs without scratch.  Addresses are fake
and 16-byte aligned; nothing is dereferenced."""
import ctypes as C
import os
import re

import pytest
import torch

import _isa
import _w8_cases as wc

A = 1 << 20  # a fake 16-byte aligned device address
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"mio_weight_quant_w8": 9, "mio_gemm_skinny_w8_workspace_bytes": 4, "mio_gemm_skinny_w8_splits": 4,
           "mio_gemm_skinny_w8_slice": 7, "mio_gemm_skinny_w8_chunk_k": 1, "mio_gemm_skinny_w8_depth": 1,
           "mio_gemm_skinny_w8_ok": 4, "mio_gemm_skinny_w8": 20}  # name -> number of C arguments
SWIGLU = 5
SHAPES = [(M, N, K) for M in (1, 5, 16, 37, 64) for N in (1, 72, 1000, 3072, 14336) for K in (16, 48, 272, 1024, 2096, 4112, 14336)]


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
    assert lib.lib.mio_version() == 106 and "#define MIO_VERSION 106" in header  # additive: the ABI version stays
    doc = header[header.index("The decode-step GEMM on weight-only FP8"):header.index("int mio_weight_quant_w8")]
    assert "F.linear" in doc and "no quantised weights" in doc


# a legal call that splits K (M 4, N 1024, K 1024): every fault below is the only thing wrong with it
_G = dict(x=A, w8=A, w_scale=A, bias=None, w8_gate=None, w_scale_gate=None, bias_gate=None, residual=None, y=A, workspace=A, M=4,
          N=1024, K=1024, ldx=1024, ldw=1024, ldy=1024, ldr=0, act=0, dtype=0)


def _call(**fault):
    return _lib().lib.mio_gemm_skinny_w8(*dict(_G, **fault).values(), None)


@pytest.mark.parametrize("fault,words", [
    (dict(M=65), "at most 64"),
    (dict(M=-1), "negative"), (dict(N=-8), "negative"), (dict(K=-16), "negative"),
    (dict(K=1032, ldx=1032, ldw=1040), "K must be a multiple of 16"),
    (dict(ldw=1032), "ldw must be a multiple of 16 bytes"), (dict(ldw=1008), "ldw smaller than K"),
    (dict(ldx=1028), "multiples of 8"), (dict(ldy=1028), "multiples of 8"), (dict(residual=A, ldr=1028), "multiples of 8"),
    (dict(ldx=1016), "smaller than row length"), (dict(ldy=1016), "smaller than row length"),
    (dict(residual=A, ldr=8), "smaller than row length"),
    (dict(x=None), "non-null"), (dict(w8=None), "non-null"), (dict(y=None), "non-null"), (dict(w_scale=None), "non-null"),
    (dict(x=A + 8), "16-byte aligned"), (dict(w8=A + 2), "16-byte aligned"), (dict(y=A + 4), "16-byte aligned"),
    (dict(w_scale=A + 4), "16-byte aligned"), (dict(bias=A + 8), "16-byte aligned"),
    (dict(residual=A + 8, ldr=1024), "16-byte aligned"), (dict(workspace=A + 4), "16-byte aligned"),
    (dict(act=SWIGLU, w8_gate=A + 8, w_scale_gate=A), "16-byte aligned"),
    (dict(act=SWIGLU, w8_gate=A, w_scale_gate=A + 4), "16-byte aligned"),
    (dict(act=SWIGLU), "w8_gate and w_scale_gate"), (dict(act=SWIGLU, w8_gate=A), "w8_gate and w_scale_gate"),
    (dict(act=SWIGLU, w_scale_gate=A), "w8_gate and w_scale_gate"), (dict(w8_gate=A, w_scale_gate=A), "w8_gate and w_scale_gate"),
    (dict(w_scale_gate=A), "w8_gate and w_scale_gate"), (dict(bias_gate=A), "bias_gate"),
    (dict(act=6), "unknown activation"), (dict(act=-1), "unknown activation"),
    (dict(dtype=2), "bf16 or fp16"),
    (dict(workspace=None), "workspace required"),
])
def test_refusals(fault, words):
    lib = _lib().lib
    assert lib.mio_gemm_skinny_w8_splits(_G["M"], _G["N"], _G["K"], 0) > 1  # the neighbour is a legal call that splits
    assert _call(**fault) != 0
    assert _err().startswith("mio_gemm_skinny_w8: ") and words in _err(), _err()


_Q = dict(w=A, ldw=1024, w8=A, ldw8=1024, scale=A, N=64, K=1024, dtype=0)


@pytest.mark.parametrize("fault,words", [
    (dict(N=-1), "negative"), (dict(K=-16), "negative"), (dict(K=1032, ldw=1032, ldw8=1040), "multiple of 16"),
    (dict(dtype=2), "bf16 or fp16"), (dict(ldw=1028), "ldw must be"), (dict(ldw=1016), "ldw must be"),
    (dict(ldw8=1032), "ldw8 must be"), (dict(ldw8=1008), "ldw8 must be"),
    (dict(w=None), "non-null"), (dict(w8=None), "non-null"), (dict(scale=None), "non-null"),
    (dict(w=A + 8), "aligned"), (dict(w8=A + 8), "aligned"), (dict(scale=A + 2), "aligned"),
])
def test_quantiser_refusals(fault, words):
    lib = _lib().lib
    assert lib.mio_weight_quant_w8(*dict(_Q, **fault).values(), None) != 0
    assert _err().startswith("mio_weight_quant_w8: ") and words in _err(), _err()
    assert lib.mio_weight_quant_w8(*dict(_Q, N=0, w=None, w8=None, scale=None).values(), None) == 0  # an empty weight


def test_empty_and_queries_refuse():
    """M == 0 or N == 0 returns 0 whatever the data pointers; the host queries refuse what the launch refuses, and the advice is 0
    on every illegal shape."""
    lib = _lib().lib
    assert _call(M=0) == 0 and _call(M=0, x=None, y=None, workspace=None) == 0 and _call(N=0, ldy=0, workspace=None) == 0
    for M, N, K, act, words in [(65, 8, 16, 0, "at most 64"), (-1, 8, 16, 0, "negative"), (4, 8, 24, 0, "multiple of 16"),
                                (4, 8, 16, 7, "unknown activation")]:
        assert lib.mio_gemm_skinny_w8_splits(M, N, K, act) < 0
        assert _err().startswith("mio_gemm_skinny_w8_splits: ") and words in _err(), _err()
        assert lib.mio_gemm_skinny_w8_ok(M, N, K, act) == 0
        assert lib.mio_gemm_skinny_w8_workspace_bytes(M, N, K, act) == 0
        kb, ke = C.c_int32(), C.c_int32()
        assert lib.mio_gemm_skinny_w8_slice(M, N, K, act, 0, C.byref(kb), C.byref(ke)) < 0
    for M, N, K, act in [(0, 8192, 8192, 0), (65, 8192, 8192, 0), (4, 8192, 8200, 0), (4, 0, 8192, 0), (4, 8192, 0, 0),
                         (4, 14336, 4096, 6), (-4, 14336, 4096, SWIGLU)]:
        assert lib.mio_gemm_skinny_w8_ok(M, N, K, act) == 0, (M, N, K, act)


@pytest.mark.parametrize("act", [0, 1, SWIGLU])
def test_workspace_follows_splits(act):
    lib = _lib().lib
    split = 0
    for M, N, K in SHAPES:
        n = lib.mio_gemm_skinny_w8_splits(M, N, K, act)
        assert n >= 1, (M, N, K)
        want = 0 if n == 1 else n * M * N * 4 * (2 if act == SWIGLU else 1)
        assert lib.mio_gemm_skinny_w8_workspace_bytes(M, N, K, act) == want, (M, N, K)
        split += n > 1
    assert split > 0 and split < len(SHAPES)  # both kinds are among the shapes


def test_splits_monotone_in_k():
    lib = _lib().lib
    for M in (1, 4, 16, 17, 64):
        for N in (8, 1000, 1024, 4096, 14336):
            last = 0
            for K in range(16, 16400, 16):
                n = lib.mio_gemm_skinny_w8_splits(M, N, K, 0)
                assert n >= last, (M, N, K, n, last)
                last = n
            assert last > 1


def test_slices_cover_k_in_whole_steps():
    """Slice s is [k_begin, k_end): they tile [0, K) in order, none is empty, every begin is a multiple of 64 and every length is
    too (the last slice ends at K, a multiple of 16), two lengths differ by one step at most, and with several slices none is
    shorter than 16 M: the fp32 partials written stay at or under 1/4 of the weight bytes read."""
    lib = _lib().lib
    for M, N, K in SHAPES + [(3, 8, 2096), (64, 264, 1024), (37, 72, 16)]:
        n = lib.mio_gemm_skinny_w8_splits(M, N, K, 0)
        at, steps = 0, []
        for s in range(n):
            kb, ke = C.c_int32(-1), C.c_int32(-1)
            assert lib.mio_gemm_skinny_w8_slice(M, N, K, 0, s, C.byref(kb), C.byref(ke)) == 0
            assert kb.value == at and kb.value % 64 == 0 and ke.value > kb.value, (M, N, K, s)
            assert (ke.value - kb.value) % 64 == 0 or ke.value == K, (M, N, K, s)
            steps.append(-(-(ke.value - kb.value) // 64))
            if n > 1:
                assert steps[-1] * 64 >= 16 * M, (M, N, K, s)
            at = ke.value
        assert at == K and max(steps) - min(steps) <= 1, (M, N, K, steps)
        kb, ke = C.c_int32(), C.c_int32()
        assert lib.mio_gemm_skinny_w8_slice(M, N, K, 0, n, C.byref(kb), C.byref(ke)) != 0
        assert _err().startswith("mio_gemm_skinny_w8_slice: ")


def test_tuning_queries():
    """k per chunk and register sets in the ring, per activation; an unknown activation is refused."""
    lib = _lib().lib
    for fn, name in ((lib.mio_gemm_skinny_w8_chunk_k, "chunk_k"), (lib.mio_gemm_skinny_w8_depth, "depth")):
        vals = [fn(a) for a in range(SWIGLU + 1)]
        assert len(set(vals[:SWIGLU])) == 1 and min(vals) > 0, (name, vals)
        for act in (-1, SWIGLU + 1):
            assert fn(act) < 0
            assert _err() == f"mio_gemm_skinny_w8_{name}: unknown activation"
    assert all(lib.mio_gemm_skinny_w8_chunk_k(a) % 64 == 0 for a in (0, SWIGLU))  # whole 64-k steps
    assert all(lib.mio_gemm_skinny_w8_depth(a) >= 2 for a in (0, SWIGLU))


def _chunks(c):
    """Chunks per slice of case c under the loaded library's plan: one entry per slice."""
    lib, act = _lib().lib, wc.ACTS.index(c.act)
    n, per = lib.mio_gemm_skinny_w8_splits(c.M, c.N, c.K, act), lib.mio_gemm_skinny_w8_chunk_k(act)
    assert n >= 1 and per > 0, (c, _err())
    out = []
    for s in range(n):
        kb, ke = C.c_int32(), C.c_int32()
        assert lib.mio_gemm_skinny_w8_slice(c.M, c.N, c.K, act, s, C.byref(kb), C.byref(ke)) == 0, (c, _err())
        out.append(-(-(ke.value - kb.value) // per))
    return out


def test_case_tables_reach_the_seams():
    """What tests/test_gpu_gemm_skinny_w8.py runs, under the plan and tuning values as they are now.  Every case splits K or not
    as its table says; the tables were laid out for the chunk length and ring depth the library reports; the deep cases reach,
    for plain and SwiGLU and for each count of row fragments, one slice of depth + 1, of depth + 2 and of depth + 3 chunks, and
    several slices of more than depth chunks with unequal counts (at M 1 too); the ragged-N cases write partials; the K tails
    cover K % 64 in {16, 32, 48} behind a split.  A requirement nobody meets is reported with the chunk counts of its table's
    cases of that kind."""
    lib = _lib().lib
    assert wc.ACTS.index("swiglu") == SWIGLU == _lib().ACT_SWIGLU and wc.ACTS.index("none") == 0
    depth = {glu: lib.mio_gemm_skinny_w8_depth(SWIGLU if glu else 0) for glu in (False, True)}
    chunk = {glu: lib.mio_gemm_skinny_w8_chunk_k(SWIGLU if glu else 0) for glu in (False, True)}
    assert (chunk, depth) == (wc.CHUNK_K, wc.DEPTH), f"tests/_w8_cases.py is laid out for {wc.CHUNK_K} / {wc.DEPTH}: {chunk} / {depth}"
    chunks = {c: _chunks(c) for t in wc.TABLES.values() for c in t}
    wrong = [(name, c.what, chunks[c]) for name, t in wc.TABLES.items() for c in t if (len(chunks[c]) > 1) != c.split]
    assert not wrong, f"the plan splits K otherwise than these cases say: {wrong}"
    missing = []

    def need(table, glu, text, pred):
        mine = [c for c in wc.TABLES[table] if c.glu == glu]
        if not any(pred(c, chunks[c]) for c in mine):
            missing.append(f"{table}: no {'SwiGLU' if glu else 'plain'} case with {text}; its cases: "
                           + ", ".join(f"{c.what} -> {chunks[c]}" for c in mine))

    for glu in (False, True):
        d = depth[glu]

        def deep(ch):  # several slices, each past the ring's depth, of unequal chunk counts
            return len(ch) > 1 and min(ch) > d and len(set(ch)) > 1

        for mf in (1, 2, 3, 4):
            for extra in (1, 2, 3):
                need("DEEP_UNSPLIT", glu, f"MF {mf}, one slice of depth + {extra} = {d + extra} chunks",
                     lambda c, ch: c.mf == mf and ch == [d + extra])
            need("DEEP_SPLIT", glu, f"MF {mf}, slices of more than {d} chunks, unequal", lambda c, ch: c.mf == mf and deep(ch))
            need("DEEP_SPLIT", glu, f"MF {mf}, a full last fragment, slices of more than {d} chunks",
                 lambda c, ch: c.mf == mf and c.M % 16 == 0 and len(ch) > 1 and min(ch) > d)
        need("DEEP_SPLIT", glu, f"M 1, slices of more than {d} chunks, unequal", lambda c, ch: c.M == 1 and deep(ch))
        for text, ok in (("N 1", lambda N: N == 1), ("1 < N < 16", lambda N: 1 < N < 16), ("48 < N < 64", lambda N: 48 < N < 64),
                         ("N > 64", lambda N: N > 64)):
            need("N_EDGES_SPLIT", glu, f"several slices, N % 4 != 0, {text}", lambda c, ch: len(ch) > 1 and c.N % 4 != 0 and ok(c.N))
        for table in ("STRIDES", "ROW_SLICE", "ZERO_SCALE", "POISONED", "EVERY_ACTIVATION"):
            for split in (False, True):
                need(table, glu, f"{'several slices' if split else 'one slice'}", lambda c, ch: (len(ch) > 1) == split)
    for tail in (16, 32, 48):
        need("K_TAILS_AND_SPLITS", False, f"several slices, K % 64 == {tail}", lambda c, ch: len(ch) > 1 and c.K % 64 == tail)
    need("K_TAILS_AND_SPLITS", False, "K 16", lambda c, ch: c.K == 16)
    assert not missing, "\n".join(missing)
    for c in wc.DEEP_UNSPLIT + wc.DEEP_SPLIT:  # nothing shallow among the deep, and within the K the borrowed bars judge
        assert min(chunks[c]) > depth[c.glu] and c.K <= 4112, (c.what, chunks[c])
    assert all(c.N == wc.DEEP_N and c.K <= wc.DEEP_LDW for c in wc.DEEP_UNSPLIT)
    assert all(c.K % 16 == 0 and (c.ldw is None or (c.ldw % 16 == 0 and c.ldw > c.K)) for t in wc.TABLES.values() for c in t)


def test_ops_queries():
    from mio import ops
    assert ops.gemm_skinny_w8_splits(4, 1024, 1024) == _lib().lib.mio_gemm_skinny_w8_splits(4, 1024, 1024, 0) > 1
    assert ops.gemm_skinny_w8_splits(37, 72, 48, "gelu") == 1
    with pytest.raises(ValueError, match="at most 64"):
        ops.gemm_skinny_w8_splits(65, 1024, 1024)
    with pytest.raises(ValueError, match="multiple of 16"):
        ops.gemm_skinny_w8_splits(4, 1024, 1032)
    with pytest.raises(ValueError, match="Unsupported activation"):
        ops.gemm_skinny_w8_splits(4, 1024, 1024, "tanh")
    assert ops.gemm_skinny_w8_ok(65, 8192, 8192) is False and ops.gemm_skinny_w8_ok(4, 8192, 8192, "tanh") is False
    # the regions of the measured sweep (profiles/skinny_gemm_w8.md), and nothing below the smallest weight that qualified
    assert all(ops.gemm_skinny_w8_ok(M, N, K, a) for M in (1, 16, 64) for N, K in ((6144, 4096), (4096, 14336)) for a in ("none", "gelu"))
    assert ops.gemm_skinny_w8_ok(16, 4096, 4096) and not ops.gemm_skinny_w8_ok(17, 4096, 4096)
    assert all(ops.gemm_skinny_w8_ok(M, 14336, 4096, "swiglu") for M in (1, 16, 64))
    assert not ops.gemm_skinny_w8_ok(1, 4096, 4096, "swiglu")
    assert not any(ops.gemm_skinny_w8_ok(M, N, K) for M in (1, 8, 16, 64) for N, K in ((1024, 1024), (3072, 1024), (1024, 4096)))


def test_ops_argument_checks(monkeypatch):
    """The checks of ops.gemm_skinny_w8 and ops.quantize_weight_w8 with the device check out of the way (each call is refused
    before a launch): wrong weight and scale dtypes are a ValueError that names float8_e4m3fn, as the KV-cache ops'."""
    from mio import ops
    fp8, bf = torch.float8_e4m3fn, torch.bfloat16
    x, w = torch.zeros(4, 64, dtype=bf), torch.zeros(128, 64, dtype=bf)
    q, s = torch.zeros(128, 64, dtype=torch.uint8).view(fp8), torch.ones(128)
    with pytest.raises(ValueError, match="CUDA"):
        ops.gemm_skinny_w8(x, q, s)
    with pytest.raises(ValueError, match="CUDA"):
        ops.quantize_weight_w8(w)
    monkeypatch.setattr(ops, "_need_cuda", lambda *ts: None)
    for bad in (w, q.view(torch.uint8), q.view(torch.float8_e5m2), q.view(torch.int8)):
        with pytest.raises(ValueError, match="float8_e4m3fn"):
            ops.gemm_skinny_w8(x, bad, s)
    for bad in (s.to(bf), s.double(), None):
        with pytest.raises(ValueError, match="float8_e4m3fn"):
            ops.gemm_skinny_w8(x, q, bad)
    with pytest.raises(ValueError, match="swiglu|gate", ):
        ops.gemm_skinny_w8(x, q, s, activation="swiglu", w8_gate=q)
    with pytest.raises(ValueError, match="float8_e4m3fn"):
        ops.gemm_skinny_w8(x, q, s, activation="swiglu", w8_gate=w, w_scale_gate=s)
    with pytest.raises(ValueError, match="Unsupported activation"):
        ops.gemm_skinny_w8(x, q, s, activation="tanh")
    with pytest.raises(ValueError, match="bf16 or fp16"):
        ops.gemm_skinny_w8(x.float(), q, s)
    with pytest.raises(ValueError, match="does not match input features"):
        ops.gemm_skinny_w8(x, q[:, :32], s)
    with pytest.raises(ValueError, match="multiple of 16"):
        ops.gemm_skinny_w8(x[:, :40], q[:, :40], s)
    with pytest.raises(ValueError, match="128 elements"):
        ops.gemm_skinny_w8(x, q, s[:64])
    with pytest.raises(ValueError, match="at most 64 rows"):
        ops.gemm_skinny_w8(torch.zeros(5, 13, 64, dtype=bf), q, s)
    with pytest.raises(ValueError, match="bf16 or fp16"):
        ops.quantize_weight_w8(w.float())
    with pytest.raises(ValueError, match="multiple of 16"):
        ops.quantize_weight_w8(w[:, :40])
    assert ops._w8_scale(torch.full((1,), 0.5), 128, "w_scale").tolist() == [0.5] * 128  # a per-tensor scale, expanded
    assert ops._w8_ok(q[:40], "w8").data_ptr() == q.data_ptr() and ops._w8_scale(s[:40], 40, "w_scale").data_ptr() == s.data_ptr()


def test_linear_takes_the_kernel_only_when_asked_and_advised(monkeypatch):
    """mio._nn.linear: skinny_w8=True goes to ops.gemm_skinny_w8 (on CastCache.get_w8's copy) only without a blocked x, without
    a column scale and where ops.gemm_skinny_w8_ok holds; anywhere else the call runs as skinny= says; skinny_w8=False never asks."""
    import torch.nn as nn
    from mio import _nn, ops
    calls, asked = [], []
    monkeypatch.setattr(ops, "gemm_skinny_w8", lambda *a, **k: calls.append("w8") or "W")
    monkeypatch.setattr(ops, "gemm_skinny", lambda *a, **k: calls.append("skinny") or "S")
    monkeypatch.setattr(ops, "gemm_bias_act", lambda *a, **k: calls.append("plain") or "P")
    monkeypatch.setattr(ops, "blocked_weight_ok", lambda *a: False)
    monkeypatch.setattr(ops, "quantize_weight_w8", lambda w: ("q", "s"))
    monkeypatch.setattr(ops, "gemm_skinny_ok", lambda M, N, K, act="none": True)
    monkeypatch.setattr(ops, "gemm_skinny_w8_ok", lambda M, N, K, act="none": asked.append((M, N, K, act)) or N >= 256)
    cache, x = _nn.CastCache(), torch.zeros(2, 1, 64, dtype=torch.bfloat16)
    big, small = nn.Linear(64, 256).bfloat16(), nn.Linear(64, 128).bfloat16()
    bf = torch.bfloat16
    assert _nn.linear(x, big, cache, bf) == "P" and _nn.linear(x, big, cache, bf, skinny=True) == "S" and asked == []
    assert _nn.linear(x, big, cache, bf, "gelu", skinny_w8=True) == "W" and asked == [(2, 256, 64, "gelu")]
    assert _nn.linear(x, small, cache, bf, skinny_w8=True) == "P" and _nn.linear(x, small, cache, bf, skinny=True, skinny_w8=True) == "S"
    assert _nn.linear(x, big, cache, bf, skinny_w8=True, col_scale=(0, 128, 2.0)) == "P"
    assert _nn.linear(x, big, cache, bf, skinny_w8=True, x_blocked_shape=(2, 1, 64)) == "P"
    assert calls == ["plain", "skinny", "w8", "plain", "skinny", "plain", "plain"]


def test_cast_cache_requantises_on_a_new_version(monkeypatch):
    import torch.nn as nn
    from mio import _nn, ops
    made = []
    monkeypatch.setattr(ops, "quantize_weight_w8", lambda w: made.append(w.clone()) or (len(made), "s"))
    cache, lin = _nn.CastCache(), nn.Linear(64, 32).bfloat16()
    assert cache.get_w8(lin.weight, torch.bfloat16) == (1, "s") and cache.get_w8(lin.weight, torch.bfloat16) == (1, "s")
    with torch.no_grad():
        lin.weight.mul_(2)
    assert cache.get_w8(lin.weight, torch.bfloat16) == (2, "s") and torch.equal(made[1], made[0] * 2)
    assert cache.get_w8(lin.weight, torch.float16) == (3, "s") and made[2].dtype == torch.float16  # the dtype is part of the key


def test_config_fields_default_off():
    from mio.kernels.attention import FlashAttentionConfig
    from mio.kernels.mlp import FusedMLPConfig
    assert FlashAttentionConfig().decode_gemm_fp8 is False and FusedMLPConfig().decode_gemm_fp8 is False
    assert FlashAttentionConfig(decode_gemm_fp8=True).decode_gemm_fp8 and FusedMLPConfig(decode_gemm_fp8=True).decode_gemm_fp8


def test_kernels_fit_256_vgprs_without_scratch(tmp_path):
    """The compiled unit's kernel metadata: every instance of the GEMM kernel (2 dtypes x 4 row-fragment counts x plain / SwiGLU),
    the scaled reduction and the quantiser use no scratch, spill nothing and stay within 256 VGPRs."""
    text = _isa.device_isa(tmp_path, "gemm_skinny_w8.hip", [], attention=False).read_text()
    for name_re, count in ((r"_Z21gemm_skinny_w8_kernel\w+", 16), (r"_Z25gemm_skinny_reduce_kernel\w+", 4),
                           (r"_Z22weight_quant_w8_kernel\w+", 2)):
        blocks = _isa.metadata(text, name_re)
        assert len(blocks) == count, (name_re, len(blocks))
        for blk in blocks:
            _isa.check_fits_256(blk)

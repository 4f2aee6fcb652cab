"""The host side of the mixture-of-experts decode step on FP8 expert weights, without a GPU: the C ABI's symbols and refusals through
dummy aligned pointers (every refusal comes before any launch, nothing is dereferenced) and the plan under the one-byte form."""
import os
import re

import pytest

from test_moe_host import A, ROOT, _err, _lib

# the launches' arguments in call order, a legal value each (T 4, k 2, E 8; up: I 72, d 1040, SwiGLU; down: d 40, I 80); stream last
UP = ("mio_moe_up_w8", dict(x=A, w=A, s=A, b=None, wg=A, sg=A, bg=None, off=A, srt=A, h=A, ws=A, T=4, k=2, E=8, I=72, d=1040, ldx=1040,
                            ldw=1040, es=72 * 1040, ldh=72, act=5, dtype=0))
DOWN = ("mio_moe_down_w8", dict(h=A, w=A, s=A, b=None, ids=A, wts=A, off=A, pos=A, res=None, y=A, ws=A, T=4, k=2, E=8, d=40, I=80, ldh=80,
                                ldw=80, es=40 * 80, ldy=40, ldr=40, dtype=0))


def _call(entry, **kw):
    return getattr(_lib().lib, entry[0])(*{**entry[1], **kw}.values(), None)


def test_symbols_declared_and_bound():
    lib = _lib()
    header = open(os.path.join(ROOT, "include", "mio_hip.h")).read()
    for s in [f"mio_moe_{side}_w8{q}" for side in ("up", "down") for q in ("", "_splits", "_workspace_bytes")]:
        assert re.search(r"\b%s\(" % s, header), f"{s} is not declared in include/mio_hip.h"
        assert s in lib.EXPORTS and hasattr(lib.lib, s)
    from mio import ops
    from mio.kernels.mlp import MoEConfig
    assert all(hasattr(ops, n) for n in ("quantize_expert_weights_w8", "moe_up_w8", "moe_down_w8", "moe_mlp_w8", "moe_up_w8_splits",
                                         "moe_down_w8_splits")) and MoEConfig().expert_weights_fp8 is False


REFUSALS = [
    (UP, dict(d=1032, ldx=1040), "K must be a multiple of 16"), (UP, dict(ldw=1048, es=72 * 1048), "multiples of 16 bytes"),
    (UP, dict(es=72 * 1040 + 8), "multiples of 16 bytes"), (UP, dict(ldw=1024), "row stride smaller"),
    (UP, dict(es=72 * 1040 - 16), "expert_stride"), (UP, dict(s=None), "s_up"), (UP, dict(sg=None), "s_gate"),
    (UP, dict(wg=None), "s_gate"), (UP, dict(act=0), "w8_gate"), (UP, dict(act=0, wg=None, sg=None, bg=A), "b_gate"),
    (UP, dict(dtype=2), "dtype"), (UP, dict(dtype=3), "dtype"), (UP, dict(T=65), "decode steps only"), (UP, dict(E=300), "E must be"),
    (UP, dict(k=9), "top_k"), (UP, dict(ldx=1036), "multiples of 8"), (UP, dict(ldh=64), "row stride smaller"),
    (UP, dict(x=A + 8), "aligned"), (UP, dict(s=A + 2), "aligned"), (UP, dict(ws=None), "workspace required"),
    (UP, dict(act=6), "activation"), (UP, dict(h=None), "non-null"), (UP, dict(T=-1), "negative"),
    (DOWN, dict(I=72, ldh=80), "K must be a multiple of 16"), (DOWN, dict(ldw=88, es=40 * 88), "multiples of 16 bytes"),
    (DOWN, dict(es=40 * 80 + 8), "multiples of 16 bytes"), (DOWN, dict(ldw=64), "row stride smaller"),
    (DOWN, dict(es=40 * 80 - 16), "expert_stride"), (DOWN, dict(s=None), "s_down"), (DOWN, dict(dtype=2), "dtype"),
    (DOWN, dict(T=65), "decode steps only"), (DOWN, dict(E=0), "E must be"), (DOWN, dict(k=3, E=2), "top_k"),
    (DOWN, dict(ldy=36), "multiples of 8"), (DOWN, dict(ldy=32), "row stride smaller"), (DOWN, dict(res=A, ldr=32), "ldr"),
    (DOWN, dict(y=A + 4), "aligned"), (DOWN, dict(ws=None), "workspace required"), (DOWN, dict(ids=None), "non-null"),
]


@pytest.mark.parametrize("i", range(len(REFUSALS)))
def test_refusals_before_any_launch(i):
    entry, kw, text = REFUSALS[i]
    assert _call(entry, **kw) < 0, (entry[0], kw)
    assert _err().startswith(entry[0] + ":") and text in _err(), (kw, _err())


def test_empty_calls_and_queries():
    lib = _lib().lib
    assert _call(UP, T=0, x=None, h=None, off=None, srt=None, ws=None) == 0 and _call(UP, I=0, ldh=0, es=0, ws=None) == 0
    assert _call(DOWN, T=0, h=None, y=None, ids=None, wts=None, off=None, pos=None, ws=None) == 0 and _call(DOWN, d=0, ldy=0, es=0, ws=None) == 0
    assert lib.mio_moe_up_w8_splits(4, 2, 8, 72, 40, 5) < 0 and _err().startswith("mio_moe_up_w8_splits:") and "multiple of 16" in _err()
    assert lib.mio_moe_down_w8_splits(65, 2, 8, 72, 48) < 0 and "decode steps only" in _err()
    assert lib.mio_moe_up_w8_workspace_bytes(4, 9, 8, 72, 48, 5) == 0 and "top_k" in _err()
    assert lib.mio_moe_down_w8_workspace_bytes(4, 2, 0, 72, 48) == 0 and "E must be" in _err()
    assert lib.mio_moe_up_w8_splits(4, 2, 8, 72, 0, 5) == 1  # K == 0: one slice, as mio_gemm_skinny_w8_splits
    from mio import ops
    with pytest.raises(ValueError):
        ops.moe_down_w8_splits(4, 2, 8, 72, 40)


@pytest.mark.parametrize("act", [0, 5])
def test_plan_properties_fp8_form(act):
    """Slices of whole 64-k steps (slice s: steps [s steps / n, (s + 1) steps / n)), none empty, at most one step apart, the count never
    falling as K grows nor above what 512 workgroups ask for; each at least 16 x the mean rows per aimed expert, so the fp32 partials
    stay at or under 1/4 of the aimed experts' one-byte weight bytes; the workspace formulas; at E = 1, k = 1 mio_gemm_skinny_w8's plan."""
    lib = _lib().lib
    for T, k, E, N in [(T, k, E, N) for T in (1, 4, 17, 64) for k, E in ((1, 1), (2, 8), (4, 60), (8, 128), (8, 256), (1, 256))
                       for N in (1, 72, 1000, 14336)]:
        aimed = max(1, min(E, T * k))
        min_len = max(64, (16 * -(-T * k // aimed) + 63) // 64 * 64)
        last = 0
        for K in (0, 16, 48, 64, 80, 272, 1040, 2048, 4096, 14336):
            ns = lib.mio_moe_up_w8_splits(T, k, E, N, K, act)
            assert ns >= 1 and ns == lib.mio_moe_down_w8_splits(T, k, E, N, K) and ns >= last, (T, k, E, N, K, ns, last)
            last = ns
            steps = -(-K // 64)
            lens = [(s + 1) * steps // ns - s * steps // ns for s in range(ns)]
            assert K == 0 or (min(lens) >= 1 and max(lens) - min(lens) <= 1), (T, k, E, N, K, lens)
            if ns > 1:
                assert K // ns >= min_len - 63 and ns <= K // min_len and ns <= -(-512 // (aimed * -(-N // 64)))
                assert 4 * (4 * T * k * N * ns) <= aimed * N * K, (T, k, E, N, K, ns)  # partials <= 1/4 of the aimed experts' bytes
            assert lib.mio_moe_up_w8_workspace_bytes(T, k, E, N, K, act) == (0 if ns == 1 else ns * T * k * N * 4 * (2 if act == 5 else 1))
            assert lib.mio_moe_down_w8_workspace_bytes(T, k, E, N, K) == ns * T * k * N * 4
            if (k, E) == (1, 1):
                assert ns == lib.mio_gemm_skinny_w8_splits(T, N, K, act), (T, N, K)

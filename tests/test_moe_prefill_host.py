"""The host side of the mixture-of-experts path for tall inputs, without a GPU: the symbols, the bound on the tile map against
every split of the routed rows over the experts, the workspace size and the refusals (all before any launch)."""
import itertools
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BM = 128
A = 0x1000  # a dummy 16-byte aligned address: nothing is dereferenced before a refusal


def _lib():
    from mio import _lib
    return _lib


def test_symbols_and_ops():
    L = _lib()
    header = open(os.path.join(ROOT, "include", "mio_hip.h")).read()
    for s in ("mio_moe_prefill_route", "mio_moe_prefill_max_tiles", "mio_moe_prefill_up", "mio_moe_prefill_down",
              "mio_moe_prefill_down_workspace_bytes"):
        assert re.search(r"\b%s\(" % s, header) and s in L.EXPORTS and hasattr(L.lib, s), s
    from mio import ops
    from mio.kernels.mlp import MoEConfig
    assert ops.MOE_PREFILL_MAX_TOKENS == 8192 and MoEConfig().grouped_prefill is False
    assert ops.MoEPrefillRoute._fields[:7] == ops.MoERoute._fields
    for name in ("moe_route_prefill", "moe_up_prefill", "moe_down_prefill", "moe_mlp_prefill", "moe_prefill_max_tiles"):
        assert hasattr(ops, name)


@pytest.mark.parametrize("E", [1, 2, 3])
def test_max_tiles_bounds_every_split(E):
    """floor(T k / BM) + min(E, T k) is at least the tile count of every way to split the routed rows over the experts (no expert
    above T rows; three experts: up to 64 tokens); the workspace is 4 T k N bytes."""
    lib = _lib().lib
    for T, k in ((1, 1), (2, 1), (64, 2), (127, 1), (128, 1), (129, 2), (200, 2), (300, 3), (385, 1)):
        if k > E:
            continue
        bound = lib.mio_moe_prefill_max_tiles(T, k, E)
        assert bound == T * k // BM + min(E, T * k)
        most = max(sum(-(-c // BM) for c in cnt) for cnt in itertools.product(range(T + 1), repeat=E) if sum(cnt) == T * k) \
            if E < 3 or T <= 64 else None
        assert most is None or most <= bound
        assert lib.mio_moe_prefill_down_workspace_bytes(T, k, E, 72, 136) == 4 * T * k * 72
    assert lib.mio_moe_prefill_max_tiles(8192, 8, 256) == 512 + 256 and lib.mio_moe_prefill_max_tiles(0, 1, 1) == 0


def _route(**kw):
    a = dict(logits=A, ld=8, T=70, E=8, k=2, dtype=0, tiles=A)
    a.update(kw)
    return _lib().lib.mio_moe_prefill_route(a["logits"], a["ld"], A, A, A, A, A, a["tiles"], A, A, a["T"], a["E"], a["k"], 1, a["dtype"], None)


def _up(**kw):
    a = dict(x=A, wg=A, T=70, k=2, E=8, I=72, d=1032, ldx=1032, ldw=1032, es=72 * 1032, ldh=72, act=5, dtype=0, nt=A)
    a.update(kw)
    return _lib().lib.mio_moe_prefill_up(a["x"], A, None, a["wg"], None, A, A, A, A, a["nt"], A, a["T"], a["k"], a["E"], a["I"], a["d"],
                                         a["ldx"], a["ldw"], a["es"], a["ldh"], a["act"], a["dtype"], None)


def _down(**kw):
    a = dict(y=A, ws=A, res=None, T=70, k=2, E=8, d=40, I=72, ldh=72, ldw=72, es=40 * 72, ldy=40, ldr=40, dtype=0)
    a.update(kw)
    return _lib().lib.mio_moe_prefill_down(A, A, None, A, A, A, A, A, A, A, a["res"], a["y"], a["ws"], a["T"], a["k"], a["E"], a["d"],
                                           a["I"], a["ldh"], a["ldw"], a["es"], a["ldy"], a["ldr"], a["dtype"], None)


REFUSALS = [
    (_route, dict(T=8193), "T must be at most 8192"), (_route, dict(E=257, ld=257), "E must be"), (_route, dict(k=9, E=16, ld=16), "top_k"),
    (_route, dict(k=4, E=3), "top_k"), (_route, dict(ld=7), "ld < E"), (_route, dict(dtype=3), "dtype"), (_route, dict(logits=A + 2), "aligned"),
    (_route, dict(tiles=None), "null"), (_route, dict(T=-1), "negative"),
    (_up, dict(T=8193), "T must be at most 8192"), (_up, dict(k=9), "top_k"), (_up, dict(d=1036, ldx=1040, ldw=1040), "K must be a multiple of 8"),
    (_up, dict(ldw=1024), "row stride smaller"), (_up, dict(ldx=1028), "multiples of 8"), (_up, dict(es=72 * 1032 - 8), "expert_stride"),
    (_up, dict(x=A + 8), "aligned"), (_up, dict(wg=None), "w_gate"), (_up, dict(act=0), "w_gate"), (_up, dict(dtype=2), "dtype"),
    (_up, dict(act=6), "activation"), (_up, dict(nt=None), "non-null"),
    (_down, dict(T=8193), "T must be at most 8192"), (_down, dict(k=3, E=2), "top_k"), (_down, dict(I=76, ldh=80, ldw=80, es=40 * 80), "K must be a multiple of 8"),
    (_down, dict(ldy=36), "multiples of 8"), (_down, dict(res=A, ldr=32), "ldr"), (_down, dict(y=A + 4), "aligned"),
    (_down, dict(ws=None), "workspace required"),
]


@pytest.mark.parametrize("i", range(len(REFUSALS)))
def test_refusals(i):
    fn, kw, text = REFUSALS[i]
    assert fn(**kw) < 0
    err = _lib().lib.mio_last_error().decode()
    assert err.startswith("mio_moe_prefill_" + fn.__name__[1:]) and text in err, err


def test_empty_calls_return_zero():
    assert _route(T=0) == 0 and _up(T=0) == 0 and _down(T=0, ws=None) == 0

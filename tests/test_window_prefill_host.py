"""CPU-only tests of sliding-window prefill (mio_fa3_{fwd,route}_window and their varlen / paged forms): the symbols are
bound, the windowed routes over a grid of geometries, every refusal at the C level and in ops, (-1, -1) equal to the
unwindowed routes, and the ISA bars of the windowed fwd5 (256 VGPRs, no scratch) and fwd3 (accumulator registers untouched,
no spill) kernels."""
import ctypes as C

import pytest
import torch

import _isa
from test_host_logic import _fa_params
from test_paged_host import _params as _paged_params
from test_varlen_host import _params as _varlen_params

NAMES = ("mio_fa3_fwd_window", "mio_fa3_route_window", "mio_fa3_fwd_varlen_window", "mio_fa3_varlen_route_window",
         "mio_fa3_fwd_paged_window", "mio_fa3_paged_route_window")


def _lib():
    from mio import _lib
    return _lib


def _dense(w, **kw):
    L = _lib()
    r = L.lib.mio_fa3_route_window(C.byref(_fa_params(**kw)), *w)
    return L.FA3_ROUTES.get(r) if r >= 0 else None


def _err():
    return _lib().lib.mio_last_error().decode()


def test_prefill_window_symbols_bound():
    L = _lib()
    for n in NAMES:
        assert n in L.EXPORTS and hasattr(L.lib, n)
    assert L.lib.mio_version() == 106


@pytest.mark.parametrize("Sq", [1, 77, 128, 129, 4096])
@pytest.mark.parametrize("D", [64, 80, 128])
@pytest.mark.parametrize("causal", [0, 1])
def test_dense_window_routes(Sq, D, causal):
    want = "fwd5" if D <= 64 else "fwd3"
    for w in ((0, 0), (63, 0), (4095, 0), (-1, 0), (100, -1)):
        assert _dense(w, Sq=Sq, Sk=300, D=D, causal=causal) == want
    if not causal:
        assert _dense((256, 256), Sq=Sq, D=D) == want
    # (-1, -1): the unwindowed route (fwd1 for Sq <= 128)
    assert _dense((-1, -1), Sq=Sq, Sk=300, D=D, causal=causal) == \
        _lib().FA3_ROUTES[_lib().lib.mio_fa3_route(C.byref(_fa_params(Sq=Sq, Sk=300, D=D, causal=causal)))]
    assert _dense((5, 0), Sq=0, D=D) == "empty"
    assert _dense((5, 0), Sq=Sq, Sk=0, D=D) == "fwd1"  # no key to window


@pytest.mark.parametrize("kw,msg", [
    (dict(mask_kind=1), "mask"), (dict(o_acc=True), "ring carry"), (dict(o_acc=True, carry_in=1), "ring carry"),
    (dict(row=1 << 27, Sk=300), "4 GiB"),
])
def test_dense_window_refusals(kw, msg):
    assert _dense((10, 0), **kw) is None and msg in _err()
    assert _dense((-1, -1), **kw) is not None or "4 GiB" not in _err()


def test_dense_window_value_refusals():
    assert _dense((-2, 0)) is None and "window values" in _err()
    assert _dense((0, -2)) is None and "window values" in _err()
    assert _dense((10, 1), causal=1) is None and "causal" in _err()
    assert _dense((10, 0), causal=1) == "fwd5" and _dense((10, -1), causal=1) == "fwd5"


@pytest.mark.parametrize("form", ["varlen", "paged"])
def test_seq_window_routes_and_refusals(form):
    L = _lib()
    mk = _varlen_params if form == "varlen" else _paged_params
    route = L.lib.mio_fa3_varlen_route_window if form == "varlen" else L.lib.mio_fa3_paged_route_window
    names = L.FA3_VARLEN_ROUTES if form == "varlen" else L.FA3_PAGED_ROUTES
    for D, want in ((64, "fwd5"), (80, "fwd3"), (128, "fwd3")):
        for w in ((0, 0), (1023, 0), (-1, 0), (7, -1)):
            assert names[route(C.byref(mk(D=D)), *w)] == want
        assert names[route(C.byref(mk(D=D, causal=0)), 100, 100)] == want
    assert names[route(C.byref(mk(B=0)), 5, 0)] == "empty"
    assert route(C.byref(mk()), -1, -1) == (L.lib.mio_fa3_varlen_route if form == "varlen" else L.lib.mio_fa3_paged_route)(C.byref(mk()))
    assert route(C.byref(mk()), -2, 0) < 0 and "window values" in _err()
    assert route(C.byref(mk(causal=1)), 5, 3) < 0 and "causal" in _err()
    assert route(C.byref(mk(max_q=1 << 28)), 5, 0) < 0 and "2^28" in _err()


@pytest.mark.parametrize("ws", [(-2, -1), (1, -3), (1.5, 0), (1, 2, 3), None, (1 << 31, 0), (0, 1 << 32)])
def test_ops_window_refusals(ws):
    from mio import ops
    t = torch.zeros(1, 300, 4, 64, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="window"):
        ops.fa3_route(t, t, t, window_size=ws)
    with pytest.raises(ValueError, match="window"):
        ops.paged_attention_route(t, t, t, t, t, t, 16, 16, 0, window_size=ws)


def test_ops_window_combination_refusals():
    from mio import ops
    t = torch.zeros(1, 300, 4, 64, dtype=torch.bfloat16)
    m = torch.ones(1, 1, 300, 300, dtype=torch.bool)
    with pytest.raises(ValueError, match="causal"):
        ops.fa3_route(t, t, t, causal=True, window_size=(10, 5))
    with pytest.raises(ValueError, match="mask"):
        ops.fa3_route(t, t, t, keep_mask=m, window_size=(10, 0))
    with pytest.raises(ValueError, match="carry"):
        ops.fa3_route(t, t, t, carry_in=True, window_size=(10, 0))
    with pytest.raises(ValueError, match="k_prescaled"):
        ops.fa3_route(t, t, t, k_prescaled=True, window_size=(10, 0))
    assert ops.fa3_route(t, t, t, causal=True, window_size=(10, 0)) == "fwd5"
    assert ops.fa3_route(t, t, t, causal=True, window_size=(-1, -1)) == ops.fa3_route(t, t, t, causal=True)


@pytest.mark.parametrize("type_id", [0, 1])
@pytest.mark.parametrize("D", [64, 96, 128])
def test_windowed_kernels_isa(tmp_path, type_id, D):
    text = _isa.fa_isa(tmp_path, "fa3_win_inst.hip", type_id, D)
    if D == 64:
        blks = _isa.metadata(text, r"_Z\d+fa3_fwd5_win\w*kernel\w+")
        assert len(blks) == 6
        for blk in blks:
            _isa.check_fits_256(blk)
    else:
        bodies = _isa.kernels(text, r"_Z\d+fa3_fwd3_win")
        assert len(bodies) == 6
        for body in bodies:
            _isa.check_agpr(tmp_path, body, _isa.fa3_agpr_floor(D))

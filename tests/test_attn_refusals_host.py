"""CPU-only: the refusals of the prefill attention entry points, pinned as literal strings.

Every case of the table goes to every entry point of its form that takes it -- the launch and the route query, with and
without the _window suffix when the window is (-1, -1) -- and mio_last_error() must be the literal: the first message a
(possibly doubly-wrong) call gets, under the prefix of the entry point that owns the check (mio_fa3_fwd_paged_kv8 reports
the paged checks as mio_fa3_fwd_paged / mio_fa3_fwd_paged_window).  The valid neighbour of each refusal has its route
asserted; a launch entry point is only called where it launches nothing (a refusal, or the "empty" route)."""
import ctypes as C

import pytest

from test_host_logic import _fa_params
from test_paged_host import _params as _paged_params
from test_varlen_host import _params as _varlen_params

A = 1 << 20  # a fake 16-byte aligned device address: nothing is dereferenced
NOWIN = (-1, -1)
L28 = 1 << 28

# form -> (params builder, launch and route query without a window argument (None: the form has none), launch and route
#          query that take the window, name of the route table in mio._lib)
FORMS = {
    "dense": (_fa_params, "mio_fa3_fwd", "mio_fa3_route", "mio_fa3_fwd_window", "mio_fa3_route_window", "FA3_ROUTES"),
    "varlen": (_varlen_params, "mio_fa3_fwd_varlen", "mio_fa3_varlen_route", "mio_fa3_fwd_varlen_window",
               "mio_fa3_varlen_route_window", "FA3_VARLEN_ROUTES"),
    "paged": (_paged_params, "mio_fa3_fwd_paged", "mio_fa3_paged_route", "mio_fa3_fwd_paged_window",
              "mio_fa3_paged_route_window", "FA3_PAGED_ROUTES"),
    "kv8": (_paged_params, None, None, "mio_fa3_fwd_paged_kv8", "mio_fa3_paged_kv8_route", "FA3_PAGED_ROUTES"),
}

# the messages, by the prefix of the entry point that owns the check
_HEAD_DIM = ": head_dim must be a multiple of 8 in [8,128]"
_DTYPE = ": dtype must be bf16 or fp16"
_SCALE = ": softmax_scale must be > 0"
_ALIGN = ": pointers must be 16-byte aligned"
_STRIDES3 = ": strides must be multiples of 8 elements (16-byte rows)"
_STRIDES2 = ": strides must be non-negative multiples of 8 elements (16-byte rows)"
_WVALUES = ": window values must be -1 (unbounded) or >= 0"
_WCAUSAL = ": causal means window_right = 0 (give -1 or 0)"
_WLEN = ": max_seqlen_q / max_seqlen_k must be below 2^28 under a window"
_BLOCK = ": block_size must be a multiple of 64 (a 64-key tile may not span two pages)"
_LAYER = ": layer_idx must be in [0, num_layers)"
_ROWS = ": the cache must hold fewer than 2^32 token rows (num_blocks * num_layers * block_size)"
_NOSCALE = ": k_scale and v_scale are required with an fp8 cache (null scale pointer)"
_SCALE4 = ": scales must be 4-byte aligned fp32"
_D16 = ": head_dim must be a multiple of 16 in [16,128] for an fp8 cache"
D, DW = "mio_fa3_fwd", "mio_fa3_fwd_window"
V, VW = "mio_fa3_fwd_varlen", "mio_fa3_fwd_varlen_window"
P, PW, P8 = "mio_fa3_fwd_paged", "mio_fa3_fwd_paged_window", "mio_fa3_fwd_paged_kv8"

SC = (A, A)  # the fp8 form's scale addresses

# (form, builder arguments, fields set afterwards (None: null params), window, scales, route, message): route or message
# is None.  Array fields take a tuple.
CASES = [
    # ---- dense
    ("dense", {}, None, NOWIN, None, None, D + ": null params"),
    ("dense", {}, None, (5, 0), None, None, D + ": null params"),
    ("dense", {}, {}, NOWIN, None, "fwd5", None),
    ("dense", {}, {}, (5, 0), None, "fwd5", None),
    ("dense", dict(D=136), {}, NOWIN, None, None, D + _HEAD_DIM),
    ("dense", dict(D=136), {}, (5, 0), None, None, D + _HEAD_DIM),
    ("dense", dict(D=128), {}, NOWIN, None, "fwd3", None),
    ("dense", dict(D=128), {}, (5, 0), None, "fwd3", None),
    ("dense", dict(dtype=2), {}, NOWIN, None, None, D + _DTYPE),
    ("dense", dict(dtype=1), {}, (5, 0), None, "fwd5", None),
    ("dense", {}, dict(softmax_scale=0.0), NOWIN, None, None, D + _SCALE),
    ("dense", {}, dict(softmax_scale=-1.0), (5, 0), None, None, D + _SCALE),
    ("dense", {}, dict(softmax_scale=float("inf")), NOWIN, None, None, D + _SCALE),
    ("dense", {}, dict(q=A + 8), NOWIN, None, None, D + _ALIGN),
    ("dense", {}, dict(v=A + 8), (5, 0), None, None, D + _ALIGN),
    ("dense", dict(row=260), {}, NOWIN, None, None, D + _STRIDES3),
    ("dense", dict(row=260), {}, (5, 0), None, None, D + _STRIDES3),
    ("dense", dict(row=264), {}, (5, 0), None, "fwd5", None),
    ("dense", {}, {}, (-2, 0), None, None, DW + _WVALUES),
    ("dense", {}, {}, (0, -2), None, None, DW + _WVALUES),
    ("dense", {}, {}, (-1, 0), None, "fwd5", None),
    ("dense", dict(causal=1), {}, (5, 1), None, None, DW + _WCAUSAL),
    ("dense", dict(causal=1), {}, (5, 0), None, "fwd5", None),
    ("dense", dict(causal=1), {}, (5, -1), None, "fwd5", None),
    ("dense", dict(causal=0), {}, (5, 1), None, "fwd5", None),
    ("dense", dict(mask_kind=1), {}, (5, 0), None, None, DW + ": a window cannot be combined with a mask"),
    ("dense", dict(mask_kind=1), {}, NOWIN, None, "fwd1_keep", None),
    ("dense", dict(o_acc=True), {}, (5, 0), None, None, DW + ": a window cannot be combined with the ring carry"),
    ("dense", dict(o_acc=True, carry_in=1), {}, (5, 0), None, None, DW + ": a window cannot be combined with the ring carry"),
    ("dense", dict(o_acc=True), {}, NOWIN, None, "fwd3", None),
    ("dense", dict(kpre=1), {}, (5, 0), None, None, DW + ": a window cannot be combined with k_prescaled"),
    ("dense", dict(kpre=1), {}, NOWIN, None, "fwd5_kpre", None),
    ("dense", dict(kpre=1, oblk=1), {}, (5, 0), None, None, DW + ": a window cannot be combined with k_prescaled"),
    ("dense", dict(kpre=1, oblk=1), {}, NOWIN, None, "fwd5_kpre_oblk", None),
    ("dense", dict(oblk=1), {}, (5, 0), None, None,
     D + ": o_blocked is not supported for this launch (needs k_prescaled and mio_fa3_o_blocked_ok != 0)"),
    ("dense", dict(Sq=0, oblk=1), {}, (5, 0), None, None, DW + ": a window cannot be combined with o_blocked"),
    ("dense", dict(Sq=0, oblk=1), {}, NOWIN, None, "empty", None),
    ("dense", dict(kpre=1, D=128), {}, NOWIN, None, None,
     D + ": k_prescaled is not supported for this launch (mio_fa3_k_prescaled_ok == 0)"),
    ("dense", dict(Sq=L28), {}, (5, 0), None, None, DW + ": Sq, Sk and |q_offset - k_offset| must be below 2^28 under a window"),
    ("dense", dict(Sq=L28 - 1), {}, (5, 0), None, "fwd5", None),
    ("dense", dict(Sq=L28), {}, NOWIN, None, "fwd5", None),
    ("dense", {}, dict(q_offset=L28), (5, 0), None, None,
     DW + ": Sq, Sk and |q_offset - k_offset| must be below 2^28 under a window"),
    ("dense", {}, dict(q_offset=L28 - 1), (5, 0), None, "fwd5", None),
    ("dense", dict(Sk=L28), {}, (5, 0), None, None,
     DW + ": K / V rows of one (batch, head) must span less than 4 GiB under a window"),
    ("dense", dict(Sk=L28), {}, NOWIN, None, "fwd1", None),
    ("dense", dict(Sq=0), {}, (5, 0), None, "empty", None),
    ("dense", dict(Sk=0), {}, (5, 0), None, "fwd1", None),
    # doubly wrong: the order of the checks
    ("dense", dict(D=136, dtype=2), {}, NOWIN, None, None, D + _HEAD_DIM),
    ("dense", dict(D=136), dict(q=None), (5, 0), None, None, D + ": q/k/v must be non-null"),
    ("dense", dict(dtype=2), dict(q=A + 8), NOWIN, None, None, D + _DTYPE),
    ("dense", dict(row=260), dict(q=A + 8), NOWIN, None, None, D + _STRIDES3),
    ("dense", dict(D=136), {}, (-2, 0), None, None, D + _HEAD_DIM),
    ("dense", dict(mask_kind=1), {}, (-2, 0), None, None, DW + _WVALUES),
    ("dense", dict(mask_kind=1, causal=1), {}, (-2, 1), None, None, DW + _WVALUES),
    ("dense", dict(kpre=1, causal=1), {}, (5, 1), None, None, DW + _WCAUSAL),
    ("dense", dict(mask_kind=1, o_acc=True), {}, (5, 0), None, None, DW + ": a window cannot be combined with a mask"),
    ("dense", dict(o_acc=True, kpre=1), {}, (5, 0), None, None, DW + ": a window cannot be combined with the ring carry"),
    ("dense", dict(Sq=0, kpre=1), {}, (5, 0), None, None, DW + ": a window cannot be combined with k_prescaled"),
    ("dense", dict(Sq=L28, Sk=L28), {}, (5, 0), None, None,
     DW + ": K / V rows of one (batch, head) must span less than 4 GiB under a window"),
    # ---- varlen
    ("varlen", {}, None, NOWIN, None, None, V + ": null params"),
    ("varlen", {}, None, (5, 0), None, None, V + ": null params"),
    ("varlen", {}, {}, NOWIN, None, "fwd5", None),
    ("varlen", dict(D=136), {}, NOWIN, None, None, V + _HEAD_DIM),
    ("varlen", dict(D=136), {}, (5, 0), None, None, V + _HEAD_DIM),
    ("varlen", dict(D=128), {}, (5, 0), None, "fwd3", None),
    ("varlen", dict(dtype=2), {}, (5, 0), None, None, V + _DTYPE),
    ("varlen", dict(dtype=1), {}, NOWIN, None, "fwd5", None),
    ("varlen", {}, dict(softmax_scale=0.0), NOWIN, None, None, V + _SCALE),
    ("varlen", {}, dict(softmax_scale=-0.5), (5, 0), None, None, V + _SCALE),
    ("varlen", dict(ptr_off=8), {}, NOWIN, None, None, V + _ALIGN),
    ("varlen", dict(ptr_off=8), {}, (5, 0), None, None, V + _ALIGN),
    ("varlen", dict(tok_stride=260), {}, NOWIN, None, None, V + _STRIDES2),
    ("varlen", dict(head_stride=68), {}, (5, 0), None, None, V + _STRIDES2),
    ("varlen", dict(tok_stride=264), {}, (5, 0), None, "fwd5", None),
    ("varlen", {}, {}, (-2, 0), None, None, VW + _WVALUES),
    ("varlen", {}, {}, (0, -3), None, None, VW + _WVALUES),
    ("varlen", {}, {}, (-1, 0), None, "fwd5", None),
    ("varlen", dict(causal=1), {}, (5, 3), None, None, VW + _WCAUSAL),
    ("varlen", dict(causal=1), {}, (5, 0), None, "fwd5", None),
    ("varlen", dict(causal=0), {}, (5, 3), None, "fwd5", None),
    ("varlen", dict(max_q=L28), {}, (5, 0), None, None, VW + _WLEN),
    ("varlen", dict(max_q=L28 - 1), {}, (5, 0), None, "fwd5", None),
    ("varlen", dict(max_q=L28), {}, NOWIN, None, "fwd5", None),
    ("varlen", dict(max_k=L28), {}, (5, 0), None, None,
     V + ": K / V rows of one sequence must span less than 4 GiB (max_seqlen_k * token stride * 2)"),
    ("varlen", dict(B=0, cu=False), {}, (5, 0), None, "empty", None),
    ("varlen", dict(total_q=0, max_q=0), {}, NOWIN, None, "empty", None),
    ("varlen", dict(max_q=0), {}, NOWIN, None, None, V + ": max_seqlen_q must be >= 1 when total_q > 0"),
    # doubly wrong
    ("varlen", dict(D=136, ptr_off=8), {}, NOWIN, None, None, V + _HEAD_DIM),
    ("varlen", dict(tok_stride=260, ptr_off=8), {}, (5, 0), None, None, V + _STRIDES2),
    ("varlen", dict(ptr_off=8), {}, (-2, 0), None, None, V + _ALIGN),
    ("varlen", dict(max_q=L28, causal=1), {}, (5, 3), None, None, VW + _WCAUSAL),
    ("varlen", dict(max_q=L28), {}, (-2, 0), None, None, VW + _WVALUES),
    ("varlen", dict(B=0, cu=False, max_q=L28), {}, (5, 0), None, None, VW + _WLEN),
    # ---- paged, 16-bit cache
    ("paged", {}, None, NOWIN, None, None, P + ": null params"),
    ("paged", {}, None, (5, 0), None, None, P + ": null params"),
    ("paged", {}, {}, NOWIN, None, "fwd5", None),
    ("paged", dict(D=136), {}, NOWIN, None, None, P + _HEAD_DIM),
    ("paged", dict(D=136), {}, (5, 0), None, None, P + _HEAD_DIM),
    ("paged", dict(D=128), {}, (5, 0), None, "fwd3", None),
    ("paged", dict(dtype=2), {}, NOWIN, None, None, P + _DTYPE),
    ("paged", {}, dict(softmax_scale=0.0), (5, 0), None, None, P + _SCALE),
    ("paged", dict(ptr_off=8), {}, NOWIN, None, None, P + _ALIGN),
    ("paged", {}, dict(k_cache=A + 4), (5, 0), None, None, P + _ALIGN),
    ("paged", dict(tok_stride=260), {}, NOWIN, None, None, P + _STRIDES2),
    ("paged", dict(head_stride=68), {}, (5, 0), None, None, P + _STRIDES2),
    ("paged", {}, {}, (-2, 0), None, None, PW + _WVALUES),
    ("paged", dict(causal=1), {}, (5, 3), None, None, PW + _WCAUSAL),
    ("paged", dict(causal=1), {}, (5, -1), None, "fwd5", None),
    ("paged", dict(max_q=L28), {}, (5, 0), None, None, PW + _WLEN),
    ("paged", dict(max_k=L28), {}, (5, 0), None, None, PW + _WLEN),
    ("paged", dict(max_k=L28 - 1), {}, (5, 0), None, "fwd5", None),
    ("paged", dict(max_k=L28), {}, NOWIN, None, "fwd5", None),
    ("paged", dict(block_size=32), {}, NOWIN, None, None, P + _BLOCK),
    ("paged", dict(block_size=32), {}, (5, 0), None, None, P + _BLOCK),
    ("paged", dict(block_size=64), {}, (5, 0), None, "fwd5", None),
    ("paged", dict(layer_idx=2), {}, NOWIN, None, None, P + _LAYER),
    ("paged", dict(layer_idx=-1), {}, (5, 0), None, None, P + _LAYER),
    ("paged", dict(layer_idx=1), {}, (5, 0), None, "fwd5", None),
    ("paged", dict(num_blocks=(1 << 31) // 64, num_layers=2), {}, NOWIN, None, None, P + _ROWS),
    ("paged", dict(num_blocks=(1 << 31) // 64, num_layers=2), {}, (5, 0), None, None, P + _ROWS),
    ("paged", dict(num_blocks=(1 << 31) // 64 - 1, num_layers=2), {}, (5, 0), None, "fwd5", None),
    ("paged", dict(total_q=0, max_q=0), {}, (5, 0), None, "empty", None),
    ("paged", dict(B=0, tables=False), {}, NOWIN, None, "empty", None),
    # doubly wrong
    ("paged", dict(block_size=32, layer_idx=2), {}, NOWIN, None, None, P + _LAYER),
    ("paged", dict(block_size=32, ptr_off=8), {}, NOWIN, None, None, P + _BLOCK),
    ("paged", dict(block_size=32), {}, (-2, 0), None, None, P + _BLOCK),
    ("paged", dict(num_blocks=(1 << 31) // 64, num_layers=2, max_q=L28), {}, (5, 0), None, None, P + _ROWS),
    ("paged", dict(max_q=L28), {}, (-2, 0), None, None, PW + _WVALUES),
    # ---- paged, fp8 cache
    ("kv8", {}, None, NOWIN, SC, None, P + ": null params"),
    ("kv8", {}, None, (5, 0), SC, None, P + ": null params"),
    ("kv8", {}, {}, NOWIN, SC, "fwd5", None),
    ("kv8", {}, {}, (5, 0), SC, "fwd5", None),
    ("kv8", dict(D=128), {}, (5, 0), SC, "fwd3", None),
    ("kv8", dict(D=136), {}, NOWIN, SC, None, P + _HEAD_DIM),
    ("kv8", dict(dtype=2), {}, (5, 0), SC, None, P + _DTYPE),
    ("kv8", {}, dict(softmax_scale=0.0), NOWIN, SC, None, P + _SCALE),
    ("kv8", dict(ptr_off=8), {}, NOWIN, SC, None, P + _ALIGN),
    ("kv8", dict(tok_stride=260), {}, (5, 0), SC, None, P + _STRIDES2),
    ("kv8", dict(block_size=32), {}, NOWIN, SC, None, P + _BLOCK),
    ("kv8", dict(layer_idx=2), {}, (5, 0), SC, None, P + _LAYER),
    ("kv8", dict(num_blocks=(1 << 31) // 64, num_layers=2), {}, NOWIN, SC, None, P + _ROWS),
    ("kv8", {}, {}, (-2, 0), SC, None, PW + _WVALUES),
    ("kv8", dict(causal=1), {}, (5, 3), SC, None, PW + _WCAUSAL),
    ("kv8", dict(max_q=L28), {}, (5, 0), SC, None, PW + _WLEN),
    ("kv8", dict(max_q=L28), {}, NOWIN, SC, "fwd5", None),
    ("kv8", {}, {}, NOWIN, (None, A), None, P8 + _NOSCALE),
    ("kv8", {}, {}, (5, 0), (A, None), None, P8 + _NOSCALE),
    ("kv8", {}, {}, NOWIN, (A + 2, A), None, P8 + _SCALE4),
    ("kv8", {}, {}, (5, 0), (A, A + 1), None, P8 + _SCALE4),
    ("kv8", {}, {}, (5, 0), (A + 4, A + 8), "fwd5", None),
    ("kv8", dict(D=40), {}, NOWIN, SC, None, P8 + _D16),
    ("kv8", dict(D=120), {}, (5, 0), SC, None, P8 + _D16),
    ("kv8", dict(D=48), {}, NOWIN, SC, "fwd5", None),
    ("kv8", dict(D=112), {}, (5, 0), SC, "fwd3", None),
    ("kv8", dict(total_q=0, max_q=0), {}, (5, 0), SC, "empty", None),
    # doubly wrong
    ("kv8", dict(D=40), {}, NOWIN, (None, None), None, P8 + _NOSCALE),
    ("kv8", dict(D=40), {}, (5, 0), (A + 2, A), None, P8 + _SCALE4),
    ("kv8", dict(block_size=32), {}, NOWIN, (None, None), None, P + _BLOCK),
    ("kv8", {}, {}, (-2, 0), (None, None), None, PW + _WVALUES),
    ("kv8", dict(max_k=L28, D=40), {}, (5, 0), SC, None, PW + _WLEN),
    ("kv8", dict(B=0, tables=False), {}, NOWIN, (None, None), None, P8 + _NOSCALE),
    ("kv8", dict(B=0, tables=False, D=40), {}, (5, 0), SC, None, P8 + _D16),
]


def _case_id(c):
    form, kw, fields, win, sc, route, msg = c
    what = "null" if fields is None else ",".join(f"{k}={v}" for k, v in {**kw, **fields}.items())
    scales = "" if sc in (None, SC) else "-sc" + "".join("0" if s is None else str(s - A) for s in sc)
    return f"{form}-{what or 'default'}-w{win[0]}_{win[1]}{scales}"


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_attention_refusals_and_neighbour_routes(case):
    from mio import _lib
    lib = _lib.lib
    form, kw, fields, win, sc, route, msg = case
    build, launch, query, launch_w, query_w, names = FORMS[form]
    names = getattr(_lib, names)
    if fields is None:
        ref = None
    else:
        p = build(**kw)
        for k, v in fields.items():
            if isinstance(v, tuple):
                getattr(p, k)[:] = v
            else:
                setattr(p, k, v)
        ref = C.byref(p)
    sc = () if sc is None else sc
    calls = [(getattr(lib, launch_w), getattr(lib, query_w), (*sc, *win))]
    if win == NOWIN and launch is not None:
        calls.append((getattr(lib, launch), getattr(lib, query), ()))
    # a refusal of another form in between: the message read afterwards is this call's own
    other, stale = (lib.mio_fa3_varlen_route, b"mio_fa3_fwd_varlen: null params") if form == "dense" else \
        (lib.mio_fa3_route, b"mio_fa3_fwd: null params")
    for fwd, rq, extra in calls:
        assert other(None) < 0 and lib.mio_last_error() == stale
        r = rq(ref, *extra)
        if msg is not None:
            assert r == -1, f"{rq.__name__}: route {r}, expected the refusal"
            assert lib.mio_last_error().decode() == msg
            assert other(None) < 0
            assert fwd(ref, *extra, None) == -1
            assert lib.mio_last_error().decode() == msg
        else:
            assert r >= 0, lib.mio_last_error().decode()
            assert names[r] == route
            assert lib.mio_last_error() == stale  # an accepted call leaves the message alone
            if route == "empty":
                assert fwd(ref, *extra, None) == 0


def test_every_prefill_entry_point_is_covered():
    from mio import _lib
    used = {n for f in FORMS.values() for n in f[1:5] if n}
    assert used == {n for n in _lib.EXPORTS if n.startswith("mio_fa3_") and "decode" not in n and not n.endswith("_ok")}
    for form in FORMS:
        assert any(c[0] == form and c[6] is not None for c in CASES) and any(c[0] == form and c[5] is not None for c in CASES)

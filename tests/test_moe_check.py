"""Check the checker (tests/_moe_check.py) on the CPU: a plain fp32 torch evaluation of the mixture-of-experts step, in two
summation orders, passes every stage; each planted defect fails, with the case named in the message."""
import math

import pytest
import torch

import _moe_check as mc

DTYPES = [torch.bfloat16, torch.float16]
OTHER = {torch.bfloat16: torch.float16, torch.float16: torch.bfloat16}
T, K_TOP, E, D, I = 24, 2, 6, 64, 72


def _mm(a, b, order):
    """a b^T in fp32: one product, or four K slices summed last to first."""
    a, b = a.float(), b.float()
    if order == "fwd":
        return a @ b.t()
    cuts = torch.linspace(0, a.shape[-1], 5).long().tolist()
    out = torch.zeros(a.shape[0], b.shape[0])
    for lo, hi in reversed(list(zip(cuts[:-1], cuts[1:]))):
        out = out + a[:, lo:hi] @ b[:, lo:hi].t()
    return out


def _act(z, act):
    F = torch.nn.functional
    return {"none": lambda v: v, "relu": torch.relu, "silu": F.silu, "gelu_erf": F.gelu,
            "gelu": lambda v: F.gelu(v, approximate="tanh")}[act](z)


def emu_route(logits, k, renorm, defect=None):
    x = logits.float().clone()
    x[torch.isnan(x)] = -math.inf
    n_e = x.shape[1]
    if defect == "tie_high":
        order = n_e - 1 - torch.sort(-x.flip(-1), dim=1, stable=True).indices
    else:
        order = torch.sort(-x, dim=1, stable=True).indices
    ids = order[:, :k].clone()
    v = x.clamp(max=mc.FLT_MAX)
    m = v.max(1, keepdim=True).values
    dead = ~torch.isfinite(m[:, 0])
    p = torch.exp2((v - torch.where(dead[:, None], torch.zeros_like(m), m)) * torch.tensor(mc.LOG2E, dtype=torch.float32))
    psel = p.gather(1, ids)
    w = psel / (psel.sum(1, keepdim=True) if defect == "softmax_topk" else p.sum(1, keepdim=True))
    if renorm and defect != "no_renorm":
        w = w / w.sum(1, keepdim=True)
    ids[dead] = torch.arange(k)
    w[dead] = 0.0
    off, srt, pos = mc.group_rows(ids, n_e)
    if defect == "sorted_desc":
        for e in range(n_e):
            srt[int(off[e]):int(off[e + 1])] = srt[int(off[e]):int(off[e + 1])].flip(0)
        pos[srt] = torch.arange(srt.numel())
    if defect == "offsets_off_by_one":
        off = off.clone()
        off[1:-1] += 1
    return ids, w, off, srt, pos


def emu_up(x, ids, off, srt, w_up, w_gate, b_up, b_gate, act, dtype, order="fwd", defect=None):
    k, rows = ids.shape[1], srt.numel()
    h = torch.zeros(rows, w_up.shape[1], dtype=dtype)
    leak = []
    for e in range(w_up.shape[0]):
        lo, hi = int(off[e]), int(off[e + 1])
        n = hi - lo + (1 if defect == "neighbour_leak" and lo < hi < rows else 0)
        if n <= 0:
            continue
        r = srt[lo:lo + n]
        xe = x[(r % x.shape[0]) if defect == "gather_r" else r // k]
        z = _mm(xe, w_up[e], order) + b_up[e].float()
        a = torch.nn.functional.silu(_mm(xe, w_gate[e], order) + b_gate[e].float()) * z if act == "swiglu" else _act(z, act)
        a = a.to(OTHER[dtype]).to(dtype) if defect == "h_twice" else a.to(dtype)
        h[lo:hi] = a[:hi - lo]
        if n > hi - lo:
            leak.append((hi, a[-1]))
    for p, row in leak:   # the row behind the expert's last, computed with this expert's weights, lands last
        h[p] = row
    return h


def emu_down(h, ids, w, pos, w_down, b_down, residual, dtype, order="fwd", defect=None):
    n_t, k = ids.shape
    y = torch.zeros(n_t, w_down.shape[1])
    for j in range(k - 1 if defect == "slot_drop_last" else k):
        for t in range(n_t):
            e = int(ids[t, j])
            z = _mm(h[int(pos[t * k + j])][None], w_down[e], order)[0]
            y[t] += (w[t, j] * z + b_down[e].float()) if defect == "weight_before_bias" else w[t, j] * (z + b_down[e].float())
    return (y + residual.float()).to(dtype)


def _inputs(dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(dtype)  # noqa: E731
    logits = r(T, E, scale=2.0)
    logits[3] = 0.5                                  # all equal: ties to the lowest index
    logits[4, 1] = logits[4, 4] = logits[4].float().max() + 1    # a tie for the first place
    logits[5, 2] = float("nan")
    logits[6] = float("-inf")                        # no finite logit
    return dict(logits=logits, x=r(T, D), w_up=r(E, I, D, scale=D ** -0.5), w_gate=r(E, I, D, scale=D ** -0.5), b_up=r(E, I, scale=0.5),
                b_gate=r(E, I, scale=0.5), w_down=r(E, D, I, scale=I ** -0.5), b_down=r(E, D, scale=0.5), res=r(T, D))


def _run(dtype, renorm, act, order, defect, what):
    """The whole emulated step through the checker, stage by stage, each judged from what the stage before it wrote."""
    v = _inputs(dtype)
    ids, w, off, srt, pos = emu_route(v["logits"], K_TOP, renorm, defect)
    ref = mc.route_reference(v["logits"], K_TOP, renorm)
    mc.check_route(ref, ids, w, off, srt, pos, what=what)
    h = emu_up(v["x"], ids, off, srt, v["w_up"], v["w_gate"], v["b_up"], v["b_gate"], act, dtype, order, defect)
    gate = dict(w_gate=v["w_gate"], b_gate=v["b_gate"]) if act == "swiglu" else {}
    mc.check_up(h, mc.up_reference(v["x"], ref, v["w_up"], act, b_up=v["b_up"], **gate), dtype, what)
    y = emu_down(h, ids, w, pos, v["w_down"], v["b_down"], v["res"], dtype, order, defect)
    mc.check_down(y, mc.down_reference(h, ref, v["w_down"], v["b_down"], v["res"], weights=w), dtype, what)
    # the composed bound of the module test holds for the same step
    _, comp = mc.composed_reference(v["x"], v["logits"], K_TOP, renorm, v["w_up"], v["w_down"], act, b_up=v["b_up"],
                                    b_down=v["b_down"], residual=v["res"], **gate)
    mc.check_down(y, comp, dtype, what + " composed")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("order", ["fwd", "rev"])
@pytest.mark.parametrize("renorm", [True, False])
@pytest.mark.parametrize("act", ["swiglu", "gelu"])
def test_fp32_evaluation_passes(dtype, order, renorm, act):
    _run(dtype, renorm, act, order, None, f"clean {order}")


DEFECTS = [("tie_high", True), ("softmax_topk", False), ("no_renorm", True), ("sorted_desc", True), ("offsets_off_by_one", True),
           ("gather_r", True), ("slot_drop_last", True), ("weight_before_bias", True), ("h_twice", True), ("neighbour_leak", True)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("defect,renorm", DEFECTS)
def test_planted_defects_fail(dtype, defect, renorm):
    what = f"planted {defect}"
    with pytest.raises(AssertionError, match=what):
        _run(dtype, renorm, "swiglu", "fwd", defect, what)


def test_defects_are_not_vacuous():
    """softmax_topk and no_renorm are each other's complement: under the other flag value the planted code is the right code."""
    _run(torch.bfloat16, True, "swiglu", "fwd", "softmax_topk", "softmax over the top-k, renormalised")
    _run(torch.bfloat16, False, "swiglu", "fwd", "no_renorm", "no renormalisation asked")


def test_allowance_is_small():
    """The route allowance is a few fp32 ulps of the weight at ordinary logits: it cannot hide a wrong weight."""
    v = _inputs(torch.bfloat16)
    ref = mc.route_reference(v["logits"], K_TOP, True)
    live = ref.allow > 0
    assert float((ref.allow[live] / ref.weights[live].clamp_min(1e-30)).max()) < 1e-4
    assert bool((ref.allow[6] == 0).all()) and bool((ref.weights[6] == 0).all()) and ref.ids[6].tolist() == [0, 1]
    assert ref.ids[3].tolist() == [0, 1] and ref.ids[4].tolist() == [1, 4]

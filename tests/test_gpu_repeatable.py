"""Same inputs, same bits: every kernel route repeated alone, cold, beside noise on a second stream and at shifted addresses.

Every kernel here documents itself as deterministic (fixed summation order, no atomics between workgroups).  The value tests
launch each route once on an idle card; a race in the hand-counted waits, the wave hand-offs or the barriers of the hot path
would depend on timing and pass them.  Each case of CASES (tests/_repeat.py has the driver and the report)

  * builds its inputs once, asserts the route with the existing host query, launches once into outputs prefilled with 0xFF
    and has that first result judged by the family's existing checker at its existing bars -- so equality cannot be met by a
    kernel that wrote nothing or wrote NaN;
  * then launches again under five conditions, every launch on inputs restored from the pristine copy and fresh 0xFF
    outputs (what a launch wrote and what it returned is overwritten with 0xFF once compared, so that a freed result block
    handed out again cannot stand in for a launch that wrote nothing), one synchronisation per condition:
      back-to-back  8 launches queued on one stream with nothing between them;
      cold          a 512 MiB fill (twice the Infinity Cache) on the same stream before each of 8 launches;
      co-run memory 8 launches while a second stream copies a 1 GiB buffer device to device, queued first and long enough;
      co-run matrix 8 launches while a second stream runs ops.gemm_bias_act at 4096^3 (p8w: LDS and MFMA), queued likewise;
      placement     3 launches on buffers whose bases are shifted by 16, 48 and 4112 bytes, the route asserted unchanged;
  * and every written byte of every launch must equal the first result's.  The first condition that differs ends the case
    with the report of _repeat.compare: condition, repeat, counts, first index, tile / (sequence, head, row block) histogram.

The decode GEMMs run the cold and co-run conditions only (alone they are covered by their own test_deterministic_and_graph).
Of a result with rows the kernel never writes (statistics rows and blocked rows past M) the written rows are compared.
The overlap line each co-run condition prints is the share of the launches' wall time (events on both streams) during which
the noise stream was busy; it is printed, never asserted.  A share of zero means the condition proved nothing for that case.

The module cases -- two folded Blocks and one FlashSelfAttention paged decode step with qk_norm, rotary, an fp8 cache and both
decode-GEMM switches -- compare the final tensor (the decode step also its caches); on a difference first_differing_launch
repeats each recorded launch of the module alone, once, and names the first that differs.

Measured by one run of this file alone on the MI355X (pytest -m gpu -s --durations=0): 212 tests, 24.0 s of pytest wall
time, no case differed; the rest of the GPU suite takes about 250 s (2678 tests) in a run of the whole suite.  Time per
family is the sum of that run's per-test durations (21.8 s; the remainder is collection and start-up), overlap is the
smallest / median share that the cases of the family printed for each co-run condition:

  family        tests   time      share   conditions                           overlap memory   overlap matrix
  prep             12   7.32 s    33.5 %  all five                             1.00 / 1.00      1.00 / 1.00
  module            6   3.15 s    14.4 %  all five                             1.00 / 1.00      1.00 / 1.00
  decode           26   2.97 s    13.6 %  all five                             0.99 / 1.00      1.00 / 1.00
  prefill          50   2.94 s    13.5 %  all five                             1.00 / 1.00      1.00 / 1.00
  gemm             26   2.05 s     9.4 %  all five                             1.00 / 1.00      1.00 / 1.00
  mlp              40   1.54 s     7.1 %  all five                             1.00 / 1.00      1.00 / 1.00
  cache_write      16   0.63 s     2.9 %  all five                             1.00 / 1.00      1.00 / 1.00
  rows             14   0.62 s     2.8 %  all five                             1.00 / 1.00      1.00 / 1.00
  decode_gemm      12   0.36 s     1.6 %  cold, co-run memory, co-run matrix   1.00 / 1.00      1.00 / 1.00
  rotary            8   0.24 s     1.1 %  all five                             1.00 / 1.00      1.00 / 1.00

No family had a share of zero, so no co-run condition was vacuous.  ln_fold_weight at K 8192 (each launch rounds 64 rows of
8192 elements greedily, eight launches take some fifty times the usual noise) queues more noise (RC.noise): 64 times the copies
and, as matrix noise, launches of eight times the rows; with the usual noise it printed 0.02, now 1.00 for both conditions.
The longest cases are those two (3.3 s and 3.6 s, most of it waiting for their noise to drain) and block_fold in bf16 (1.5 s);
every other case takes under a second.
"""
import copy
import ctypes
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Callable, Optional

import pytest
import torch

import _attn_steep as st
import _decode_check as dc
import _gemm_check as gc
import _qknorm_check as qc
import _repeat as rp
import _rms_check as rmc
import _rope_check as rc
import _rows_check as rw
import _skinny_cases as sk
import _w8_cases as wc
import _w8_check as w8c

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
F8 = torch.float8_e4m3fn
SENT = 0x5A
EPS_QK = 1e-6


def _ops():
    from mio import ops
    return ops


def _lib():
    from mio import _lib
    return _lib


def _is_dev(dev):
    return str(dev).startswith("cuda")


# ---------------------------------------------------------------------------------------------------------------------
# the conditions
# ---------------------------------------------------------------------------------------------------------------------
_SHARED = {}


def _shared(name, make):
    if name not in _SHARED:
        _SHARED[name] = make()
    return _SHARED[name]


@pytest.fixture(scope="module", autouse=True)
def _release_shared():
    yield
    _SHARED.clear()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


class BackToBack(rp.Condition):
    name = "back-to-back"

    def stop(self):
        torch.cuda.synchronize()


class Cold(rp.Condition):
    name = "cold"

    def before(self, i):
        _shared("scratch", lambda: torch.empty(512 << 20, dtype=torch.uint8, device=DEV)).fill_(i)

    def stop(self):
        torch.cuda.synchronize()


class CoRun(rp.Condition):
    """`count` units of noise on the side stream, queued before the first launch; events on both streams give the overlap."""

    def __init__(self, name, unit, count):
        self.name, self.unit, self.count = name, unit, count

    def start(self):
        ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
        self.base, self.n0, self.n1, self.t0, self.t1 = ev(), ev(), ev(), ev(), ev()
        main = torch.cuda.current_stream()
        side = _shared("side", torch.cuda.Stream)
        self.base.record(main)
        side.wait_event(self.base)
        with torch.cuda.stream(side):
            self.n0.record(side)
            for _ in range(self.count):
                self.unit()
            self.n1.record(side)
        self.t0.record(main)

    def stop(self):
        self.t1.record(torch.cuda.current_stream())
        torch.cuda.synchronize()
        ns, ne = self.base.elapsed_time(self.n0), self.base.elapsed_time(self.n1)
        ts, te = self.base.elapsed_time(self.t0), self.base.elapsed_time(self.t1)
        return max(0.0, min(ne, te) - max(ns, ts)) / max(te - ts, 1e-6)


def _memory_noise():
    a, b = _shared("copy", lambda: (torch.zeros(1 << 30, dtype=torch.uint8, device=DEV),
                                    torch.empty(1 << 30, dtype=torch.uint8, device=DEV)))
    b.copy_(a)


def _matrix_noise(M=4096):
    def make():
        g = torch.Generator(device=DEV).manual_seed(1)
        x = torch.randn(M, 4096, device=DEV, generator=g).to(torch.bfloat16)
        w = (torch.randn(4096, 4096, device=DEV, generator=g) / 64).to(torch.bfloat16)
        assert _ops().gemm_route(x, w) == "p8w"
        return x, w, torch.empty(M, 4096, dtype=torch.bfloat16, device=DEV)
    x, w, y = _shared(f"matrix{M}", make)
    _ops().gemm_bias_act(x, w, out=y)  # inside torch.cuda.stream(side): ops._stream() reads the current stream


def _matrix_noise_x8():
    """Eight times the rows per launch: for noise that has to last seconds the host would otherwise queue the small launches
    hardly faster than the card retires them, and the launches under test would start after most of the noise."""
    _matrix_noise(8 * 4096)


def _conditions(which, scale=(1, 1)):
    """scale: how many times the usual (memory, matrix) noise a case needs for the noise to outlast its eight launches."""
    matrix = CoRun("co-run matrix", _matrix_noise, 64) if scale[1] == 1 else \
        CoRun("co-run matrix", _matrix_noise_x8, 64 * scale[1] // 8)
    noise = [Cold(), CoRun("co-run memory", _memory_noise, 24 * scale[0]), matrix]
    if which == "noise":
        return noise
    return [BackToBack()] + noise + [rp.Placement(sync=torch.cuda.synchronize)]


# ---------------------------------------------------------------------------------------------------------------------
# a case: build once, then states with every tensor placed afresh
# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class RC:
    family: str
    name: str
    covers: tuple                         # ("gemm:p8w", "write:rope_and_cache_varlen", "row:layernorm", ...)
    build: Callable                       # (dtype, dev) -> p: a SimpleNamespace; every tensor in it is placed per launch
    launch: Callable                      # (p) -> ret, queued on the current stream
    written: Callable                     # (p, ret) -> {name: tensor or rp.Attn}
    judge: Callable                       # (p, ret): the family's existing checks on the first launch
    route: Optional[Callable] = None      # (p) -> the host route query's answer
    want: object = None                   # what route(p) must answer (None: p.route)
    outputs: Optional[Callable] = None    # (p) -> {attribute: (shape, dtype)}: fresh 0xFF buffers set on p per launch
    conditions: str = "all"
    noise: tuple = (1, 1)                 # the co-run conditions queue this many times the usual (memory, matrix) noise
    host: bool = True                     # build(dtype, "cpu") works as it is; False: the operands come from the GEMM tables'
    #                                       builders (their DEV and the device preparations are stubbed in the host test), or,
    #                                       for the module cases, from modules on the device (no route query; GPU only)
    dtypes: tuple = tuple(DTYPES)

    @property
    def id(self):
        return f"{self.family}-{self.name}"


def _place_tree(obj, shift, memo):
    if isinstance(obj, torch.Tensor):
        if id(obj) not in memo:
            memo[id(obj)] = rp.place(obj, shift)
        return memo[id(obj)]
    if isinstance(obj, SimpleNamespace):
        out = copy.copy(obj)
        for k, v in vars(obj).items():
            if k != "ref":  # (reference-only data is shared, not placed)
                setattr(out, k, _place_tree(v, shift, memo))
        return out
    if isinstance(obj, dict):
        return {k: _place_tree(v, shift, memo) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)) and any(isinstance(v, (torch.Tensor, dict, SimpleNamespace)) for v in obj):
        return type(obj)(_place_tree(v, shift, memo) for v in obj)
    return obj


def _tensors(obj, acc):
    if isinstance(obj, torch.Tensor):
        acc.append(obj)
    elif isinstance(obj, SimpleNamespace):
        for k, v in vars(obj).items():
            if k != "ref":
                _tensors(v, acc)
    elif isinstance(obj, dict):
        for v in obj.values():
            _tensors(v, acc)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            _tensors(v, acc)
    return acc


def make_state(case, prob, shift, dev):
    """prob with every tensor copied into a buffer of its own (base shifted by `shift` bytes; the same tensor object twice
    stays one tensor) and the case's outputs as fresh 0xFF buffers."""
    p = _place_tree(prob, shift, {})
    if case.outputs is not None:
        for name, (shape, dtype) in case.outputs(prob).items():
            setattr(p, name, rp.fresh(shape, dtype, dev, shift))
    return p


def check_placement(case, prob, dev):
    """The shifted buffers keep every pointer 16-byte aligned and every stride, and the route query answers as unshifted."""
    p0 = make_state(case, prob, 0, dev)
    want = case.want if case.want is not None else getattr(prob, "route", None)
    r0 = case.route(p0) if case.route is not None else None
    if case.route is not None:
        assert r0 == want, f"{case.id}: route {r0}, expected {want}"
    t0 = _tensors(p0, [])
    for s in rp.SHIFTS:
        ps = make_state(case, prob, s, dev)
        ts = _tensors(ps, [])
        assert len(ts) == len(t0)
        for a, b in zip(t0, ts):
            assert a.stride() == b.stride() and a.shape == b.shape
        assert rp.aligned16(*ts), f"{case.id}: a buffer shifted by {s} bytes is not 16-byte aligned"
        if case.route is not None:
            assert case.route(ps) == r0, f"{case.id}: the route changes with a shift of {s} bytes"


def run_case(case, dtype):
    prob = case.build(dtype, DEV)
    check_placement(case, prob, DEV)

    def written(p, ret):
        return case.written(p, ret)

    res = rp.run_repeats(lambda s: make_state(case, prob, s, DEV), case.launch, written, _conditions(case.conditions, case.noise),
                         repeats=rp.REPEATS, judge=case.judge, allocated=lambda p, ret: _tensors(ret, []))
    for cond, share in res.overlap.items():
        print(f"OVERLAP {case.family} | {case.name} | {str(dtype).split('.')[-1]} | {cond} | {share:.2f}")
    res.check(f"{case.id} {dtype}")
    assert res.ran == [c.name for c in _conditions(case.conditions, case.noise)] and res.launches == 1 + sum(
        len(c.shifts) if c.shifts else rp.REPEATS for c in _conditions(case.conditions, case.noise))


def _to(t, dev):
    return None if t is None else t.to(dev)


# ---------------------------------------------------------------------------------------------------------------------
# prefill: one _attn_steep case per group and route
# ---------------------------------------------------------------------------------------------------------------------
def _steep(group, route, **attrs):
    return next(c for c in st.CASES if c.group == group and c.route == route and all(getattr(c, k) == v for k, v in attrs.items()))


def _cu(lens):
    c = [0]
    for n in lens:
        c.append(c[-1] + n)
    return torch.tensor(c, dtype=torch.int32)


def _unblock_attn(ob, B, Sq, H, D):
    M = ob.shape[0]
    return ob.view(M // 256, H * D // 32, 256, 32).permute(0, 2, 1, 3).reshape(M, H * D)[:B * Sq].view(B, Sq, H, D)


def _dense_case(case):
    def build(dtype, dev):
        prob, = st.build(case, dtype)
        keep, add = prob.extra["keep"], prob.extra["add"]
        kw = dict(causal=case.causal, q_offset=prob.extra["off"], softmax_scale=case.scale, k_prescaled=case.kpre,
                  out_blocked=case.oblk, window_size=case.window, keep_mask=_to(keep, dev), additive_mask=_to(add, dev),
                  return_lse=not case.oblk)
        return SimpleNamespace(dtype=dtype, q=prob.q.to(dev), k=prob.k.to(dev), v=prob.v.to(dev), kw=kw, route=case.route,
                               ref=SimpleNamespace(prob=prob))

    def outputs(p):
        return {} if case.oblk else {"out": (tuple(p.q.shape), p.dtype)}

    def kwargs(p):
        return dict(p.kw, out=None if case.oblk else p.out)

    def written(p, ret):
        B, Sq, H, D = p.q.shape
        if case.oblk:
            return {"o": rp.Attn(_unblock_attn(ret, B, Sq, H, D), "bshd")}
        return {"o": rp.Attn(ret[0], "bshd"), "lse": rp.Attn(ret[1], "bhs")}

    def judge(p, ret):
        prob, dtype = p.ref.prob, p.dtype
        w = written(p, ret)
        if not case.oblk:
            assert ret[0].data_ptr() == p.out.data_ptr()
        ref, rlse = st.reference(prob)
        st.judge(w["o"].tensor.cpu(), w["lse"].tensor.cpu() if "lse" in w else None, ref, rlse, dtype, case.route, case.id,
                 lambda: st.plan(case, dtype, prob))

    return RC("prefill", case.id, (f"fa3:{case.route}",), build, lambda p: _ops().fa3_fwd(p.q, p.k, p.v, **kwargs(p)), written,
              judge, route=lambda p: _ops().fa3_route(p.q, p.k, p.v, **kwargs(p)), outputs=outputs)


def _carry_case(case):
    def build(dtype, dev):
        prob, = st.build(case, dtype)
        return SimpleNamespace(dtype=dtype, q=prob.q.to(dev), k=prob.k.to(dev), v=prob.v.to(dev), route=case.route,
                               ref=SimpleNamespace(prob=prob, parts=st.shards(case, prob)))

    def outputs(p):
        B, Sq, H, D = p.q.shape
        return {"out": ((B, Sq, H, D), p.dtype), "acc": ((B, Sq, H, D), torch.float32), "lse": ((B, H, Sq), torch.float32)}

    def each(p, fn):
        parts, res = p.ref.parts, []
        for i, (lo, hi) in enumerate(parts):
            last = i == len(parts) - 1
            kw = dict(softmax_scale=case.scale, k_prescaled=case.kpre, k_offset=lo, o_acc=p.acc, lse=p.lse, carry_in=i > 0,
                      write_out=last, out=p.out if last else None)
            res.append(fn(p.q, p.k[:, lo:hi], p.v[:, lo:hi], **kw))
        return res

    def written(p, ret):
        return {"o": rp.Attn(p.out, "bshd"), "carry": rp.Attn(p.acc, "bshd"), "lse": rp.Attn(p.lse, "bhs")}

    def judge(p, ret):
        prob, dtype = p.ref.prob, p.dtype
        ref, rlse = st.reference(prob)
        pl = lambda: st.plan(case, dtype, prob)  # noqa: E731
        st.judge(p.out.cpu(), p.lse.cpu(), ref, rlse, dtype, case.route, case.id, pl)
        st.judge(p.acc.cpu(), None, ref, rlse, dtype, case.route, case.id + " (fp32 carry)", pl)

    return RC("prefill", case.id, (f"fa3:{case.route}",), build, lambda p: each(p, _ops().fa3_fwd), written, judge,
              route=lambda p: sorted(set(each(p, _ops().fa3_route))), want=[case.route], outputs=outputs)


def _pack(probs, dev):
    return (torch.cat([p.q[0] for p in probs]).to(dev), torch.cat([p.k[0] for p in probs]).to(dev),
            torch.cat([p.v[0] for p in probs]).to(dev))


def _judge_sequences(case, dtype, probs, out, lse):
    q0 = 0
    for b, prob in enumerate(probs):
        Lq = prob.q.shape[1]
        ref, rlse = st.reference(prob)
        st.judge(out[q0:q0 + Lq][None].cpu(), lse[:, q0:q0 + Lq][None].cpu(), ref, rlse, dtype, case.route,
                 f"{case.id} seq {b} (Lq {Lq}, Lk {prob.k.shape[1]})", lambda prob=prob: st.plan(case, dtype, prob))
        q0 += Lq


def _packed_written(case):
    cu = _cu(case.lens_q).tolist()
    return lambda p, ret: {"o": rp.Attn(ret[0], "thd", cu), "lse": rp.Attn(ret[1], "ht", cu)}


def _varlen_case(case):
    mq, mk = max(case.lens_q), max(case.lens_k)

    def build(dtype, dev):
        probs = st.build(case, dtype)
        q, k, v = _pack(probs, dev)
        return SimpleNamespace(dtype=dtype, q=q, k=k, v=v, cu_q=_cu(case.lens_q).to(dev), cu_k=_cu(case.lens_k).to(dev),
                               route=case.route, ref=SimpleNamespace(probs=probs))

    def args(p):
        return (p.q, p.k, p.v, p.cu_q, p.cu_k, mq, mk), dict(causal=case.causal, softmax_scale=case.scale, return_lse=True,
                                                              out=p.out, window_size=case.window)

    def call(fn, p):
        a, kw = args(p)
        return fn(*a, **kw)

    def judge(p, ret):
        assert ret[0].data_ptr() == p.out.data_ptr()
        _judge_sequences(case, p.dtype, p.ref.probs, ret[0], ret[1])

    return RC("prefill", case.id, (f"fa3_varlen:{case.route}",), build, lambda p: call(_ops().flash_attention_varlen, p),
              _packed_written(case), judge, route=lambda p: call(_ops().fa3_varlen_route, p),
              outputs=lambda p: {"out": (tuple(p.q.shape), p.dtype)})


def _paged_case(case):
    mq, mk = max(case.lens_q), max(case.lens_k)
    bs, Hkv, D, L, layer = case.bs, case.Hkv, case.D, 2, 1
    kv8 = case.group == "kv8"

    def build(dtype, dev):
        probs = st.build(case, dtype)
        q, k, v = _pack(probs, dev)
        g = torch.Generator().manual_seed(case.bs + D)
        npages = [(n + bs - 1) // bs + 1 for n in case.lens_k]
        nb = sum(npages) + 3
        perm = torch.randperm(nb, generator=g)
        bt = torch.zeros(len(npages), max(npages), dtype=torch.int32)
        nxt = 0
        for b, n in enumerate(npages):
            bt[b, :n] = perm[nxt:nxt + n]
            nxt += n
        bt = bt.to(dev)
        scales = {}
        if kv8:
            kc = torch.full((nb, L, bs, Hkv, D), 0x7F, dtype=torch.uint8, device=dev).view(F8)
            vc = torch.full((nb, L, bs, Hkv, D), 0xFF, dtype=torch.uint8, device=dev).view(F8)
            ks, vs = st.KV8_SCALES
            scales = dict(k_scale=torch.tensor([0.7, ks], device=dev), v_scale=torch.tensor([1.3, vs], device=dev))
        else:
            kc = torch.randn(nb, L, bs, Hkv, D, generator=g).to(dtype).to(dev)
            vc = torch.randn(nb, L, bs, Hkv, D, generator=g).to(dtype).to(dev)
        used = torch.tensor(case.lens_k, dtype=torch.int32, device=dev)
        if _is_dev(dev):  # (the route query reads no data: on the host the cache stays as it is)
            _ops().reshape_and_cache_varlen(k, v, kc, vc, bt, _cu(case.lens_k).to(dev), used, bs, layer, **scales)
        return SimpleNamespace(dtype=dtype, q=q, kc=kc, vc=vc, bt=bt, cu_q=_cu(case.lens_q).to(dev), used=used, scales=scales,
                               route=case.route, ref=SimpleNamespace(probs=probs))

    def call(fn, p):
        return fn(p.q, p.kc, p.vc, p.bt, p.cu_q, p.used, mq, mk, layer_idx=layer, causal=case.causal, softmax_scale=case.scale,
                  return_lse=True, out=p.out, window_size=case.window, **p.scales)

    def judge(p, ret):
        assert ret[0].data_ptr() == p.out.data_ptr()
        if kv8:
            p0 = p.ref.probs[0]
            pos = torch.arange(p0.k.shape[1], device=DEV)
            got = p.kc[p.bt[0, pos // bs].long(), layer, pos % bs].double().cpu() * st.KV8_SCALES[0]
            assert torch.equal(got, p0.kk[0]), "the fp8 cache differs from the CPU quantisation formula"
        _judge_sequences(case, p.dtype, p.ref.probs, ret[0], ret[1])

    return RC("prefill", case.id, (f"fa3_paged:{case.route}",), build, lambda p: call(_ops().flash_attention_varlen_paged, p),
              _packed_written(case), judge, route=lambda p: call(_ops().fa3_paged_route, p),
              outputs=lambda p: {"out": (tuple(p.q.shape), p.dtype)})


def _prefill_cases():
    out = [_dense_case(_steep("dense", r)) for r in ("fwd5", "fwd5_kpre", "fwd5_kpre_oblk", "fwd3", "fwd3_kpre", "fwd1",
                                                      "fwd1_add", "fwd1_keep")]
    out += [_carry_case(_steep("carry", r)) for r in ("fwd5_kpre_carry", "fwd3", "fwd1")]
    for r in ("fwd5", "fwd3"):
        out.append(_varlen_case(_steep("varlen", r)))
        out += [_paged_case(_steep("paged", r, bs=b)) for b in (64, 128)]
        out.append(_paged_case(_steep("kv8", r)))
        out.append(_dense_case(_steep("window_dense", r)))
        out.append(_varlen_case(_steep("window_varlen", r)))
        out.append(_paged_case(_steep("window_paged", r)))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# paged decode: the first case of each (route, cache kind, windowed) family whose launch splits, and the block-table slices
# ---------------------------------------------------------------------------------------------------------------------
def _decode_ws(c):
    return _lib().lib.mio_fa3_decode_workspace_bytes(c["B"], c["H"], c["q_len"], c["D"], c["msl"])


def _decode_case(base):
    def build(dtype, dev):
        case = dict(base, dtype=dtype)
        t = dc.build_case(case)
        p = SimpleNamespace(dtype=dtype, kc=t["kc"].to(dev), vc=t["vc"].to(dev), bt=t["bt"].to(dev), ctx=t["ctx"].to(dev),
                            route=case["route"], scales={}, ref=SimpleNamespace(case=case, t=t))
        B, H, q_len, D = case["B"], case["H"], case["q_len"], case["D"]
        if case["q_packed"]:
            qkv = torch.full((B, q_len, 3, H, D), float("nan"), dtype=dtype)
            qkv[:, :, 0] = t["q"].permute(0, 2, 1, 3)
            p.qkv = qkv.to(dev)
        else:
            p.q = t["q"].to(dev)
        if case["kv8"]:
            p.scales = dict(k_scale=torch.tensor(t["k_scale"], dtype=torch.float32, device=dev),
                            v_scale=torch.tensor(t["v_scale"], dtype=torch.float32, device=dev))
        return p

    def call(fn, p):
        q = p.qkv[:, :, 0].permute(0, 2, 1, 3) if base["q_packed"] else p.q
        out = p.buf[..., :base["D"]]
        assert (tuple(q.stride()[:3]), tuple(out.stride()[:3])) == dc.case_strides(base)
        return fn(q, out, p.kc, p.vc, p.bt, p.ctx, base["bs"], base["msl"], dc.LAYER, window_size=(base["left"], -1), **p.scales)

    def judge(p, ret):
        case, t = p.ref.case, p.ref.t
        assert _decode_ws(case) > 0, "the case has a single split: the reduce kernel is not in the chain"
        ref, lse, model_o = dc.case_reference(case, t)
        if case["out_pad"]:
            assert (p.buf[..., case["D"]:].contiguous().view(torch.uint8) == 0xFF).all(), "the padding behind the rows was written"
        dc.check(p.buf[..., :case["D"]], ref, lse, p.dtype, dc.family(case), model_o, case["name"],
                 win=case["left"] >= 0 and not case["equal_unwindowed"])

    return RC("decode", base["name"], (f"decode:{base['route']}",), build, lambda p: call(_ops().paged_attention_forward, p),
              lambda p, ret: {"o": rp.Attn(p.buf, "bhsd")}, judge, route=lambda p: call(_ops().paged_attention_route, p),
              outputs=lambda p: {"buf": ((base["B"], base["H"], base["q_len"], base["D"] + base["out_pad"]), p.dtype)})


def _decode_cases():
    """The first case of each family in _decode_check.CASES, passing over the table's msl 32768 cases (their workspace and
    block tables are the largest of the table and most of their splits are empty); the chosen ones all have max_seq_len 1100."""
    out = []
    for route in ("head", "rows", "gqa"):
        for kv8 in (False, True):
            for win in (False, True):
                out.append(_decode_case(next(
                    c for c in dc.CASES if c["route"] == route and c["kv8"] == kv8 and not c["equal_unwindowed"]
                    and (c["left"] >= 0) == win and c["msl"] <= 2100 and _decode_ws(c) > 0)))
    out.append(_decode_case(next(c for c in dc.CASES if c["name"] == "gqa-kv16-bt-slice")))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# GEMM routes and the fused MLP: the build / launch / judge parts of tests/test_gpu_gemm_matrix.py
# ---------------------------------------------------------------------------------------------------------------------
def _gm():
    import test_gpu_gemm_matrix as gm
    return gm


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _tiles(M, N, glu=False):
    return ((M + 255) // 256) * ((N + (127 if glu else 255)) // (128 if glu else 256))


def _loops(M, N, glu=False):
    """More 256-row tiles than workgroups: the persistent kernel's workgroups loop over tiles."""
    assert _tiles(M, N, glu) > (_cus() + 7) // 8 * 8, f"{_tiles(M, N, glu)} tiles on {_cus()} CUs: no workgroup takes a second tile"


def _wide(M, N, glu=False):
    """N as the table has it where its tiles outnumber the CUs rounded up to 8 (256 on the MI355X: every N below is the table's),
    else enlarged by whole tiles until they do."""
    while _tiles(M, N, glu) <= (_cus() + 7) // 8 * 8:
        N += 256
    return N


def _table_case(route, name, kind, persistent=True, parts=None, tag=None):
    """A case of test_gpu_gemm_matrix.CASES[route][name] (or the given parts).  kind "act": gemm_bias_act into a fresh out=;
    "ln": gemm_ln, which allocates (y, statistics) itself."""
    def get():
        return parts() if parts is not None else _gm().CASES[route][name]

    def build(dtype, dev):
        p = get().build(dtype)
        assert p.buf is None if kind == "act" else True
        return p

    def judge(p, ret):
        M, N, _ = p.shape
        if persistent:
            _loops(M, N, glu=route.startswith("p8w_glu"))
        get().judge(p, ret)

    if kind == "act":
        kw = lambda p: dict(p.kw, out=p.out)  # noqa: E731
        return RC("gemm", tag or f"{route}-{name}", (f"gemm:{route}",), build,
                  lambda p: _ops().gemm_bias_act(p.xin, p.w, p.b, p.act, **kw(p)), lambda p, y: {"y": y}, judge,
                  route=lambda p: _ops().gemm_route(p.xin, p.w, p.b, p.act, **kw(p)), want=route,
                  outputs=lambda p: {"out": (p.shape[:2], p.dtype)}, host=False)

    def written(p, ret):
        y, stats = ret
        M = p.shape[0]
        return {"y": y[:M], "stats": None if stats is None else stats[:, :M]}

    return RC("gemm", tag or f"{route}-{name}", (f"gemm:{route}",), build, lambda p: _gm()._ln_launch(p), written, judge,
              route=lambda p: _gm()._ln_route_of(p), want=route, host=False)


def _blocked_io_case():
    """The consumer with the blocked activation layout on both sides: judged through the row-major launch of the same operands
    (test_gemm_route's "blocked_x_and_out" judges that one and asserts the two equal bit for bit)."""
    def build(dtype, dev):
        from test_gpu_kernels import _block
        p = _gm().CASES["p8w_fold"]["blocked_x_and_out"].build(dtype)
        p.xb = _block(p.x)
        return p

    def launch(p):
        return _ops().gemm_ln(p.xb, p.wb, p.b, x_blocked=True, out_blocked=True, **p.kw)

    def written(p, ret):
        from test_gpu_kernels import _unblock
        M, N, _ = p.shape
        return {"y": _unblock(ret[0], M, N)}

    def judge(p, ret):
        _loops(p.shape[0], p.shape[1])
        z = _gm()._ln_launch(p)
        _gm()._fold_judge(p, z)
        assert torch.equal(written(p, ret)["y"], z[0]), "blocked x / blocked output differs from the row-major launch"

    return RC("gemm", "p8w_fold-blocked_x_and_out", ("gemm:p8w_fold",), build, launch, written, judge,
              route=lambda p: _ops().gemm_route(p.xb, p.wb, p.b, x_blocked=True, out_blocked=True, **p.kw), want="p8w_fold",
              host=False)


def _rms_fold_case():
    """The RMSNorm fold on the producer's stream of 65 row tiles: test_gpu_rmsnorm._rms_consumer's operands and judgement."""
    M, K, seed = 16500, 1024, 5

    def build(dtype, dev):
        gm, ops = _gm(), _ops()
        N = _wide(M, 2048)
        y, stats = gm._fold_stream(dtype, M, K, seed)
        gam = gm._rand((K,), dtype, 0.2, seed + 4, shift=1.0)
        wc_, bc = gm._rand((N, K), dtype, K ** -0.5, seed + 6), gm._rand((N,), dtype, 0.1, seed + 7)
        ws, _ = ops.rms_fold_weight(wc_, gam, bc, blocked=False)
        wb, _ = ops.rms_fold_weight(wc_, gam, bc)
        return SimpleNamespace(dtype=dtype, route="p8w_fold", shape=(M, N, K), x=y, wb=wb, b=bc, ws=ws,
                               kw=dict(M=M, N=N, K=K, activation="none", ln_stats=stats, eps=1e-6, norm="rms"))

    def judge(p, ret):
        _loops(M, p.shape[1])
        stl = _ops().ln_stats_for_launch(p.kw["ln_stats"], M)
        ref = rmc.reference_fold_rms(p.x, stl[:, :M], p.ws, p.b, eps=1e-6, act="none", col_scale=None, device=DEV)
        gc.check(ret[0], ref, p.dtype, "p8w_fold", bars=gc.BARS[(p.dtype, "p8w_fold")], what="rms fold")

    return RC("gemm", "p8w_fold-rms", ("gemm:p8w_fold", "fold:rms"), build, lambda p: _gm()._ln_launch(p),
              lambda p, ret: {"y": ret[0]}, judge, route=lambda p: _gm()._ln_route_of(p), want="p8w_fold", host=False)


def _gemm_cases():
    gm = _gm()
    out = [
        _table_case("t128", "m300_n512_k1024", "act", persistent=False),
        _table_case("t256", "k264_none", "act", persistent=False),
        _table_case("glu_t128x64", "n_ragged_no_bias_gate", "act", persistent=False),
        _table_case("glu_t256x128", "n4104", "act", persistent=False),
        # the persistent routes: the table's case, rebuilt from its arguments with N = _wide(M, the table's N)
        _table_case("p8w", "blocked_w_k544", "act",
                    parts=lambda: gm._gemm_parts("p8w", 4096 + 37, _wide(4096 + 37, 4096 + 8), 544, "silu", blocked_w=True)),
        _table_case("p8w_res", "k4096", "act",
                    parts=lambda: gm._gemm_parts("p8w_res", 4096 + 100, _wide(4096 + 100, 4096 + 8), 4096, res=True)),
        _table_case("p8w_stats", "n1024_k1024", "ln", parts=lambda: gm._stats_parts(16500, _wide(16500, 1024), 1024)),
        _table_case("p8w_fold", "none", "ln", parts=lambda: gm._fold_parts("p8w_fold", gm.MP, _wide(gm.MP, 2048), 1024, "none")),
        # K 4096: 16 statistic slots summed to 8 by ln_stats_reduce; the table's shape at the 65 row tiles of MP
        _table_case("p8w_fold", "k4096", "ln", tag="p8w_fold-k4096-m16500",
                    parts=lambda: gm._fold_parts("p8w_fold", gm.MP, _wide(gm.MP, 2048), 4096, "none", seed=4096)),
        _table_case("p8w_glu", "gemm_ln_ragged_m_k1024", "ln",
                    parts=lambda: gm._glu_ln_parts("p8w_glu", 4096 + 100, _wide(4096 + 100, 2048, True), 1024, seed=2)),
        _table_case("p8w_glu_fold", "gemm_ln_fold", "ln",
                    parts=lambda: gm._fold_parts("p8w_glu_fold", gm.MP, _wide(gm.MP, 2048, True), 1024, "swiglu")),
        _rms_fold_case(),
        _blocked_io_case(),
    ]
    return out


def _mlp_case(act, blocked):
    """The two launches of one test_fused_mlp_paths case, as two cases: without the residual and with it."""
    def one(res):
        parts = lambda: _gm()._mlp_parts(act, blocked, res, seed=3 * res)  # noqa: E731

        def build(dtype, dev):
            return parts().build(dtype)

        covers = ("mlp:" + act + (":blocked" if blocked else ":two_launch"),)
        return RC("mlp", f"{act}-{'blocked' if blocked else 'two_launch'}-{'res' if res else 'plain'}", covers, build,
                  lambda p: _gm()._mlp_launch(p), lambda p, y: {"y": y[0]}, lambda p, y: parts().judge(p, y),
                  route=lambda p: _gm()._mlp_route_of(p), host=False)
    return [one(False), one(True)]


MLP_ACTS = ["gelu", "gelu_erf", "relu", "silu", "swiglu"]


def _mlp_cases():
    return [c for act in MLP_ACTS for blocked in (True, False) for c in _mlp_case(act, blocked)]


# ---------------------------------------------------------------------------------------------------------------------
# decode GEMM (alone: test_deterministic_and_graph): the cold and co-run conditions, both weight forms
# ---------------------------------------------------------------------------------------------------------------------
def _skinny_case(c, w8):
    def build(dtype, dev):
        if w8:
            import test_gpu_gemm_skinny_w8 as t8
            x, q, s, b, r, qg, sg, bg = t8._operands(dtype, c)
            return SimpleNamespace(dtype=dtype, x=x, q=q, s=s, b=b, r=r, qg=qg, sg=sg, bg=bg)
        import test_gpu_gemm_skinny as ts
        x, w, b, r, wg, bg = ts._operands(dtype, c.M, c.N, c.K, c.bias, c.res, c.seed, c.ldx, c.glu, c.bias_gate)
        return SimpleNamespace(dtype=dtype, x=x, w=w, b=b, r=r, wg=wg, bg=bg)

    def launch(p):
        if w8:
            return _ops().gemm_skinny_w8(p.x, p.q, p.s, p.b, c.act, p.qg, p.sg, p.bg, residual=p.r, out=p.out)
        return _ops().gemm_skinny(p.x, p.w, p.b, c.act, w_gate=p.wg, bias_gate=p.bg, residual=p.r, out=p.out)

    def judge(p, y):
        assert y.data_ptr() == p.out.data_ptr()
        if w8:
            w8c.judge(y, w8c.reference_w8(p.x, p.q, p.s, p.b, c.act, p.qg, p.sg, p.bg, p.r, device=DEV), p.dtype, c.what)
        else:
            import test_gpu_gemm_skinny as ts
            ts._judge(y, gc.reference(p.x, p.w, p.b, c.act, p.wg, p.bg, p.r, device=DEV), p.dtype, c.what)

    splits = (lambda p: _ops().gemm_skinny_w8_splits(c.M, c.N, c.K, c.act) > 1) if w8 else \
        (lambda p: _ops().gemm_skinny_splits(c.M, c.N, c.K, c.act) > 1)
    return RC("decode_gemm", f"{'w8' if w8 else 'w16'}-{c.what.replace(' ', '-')}", ("skinny:w8" if w8 else "skinny:w16",), build,
              launch, lambda p, y: {"y": y}, judge, route=splits, want=True,
              outputs=lambda p: {"out": ((c.M, c.N), p.dtype)}, conditions="noise", host=False)


def _skinny_cases():
    glu16 = next(c for c in sk.DEEP_SPLIT if c.glu and c.M == 64)
    glu8 = next(c for c in wc.DEEP_SPLIT if c.glu and c.M == 64)
    return ([_skinny_case(c, False) for c in sk.DETERMINISTIC + [glu16]] +
            [_skinny_case(c, True) for c in wc.DETERMINISTIC + [glu8]])


# ---------------------------------------------------------------------------------------------------------------------
# one-time preparations
# ---------------------------------------------------------------------------------------------------------------------
def _rand(shape, dtype, dev, scale=1.0, seed=0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale + shift).to(dtype).to(dev)


def _prep_cases():
    N, K = 600, 1024   # three 256-row tiles, the last ragged

    def bw_build(dtype, dev):
        return SimpleNamespace(dtype=dtype, w=_rand((N, K), dtype, dev, 0.03, 1), wg=_rand((N, K), dtype, dev, 0.03, 2))

    def bw_judge(p, wb):
        from test_gpu_kernels import _block
        assert torch.equal(wb, _block(p.w)), "block_weight is not the blocked layout of w (rows past N zero)"

    def glu_judge(p, wb):
        # include/mio_hip.h: row wn * 64 + h * 32 + j of tile tn <- row tn * 128 + wn * 32 + j of the gate (h 0) / up (h 1) weight
        tn = (N + 127) // 128
        pad = lambda t: torch.cat([t, torch.zeros(tn * 128 - N, K, dtype=t.dtype, device=t.device)])  # noqa: E731
        g4, u4 = (pad(t).view(tn, 4, 32, K // 32, 32) for t in (p.wg, p.w))
        want = torch.stack([g4, u4], dim=2).permute(0, 4, 1, 2, 3, 5).reshape(tn * 256, K)
        assert torch.equal(wb, want), "block_weight_glu is not the interleaved blocked layout (rows past I zero)"

    out = [RC("prep", "block_weight", ("prep:block_weight",), bw_build, lambda p: _ops().block_weight(p.w),
              lambda p, r: {"wb": r}, bw_judge, host=True),
           RC("prep", "block_weight_glu", ("prep:block_weight_glu",), bw_build, lambda p: _ops().block_weight_glu(p.wg, p.w),
              lambda p, r: {"wb": r}, glu_judge, host=True)]

    for Kf in (256, 8192):
        def fold_build(dtype, dev, Kf=Kf):
            g = torch.Generator(device=dev).manual_seed(Kf)
            gamma, w, beta, bias = _gm()._fold_weight_inputs(dtype, Kf, False, g)
            return SimpleNamespace(dtype=dtype, gamma=gamma, w=w, beta=beta, bias=bias)

        def fold_launch(p, Kf=Kf):
            lib = _lib().lib
            rcode = lib.mio_ln_fold_weight(p.w.data_ptr(), p.w.stride(0), p.gamma.data_ptr(), p.beta.data_ptr(),
                                           p.bias.data_ptr(), p.ws.data_ptr(), p.bo.data_ptr(), p.w.shape[0], Kf,
                                           _ops()._dtype_id(p.w), torch.cuda.current_stream().cuda_stream)
            assert rcode == 0, lib.mio_last_error()
            return p.ws, p.bo

        def fold_judge(p, ret, Kf=Kf):
            gm = _gm()
            ws, bo = ret
            assert bool(torch.isfinite(ws).all() and torch.isfinite(bo).all())
            gm._check_fold_rows(ws, p.w, p.gamma, p.dtype, False, f"ln_fold_weight K {Kf}")
            gm._check_bias_out(bo, p.w, p.beta, p.bias, p.dtype, f"ln_fold_weight K {Kf}")

        out.append(RC("prep", f"ln_fold_weight-k{Kf}", ("prep:ln_fold_weight",), fold_build, fold_launch,
                      lambda p, ret: {"ws": ret[0], "bias": ret[1]}, fold_judge,
                      outputs=lambda p: {"ws": (tuple(p.w.shape), p.dtype), "bo": ((p.w.shape[0],), p.dtype)}, host=False,
                      # K 8192: eight launches take some fifty times the usual memory noise and 150 times the matrix noise
                      noise=(64, 192) if Kf == 8192 else (1, 1)))

    def rms_build(dtype, dev):
        return SimpleNamespace(dtype=dtype, w=_rand((N, K), dtype, dev, 0.03, 5), gamma=_rand((K,), dtype, dev, 0.2, 6, shift=1.0))

    def rms_judge(p, ret):
        from test_gpu_kernels import _block
        want = (p.w.double() * p.gamma.double()).to(p.dtype)
        assert ret[1] is None and torch.equal(ret[0], _block(want)), "rms_fold_weight is not one rounding of w * gamma, blocked"

    out.append(RC("prep", "rms_fold_weight", ("prep:rms_fold_weight",), rms_build, lambda p: _ops().rms_fold_weight(p.w, p.gamma),
                  lambda p, ret: {"wb": ret[0]}, rms_judge, host=True))

    def q_build(dtype, dev):
        return SimpleNamespace(dtype=dtype, w=_rand((73, 1040), dtype, dev, 0.05, 7))

    def q_judge(p, ret):
        import test_gpu_gemm_skinny_w8 as t8
        q, s = ret
        eq, es = t8._quant_expect(p.w)
        assert torch.equal(s.cpu().view(torch.int32), es.view(torch.int32)), "quantize_weight_w8: the scales"
        assert torch.equal(q.cpu().view(torch.uint8), eq.view(torch.uint8)), "quantize_weight_w8: the bytes"

    out.append(RC("prep", "quantize_weight_w8", ("prep:quantize_weight_w8",), q_build, lambda p: _ops().quantize_weight_w8(p.w),
                  lambda p, ret: {"w8": ret[0], "scale": ret[1]}, q_judge, host=True))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# cache writes and rotary on the scene of tests/test_gpu_rope.py
# ---------------------------------------------------------------------------------------------------------------------
_SCENE = dict(D=128, rot=64, H=8, Hkv=2, bs=16, use_positions=True, seed=99)
WRITES = ("reshape_and_cache", "reshape_and_cache_varlen", "rope_and_cache_varlen", "qknorm_rope_and_cache_varlen")


def _scene(dtype, kv8):
    import test_gpu_rope as tr
    sc = tr._Scene(dtype, kv8, _SCENE["D"], _SCENE["rot"], H=_SCENE["H"], Hkv=_SCENE["Hkv"], bs=_SCENE["bs"],
                   use_positions=_SCENE["use_positions"], seed=_SCENE["seed"])
    g = torch.Generator().manual_seed(5)
    sc.wq = (0.5 + torch.rand(sc.D, generator=g)).to(dtype)
    sc.wk = (1.5 - torch.rand(sc.D, generator=g) * torch.linspace(0.2, 1.0, sc.D)).to(dtype)
    return sc


def single_writer(sc, tokens):
    """Every cache slot the given packed tokens fill is filled by one of them only: the scene shares pages between two
    sequences, and two writers of one slot would make the result depend on their order."""
    pairs = list(zip(sc.blk[tokens].tolist(), sc.slot[tokens].tolist()))
    return len(pairs) == len(set(pairs)) and len(pairs) > 0


def _sentinel_caches(sc, dev):
    shape = (sc.nb, sc.L, sc.bs, sc.Hkv, sc.D)
    if sc.kv8:
        c = torch.full(shape, SENT, dtype=torch.uint8, device=dev).view(F8)
    else:
        c = torch.full(shape, SENT, dtype=torch.uint8, device=dev).repeat_interleave(2, -1).view(sc.dtype)
    return c, c.clone()


def _b(t):
    return t.detach().cpu().contiguous().view(torch.uint8)


def _stored(sc, x, scale):
    """What a plain cache write stores of the rows x: the bytes themselves, or the e4m3 quantisation."""
    return dc.quantise(x, scale) if sc.kv8 else x


def _expect_plain(sc, which, tokens, rows):
    """The cache (CPU) after a plain write of rows [n, Hkv, D] for the packed tokens `tokens` into the sentinel cache."""
    exp = _sentinel_caches(sc, "cpu")[which]
    scale = (sc.k_scale, sc.v_scale)[which][sc.layer] if sc.kv8 else 1.0
    exp[sc.blk[tokens], sc.layer, sc.slot[tokens]] = _stored(sc, rows, scale)
    return exp


def _write_case(op, kv8):
    def build(dtype, dev):
        sc = _scene(dtype, kv8)
        kc, vc = _sentinel_caches(sc, dev)
        p = SimpleNamespace(dtype=dtype, qkv=sc.qkv.to(dev), kc=kc, vc=vc, bt=sc.bt.to(dev), cu=sc.cu.to(dev), cl=sc.cl.to(dev),
                            cos=sc.cos.to(dev), sin=sc.sin.to(dev), pos=sc.positions.to(dev), wq=sc.wq.to(dev), wk=sc.wk.to(dev),
                            scales={}, ref=SimpleNamespace(sc=sc))
        if kv8:
            p.scales = dict(k_scale=torch.tensor(sc.k_scale, dtype=torch.float32, device=dev),
                            v_scale=torch.tensor(sc.v_scale, dtype=torch.float32, device=dev))
        return p

    def launch(p):
        ops, sc = _ops(), p.ref.sc
        q, k, v = sc.views(p.qkv)
        if op == "reshape_and_cache":   # a decode step: the first token of the packed rows for each of the four sequences
            return ops.reshape_and_cache(k[:4][:, None], v[:4][:, None], p.kc, p.vc, p.bt, p.cl, sc.bs, sc.layer, **p.scales)
        if op == "reshape_and_cache_varlen":
            return ops.reshape_and_cache_varlen(k, v, p.kc, p.vc, p.bt, p.cu, p.cl, sc.bs, sc.layer, **p.scales)
        if op == "rope_and_cache_varlen":
            return ops.rope_and_cache_varlen(q, k, v, p.kc, p.vc, p.bt, p.cu, p.cl, sc.bs, sc.layer, p.cos, p.sin, positions=p.pos,
                                             q_out=p.q_out, **p.scales)
        return ops.qknorm_rope_and_cache_varlen(q, k, v, p.kc, p.vc, p.bt, p.cu, p.cl, sc.bs, sc.layer, p.cos, p.sin, p.wq, p.wk,
                                                eps=EPS_QK, positions=p.pos, q_out=p.q_out, **p.scales)

    rotating = op in WRITES[2:]

    def written(p, ret):
        w = {"k_cache": p.kc, "v_cache": p.vc}
        if rotating:
            w["q_out"] = p.q_out
        return w

    def judge(p, ret):
        import test_gpu_rope as tr
        sc = p.ref.sc
        q_cpu, k_cpu, v_cpu = sc.views(sc.qkv)
        kcb, vcb = p.kc.cpu(), p.vc.cpu()
        if op == "reshape_and_cache":
            pos = sc.cl.long() - 1
            ok = pos < sc.M * sc.bs
            b = torch.arange(4)[ok]
            blk, slot = sc.bt[b, pos[ok] // sc.bs].long(), pos[ok] % sc.bs
            assert len(set(zip(blk.tolist(), slot.tolist()))) == len(b) == 3
            for which, (got, src) in enumerate(((kcb, k_cpu), (vcb, v_cpu))):
                exp = _sentinel_caches(sc, "cpu")[which]
                scale = (sc.k_scale, sc.v_scale)[which][sc.layer] if sc.kv8 else 1.0
                exp[blk, sc.layer, slot] = _stored(sc, src[b], scale)
                assert torch.equal(_b(got), _b(exp)), f"{op}: cache {which} is not the plain write"
            return
        if op == "reshape_and_cache_varlen":
            t = sc.has_row
            assert single_writer(sc, t)
            assert torch.equal(_b(kcb), _b(_expect_plain(sc, 0, t, k_cpu[t]))), f"{op}: the K cache"
            assert torch.equal(_b(vcb), _b(_expect_plain(sc, 1, t, v_cpu[t]))), f"{op}: the V cache"
            return
        wr = sc.live & sc.has_row
        assert single_writer(sc, wr)
        if op == "rope_and_cache_varlen":   # the existing judgement of the same scene, and its result bit for bit
            qo, kj, vj = tr._run_scene(sc, False, alias=False)
            assert torch.equal(_b(p.q_out), _b(qo)) and torch.equal(_b(kcb), _b(kj)) and torch.equal(_b(vcb), _b(vj))
            return
        # QK-norm: q_out and the written K rows inside the derived interval, dead q rows zero, V the plain write, the rest untouched
        qo = p.q_out.cpu()
        live = sc.live
        assert (_b(qo[~live]) == 0).all()
        ref_q, dq = qc.reference(q_cpu[live], sc.wq, EPS_QK, sc.cos, sc.sin, sc.rpos[live], False)
        assert qc.outside16(qo[live], ref_q, dq, sc.dtype)[0] == 0
        assert torch.equal(_b(vcb), _b(_expect_plain(sc, 1, wr, v_cpu[wr])))
        blk, slot = sc.blk[wr], sc.slot[wr]
        krows = kcb[blk, sc.layer, slot]
        exp_k = _sentinel_caches(sc, "cpu")[0]
        exp_k[blk, sc.layer, slot] = krows
        assert torch.equal(_b(kcb), _b(exp_k)), "K cache bytes outside the written rows changed"
        ref_k, dk = qc.reference(k_cpu[wr], sc.wk, EPS_QK, sc.cos, sc.sin, sc.rpos[wr], False)
        if sc.kv8:
            assert qc.outside8(krows, ref_k, dk, sc.k_scale[sc.layer]) == 0
        else:
            assert qc.outside16(krows, ref_k, dk, sc.dtype)[0] == 0

    outputs = (lambda p: {"q_out": ((p.ref.sc.T, p.ref.sc.H, p.ref.sc.D), p.dtype)}) if rotating else None
    return RC("cache_write", f"{op}-{'fp8' if kv8 else 'kv16'}", (f"write:{op}",), build, launch, written, judge, outputs=outputs)


def _rotary_case(op, inplace):
    def build(dtype, dev):
        sc = _scene(dtype, False)
        rpos = torch.where(sc.seq >= 0, sc.rpos, torch.full_like(sc.rpos, -1)).to(torch.int32)
        return SimpleNamespace(dtype=dtype, qkv=sc.qkv.to(dev), cos=sc.cos.to(dev), sin=sc.sin.to(dev), pos=rpos.to(dev),
                               wq=sc.wq.to(dev), ref=SimpleNamespace(sc=sc))

    def launch(p):
        q = p.ref.sc.views(p.qkv)[0]
        out = q if inplace else p.out
        if op == "apply_rotary":
            return _ops().apply_rotary(q, p.cos, p.sin, p.pos, out=out)
        return _ops().qk_norm_rotary(q, p.wq, p.cos, p.sin, p.pos, eps=EPS_QK, out=out)

    def judge(p, ret):
        sc = p.ref.sc
        q_cpu = sc.views(sc.qkv)[0]
        y, live, rot = ret.cpu(), sc.live, sc.rot
        assert ret.data_ptr() == (p.ref.sc.views(p.qkv)[0] if inplace else p.out).data_ptr()
        assert (_b(y[~live]) == 0).all(), "rows without a valid position are not zero"
        if op == "apply_rotary":
            ref, delta = rc.reference(q_cpu[live], sc.cos, sc.sin, sc.rpos[live], False)
            assert rc.outside16(y[live][..., :rot], ref, delta, sc.dtype)[0] == 0
            assert torch.equal(_b(y[live][..., rot:]), _b(q_cpu[live][..., rot:]))
        else:
            ref, delta = qc.reference(q_cpu[live], sc.wq, EPS_QK, sc.cos, sc.sin, sc.rpos[live], False)
            assert qc.outside16(y[live], ref, delta, sc.dtype)[0] == 0
        if inplace:  # k and v of the fused buffer are untouched
            for got, want in zip(sc.views(p.qkv.cpu())[1:], sc.views(sc.qkv)[1:]):
                assert torch.equal(_b(got), _b(want))

    outputs = None if inplace else (lambda p: {"out": ((p.ref.sc.T, p.ref.sc.H, p.ref.sc.D), p.dtype)})
    return RC("rotary", f"{op}-{'in_place' if inplace else 'out_of_place'}", (f"write:{op}",), build, launch,
              lambda p, ret: {"y": ret}, judge, outputs=outputs)


def _write_cases():
    return ([_write_case(op, kv8) for op in WRITES for kv8 in (False, True)] +
            [_rotary_case(op, ip) for op in ("apply_rotary", "qk_norm_rotary") for ip in (False, True)])


# ---------------------------------------------------------------------------------------------------------------------
# row kernels
# ---------------------------------------------------------------------------------------------------------------------
ROWS, ALPHA = 257, 0.5


def _norm_case(rms, cols, blocked):
    eps = 1e-6 if rms else rw.EPS

    def build(dtype, dev):
        x, res, w, b, _ = rw.ln_case(dtype, ROWS, cols, dev)
        return SimpleNamespace(dtype=dtype, x=x, res=res, w=w, b=b)

    def outputs(p):
        return {"y": (((ROWS + 255) // 256 * 256 if blocked else ROWS, cols), p.dtype), "s": ((ROWS, cols), p.dtype)}

    def launch(p):
        lib = _lib().lib
        dt = _lib().MIO_BF16 if p.dtype == torch.bfloat16 else _lib().MIO_FP16
        tail = (p.y.data_ptr(), p.s.data_ptr(), ROWS, cols, ctypes.c_float(eps), ctypes.c_float(ALPHA), dt)
        stream = torch.cuda.current_stream().cuda_stream
        if rms:
            rcode = lib.mio_rmsnorm_fwd(p.x.data_ptr(), p.res.data_ptr(), p.w.data_ptr(), *tail, int(blocked), stream)
        else:
            entry = lib.mio_layernorm_fwd_bx if blocked else lib.mio_layernorm_fwd
            rcode = entry(p.x.data_ptr(), p.res.data_ptr(), p.w.data_ptr(), p.b.data_ptr(), *tail, stream)
        assert rcode == 0, lib.mio_last_error()
        return p.y, p.s

    def judge(p, ret):
        from test_gpu_kernels import _unblock
        y, s = ret
        what = f"{'rmsnorm' if rms else 'layernorm'} cols {cols} blocked {blocked}"
        if blocked:
            pad = y.view(2, cols // 32, 256, 32)[1, :, 1:]
            assert bool((pad.contiguous().view(torch.uint8) == 0xFF).all()), "rows past 257 of the blocked output were written"
            y = _unblock(y, ROWS, cols)
        sref, sbound = rmc.sum_bound(p.x, p.res, ALPHA, p.dtype, device=DEV)
        serr = (s.double() - sref).abs()
        assert bool((serr <= sbound).all()), f"{what}: sum_out off by {(serr / sbound).max().item():.3g} x its bound"
        assert bool(torch.isfinite(y).all()), what
        if rms:
            gc.check(y, rmc.reference_rows(s, p.w, eps, device=DEV), p.dtype, "rmsnorm", bars=False, what=what)
        else:
            rw.admissible(y, rw.reference_layernorm(s, p.w, p.b, eps, device=DEV), p.dtype, what)

    name = "rmsnorm" if rms else "layernorm"
    return RC("rows", f"{name}-cols{cols}-{'blocked' if blocked else 'rows'}", (f"row:{name}",), build, launch,
              lambda p, ret: {"y": ret[0], "sum": ret[1]}, judge, outputs=outputs)


def _merge_case(out_dtype):
    shape = rw.MERGE_SHAPES[1]
    B, Sq, H, D = shape

    def build(dtype, dev):
        o_a, l_a, o_b, l_b = rw.merge_states(*shape, seed=sum(shape), device=dev)
        return SimpleNamespace(dtype=dtype, o_a=o_a, l_a=l_a, o_b=o_b, l_b=l_b,
                               ref=SimpleNamespace(st=(o_a.clone(), l_a.clone(), o_b.clone(), l_b.clone())))

    def launch(p):
        _ops().attn_merge(p.o_a, p.l_a, p.o_b, p.l_b, out=p.out)
        return p.out

    def judge(p, ret):
        ref, L, tol = rw.reference_merge(*p.ref.st, device=DEV)
        rw.within32(p.o_a, ref, "merge")
        rw.lse_within(p.l_a, L, tol, "merge")
        assert torch.equal(p.o_b, p.ref.st[2]) and torch.equal(p.l_b, p.ref.st[3]), "side b was written"
        assert rw.admissible(p.out.view(-1, D), ref, out_dtype, "merge") <= rw.CAP_MERGE
        assert torch.equal(p.out, p.o_a.to(out_dtype)), "o_out is not the rounding of o_a"

    return RC("rows", f"attn_merge-{str(out_dtype).split('.')[-1]}", ("row:attn_merge",), build, launch,
              lambda p, ret: {"o_a": rp.Attn(p.o_a, "bshd"), "lse_a": rp.Attn(p.l_a, "bhs"), "out": rp.Attn(p.out, "bshd")}, judge,
              outputs=lambda p: {"out": ((B, Sq, H, D), out_dtype)}, dtypes=(out_dtype,))


def _row_cases():
    out = []
    for rms in (False, True):
        # (a blocked output takes cols % 32 == 0: 1032 has the row-major form only)
        out += [_norm_case(rms, 1032, False), _norm_case(rms, 4096, False), _norm_case(rms, 4096, True)]
    return out + [_merge_case(dt) for dt in DTYPES]


# ---------------------------------------------------------------------------------------------------------------------
# module level: one Block of tests/_module_check.py's table per fold; the final tensor is compared
# ---------------------------------------------------------------------------------------------------------------------
def _clone(v):
    if isinstance(v, torch.Tensor):
        return rp.place(v)
    if isinstance(v, (list, tuple)):
        return type(v)(_clone(e) for e in v)
    if isinstance(v, dict):
        return {k: _clone(e) for k, e in v.items()}
    return v


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return torch.equal(rp.snapshot({"t": a})["t"].data, rp.snapshot({"t": b})["t"].data)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    return True


# the launches of the decode step that _module_trace.WRAPPED (the golden traces' list) does not name
MORE_WRAPPED = ("qk_norm_rotary", "qknorm_rope_and_cache_varlen", "rope_and_cache_varlen", "reshape_and_cache",
                "reshape_and_cache_varlen", "gemm_skinny", "gemm_skinny_w8", "quantize_weight_w8")


def first_differing_launch(run):
    """run() once with every launch of _module_trace.WRAPPED and MORE_WRAPPED recorded with copies of its arguments before and
    after the call and of what it returned; then each launch once more, alone, on its recorded arguments.  Returns "launch i:
    name" of the first whose result, or whose arguments after the call (out=, caches, in-place forms), are not the recorded ones
    byte for byte, or None.  One pass, no retries.  _module_trace.record itself keeps shapes, not tensors, and its call list is
    what the golden traces are compared with, so the wrapping is repeated here on its list of names.  (A result with rows its
    kernel never writes -- statistics and blocked rows past M -- is compared whole: read the named kernel before believing it.)"""
    from _module_trace import WRAPPED
    ops = _ops()
    recs, depth = [], [0]
    saved = {name: getattr(ops, name) for name in WRAPPED + MORE_WRAPPED}

    def wrap(name, fn):
        def call(*a, **k):
            if depth[0]:   # a nested launch belongs to its caller
                return fn(*a, **k)
            before = _clone((a, k))
            depth[0] += 1
            try:
                out = fn(*a, **k)
            finally:
                depth[0] -= 1
            recs.append((name, fn, before, _clone((a, k)), _clone(out)))   # the arguments afterwards: out=, caches, in place
            return out
        return call

    for name, fn in saved.items():
        setattr(ops, name, wrap(name, fn))
    try:
        run()
    finally:
        for name, fn in saved.items():
            setattr(ops, name, fn)
    torch.cuda.synchronize()
    for i, (name, fn, before, after, out) in enumerate(recs):
        a, k = before
        again = fn(*a, **k)
        torch.cuda.synchronize()
        if not _same(again, out):
            return f"launch {i}: {name}"
        if not _same(before, after):   # (before now holds the arguments as the repeated launch left them)
            return f"launch {i}: {name} (an argument it writes)"
    return None


def _block_case(name):
    def build(dtype, dev):
        assert _is_dev(dev)
        import _module_check as mc
        import test_gpu_module_rows as tmr
        st_ = tmr._build(mc.case(name), dtype)
        return SimpleNamespace(dtype=dtype, x=st_["x"].to(dev), ref=SimpleNamespace(st=st_))

    @torch.no_grad()
    def launch(p):
        st_ = p.ref.st
        return st_["blocks"][0]["m"](p.x, stream_out=False, fold=st_["c"]["fold"])

    def written(p, ret):
        return {"y": ret.reshape(-1, ret.shape[-1])}

    def judge(p, ret):
        """tests/test_gpu_module_rows.py's own run of the same block (routes asserted, every sub-layer judged on its actual
        input), and its final tensor bit for bit the one compared here."""
        import test_gpu_module_rows as tmr
        seen = []
        hook = p.ref.st["blocks"][0]["m"].register_forward_hook(lambda _m, _i, o: seen.append(o))
        try:
            tmr._run(p.ref.st)
        finally:
            hook.remove()
        assert len(seen) == 1 and torch.equal(seen[0].view(torch.int16), ret.view(torch.int16)), "the judged run differs"
        seen[0].view(torch.int16).fill_(-1)   # its block goes back to the allocator as 0xFF, not as the right answer

    return RC("module", name, (f"module:{name}",), build, launch, written, judge, host=False)


DECODE_STEP = dict(d=4096, H=32, Hkv=8, bs=16, ctxs=(700, 333, 1000), msl=1100, scales=(0.043, 0.02))


def _decode_step_case():
    """One FlashSelfAttention paged decode step with qk_norm, rotary, an fp8 cache, decode_gemm and decode_gemm_fp8: the new
    token's K / V go into the cache through ops.qknorm_rope_and_cache_varlen, then the layer runs the q projection and the output
    projection on ops.gemm_skinny_w8 (d 4096: the size from which ops.gemm_skinny_w8_ok advises it), ops.qk_norm_rotary on q and the
    split paged decode with its reduce.  The cache before the step (restored for every launch) holds the contexts, written the
    same way.  Judged as tests/test_gpu_qknorm.py judges the paged module (the fp64 chain over the cache as written) on the
    dequantised weights, at that file's bar (tr.MODULE_BARS: the worst normwise row error of the paged module) and at the bar
    of tests/test_gpu_decode_gemm_w8_modules.py (mean relative error below 5e-3)."""
    c = DECODE_STEP
    d, H, Hkv, bs, ctxs = c["d"], c["H"], c["Hkv"], c["bs"], list(c["ctxs"])
    D, B = d // H, len(ctxs)
    ks, vs = c["scales"]

    def build(dtype, dev):
        from mio.kernels.attention import flash_attention as fa
        ops = _ops()
        torch.manual_seed(17)
        cfg = fa.FlashAttentionConfig(causal=True, precision="bf16" if dtype == torch.bfloat16 else "fp16", rotary_dim=D,
                                      max_position=2048, qk_norm=True, qk_norm_eps=EPS_QK, decode_gemm=True, decode_gemm_fp8=True)
        layer = fa.FlashSelfAttention(d, H, cfg, num_kv_heads=Hkv).to(DEV).to(dtype).eval()
        g = torch.Generator().manual_seed(23)
        with torch.no_grad():
            layer.q_norm.weight.copy_((0.5 + torch.rand(D, generator=g)).to(dtype))
            layer.k_norm.weight.copy_((1.5 - torch.rand(D, generator=g) * torch.linspace(0.2, 1.0, D)).to(dtype))
        assert _nn_route(B, d) == "w8"
        M = (max(ctxs) + 1) // bs + 2
        bt = torch.randperm(B * M, generator=g).view(B, M).to(torch.int32)
        kc = torch.full((B * M, 1, bs, Hkv, D), 0x7F, dtype=torch.uint8, device=DEV).view(F8)   # NaN where nothing is written
        vc = kc.clone()
        cos, sin = (t.to(DEV) for t in ops.rope_tables(2048, D))
        scales = dict(k_scale=torch.tensor([ks], device=DEV), v_scale=torch.tensor([vs], device=DEV))
        wqn, wkn = layer.q_norm.weight.detach(), layer.k_norm.weight.detach()

        def rows(n):  # K / V rows as the layer's projection would hand them over: unit scale, not centred
            return ((torch.randn(n, Hkv, D, generator=g) + 0.3).to(dtype).to(DEV) for _ in range(2))

        def write(p, kn, vn, n, after):
            cu = torch.tensor([0] + [sum(n[:i + 1]) for i in range(B)], dtype=torch.int32, device=DEV)
            cl = torch.tensor(after, dtype=torch.int32, device=DEV)
            ops.qknorm_rope_and_cache_varlen(torch.zeros(kn.shape[0], H, D, dtype=dtype, device=DEV), kn, vn, p.kc, p.vc, p.bt, cu,
                                             cl, bs, 0, p.cos, p.sin, wqn, wkn, eps=EPS_QK, **p.scales)
            return cl

        p = SimpleNamespace(dtype=dtype, bt=bt.to(DEV), cos=cos, sin=sin, scales=scales, kc=kc, vc=vc,
                            x=(torch.randn(B, 1, d, generator=g)).to(dtype).to(DEV))
        kn, vn = rows(sum(ctxs))
        write(p, kn, vn, ctxs, ctxs)
        p.kn, p.vn = rows(B)
        p.ref = SimpleNamespace(layer=layer, write=write, bt=bt, lens=[n + 1 for n in ctxs])
        return p

    @torch.no_grad()
    def launch(p):
        cl = p.ref.write(p, p.kn, p.vn, [1] * B, p.ref.lens)
        return p.ref.layer(p.x, physical_kv_cache_k=p.kc, physical_kv_cache_v=p.vc, block_tables=p.bt, context_lengths=cl,
                           kv_cache_block_size=bs, max_seq_len=c["msl"], layer_idx=0, **p.scales)

    def judge(p, y):
        import test_gpu_qknorm as tq
        import test_gpu_rope as tr
        ops, layer, dt, lens = _ops(), p.ref.layer, p.dtype, p.ref.lens
        assert _lib().lib.mio_fa3_decode_workspace_bytes(B, H, 1, D, c["msl"]) > 0, "a single split: no reduce in the chain"
        calls, real = [], ops.gemm_skinny_w8
        ops.gemm_skinny_w8 = lambda *a, **k: (calls.append(tuple(a[0].shape)), real(*a, **k))[1]
        try:   # the same step once more (it rewrites the same cache slots): both projections on the fp8 kernel, the same bits
            again = launch(p)
        finally:
            ops.gemm_skinny_w8 = real
        assert calls == [(B, 1, d), (B, 1, d)], calls
        assert torch.equal(again.view(torch.int16), y.view(torch.int16))
        again.view(torch.int16).fill_(-1)

        def deq(w):
            q, s = ops.quantize_weight_w8(w.detach().to(dt).contiguous())
            return (q.float().double() * s.double()[:, None]).cpu()

        sd = layer.state_dict()
        wq, bq = deq(sd["qkv_proj.weight"][:d]), sd["qkv_proj.bias"][:d].to(dt).double().cpu()
        wo, bo = deq(sd["o_proj.weight"]), sd["o_proj.bias"].to(dt).double().cpu()
        nq = layer.q_norm.weight.detach().to(dt).double().cpu()
        x = p.x.double().cpu()
        q = tq._norm64((x @ wq.t() + bq).view(B, 1, H, D), nq)
        q = torch.stack([tr._rot64(q[b], torch.arange(lens[b] - 1, lens[b]), D) for b in range(B)])
        o, _ = dc.reference(q.permute(0, 2, 1, 3), p.kc.cpu(), p.vc.cpu(), p.ref.bt, torch.tensor(lens), bs, 0, k_scale=ks,
                            v_scale=vs)
        ref = o.permute(0, 2, 1, 3).reshape(B, 1, d) @ wo.t() + bo
        assert bool(torch.isfinite(y).all())
        rel = ((y.double().cpu() - ref).abs().mean() / ref.abs().mean()).item()
        print(f"MODULE FlashSelfAttention decode step {str(dt).split('.')[-1]}: mean relative error {rel:.3e} (bar 5e-3), "
              f"worst row error {tr._row_err(y, ref, dt):.3f} u")
        assert rel < 5e-3 and tr._row_err(y, ref, dt) <= tr.MODULE_BARS[("FlashSelfAttention", dt, "paged")]

    return RC("module", "self_decode_step_qknorm_rope_fp8_w8", ("module:decode_step",), build, launch,
              lambda p, y: {"y": y.reshape(-1, y.shape[-1]), "k_cache": p.kc, "v_cache": p.vc}, judge, host=False)


def _nn_route(B, d):
    from mio import _nn
    return _nn.decode_route([(B, d, d, "none")], True, True)


def _module_cases():
    return [_block_case("block_fold"), _block_case("block_rms_swiglu"), _decode_step_case()]


def run_module_case(case, dtype):
    """run_case, and on a difference the launch-by-launch pass that names the first launch of the module that differs."""
    try:
        run_case(case, dtype)
    except AssertionError as e:
        if "not bit-reproducible" not in str(e):
            raise
        p = make_state(case, case.build(dtype, DEV), 0, DEV)
        raise AssertionError(f"{e}\nfirst differing launch, each repeated alone on recorded inputs: "
                             f"{first_differing_launch(lambda: case.launch(p))}") from None


# ---------------------------------------------------------------------------------------------------------------------
CASES = (_module_cases() +_prefill_cases() + _decode_cases() + _gemm_cases() + _mlp_cases() + _skinny_cases() + _prep_cases() + _write_cases()
         + _row_cases())
_GPU_ERROR = []
_PARAMS = [pytest.param(c, dt, id=f"{c.id}-{str(dt).split('.')[-1]}") for c in CASES for dt in c.dtypes]


@pytest.mark.parametrize("case,dtype", _PARAMS)
def test_repeatable(case, dtype):
    assert not _GPU_ERROR, f"not run: an earlier case of this process met a GPU error ({_GPU_ERROR[0]})"
    try:
        (run_module_case if case.family == "module" else run_case)(case, dtype)
        torch.cuda.synchronize()
    except RuntimeError as e:
        if "HIP" in str(e) or "hip" in str(e):  # the context is gone: the cases after this one queue nothing
            _GPU_ERROR.append(case.id)
        raise
    torch.cuda.empty_cache()


def test_first_differing_launch_names_the_launch(monkeypatch):
    """Three recorded launches, the second of which answers with its own call count: the pass names it, and names none once it
    is reproducible."""
    ops = _ops()
    x = torch.randn(37, 72, device=DEV).to(torch.bfloat16)
    w = torch.randn(72, 72, device=DEV).to(torch.bfloat16)
    g = torch.ones(72, dtype=torch.bfloat16, device=DEV)
    n = [0]

    def counting(x, weight, *a, **k):
        n[0] += 1
        return torch.full_like(x, float(n[0]))

    def run():
        ops.rmsnorm(ops.layernorm(ops.gemm_bias_act(x, w), g), g)

    assert first_differing_launch(run) is None
    monkeypatch.setattr(ops, "layernorm", counting)
    assert first_differing_launch(run) == "launch 1: layernorm"
    monkeypatch.undo()

    def writes_its_argument(x, weight, *a, **k):   # returns nothing; the call count goes into the argument, in place
        n[0] += 1
        x.fill_(float(n[0]))

    monkeypatch.setattr(ops, "rmsnorm", writes_its_argument)
    assert first_differing_launch(run) == "launch 2: rmsnorm (an argument it writes)"


def test_harness_reads_device_memory():
    """A launch that writes its call index into one element of a device tensor: run_repeats reports exactly that element for
    every repeat of the first condition and queues nothing further -- the comparison reads device memory for each repeat."""
    calls = []

    def launch(p):
        p.out[1, 300, 517] = float(len(calls))
        calls.append(1)
        return p.out

    res = rp.run_repeats(lambda s: SimpleNamespace(out=rp.fresh((2, 600, 600), torch.float32, DEV, s)), launch,
                         lambda p, ret: {"out": ret}, _conditions("all"))
    f = res.failure
    assert f is not None and f.condition == "back-to-back" and res.ran == ["back-to-back"] and len(calls) == 1 + rp.REPEATS
    assert [i for i, _ in f.repeats] == list(range(1, rp.REPEATS + 1))
    for _, diffs in f.repeats:
        d = diffs["out"]
        assert d.elements == 1 and d.first == (1, 300, 517) and 1 <= d.bytes <= 4
    assert "first at (1, 300, 517)" in str(f)

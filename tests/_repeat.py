"""Same inputs, same bits: snapshots of what a launch writes, their byte-wise comparison, and the driver that repeats a launch
under conditions (back to back, cold, beside noise on a second stream, at shifted addresses).  Torch only; runs on CPU tensors
as well (tests/test_repeat_host.py), so the reports are tested without a GPU.

Bytes, not values: NaN equals the same NaN, a changed NaN payload differs, and -0 differs from +0.

  snapshot(tensors)       name -> Snap: a uint8 view (no copy) of every written tensor; wrap an attention output in Attn(...)
  compare(first, other)   name -> Diff: differing bytes / elements, the first differing index, and the histograms that name the
                          kernel seam: (row // 256, col // 256) of a 2-D result, (sequence, head, row // 64) of an Attn one
  report(diffs)           the text of a failure
  run_repeats(...)        one judged launch, then every condition's launches against it; stops at the first differing condition
"""
import bisect
from collections import Counter
from dataclasses import dataclass, field
from typing import Optional

import torch

REPEATS = 8
SHIFTS = (16, 48, 4112)   # bytes: multiples of 16 that are no multiple of 32, of 64, and one past a 4 KiB page
TILE = 256                # the GEMM tile (rows and columns) of the 2-D histogram
ATTN_ROWS = 64            # the query rows of one attention work item
HIST_SHOWN = 12


# ---- buffers -----------------------------------------------------------------------------------------------------------------
def _span(shape, stride):
    return 1 + sum((n - 1) * s for n, s in zip(shape, stride)) if all(shape) else 0


def fresh(shape, dtype, device, shift=0, stride=None):
    """A tensor of 0xFF bytes (NaN in every float format here, -1 in the integer ones) whose first element lies `shift` bytes
    past the start of its own allocation; contiguous, or with the given element strides."""
    shape = tuple(shape)
    if stride is None:
        stride, n = [], 1
        for s in reversed(shape):
            stride.insert(0, n)
            n *= max(s, 1)
    item = torch.empty((), dtype=dtype).element_size()
    assert shift % item == 0
    buf = torch.full((_span(shape, stride) * item + shift,), 0xFF, dtype=torch.uint8, device=device)
    return buf[shift:].view(dtype).as_strided(shape, tuple(stride))


def place(t, shift=0, device=None):
    """A copy of t with t's shape and strides (gaps between rows hold 0xFF) on `device`, its base shifted as in fresh()."""
    if t is None:
        return None
    out = fresh(t.shape, t.dtype, t.device if device is None else device, shift, t.stride())
    if t.dtype in (torch.float8_e4m3fn, torch.float8_e5m2):
        out.view(torch.uint8).copy_(t.view(torch.uint8))
    else:
        out.copy_(t)
    return out


def aligned16(*tensors):
    """Every given tensor starts on a 16-byte boundary: what the ops document for their operands (include/mio_hip.h) and what
    a shifted launch must still satisfy."""
    return all(t is None or t.numel() == 0 or t.data_ptr() % 16 == 0 for t in tensors)


# ---- snapshots ---------------------------------------------------------------------------------------------------------------
@dataclass
class Attn:
    """Marks an attention result for the (sequence, head, row // 64) histogram.  layout names the dims: b batch, s query row,
    h head, d head dim, t packed token (then cu = the cumulative sequence lengths), e.g. "bshd", "bhs" (lse), "thd", "ht"."""
    tensor: torch.Tensor
    layout: str
    cu: Optional[tuple] = None


@dataclass
class Snap:
    data: torch.Tensor          # uint8 [*shape, itemsize], a view where the tensor allows one
    shape: tuple
    dtype: torch.dtype
    layout: Optional[str] = None
    cu: Optional[tuple] = None


def _bytes(t):
    t = t.detach()
    if t.dim() == 0:
        t = t.reshape(1)
    if t.stride(-1) != 1 and t.numel():
        t = t.contiguous()
    item = t.element_size()
    return t.view(torch.uint8).reshape(*t.shape, item)


def snapshot(tensors):
    """name -> Snap for a dict of written tensors (or Attn-wrapped ones); None entries are left out."""
    out = {}
    for name, t in tensors.items():
        if t is None:
            continue
        layout = cu = None
        if isinstance(t, Attn):
            t, layout, cu = t.tensor, t.layout, None if t.cu is None else tuple(int(c) for c in t.cu)
            assert len(layout) == t.dim(), (name, layout, tuple(t.shape))
        out[name] = Snap(_bytes(t), tuple(t.shape) if t.dim() else (1,), t.dtype, layout, cu)
    return out


# ---- comparison --------------------------------------------------------------------------------------------------------------
@dataclass
class Diff:
    bytes: int = 0
    elements: int = 0
    total: int = 0
    first: Optional[tuple] = None                  # index of the first differing element, in the tensor's own shape
    tiles: dict = field(default_factory=dict)      # 2-D results: (row // 256, col // 256) -> differing elements
    attn: dict = field(default_factory=dict)       # Attn results: (sequence, head, row // 64) -> differing elements

    def __bool__(self):
        return self.bytes > 0


def _attn_keys(idx, layout, cu):
    """(sequence, head, row // 64) of each differing element index (rows of idx)."""
    col = {c: idx[:, i].tolist() for i, c in enumerate(layout)}
    n = idx.shape[0]
    head = col.get("h", [0] * n)
    if "t" in col:
        seq = [bisect.bisect_right(cu, t) - 1 for t in col["t"]]
        row = [t - cu[s] for t, s in zip(col["t"], seq)]
    else:
        seq, row = col.get("b", [0] * n), col.get("s", [0] * n)
    return Counter(zip(seq, head, (r // ATTN_ROWS for r in row)))


def compare(first, other):
    """name -> Diff of two snapshots of the same launch.  Equal tensors cost one torch.equal on their own device."""
    assert first.keys() == other.keys(), (sorted(first), sorted(other))
    out = {}
    for name, a in first.items():
        b = other[name]
        assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape, a.dtype, b.dtype)
        d = Diff(total=a.data.numel() // max(a.data.shape[-1], 1))
        out[name] = d
        if torch.equal(a.data, b.data):
            continue
        ne = (a.data != b.data).cpu()
        d.bytes = int(ne.sum())
        idx = ne.any(-1).nonzero()
        d.elements = idx.shape[0]
        d.first = tuple(idx[0].tolist())
        if len(a.shape) == 2:
            d.tiles = dict(Counter(zip((idx[:, 0] // TILE).tolist(), (idx[:, 1] // TILE).tolist())))
        if a.layout is not None:
            d.attn = dict(_attn_keys(idx, a.layout, a.cu))
    return out


def _hist(h):
    items = sorted(h.items())
    s = ", ".join(f"{k}: {v}" for k, v in items[:HIST_SHOWN])
    return s + (f", ... {len(items) - HIST_SHOWN} more cells" if len(items) > HIST_SHOWN else "")


def report(diffs):
    """One line per differing tensor: counts, the first element, the histograms."""
    lines = []
    for name, d in diffs.items():
        if not d:
            continue
        s = f"{name}: {d.bytes} bytes in {d.elements} of {d.total} elements differ, first at {d.first}"
        if d.tiles:
            s += f"; (row // {TILE}, col // {TILE}) tiles {{{_hist(d.tiles)}}}"
        if d.attn:
            s += f"; (sequence, head, row // {ATTN_ROWS}) {{{_hist(d.attn)}}}"
        lines.append(s)
    return "\n".join(lines) if lines else "no difference"


# ---- the driver --------------------------------------------------------------------------------------------------------------
class Condition:
    """`repeats` launches of the same call with nothing around them.  Subclasses queue work around the launches."""
    name = "back-to-back"
    shifts = None             # a tuple of byte shifts: one launch per shift instead of `repeats` launches

    def __init__(self, name=None):
        if name is not None:
            self.name = name

    def start(self):          # before the first launch of the condition is queued
        pass

    def before(self, i):      # before launch i is queued, on the launch's stream
        pass

    def stop(self):           # after the last launch is queued: synchronise; may return the noise overlap share
        return None


class Placement(Condition):
    name = "placement"

    def __init__(self, shifts=SHIFTS, sync=None):
        self.shifts, self._sync = tuple(shifts), sync

    def stop(self):
        if self._sync is not None:
            self._sync()
        return None


@dataclass
class Failure:
    condition: str
    repeats: list               # [(repeat index, name -> Diff)] of the launches of that condition that differ

    def __str__(self):
        return "\n".join(f"condition {self.condition!r}, repeat {i}:\n{report(d)}" for i, d in self.repeats)


@dataclass
class Result:
    first: dict                                   # the judged snapshot
    failure: Optional[Failure] = None
    ran: list = field(default_factory=list)       # the conditions that were queued
    overlap: dict = field(default_factory=dict)   # condition -> share of the launches' wall time beside running noise
    launches: int = 0

    def check(self, what=""):
        assert self.failure is None, f"{what}: the launch is not bit-reproducible\n{self.failure}"
        return self


def run_repeats(make_inputs, launch, written, conditions, repeats=REPEATS, judge=None, allocated=None):
    """make_inputs(shift) -> a state: the inputs restored from the pristine copy and fresh 0xFF outputs, every buffer's base
    shifted by `shift` bytes; launch(state) queues the call and returns what it returns; written(state, ret) -> {name: tensor or
    Attn} of everything the call wrote; judge(state, ret) judges the values of the first launch (repeat 0).

    Then, per condition: all states are made, the launches are queued (repeats 1 .. n of that condition), the condition
    synchronises once, and every snapshot is compared with repeat 0's.  The first condition with a difference ends the run:
    Result.failure lists every differing repeat of it, and nothing further is queued.

    Once compared, what a repeat wrote is overwritten with 0xFF: the written tensors, and the tensors of allocated(state, ret)
    (default: none) -- what the op allocated and returned itself, where the written tensor is a copy of it (an un-blocked view).
    A result block that goes back to the allocator holds 0xFF then, not a right answer for a later launch that writes nothing."""
    state = make_inputs(0)
    ret = launch(state)
    first = snapshot(written(state, ret))
    if judge is not None:
        judge(state, ret)
    res = Result(first, launches=1)
    for cond in conditions:
        shifts = cond.shifts if cond.shifts is not None else (0,) * repeats
        states = [make_inputs(s) for s in shifts]
        cond.start()
        rets = []
        for i, st in enumerate(states):
            cond.before(i)
            rets.append(launch(st))
        share = cond.stop()
        res.ran.append(cond.name)
        res.launches += len(states)
        if share is not None:
            res.overlap[cond.name] = share
        bad = []
        for i, (st, r) in enumerate(zip(states, rets)):
            snap = snapshot(written(st, r))
            diffs = compare(first, snap)
            if any(diffs.values()):
                bad.append((i + 1, diffs))
            for s in snap.values():
                s.data.fill_(0xFF)
            for t in (allocated(st, r) if allocated is not None else ()):
                if t.numel() and t.dim() and t.stride(-1) == 1:
                    t.view(torch.uint8).fill_(0xFF)
        if bad:
            res.failure = Failure(cond.name, bad)
            break
    return res

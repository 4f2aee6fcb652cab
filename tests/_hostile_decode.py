"""Hostile memory around every operand of paged decode (a plain helper module, not a conftest).

mio_fa3_decode_paged, mio_fa3_decode_paged_window and mio_fa3_decode_paged_kv8 are launched through the C ABI on operands
that are views into larger buffers, at the same addresses, with the bytes the launch has no business with holding
  benign   finite values (16-bit: randn; e4m3fn: quantised randn; fp32 scales: finite; the workspace: 0xA5 in every byte,
           -2.9e-16 as fp32, what tests/test_gpu_decode_matrix.py used to leave there),
  nan      0xFF in every byte (a NaN in bf16, fp16, fp32 and e4m3fn alike),
  huge     finfo(dtype).max / 8 with random signs (e4m3fn: +-448, fp32: 1e30).
A masked key has weight 0 and 0 x finite = 0, so a kernel that lets a value it does not own into a product computes the
right numbers on `benign` and NaN on `nan`.  fmaxf drops a NaN operand, so a stale score that only enters a running
maximum is invisible to `nan`; a huge finite score raises the maximum and zeroes the row, which is what `huge` is for
(tests/_hostile.py says the same of prefill).  With an e4m3fn cache `huge` is bounded by the format: +-448 times the scale.

Integers are never out of range, in any fill.  A table entry the launch does not own names an in-range block whose bytes
follow the fill: entries past the last needed block, guard rows and (from one sequence's point of view) the other
sequences' rows name ONE hostile block under `nan` / `huge`; under `benign` the entries past the last needed block name
the sequence's own stale pages (finite data), as a serving engine leaves them.  Entries in front of a window keep naming
their pages, whose bytes follow the fill.  A not-owned entry of context_lengths holds a value in [0, max_ctx]: its owned
neighbour's under `benign` (a read of it is silently right), min(max_ctx, 2100) under `nan`, half of that + 1 under `huge`.

OWNERSHIP, from the contract in include/mio_hip.h and the docstrings of mio.ops (not from kernel code).
Owned inputs (their value may influence the result):
  * the D elements of each (b, h, qi) row of q, b < B;
  * context_lengths[0 .. B);
  * the K / V slots of the tested layer at positions lo_b <= j < Lk_b, Lk_b = min(ctx_b, max_blocks * block_size),
    lo_b = max(0, ctx_b - q_len - window_left) under a window ("the splits cover [max(0, ctx_b - q_len - window_left),
    ctx_b)", "only the window's keys are read"), else 0;
  * the table entries of the logical blocks that hold at least one such slot;
  * the tested layer's k_scale / v_scale.
Not owned, by class (CLASS_NAMES): bytes past D up to the row stride of q / o; guard heads, guard rows and guard batch
entries of q / o; the k / v thirds of a packed projection; stale slots at or past Lk_b; pre-window slots j < lo_b, the pages
holding only such slots and their table entries; spare pages, the other layers, guard blocks in front of and behind the
cache; table entries past the last needed block (and the hostile block they name) and guard rows of the table; guard
entries of context_lengths; the other layers' scales and guard scales; the whole workspace before the launch and the bytes
on either side of it; and the neighbours: another sequence's q rows, slots, table row and length as seen from sequence b,
another kv head's slots and q heads as seen from kv head g.
Owned outputs: the D elements of each (b, h, qi) row of o.  The workspace interior (mio_fa3_decode_workspace_bytes()) is
the launch's to write; nothing is said about what it holds afterwards.

judge(run, built): see its docstring.  Model is the torch model of the launch (per-split partial states into the
workspace, then the merge) that tests/test_hostile_decode_host.py proves the harness on, clean and with planted defects.

plan() mirrors the split geometry of csrc/decode_plan.h.  It decides nothing about ownership: the Model lays its
workspace out by it, the failure reports count differing workspace rows per (sequence, split) by it, and the case table's
"more than one split" is asserted through it (on the GPU the changed workspace interior proves it).  A window below q_len
spans fewer keys than the shortest split, so those cases have one split and leave the workspace alone; every other case
has at least two.

One run on the MI355X (tests/test_gpu_decode_hostile.py): 46 cases and 6 graph tests, 52 tests in 18.8 s of wall time, the
slowest 2.0 s.  Found: nothing; no kernel was changed.
"""
from __future__ import annotations

import ctypes as C
import math
import random
from dataclasses import dataclass
from typing import Dict, Tuple

import torch

import _decode_check as dc
from _hostile import FILLS, Buf, HostileFailure, bits

LAYER = dc.LAYER
GB = 1        # guard blocks on each side of a cache
GC = 4        # guard entries on each side of context_lengths
GS = 4        # guard scales on each side of k_scale / v_scale
Q_PAD = 8     # elements between D and the row stride of q
WS_BENIGN = 0xA5
CTX_POISON = 2100   # a not-owned context length under `nan` (max_ctx where that is smaller), past every allocated page

(OWNED, PAST_D, GUARD_HEAD, GUARD_ROW, GUARD_BATCH, PACKED, STALE, PRE_WINDOW, SPARE, OTHER_LAYER, GUARD_BLOCK, TABLE,
 GUARD_CTX, GUARD_SCALE, WORKSPACE, WS_GUARD, NEIGHBOUR, NEIGHBOUR_HEAD) = range(18)
CLASS_NAMES = {PAST_D: "past D", GUARD_HEAD: "guard head", GUARD_ROW: "guard row", GUARD_BATCH: "guard batch entry",
               PACKED: "k / v third of a packed projection", STALE: "stale slot", PRE_WINDOW: "pre-window",
               SPARE: "spare page", OTHER_LAYER: "other layer", GUARD_BLOCK: "guard block",
               TABLE: "table entry past the last needed block", GUARD_CTX: "guard entry of context_lengths",
               GUARD_SCALE: "guard scale", WORKSPACE: "workspace", WS_GUARD: "beside the workspace",
               NEIGHBOUR: "neighbour sequence", NEIGHBOUR_HEAD: "neighbour kv head"}


# ---- cases -------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    route: str                # head | rows | gqa: what the host-only route query must give
    kv8: bool
    dtype: torch.dtype        # the dtype the GPU test runs the case in (the host test runs both)
    B: int
    H: int
    Hkv: int
    D: int
    q_len: int
    bs: int
    left: int                 # window_left, -1: none
    msl: int
    ctxs: Tuple[int, ...]
    max_blocks: int
    q_packed: bool
    out_pad: int
    kind: str                 # none | inside | below | long | short | short_win | sparse | wide

    @property
    def span(self):
        """The keys a sequence's splits cover at most (include/mio_hip.h: sized from min(max_ctx, left + q_len))."""
        return self.left + self.q_len if 0 <= self.left and self.left + self.q_len < self.msl else self.msl

    @property
    def windowed(self):
        return self.left >= 0 and self.span < self.msl

    @property
    def cap(self):
        return self.max_blocks * self.bs

    def lk(self, ctx):
        return max(0, min(int(ctx), self.cap))

    def lo(self, ctx):
        return max(0, int(ctx) - self.q_len - self.left) if self.left >= 0 else 0


def plan(c: Case):
    """(nsplit, split_len) of a launch: the mirror of dec_plan in csrc/decode_plan.h (see the module docstring)."""
    span = c.span
    if c.route == "gqa":
        target = 256 if c.D * (1 if c.kv8 else 2) > 128 else 512
        units, cap, gran = c.B * c.Hkv, (span + 255) // 256, 128
    elif c.route == "rows":
        target, units, cap, gran = 512, c.B, (span + 63) // 64, 32
    else:
        target, units, cap, gran = 512, c.B * c.H * c.q_len, (span + 255) // 256, 32
    ns = max(1, min((target + units - 1) // units, max(cap, 1)))
    if c.route == "gqa":
        while ((span + ns - 1) // ns + 127) // c.bs + 2 > 2048:
            ns += 1
    sl = (span + ns - 1) // ns
    return ns, max(gran, (sl + gran - 1) // gran * gran)


_BS = [16, 64, 256, 1]
_LONG_LEFT, _INSIDE_LEFT = 1029, 301   # 301: no multiple of 32 or of a block size, a span of two or more splits


def _geom(route, kv8, want_rows, i):
    """A geometry of _decode_check._GEOMS (so the route is the table's): small caches, B >= 3, q_len > 1 when wanted."""
    ok = [g for g in dc._GEOMS[(route, kv8)] if g["B"] >= 3 and g["Hkv"] * g["D"] <= 512 and g["H"] <= 16
          and (not want_rows or g["q_len"] > 1)]
    return dict(ok[i % len(ok)])


def _contexts(route, bs, msl, B, short, rnd):
    ctxs, max_blocks = dc.edge_contexts(route, bs, msl, B, short, rnd)
    if msl not in ctxs:   # small batches start anywhere in the list of edges: the longest becomes max_seq_len
        ctxs[ctxs.index(max(ctxs))] = msl
    if 1 not in ctxs:   # every batch holds a 1-key sequence: its splits after the first are empty
        live = [i for i, n in enumerate(ctxs) if n > 0 and n != max(ctxs)]
        ctxs[min(live, key=lambda i: ctxs[i])] = 1
    return tuple(ctxs), max_blocks


def _table():
    cases = []
    n = 0
    for route in ("head", "rows", "gqa"):
        for kv8 in (False, True):
            rnd = random.Random(f"hostile{route}{kv8}")
            kinds = ["none", "inside", "below", "long", "short", "short_win", "sparse", "wide"]
            if route == "rows":   # one query row per sequence: no window below q_len
                kinds.remove("below")
            for k, kind in enumerate(kinds):
                geo = _geom(route, kv8, kind == "below", n)
                if kind.startswith("short"):
                    geo = next(dict(g) for g in dc._GEOMS[(route, kv8)] if g["B"] >= 10 and g["Hkv"] * g["D"] <= 512)
                out_pad = geo.pop("out_pad") or 8
                bs = _BS[n % 4]
                if kind in ("inside", "short_win") and bs == 1:   # every window is a multiple of block size 1
                    bs = 16
                msl, short = 1100, kind.startswith("short")
                left = {"inside": _INSIDE_LEFT, "short_win": _INSIDE_LEFT, "below": geo["q_len"] - 1, "long": _LONG_LEFT,
                        "wide": 1100 + geo["q_len"]}.get(kind, -1)
                if kind == "long":
                    msl = 2100
                if kind == "sparse":   # max_seq_len far above every context: most splits are empty
                    msl, bs = 32768, 16
                    ctxs = tuple([300, 0, 1, 33, 257, 129, 64, 299, 17, 250, 128, 100, 31, 200, 2, 290, 96, 77][:geo["B"]])
                    max_blocks = msl // bs
                else:
                    ctxs, max_blocks = _contexts(route, bs, msl, geo["B"], short, rnd)
                cases.append(Case(name=f"{route}-{'fp8' if kv8 else 'kv16'}-{kind}", route=route, kv8=kv8,
                                  dtype=(dc.BF, dc.FP)[(n + n // 8) % 2], bs=bs, left=left, msl=msl, ctxs=ctxs,
                                  max_blocks=max_blocks, q_packed=n % 3 == 0, out_pad=out_pad, kind=kind, **geo))
                n += 1
    assert len({c.name for c in cases}) == len(cases)
    return cases


CASES = _table()


# ---- buffers -----------------------------------------------------------------------------------------------------------
@dataclass
class Built:
    case: Case
    dtype: torch.dtype
    bufs: Dict[str, Buf]
    nsplit: int
    split_len: int
    ws_n: int                  # fp32 elements of mio_fa3_decode_workspace_bytes()
    ws_g: int                  # fp32 elements of each guard zone beside it
    hostile_block: int
    alloc: Tuple[int, ...]     # keys in the pages of each sequence: the contexts of the stale pre-launch
    seq_of_block: torch.Tensor  # [num_blocks] sequence whose pages these are, -1: nobody's
    ref: torch.Tensor
    ref_lse: torch.Tensor
    model_o: torch.Tensor
    persp: list                # [(name, {buf: bool map of owned elements that turn not-owned}, class, judged o map)]
    declared: set

    def q(self, t):
        c = self.case
        if c.q_packed:
            return t[1:1 + c.B, 1:1 + c.q_len, 0, 1:1 + c.H, :c.D].permute(0, 2, 1, 3)
        return t[1:1 + c.B, 1:1 + c.H, 1:1 + c.q_len, :c.D]

    def o(self, t):
        c = self.case
        return t[1:1 + c.B, 1:1 + c.H, 1:1 + c.q_len, :c.D]

    def cache(self, t):
        return t[GB:t.shape[0] - GB]

    def table(self, t):
        return t[1:1 + self.case.B]

    def ctx(self, t):
        return t[GC:GC + self.case.B]


def _embed_rows(c, dtype, gen, role, pad, packed=False):
    """q / o: [B+2, H+2, q_len+2, D+pad] (packed: the first third of [B+2, q_len+2, 3, H+2, D+pad]) with its class map."""
    B, H, S, D = c.B, c.H, c.q_len, c.D
    full = (B + 2, S + 2, 3, H + 2, D + pad) if packed else (B + 2, H + 2, S + 2, D + pad)
    ax = dict(b=0, s=1, h=3) if packed else dict(b=0, h=1, s=2)
    cls = torch.zeros(full, dtype=torch.uint8)
    cls[..., D:] = PAST_D
    for key, n, cl in (("s", S, GUARD_ROW), ("h", H, GUARD_HEAD), ("b", B, GUARD_BATCH)):   # later wins
        sl = [slice(None)] * len(full)
        sl[ax[key]] = slice(0, 1)
        cls[tuple(sl)] = cl
        sl[ax[key]] = slice(1 + n, None)
        cls[tuple(sl)] = cl
    if packed:
        cls[:, :, 1:] = PACKED
    if role == "in":
        data = (torch.randn(full, generator=gen) * 1.5).to(dtype)
    else:
        data = torch.full(full, -1, dtype=torch.int16).view(dtype)
    return Buf("q" if role == "in" else "o", role, "f16", data, cls)


def _benign_cache(t, scale, gen):
    """Whatever hostile_cache left NaN holds finite data."""
    if t.dtype == dc.F8:
        nan = t.view(torch.uint8) == dc.F8_NAN
        t.view(torch.uint8)[nan] = dc.quantise(torch.randn(t.shape, generator=gen), scale).view(torch.uint8)[nan]
    else:
        nan = torch.isnan(t)
        t[nan] = torch.randn(t.shape, generator=gen).to(t.dtype)[nan]


def workspace_bytes(c: Case):
    from mio import _lib
    return int(_lib.lib.mio_fa3_decode_workspace_bytes(c.B, c.H, c.q_len, c.D, c.msl))


def build(c: Case, dtype=None, seed=0) -> Built:
    dtype = dtype or c.dtype
    gen = torch.Generator().manual_seed(seed * 7919 + sum(ord(ch) for ch in c.name))
    B, H, Hkv, D, bs = c.B, c.H, c.Hkv, c.D, c.bs
    L = 3 if c.kv8 else 2
    ks, vs = dc.case_scales(dict(kv8=c.kv8, data="randn", D=D))
    bufs: Dict[str, Buf] = {}
    bufs["q"] = _embed_rows(c, dtype, gen, "in", Q_PAD, c.q_packed)
    bufs["o"] = _embed_rows(c, dtype, gen, "out", c.out_pad)

    # the pages of a sequence hold the keys of the stale pre-launch: the longest context for the 1-key sequence, 300 for
    # the empty one, a page and five keys more for the others
    longest = max(c.ctxs)
    alloc = tuple(min(c.msl, longest if n == 1 else 300 if n == 0 else n + bs + 5) for n in c.ctxs)
    kc, vc, bt, hostile = dc.hostile_cache(list(alloc), block_size=bs, Hkv=Hkv, D=D, L=L, layer=LAYER,
                                           cache_dtype=dc.F8 if c.kv8 else dtype, gen=gen, max_blocks=c.max_blocks,
                                           k_scale=ks[LAYER], v_scale=vs[LAYER])
    nb = kc.shape[0]
    ccls = torch.full((nb, L, bs, Hkv, 1), OTHER_LAYER, dtype=torch.uint8)
    ccls[:, LAYER] = SPARE
    ccls[hostile] = TABLE
    tcls = torch.full(bt.shape, TABLE, dtype=torch.uint8)
    seq_of_block = torch.full((nb,), -1, dtype=torch.int64)
    for b, n in enumerate(c.ctxs):
        pages = min((alloc[b] + bs - 1) // bs, c.max_blocks)
        mine = bt[b, :pages].long()
        seq_of_block[mine] = b
        slot = ccls[:, LAYER, :, :, 0]   # a view
        slot[mine] = STALE
        lo, lk = c.lo(n), c.lk(n)
        for cl, a, e in ((PRE_WINDOW, 0, min(lo, c.lk(alloc[b]))), (OWNED, lo, lk)):
            pos = torch.arange(a, max(a, e))
            slot[bt[b, pos // bs].long(), pos % bs] = cl
        for j in range(pages):
            if (j + 1) * bs <= lo:
                tcls[b, j] = PRE_WINDOW
            elif j * bs < lk and (j + 1) * bs > lo:
                tcls[b, j] = OWNED
    for t, s in ((kc, ks[LAYER]), (vc, vs[LAYER])):
        _benign_cache(t, s, gen)
    for name, t, s in (("k_cache", kc, ks[LAYER]), ("v_cache", vc, vs[LAYER])):
        guard = torch.randn((GB,) + tuple(t.shape[1:]), generator=gen)
        guard = dc.quantise(guard, s) if c.kv8 else guard.to(dtype)
        gcls = torch.full((GB,) + tuple(ccls.shape[1:]), GUARD_BLOCK, dtype=torch.uint8)
        data = torch.cat([bits(x) for x in (guard, t, guard)]).view(t.dtype)
        bufs[name] = Buf(name, "in", "f8" if c.kv8 else "f16", data, torch.cat([gcls, ccls, gcls]))
    grow = torch.full((1, c.max_blocks), hostile, dtype=torch.int32)
    bufs["table"] = Buf("table", "in", "table", torch.cat([grow, bt, grow]),
                        torch.cat([torch.full_like(grow, GUARD_ROW, dtype=torch.uint8), tcls,
                                   torch.full_like(grow, GUARD_ROW, dtype=torch.uint8)]))
    ctx = torch.tensor((c.ctxs[0],) * GC + c.ctxs + (c.ctxs[-1],) * GC, dtype=torch.int32)
    ccl = torch.full(ctx.shape, GUARD_CTX, dtype=torch.uint8)
    ccl[GC:GC + B] = OWNED
    bufs["ctx"] = Buf("ctx", "in", "ctx", ctx, ccl)
    if c.kv8:
        for name, vals in (("k_scale", ks), ("v_scale", vs)):
            s = torch.tensor([0.31, 2.3, 0.7, 1.9][:GS] + list(vals) + [0.45, 3.1, 0.6, 1.2][:GS], dtype=torch.float32)
            scl = torch.full(s.shape, GUARD_SCALE, dtype=torch.uint8)
            scl[GS:GS + L] = OTHER_LAYER
            scl[GS + LAYER] = OWNED
            bufs[name] = Buf(name, "in", "f32", s, scl)
    nbytes = workspace_bytes(c)
    assert nbytes % 4 == 0
    ws_n, ws_g = nbytes // 4, (nbytes + 255) // 256 * 64   # guards at least as large as the region: an overrun stays inside
    wcls = torch.full((2 * ws_g + ws_n,), WS_GUARD, dtype=torch.uint8)
    wcls[ws_g:ws_g + ws_n] = WORKSPACE
    bufs["ws"] = Buf("ws", "work", "f32", torch.full((4 * (2 * ws_g + ws_n),), WS_BENIGN, dtype=torch.uint8).view(torch.float32),
                     wcls)

    nsplit, split_len = plan(c)
    bt_ = Built(c, dtype, bufs, nsplit, split_len, ws_n, ws_g, hostile, alloc, seq_of_block, None, None, None, [], set())
    kw = dict(left=c.left, k_scale=ks[LAYER], v_scale=vs[LAYER])
    args = (bt_.q(bufs["q"].data), bt_.cache(bufs["k_cache"].data), bt_.cache(bufs["v_cache"].data),
            bt_.table(bufs["table"].data), bt_.ctx(bufs["ctx"].data), bs, LAYER)
    bt_.ref, bt_.ref_lse = dc.reference(*args, **kw)
    bt_.model_o = dc.model(*args, dtype=dtype, p16=c.route == "gqa", **kw)

    # the neighbour judgements: the empty sequence, the longest, the one at the end of a short table row (else the
    # shortest that is not empty), and one kv head
    picks = []
    if 0 in c.ctxs:
        picks.append(c.ctxs.index(0))
    picks.append(c.ctxs.index(longest))
    over = [b for b, n in enumerate(c.ctxs) if n >= c.cap]
    live = [b for b, n in enumerate(c.ctxs) if n > 0]
    picks.append(over[0] if c.cap < c.msl and over else min(live, key=lambda b: c.ctxs[b]))
    for b in dict.fromkeys(picks):
        extra = {}
        for name in ("q", "o"):
            m = torch.ones_like(bufs[name].cls, dtype=torch.bool)
            m[1 + b] = False
            extra[name] = m
        other = (seq_of_block != b) & (seq_of_block >= 0)
        m = torch.cat([torch.zeros(GB, dtype=torch.bool), other, torch.zeros(GB, dtype=torch.bool)])
        extra["k_cache"] = extra["v_cache"] = m.view(-1, 1, 1, 1, 1).expand_as(bufs["k_cache"].cls)
        for name in ("table", "ctx"):
            m = torch.ones_like(bufs[name].cls, dtype=torch.bool)
            m[(1 if name == "table" else GC) + b] = False
            extra[name] = m
        judged = (bufs["o"].cls == OWNED) & ~extra.pop("o")
        bt_.persp.append((f"sequence {b} (ctx {c.ctxs[b]})", extra, NEIGHBOUR, judged))
    if Hkv > 1:
        g, rep = len(c.name) % Hkv, H // Hkv
        heads = torch.zeros(H + 2, dtype=torch.bool)
        heads[1 + g * rep:1 + (g + 1) * rep] = True
        shape = [1] * bufs["q"].cls.dim()
        shape[3 if c.q_packed else 1] = H + 2
        extra = {"q": ~heads.view(shape).expand_as(bufs["q"].cls)}
        kvh = torch.ones(Hkv, dtype=torch.bool)
        kvh[g] = False
        extra["k_cache"] = extra["v_cache"] = kvh.view(1, 1, 1, Hkv, 1).expand_as(bufs["k_cache"].cls)
        judged = (bufs["o"].cls == OWNED) & heads.view(1, H + 2, 1, 1)
        bt_.persp.append((f"kv head {g}", extra, NEIGHBOUR_HEAD, judged))
    bt_.declared = {PAST_D, GUARD_HEAD, GUARD_ROW, GUARD_BATCH, STALE, SPARE, OTHER_LAYER, GUARD_BLOCK, TABLE, GUARD_CTX,
                    WORKSPACE, WS_GUARD, NEIGHBOUR}
    bt_.declared |= ({PACKED} if c.q_packed else set()) | ({PRE_WINDOW} if c.windowed else set())
    bt_.declared |= ({GUARD_SCALE} if c.kv8 else set()) | ({NEIGHBOUR_HEAD} if Hkv > 1 else set())
    return bt_


# ---- fills -------------------------------------------------------------------------------------------------------------
def eff_cls(built: Built, name, persp=None):
    cls = built.bufs[name].cls
    if persp is not None and name in persp[1]:
        cls = torch.where(persp[1][name] & (cls == OWNED), torch.tensor(persp[2], dtype=torch.uint8), cls)
    return cls


def _huge(bf, built):
    """The `huge` image of a buffer as bit patterns, the same in every launch: finfo.max / 8 with random signs, +-448 as
    e4m3fn bytes (0x7E / 0xFE), 1e30 in fp32."""
    if bf._sign is None:
        g = torch.Generator().manual_seed(bf.data.numel())
        neg = torch.randint(0, 2, bf.data.shape, generator=g, dtype=torch.int8)
        if bf.kind == "f32":
            img = torch.full(bf.data.shape, 1e30, dtype=torch.float32)
        elif bf.kind == "f8":
            img = (0x7E + 0x80 * neg).to(torch.uint8)
        else:
            img = ((1 - 2 * neg) * (torch.finfo(bf.data.dtype).max / 8)).to(bf.data.dtype)
        bf._sign = bits(img)
    return bf._sign


def inputs(built: Built, fill: str, persp=None, only=None) -> Dict[str, torch.Tensor]:
    """Every buffer of a launch (fresh tensors): inputs and the workspace with the not-owned elements holding `fill`
    (only: just these classes, the rest benign), o pre-filled with 0xFF bytes.  persp: one of built.persp, whose
    neighbours turn not-owned."""
    assert fill in FILLS
    c, out = built.case, {}
    for name, bf in built.bufs.items():
        d = bf.data.clone()
        if bf.role != "out" and fill != "benign":
            cls = eff_cls(built, name, persp)
            m = cls != OWNED
            if only is not None:
                m = m & torch.isin(cls, torch.tensor(sorted(only), dtype=torch.uint8))
            if bf.kind == "table":   # entries in front of a window keep naming their (poisoned) pages
                d[m & (cls != PRE_WINDOW)] = built.hostile_block
            elif bf.kind == "ctx":
                d[m] = min(c.msl, CTX_POISON) if fill == "nan" else min(c.msl, CTX_POISON) // 2 + 1
            else:
                b = bits(d)
                ones = torch.tensor(255 if b.dtype == torch.uint8 else -1, dtype=b.dtype)
                d = torch.where(m, ones if fill == "nan" else _huge(bf, built), b).view(d.dtype)
        out[name] = d
    return out


def stale_inputs(built: Built) -> Dict[str, torch.Tensor]:
    """The launch that ran before in the same workspace: the same plan, another q, every cached value negated, and each
    sequence's context the longer (or equal) one its pages were allocated for."""
    c, t = built.case, inputs(built, "benign")
    gen = torch.Generator().manual_seed(c.B * 131 + c.D)
    t["q"] = (torch.randn(t["q"].shape, generator=gen) * 1.5).to(built.dtype)
    for name in ("k_cache", "v_cache"):
        b = bits(t[name])   # the sign bit of every element
        b ^= 0x80 if b.dtype == torch.uint8 else -32768
    built.ctx(t["ctx"])[:] = torch.tensor(built.alloc, dtype=torch.int32)
    return t


# ---- the launch --------------------------------------------------------------------------------------------------------
def launch_args(built: Built, t):
    """(route query, its arguments, launch function, its arguments up to the stream) of the case's C-ABI launch on the
    buffers t ({name: tensor}, any device; the route query dereferences nothing): every operand is its embedded view."""
    from mio import _lib
    lib, c = _lib.lib, built.case
    q, o = built.q(t["q"]), built.o(t["o"])
    assert q.stride(-1) == 1 and o.stride(-1) == 1 and q.data_ptr() % 16 == 0
    qs, os_ = (C.c_int64 * 3)(*q.stride()[:3]), (C.c_int64 * 3)(*o.stride()[:3])
    ptr = [q.data_ptr(), o.data_ptr(), built.cache(t["k_cache"]).data_ptr(), built.cache(t["v_cache"]).data_ptr()]
    if c.kv8:
        ptr += [t["k_scale"].data_ptr() + 4 * (GS + LAYER), t["v_scale"].data_ptr() + 4 * (GS + LAYER)]
    ptr += [built.table(t["table"]).data_ptr(), built.ctx(t["ctx"]).data_ptr()]
    dt = 0 if built.dtype == torch.bfloat16 else 1
    args = (*ptr, qs, os_, c.B, c.H, c.Hkv, c.q_len, c.D, 3 if c.kv8 else 2, LAYER, c.bs, c.max_blocks, c.msl,
            1.0 / math.sqrt(c.D))
    ws = t["ws"].data_ptr() + 4 * built.ws_g
    assert ws % 16 == 0
    if c.kv8:
        return lib.mio_fa3_decode_kv8_route, (*args, c.left, dt, None, None), lib.mio_fa3_decode_paged_kv8, \
            (*args, c.left, dt, ws)
    rq = (lib.mio_fa3_decode_window_route, (*args, c.left, -1, dt, None, None))
    if c.left >= 0:
        return (*rq, lib.mio_fa3_decode_paged_window, (*args, c.left, -1, dt, ws))
    return (*rq, lib.mio_fa3_decode_paged, (*args, dt, ws))


def route(built: Built, t) -> str:
    from mio import _lib
    query, qargs, _fn, _args = launch_args(built, t)
    r = query(*qargs)
    assert r >= 0, (built.case.name, _lib.lib.mio_last_error().decode())
    return _lib.DECODE_ROUTES[r]


# ---- the judgement -----------------------------------------------------------------------------------------------------
def _first(mask):
    return tuple(int(x) for x in torch.nonzero(mask)[0])


def locate(built: Built, name: str, idx) -> str:
    """A buffer element in the operand's own coordinates, guards included (for messages)."""
    c = built.case
    if name in ("q", "o"):
        if name == "q" and c.q_packed:
            return f"sequence {idx[0] - 1}, row {idx[1] - 1}, third {idx[2]}, head {idx[3] - 1}, column {idx[4]}"
        return f"sequence {idx[0] - 1}, head {idx[1] - 1}, row {idx[2] - 1}, column {idx[3]}"
    if name in ("k_cache", "v_cache"):
        blk = idx[0] - GB
        seq = int(built.seq_of_block[blk]) if 0 <= blk < built.seq_of_block.numel() else -1
        return f"block {blk} (sequence {seq}), layer {idx[1]}, slot {idx[2]}, kv head {idx[3]}, column {idx[4]}"
    if name == "table":
        return f"row {idx[0] - 1}, entry {idx[1]}"
    if name == "ctx":
        return f"entry {idx[0] - GC}"
    if name == "ws":
        return f"fp32 element {idx[0] - built.ws_g} of {built.ws_n}"
    return f"element {idx[0] - GS - LAYER} from the tested layer's"


def split_counts(built: Built, base, after) -> str:
    """Rows of o that differ per sequence, and rows of the workspace (partial or lse) that differ per (sequence, split)."""
    c, ns = built.case, built.nsplit
    R = c.H * c.q_len
    rows = (bits(built.o(after["o"])) != bits(built.o(base["o"]))).any(-1).reshape(c.B, R).sum(1)
    msg = "rows of o differing per sequence " + str({b: int(n) for b, n in enumerate(rows) if n})
    if ns > 1:
        g, n = built.ws_g, c.B * R * ns
        x, y = bits(after["ws"])[g:g + built.ws_n], bits(base["ws"])[g:g + built.ws_n]
        d = (x[:n * c.D] != y[:n * c.D]).view(n, c.D).any(-1) | (x[n * c.D:n * c.D + n] != y[n * c.D:n * c.D + n])
        d = d.view(c.B, R, ns).sum(1)
        per = {b: {s: int(d[b, s]) for s in range(ns) if d[b, s]} for b in range(c.B) if d[b].any()}
        msg += f"; workspace rows differing per sequence and split (of {ns} x {built.split_len} keys) {per}"
    return msg


def _launch(run, built, given, fill, what):
    """One launch; then: every input equals its snapshot byte for byte, every not-owned byte of o and of the buffer
    around the workspace holds its pre-fill."""
    snap = {k: v.clone() for k, v in given.items()}
    after = run(built, given)
    for name, bf in built.bufs.items():
        changed = bits(after[name]) != bits(snap[name])
        if bf.role == "out":
            changed = changed & (bf.cls != OWNED)
        elif bf.role == "work":
            changed = changed & (bf.cls != WORKSPACE)
        if changed.any():
            idx = _first(changed)
            cl = CLASS_NAMES.get(int(bf.cls.expand_as(changed)[idx]), "owned")
            verb = "input modified" if bf.role == "in" else "not-owned bytes written"
            raise HostileFailure(f"{built.case.name} [{built.case.route}] {what} fill {fill}: {verb}: {name} at "
                                 f"{locate(built, name, idx)} [{cl}], {int(changed.sum())} elements", fill, name, [cl])
    return after


def _compare(run, built, base, after, given_fn, fill, what, judged, persp=None):
    d = (bits(after["o"]) != bits(base["o"])) & judged
    if not d.any():
        return
    guilty = []
    if given_fn is not None:   # one relaunch per class with only that class poisoned
        present = set()
        for n, bf in built.bufs.items():
            if bf.role != "out":
                present |= set(torch.unique(eff_cls(built, n, persp)).tolist())
        for cl in sorted(present - {OWNED}):
            one = run(built, given_fn(only={cl}))
            if ((bits(one["o"]) != bits(base["o"])) & judged).any():
                guilty.append(CLASS_NAMES[cl])
    c = built.case
    raise HostileFailure(
        f"{c.name} [{c.route}, {'fp8' if c.kv8 else 'kv16'}, left {c.left}] {what} fill {fill}: o differs from the "
        f"benign launch in {int(d.sum())} elements, first at {locate(built, 'o', _first(d))}; not-owned memory that "
        f"reaches the result: {guilty or 'no single class'}; {split_counts(built, base, after)}", fill, "o", guilty)


def nonvacuous(built: Built):
    """The conditions under which a pass means something; none is a measurement."""
    c = built.case
    seen = set()
    for p in [None] + built.persp:
        for name, bf in built.bufs.items():
            if bf.role != "out":
                seen |= set(torch.unique(eff_cls(built, name, p)).tolist())
    seen |= set(torch.unique(built.bufs["o"].cls).tolist())
    missing = [CLASS_NAMES[x] for x in built.declared if x not in seen]
    assert not missing, f"{c.name}: declared classes of not-owned memory are empty: {missing}"
    assert 1 in c.ctxs and (c.B < 3 or c.ctxs.count(0) == 1), f"{c.name}: needs a 1-key and an empty sequence"
    assert built.nsplit > 1 or c.kind == "below", f"{c.name}: a single split"
    tcls = built.table(built.bufs["table"].cls)
    if c.windowed:   # whole pages in front of a window, behind live table entries, next to owned pages
        assert (tcls == PRE_WINDOW).any() and (built.bufs["k_cache"].cls == PRE_WINDOW).any(), \
            f"{c.name}: no page lies in front of a window"
    else:
        assert PRE_WINDOW not in seen, f"{c.name}: has pre-window slots it does not declare"
    given = inputs(built, "nan")
    padded = (tcls == TABLE).any(1)
    assert padded.any() and ((built.table(given["table"]) == built.hostile_block) & (tcls == TABLE)).any(1)[padded].all(), \
        f"{c.name}: a padded table row does not name the hostile block"
    for t in given.values():   # every integer in range
        if t.dtype == torch.int32:
            hi = built.seq_of_block.numel() if t.dim() == 2 else c.msl + 1
            assert int(t.min()) >= 0 and int(t.max()) < hi, c.name
    for p in [None] + built.persp:   # every not-owned element is poisoned, every owned one is not
        given = inputs(built, "nan", p)
        for name, bf in built.bufs.items():
            if bf.kind in ("f16", "f8", "f32") and bf.role != "out":
                m = eff_cls(built, name, p) != OWNED
                got, ones = bits(given[name]), (-1 if bf.data.element_size() > 1 else 255)
                assert ((got == ones) | ~m).all() and ((got == bits(bf.data)) | m).all(), (c.name, name)
    union = torch.zeros_like(built.bufs["o"].cls, dtype=torch.bool)
    for _n, _e, cl, judged in built.persp:
        if cl == NEIGHBOUR:
            union |= judged
    assert union.any() and not (union & (built.bufs["o"].cls != OWNED)).any()


def judge(run, built: Built, fills=("nan", "huge"), parts=("fills", "stale", "neighbours", "reference")):
    """run(built, bufs) -> bufs after the launch ({name: CPU tensor}, every buffer of built.bufs, the workspace as the
    launch found and left it).  All launches of a judgement run at the same addresses.

    0. `benign` launch: the base.
    1. fills: each of `fills` with everything not owned poisoned, the workspace included: every owned byte of o equals the
       base's; after the `nan` launch the workspace interior has changed where the plan has more than one split.
    2. stale: stale_inputs() is launched, then the case's own benign launch into the workspace that left: o equals the base's.
    3. neighbours: per perspective of built.persp (three sequences, one kv head), each of `fills` with the neighbours'
       memory poisoned as well: the perspective's rows of o equal the base's.
    4. reference: the base is held to the unchanged _decode_check.check() bars against the fp64 reference and the fp32
       model of the owned data (last, so that a defect the poison shows is reported with its fill and class).
    After every launch: inputs equal their snapshots, not-owned bytes of o and the bytes either side of the workspace hold
    their fill.  tests/test_gpu_repeatable.py holds reruns of these routes bit-identical, so a difference is the poison's
    doing.  Raises HostileFailure (an AssertionError) naming fill, tensor, classes, route and the differing rows."""
    nonvacuous(built)
    c = built.case
    owned_o = built.bufs["o"].cls == OWNED
    base = _launch(run, built, inputs(built, "benign"), "benign", "")
    if "fills" in parts:
        for fill in fills:
            given = inputs(built, fill)
            g = built.ws_g
            before = bits(given["ws"])[g:g + built.ws_n].clone()   # a run may work in the given tensors
            after = _launch(run, built, given, fill, "")
            if fill == "nan" and built.nsplit > 1 and torch.equal(bits(after["ws"])[g:g + built.ws_n], before):
                raise HostileFailure(f"{c.name} [{c.route}]: the launch left the workspace untouched: a single split",
                                     fill, "ws", [CLASS_NAMES[WORKSPACE]])
            _compare(run, built, base, after, lambda only: inputs(built, fill, only=only), fill, "", owned_o)
    if "stale" in parts:
        before = _launch(run, built, stale_inputs(built), "stale", "pre-launch")
        given = inputs(built, "benign")
        given["ws"] = before["ws"].clone()
        after = _launch(run, built, given, "stale", "")
        _compare(run, built, base, after, None, "stale", "after a launch with longer contexts in the same workspace,",
                 owned_o)
    if "neighbours" in parts:
        for p in built.persp:
            for fill in fills:
                after = _launch(run, built, inputs(built, fill, p), fill, f"[{p[0]}]")
                _compare(run, built, base, after, lambda only: inputs(built, fill, p, only=only), fill, f"[{p[0]}]", p[3], p)
    if "reference" in parts:
        try:
            dc.check(built.o(base["o"]), built.ref, built.ref_lse, built.dtype, (built.dtype, c.route, "fp8" if c.kv8 else "kv16"),
                     built.model_o, c.name, win=c.windowed)
        except HostileFailure:
            raise
        except AssertionError as e:
            raise HostileFailure(f"{c.name} [{c.route}] fill benign: {e}", "benign", "o") from e
    return base


# ---- the CPU model of the launch ---------------------------------------------------------------------------------------
DEFECTS = ("slot_at_lk", "max_before_mask", "table_past_need", "page_early", "key_early", "q_past_d", "q_next_head",
           "scale_next_layer", "ctx_next", "empty_no_lse", "merge_extra_split", "o_past_d", "partial_past_ws",
           "table_next_row")


class Model:
    """A torch model of mio_fa3_decode_paged(_window / _kv8) that reads its operands through the embedded views, in fp64:
    per (sequence, split of plan()) a partial state (o, lse) of the keys lo_b <= j < Lk_b, stored as fp32 into the
    workspace ([rows, nsplit, D] then [rows, nsplit]), then the merge of every row's splits read back from there; with one
    split o is written directly.  defect: one of DEFECTS, a planted out-of-ownership access."""

    def __init__(self, defect=None):
        assert defect is None or defect in DEFECTS
        self.defect = defect

    def __call__(self, built: Built, bufs):
        c, d = built.case, self.defect
        B, H, Hkv, D, S, bs, ns, sl = c.B, c.H, c.Hkv, c.D, c.q_len, c.bs, built.nsplit, built.split_len
        R, rep, scale = H * S, H // Hkv, 1.0 / math.sqrt(D)
        kc, vc = built.cache(bufs["k_cache"]), built.cache(bufs["v_cache"])
        ks = vs = 1.0
        if c.kv8:
            at = GS + LAYER + (1 if d == "scale_next_layer" else 0)
            ks, vs = float(bufs["k_scale"][at]), float(bufs["v_scale"][at])
        g = built.ws_g
        ws = bufs["ws"]
        wo = ws[g:g + B * R * ns * D].view(B * R, ns, D)
        wl = ws[g + B * R * ns * D:g + B * R * ns * (D + 1)].view(B * R, ns)
        neg = torch.tensor(float("-inf"), dtype=torch.float64)

        def rows(name, row, p):
            t = (kc if name == "k" else vc)[row[p // bs].long(), LAYER, p % bs]
            t = t.float() if c.kv8 else t
            return t.double().repeat_interleave(rep, 1) * (ks if name == "k" else vs)   # [n, H, D]

        direct = {}
        for b in range(B):
            cb = int(bufs["ctx"][GC + b + (1 if d == "ctx_next" and b == B - 1 else 0)])
            lk, lo = c.lk(cb), (max(0, cb - S - c.left) if c.left >= 0 else 0)
            row = bufs["table"][1 + b]
            first = max(0, lo - 1) if d == "key_early" else lo
            pos = torch.arange(first, max(first, lk))
            sel = torch.zeros(pos.shape, dtype=torch.bool)
            if d == "table_next_row" and b < B - 1 and pos.numel() and \
                    c.lk(int(bufs["ctx"][GC + b + 1])) >= lk:   # where the next sequence owns those slots
                sel = pos // bs == (lk - 1) // bs
            qb = bufs["q"][1 + b]
            heads = torch.arange(1, 1 + H)
            if d == "q_next_head":
                heads[-1] += 1
            q = (qb[1:1 + S, 0][:, heads].permute(1, 0, 2) if c.q_packed else qb[heads, 1:1 + S]).double()   # [H, S, D + pad]
            s = torch.zeros(H, S, 0, dtype=torch.float64)
            if pos.numel():
                K, V = rows("k", row, pos), rows("v", row, pos)
                if sel.any():
                    K[sel], V[sel] = rows("k", bufs["table"][2 + b], pos[sel]), rows("v", bufs["table"][2 + b], pos[sel])
                s = torch.einsum("hqd,nhd->hqn", q[..., :D], K) * scale
                if d == "q_past_d":
                    s = s + (q[..., D:] * 0).sum(-1, keepdim=True)
                if c.left >= 0:
                    qlo = cb - S + torch.arange(S).view(S, 1) - c.left - (1 if d == "key_early" else 0)
                    s = s.masked_fill((pos.view(1, -1) < qlo)[None], float("-inf"))
            # a slot read at weight 0: 0 x its V row reaches the output
            zero = []
            if d == "slot_at_lk" and lk < c.cap and lk == cb:
                zero.append(lk)
            if d == "table_past_need" and (lk + bs - 1) // bs < c.max_blocks:
                zero.append((lk + bs - 1) // bs * bs)
            if d == "page_early" and c.left >= 0 and lo // bs >= 1:
                zero.append((lo // bs - 1) * bs)
            leak = (rows("v", row, torch.tensor(zero)) * 0).sum(0)[:, None] if zero else 0.0   # [H, 1, D]
            split = ((pos - lo).clamp_min(0) // sl).clamp_max(ns - 1)
            last = int(split.max()) if pos.numel() else -1
            r0 = slice(b * R, (b + 1) * R)
            live = sorted(set(split.tolist()))
            if ns == 1:
                direct[b] = torch.zeros(H, S, D, dtype=torch.float64)
            else:   # an empty split stores o = 0, lse = -inf
                wo[r0] = 0.0
                if d == "empty_no_lse":
                    wl[r0, :(live[-1] + 1 if live else 0)] = float("-inf")   # the splits past the last key store none
                else:
                    wl[r0] = float("-inf")
            for sp in live:
                idx = split == sp
                ss = s[..., idx]
                m = ss.amax(-1)
                if d == "max_before_mask" and sp == last and lk < c.cap and lk == cb:   # the stale score joins the maximum
                    sx = torch.einsum("hqd,nhd->hqn", q[..., :D], rows("k", row, torch.tensor([lk])))[..., 0] * scale
                    m = torch.fmax(m, sx)
                dead = torch.isinf(m) & (m < 0)
                p = torch.exp(ss - torch.where(dead, torch.zeros_like(m), m)[..., None])
                p = torch.where(dead[..., None], torch.zeros_like(p), p)
                l = p.sum(-1)
                o_s = torch.einsum("hqn,nhd->hqd", p / torch.where(l > 0, l, torch.ones_like(l))[..., None], V[idx]) + leak
                lse = torch.where(l > 0, m + torch.log(torch.where(l > 0, l, torch.ones_like(l))), neg)
                if ns == 1:
                    direct[b] = o_s
                else:
                    wo[r0, sp] = o_s.reshape(R, D).float()
                    wl[r0, sp] = lse.reshape(R).float()
        if d == "partial_past_ws":
            ws[g + built.ws_n:g + built.ws_n + D] = 0.0
        ob = bufs["o"]
        for b in range(B):
            if ns == 1:
                o = direct[b]
            else:   # the merge, from what the workspace holds
                n_in = ns + (1 if d == "merge_extra_split" else 0)
                at = (torch.arange(b * R, (b + 1) * R).view(R, 1) * ns + torch.arange(n_in).view(1, -1))
                flat = ws[g:g + built.ws_n]
                L_ = flat[B * R * ns * D + at].double()                                        # [R, n_in]
                O_ = flat[(at * D)[..., None] + torch.arange(D)].double()                      # [R, n_in, D]
                M = torch.where(torch.isnan(L_), neg, L_).amax(-1, keepdim=True)               # fmaxf drops a NaN
                w = torch.exp(L_ - torch.where(torch.isinf(M) & (M < 0), torch.zeros_like(M), M))
                w = torch.where(torch.isinf(M) & (M < 0), torch.zeros_like(w), w)
                W, acc = w.sum(-1, keepdim=True), (w[..., None] * O_).sum(1)
                o = torch.where(W > 0, acc / W, torch.zeros_like(acc)).view(H, S, D)          # NaN > 0 is false
            ob[1 + b, 1:1 + H, 1:1 + S, :D] = o.to(built.dtype)
            if d == "o_past_d":
                ob[1 + b, 1:1 + H, 1:1 + S, D:] = 0
        return bufs

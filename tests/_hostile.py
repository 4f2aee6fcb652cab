"""Hostile memory around every operand of the 16-bit attention prefill family (a plain helper module, not a conftest).

mio_fa3_fwd, mio_fa3_fwd_varlen, mio_fa3_fwd_paged and their _window forms are launched on operands that are views into
larger buffers, three times at the same addresses, with the bytes the launch has no business with holding
  benign   finite randn (what the other attention tests have there),
  nan      0xFF in every byte (a NaN in bf16 / fp16 / fp32, 255 in a keep mask),
  huge     finfo(dtype).max / 8 with random signs (1e30 in an additive mask, 1 in a keep mask).
A masked key has weight 0 and 0 x finite = 0, so a kernel that lets a value it does not own into a product -- a row past
Sk in the last tile, a chunk past D, a tile a windowed pass should not walk, the page behind a stale table entry --
computes the right numbers on `benign` and NaN on `nan`.  v_max drops a NaN operand, so a value that only enters a row
maximum is invisible to `nan`; a huge finite score raises the maximum and zeroes the row, which is what `huge` is for.

OWNERSHIP, from the contract in include/mio_hip.h and the docstrings of mio.ops (not from kernel code).  Owned inputs
(their value may influence the result):
  * the D elements of each (row, head) of q for rows inside a sequence;
  * the D elements of the k / v rows that are keys of a sequence, up to Lk_b (paged: min(seqused_k, max_seqlen_k,
    max_blocks_per_seq * block_size));
  * the mask elements of the broadcast [B,H,Sq,Sk]; the cu_seqlens / seqused_k entries; the carried o_acc / lse;
  * the block-table entries of logical blocks that hold at least one owned key.
Without a user mask (fwd1, fwd3, fwd5, the kpre forms, varlen, paged, windowed) a 64-key tile, aligned to key 0 of its
sequence, with no key visible to any query of that sequence is NOT owned ("excluded blocks are skipped", "only the pages
inside each query block's window are read"): its K / V rows, the pages holding only such tiles and their table entries.
Masked keys that share a tile with a visible key stay owned.  With a user mask (fwd1_keep, fwd1_add) every key < Sk is
owned: masked keys get a finite fill and a fully masked row averages all keys.
Everything else is not owned, by class (CLASS_NAMES): bytes past D up to the head stride, guard heads, guard rows (and
the rows of a packed buffer outside every sequence), guard batch entries, the other sequences of a packed buffer as
seen from one sequence, cache slots at or past Lk_b, spare pages, the other layers, invisible tiles, table entries past
the last needed block (and the page they name), guard columns of a mask, guard elements of the 1-D lse / o_acc.
Owned outputs (the launch must write them): o / lse / o_acc of rows inside a sequence.  Of the blocked output (o_blocked)
the padding rows past B*Sq of the last 256-row block are NOT written: every store of csrc/fa3_fwd5_body.inc is
predicated on the query row being < Sq, so they keep their pre-fill like any guard.

Packed varlen launches are judged once per sequence b: all rows of every other sequence are poisoned and b's output is
compared.  Not-owned table entries name hostile_cache's all-NaN block under `nan` / `huge` (an out-of-range entry is out
of scope here); that block's bytes follow the fill.

judge(run, built): see its docstring.  Model is the torch model of the four launch forms that tests/test_hostile_host.py
proves the harness on, clean and with planted defects.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, replace
from typing import Dict, List, Optional, Tuple

import torch

import _attn_check as ac
import _decode_check as dc

TILE = 64
LOG2E = 1.4426950408889634
G_ROWS = 3    # guard rows on each side of S
G_1D = 8      # guard elements on each side of a 1-D lse / o_acc / blocked-output buffer (keeps 16-byte alignment)
PAD_D = 8     # elements between D and the head stride
TRAIL = 5     # rows of a packed view past cu_seqlens[-1]
M_COL = 4     # guard columns on each side of a mask's Sk
CARRY_PREV = 70   # keys behind the carried state of a carry_in launch
LAYERS, LAYER = 3, 1

(OWNED, PAST_D, GUARD_HEAD, GUARD_ROW, GUARD_BATCH, NEIGHBOUR, STALE, SPARE, OTHER_LAYER, INVISIBLE, TABLE, GUARD_COL,
 GUARD_1D, PAD_ROW) = range(14)
CLASS_NAMES = {PAST_D: "past D", GUARD_HEAD: "guard head", GUARD_ROW: "guard row", GUARD_BATCH: "guard batch entry",
               NEIGHBOUR: "neighbour sequence", STALE: "stale slot", SPARE: "spare page", OTHER_LAYER: "other layer",
               INVISIBLE: "invisible tile", TABLE: "table entry past the last needed block", GUARD_COL: "guard column",
               GUARD_1D: "guard element", PAD_ROW: "padding row of the blocked output"}
FILLS = ("benign", "nan", "huge")


class HostileFailure(AssertionError):
    """A judgement failed: .fill, .tensor, .classes (names of the not-owned classes involved)."""

    def __init__(self, msg, fill, tensor, classes=()):
        super().__init__(msg)
        self.fill, self.tensor, self.classes = fill, tensor, tuple(classes)


# ---- geometry ----------------------------------------------------------------------------------------------------------
def visible(Lq, Lk, off, causal, window):
    """[Lq, Lk] bool: query i sees key j (include/mio_hip.h: off = q_offset - k_offset, or Lk - Lq for the packed forms)."""
    left, right = window
    if causal:
        right = 0
    i = torch.arange(Lq).view(-1, 1) + off
    j = torch.arange(Lk).view(1, -1)
    vis = torch.ones(Lq, Lk, dtype=torch.bool)
    if right >= 0:
        vis &= j <= i + right
    if left >= 0:
        vis &= j >= i - left
    return vis


def owned_tiles(Lq, Lk, off, causal, window, user_mask):
    """Per 64-key tile of a sequence: is it owned?  Closed form: the windows of consecutive rows overlap, so their union
    is the interval [off - left, Lq - 1 + off + right] cut to [0, Lk)."""
    n = (Lk + TILE - 1) // TILE
    if user_mask:
        return [True] * n
    if Lq == 0:
        return [False] * n
    left, right = window
    if causal:
        right = 0
    lo = 0 if left < 0 else max(0, off - left)
    hi = Lk - 1 if right < 0 else min(Lk - 1, Lq - 1 + off + right)
    return [lo <= hi and t * TILE <= hi and min(Lk, (t + 1) * TILE) - 1 >= lo for t in range(n)]


def blocked_index(M, HD):
    """[M, HD] int64: element offset of (m, c) in the blocked activation layout (include/mio_hip.h)."""
    m = torch.arange(M).view(-1, 1)
    c = torch.arange(HD).view(1, -1)
    return ((m // 256) * (HD // 32) + c // 32) * (256 * 32) + (m % 256) * 32 + c % 32


# ---- cases -------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    form: str                 # dense | varlen | paged
    route: str                # the name the route query must give (and the _attn_check family)
    D: int
    H: int = 4
    Hkv: int = 2
    causal: bool = False
    window: Tuple[int, int] = (-1, -1)
    # dense
    B: int = 2
    Sq: int = 300
    Sk: int = 333
    layout: str = "bshd"
    q_offset: int = 0
    k_offset: int = 0
    mask: Optional[str] = None     # keep | add
    mask_rows: bool = True         # [B,1,Sq,Sk], else [B,1,1,Sk]
    kpre: bool = False
    carry: Optional[int] = None    # None, or carry_in 0 / 1 with (o_acc, lse)
    oblk: bool = False
    # packed
    lens_q: Tuple[int, ...] = ()
    lens_k: Tuple[int, ...] = ()   # paged: seqused_k
    fused: bool = False
    # paged
    alloc: Tuple[int, ...] = ()    # keys in the pages of each sequence (>= what the launch may use)
    max_k: Optional[int] = None
    bs: int = 64
    shared: int = 0                # leading pages sequences 0 and 1 share
    invisible: Optional[bool] = None   # must the case have whole not-owned tiles? default: windowed / offset cases

    @property
    def windowed(self):
        return tuple(self.window) != (-1, -1)


def _dense(route, D, **kw):
    tag = [f"dense_{route}_D{D}"]
    tag += ["bhsd"] if kw.get("layout") == "bhsd" else []
    tag += ["causal"] if kw.get("causal") else []
    tag += [("rows" if kw.get("mask_rows", True) else "bcast")] if kw.get("mask") else []
    tag += [f"carry{kw['carry']}"] if kw.get("carry") is not None else []
    return Case(name=kw.pop("name", "_".join(tag)), form="dense", route=route, D=D, **kw)


def _table():
    cs: List[Case] = []
    # dense, one or more cases per route; fwd1 at Sq 100, the pipelined routes at Sq 300
    cs += [_dense("fwd1", 40, Sq=100), _dense("fwd1", 120, Sq=100, layout="bhsd", causal=True, q_offset=20, invisible=True),
           _dense("fwd1_keep", 64, Sq=100, mask="keep", causal=True),
           _dense("fwd1_keep", 88, Sq=100, mask="keep", mask_rows=False, layout="bhsd"),
           _dense("fwd1_add", 40, Sq=100, mask="add"),
           _dense("fwd1_add", 128, Sq=100, mask="add", mask_rows=False, causal=True),
           _dense("fwd5", 40, layout="bhsd", causal=True, q_offset=33), _dense("fwd5", 64),
           _dense("fwd5_kpre", 40, kpre=True), _dense("fwd5_kpre", 64, kpre=True, causal=True, q_offset=33, layout="bhsd"),
           _dense("fwd5_kpre_carry", 64, kpre=True, carry=0, causal=True, q_offset=33),
           _dense("fwd5_kpre_carry", 40, kpre=True, carry=1),
           _dense("fwd5_kpre_oblk", 40, kpre=True, oblk=True, causal=True, q_offset=33),
           _dense("fwd5_kpre_oblk", 64, kpre=True, oblk=True),
           _dense("fwd3", 88, causal=True, q_offset=33), _dense("fwd3", 96, layout="bhsd"),
           _dense("fwd3", 120), _dense("fwd3", 128, layout="bhsd", causal=True, q_offset=33),
           _dense("fwd3", 128, carry=0), _dense("fwd3", 96, carry=1),
           _dense("fwd3_kpre", 88, kpre=True), _dense("fwd3_kpre", 96, kpre=True, causal=True, q_offset=33, layout="bhsd")]
    # causal offsets: whole trailing key tiles invisible and leading rows that see nothing (a causal rule alone cannot hide
    # a leading tile: key 0 is the most visible one -- the windowed cases below do that); Lq > Lk rows that see nothing.
    # The last row inside Sq sees the last key of a tile (fwd1: Sq - 1 + 20 = 119, here 299 - 44 = 255, windowed below
    # 299 + 340 = 639): the rows past Sq of the last wave would see into the next tile, which no row inside Sq does
    for route, D in (("fwd5", 64), ("fwd3", 128)):
        cs += [_dense(route, D, Sk=500, causal=True, k_offset=44, invisible=True, name=f"dense_{route}_D{D}_trailing_tiles"),
               _dense(route, D, Sk=130, causal=True, k_offset=170, name=f"dense_{route}_D{D}_rows_see_nothing")]
    # packed varlen: a length-1 sequence between long ones, an empty one, one ending on a tile, one a row past a tile,
    # Lq > Lk and Lq < Lk
    lq, lk = (150, 1, 40, 65, 100, 300), (200, 1, 0, 65, 300, 64)
    for D in (64, 96, 128):
        for fused in (False, True):
            for causal in (False, True):
                cs.append(Case(name=f"varlen_D{D}_{'fused' if fused else 'split'}_c{int(causal)}", form="varlen",
                               route="fwd5" if D <= 64 else "fwd3", D=D, causal=causal, lens_q=lq, lens_k=lk, fused=fused))
    # paged: seqused_k shorter than the allocated pages, max_seqlen_k cutting the longest, Lk = 0, chunk over prefix,
    # Lq > Lk, sequences 0 and 1 sharing their first page
    for bs in (64, 128, 256):
        for D in (64, 128):
            for causal in (False, True):
                cs.append(Case(name=f"paged_bs{bs}_D{D}_c{int(causal)}", form="paged", route="fwd5" if D <= 64 else "fwd3",
                               D=D, causal=causal, lens_q=(100, 300, 40, 7, 80), lens_k=(333, 500, 0, 200, 30),
                               alloc=(333 + 2 * bs, 500, 70, 200 + bs, 64), max_k=450, bs=bs, shared=1))
    # windowed: queries late in a long key range (dense: in its middle, so right windows leave trailing tiles out too; the
    # packed forms are bottom-right aligned, their last query sees the last key and (-1, 100) leaves no tile out there)
    wins = [((0, 0), True), ((63, 0), True), ((64, 0), True), ((100, 0), True), ((64, 32), False), ((-1, 100), False)]
    for i, (w, causal) in enumerate(wins):
        for form in ("dense", "varlen", "paged"):
            D = (64, 128)[(i + (form == "varlen")) % 2]
            kw = dict(route="fwd5" if D <= 64 else "fwd3", D=D, causal=causal, window=w)
            name = f"window_{form}_l{w[0]}_r{w[1]}_D{D}"
            if form == "dense":
                cs.append(Case(name=name, form=form, Sq=300, Sk=800, q_offset=340 if causal else 300, **kw))
            elif form == "varlen":
                cs.append(Case(name=name, form=form, lens_q=(100, 300, 1), lens_k=(500, 420, 200), fused=bool(i % 2),
                               invisible=w[0] >= 0, **kw))
            else:
                cs.append(Case(name=name, form=form, lens_q=(100, 300, 1), lens_k=(500, 420, 200),
                               alloc=(500 + 64, 420, 200), bs=(64, 128, 256)[i % 3], invisible=w[0] >= 0, **kw))
    assert len({c.name for c in cs}) == len(cs)
    return cs


CASES = _table()


def shrunk(c: Case) -> Case:
    """The case at the sizes the CPU model is run at: fewer heads and batch entries, the same sequence geometry."""
    return replace(c, B=1) if c.oblk else replace(c, H=2, Hkv=1, B=1)   # a blocked output needs (H * D) % 32 == 0


# ---- buffers -----------------------------------------------------------------------------------------------------------
def _ff(shape, dtype):
    n = 1
    for s in shape:
        n *= s
    return torch.full((n * torch.empty((), dtype=dtype).element_size(),), 255, dtype=torch.uint8).view(dtype).view(shape)


def bits(t):
    """t as integers of its element size (for byte-for-byte comparison)."""
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


class Buf:
    """One backing buffer: .data (benign inputs / pre-filled outputs), .cls (class per element, OWNED = 0), .role in / out,
    .kind f16 | f32 | keep | add | table | int, .seq (packed: sequence of each element or -1), .spec (how to address rows)."""

    def __init__(self, name, role, kind, data, cls, spec=None):
        self.name, self.role, self.kind, self.data, self.cls, self.spec = name, role, kind, data, cls, spec
        self.seq = None
        self._sign = None

    def sign(self):
        if self._sign is None:
            g = torch.Generator().manual_seed(self.data.numel())
            self._sign = torch.randint(0, 2, self.data.shape, generator=g) * 2 - 1
        return self._sign


@dataclass
class Spec:
    """Where a logical tensor sits inside its buffer: layout bshd | bhsd | thd, offsets of batch / row / head, sizes."""
    buf: str
    layout: str
    b0: int
    r0: int
    h0: int
    B: int
    S: int
    h: int
    D: int

    def index(self):
        b, r, h, d = slice(self.b0, self.b0 + self.B), slice(self.r0, self.r0 + self.S), slice(self.h0, self.h0 + self.h), \
            slice(0, self.D)
        return {"bshd": (b, r, h, d), "bhsd": (b, h, r, d), "thd": (r, h, d)}[self.layout]

    def view(self, t):
        return t[self.index()]

    def rows(self, b, r0, r1, dw=None):
        """Index into the BUFFER of rows [r0, r1) of batch entry b, every head, dw (default D) columns; rows may lie in the
        guards.  The indexed tensor is [n, h, dw] for bshd / thd and [h, n, dw] for bhsd."""
        r, h, d = slice(self.r0 + r0, self.r0 + r1), slice(self.h0, self.h0 + self.h), slice(0, self.D if dw is None else dw)
        return {"bshd": (self.b0 + b, r, h, d), "bhsd": (self.b0 + b, h, r, d), "thd": (r, h, d)}[self.layout]

    def get(self, t, b, r0, r1, dw=None):
        x = t[self.rows(b, r0, r1, dw)]
        return x.permute(1, 0, 2) if self.layout == "bhsd" else x

    def put(self, t, b, r0, r1, val, dw=None):
        t[self.rows(b, r0, r1, dw)] = val.permute(1, 0, 2) if self.layout == "bhsd" else val


def _embed(name, role, layout, shape, dtype, gen, heads_before=1, heads_after=1, rows_after=G_ROWS):
    """A buffer around a logical [B,S,h,D] / [B,h,S,D] / [T,h,D] tensor: guard batch entries, guard rows, guard heads and
    a head stride of D + 8, with its class map and Spec."""
    if layout == "thd":
        (S, h, D), B = shape, 1
    elif layout == "bshd":
        B, S, h, D = shape
    else:
        B, h, S, D = shape
    ext = {"batch": (1, B, 1), "row": (G_ROWS, S, rows_after), "head": (heads_before, h, heads_after), "d": (0, D, PAD_D)}
    order = {"bshd": ("batch", "row", "head", "d"), "bhsd": ("batch", "head", "row", "d"), "thd": ("row", "head", "d")}[layout]
    full = tuple(sum(ext[k]) for k in order)
    cls = torch.zeros(full, dtype=torch.uint8)
    for kind, c in (("d", PAST_D), ("head", GUARD_HEAD), ("row", GUARD_ROW), ("batch", GUARD_BATCH)):  # later wins
        if kind not in order:
            continue
        ax = order.index(kind)
        a, n, _ = ext[kind]
        sl = [slice(None)] * len(full)
        sl[ax] = slice(0, a)
        cls[tuple(sl)] = c
        sl[ax] = slice(a + n, None)
        cls[tuple(sl)] = c
    data = torch.randn(full, generator=gen).to(dtype) if role == "in" else _ff(full, dtype)
    spec = Spec(name, layout, 1, G_ROWS, heads_before, B, S, h, D)
    return Buf(name, role, "f16", data, cls, spec), spec


def _guarded_1d(name, n, dtype, kind):
    data = _ff((G_1D + n + G_1D,), dtype)
    cls = torch.full((G_1D + n + G_1D,), GUARD_1D, dtype=torch.uint8)
    cls[G_1D:G_1D + n] = OWNED
    return Buf(name, "out", kind, data, cls)


def _ints(name, values):
    t = torch.tensor(list(values), dtype=torch.int32)
    return Buf(name, "in", "int", t, torch.zeros(t.shape, dtype=torch.uint8))


@dataclass
class Built:
    case: Case
    dtype: torch.dtype
    bufs: Dict[str, Buf]
    specs: Dict[str, Spec]      # q, k, v, o (not for a blocked output or a paged cache)
    seqs: List[Tuple[int, int, int]]   # (Lq, Lk, off) per sequence (dense: per batch entry)
    persp: list                 # [(name, {buf: bool map of extra not-owned}, {out buf: bool map of judged elements})]
    refs: list                  # [(what, b, ref_o [1|B,Lq,H,D], ref_lse)]
    meta: dict
    declared: set
    full_invisible_tiles: int = 0


def _window_reference(q, k, v, causal, window, off, scale):
    """The fp64 reference of tests/test_gpu_attention_window_prefill.py (keys outside the window absent), on the CPU."""
    B, Sq, H, D = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    qd = q.double().permute(0, 2, 1, 3)
    kd = k.double().repeat_interleave(H // Hkv, dim=2).permute(0, 2, 1, 3)
    vd = v.double().repeat_interleave(H // Hkv, dim=2).permute(0, 2, 1, 3)
    s = qd @ kd.transpose(-1, -2) * scale
    vis = visible(Sq, Sk, off, causal, window)
    s = s.masked_fill(~vis, float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - torch.where(torch.isfinite(lse), lse, torch.zeros_like(lse)).unsqueeze(-1))
    p = torch.where(vis.any(-1).view(1, 1, Sq, 1), p, torch.zeros_like(p))
    return (p @ vd).permute(0, 2, 1, 3), lse


def _reference(c, q, k, v, off, scale, keep=None, add=None):
    """q [B,Lq,H,D], k / v [B,Lk,Hkv,D] compact copies of the owned inputs -> the family's existing fp64 reference."""
    if c.windowed:
        return _window_reference(q, k, v, c.causal, c.window, off, scale)
    return ac.reference(q, k, v, causal=c.causal, softmax_scale=scale, keep_mask=keep, additive_mask=add, q_offset=off)


def _mark_tiles(built_tiles, cls_rows, base, Lk, tiles):
    """cls_rows: a [rows, ...] view of a class map whose row `base + j` is key j; not-owned tiles become INVISIBLE."""
    full = 0
    for t, own in enumerate(tiles):
        if not own:
            cls_rows[base + t * TILE:base + min(Lk, (t + 1) * TILE)] = INVISIBLE
            full += min(Lk, (t + 1) * TILE) - t * TILE == TILE
    return full


def build(c: Case, dtype, seed=0) -> Built:
    gen = torch.Generator().manual_seed(seed * 7919 + sum(ord(ch) for ch in c.name))
    b = {"dense": _build_dense, "varlen": _build_packed, "paged": _build_packed}[c.form](c, dtype, gen)
    want_invisible = c.invisible if c.invisible is not None else c.windowed
    if want_invisible:
        b.declared.add(INVISIBLE)
    b.meta["want_invisible"] = want_invisible
    return b


def _build_dense(c, dtype, gen):
    B, Sq, Sk, H, Hkv, D = c.B, c.Sq, c.Sk, c.H, c.Hkv, c.D
    shp = (lambda S, h: (B, S, h, D)) if c.layout == "bshd" else (lambda S, h: (B, h, S, D))
    bufs, specs = {}, {}
    for name, S, h in (("q", Sq, H), ("k", Sk, Hkv), ("v", Sk, Hkv)):
        bufs[name], specs[name] = _embed(name, "in", c.layout, shp(S, h), dtype, gen)
    scale = 1.0 / math.sqrt(D)
    ref_scale = scale
    if c.kpre:  # K as the projection epilogue hands it over; scores are then base 2
        bufs["k"].data = (bufs["k"].data.float() * (scale * LOG2E)).to(dtype)
        ref_scale = math.log(2.0)
    off = c.q_offset - c.k_offset
    tiles = owned_tiles(Sq, Sk, off, c.causal, c.window, c.mask is not None)
    full = 0
    for name in ("k", "v"):
        rows_first = specs[name].view(bufs[name].cls)
        rows_first = rows_first.permute(1, 0, 2, 3) if c.layout == "bshd" else rows_first.permute(2, 0, 1, 3)
        full = _mark_tiles(None, rows_first, 0, Sk, tiles)
    declared = {PAST_D, GUARD_HEAD, GUARD_ROW, GUARD_BATCH}
    keep = add = None
    if c.mask:
        Sm = Sq if c.mask_rows else 1
        fullm = (B + 2, 3, Sm + 2, Sk + 2 * M_COL)
        idx = (slice(1, 1 + B), slice(1, 2), slice(1, 1 + Sm), slice(M_COL, M_COL + Sk))
        cls = torch.full(fullm, GUARD_COL, dtype=torch.uint8)
        cls[:, :, :1], cls[:, :, 1 + Sm:] = GUARD_ROW, GUARD_ROW
        cls[:, :1], cls[:, 2:] = GUARD_HEAD, GUARD_HEAD
        cls[:1], cls[1 + B:] = GUARD_BATCH, GUARD_BATCH
        cls[idx] = OWNED
        if c.mask == "keep":
            data = (torch.rand(fullm, generator=gen) < 0.7).to(torch.uint8)
            keep = data[idx].clone()
        else:
            data = torch.randn(fullm, generator=gen) * 2.0
            data[torch.rand(fullm, generator=gen) < 0.2] = float("-inf")
            add = data[idx].clone()
        bufs["mask"] = Buf("mask", "in", c.mask, data, cls)
        bufs["mask"].spec = idx
        declared.add(GUARD_COL)

    if c.oblk:
        M = (B * Sq + 255) // 256 * 256
        ob = _guarded_1d("o", M * H * D, dtype, "f16")
        inner = ob.cls[G_1D:G_1D + M * H * D]
        inner[:] = PAD_ROW
        inner[blocked_index(B * Sq, H * D).reshape(-1)] = OWNED
        bufs["o"] = ob
    else:
        bufs["o"], specs["o"] = _embed("o", "out", c.layout, shp(Sq, H), dtype, gen)
        bufs["lse"] = _guarded_1d("lse", B * H * Sq, torch.float32, "f32")
    if c.carry is not None:
        bufs["o_acc"] = _guarded_1d("o_acc", B * Sq * H * D, torch.float32, "f32")

    q = specs["q"].view(bufs["q"].data)
    k, v = (torch.where(specs[n].view(bufs[n].cls) == OWNED, specs[n].view(bufs[n].data),
                        torch.zeros((), dtype=dtype)) for n in ("k", "v"))
    if c.layout == "bhsd":
        q, k, v = (t.permute(0, 2, 1, 3) for t in (q, k, v))
    if c.carry:  # the carried state: exact attention over CARRY_PREV keys in front of k, rounded to fp32
        assert not c.causal and not c.windowed
        kp = torch.randn(B, CARRY_PREV, Hkv, D, generator=gen)
        kp = (kp * (scale * LOG2E)).to(dtype) if c.kpre else kp.to(dtype)
        vp = torch.randn(B, CARRY_PREV, Hkv, D, generator=gen).to(dtype)
        o_p, lse_p = ac.reference(q, kp, vp, softmax_scale=ref_scale)
        bufs["o_acc"].data[G_1D:-G_1D] = o_p.float().reshape(-1)
        bufs["lse"].data[G_1D:-G_1D] = lse_p.float().reshape(-1)
        k, v = torch.cat([kp, k], 1), torch.cat([vp, v], 1)
    ref, rlse = _reference(c, q, k, v, off, ref_scale, keep, add)
    judged = {n: bufs[n].cls == OWNED for n in bufs if bufs[n].role == "out"}
    meta = dict(scale=scale, ref_scale=ref_scale, off=off)
    bt = Built(c, dtype, bufs, specs, [(Sq, Sk, off)] * B, [("all", {}, judged)], [("", None, ref, rlse)], meta, declared, full)
    return bt


def _cu(lens):
    out = [0]
    for n in lens:
        out.append(out[-1] + n)
    return out


def _build_packed(c, dtype, gen):
    paged = c.form == "paged"
    H, Hkv, D = c.H, c.Hkv, c.D
    nseq = len(c.lens_q)
    cu_q = _cu(c.lens_q)
    Tq = cu_q[-1]
    bufs, specs = {}, {}
    declared = {PAST_D, GUARD_HEAD, GUARD_ROW}
    if paged:
        bufs["q"], specs["q"] = _embed("q", "in", "thd", (Tq + TRAIL, H, D), dtype, gen)
    else:
        cu_k = _cu(c.lens_k)
        Tk = cu_k[-1]
        if c.fused:  # q / k / v heads side by side in the rows of one buffer, each group between guard heads
            Tm = max(Tq, Tk) + TRAIL
            fb, _ = _embed("qkv", "in", "thd", (Tm, H + 2 * Hkv + 4, D), dtype, gen)
            fb.cls[G_ROWS:G_ROWS + Tm, :, :D] = GUARD_HEAD
            for name, T, h0, h in (("q", Tq, 1, H), ("k", Tk, H + 3, Hkv), ("v", Tk, H + Hkv + 5, Hkv)):
                specs[name] = Spec("qkv", "thd", 0, G_ROWS, h0, 1, T + TRAIL, h, D)
                fb.cls[G_ROWS:G_ROWS + T + TRAIL, h0:h0 + h, :D] = OWNED
                fb.cls[G_ROWS + T + TRAIL:G_ROWS + Tm, h0:h0 + h, :D] = GUARD_ROW
            bufs["qkv"] = fb
        else:
            for name, T, h in (("q", Tq, H), ("k", Tk, Hkv), ("v", Tk, Hkv)):
                bufs[name], specs[name] = _embed(name, "in", "thd", (T + TRAIL, h, D), dtype, gen)
        bufs["cu_k"] = _ints("cu_k", cu_k)
        declared.add(NEIGHBOUR)
    bufs["cu_q"] = _ints("cu_q", cu_q)
    bufs["o"], specs["o"] = _embed("o", "out", "thd", (Tq + TRAIL, H, D), dtype, gen)
    total_q = Tq + TRAIL
    bufs["lse"] = _guarded_1d("lse", H * total_q, torch.float32, "f32")
    bufs["lse"].cls[G_1D:-G_1D].view(H, total_q)[:, Tq:] = GUARD_ROW

    def mark_seq(name, cu, trailing_from):
        s = specs[name]
        buf = bufs[s.buf]
        if buf.seq is None:
            buf.seq = torch.full(buf.data.shape, -1, dtype=torch.int16)
        s.view(buf.cls)[trailing_from:] = GUARD_ROW   # rows of the view outside every sequence
        for i in range(nseq):
            s.view(buf.seq)[cu[i]:cu[i + 1]] = i

    mark_seq("q", cu_q, Tq)
    mark_seq("o", cu_q, Tq)
    bufs["lse"].seq = torch.full(bufs["lse"].data.shape, -1, dtype=torch.int16)
    for i in range(nseq):
        bufs["lse"].seq[G_1D:-G_1D].view(H, total_q)[:, cu_q[i]:cu_q[i + 1]] = i

    scale = 1.0 / math.sqrt(D)
    meta = dict(scale=scale, ref_scale=scale, cu_q=cu_q, total_q=total_q, max_q=max(c.lens_q + (1,)))
    seqs, full = [], 0
    if not paged:
        mark_seq("k", cu_k, Tk)
        mark_seq("v", cu_k, Tk)
        for i in range(nseq):
            Lq, Lk = c.lens_q[i], c.lens_k[i]
            seqs.append((Lq, Lk, Lk - Lq))
            tiles = owned_tiles(Lq, Lk, Lk - Lq, c.causal, c.window, False)
            for name in ("k", "v"):
                f = _mark_tiles(None, specs[name].view(bufs[specs[name].buf].cls), cu_k[i], Lk, tiles)
            full += f
        meta.update(cu_k=cu_k, max_k=max(c.lens_k + (1,)))
    else:
        bs = c.bs
        kc, vc, bt, nan_block = dc.hostile_cache(list(c.alloc), block_size=bs, Hkv=Hkv, D=D, L=LAYERS, layer=LAYER,
                                                 cache_dtype=dtype, gen=gen)
        if c.shared:
            bt[1, :c.shared] = bt[0, :c.shared]
        for t in (kc, vc):  # benign: whatever hostile_cache left NaN holds finite data
            nan = torch.isnan(t)
            t[nan] = torch.randn(t.shape, generator=gen).to(dtype)[nan]
        nb, maxb = kc.shape[0], bt.shape[1]
        max_k = c.max_k if c.max_k is not None else max(c.lens_k + (1,))
        own = torch.zeros(nb, bs, dtype=torch.bool)
        other = torch.full((nb, bs), SPARE, dtype=torch.uint8)
        tcls = torch.full(bt.shape, TABLE, dtype=torch.uint8)
        for i in range(nseq):
            Lq, Lk = c.lens_q[i], min(c.lens_k[i], max_k, maxb * bs)
            assert Lk <= c.alloc[i], "a case must allocate the pages its launch may read"
            seqs.append((Lq, Lk, Lk - Lq))
            tiles = owned_tiles(Lq, Lk, Lk - Lq, c.causal, c.window, False)
            for j in range(min((c.alloc[i] + bs - 1) // bs, maxb)):   # the allocated pages: stale unless said otherwise
                other[int(bt[i, j])].clamp_(max=STALE)
            for t, o in enumerate(tiles):
                page, s0 = int(bt[i, t * TILE // bs]), t * TILE % bs
                n = min(Lk, (t + 1) * TILE) - t * TILE
                if o:
                    own[page, s0:s0 + n] = True
                    tcls[i, t * TILE // bs] = OWNED
                else:
                    other[page, s0:s0 + n] = INVISIBLE
                    full += n == TILE
        ccls = torch.full(kc.shape, OTHER_LAYER, dtype=torch.uint8)
        ccls[:, LAYER] = torch.where(own, torch.tensor(OWNED, dtype=torch.uint8), other)[:, :, None, None]
        ccls[nan_block] = TABLE
        bufs["k_cache"] = Buf("k_cache", "in", "f16", kc, ccls)
        bufs["v_cache"] = Buf("v_cache", "in", "f16", vc, ccls.clone())
        bufs["table"] = Buf("table", "in", "table", bt, tcls)
        bufs["seqused"] = _ints("seqused", c.lens_k)
        declared |= {STALE, SPARE, OTHER_LAYER, TABLE}
        meta.update(nan_block=nan_block, max_k=max_k, bs=bs)

    # references per sequence, from compact copies of the owned inputs
    refs = []
    qv = specs["q"].view(bufs[specs["q"].buf].data)
    for i, (Lq, Lk, off) in enumerate(seqs):
        if Lq == 0:
            continue
        qb = qv[cu_q[i]:cu_q[i] + Lq][None]
        if paged:
            pos = torch.arange(Lk)
            pages, slots = bufs["table"].data[i, pos // c.bs].long(), pos % c.bs
            kb, vb = (torch.where(bufs[n].cls[pages, LAYER, slots] == OWNED, bufs[n].data[pages, LAYER, slots],
                                  torch.zeros((), dtype=dtype))[None] for n in ("k_cache", "v_cache"))
        else:
            kb, vb = (torch.where(specs[n].view(bufs[specs[n].buf].cls)[cu_k[i]:cu_k[i] + Lk] == OWNED,
                                  specs[n].view(bufs[specs[n].buf].data)[cu_k[i]:cu_k[i] + Lk],
                                  torch.zeros((), dtype=dtype))[None] for n in ("k", "v"))
        ref, rlse = _reference(c, qb, kb, vb, off, scale)
        refs.append((f"seq {i} (Lq {Lq}, Lk {Lk})", i, ref, rlse))

    outs = ("o", "lse")
    if paged:
        persp = [("all", {}, {n: bufs[n].cls == OWNED for n in outs})]
    else:  # one judgement per sequence: every other sequence's rows are poisoned, this one's output is compared
        persp = []
        for i in range(nseq):
            if c.lens_q[i] == 0:
                continue
            extra = {}
            for name in {specs[n].buf for n in ("q", "k", "v")}:
                bf = bufs[name]
                extra[name] = (bf.seq >= 0) & (bf.seq != i) & (bf.cls == OWNED)
            persp.append((f"seq {i}", extra, {n: (bufs[n].cls == OWNED) & (bufs[n].seq == i) for n in outs}))
    return Built(c, dtype, bufs, specs, seqs, persp, refs, meta, declared, full)


# ---- fills -------------------------------------------------------------------------------------------------------------
def eff_cls(built, name, extra):
    cls = built.bufs[name].cls
    return torch.where(extra[name], torch.tensor(NEIGHBOUR, dtype=torch.uint8), cls) if name in extra else cls


def inputs(built: Built, fill: str, extra=None, only=None) -> Dict[str, torch.Tensor]:
    """Every buffer of a launch (fresh tensors): inputs with the not-owned elements holding `fill` (only: just these
    classes, the rest benign), outputs pre-filled with 0xFF bytes (and the carried state of a carry_in launch)."""
    extra = extra or {}
    out = {}
    for name, bf in built.bufs.items():
        d = bf.data.clone()
        if bf.role == "in" and fill != "benign" and bf.kind != "int":
            cls = eff_cls(built, name, extra)
            m = cls != OWNED
            if only is not None:
                m = m & torch.isin(cls, torch.tensor(sorted(only), dtype=torch.uint8))
            if bf.kind == "table":
                d[m] = built.meta["nan_block"]
            elif fill == "nan":
                bits(d)[m] = -1 if d.element_size() > 1 else 255
            elif bf.kind == "keep":
                d[m] = 1
            elif bf.kind == "add":
                d[m] = 1e30
            else:
                huge = torch.finfo(d.dtype).max / 8
                d[m] = (bf.sign()[m] * huge).to(d.dtype)
        out[name] = d
    return out


# ---- the judgement -----------------------------------------------------------------------------------------------------
def _first(mask):
    return tuple(int(x) for x in torch.nonzero(mask)[0])


def locate(built: Built, name: str, idx) -> str:
    """A buffer element as (sequence / batch entry, head, row) of the operand, guards included."""
    bf, c = built.bufs[name], built.case
    sp = bf.spec if isinstance(bf.spec, Spec) else None
    if sp is not None:
        if sp.layout == "thd":
            row, head = idx[0] - sp.r0, idx[1] - sp.h0
            seq = int(bf.seq[idx]) if bf.seq is not None else -1
            cu = built.meta.get("cu_q" if name in ("q", "o") else "cu_k", built.meta["cu_q"])
            rel = f", row {row - cu[seq]} of it" if seq >= 0 else ""
            return f"sequence {seq}{rel}, head {head}, packed row {row}, column {idx[2]}"
        b, r, h = (idx[0] - sp.b0, idx[1] - sp.r0, idx[2] - sp.h0) if sp.layout == "bshd" else \
            (idx[0] - sp.b0, idx[2] - sp.r0, idx[1] - sp.h0)
        return f"batch entry {b}, head {h}, row {r}, column {idx[3]}"
    if name in ("k_cache", "v_cache"):
        return f"page {idx[0]}, layer {idx[1]}, slot {idx[2]}, head {idx[3]}, column {idx[4]}"
    if name == "lse" and bf.cls.dim() == 1:
        e = idx[0] - G_1D
        if c.form == "dense":
            return f"batch entry {e // (c.H * c.Sq)}, head {e // c.Sq % c.H}, row {e % c.Sq}"
        tq = built.meta["total_q"]
        seq = int(bf.seq[idx]) if bf.seq is not None else -1
        return f"sequence {seq}, head {e // tq}, packed row {e % tq}"
    if name == "o_acc":
        e = idx[0] - G_1D
        return f"batch entry {e // (c.Sq * c.H * c.D)}, head {e // c.D % c.H}, row {e // (c.H * c.D) % c.Sq}"
    if name == "o" and c.oblk:
        e = idx[0] - G_1D
        HD = c.H * c.D
        blk, m, col = e // 8192, e % 8192 // 32, e % 32
        m, col = blk // (HD // 32) * 256 + m, blk % (HD // 32) * 32 + col
        return f"batch entry {m // c.Sq}, head {col // c.D}, row {m % c.Sq} (blocked row {m})"
    return f"element {idx}"


def _launch(run, built, given, fill, what):
    """One launch; then: every input equals its snapshot byte for byte, every not-owned output byte holds its pre-fill."""
    snap = {k: v.clone() for k, v in given.items()}
    after = run(built, given)
    for name, bf in built.bufs.items():
        changed = bits(after[name]) != bits(snap[name])
        if bf.role == "out":
            changed = changed & (bf.cls != OWNED)
        if changed.any():
            idx = _first(changed)
            cl = CLASS_NAMES.get(int(bf.cls[idx]), "owned")
            verb = "input modified" if bf.role == "in" else "not-owned output written"
            raise HostileFailure(f"{built.case.name} {what} fill {fill}: {verb}: {name} at {locate(built, name, idx)} "
                                 f"[{cl}], {int(changed.sum())} elements", fill, name, [cl])
    return after


def outputs(built: Built, after, b=None):
    """(o [B|1,Lq,H,D], lse or None, o_acc or None) of the whole dense launch or of packed sequence b."""
    c = built.case
    if c.form == "dense":
        if c.oblk:
            o = after["o"][G_1D:-G_1D][blocked_index(c.B * c.Sq, c.H * c.D)].view(c.B, c.Sq, c.H, c.D)
            return o, None, None
        o = built.specs["o"].view(after["o"])
        o = o.permute(0, 2, 1, 3) if c.layout == "bhsd" else o
        lse = after["lse"][G_1D:-G_1D].view(c.B, c.H, c.Sq)
        acc = after["o_acc"][G_1D:-G_1D].view(c.B, c.Sq, c.H, c.D) if c.carry is not None else None
        return o, lse, acc
    cu, Lq = built.meta["cu_q"][b], built.seqs[b][0]
    o = built.specs["o"].view(after["o"])[cu:cu + Lq][None]
    lse = after["lse"][G_1D:-G_1D].view(c.H, built.meta["total_q"])[:, cu:cu + Lq][None]
    return o, lse, None


def nonvacuous(built: Built):
    """The conditions under which a pass means something; none is a measurement."""
    c = built.case
    seen = set()
    for _pname, extra, _j in built.persp:
        for name, bf in built.bufs.items():
            if bf.role == "in":
                seen |= set(torch.unique(eff_cls(built, name, extra)).tolist())
    missing = [CLASS_NAMES[x] for x in built.declared if x not in seen]
    assert not missing, f"{c.name}: declared classes of not-owned input are empty: {missing}"
    if built.meta["want_invisible"]:
        assert built.full_invisible_tiles >= 1, f"{c.name}: no whole 64-key tile is poisoned"
    else:
        assert INVISIBLE not in seen, f"{c.name}: has not-owned tiles it does not declare"
    # a poisoned key row next to an owned one
    if c.form == "paged":
        own = (built.bufs["k_cache"].cls[:, LAYER] == OWNED).all(-1).all(-1)
    else:
        sp = built.specs["k"]
        own = (sp.view(built.bufs[sp.buf].cls) == OWNED).all(-1)
        own = own.all(1) if c.form == "dense" and c.layout == "bhsd" else own.all(-1)
        own = torch.cat([own, torch.zeros_like(own[..., :1])], -1)   # the row behind the view's last is a guard row
    assert (own[..., :-1] & ~own[..., 1:]).any(), f"{c.name}: no poisoned row is adjacent to an owned row"
    # every not-owned input element is poisoned, every owned output element is judged
    for _pname, extra, judged in built.persp:
        given = inputs(built, "nan", extra)
        for name, bf in built.bufs.items():
            if bf.role == "in" and bf.kind not in ("int", "table"):
                m = eff_cls(built, name, extra) != OWNED
                assert (bits(given[name])[m] == (-1 if given[name].element_size() > 1 else 255)).all(), (c.name, name)
                assert torch.equal(bits(given[name])[~m], bits(bf.data)[~m]), (c.name, name)
    for name, bf in built.bufs.items():
        if bf.role == "out":
            union = torch.zeros_like(bf.cls, dtype=torch.bool)
            for _p, _e, judged in built.persp:
                union |= judged[name]
            assert torch.equal(union, bf.cls == OWNED), f"{c.name}: owned elements of {name} are not judged"


def _check_reference(built, after):
    c, dtype = built.case, built.dtype
    for what, b, ref, rlse in built.refs:
        o, lse, acc = outputs(built, after, b)
        tag = f"{c.name} {what}".strip()
        ac.check(o, ref, dtype, c.route, lse, rlse, tag)
        if acc is not None:
            ac.check(acc, ref, dtype, c.route, None, rlse, tag + " (fp32 carry)")


def _diff(built, judged, base, after):
    for name, m in judged.items():
        d = (bits(after[name]) != bits(base[name])) & m
        if d.any():
            return name, _first(d), int(d.sum())
    return None


def judge(run, built: Built, fills=("nan", "huge")):
    """run(built, bufs) -> bufs after the launch ({name: CPU tensor}, every buffer of built.bufs).

    1. `benign` launch, outputs pre-filled with 0xFF: every owned output element finite (or 0 / -inf for rows with no
       visible key) and the result within the unchanged _attn_check bars of the case's route against the fp64 reference
       computed from compact copies of the owned inputs.
    2. each of `fills`, per perspective (packed varlen: per sequence): every judged output byte equals the benign
       launch's.  tests/test_gpu_repeatable.py holds reruns of these routes bit-identical, so a difference is the poison's
       doing; the report names the fill, the tensor, the first differing (sequence, head, row) and -- from one relaunch
       per class with only that class poisoned -- the classes of not-owned memory that reach the result.
    3. after every launch: not-owned output bytes hold their pre-fill, inputs equal their snapshots byte for byte.
    Raises HostileFailure (an AssertionError)."""
    nonvacuous(built)
    c = built.case
    base = _launch(run, built, inputs(built, "benign"), "benign", "")
    _check_reference(built, base)
    for pname, extra, judged in built.persp:
        for fill in fills:
            after = _launch(run, built, inputs(built, fill, extra), fill, pname)
            bad = _diff(built, judged, base, after)
            if bad is None:
                continue
            name, idx, count = bad
            present = set()
            for n, bf in built.bufs.items():
                if bf.role == "in" and bf.kind != "int":
                    present |= set(torch.unique(eff_cls(built, n, extra)).tolist())
            guilty = []
            for cl in sorted(present - {OWNED}):
                try:
                    one = run(built, inputs(built, fill, extra, only={cl}))
                except Exception:
                    continue
                if _diff(built, judged, base, one) is not None:
                    guilty.append(CLASS_NAMES[cl])
            raise HostileFailure(
                f"{c.name} [{pname}] fill {fill}: {name} differs from the benign launch in {count} elements, first at "
                f"{locate(built, name, idx)}; not-owned memory that reaches the result: {guilty or 'no single class'}",
                fill, name, guilty)
    return base


# ---- the CPU model of the four launch forms ----------------------------------------------------------------------------
DEFECTS = ("key_past_lk", "tile_into_next_seq", "chunk_past_d", "table_past_need", "other_layer", "window_tile_early",
           "max_only", "output_row_past", "output_past_d", "input_modified")


class Model:
    """A torch model of mio_fa3_fwd(_varlen / _paged)(_window) that reads its operands through the embedded views, in
    fp64, tile by tile: it touches the tiles with a visible key (every tile under a user mask) and, in the last one, the
    rows below Lk only.  defect: one of DEFECTS, a planted out-of-ownership access."""

    def __init__(self, defect=None):
        assert defect is None or defect in DEFECTS
        self.defect = defect

    def __call__(self, built: Built, bufs):
        c, d = built.case, self.defect
        sp = built.specs
        scale = built.meta["ref_scale"]
        H, Hkv, D = c.H, c.Hkv, c.D
        paged, dense = c.form == "paged", c.form == "dense"
        dw = D + PAD_D if d == "chunk_past_d" and not paged else D
        if dense:
            geo = [(b, c.Sq, c.Sk, c.q_offset - c.k_offset, 0, 0) for b in range(c.B)]
        else:
            cu_q = bufs["cu_q"].tolist()
            if paged:
                bt, bs = bufs["table"], c.bs
                lk = [min(int(n), built.meta["max_k"], bt.shape[1] * bs) for n in bufs["seqused"].tolist()]
                cu_k = [0] * (len(lk) + 1)
            else:
                cu_k = bufs["cu_k"].tolist()
                lk = [cu_k[i + 1] - cu_k[i] for i in range(len(cu_k) - 1)]
            geo = [(0, cu_q[i + 1] - cu_q[i], lk[i], lk[i] - (cu_q[i + 1] - cu_q[i]), cu_q[i], cu_k[i]) for i in range(len(lk))]
        tq = bufs[sp["q"].buf]
        for i, (b, Lq, Lk, off, q0, k0) in enumerate(geo):
            if Lq == 0:
                continue
            seq = i if not dense else b
            q = sp["q"].get(tq, b, q0, q0 + Lq, None).double()           # [Lq, H, D]
            if dw != D:
                q = torch.nn.functional.pad(q, (0, dw - D))
            vis = visible(Lq, Lk, off, c.causal, c.window)
            ntile = (Lk + TILE - 1) // TILE
            tiles = [t for t in range(ntile) if c.mask or vis[:, t * TILE:(t + 1) * TILE].any()]
            if d == "window_tile_early" and tiles and tiles[0] > 0:
                tiles = [tiles[0] - 1] + tiles
            pos = [torch.arange(t * TILE, min(Lk, (t + 1) * TILE)) for t in tiles]
            extra_max = None
            if tiles:
                last_end = min(Lk, (tiles[-1] + 1) * TILE)
                if d == "key_past_lk" and last_end == Lk:
                    pos.append(torch.tensor([Lk]))
                if d == "tile_into_next_seq" and last_end == Lk and Lk % TILE:
                    pos.append(torch.arange(Lk, (tiles[-1] + 1) * TILE))
                if d == "table_past_need" and paged and (Lk + bs - 1) // bs < bt.shape[1]:
                    pos.append(torch.tensor([(Lk + bs - 1) // bs * bs]))
            pos = torch.cat(pos) if pos else torch.zeros(0, dtype=torch.long)

            if not paged:   # the buffer ends somewhere: a planted over-read stops there
                sk = sp["k"]
                lim = bufs[sk.buf].shape[{"thd": 0, "bshd": 1, "bhsd": 2}[sk.layout]] - sk.r0 - k0
                pos = pos[pos < lim]

            def rows(name, p, layer=LAYER):
                if paged:
                    pages = bt[seq, p // bs].long()
                    return bufs[name + "_cache"][pages, layer, p % bs].double()
                s = sp[name]
                if p.numel() == 0:
                    return torch.zeros(0, s.h, dw, dtype=torch.float64)
                return self._gather(s, bufs[s.buf], b, k0, p, dw).double()

            K, V = rows("k", pos), rows("v", pos)
            if d == "other_layer" and paged and pos.numel():
                K = torch.cat([K, rows("k", pos[:1], LAYER + 1)])
                V = torch.cat([V, rows("v", pos[:1], LAYER + 1)])
                pos = torch.cat([pos, torch.tensor([1 << 20])])
            if d == "max_only" and tiles and min(Lk, (tiles[-1] + 1) * TILE) == Lk:
                kx = rows("k", torch.tensor([Lk]))
                if kx.shape[0]:
                    extra_max = torch.einsum("qhd,khd->hqk", q, kx.repeat_interleave(H // Hkv, 1)) * scale
            n = pos.numel()
            inside = pos < Lk
            visn = torch.zeros(Lq, n, dtype=torch.bool)
            visn[:, inside] = vis[:, pos[inside]]
            if n:
                Ke, Ve = K.repeat_interleave(H // Hkv, 1), V.repeat_interleave(H // Hkv, 1)
                if Ve.shape[-1] != D:
                    Ve = Ve[..., :D]
                s = torch.einsum("qhd,khd->hqk", q, Ke) * scale
                if c.mask:
                    s = s.masked_fill(~visn[None], -1e9)
                    m4 = bufs["mask"][built.bufs["mask"].spec][b, 0]                   # [Sq | 1, Sk]
                    mrow = m4.expand(Lq, Lk)[:, pos.clamp_max(Lk - 1)]
                    if c.mask == "keep":
                        s = torch.where(mrow[None] != 0, s, torch.full_like(s, -1e9))
                    else:
                        s = s + mrow[None].double().clamp_min(ac.ADD_MASK_FLOOR)
                    s = s.masked_fill(~inside[None, None], float("-inf"))
                else:
                    s = s.masked_fill(~visn[None], float("-inf"))
                m = s.amax(-1)
                if extra_max is not None:
                    m = torch.fmax(m, extra_max[..., 0])
                empty = torch.isinf(m) & (m < 0)
                p = torch.exp(s - torch.where(empty, torch.zeros_like(m), m)[..., None])
                p = torch.where(empty[..., None], torch.zeros_like(p), p)
                l = p.sum(-1)
                lse = torch.where(empty, m, m + torch.log(l))                              # [H, Lq]
                o = torch.einsum("hqk,khd->qhd", p / torch.where(empty | (l == 0), torch.ones_like(l), l)[..., None], Ve)
            else:
                lse = torch.full((H, Lq), float("-inf"), dtype=torch.float64)
                o = torch.zeros(Lq, H, D, dtype=torch.float64)
            if dense and c.carry:   # continue from the carried (o_acc, lse)
                lp = bufs["lse"][G_1D:-G_1D].view(c.B, H, Lq)[b].double()
                op = bufs["o_acc"][G_1D:-G_1D].view(c.B, Lq, H, D)[b].double()
                ln = torch.logaddexp(lp, lse)
                dead = torch.isinf(ln) & (ln < 0)
                wp = torch.where(dead, torch.zeros_like(ln), torch.exp(lp - torch.where(dead, torch.zeros_like(ln), ln)))
                wc = torch.where(dead, torch.zeros_like(ln), torch.exp(lse - torch.where(dead, torch.zeros_like(ln), ln)))
                o = wp.t()[..., None] * op + wc.t()[..., None] * o
                lse = ln
            # outputs
            ot = o.to(built.dtype)
            if dense and c.oblk:
                blk = blocked_index(c.B * c.Sq, H * D)[b * c.Sq:(b + 1) * c.Sq]
                bufs["o"][G_1D:-G_1D][blk] = ot.reshape(Lq, H * D)
            else:
                so, to = sp["o"], bufs["o"]
                if d == "output_past_d":
                    ot = torch.nn.functional.pad(ot, (0, PAD_D))
                    so.put(to, b, q0, q0 + Lq, ot, D + PAD_D)
                else:
                    so.put(to, b, q0, q0 + Lq, ot)
                if d == "output_row_past":
                    so.put(to, b, q0 + Lq, q0 + Lq + 1, ot[-1:])
                if dense:
                    bufs["lse"][G_1D:-G_1D].view(c.B, H, Lq)[b] = lse.float()
                else:
                    bufs["lse"][G_1D:-G_1D].view(H, built.meta["total_q"])[:, q0:q0 + Lq] = lse.float()
            if dense and c.carry is not None:
                bufs["o_acc"][G_1D:-G_1D].view(c.B, Lq, H, D)[b] = o.float()
        if d == "input_modified":
            s = sp["k"] if not paged else None
            t = bufs[s.buf] if s is not None else bufs["k_cache"]
            bits(t).view(-1)[t.numel() // 2] ^= 1
        return bufs

    @staticmethod
    def _gather(s, t, b, k0, p, dw):
        """Rows k0 + p of operand s of buffer t as [n, h, dw]."""
        full = s.get(t, b, 0, int(p.max()) + k0 + 1, dw)
        return full[(p + k0).long()]


# ---- the launch ----------------------------------------------------------------------------------------------------------
def params(built: Built, t):
    """The C-ABI parameters of the case's launch on the buffers t ({name: tensor}, any device; nothing is dereferenced),
    built by mio.ops' own argument checks, with lse / the blocked output pointed into their guarded buffers.  Asserts that
    every operand address is its embedded view's: a copy made on the way would make the case vacuous.
    Returns (params, window, route query, launch function, route names, keep-alive)."""
    import ctypes

    from mio import _lib, ops
    c, sp = built.case, built.specs
    V = {n: sp[n].view(t[sp[n].buf]) for n in sp}
    lib = _lib.lib
    lse_ptr = t["lse"].data_ptr() + 4 * G_1D if "lse" in t else None
    if c.form == "dense":
        kw = dict(layout=c.layout, causal=c.causal, q_offset=c.q_offset, k_offset=c.k_offset, k_prescaled=c.kpre,
                  out_blocked=c.oblk)
        if c.mask:
            kw["keep_mask" if c.mask == "keep" else "additive_mask"] = t["mask"][built.bufs["mask"].spec]
        if not c.oblk:
            kw.update(out=V["o"], lse=t["lse"][G_1D:-G_1D].view(c.B, c.H, c.Sq))
        if c.carry is not None:
            kw.update(o_acc=t["o_acc"][G_1D:-G_1D].view(c.B, c.Sq, c.H, c.D), carry_in=bool(c.carry))
        p, _out, _lse, keep = ops._fa3_params(V["q"], V["k"], V["v"], **kw)
        keep = (keep, _out, _lse)
        if c.oblk:
            p.o = t["o"].data_ptr() + G_1D * t["o"].element_size()
        else:
            assert p.o == V["o"].data_ptr() and p.lse == lse_ptr
        if c.mask:
            assert p.mask == t["mask"][built.bufs["mask"].spec].data_ptr(), "the mask was copied"
        if c.carry is not None:
            assert p.o_acc == t["o_acc"].data_ptr() + 4 * G_1D
        assert (p.q, p.k, p.v) == tuple(V[n].data_ptr() for n in "qkv"), "an operand was copied"
        fns = (lib.mio_fa3_route_window, lib.mio_fa3_fwd_window, _lib.FA3_ROUTES)
    elif c.form == "varlen":
        p, _out, _lse, keep = ops._varlen_params(V["q"], V["k"], V["v"], t["cu_q"], t["cu_k"], built.meta["max_q"],
                                                 built.meta["max_k"], causal=c.causal, return_lse=True, out=V["o"])
        p.lse = lse_ptr
        assert (p.q, p.k, p.v, p.o) == tuple(V[n].data_ptr() for n in "qkvo"), "an operand was copied"
        fns = (lib.mio_fa3_varlen_route_window, lib.mio_fa3_fwd_varlen_window, _lib.FA3_VARLEN_ROUTES)
    else:
        p, _out, _lse, keep = ops._paged_params(V["q"], t["k_cache"], t["v_cache"], t["table"], t["cu_q"], t["seqused"],
                                                built.meta["max_q"], built.meta["max_k"], layer_idx=LAYER, causal=c.causal,
                                                return_lse=True, out=V["o"])
        p.lse = lse_ptr
        assert (p.q, p.o) == (V["q"].data_ptr(), V["o"].data_ptr()), "an operand was copied"
        fns = (lib.mio_fa3_paged_route_window, lib.mio_fa3_fwd_paged_window, _lib.FA3_PAGED_ROUTES)
    assert p.q % 16 == 0 and p.o % 16 == 0
    return (p, ops._window(c.window, c.causal)) + fns + (keep,)


def route(built: Built, t) -> str:
    from mio import ops
    p, w, query, _fwd, names, _keep = params(built, t)
    return ops._route(query, p, w, names)

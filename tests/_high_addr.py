"""Placements of the high-address tests (a plain helper module, not a conftest): where, in allocations of many GiB, the few
live rows of a case lie, so that the bytes a launch touches sit on both sides of the byte offsets 2^31, 2^32 and 2^33 of the
tensor the kernel is handed (BOUNDS; 2^32 bytes is 2^31 16-bit elements, 2^33 bytes 2^32 of them -- and the 2^32-unit edge
of an fp8 cache whose strides travel in 16-bit units).

Everything here is integer arithmetic on byte offsets and runs on the host (tests/test_high_addr_host.py checks it); the GPU
tests (tests/test_gpu_high_addr_attention.py, tests/test_gpu_high_addr_writes.py) allocate what a Case describes.

A Case names its allocations (every byte of which the GPU test first sets to 0xFF: NaN as bf16, fp16 and e4m3fn) and its
tensors: the allocation a tensor lives in, the offset of its first byte there, its live byte ranges relative to that first
byte, and the boundaries it claims.  The rules the host test holds every case to:
  * a claimed boundary has a live range ending at or below it and one starting at or above it, each within `near` bytes;
  * for every live range at offset a, the ranges at a + 2^32, a - 2^32, a mod 2^32 and a mod 2^31 (what a truncated, a
    sign-flipped or a wrapped address computation would touch) lie inside the same allocation and on no live range of any
    tensor there -- a wrong read returns NaN, a wrong write damages filler that the scan after the launch counts; no case can
    reach memory outside its allocations;
  * allocations plus the case's other device memory stay within 24 GiB.

Paged caches [num_blocks, L, block_size, Hkv, D] use L = 3 and layer 2: a page is 3 * 2^m bytes, so no page ends on a power
of two, and a shift by 2^31 or 2^32 bytes moves a live layer onto another layer of some page -- filler, whatever the page
numbers.  (A shift by 3 * 2^31 keeps the layer: the pages around the three boundaries are therefore taken at distances
1 + i + 3j below and i + 3j above boundary i, which never differ by a multiple of the shift.)  Logical pages alternate below
/ above the boundaries in turn, so consecutive key tiles of one sequence cross a boundary in both directions.
"""
from __future__ import annotations

import bisect
from dataclasses import dataclass, field
from typing import Dict, List, Tuple

GIB = 1 << 30
BOUNDS = (1 << 31, 1 << 32, 1 << 33)
LIMIT = 24 * GIB
FILL = 0xFF
L, LAYER = 3, 2


def alias_offsets(a: int) -> Tuple[int, ...]:
    """Where a wrong 64-bit address computation would put offset a (the forms of the module docstring), a itself dropped."""
    return tuple(x for x in dict.fromkeys((a + (1 << 32), a - (1 << 32), a % (1 << 32), a % (1 << 31))) if x != a)


@dataclass
class Tensor:
    name: str
    alloc: str
    base: int                              # byte offset of the tensor's first element in its allocation
    live: List[Tuple[int, int]]            # [start, end) byte ranges relative to base
    bounds: Tuple[int, ...] = ()           # the boundaries (relative to base) the tensor claims
    near: int = 0                          # "immediately": a live range within this many bytes of a claimed boundary


@dataclass
class Case:
    name: str
    allocs: Dict[str, int]
    tensors: List[Tensor]
    extra: int = 0                         # other device memory alive with the allocations (compact twins, references)
    info: dict = field(default_factory=dict)

    def tensor(self, name: str) -> Tensor:
        return next(t for t in self.tensors if t.name == name)

    def peak(self) -> int:
        return sum(self.allocs.values()) + self.extra


def _absolute(case: Case, alloc: str):
    iv = sorted((t.base + s, t.base + e) for t in case.tensors if t.alloc == alloc for s, e in t.live)
    return iv, [s for s, _ in iv]


def check_case(case: Case) -> None:
    """The rules of the module docstring; AssertionError naming the case, the tensor and the range."""
    assert case.peak() <= LIMIT, f"{case.name}: {case.peak() / GIB:.2f} GiB alive"
    for alloc in case.allocs:
        iv, _ = _absolute(case, alloc)
        for (s0, e0), (s1, e1) in zip(iv, iv[1:]):
            assert e0 <= s1, f"{case.name}: live ranges overlap in {alloc}: [{s0}, {e0}) and [{s1}, {e1})"
    for t in case.tensors:
        size = case.allocs[t.alloc]
        iv, starts = _absolute(case, t.alloc)
        assert t.live, f"{case.name}: {t.name} has no live range"
        for b in t.bounds:
            below = [b - e for s, e in t.live if e <= b]
            above = [s - b for s, e in t.live if s >= b]
            assert below and min(below) < t.near, f"{case.name}: {t.name} has no live range just below {b:#x}"
            assert above and min(above) < t.near, f"{case.name}: {t.name} has no live range just above {b:#x}"
        for s, e in t.live:
            assert 0 <= t.base + s and t.base + e <= size, f"{case.name}: {t.name} [{s}, {e}) leaves {t.alloc}"
            for a in alias_offsets(s):
                lo, hi = t.base + a, t.base + a + (e - s)
                assert 0 <= lo and hi <= size, f"{case.name}: {t.name} alias {a:#x} of [{s:#x}, {e:#x}) leaves {t.alloc}"
                i = bisect.bisect_right(starts, lo)
                for j in (i - 1, i):
                    if 0 <= j < len(iv):
                        assert iv[j][1] <= lo or iv[j][0] >= hi, (
                            f"{case.name}: {t.name} alias {a:#x} of [{s:#x}, {e:#x}) lies on a live range")


# ---- paged caches --------------------------------------------------------------------------------------------------------
def boundary_pages(page_bytes: int, layer_bytes: int, n: int, layer: int = LAYER) -> List[int]:
    """n physical pages whose `layer` lies entirely below or entirely above a boundary, in the order below 2^31, above 2^31,
    below 2^32, above 2^32, below 2^33, above 2^33, then the next ring of pages further out (module docstring)."""
    out: List[int] = []
    j = 0
    while len(out) < n:
        for i, b in enumerate(BOUNDS):
            d = i + 3 * j
            out.append(b // page_bytes - 1 - d)                          # the whole page ends at or below b
            out.append(-(-(b - layer * layer_bytes) // page_bytes) + d)  # its live layer starts at or above b
        j += 1
    return out[:n]


def paged_case(name: str, *, bs: int, Hkv: int, D: int, esz: int, npages: int, extra: int = 0) -> Case:
    """K and V caches [num_blocks, 3, bs, Hkv, D] of esz-byte elements, each just over 8 GiB, side by side in one allocation
    "kv" (so each one's aliases past its own ends fall into filler of the same allocation): 2 GiB and 32 pages of filler,
    the K cache, the V cache, 4 GiB of filler.  info: pages (boundary_pages, the physical pages of logical pages 0 .. npages
    - 1, the same in K and V), num_blocks, page / layer / token bytes."""
    tok = Hkv * D * esz
    lb = bs * tok
    pb = L * lb
    pages = boundary_pages(pb, lb, npages)
    nb = max(pages) + 2
    cache = nb * pb
    front = (1 << 31) + 32 * pb
    live = sorted((p * pb + LAYER * lb, p * pb + (LAYER + 1) * lb) for p in pages)
    reach = tuple(b for b in BOUNDS)
    tensors = [Tensor("k_cache", "kv", front, live, reach, near=4 * pb),
               Tensor("v_cache", "kv", front + cache, list(live), reach, near=4 * pb)]
    return Case(name, {"kv": front + 2 * cache + (1 << 32)}, tensors, extra,
                dict(pages=pages, num_blocks=nb, page_bytes=pb, layer_bytes=lb, tok_bytes=tok, bs=bs, Hkv=Hkv, D=D, esz=esz,
                     cache_bytes=cache))


def pages_needed(lens_k, bs: int) -> List[int]:
    return [(n + bs - 1) // bs for n in lens_k]


def block_table(lens_k, bs: int, pages: List[int]) -> List[List[int]]:
    """Rows of physical pages, logical page j of sequence b the (sum of earlier sequences' pages + j)-th of `pages`; rows
    padded with page 0 (never read: past seqused_k)."""
    need = pages_needed(lens_k, bs)
    width = max(need + [1])
    rows, nxt = [], 0
    for n in need:
        rows.append(pages[nxt:nxt + n] + [0] * (width - n))
        nxt += n
    return rows


# ---- strided views -------------------------------------------------------------------------------------------------------
ROW_PITCH = (1 << 23) + 4096   # bytes between token rows of the wide buffers: 2^22 + 2048 16-bit elements, a multiple of 8


def rows_case(name: str, *, rows: int, cols: Dict[str, Tuple[int, int]], pitch: int = ROW_PITCH, extra: int = 0,
              bounds=BOUNDS) -> Case:
    """Token rows `pitch` bytes apart in one allocation "wide", the view starting 4 GiB into it and 4 GiB of filler behind
    the last row; cols: tensor name -> (byte offset of its columns in a row, bytes per row).  The pitch is no power of two,
    so a shift by 2^31 or 2^32 lands between the columns of another row."""
    front = 1 << 32
    tensors = []
    for tname, (off, width) in cols.items():
        live = [(r * pitch, r * pitch + width) for r in range(rows)]
        reach = tuple(b for b in bounds if b + pitch <= rows * pitch)
        tensors.append(Tensor(tname, "wide", front + off, live, reach, near=pitch))
    return Case(name, {"wide": front + rows * pitch + (1 << 32)}, tensors, extra, dict(pitch=pitch, rows=rows, front=front))


BATCH_PITCH = (1 << 32) + (1 << 22)   # bytes between the batches of the dense cases


def dense_case(name: str, *, B: int, S: int, cols: Dict[str, Tuple[int, int]], row_bytes: int, extra: int = 0) -> Case:
    """[B, S, ..] tensors whose batches lie BATCH_PITCH bytes apart (batch 1 starts past 2^32, batch 2 past 2^33), rows
    row_bytes apart inside a batch, the columns of q / k / v / o side by side in a row; 4 GiB of filler in front and behind.
    With S rows of a few KiB no batch reaches a boundary from below, so the tensors claim none: what the case shows is the
    batch product b * stride past 2^32 and 2^33 bytes."""
    assert S * row_bytes < (1 << 22)
    front = 1 << 32
    tensors = []
    for tname, (off, width) in cols.items():
        live = [(b * BATCH_PITCH + s * row_bytes, b * BATCH_PITCH + s * row_bytes + width) for b in range(B) for s in range(S)]
        tensors.append(Tensor(tname, "wide", front + off, live))
    return Case(name, {"wide": front + (B - 1) * BATCH_PITCH + S * row_bytes + (1 << 32)}, tensors, extra,
                dict(front=front, row_bytes=row_bytes))


# ---- the span limit of the pipelined kernels -----------------------------------------------------------------------------
def span32(Sk: int, ks_s: int, vs_s: int) -> bool:
    """csrc/fa3_route.h, fa3_pick_route: K / V rows within 4 GiB of their (batch, head) base."""
    return Sk * ks_s * 2 < (1 << 32) and Sk * vs_s * 2 < (1 << 32)


def largest_stride(Sk: int) -> int:
    """The largest row stride (elements, a multiple of 8) span32 admits for Sk keys."""
    return ((1 << 32) - 1) // (2 * Sk) // 8 * 8


SPAN_SQ = 200
SPAN_SK = {"i": 320, "ii": 100}   # (i): the last tile's scalar offset just under 2^32; (ii): lane offsets of tile 0 past 2^31


def span_case(which: str, D: int, step: int) -> Case:
    """K and V [1, Sk, 1, D] with the row stride largest_stride(Sk) + 8 * step elements (step 0: the last stride the pipelined
    kernels take; step 1: the first one fwd1 takes), V's columns 16 KiB behind K's in the same rows; q and o are compact."""
    Sk = SPAN_SK[which]
    stride = largest_stride(Sk) + 8 * step
    case = rows_case(f"span_{which}_D{D}_step{step}", rows=Sk, cols={"k": (0, 2 * D), "v": (16384, 2 * D)}, pitch=2 * stride,
                     extra=1 << 26)
    case.info.update(Sk=Sk, stride=stride, Sq=SPAN_SQ)
    return case


# ---- what the GPU tests share ---------------------------------------------------------------------------------------------
def allocate(case: Case, device="cuda"):
    """The allocations of a case, every byte 0xFF: dict name -> uint8 tensor.  A failed allocation is a failure."""
    import torch
    out = {}
    for aname, size in case.allocs.items():
        try:
            buf = torch.empty(size, dtype=torch.uint8, device=device)
        except RuntimeError as e:  # no skip on low memory
            raise AssertionError(f"{case.name}: cannot allocate {size / GIB:.2f} GiB for '{aname}': {e}") from None
        buf.fill_(FILL)
        out[aname] = buf
    return out


def view(bufs, case: Case, name: str, dtype, shape, strides=None):
    """The tensor `name` of the case as a view of its allocation: contiguous `shape`, or as_strided in elements."""
    import torch
    t = case.tensor(name)
    esz = torch.empty((), dtype=dtype).element_size()
    flat = bufs[t.alloc][t.base:].view(dtype)
    if strides is None:
        n = 1
        for s in shape:
            n *= s
        return flat[:n].view(shape)
    assert all(s >= 0 for s in strides) and esz
    return flat.as_strided(shape, strides)


def count_not_fill(buf, chunk: int = 1 << 27) -> int:
    """Bytes of a uint8 device tensor that are not 0xFF: one pass over 8-byte words, then the bytes of the few words that
    differ."""
    import torch
    n8 = buf.numel() // 8 * 8
    words = buf[:n8].view(torch.int64)
    total = int((buf[n8:] != FILL).sum())
    for i in range(0, words.numel(), chunk):
        w = words[i:i + chunk]
        hit = w[w != -1]
        if hit.numel():
            total += int((hit.view(torch.uint8) != FILL).sum())
    return total


def live_bytes(*tensors) -> int:
    """Bytes != 0xFF of the given (compact) tensors: what the scan of an allocation holding exactly them must count."""
    import torch
    return sum(int((t.contiguous().view(torch.uint8) != FILL).sum()) for t in tensors)


# ---- the expected bytes of a cache write ---------------------------------------------------------------------------------
def write_slots(new, ctx_after, bs: int, table: List[List[int]]):
    """(token, page, slot) of every token a varlen cache write stores: token i of the n_b new ones of sequence b goes to
    position ctx_after[b] - n_b + i, page table[b][pos // bs], slot pos % bs; negative positions and positions past the
    table row are skipped."""
    out, t = [], 0
    for b, n in enumerate(new):
        for i in range(n):
            pos = ctx_after[b] - n + i
            if pos >= 0 and pos // bs < len(table[b]):
                out.append((t, table[b][pos // bs], pos % bs))
            t += 1
    return out


def expected_cache(cache, rows, slots, layer: int):
    """cache [num_blocks, L, bs, Hkv, D] (any device) with rows[t] ([T, Hkv, D], already in the cache's format) stored at
    the (page, slot) of write_slots; returns the modified clone."""
    import torch
    out = cache.clone()
    if slots:
        t, page, slot = (torch.tensor(x, dtype=torch.long, device=cache.device) for x in zip(*slots))
        esz = cache.element_size()
        bits = {1: torch.uint8, 2: torch.int16}[esz]
        out.view(bits)[page, layer, slot] = rows.to(cache.device).contiguous().view(bits)[t]
    return out


# ---- the cases of the GPU tests ------------------------------------------------------------------------------------------
H, HKV = 4, 2
PAGED_LQ, PAGED_LK = [300, 77, 1], [700, 77, 513]   # a chunk over a prefix, a whole short prompt, a decode-like row
PAGED_GEOM = [(bs, D) for bs in (64, 256) for D in (64, 128)]


def paged_attention_case(bs: int, D: int, esz: int) -> Case:
    """The caches of the paged-prefill cases: PAGED_LK's pages, in order, on boundary_pages."""
    return paged_case(f"paged_bs{bs}_D{D}_esz{esz}", bs=bs, Hkv=HKV, D=D, esz=esz, npages=sum(pages_needed(PAGED_LK, bs)),
                      extra=1 << 28)


VARLEN_LENS = [300, 300, 500]   # rows 0 .. 299 below 4 GiB, 300 .. 599 across it (row 512), 600 .. 1099 above it and across 8 GiB


def varlen_case(D: int) -> Case:
    """q, k, v and o of the packed cases: columns of the same wide rows (q at 0, k at 16 KiB, v at 32 KiB, o at 48 KiB)."""
    return rows_case(f"varlen_D{D}", rows=sum(VARLEN_LENS), extra=1 << 28,
                     cols={"q": (0, 2 * H * D), "k": (16384, 2 * HKV * D), "v": (32768, 2 * HKV * D), "o": (49152, 2 * H * D)})


DENSE_B, DENSE_S = 3, 200


def dense_attention_case(D: int) -> Case:
    return dense_case(f"dense_D{D}", B=DENSE_B, S=DENSE_S, row_bytes=4096, extra=1 << 28,
                      cols={"q": (0, 2 * H * D), "k": (1024, 2 * HKV * D), "v": (1536, 2 * HKV * D), "o": (2048, 2 * H * D)})


SRC_PITCH = (1 << 26) + 4096   # bytes between the source tokens of the write cases: token 64 starts past 2^32
WRITE_NEW = [70, 1, 5]         # 76 new tokens: sequence 0 crosses from its first page (below 2^31) to its second (above)
WRITE_GEOM = [(64, 2, 64), (64, 2, 128), (256, 2, 64)]   # (bs, Hkv, D)


def write_ctx(bs: int) -> List[int]:
    """context_lengths after the append: sequence 0 ends 36 slots into its second page, sequence 1's one token is the
    second slot of its third page, sequence 2 crosses from its first page to its second."""
    return [bs + 36, 2 * bs + 2, bs + 2]


def write_case(bs: int, Hkv: int, D: int, esz: int, heads: int = 0) -> Case:
    """The caches of paged_case with the pages of write_ctx, and the sources inside the same allocation, on filler of the K
    cache's region: key / value (and, heads > 0, q / q_out [T, heads, D]) are columns of token rows SRC_PITCH apart whose
    first row lies 4 GiB and 16 MiB into the allocation."""
    ctx = write_ctx(bs)
    case = paged_case(f"write_bs{bs}_Hkv{Hkv}_D{D}_esz{esz}_h{heads}", bs=bs, Hkv=Hkv, D=D, esz=esz,
                      npages=sum(pages_needed(ctx, bs)), extra=1 << 28)
    T = sum(WRITE_NEW)
    src = (1 << 32) + (1 << 24)
    cols = {"key": (0, 2 * Hkv * D), "value": (1024, 2 * Hkv * D)}
    if heads:
        cols.update(q=(2048, 2 * heads * D), q_out=(4096, 2 * heads * D))
    for tname, (off, width) in cols.items():
        live = [(t * SRC_PITCH, t * SRC_PITCH + width) for t in range(T)]
        case.tensors.append(Tensor(tname, "kv", src + off, live, (1 << 32,), near=SRC_PITCH))
    case.info.update(ctx=ctx, new=list(WRITE_NEW), table=block_table(ctx, bs, case.info["pages"]), T=T)
    return case


ROTARY_T, ROTARY_HEADS = 80, 4


def rotary_case(D: int) -> Case:
    return rows_case(f"rotary_D{D}", rows=ROTARY_T, pitch=SRC_PITCH, extra=1 << 26, bounds=(1 << 32,),
                     cols={"x": (0, 2 * ROTARY_HEADS * D), "out": (8192, 2 * ROTARY_HEADS * D)})


NORM_ROWS, NORM_COLS = (1 << 21) + 300, 1024            # x and y each just over 4 GiB
MERGE_SHAPE = (((1 << 31) // (8 * 64 * 256)) + 1, 256, 8, 64)   # B*Sq*H*D just over 2^31: o_a / o_b 8 GiB, o_out 4 GiB
BLOCKED_SHAPE = ((1 << 14) + 1, 256, 8, 2, 64)            # (B, Sq, H, Hkv, D) of the blocked-output case: o just over 4 GiB


def contiguous_peaks() -> Dict[str, int]:
    """Bytes alive in the cases on whole contiguous tensors (no placement: every element is live)."""
    norm = NORM_ROWS * NORM_COLS * 2
    slab = (1 << 16) * NORM_COLS * 2
    B, Sq, Hm, D = MERGE_SHAPE
    merge32 = B * Sq * Hm * D * 4
    mslab = 512 * Sq * Hm * D * 4
    Bb, Sb, Hb, Hkvb, Db = BLOCKED_SHAPE
    qb = Bb * Sb * Hb * Db * 2
    return {
        # x, residual, y and sum_out with their guards; two slabs, a slice's x / residual / y / sum, a 2 GiB compare mask
        "norm": 4 * norm + 2 * slab + 4 * slab + (1 << 31) + (1 << 20),
        # o_a, o_b, the 16-bit o_out, two lse; the slab's four states, its merged copy and 16-bit output
        "merge": 2 * merge32 + merge32 // 2 + 2 * merge32 // D + 3 * mslab + mslab // 2 + 4 * mslab // D,
        # q, o, k, v and the slab's
        "blocked": 2 * qb + 2 * qb * Hkvb // Hb + (2 * qb + 2 * qb * Hkvb // Hb) * 512 // Bb + (1 << 28),
    }


def all_cases() -> List[Case]:
    out = [paged_attention_case(bs, D, esz) for bs, D in PAGED_GEOM for esz in (2, 1)]
    out += [varlen_case(D) for D in (64, 128)] + [dense_attention_case(D) for D in (64, 128)]
    out += [span_case(w, D, step) for w in ("i", "ii") for D in (64, 128) for step in (0, 1)]
    out += [write_case(bs, Hkv, D, esz) for bs, Hkv, D in WRITE_GEOM for esz in (2, 1)]
    out += [write_case(64, 2, D, esz, heads=4) for D in (64, 128) for esz in (2, 1)]
    out += [rotary_case(D) for D in (64, 128)]
    return out

"""The placements of the high-address GPU tests (tests/_high_addr.py), checked on the host: integer arithmetic only, nothing
is allocated.  Every case keeps the rules of _high_addr's docstring (boundaries, aliases on filler inside the allocation,
24 GiB); the span-limit strides sit on the two sides of fa3_route.h's span32 and case (ii) has lane offsets past 2^31; the
expected-bytes builder of the write cases reproduces the byte-exact expectations of tests/test_gpu_kv8.py at their shapes;
and a planted truncation of a page's address does land on filler of the case's own allocation."""
import pytest
import torch

import _high_addr as ha

CASES = ha.all_cases()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_case_rules(case):
    ha.check_case(case)


def test_rules_bite():
    """check_case refuses a power-of-two row pitch (aliases on live rows), a missing side of a boundary, an alias outside
    the allocation and an allocation past 24 GiB."""
    with pytest.raises(AssertionError, match="lies on a live range"):
        ha.check_case(ha.rows_case("pow2", rows=1100, cols={"q": (0, 512)}, pitch=1 << 23))
    c = ha.rows_case("one_sided", rows=600, cols={"q": (0, 512)})
    c.tensors[0].bounds = (1 << 33,)
    with pytest.raises(AssertionError, match="just below|just above"):
        ha.check_case(c)
    c = ha.rows_case("no_front", rows=600, cols={"q": (0, 512)})
    c.tensors[0].base -= 1 << 32
    with pytest.raises(AssertionError, match="leaves"):
        ha.check_case(c)
    c = ha.paged_attention_case(64, 64, 2)
    c.extra = 3 * ha.GIB
    with pytest.raises(AssertionError, match="GiB alive"):
        ha.check_case(c)


def test_contiguous_cases_reach_their_boundaries_within_24_gib():
    for name, peak in ha.contiguous_peaks().items():
        assert peak <= ha.LIMIT, f"{name}: {peak / ha.GIB:.2f} GiB alive"
    assert ha.NORM_ROWS * ha.NORM_COLS * 2 > 1 << 32 and ha.NORM_ROWS % 256 != 0          # y crosses 2^31 and 2^32 bytes, ragged tail
    B, Sq, H, D = ha.MERGE_SHAPE
    assert B * Sq * H * D > 1 << 31 and (B - 1) * Sq * H * D == 1 << 31                  # the last batch starts at element 2^31
    Bb, Sb, Hb, _, Db = ha.BLOCKED_SHAPE
    assert Bb * Sb * Hb * Db > 1 << 31 and Sb == 256 and (Hb * Db) % 32 == 0              # one 256-row block per batch


@pytest.mark.parametrize("bs,D", ha.PAGED_GEOM)
@pytest.mark.parametrize("esz", [2, 1])
def test_paged_pages_alternate_across_every_boundary(bs, D, esz):
    """Consecutive logical pages of the first ring lie on opposite sides of a boundary, every page's row index fits 32 bits
    (the kernels' `fewer than 2^32 token rows`), every page is distinct, and each cache is just over 8 GiB."""
    case = ha.paged_attention_case(bs, D, esz)
    i = case.info
    pages, pb, lb = i["pages"], i["page_bytes"], i["layer_bytes"]
    assert len(set(pages)) == len(pages) and min(pages) > 0
    for n, b in enumerate(ha.BOUNDS):
        lo, hi = pages[2 * n], pages[2 * n + 1]
        assert (lo + 1) * pb <= b <= hi * pb + ha.LAYER * lb
    assert i["num_blocks"] * ha.L * bs < 1 << 32
    assert (1 << 33) < i["cache_bytes"] < (1 << 33) + (1 << 26)
    # a truncated product r * row_bytes (fa3_paged.h, tile_base) of a page above 2^32 lands inside the cache, on filler
    t = case.tensor("k_cache")
    for p in pages:
        a = p * pb + ha.LAYER * lb
        if a >= 1 << 32:
            w = a % (1 << 32)
            assert all(e <= w or s >= w + lb for s, e in t.live)


@pytest.mark.parametrize("which", ["i", "ii"])
@pytest.mark.parametrize("D", [64, 128])
def test_span_limit_strides(which, D):
    Sk = ha.SPAN_SK[which]
    s = ha.largest_stride(Sk)
    assert s % 8 == 0 and ha.span32(Sk, s, s) and not ha.span32(Sk, s + 8, s + 8)
    assert not ha.span32(Sk, s + 8, s) and not ha.span32(Sk, s, s + 8)
    if which == "i":
        assert s == 6710880
        last_tile = (Sk - 1) // 64
        assert 1 << 31 < last_tile * 64 * 2 * s < 1 << 32                       # the last tile's scalar offset
        assert (1 << 32) - 16 * Sk <= Sk * 2 * s < 1 << 32                     # the span: one stride step under 2^32
    else:
        over = [r for r in range(64) if r * 2 * s + 2 * D - 16 >= 1 << 31]       # rows of tile 0 whose lane offset is past 2^31
        assert over and over[-1] == 63 and 64 * 2 * s >= 1 << 31 and 63 * 2 * s < 1 << 32
    for step in (0, 1):
        c = ha.span_case(which, D, step)
        assert c.info["stride"] == s + 8 * step and c.tensor("k").base >= 1 << 32


def test_write_case_crosses_the_boundaries():
    for bs, Hkv, D in ha.WRITE_GEOM:
        c = ha.write_case(bs, Hkv, D, 2)
        i = c.info
        slots = ha.write_slots(i["new"], i["ctx"], bs, i["table"])
        assert len(slots) == i["T"]
        pb, lb, tok = i["page_bytes"], i["layer_bytes"], i["tok_bytes"]
        addr = [p * pb + ha.LAYER * lb + s * tok for _, p, s in slots]
        for b in ha.BOUNDS:
            assert any(a + tok <= b for a in addr) and any(a >= b for a in addr)
        seq0 = addr[:i["new"][0]]
        assert min(seq0) < 1 << 31 <= max(seq0)                      # one sequence's tokens cross 2^31
        assert (i["T"] - 1) * ha.SRC_PITCH > 1 << 32                   # and the source rows pass 2^32


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_expected_bytes_match_the_kv8_fixture(dtype):
    """tests/test_gpu_kv8.py::test_kv8_write_varlen_byte_exact's inputs and its own loop, against write_slots +
    expected_cache (16-bit rows and _quant_ref rows)."""
    from test_gpu_kv8 import F8, _quant_ref
    g = torch.Generator().manual_seed(11)
    Hkv, D, L, bs, layer = 2, 128, 3, 16, 1
    key = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dtype).view(256, Hkv, D)
    maxb, nb = 9, 40
    bt = torch.randperm(nb, generator=g)[:3 * maxb].view(3, maxb).to(torch.int32)
    cu = [0, 100, 220, 256]
    ctx = [130, 120, 160]
    new = [cu[b + 1] - cu[b] for b in range(3)]
    for cache_dtype, rows in ((F8, _quant_ref(key, 0.37)), (dtype, key)):
        if cache_dtype == F8:
            cache = torch.full((nb, L, bs, Hkv, D), 0x5A, dtype=torch.uint8).view(F8)
        else:
            cache = torch.full((nb, L, bs, Hkv, D), 1.5, dtype=dtype)
        want = cache.clone()
        for b in range(3):
            for i in range(new[b]):
                pos = ctx[b] - new[b] + i
                if pos < 0 or pos // bs >= maxb:
                    continue
                want[int(bt[b, pos // bs]), layer, pos % bs] = rows[cu[b] + i]
        got = ha.expected_cache(cache, rows, ha.write_slots(new, ctx, bs, bt.tolist()), layer)
        bits = torch.uint8 if cache_dtype == F8 else torch.int16
        assert torch.equal(got.view(bits), want.view(bits))
        assert not torch.equal(got.view(bits), cache.view(bits))

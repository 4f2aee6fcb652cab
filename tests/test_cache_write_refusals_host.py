"""CPU-only: what the six writes into the paged KV cache refuse and what they accept without work, pinned through the C ABI.

  mio_reshape_and_cache(_kv8)             one token per sequence, 16-bit or fp8 (e4m3fn) cache
  mio_reshape_and_cache_varlen(_kv8)      packed new tokens
  mio_rope_and_cache_varlen(_kv8)         packed new tokens, rotary position embedding fused in

Every case of CASES is BASE[fn] with `changes` applied.  BASE[fn] itself is a valid call that would launch, so it is never
made: a case is either wrong in exactly one way (refused with a non-zero return and mio_last_error() equal to the literal,
entry-point prefix included), or has no work (B == 0 or total_new == 0 of a varlen form) and returns 0 without a launch,
listed directly after the refusal it neighbours.  `_call` asserts that a call expected to return 0 has no work, so nothing
here reaches the fake addresses; the file is safe where a GPU is present.  The order of the checks is not part of the
contract: a doubly-wrong call (PAIRS) is refused with either of its two messages.

Where a form does not check what its siblings check, a no-work call pins the accept.  What only a launching call could show
is left to the GPU tests (the single-token forms require B > 0, so they have no accepting side here):
  mio_reshape_and_cache accepts max_blocks_per_seq <= 0 (its kernel then writes nothing); its fp8 twin refuses it
  both single-token forms accept negative strides; the varlen forms refuse them
  no plain form bounds head_dim from above; the rotating forms stop at 128
The one case in which the forms were brought into line: mio_reshape_and_cache refuses a null k_stride / v_stride with its
"null pointer" message as its fp8 twin does (test_single_token_null_stride_is_refused); it used to read through them."""
import ctypes as C

import pytest

A = 1 << 20  # a fake 16-byte aligned device address

_PLAIN = "key value k_cache v_cache {s}block_tables {cu}context_lengths k_stride v_stride B {t}Hkv D {nb}num_layers layer_idx " \
    "block_size max_blocks_per_seq dtype"
_ROPE = "q q_out key value k_cache v_cache {s}block_tables cu_seqlens_new context_lengths positions cos sin q_stride q_out_stride " \
    "k_stride v_stride B total_new H Hkv D rot_dim max_position interleaved num_blocks num_layers layer_idx block_size " \
    "max_blocks_per_seq dtype"
_SC = "k_scale v_scale "
# argument order of every entry point (include/mio_hip.h); `stream` is always null
SIG = {
    "mio_reshape_and_cache": _PLAIN.format(s="", cu="", t="", nb=""),
    "mio_reshape_and_cache_kv8": _PLAIN.format(s=_SC, cu="", t="", nb=""),
    "mio_reshape_and_cache_varlen": _PLAIN.format(s="", cu="cu_seqlens_new ", t="total_new ", nb="num_blocks "),
    "mio_reshape_and_cache_varlen_kv8": _PLAIN.format(s=_SC, cu="cu_seqlens_new ", t="total_new ", nb="num_blocks "),
    "mio_rope_and_cache_varlen": _ROPE.format(s=""),
    "mio_rope_and_cache_varlen_kv8": _ROPE.format(s=_SC),
}
ONE, ONE8, VAR, VAR8, ROPE, ROPE8 = SIG
VARLEN, KV8, ROTARY = (VAR, VAR8, ROPE, ROPE8), (ONE8, VAR8, ROPE8), (ROPE, ROPE8)

# a valid call of every form: 2 sequences (3 packed tokens), 8 / 2 heads of 128, layer 1 of 2, 8 blocks of 16, 4 per sequence
_ALL = dict(q=A, q_out=A, key=A, value=A, k_cache=A, v_cache=A, k_scale=A, v_scale=A, block_tables=A, cu_seqlens_new=A,
            context_lengths=A, positions=None, cos=A, sin=A, q_stride=(1024, 128), q_out_stride=(1024, 128),
            k_stride=(256, 128), v_stride=(256, 128), B=2, total_new=3, H=8, Hkv=2, D=128, rot_dim=64, max_position=4096,
            interleaved=0, num_blocks=8, num_layers=2, layer_idx=1, block_size=16, max_blocks_per_seq=4, dtype=0)
BASE = {fn: {k: _ALL[k] for k in sig.split()} for fn, sig in SIG.items()}

_NULL, _NULLST, _SIZES, _GEOM, _ALIGN = ": null pointer", ": null strides", ": bad sizes", ": bad cache geometry", ": 16-byte alignment"
_SCALES = ": k_scale and v_scale are required with an fp8 cache (null scale pointer or not 4-byte aligned)"
_D8 = ": head_dim must be a multiple of 16 for an fp8 cache"
_DTYPE, _DTYPE8 = ": dtype must be bf16 or fp16", ": dtype (of key and value) must be bf16 or fp16"
_MANY = ": too many tokens"
_RD, _RD8 = ": head_dim must be a multiple of 8 in [8,128]", ": head_dim must be a multiple of 16 in [16,128] for an fp8 cache"
_ROT = ": rot_dim must be a multiple of 16 in [16, head_dim]"
_IL = ": interleaved must be 0 (neox pairing) or 1"
_ROT32 = ": rot_dim must be a multiple of 32 for an fp8 cache with the neox pairing"
_MAXPOS, _TABNULL, _TABALIGN = ": max_position must be positive", ": null cos / sin table", ": 16-byte alignment (cos / sin tables)"
OK = None  # the expectation of a call that returns 0


def _head_dim_msg(fn):
    """The message of a head_dim the form does not take: the plain 16-bit forms fold it into their sizes check."""
    if fn in ROTARY:
        return _RD8 if fn in KV8 else _RD
    return _D8 if fn in KV8 else _SIZES


def _dtype_msg(fn):
    return _DTYPE8 if fn in KV8 and fn not in ROTARY else _DTYPE


def _strides(fn):
    return [s for s in ("q_stride", "q_out_stride", "k_stride", "v_stride") if s in BASE[fn]]


def _stride_faults(fn, bad):
    """Each element of each stride pair replaced by bad(element)."""
    for s in _strides(fn):
        t, h = BASE[fn][s]
        yield {s: (bad(t), h)}
        yield {s: (t, bad(h))}


def _cases(fn):
    """(changes, expectation) of one entry point: single faults, each no-work accept right after the refusal it neighbours."""
    varlen, kv8, rotary = fn in VARLEN, fn in KV8, fn in ROTARY
    data = [p for p in ("q", "q_out", "key", "value", "k_cache", "v_cache", "block_tables", "cu_seqlens_new", "context_lengths")
            if p in BASE[fn]]
    idle = (dict(B=0), dict(total_new=0)) if varlen else ()
    for z in idle:
        yield z, OK
    # ---- pointers: a varlen form looks at its strides first and at its data pointers only when there is work
    for p in data:
        yield {p: None}, _NULL
        for z in idle:
            yield dict(z, **{p: None}), OK
    for z in idle:
        yield dict(z, **{p: None for p in data}), OK
    for s in _strides(fn):
        if varlen:
            yield {s: None}, _NULLST
            for z in idle:
                yield dict(z, **{s: None}), _NULLST
        elif kv8:
            yield {s: None}, _NULL  # the 16-bit single-token form: test_single_token_null_stride_is_refused
    if kv8:
        for bad in (dict(k_scale=None), dict(v_scale=None), dict(k_scale=A + 2), dict(v_scale=A + 1),
                    dict(k_scale=None, v_scale=None)):
            yield bad, _SCALES
            for z in idle:
                yield dict(z, **bad), _SCALES
    # ---- sizes
    for bad in (dict(B=-1), dict(Hkv=0), dict(Hkv=-2)) + ((dict(total_new=-1),) if varlen else (dict(B=0),)):
        yield bad, _SIZES
    for z in idle:
        yield dict(z, Hkv=0), _SIZES
    if rotary:
        for bad in (dict(H=0), dict(H=-8), dict(H=3), dict(H=9)):
            yield bad, _SIZES
    # ---- head_dim: below, off-multiple, above.  A rotating form gets a rot_dim the head holds, so the head_dim is the only
    # fault; one below its smallest rot_dim never is (PAIRS)
    step = 16 if kv8 else 8
    for D in (((40, 72, 136, 144) if kv8 else (20, 68, 132, 136)) if rotary else (0, step // 2, step + step // 2, -step)):
        yield dict(D=D, rot_dim=32 if D > 32 else 16) if rotary else dict(D=D), _head_dim_msg(fn)
    if varlen and not rotary:  # no upper bound in the plain forms
        yield dict(B=0, D=256 + step), OK
        yield dict(total_new=0, D=1 << 20), OK
    if rotary:
        yield dict(B=0, D=144, rot_dim=64), _head_dim_msg(fn)
    # ---- cache geometry
    geom = [dict(layer_idx=-1), dict(layer_idx=2), dict(num_layers=0), dict(num_layers=1), dict(block_size=0), dict(block_size=-16)]
    if varlen:
        geom += [dict(num_blocks=0), dict(num_blocks=-1)]
    if varlen or kv8:  # mio_reshape_and_cache takes any max_blocks_per_seq
        geom += [dict(max_blocks_per_seq=0), dict(max_blocks_per_seq=-4)]
    for bad in geom:
        yield bad, _GEOM
    for z in idle:
        yield dict(z, num_blocks=0), _GEOM
        yield dict(z, max_blocks_per_seq=0), _GEOM
    for dt in (2, -1):
        yield dict(dtype=dt), _dtype_msg(fn)
    for z in idle:
        yield dict(z, dtype=2), _dtype_msg(fn)
    # ---- the rotation (as tests/test_rope_host.py, by literal)
    if rotary:
        for rot in (0, -16, 8, 24, 72, 144):
            yield dict(rot_dim=rot), _ROT
        yield dict(D=64, rot_dim=128), _ROT
        yield dict(B=0, rot_dim=24), _ROT
        for il in (2, -1):
            yield dict(interleaved=il), _IL
        if kv8:
            yield dict(rot_dim=16), _ROT32
            yield dict(D=64, rot_dim=48), _ROT32
            yield dict(B=0, rot_dim=16), _ROT32
            yield dict(B=0, rot_dim=16, interleaved=1), OK  # the interleaved pairing has no partner chunk
        else:
            yield dict(B=0, rot_dim=16), OK
        for mp in (0, -3):
            yield dict(max_position=mp), _MAXPOS
        yield dict(cos=None), _TABNULL
        yield dict(sin=None), _TABNULL
        yield dict(total_new=0, sin=None), _TABNULL
        yield dict(cos=A + 4), _TABALIGN
        yield dict(sin=A + 8), _TABALIGN
        yield dict(B=0, cos=A + 8), _TABALIGN
    # ---- 16-byte rows: strides of whole chunks, aligned addresses; only a varlen form refuses a negative stride
    for bad in _stride_faults(fn, lambda s: s + 4):
        yield bad, _ALIGN
        for z in idle:
            yield dict(z, **bad), OK
    if varlen:
        for bad in _stride_faults(fn, lambda s: -s):
            yield bad, _ALIGN
            for z in idle:
                yield dict(z, **bad), OK
    for p in data[:-3] if varlen else data[:-2]:  # the int32 arrays need no 16-byte alignment
        yield {p: A + 8}, _ALIGN
        for z in idle:
            yield dict(z, **{p: A + 8}), OK
    if rotary:
        yield dict(positions=A + 2), _ALIGN
        yield dict(positions=A + 1), _ALIGN
        yield dict(B=0, positions=A + 2), OK
    # ---- the grid: 2^20 tokens of 2^16 heads of 128 are 2^32 workgroups
    if varlen:
        big = dict(total_new=1 << 20, Hkv=1 << 16, k_stride=(1 << 23, 128), v_stride=(1 << 23, 128))
        if rotary:
            big.update(H=1 << 16, q_stride=(1 << 23, 128), q_out_stride=(1 << 23, 128))
        yield big, _MANY
        yield dict(big, B=0), OK


CASES = [(fn, ch, want) for fn in SIG for ch, want in _cases(fn)]

# doubly-wrong calls: (entry point, changes, the two messages either of which refuses it)
PAIRS = [
    (ONE, dict(key=None, B=0), (_NULL, _SIZES)),
    (ONE, dict(D=12, dtype=2), (_SIZES, _DTYPE)),
    (ONE, dict(layer_idx=2, k_cache=A + 8), (_GEOM, _ALIGN)),
    (ONE, dict(dtype=3, k_stride=(260, 128)), (_DTYPE, _ALIGN)),
    (ONE8, dict(k_scale=None, D=24), (_SCALES, _D8)),
    (ONE8, dict(value=None, v_scale=A + 2), (_NULL, _SCALES)),
    (ONE8, dict(B=0, max_blocks_per_seq=0), (_SIZES, _GEOM)),
    (ONE8, dict(D=8, dtype=2), (_D8, _DTYPE8)),
    (ONE8, dict(block_size=0, value=A + 8), (_GEOM, _ALIGN)),
    (VAR, dict(k_stride=None, Hkv=0), (_NULLST, _SIZES)),
    (VAR, dict(D=4, num_blocks=0), (_SIZES, _GEOM)),
    (VAR, dict(dtype=2, key=None), (_DTYPE, _NULL)),
    (VAR, dict(key=None, value=A + 8), (_NULL, _ALIGN)),
    (VAR, dict(B=0, D=4, dtype=2), (_SIZES, _DTYPE)),
    (VAR, dict(total_new=1 << 20, Hkv=1 << 16, k_stride=(1 << 23, 132), v_stride=(1 << 23, 128)), (_ALIGN, _MANY)),
    (VAR8, dict(v_stride=None, k_scale=None), (_NULLST, _SCALES)),
    (VAR8, dict(k_scale=A + 2, D=40), (_SCALES, _D8)),
    (VAR8, dict(D=40, layer_idx=2), (_D8, _GEOM)),
    (VAR8, dict(dtype=2, context_lengths=None), (_DTYPE8, _NULL)),
    (VAR8, dict(cu_seqlens_new=None, v_stride=(-256, 128)), (_NULL, _ALIGN)),
    (VAR8, dict(total_new=0, Hkv=0, dtype=-1), (_SIZES, _DTYPE8)),
    (ROPE, dict(q_stride=None, H=3), (_NULLST, _SIZES)),
    (ROPE, dict(H=3, layer_idx=2), (_SIZES, _GEOM)),
    (ROPE, dict(D=4, rot_dim=16), (_RD, _ROT)),         # a head_dim below the smallest rot_dim is never the only fault
    (ROPE, dict(D=0, rot_dim=16), (_RD, _ROT)),
    (ROPE, dict(rot_dim=24, max_position=0), (_ROT, _MAXPOS)),
    (ROPE, dict(interleaved=2, dtype=2), (_IL, _DTYPE)),
    (ROPE, dict(cos=None, sin=A + 8), (_TABNULL, _TABALIGN)),
    (ROPE, dict(max_position=0, q=None), (_MAXPOS, _NULL)),
    (ROPE, dict(q_out=None, positions=A + 2), (_NULL, _ALIGN)),
    (ROPE, dict(B=0, num_blocks=0, rot_dim=24), (_GEOM, _ROT)),
    (ROPE8, dict(k_stride=None, k_scale=None), (_NULLST, _SCALES)),
    (ROPE8, dict(v_scale=None, Hkv=0), (_SCALES, _SIZES)),
    (ROPE8, dict(D=8, rot_dim=16, interleaved=1), (_RD8, _ROT)),
    (ROPE8, dict(D=72, rot_dim=16), (_RD8, _ROT32)),
    (ROPE8, dict(rot_dim=48, max_position=0), (_ROT32, _MAXPOS)),
    (ROPE8, dict(dtype=2, cos=None), (_DTYPE, _TABNULL)),
    (ROPE8, dict(sin=A + 4, key=None), (_TABALIGN, _NULL)),
    (ROPE8, dict(k_cache=None, q=A + 8), (_NULL, _ALIGN)),
    (ROPE8, dict(total_new=0, block_size=0, max_position=-1), (_GEOM, _MAXPOS)),
]


def _call(fn, changes, refused):
    from mio import _lib
    a = dict(BASE[fn])
    assert set(changes) <= set(a), (fn, changes)
    a.update(changes)
    if not refused:  # only a call without work may be expected to return 0: nothing may be launched on the fake addresses
        assert fn in VARLEN and (a["B"] == 0 or a["total_new"] == 0), (fn, changes)
    args = [(C.c_int64 * 2)(*a[k]) if k.endswith("_stride") and a[k] is not None else a[k] for k in SIG[fn].split()]
    rc = getattr(_lib.lib, fn)(*args, None)
    return rc, _lib.lib.mio_last_error().decode()


def _id(v):
    if isinstance(v, dict):
        return ",".join(f"{k}={'x'.join(map(str, x)) if isinstance(x, tuple) else x}" for k, x in v.items()) or "base"
    return v[2:].replace(" ", "_")[:24] if isinstance(v, str) and v.startswith(": ") else None


def test_signatures_match_the_bound_symbols():
    from mio import _lib
    assert _lib.lib.mio_version() == 106
    for fn, sig in SIG.items():
        assert fn in _lib.EXPORTS and len(getattr(_lib.lib, fn).argtypes) == len(sig.split()) + 1, fn


@pytest.mark.parametrize("fn,changes,want", CASES, ids=_id)
def test_cache_write_single_fault_or_no_work(fn, changes, want):
    rc, err = _call(fn, changes, refused=want is not OK)
    if want is OK:
        assert rc == 0, (fn, changes, err)
    else:
        assert rc != 0 and err == fn + want, (fn, changes, rc, err)


@pytest.mark.parametrize("fn,changes,either", PAIRS, ids=_id)
def test_cache_write_doubly_wrong_is_refused(fn, changes, either):
    rc, err = _call(fn, changes, refused=True)
    assert rc != 0 and err in [fn + m for m in either], (fn, changes, rc, err)


@pytest.mark.parametrize("stride", ["k_stride", "v_stride"])
def test_single_token_null_stride_is_refused(stride):
    """The single intended difference between the forms' earlier checks and the shared plan: see the module docstring."""
    rc, err = _call(ONE, {stride: None}, refused=True)
    assert rc != 0 and err == ONE + _NULL


def test_every_message_of_every_form_is_reached():
    """The table covers each message a form can give (its launch failure aside)."""
    plain16, plain8 = {_NULL, _SIZES, _GEOM, _DTYPE, _ALIGN}, {_NULL, _SCALES, _SIZES, _D8, _GEOM, _DTYPE8, _ALIGN}
    rot = {_NULLST, _NULL, _SIZES, _GEOM, _ROT, _IL, _MAXPOS, _DTYPE, _TABNULL, _TABALIGN, _ALIGN, _MANY}
    want = {ONE: plain16, ONE8: plain8, VAR: plain16 | {_NULLST, _MANY}, VAR8: plain8 | {_NULLST, _MANY},
            ROPE: rot | {_RD}, ROPE8: rot | {_RD8, _ROT32, _SCALES}}
    for fn in SIG:
        assert {w for f, _, w in CASES if f == fn and w is not OK} == want[fn], fn

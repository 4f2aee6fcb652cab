"""The 16-bit attention prefill family in hostile memory (tests/_hostile.py): mio_fa3_fwd, mio_fa3_fwd_varlen,
mio_fa3_fwd_paged and their _window forms, every route, both storage dtypes.

Each case launches through the C ABI on operands embedded in guarded buffers (addresses asserted: no copy on the way),
asserts the route first, and is judged by _hostile.judge: the benign launch within the unchanged _attn_check bars of its
route against the fp64 reference of the owned inputs; the launches with every not-owned byte NaN, then huge, equal to it
bit for bit in every owned output; guards and inputs untouched after each.  The three launches of a case run in the same
device buffers at the same addresses.

The padding rows past B*Sq of the last 256-row block of a blocked output (fwd5_kpre_oblk) are not written: every output
store of csrc/fa3_fwd5_body.inc is predicated on the query row being < Sq.  They are held to their pre-fill.

One run on the MI355X: 137 tests (136 judgements and the statistics line) in 12.4 s, the slowest 0.4 s.  Worst statistic
over the file's _attn_check judgements per (dtype, family), against the unchanged bars (worst row / mean / 16-row group in
u, lse):
  bf16  fwd1 0.921 0.585 0.695 1.63e-7      fwd1_keep 0.861 0.590 0.671 1.69e-7     fwd1_add 1.091 0.556 0.635 1.69e-7
        fwd5 1.065 0.604 0.678 1.23e-3      fwd5_kpre 0.883 0.580 0.661 2.00e-4     fwd5_kpre_carry 0.910 0.570 0.628 2.31e-4
        fwd5_kpre_oblk 0.937 0.591 0.651 -  fwd3 1.119 0.596 0.672 1.13e-3          fwd3_kpre 0.890 0.579 0.627 2.19e-4
  fp16  fwd1 0.851 0.580 0.654 1.52e-7      fwd1_keep 0.879 0.589 0.646 1.48e-7     fwd1_add 1.088 0.553 0.627 1.75e-7
        fwd5 1.010 0.604 0.739 1.61e-4      fwd5_kpre 0.979 0.580 0.673 2.02e-5     fwd5_kpre_carry 1.039 0.571 0.643 2.72e-5
        fwd5_kpre_oblk 0.968 0.592 0.632 -  fwd3 0.996 0.595 0.664 1.21e-4          fwd3_kpre 0.887 0.581 0.626 2.33e-5
Before the tile range of a pass was clamped to the rows below Sq, window_dense_l64_r32_D64 failed under
the nan fill: o differed in 6144 elements, rows 288 .. 299 of every head, through the invisible tile 640 .. 703.
"""
import ctypes

import pytest
import torch

import _attn_check as ac
import _hostile as hs

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]


class GpuRun:
    """run(built, bufs) of _hostile.judge on the GPU: the buffers of a case live at fixed device addresses; every launch
    copies the given bytes in, launches once and copies every buffer back."""

    def __init__(self):
        self.dev = {}

    def __call__(self, built, bufs):
        from mio import _lib, ops
        for name, t in bufs.items():
            if name not in self.dev:
                self.dev[name] = t.to(DEV)
            else:
                self.dev[name].copy_(t)
        p, w, query, fwd, names, _keep = hs.params(built, self.dev)
        assert ops._route(query, p, w, names) == built.case.route, built.case.name
        _lib.check(fwd(ctypes.byref(p), w[0], w[1], torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return {name: t.cpu() for name, t in self.dev.items()}


def _cases(form, windowed=False):
    return [c.name for c in hs.CASES if c.form == form and c.windowed == windowed]


def _judge(name, dtype):
    case = next(c for c in hs.CASES if c.name == name)
    hs.judge(GpuRun(), hs.build(case, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", _cases("dense"))
def test_dense(name, dtype):
    """One or more cases per route (fwd1, fwd1_keep, fwd1_add, fwd5, fwd5_kpre, fwd5_kpre_carry with carry_in 0 and 1,
    fwd5_kpre_oblk, fwd3, fwd3_kpre): head dims that are no multiple of 16 or of the padded head dim, both layouts, causal
    offsets with whole trailing tiles invisible and rows that see nothing, embedded masks [B,1,Sq,Sk] and [B,1,1,Sk]."""
    _judge(name, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", _cases("varlen"))
def test_varlen(name, dtype):
    """Key lengths (200, 1, 0, 65, 300, 64) with differing query lengths, rows past cu_seqlens[-1], q / k / v in one
    fused buffer or three; judged once per sequence with every other sequence's rows poisoned."""
    _judge(name, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", _cases("paged"))
def test_paged(name, dtype):
    """hostile_cache at block sizes 64 / 128 / 256, layer 1 of 3, permuted pages, a shared first page, seqused_k shorter
    than the allocated pages, max_seqlen_k cutting the longest sequence, Lk = 0, Lq > Lk."""
    _judge(name, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", _cases("dense", True) + _cases("varlen", True) + _cases("paged", True))
def test_windowed(name, dtype):
    """Windows (0,0) (63,0) (64,0) (100,0) causal, (64,32) and (-1,100): whole leading (dense: also trailing) key tiles
    outside the union of a sequence's windows, the pages that hold only such tiles and their table entries poisoned."""
    _judge(name, dtype)


def test_zz_statistics():
    """Prints the worst statistic per (dtype, family) of this file's _attn_check judgements (run with -s)."""
    for (dtype, fam), rec in sorted(ac.STATS.items(), key=str):
        print(f"{str(dtype).split('.')[-1]:9s}{fam:17s} worst {rec['worst']:.3f} mean {rec['mean']:.3f} "
              f"group {rec['group']:.3f} lse {rec['lse']:.2e}  ({rec['n']} checks; bars {ac.BARS[(dtype, fam)]})")

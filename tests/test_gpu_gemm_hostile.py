"""The GEMM family in hostile memory (tests/_hostile_gemm.py): mio_gemm_bias_act, its blocked-weight forms, mio_gemm_ln_bw /
mio_gemm_rms_bw, the three fused-MLP forwards and the weight preparations, every route of mio_gemm_route_t, both storage dtypes.

Each case launches through the C ABI on operands embedded in guarded buffers (every pointer is its embedded view's), asserts
the route first, and is judged by _hostile_gemm.judge: the benign launch within the unchanged _gemm_check bars of its route
against the fp64 reference of the owned inputs; the launches with every not-owned byte NaN, then huge, equal to it bit for bit
in every owned output (y, stats_out, the prepared weights); guards and inputs untouched after each.  The three launches of a
case run in the same device buffers at the same addresses, and a blocked weight is prepared again under each fill from its
source in hostile memory (row stride K + 72, 256 guard rows).

The padding rows of a blocked y are not written (csrc/gemm8w_kernel.h predicates every output store on the row being < M) and
are held to their pre-fill; the rows past M of stats_out are written and compared bit for bit across the fills.

One run on the MI355X: 67 tests (66 judgements -- 21 GEMM, 6 fused-MLP and 6 preparation cases in bf16 and fp16 -- and the
statistics line) in 34.9 s, the slowest 1.8 s (a fused MLP at M 16484, d = I = 1024).  Every case passed on its first run: no
launch of the family lets a value it does not own into a stored result.  Worst statistic of the file's _gemm_check judgements
per (dtype, route), against the unchanged bars (not round-to-nearest share, worst row / mean / 16x16 fragment in u):
  bf16  t128 7.30e-04 0.551 0.429 0.608     t256 2.62e-05 0.454 0.426 0.684          p8w 1.71e-03 0.479 0.429 0.647
        p8w_res 1.47e-03 0.475 0.426 0.561  p8w_fold 1.06e-04 0.482 0.426 0.612      p8w_stats 6.01e-05 0.460 0.424 0.531
        glu_t128x64 0.00e+00 0.621 0.414 0.572   glu_t256x128 2.52e-04 0.522 0.424 0.754
        p8w_glu 1.34e-04 0.520 0.424 0.760  p8w_glu_fold 1.92e-04 0.588 0.424 0.754
  fp16  t128 7.81e-03 0.630 0.436 0.673     t256 2.22e-04 0.457 0.426 0.694          p8w 1.34e-02 0.514 0.428 0.736
        p8w_res 1.16e-02 0.561 0.424 0.577  p8w_fold 8.90e-04 0.474 0.427 0.617      p8w_stats 4.77e-04 0.459 0.424 0.541
        glu_t128x64 3.42e-04 0.646 0.415 0.723   glu_t256x128 1.82e-03 0.524 0.425 0.765
        p8w_glu 9.91e-04 0.521 0.424 0.839  p8w_glu_fold 1.46e-03 0.577 0.424 0.744
"""
import pytest
import torch

import _gemm_check as gc
import _hostile_gemm as hg

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]


class GpuRun:
    """run(built, bufs) of _hostile_gemm.judge on the GPU: the buffers of a case live at fixed device addresses; every launch
    copies the given bytes in, runs the case's launches once and copies every buffer back."""

    def __init__(self):
        self.dev = {}

    def __call__(self, built, bufs):
        for name, t in bufs.items():
            if name not in self.dev:
                self.dev[name] = t.to(DEV)
            else:
                self.dev[name].copy_(t)
        hg.launch(built, self.dev, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return {name: t.cpu() for name, t in self.dev.items()}


def _names(kind):
    return [c.name for c in hg.CASES if c.kind == kind]


def _judge(name, dtype):
    case = next(c for c in hg.CASES if c.name == name)
    try:
        hg.judge(GpuRun(), hg.build(case, dtype), device=DEV)
    finally:
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", _names("gemm"))
def test_gemm(name, dtype):
    """One or more cases per route: the zero-filled K tail against the columns past K (K 40, 4104), ragged M and N against
    guard rows and the elements around the biases, ldr > N, blocked x / residual / y with padding rows, the fold forms with a
    statistics buffer that holds a slot more than ln_slots (under mio_gemm_rms_bw the sum entries are poison too), the
    producer's statistics, a column-scale band that ends at a ragged N."""
    _judge(name, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", _names("mlp"))
def test_fused_mlp(name, dtype):
    """mio_fused_mlp_fwd, _fwd_bw and _glu_fwd_bw: a workspace pre-filled with the fill inside more of it, ragged M, the
    row-major and the blocked intermediate."""
    _judge(name, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", _names("prep"))
def test_preparations(name, dtype):
    """mio_weight_block, mio_weight_block_glu, mio_ln_fold_weight, mio_weight_quant_w8 from a source with ldw > K and guard
    rows, mio_ln_stats_reduce with padding rows and a spare slot: the prepared bytes identical under the three fills, the
    padding rows of a blocked weight zero (bit-equal to the permutation of the owned rows)."""
    _judge(name, dtype)


def test_zz_statistics():
    """Prints the worst statistic per (dtype, route) of this file's _gemm_check judgements (run with -s)."""
    print("\n" + gc.stats_table())

"""Module-layer checker shared by tests/test_module_check.py (CPU) and tests/test_gpu_module_rows.py (a plain helper module, not
a conftest; torch only, no function of the package is called here).

The module layer (mio/_nn.py, the modules of mio/kernels/attention/flash_attention.py and mio/kernels/mlp/fused_mlp.py,
mio/synthetic.py) decides whether K leaves its projection pre-scaled, whether the context is written blocked, whether a norm
is folded into the GEMMs on either side of it, and which cached weight copy a launch reads.  This file states what every such
route has to compute, row by row:

reference(): one sub-layer -- norm (LayerNorm / RMSNorm at the module's eps), fused or separate q / k / v projection, rotary,
query normalisation, keep mask or window, attention with GQA (the formula of _attn_check.reference), out-projection + residual;
or norm, fc1 (+ gate), tanh-GELU / erf-GELU / ReLU / SiLU / SwiGLU, fc2 + residual -- in fp64 without any rounding, from the
module's own 16-bit parameters and the 16-bit input rows, on `device` (torch's fp64 matmul shares nothing with the kernels).

model(): the same operation with fp64 arithmetic inside every operator, rounded to the storage dtype (directly from fp64, rn16)
exactly where the module layer stores a 16-bit tensor on that route.  The rounding points, and what makes each one:
  unfolded form
    * the norm output:        mio/_nn.py apply_norm -> ops.layernorm / ops.rmsnorm (one fp32 row kernel, one store);
    * the projection output:  mio/_nn.py linear / prenorm_linear -> ops.gemm_bias_act; with a pre-scaled K its columns are
                              multiplied by softmax_scale * log2(e) (the fp32 value of mio/_nn.py attention_plan) BEFORE that
                              single rounding (include/mio_hip.h, mio_gemm_bias_act_bw_cs: "in fp32 after bias / activation and
                              before the rounding to 16 bits");
    * rotary / normalize_query: flash_attention.py _AttentionBase._rotate (ops.apply_rotary, "in fp32, rounded once", in place)
                              and _context (F.normalize on the 16-bit q: the norm is a 16-bit tensor, then the quotient);
    * the attention weights:  P = exp(s - max) rounded to the dtype before the P.V product and summed as rounded, as
                              _decode_check.model does with p16 (the matrix-core kernels);
    * the context:            flash_attention.py _context -> ops.fa3_fwd's output (row-major or blocked: the same values);
    * the sub-layer output:   the out-projection / fc2 with the residual added in the epilogue before the store
                              (mio/_nn.py linear(residual=) / residual_linear);
    * the MLP intermediate:   fused_mlp.py forward -> ops.fused_mlp's workspace, or _forward_stream's h.
  folded form (the input is a ResidualStream: mio/_nn.py folded_linear -> ops.gemm_ln(ln_stats=))
    * no norm output exists;
    * the prepared weights are rounded as ops.ln_fold_weight / ops.rms_fold_weight document them (include/mio_hip.h,
      mio_ln_fold_weight: "w * gamma - mean_k(w * gamma) (rounded once), bias_out = bias + w beta"; mio_gemm_rms_bw: "the 16-bit
      rounding of w * gamma", bias unchanged), and the read-out computes rstd * acc + bias' with the row statistics taken from
      the ROUNDED stream rows (include/mio_hip.h: the producer writes "(sum, sum of squares) of the ROUNDED row").
      mio_ln_fold_weight additionally picks the rounding direction of a few elements per row so that the 16-bit row sums to
      zero; the model rounds plainly to nearest, which leaves it a little LOOSER than the kernel on streams with a mean
      (about 0.1 u at mean 0.3), never tighter;
    * everything behind the pre-activation value is the unfolded form.
  tensor-parallel form (model(tp=): mio/parallelism/tensor_parallel.py, judged by tests/_parallel_check.py)
    * the projections, the attention and the activation are those of the unfolded form: a rank computes its own heads /
      intermediate columns, and what it stores are column slices of what one device stores;
    * the out-projection / fc2 is tp partial products over the column slices of the stored context / intermediate
      (RowParallelLinear.forward: "_local.cached_linear(self._cast, x2[a:b], self.weight, bias, "none", ..., out=out2[a:b])" --
      one GEMM store per rank and row chunk), rank 0's carrying bias and residual ("add_here = (rank == 0)");
    * the partials are summed in the activation dtype ("torch.distributed.all_reduce(out2[a:b], group=group, async_op=True)"
      on the 16-bit out2): a store after each add, in rank order.  At tp = 2 the one add is order-free.
  A module whose compute dtype differs from its parameters' / input's (fp16 into a bf16 module) first rounds both to the compute
  dtype (mio/_nn.py CastCache.get, as_dtype); the model does the same, the reference reads the tensors as they are.

judge(): every output finite; then the per-row normwise error ||y - ref|| / ||ref|| in units of u (bf16 2^-8, fp16 2^-11) as
four statistics: the worst row, the mean over rows, the worst mean over one 256-row GEMM tile (the unit a tile-index or
ragged-tile fault corrupts) and the worst mean over one sequence (the unit an attention or blocked-context fault corrupts).  The
bars are the same statistics of model() on the same inputs times MARGINS, floored at FLOOR u -- _decode_check.MARGINS / FLOOR,
the project's figures for a kernel against an independent rounding model of this construction (3 / 1.5 / 2, 0.75 u; the tile
and the sequence statistic both take the 2).  They are never taken from the kernels and never set per case.
judge_stats(): a ResidualStream's stats[:, :M] against the fp64 sum and sum of squares of the stream's own dense() rows per
256-column slot, within the fp32 summation bound for 256 addends: 256 * 2^-24 * sum|x| per entry, and the same with x^2.

Sub-layers are judged on their actual input: the MLP's reference reads the stream the attention sub-layer really produced, so
each sub-layer's error stands alone; the chained case judges two blocks end to end, reference chain against kernel chain, with
the model chain as the yardstick.

CASES is the case table of tests/test_gpu_module_rows.py: per case the module, the shape (SHAPES: the smallest at which its
route fires, rows no multiple of 256), the route every GEMM / attention launch must take, and the number of norm launches (0:
folded).  tests/test_module_check.py confirms the shapes through the ops.*_ok queries and mio._nn.attention_plan, and that
they fail one 256-row tile below.  DEFECTS are the faults the CPU test plants into model() to show judge() refusing them.

Inputs (draw_params / draw_rows): norm weights 1 + 0.1 randn, norm and Linear biases 0.1 randn, rows 0.3 + randn (the mean
exercises the fold's centring).  Matrices are N(0, (g / sqrt(fan_in))^2) with g = GAIN per matrix, so that the scores have a
standard deviation of about 2.4 (the softmax depends on K: a wrong column scale shows) and the median over rows of
||branch|| / ||residual|| lies in [0.5, 2] (tests/test_module_check.py asserts it on the fp64 reference): a 2 u fault in the
branch is then not drowned by the residual.

Measured on the MI355X by one run of tests/test_gpu_module_rows.py (largest value per (dtype, family) over its judge() calls,
kernel / model, in u; "ratio" is the largest statistic / bar over the four statistics, 1.0 = at the bar; n = judge() calls.  A
stream case judges its two calls as <family>_out / _in, a block its sub-layers as <family>_attn / _mlp; block_chain is the
two-block chain against the reference chain):

  dtype    family                  |  kernel: worst   mean   tile    seq  |  model: worst   mean   tile    seq  | ratio   n
  bfloat16 block_chain             |           2.61  1.784   1.83   1.83  |          2.56  1.782   1.83   1.83  |  0.67   1
  bfloat16 block_chain_attn        |           1.63  1.075   1.10   1.10  |          1.65  1.072   1.10   1.10  |  0.67   2
  bfloat16 block_chain_mlp         |           0.66  0.569   0.58   0.57  |          0.66  0.572   0.58   0.58  |  0.67   2
  bfloat16 block_fold_attn         |           1.76  1.081   1.10   1.10  |          1.76  1.078   1.10   1.10  |  0.67   4
  bfloat16 block_fold_mlp          |           0.74  0.590   0.61   0.59  |          0.74  0.590   0.61   0.59  |  0.67   4
  bfloat16 block_no_fold_attn      |           1.93  1.094   1.11   1.11  |          1.93  1.092   1.11   1.11  |  0.67   1
  bfloat16 block_no_fold_mlp       |           0.66  0.567   0.58   0.57  |          0.66  0.567   0.58   0.57  |  0.67   1
  bfloat16 cross_block_fold_attn   |           1.43  0.878   0.90   0.90  |          1.44  0.874   0.89   0.89  |  0.67   1
  bfloat16 cross_block_fold_mlp    |           0.64  0.565   0.57   0.57  |          0.63  0.567   0.57   0.57  |  0.66   1
  bfloat16 layer_kpre              |           1.42  0.857   0.87   0.87  |          1.42  0.854   0.87   0.87  |  0.67   1
  bfloat16 layer_small             |           1.32  0.849   0.85   0.85  |          1.32  0.847   0.85   0.85  |  0.67   1
  bfloat16 mlp_blocked             |           0.83  0.673   0.68   0.68  |          0.83  0.673   0.68   0.68  |  0.67   6
  bfloat16 mlp_fold_in             |           0.62  0.538   0.54   0.54  |          0.63  0.539   0.54   0.54  |  0.67   6
  bfloat16 mlp_fold_out            |           0.76  0.615   0.63   0.62  |          0.78  0.618   0.64   0.62  |  0.67   6
  bfloat16 mlp_small               |           0.68  0.618   0.62   0.62  |          0.68  0.618   0.62   0.62  |  0.67   5
  bfloat16 self_kpre               |           1.35  0.847   0.86   0.86  |          1.36  0.844   0.86   0.86  |  0.67   1
  bfloat16 self_kpre_oblk          |           1.78  1.082   1.10   1.10  |          1.73  1.080   1.09   1.09  |  0.67   5
  bfloat16 self_plain_k            |           1.63  0.875   0.88   0.89  |          1.55  0.869   0.88   0.89  |  0.67   2
  bfloat16 self_small              |           1.91  1.329   1.34   1.33  |          1.84  1.327   1.34   1.33  |  0.68   6
  bfloat16 self_stream_in          |           1.32  0.823   0.84   0.84  |          1.30  0.828   0.84   0.84  |  0.66   1
  bfloat16 self_stream_out         |           1.65  1.079   1.09   1.09  |          1.65  1.076   1.09   1.09  |  0.67   1
  bfloat16 self_stream_plain_k_in  |           1.26  0.813   0.82   0.82  |          1.20  0.821   0.83   0.83  |  0.66   1
  bfloat16 self_stream_plain_k_out |           1.63  1.073   1.09   1.09  |          1.59  1.071   1.08   1.09  |  0.67   1
  float16  block_chain             |           2.55  1.767   1.80   1.81  |          2.83  1.766   1.80   1.81  |  0.67   1
  float16  block_chain_attn        |           1.70  1.076   1.09   1.09  |          1.69  1.074   1.09   1.09  |  0.67   2
  float16  block_chain_mlp         |           0.65  0.570   0.58   0.57  |          0.65  0.572   0.59   0.58  |  0.67   2
  float16  block_fold_attn         |           1.82  1.087   1.11   1.11  |          1.75  1.085   1.11   1.10  |  0.67   4
  float16  block_fold_mlp          |           0.71  0.589   0.60   0.59  |          0.71  0.589   0.60   0.59  |  0.67   4
  float16  block_no_fold_attn      |           1.81  1.074   1.10   1.09  |          1.81  1.072   1.09   1.09  |  0.67   1
  float16  block_no_fold_mlp       |           0.66  0.570   0.58   0.57  |          0.66  0.570   0.58   0.57  |  0.67   1
  float16  cross_block_fold_attn   |           1.29  0.873   0.89   0.89  |          1.31  0.871   0.88   0.88  |  0.67   1
  float16  cross_block_fold_mlp    |           0.65  0.570   0.57   0.57  |          0.66  0.571   0.58   0.58  |  0.66   1
  float16  layer_kpre              |           1.39  0.854   0.87   0.87  |          1.40  0.852   0.87   0.86  |  0.67   1
  float16  layer_small             |           1.26  0.851   0.86   0.85  |          1.26  0.850   0.86   0.85  |  0.67   1
  float16  mlp_blocked             |           0.82  0.677   0.68   0.68  |          0.82  0.677   0.68   0.68  |  0.67   6
  float16  mlp_fold_in             |           0.63  0.537   0.54   0.54  |          0.63  0.537   0.55   0.54  |  0.67   6
  float16  mlp_fold_out            |           0.74  0.610   0.63   0.62  |          0.75  0.613   0.64   0.62  |  0.67   6
  float16  mlp_small               |           0.68  0.615   0.62   0.62  |          0.67  0.615   0.62   0.62  |  0.67   5
  float16  self_kpre               |           1.33  0.850   0.86   0.86  |          1.33  0.848   0.86   0.86  |  0.67   1
  float16  self_kpre_oblk          |           1.71  1.099   1.11   1.11  |          1.75  1.098   1.11   1.12  |  0.67   4
  float16  self_plain_k            |           1.38  0.872   0.88   0.89  |          1.33  0.867   0.88   0.88  |  0.67   2
  float16  self_small              |           1.56  1.046   1.06   1.05  |          1.54  1.044   1.06   1.05  |  0.68   5
  float16  self_stream_in          |           1.29  0.822   0.85   0.84  |          1.20  0.824   0.85   0.84  |  0.67   1
  float16  self_stream_out         |           1.78  1.076   1.10   1.09  |          1.77  1.075   1.10   1.09  |  0.67   1
  float16  self_stream_plain_k_in  |           1.17  0.820   0.83   0.83  |          1.14  0.825   0.84   0.83  |  0.66   1
  float16  self_stream_plain_k_out |           1.65  1.078   1.09   1.09  |          1.67  1.076   1.09   1.09  |  0.67   1

  (76 tests in 13.4 s of wall time, the slowest 1.2 s -- the first launch of the process -- and every other under 0.5 s; nearly
  all of it is drawing the inputs on the CPU and the fp64 reference and model on the GPU.)
  Every route lands on its model to within a few hundredths of a u in the mean, the tile and the sequence statistic, in both
  dtypes: the module layer's planned routes add nothing to what their rounding points cost.  The bar that comes closest is the
  mean (1.5 x the model's): the largest statistic-to-bar ratio measured is 0.68.  No family comes near a margin, so MARGINS
  stands as taken from _decode_check, none widened.  Every ResidualStream's statistics passed the fp32 summation bound.
  Not measured here: the tensor- and sequence-parallel wrappers (tests/_parallel_check.py has their table) and the paged decode
  path through the modules.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional

import torch

U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
_P = {torch.bfloat16: 8, torch.float16: 11}
_EMIN = {torch.bfloat16: -126, torch.float16: -14}
BF, FP = torch.bfloat16, torch.float16
TILE = 256                      # rows of a GEMM tile / of a block of the blocked activation layout
SLOT = 256                      # columns per statistics slot of a ResidualStream
LOG2E = 1.4426950408889634
NEG_FILL = -1e9                 # keep-masked scores (ops.flash_attention)
ADD_MASK_FLOOR = -1e30          # additive-mask entries below count as this (_attn_check.ADD_MASK_FLOOR)
MARGINS = {"worst": 3.0, "mean": 1.5, "tile": 2.0, "seq": 2.0}   # _decode_check.MARGINS; tile and seq take its 2
FLOOR = 0.75                                                      # _decode_check.FLOOR
OLD_BAR = 3e-3                  # the whole-tensor bar of tests/test_gpu_modules.py (bf16 routes)

STATS: dict = {}


# ---- rounding ------------------------------------------------------------------------------------------------------------------
def ulp16(v: torch.Tensor, dtype) -> torch.Tensor:
    """Spacing of the 16-bit grid of `dtype` at the fp64 values v (subnormal spacing below the smallest normal)."""
    a = v.abs()
    _, e = torch.frexp(a)
    e = torch.where(a > 0, e - 1, torch.full_like(e, _EMIN[dtype])).clamp_min(_EMIN[dtype])
    return torch.bitwise_left_shift((e - (_P[dtype] - 1) + 1023).to(torch.int64), 52).view(torch.float64)


def rn16(v: torch.Tensor, dtype) -> torch.Tensor:
    """Round-to-nearest-even of fp64 values onto the 16-bit grid, directly (no double rounding through fp32); fp64 out."""
    q = ulp16(v, dtype)
    return torch.round(v / q) * q


class _Arith:
    """fp64 arithmetic on one device; r() is the store into a 16-bit tensor (identity for the reference)."""

    def __init__(self, dtype, device):
        self.dtype, self.dev = dtype, torch.device("cpu" if device is None else device)

    def f(self, t):
        return None if t is None else t.detach().to(self.dev, torch.float64)

    def r(self, t):
        return t if (self.dtype is None or t is None) else rn16(t, self.dtype)

    def load(self, t):
        """A parameter or input as the module's kernels read it: cast to the compute dtype (a no-op where it already is)."""
        return self.r(self.f(t))


# ---- operators -----------------------------------------------------------------------------------------------------------------
def _act(z, act):
    if act == "gelu":
        return 0.5 * z * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (z + 0.044715 * z ** 3)))
    if act == "gelu_erf":
        return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))
    if act == "relu":
        return torch.relu(z)
    if act == "silu":
        return z * torch.sigmoid(z)
    raise ValueError(act)


def norm_eps(kind: str, eps: Optional[float], dtype) -> float:
    """The eps a norm module runs at: its own, or for an RMSNorm with eps=None torch.finfo(activation dtype).eps."""
    if eps is not None:
        return float(eps)
    if kind == "layernorm":
        return 1e-5
    return float(torch.finfo(dtype).eps)


def _norm_rows(x, n):
    """x [M, d] -> norm(x) in fp64 (unrounded); n = dict(kind, weight, bias, eps) in fp64."""
    if n["kind"] == "rms":
        return x * (x.square().mean(-1, keepdim=True) + n["eps"]) ** -0.5 * n["weight"]
    mu = x.mean(-1, keepdim=True)
    var = (x - mu).square().mean(-1, keepdim=True)
    return (x - mu) * (var + n["eps"]) ** -0.5 * n["weight"] + n["bias"]


def _tail0(M: int) -> int:
    """First row of the last (ragged) 256-row tile."""
    return (M - 1) // TILE * TILE


def _pre(A, x, lins, n, fold, defect=None):
    """Pre-activation values [M, N] (fp64, unrounded) of each (weight, bias) of `lins` applied to norm(x), x [M, d] the rounded
    input rows.  fold: the norm sits in the GEMM's read-out (module docstring, folded form)."""
    if n is None:
        return [x @ w.t() + b for w, b in lins]
    if not fold:
        xn = A.r(_norm_rows(x, n))                              # apply_norm: the norm output is stored
        return [xn @ w.t() + b for w, b in lins]
    g = n["weight"]
    if defect == "stale_gamma":                                 # the fold was made when gamma still had its initial value
        g = torch.ones_like(g)
    sq = x.square().mean(-1, keepdim=True)
    if n["kind"] == "rms":
        r = (sq + n["eps"]) ** -0.5
    else:
        mu = x.mean(-1, keepdim=True)
        r = ((sq - mu * mu).clamp_min(0.0) + n["eps"]) ** -0.5
    if defect == "stats_shift":                                 # the rows of tile 1 read the statistics of row + 1
        r = torch.cat([r[:TILE], r[TILE + 1:2 * TILE + 1], r[2 * TILE:]])
    out = []
    for w, b in lins:
        if n["kind"] == "rms":
            wf, bf = A.r(w * g), b                              # ops.rms_fold_weight
        else:
            ws = w * g
            wf = A.r(ws - ws.mean(1, keepdim=True))             # ops.ln_fold_weight: scaled, centred, rounded once
            bf = b if defect == "beta_unfolded" else A.r(b + w @ n["bias"])
        out.append(r * (x @ wf.t()) + bf)
    return out


def _add_residual(z, res, defect=None):
    if res is None:
        return z
    M = z.shape[0]
    if defect == "neighbour_residual":                          # one row of the last ragged tile takes its neighbour's
        res = res.clone()
        res[M - 2] = res[M - 1]
    elif defect == "tail_no_residual":                          # the last partial tile's rows lose the residual
        res = res.clone()
        res[_tail0(M):] = 0.0
    return z + res


def _row_parallel(A, h, w, b, res, tp=1, defect=None):
    """The out-projection / fc2 of the stored context / intermediate h [M, K]: (stored output, unrounded branch).  tp = 1: one
    GEMM with bias and residual in its epilogue, one store.  tp > 1: the tensor-parallel form (module docstring): tp partial
    products over the column slices of h, rank 0's with bias and residual, each stored, then summed in rank order with a store
    after each add."""
    branch = h @ w.t() + b
    if tp == 1:
        return A.r(_add_residual(branch, res, defect)), branch
    M, K = h.shape
    per = K // tp
    parts = []
    for r in range(tp):
        part = h[:, r * per:(r + 1) * per] @ w[:, r * per:(r + 1) * per].t()
        if r == 0 or defect == "tp_bias_every_rank":
            part = part + b
        if res is not None and (r == 0 or defect == "tp_residual_every_rank"):
            part = part + res
        parts.append(A.r(part))                                 # RowParallelLinear.forward: the chunk GEMM's store
    total = parts[0]
    for part in parts[1:]:
        total = A.r(total + part)                               # the all-reduce in the activation dtype
    if defect == "tp_chunk_unreduced":                          # the last of TP_DEFECT_CHUNKS row chunks never met its all-reduce
        total = total.clone()
        a = (TP_DEFECT_CHUNKS - 1) * M // TP_DEFECT_CHUNKS
        total[a:] = parts[0][a:]
    return total, branch


def _rotate(A, t, rot, base, interleaved=False):
    """t [B, S, h, D]: the first rot elements of every head rotated at positions 0 .. S-1 (neox pairing), stored in place."""
    S = t.shape[1]
    inv = float(base) ** (-torch.arange(0, rot, 2, dtype=torch.float64, device=t.device) / rot)
    ang = torch.arange(S, dtype=torch.float64, device=t.device)[:, None] * inv[None, :]
    c, s = ang.cos()[None, :, None, :], ang.sin()[None, :, None, :]
    if interleaved:
        x1, x2 = t[..., 0:rot:2], t[..., 1:rot:2]
    else:
        x1, x2 = t[..., :rot // 2], t[..., rot // 2:rot]
    y1, y2 = x1 * c - x2 * s, x2 * c + x1 * s
    out = t.clone()
    if interleaved:
        out[..., 0:rot:2], out[..., 1:rot:2] = y1, y2
    else:
        out[..., :rot // 2], out[..., rot // 2:rot] = y1, y2
    return A.r(out)


def _attention(A, q, k, v, scale_nat, causal, keep=None, window=None, chunk=8, additive=None):
    """q [B,Sq,H,D], k / v [B,Sk,Hkv,D] fp64 -> context [B,Sq,H,D] (unrounded): softmax(q k^T * scale_nat) v with GQA, the mask
    conventions of _attn_check.reference (causal-excluded keys absent, or at -1e9 next to a keep mask; keep-masked keys at -1e9;
    keys outside a window absent; additive [B,1|H,Sq,Sk] entries floored at -1e30); the model rounds P = exp(s - max) to the
    dtype and sums it as rounded."""
    B, Sq, H, D = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    qi = torch.arange(Sq, device=q.device)[:, None]
    ki = torch.arange(Sk, device=q.device)[None, :]
    out = torch.empty_like(q)
    for b0 in range(0, B, chunk):
        b1 = min(b0 + chunk, B)
        kk = k[b0:b1].repeat_interleave(H // Hkv, dim=2)
        vv = v[b0:b1].repeat_interleave(H // Hkv, dim=2)
        s = torch.einsum("bshd,bkhd->bhsk", q[b0:b1], kk) * scale_nat
        if causal:
            s = s.masked_fill((ki > qi)[None, None], NEG_FILL if keep is not None else float("-inf"))
        if window is not None:
            left, right = window
            gone = torch.zeros(Sq, Sk, dtype=torch.bool, device=q.device)
            if left >= 0:
                gone |= ki < qi - left
            if right >= 0:
                gone |= ki > qi + right
            s = s.masked_fill(gone[None, None], float("-inf"))
        if keep is not None:
            kp = keep[b0:b1].to(q.device) != 0
            s = torch.where(kp[:, None, None, :], s, torch.full_like(s, NEG_FILL))
        if additive is not None:
            s = s + additive[b0:b1].to(q.device, torch.float64).clamp_min(ADD_MASK_FLOOR)
        p = A.r(torch.exp(s - s.amax(dim=-1, keepdim=True)))
        out[b0:b1] = torch.einsum("bhsk,bkhd->bshd", p, vv) / p.sum(-1).permute(0, 2, 1)[..., None]
    return out


def _sublayer(A, spec, P, x, norm=None, fold=False, residual=True, context=None, keep=None, defect=None, tp=1):
    """One sub-layer on x [B, S, d]: (out [B, S, d], branch [B, S, d]) in fp64; A decides what is rounded.  tp: the tensor-parallel
    degree of the out-projection / fc2 (_row_parallel)."""
    B, S, d = x.shape
    M = B * S
    x2 = A.load(x).reshape(M, d)
    res = x2 if residual else None
    n = None
    if norm is not None:
        n = dict(kind=norm["kind"], eps=norm["eps"], weight=A.load(norm["weight"]),
                 bias=A.load(norm.get("bias")) if norm["kind"] == "layernorm" else None)
    W = {k_: A.load(t) for k_, t in P.items()}
    lin = lambda name: (W[name + ".weight"], W[name + ".bias"])  # noqa: E731
    if spec["op"] == "mlp":
        act = spec["act"]
        if act == "swiglu":
            zu, zg = _pre(A, x2, [lin("fc1"), lin("fc1_gate")], n, fold, defect)
            if defect == "gate_up_swap":                        # one 128-column group of the interleaved tile
                zu, zg = zu.clone(), zg.clone()
                zu[:, 128:256], zg[:, 128:256] = zg[:, 128:256].clone(), zu[:, 128:256].clone()
            h = zg * torch.sigmoid(zg) * zu
        else:
            h = _act(_pre(A, x2, [lin("fc1")], n, fold, defect)[0], act)
        h = A.r(h)                                              # the intermediate is stored
        w2, b2 = lin("fc2")
        out, branch = _row_parallel(A, h, w2, b2, res, tp, defect)
        return out.view(B, S, d), branch.view(B, S, d)
    H, Hkv, D = spec["H"], spec["Hkv"], d // spec["H"]
    kvd = Hkv * D
    scale = spec.get("scale") or 1.0 / math.sqrt(D)
    cs = float(torch.tensor(scale * LOG2E, dtype=torch.float32)) if spec.get("kpre") else None
    kind = spec["kind"]
    if kind == "self":
        z = _pre(A, x2, [lin("qkv_proj")], n, fold, defect)[0]
        if cs is not None:
            z = z.clone()
            hi = d + kvd - (128 if defect == "kscale_short" else 0)   # the scale stops 128 columns early
            z[:, d:hi] *= cs
        z = A.r(z)
        q, k, v = z[:, :d], z[:, d:d + kvd], z[:, d + kvd:]
        if defect == "tp_k_from_rank0":                         # every rank's attention reads rank 0's K columns
            per = kvd // tp
            k = torch.cat([k[:, :per]] * tp, dim=1)
        Sk, Bk = S, B
    else:
        q = A.r(_pre(A, x2, [lin("q_proj")], n, fold, defect)[0])
        xkv = x2 if kind == "layer" else A.load(context).reshape(-1, d)
        if kind == "layer" and n is not None:
            raise ValueError("FlashAttentionLayer takes no pre_norm")
        zk = xkv @ W["k_proj.weight"].t() + W["k_proj.bias"]
        if cs is not None:
            zk = zk.clone()
            zk[:, :kvd - (128 if defect == "kscale_short" else 0)] *= cs
        k, v = A.r(zk), A.r(xkv @ W["v_proj.weight"].t() + W["v_proj.bias"])
        Bk = B
        Sk = xkv.shape[0] // B
    q, k, v = q.reshape(B, S, H, D), k.reshape(Bk, Sk, Hkv, D), v.reshape(Bk, Sk, Hkv, D)
    if spec.get("rotary"):
        q = _rotate(A, q, spec["rotary"], spec.get("rotary_base", 10000.0))
        k = _rotate(A, k, spec["rotary"], spec.get("rotary_base", 10000.0))
    if spec.get("normq"):
        # F.normalize on the 16-bit q is q / max(||q||, eps) with ||q|| itself a 16-bit tensor: two stores
        q = A.r(q / A.r(q.norm(dim=-1, keepdim=True)).clamp_min(1e-12))
    ctx = _attention(A, q, k, v, (1.0 / LOG2E) if cs is not None else scale, spec.get("causal", False), keep,
                     spec.get("window"))
    if defect == "head_shift":                                  # one sequence: two neighbouring heads' columns exchanged
        ctx = ctx.clone()
        h0 = H // 2
        ctx[1, :, h0], ctx[1, :, h0 + 1] = ctx[1, :, h0 + 1].clone(), ctx[1, :, h0].clone()
    ctx = A.r(ctx).reshape(M, d)                                # the context is stored
    wo, bo = lin("out_proj" if kind == "cross" else "o_proj")
    out, branch = _row_parallel(A, ctx, wo, bo, res, tp, defect)
    return out.view(B, S, d), branch.view(B, S, d)


def reference(spec, P, x, *, norm=None, residual=True, context=None, keep=None, device=None, parts=False, tp=1):
    """fp64 [B, S, d] of one sub-layer (module docstring), nothing rounded; parts: (out, branch) -- the branch is what the
    sub-layer adds to its residual."""
    out, branch = _sublayer(_Arith(None, device), spec, P, x, norm, False, residual, context, keep, None, tp)
    return (out, branch) if parts else out


def model(spec, P, x, *, dtype, norm=None, fold=False, residual=True, context=None, keep=None, device=None, defect=None,
          tp: int = 1):
    """The rounding model of one sub-layer at compute dtype `dtype`: fp64 values on the 16-bit grid, [B, S, d].  fold: the
    folded form (the input is a ResidualStream).  defect: one of DEFECTS (or, with tp > 1, of TP_DEFECTS), planted.  tp: the
    sub-layer as TensorParallelAttention / TensorParallelMLP run it over tp ranks (module docstring)."""
    if defect is not None and defect not in DEFECTS and not (tp > 1 and defect in TP_DEFECTS):
        raise ValueError(defect)
    return _sublayer(_Arith(dtype, device), spec, P, x, norm, fold, residual, context, keep, defect, tp)[0]


# ---- judging -------------------------------------------------------------------------------------------------------------------
def row_errors(y, ref):
    """Per-row ||y - ref|| / ||ref|| over the last dim, rows flattened: fp64 [M] on ref's device."""
    d = ref.shape[-1]
    r = ref.reshape(-1, d)
    e = y.detach().to(r.device, torch.float64).reshape(-1, d) - r
    rn = r.norm(dim=-1)
    return e.norm(dim=-1) / torch.where(rn > 0, rn, torch.ones_like(rn))


def _group_max(e, size):
    """Worst mean of e over consecutive groups of `size` rows (the last one may be shorter)."""
    M = e.numel()
    pad = (-M) % size
    s = torch.nn.functional.pad(e, (0, pad)).view(-1, size).sum(-1)
    n = torch.full_like(s, float(size))
    if pad:
        n[-1] = size - pad
    return (s / n).max().item()


def measure(y, ref, dtype, S: int) -> dict:
    """dict(worst, mean, tile, seq) in units of u; S = rows per sequence."""
    e = row_errors(y, ref) / U[dtype]
    return {"worst": e.max().item(), "mean": e.mean().item(), "tile": _group_max(e, TILE), "seq": _group_max(e, S)}


def bars(model_y, ref, dtype, S: int):
    ms = measure(model_y, ref, dtype, S)
    return {k: max(MARGINS[k] * ms[k], FLOOR) for k in MARGINS}, ms


def judge(y, ref, model_y, dtype, S: int, family: str, what: str = "", record: bool = True) -> dict:
    """Assert the module output y ([B, S, d] or [M, d], 16-bit) against the fp64 reference within the bars taken from model_y
    (model() on the same inputs); dtype is the compute dtype whose u the error is counted in.  Returns the statistics."""
    tag = f"{what} [{family} {str(dtype).split('.')[-1]}]"
    assert y.numel() == ref.numel(), f"{tag}: {tuple(y.shape)} vs {tuple(ref.shape)}"
    bad = ~torch.isfinite(y.detach().float())
    assert not bad.any(), f"{tag}: non-finite output ({int(bad.sum())} values)"
    st = measure(y, ref, dtype, S)
    bar, ms = bars(model_y, ref, dtype, S)
    if record:
        rec = STATS.setdefault((dtype, family), {"n": 0, "ratio": 0.0, **{k: 0.0 for k in MARGINS},
                                                 **{"model_" + k: 0.0 for k in MARGINS}})
        rec["n"] += 1
        for k in MARGINS:
            rec[k] = max(rec[k], st[k])
            rec["model_" + k] = max(rec["model_" + k], ms[k])
            rec["ratio"] = max(rec["ratio"], st[k] / bar[k])
    if not all(st[k] <= bar[k] for k in MARGINS):
        e = row_errors(y, ref) / U[dtype]
        at = int(e.argmax())
        raise AssertionError(
            f"{tag}: worst row {st['worst']:.2f} u (bar {bar['worst']:.2f}, model {ms['worst']:.2f}) at row {at} (sequence "
            f"{at // S}, tile {at // TILE}); mean {st['mean']:.3f} u (bar {bar['mean']:.3f}, model {ms['mean']:.3f}); worst "
            f"tile mean {st['tile']:.2f} u (bar {bar['tile']:.2f}, model {ms['tile']:.2f}); worst sequence mean "
            f"{st['seq']:.2f} u (bar {bar['seq']:.2f}, model {ms['seq']:.2f})")
    return st


def judge_stats(stats, rows, what: str = "") -> None:
    """A ResidualStream's stats[:, :M] ([d / 256, M, 2] fp32) against the fp64 (sum, sum of squares) of its own dense rows
    ([M, d] or [B, S, d], 16-bit) per 256-column slot, within 256 * 2^-24 * sum|x| (and the same with x^2)."""
    d = rows.shape[-1]
    x = rows.detach().to(torch.float64).reshape(-1, d // SLOT, SLOT)
    M = x.shape[0]
    assert tuple(stats.shape) == (d // SLOT, M, 2), f"{what}: statistics of shape {tuple(stats.shape)}"
    st = stats.detach().to(x.device, torch.float64)
    assert bool(torch.isfinite(st).all()), f"{what}: non-finite row statistics"
    c = SLOT * 2.0 ** -24
    for j, (want, mag) in enumerate(((x.sum(-1), x.abs().sum(-1)), (x.square().sum(-1), x.square().sum(-1)))):
        err = (st[..., j] - want.t()).abs()
        over = err > c * mag.t()
        if bool(over.any()):
            s_, m_ = (int(i) for i in over.nonzero()[0])
            raise AssertionError(f"{what}: {int(over.sum())} row statistics ({('sum', 'sum of squares')[j]}) outside the fp32 "
                                 f"summation bound; first at slot {s_} row {m_}: {st[s_, m_, j].item():.9g} vs "
                                 f"{want[m_, s_].item():.9g} (bound {c * mag[m_, s_].item():.3g})")


def old_aggregate(y, ref):
    """What tests/test_gpu_modules.py computes: ((y - ref).abs().mean() / ref.abs().mean(), passes the 3e-3 bar)."""
    r = ref.reshape(-1)
    rel = ((y.detach().to(r.device, torch.float64).reshape(-1) - r).abs().mean() / r.abs().mean()).item()
    return rel, rel < OLD_BAR


def branch_ratio(out_branch, residual) -> float:
    """Median over rows of ||branch|| / ||residual||."""
    d = residual.shape[-1]
    return (out_branch.reshape(-1, d).norm(dim=-1) / residual.double().reshape(-1, d).to(out_branch.device).norm(dim=-1)
            ).median().item()


def stats_table() -> str:
    """STATS as the lines of the module docstring's table."""
    lines = ["dtype    family                  |  kernel: worst   mean   tile    seq  |  model: worst   mean   tile    seq  | ratio   n"]
    for key in sorted(STATS, key=str):
        dt, fam = key
        r = STATS[key]
        lines.append(f"{str(dt).split('.')[-1]:8s} {fam:23s} |        {r['worst']:6.2f} {r['mean']:6.3f} {r['tile']:6.2f} "
                     f"{r['seq']:6.2f}  |       {r['model_worst']:6.2f} {r['model_mean']:6.3f} {r['model_tile']:6.2f} "
                     f"{r['model_seq']:6.2f}  | {r['ratio']:5.2f} {r['n']:3d}")
    return "\n".join(lines)


# ---- inputs --------------------------------------------------------------------------------------------------------------------
# standard deviation of a matrix = GAIN / sqrt(fan_in) (module docstring, "Inputs")
GAIN = {"qkv_proj": 1.5, "q_proj": 1.5, "k_proj": 1.5, "v_proj": 1.5, "o_proj": 1.5, "out_proj": 1.5,
        "fc1": 1.0, "fc1_gate": 1.0, "fc2": 1.7}


def linears(spec, d: int) -> Dict[str, tuple]:
    """name -> (out_features, in_features) of a sub-layer's Linear modules."""
    if spec["op"] == "mlp":
        I = spec["I"]
        out = {"fc1": (I, d), "fc2": (d, I)}
        if spec["act"] == "swiglu":
            out["fc1_gate"] = (I, d)
        return out
    kvd = spec["Hkv"] * (d // spec["H"])
    if spec["kind"] == "self":
        return {"qkv_proj": (d + 2 * kvd, d), "o_proj": (d, d)}
    o = "out_proj" if spec["kind"] == "cross" else "o_proj"
    return {"q_proj": (d, d), "k_proj": (kvd, d), "v_proj": (kvd, d), o: (d, d)}


def draw_params(spec, d: int, gen, dtype) -> Dict[str, torch.Tensor]:
    """The sub-layer's parameters on the CPU in dtype, under the names of the module's own Linear children."""
    P = {}
    for name, (n_out, n_in) in linears(spec, d).items():
        P[name + ".weight"] = (torch.randn(n_out, n_in, generator=gen) * (GAIN[name] / math.sqrt(n_in))).to(dtype)
        P[name + ".bias"] = (torch.randn(n_out, generator=gen) * 0.1).to(dtype)
    return P


def draw_norm(kind: str, d: int, gen, dtype, eps: Optional[float] = None) -> dict:
    n = {"kind": kind, "eps": norm_eps(kind, eps, dtype), "weight": (1.0 + 0.1 * torch.randn(d, generator=gen)).to(dtype)}
    if kind == "layernorm":
        n["bias"] = (0.1 * torch.randn(d, generator=gen)).to(dtype)
    return n


def draw_rows(B: int, S: int, d: int, gen, dtype) -> torch.Tensor:
    return (0.3 + torch.randn(B, S, d, generator=gen)).to(dtype)


def keep_mask(B: int, S: int) -> torch.Tensor:
    """[B, S] keep mask: the last 37 keys of sequence 1 are masked."""
    keep = torch.ones(B, S)
    keep[1, S - 37:] = 0
    return keep


# ---- the faults planted into model() by tests/test_module_check.py ---------------------------------------------------------------
DEFECTS = {
    "neighbour_residual": "a row of the last ragged tile takes its neighbour's residual",
    "tail_no_residual": "the last partial tile's rows lose the residual",
    "kscale_short": "the K column scale stops 128 columns early",
    "stats_shift": "the rows of one tile read the statistics of row + 1",
    "beta_unfolded": "beta is not folded into the bias",
    "gate_up_swap": "gate and up are swapped in one 128-column group",
    "head_shift": "one head's context lands in the neighbouring head's columns for one sequence",
    "stale_gamma": "a folded weight is built from a stale gamma",
}


# the faults tests/test_parallel_check.py plants into model(tp=2)
TP_DEFECT_CHUNKS = 3            # RowParallelLinear's row chunks in the tp_chunk_unreduced fault (overlap_chunks = 3)
TP_DEFECTS = {
    "tp_bias_every_rank": "every rank adds the out-projection / fc2 bias to its partial",
    "tp_residual_every_rank": "every rank adds the residual to its partial",
    "tp_chunk_unreduced": "the last RowParallelLinear row chunk holds rank 0's partial only",
    "tp_k_from_rank0": "rank 1's attention reads rank 0's K columns of the fused projection",
}


# ---- the case table ------------------------------------------------------------------------------------------------------------
# (d, H, B, S): the smallest shapes whose routes fire (csrc/gemm_route.h: the persistent kernel needs >= 256 tiles of 256 x 256;
# csrc/fa3_api.hip: a pre-scaled K needs Sq > 128), rows no multiple of 256, sequence boundaries off the 256-row tiles
SHAPES = {
    "hd64": (1024, 16, 63, 257),     # 16 191 rows: 64 row tiles x 4 column tiles
    "hd80": (1280, 16, 51, 257),     # 13 107 rows: 52 x 5
    "hd128": (2048, 16, 31, 257),    # 7 967 rows: 32 x 8
    "short": (1024, 16, 127, 128),   # 16 256 rows, Sq <= 128
    "small": (1024, 16, 2, 300),     # 600 rows: T128 GEMMs, row-kernel norms
}
MLP_I = 1024                         # the smallest I at which both MLP stages fill the chip at d = 1024
BOTH = (BF, FP)

P8W_KPRE_OBLK = ("gemm:p8w+cs", "attn:kpre+oblk", "gemm:p8w_res")


def attn_spec(kind="self", H=16, Hkv=None, causal=True, kpre=False, **kw):
    return dict(op="attn", kind=kind, H=H, Hkv=H if Hkv is None else Hkv, causal=causal, kpre=kpre, **kw)


def mlp_spec(act="gelu", I=MLP_I):
    return dict(op="mlp", act=act, I=I)


def _case(name, module, shape, family, routes, norms, dtypes=BOTH, **kw):
    """routes: what every launch with a route must be, in order -- "gemm:<route>" (+cs: with a column scale),
    "mlp:<path>/<stage1>/<stage2>", "attn:plain" / "attn:kpre" / "attn:kpre+oblk"; norms: norm kernel launches."""
    return dict(name=name, module=module, shape=shape, family=family, routes=tuple(routes), norms=norms, dtypes=dtypes, **kw)


def _small_self(name, **spec_kw):
    return _case(name, "self", "small", "self_small", ("gemm:t128", "attn:plain", "gemm:t128"), 0,
                 spec=attn_spec(**spec_kw), norm=None, stream=None)


_STREAM_SELF = ("gemm:p8w+cs", "attn:kpre+oblk", "gemm:p8w_stats", "gemm:p8w_fold+cs", "attn:kpre+oblk", "gemm:p8w_res")
_MLP_BLOCKED = {"gelu": ("mlp:blocked/p8w/p8w_res",), "swiglu": ("mlp:blocked/p8w_glu/p8w_res",)}
_MLP_FOLD = {"gelu": "gemm:p8w_fold", "swiglu": "gemm:p8w_glu_fold"}

CASES: List[dict] = [
    # FlashSelfAttention, head dim 64: pre-scaled K, blocked context
    _case("self_hd64_plain", "self", "hd64", "self_kpre_oblk", P8W_KPRE_OBLK, 0, spec=attn_spec(kpre=True), norm=None, stream=None),
    _case("self_hd64_prenorm_ln", "self", "hd64", "self_kpre_oblk", P8W_KPRE_OBLK, 1, spec=attn_spec(kpre=True),
          norm="layernorm", stream=None),
    _case("self_hd64_prenorm_rms", "self", "hd64", "self_kpre_oblk", P8W_KPRE_OBLK, 1, spec=attn_spec(kpre=True), norm="rms",
          stream=None),
    _case("self_hd64_stream_out_in", "self", "hd64", "self_stream", _STREAM_SELF, 1, spec=attn_spec(kpre=True),
          norm="layernorm", stream="out_in"),
    _case("self_hd64_kv4", "self", "hd64", "self_kpre_oblk", P8W_KPRE_OBLK, 0, spec=attn_spec(Hkv=4, kpre=True), norm=None,
          stream=None),
    _case("self_hd64_kv1", "self", "hd64", "self_plain_k", ("gemm:p8w", "attn:plain", "gemm:p8w_res"), 0,
          spec=attn_spec(Hkv=1), norm=None, stream=None),
    _case("self_hd64_noncausal", "self", "hd64", "self_kpre_oblk", P8W_KPRE_OBLK, 0, spec=attn_spec(causal=False, kpre=True),
          norm=None, stream=None, dtypes=(BF,)),
    # head dim 80: pre-scaled K, row-major context
    _case("self_hd80_plain", "self", "hd80", "self_kpre", ("gemm:p8w+cs", "attn:kpre", "gemm:p8w_res"), 0,
          spec=attn_spec(kpre=True), norm=None, stream=None),
    # head dim 128: plain K, both folds
    _case("self_hd128_stream_out_in", "self", "hd128", "self_stream_plain_k",
          ("gemm:p8w", "attn:plain", "gemm:p8w_stats", "gemm:p8w_fold", "attn:plain", "gemm:p8w_res"), 1, spec=attn_spec(),
          norm="layernorm", stream="out_in"),
    # column-scale shape, but Sq <= 128: the plan must say no
    _case("self_short_plain", "self", "short", "self_plain_k", ("gemm:p8w", "attn:plain", "gemm:p8w_res"), 0, spec=attn_spec(),
          norm=None, stream=None),
    # small shapes: T128 GEMMs, the plain attention path
    _case("self_small_keep_mask", "self", "small", "self_small", ("gemm:t128", "attn:plain", "gemm:t128"), 0,
          spec=attn_spec(causal=False), norm=None, stream=None, mask=True),
    _small_self("self_small_window", window=(64, 0)),
    _small_self("self_small_rotary", rotary=64),
    _small_self("self_small_normalize_query", causal=False, normq=True),
    dict(_small_self("self_small_fp16_in_bf16"), dtypes=(BF,), storage=FP),
    _case("self_small_prenorm_rms", "self", "small", "self_small", ("gemm:t128", "attn:plain", "gemm:t128"), 1,
          spec=attn_spec(), norm="rms", stream=None),
    # FlashAttentionLayer
    _case("layer_hd64", "layer", "hd64", "layer_kpre", ("gemm:p8w", "gemm:p8w+cs", "gemm:p8w", "attn:kpre", "gemm:p8w_res"), 0,
          spec=attn_spec("layer", kpre=True), norm=None, stream=None),
    _case("layer_small", "layer", "small", "layer_small", ("gemm:t128",) * 3 + ("attn:plain", "gemm:t128"), 0,
          spec=attn_spec("layer"), norm=None, stream=None),
]
for _act_ in ("gelu", "swiglu"):
    CASES += [
        _case(f"mlp_{_act_}_large", "mlp", "hd64", "mlp_blocked", _MLP_BLOCKED[_act_], 0, spec=mlp_spec(_act_), norm=None,
              stream=None),
        _case(f"mlp_{_act_}_prenorm", "mlp", "hd64", "mlp_blocked", _MLP_BLOCKED[_act_], 1, spec=mlp_spec(_act_),
              norm="layernorm", stream=None),
        _case(f"mlp_{_act_}_stream_ln", "mlp", "hd64", "mlp_fold",
              (_MLP_FOLD[_act_], "gemm:p8w_stats", _MLP_FOLD[_act_], "gemm:p8w_res"), 0, spec=mlp_spec(_act_), norm="layernorm",
              stream="out_in"),
        _case(f"mlp_{_act_}_stream_rms", "mlp", "hd64", "mlp_fold",
              (_MLP_FOLD[_act_], "gemm:p8w_stats", _MLP_FOLD[_act_], "gemm:p8w_res"), 0, spec=mlp_spec(_act_), norm="rms",
              stream="out_in"),
    ]
CASES += [
    _case("mlp_small_gelu", "mlp", "small", "mlp_small", ("mlp:two_launch/t128/t128",), 0, spec=mlp_spec("gelu", 2048),
          norm=None, stream=None),
    _case("mlp_small_swiglu", "mlp", "small", "mlp_small", ("mlp:two_launch/glu_t128x64/t128",), 0,
          spec=mlp_spec("swiglu", 2048), norm=None, stream=None),
    _case("mlp_small_relu", "mlp", "small", "mlp_small", ("mlp:two_launch/t128/t128",), 0, spec=mlp_spec("relu", 2048),
          norm=None, stream=None),
    _case("mlp_small_silu", "mlp", "small", "mlp_small", ("mlp:two_launch/t128/t128",), 0, spec=mlp_spec("silu", 2048),
          norm=None, stream=None),
    _case("mlp_small_erf_gelu_prenorm", "mlp", "small", "mlp_small", ("mlp:two_launch/t128/t128",), 1,
          spec=mlp_spec("gelu_erf", 2048), norm="layernorm", stream=None),
    # synthetic.Block / CrossBlock: the attention sub-layer, then the MLP on the stream it really produced
    _case("block_fold", "block", "hd64", "block_fold",
          ("gemm:p8w+cs", "attn:kpre+oblk", "gemm:p8w_stats", "gemm:p8w_fold", "gemm:p8w_res"), 1,
          spec=attn_spec(kpre=True), mlp=mlp_spec("gelu"), norm="layernorm", fold=True),
    _case("block_no_fold", "block", "hd64", "block_no_fold",
          ("gemm:p8w+cs", "attn:kpre+oblk", "gemm:p8w_res", "mlp:blocked/p8w/p8w_res"), 2,
          spec=attn_spec(kpre=True), mlp=mlp_spec("gelu"), norm="layernorm", fold=False),
    _case("block_rms_swiglu", "block", "hd64", "block_fold",
          ("gemm:p8w+cs", "attn:kpre+oblk", "gemm:p8w_stats", "gemm:p8w_glu_fold", "gemm:p8w_res"), 1,
          spec=attn_spec(kpre=True), mlp=mlp_spec("swiglu"), norm="rms", fold=True),
    _case("block_chain", "chain", "hd64", "block_chain",
          ("gemm:p8w+cs", "attn:kpre+oblk", "gemm:p8w_stats", "gemm:p8w_fold", "gemm:p8w_stats",
           "gemm:p8w_fold+cs", "attn:kpre+oblk", "gemm:p8w_stats", "gemm:p8w_fold", "gemm:p8w_res"), 1,
          spec=attn_spec(kpre=True), mlp=mlp_spec("gelu"), norm="layernorm", fold=True),
    _case("cross_block_fold", "cross_block", "hd64", "cross_block_fold",
          ("gemm:p8w", "gemm:p8w+cs", "gemm:p8w", "attn:kpre", "gemm:p8w_stats", "gemm:p8w_fold", "gemm:p8w_res"), 1,
          spec=attn_spec("cross", causal=False, kpre=True), mlp=mlp_spec("gelu"), norm="layernorm", fold=True),
]


def case(name: str) -> dict:
    return next(c for c in CASES if c["name"] == name)


def case_ids() -> List[tuple]:
    """(case name, compute dtype) of every GPU test."""
    return [(c["name"], dt) for c in CASES for dt in c["dtypes"]]


def seed_of(name: str, dtype) -> int:
    return (sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) + (0 if dtype == BF else 7919)) % (2 ** 31)

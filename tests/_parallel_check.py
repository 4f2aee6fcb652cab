"""Parallel-layer checker shared by tests/test_parallel_check.py (CPU) and tests/test_gpu_parallel_rows.py (a plain helper module,
not a conftest).  It judges the ring, tensor-parallel and sequence-parallel routes of mio/parallelism row by row against fp64, with
bars that come from a rounding model and never from the kernels.

Placement.  positions(rank, sp, S_local, zigzag): the global positions of a rank's local rows (contiguous: rank * S_local + i;
zig-zag: blocks (rank, 2 sp - 1 - rank) of S_local / 2 rows, sequence_parallel.zigzag_blocks); local_of() is its inverse, and
shard() / place() move rows between the full sequence and the shards with it.

Ring reference and model.  ring_reference(): the fp64, unrounded attention of the full q [B,S,H,D] over the full k / v
[B,Sk,Hkv,D] (16-bit inputs) with _attn_check.reference's mask conventions -- causal, or an additive mask [B,1|H,S,Sk], or
k_prescaled (K~ is given as rounded, the scores are q . K~ in base 2: softmax_scale = ln 2, as tests/test_gpu_parallel.py::_w_ring
does); it returns (o, lse).  ring_model(): _module_check._attention under a rounding _Arith -- P rounded to 16 bits before P.V --
with the context rounded once to the dtype.  The ring adds NO 16-bit rounding point to the dense attention: its carry between
launches is the fp32 (o_acc, lse) pair of sequence_parallel.ring_attention ("states = [(torch.zeros(B, n, H, D,
dtype=torch.float32 ...") and only the last launch of a query segment stores 16 bits ("write_out=fin").  So the model of a ring,
whatever sp, placement and exchange, is the model of the dense attention.

Tensor-parallel model.  _module_check.model(tp=2) (its docstring, "tensor-parallel form").  tp_params() / sp_params() map a
sub-layer's parameters (the spec names of _module_check: qkv_proj / q_proj / k_proj / v_proj / o_proj, fc1 / fc2) onto the Linear
names of the parallel modules (query / key / value / output, dense_h_to_4h / dense_4h_to_h) and slice a rank's share.
sp_reference() / sp_model(): SequenceParallelAttention on the full sequence -- the pre-norm output stored (_local.prenorm), q / k
/ v projections stored (K pre-scaled in ring mode where _nn.attention_plan says so), the attention of the mode ("ring" and "full":
the whole sequence; "local": every shard on its own), the out-projection with the residual in its epilogue -- whose rows a rank
holds at positions().

Judgement.  Every output finite; per-row ||y - ref|| / ||ref|| in u as the worst row, the mean, and two group means, against the
same statistics of the model times _module_check.MARGINS (3 / 1.5 / 2 / 2), floored at FLOOR (0.75 u): the project's figures,
unchanged, never taken from a kernel result and never set per case.  Modules: _module_check.judge on a rank's rows against the
reference rows at its positions (groups: 256-row tiles and sequences of the LOCAL rows, the units the rank's kernels work in).
Ring: judge_ring on the rows of all ranks placed at their global positions; a row is one (batch, head, query) vector, the groups are
_attn_check's 16 consecutive queries inside a query segment ("tile") and one query segment of one (batch, head) ("seq").  No row is
exempt: tests/test_parallel_check.py asserts that every row of every case has a finite reference lse.

Loopback.  loopback(rank, sp, shards) lets sequence_parallel.ring_attention run as rank `rank` of `sp` in one process without a
process group.  It replaces what sequence_parallel asks of `comm` / `dist` and nothing else: world size, rank, is_initialized,
mesh_exchange_start and ring_exchange, the last two served from the table `shards` of all ranks' (k, v): chunks[i] are fresh
contiguous copies of the shards of origin (rank - i) % sp, handles whose wait / wait_chunk do nothing.  Ranks run one after the
other; every launch, narrow view, carry buffer and output write is the product's.  run_ring() does that for all ranks.

Recorder.  steps() wraps _local.attention_step and asks ops.fa3_route with the same arguments before each launch: the route of
every launch of every rank is known (and a hook may alter a launch: the faults of tests/test_parallel_check.py).

RING_CASES / MODULE_CASES are the case tables of tests/test_gpu_parallel_rows.py; tests/test_parallel_check.py confirms their
routes on the CPU.

Measured on the MI355X by one run of tests/test_gpu_parallel_rows.py (largest value per (dtype, family) over its judged cases,
kernel / model, in u; "ratio" is the largest statistic / bar, 1.0 = at the bar; n = judged cases, a module case counting once per
rank):

  dtype    family                  |  kernel: worst   mean   tile    seq  |  model: worst   mean   tile    seq  | ratio   n
  bfloat16 ring_causal             |          1.06  0.539   0.69   0.59  |         0.87  0.500   0.60   0.52  |  0.72   8
  bfloat16 ring_kpre_causal        |          1.06  0.523   0.63   0.55  |         0.76  0.494   0.55   0.51  |  0.70   1
  bfloat16 ring_kpre_noncausal     |          1.04  0.547   0.63   0.56  |         0.83  0.500   0.56   0.51  |  0.73   2
  bfloat16 ring_kpre_zigzag        |          0.98  0.530   0.61   0.56  |         0.82  0.496   0.56   0.51  |  0.71   2
  bfloat16 ring_mask               |          1.21  0.574   0.68   0.59  |         0.83  0.497   0.56   0.51  |  0.77   4
  bfloat16 ring_noncausal          |          1.17  0.569   0.65   0.59  |         0.86  0.510   0.60   0.52  |  0.76   9
  bfloat16 ring_zigzag             |          1.11  0.547   0.66   0.60  |         0.87  0.504   0.57   0.52  |  0.72   8
  bfloat16 sp_attn_full            |          1.80  1.083   1.10   1.10  |         1.76  1.081   1.10   1.10  |  0.67   2
  bfloat16 sp_attn_local           |          1.76  1.042   1.06   1.06  |         1.77  1.037   1.05   1.05  |  0.67   2
  bfloat16 sp_attn_ring            |          1.87  1.083   1.10   1.10  |         1.87  1.081   1.10   1.10  |  0.67   4
  bfloat16 sp_mlp_small            |          0.68  0.618   0.62   0.62  |         0.68  0.618   0.62   0.62  |  0.67   2
  bfloat16 tp_attn_hd64            |          1.94  1.180   1.20   1.20  |         1.92  1.178   1.20   1.20  |  0.67   6
  bfloat16 tp_attn_small           |          1.60  1.177   1.18   1.18  |         1.61  1.174   1.18   1.18  |  0.67   4
  bfloat16 tp_mlp_hd64             |          0.87  0.768   0.77   0.77  |         0.87  0.768   0.77   0.77  |  0.67   4
  bfloat16 tp_mlp_small            |          0.83  0.766   0.77   0.77  |         0.83  0.766   0.77   0.77  |  0.67   2
  float16  ring_causal             |          1.12  0.540   0.70   0.58  |         0.88  0.500   0.58   0.51  |  0.72   8
  float16  ring_kpre_causal        |          0.97  0.517   0.62   0.55  |         0.82  0.493   0.55   0.51  |  0.69   1
  float16  ring_kpre_noncausal     |          1.01  0.541   0.62   0.55  |         0.89  0.503   0.57   0.52  |  0.72   2
  float16  ring_kpre_zigzag        |          1.08  0.531   0.63   0.58  |         0.87  0.497   0.56   0.52  |  0.71   2
  float16  ring_mask               |          1.20  0.574   0.67   0.59  |         0.82  0.497   0.56   0.51  |  0.77   4
  float16  ring_noncausal          |          1.05  0.568   0.71   0.59  |         0.87  0.510   0.58   0.52  |  0.76   9
  float16  ring_zigzag             |          1.14  0.547   0.68   0.59  |         0.84  0.504   0.59   0.54  |  0.72   8
  float16  sp_attn_full            |          1.69  1.086   1.10   1.10  |         1.74  1.084   1.10   1.10  |  0.67   2
  float16  sp_attn_local           |          1.76  1.046   1.06   1.06  |         1.77  1.043   1.06   1.06  |  0.67   2
  float16  sp_attn_ring            |          1.86  1.091   1.10   1.11  |         1.87  1.089   1.10   1.10  |  0.67   4
  float16  sp_mlp_small            |          0.68  0.618   0.62   0.62  |         0.67  0.618   0.62   0.62  |  0.67   2
  float16  tp_attn_hd64            |          1.91  1.170   1.19   1.19  |         1.88  1.167   1.18   1.18  |  0.67   6
  float16  tp_attn_small           |          1.57  1.176   1.18   1.18  |         1.60  1.172   1.18   1.18  |  0.67   4
  float16  tp_mlp_hd64             |          0.86  0.767   0.77   0.77  |         0.86  0.767   0.77   0.77  |  0.67   4
  float16  tp_mlp_small            |          0.83  0.766   0.77   0.77  |         0.84  0.766   0.77   0.77  |  0.67   2

  (76 tests in 53.4 s of wall time.  The 68 ring cases take 5 s together: the slowest 1.0 s -- the first launch of the process --
  and every other at most 0.15 s.  The eight spawns take the rest: 3.4 to 4.1 s each for the tensor-parallel ones, which is what
  a spawn of tests/test_gpu_parallel.py costs on the same machine (3.3 to 3.9 s), and 7.7 to 9.5 s for the four with a ring case:
  gloo moves that case's K / V shards, 2 x 33 MB per rank, through the host in 4.6 s -- test_gpu_parallel.py's
  k_prescaled_module_branches[sp] moves as much and takes 8.7 s; the all-gather of the same bytes in "full" mode takes 0.1 s.)
  The modules land on their model to within a few hundredths of a u in every statistic, in both dtypes: sharding, the chunked
  row-parallel GEMM, the all-reduce and the ring add nothing to what their rounding points cost.  The ring launches sit
  about 0.05 u above the model in the mean (0.52 to 0.57 against 0.50) and 0.2 to 0.4 u in the worst row, where the same
  kernels sit without a carry (tests/_attn_check.py: fwd3 0.59, fwd1 0.62, fwd5_kpre_carry 0.61 in the mean): the fp32
  arithmetic inside a launch, which the model does not round.  The largest statistic-to-bar ratio is 0.77 (the mean
  of the masked ring, bar 1.5 x the model's); no family comes near a margin, so MARGINS stands unchanged.
"""
from __future__ import annotations

import contextlib
import math
from typing import Callable, Dict, List, Optional

import torch

import _attn_check as ac
import _module_check as mc

BF, FP = mc.BF, mc.FP
LN2 = math.log(2.0)
SCORE_STD = 2.4                 # standard deviation the scores are drawn at (_module_check, "Inputs")
GROUP = ac.GROUP


# ---- placement -----------------------------------------------------------------------------------------------------------------
def positions(rank: int, sp: int, S_local: int, zigzag: bool) -> torch.Tensor:
    """Global positions [S_local] of the local rows of `rank`."""
    i = torch.arange(S_local)
    if not zigzag:
        return rank * S_local + i
    if S_local % 2:
        raise ValueError("zig-zag shards have even length")
    h = S_local // 2
    return torch.where(i < h, rank * h + i, (2 * sp - 1 - rank) * h + (i - h))


def local_of(pos, sp: int, S_local: int, zigzag: bool):
    """Inverse of positions(): (rank, local row) of the global positions `pos` (a tensor or an int)."""
    pos = torch.as_tensor(pos)
    if not zigzag:
        return pos // S_local, pos % S_local
    h = S_local // 2
    blk = pos // h
    first = blk < sp
    return torch.where(first, blk, 2 * sp - 1 - blk), torch.where(first, pos % h, h + pos % h)


def shard(t: torch.Tensor, rank: int, sp: int, zigzag: bool, dim: int = 1) -> torch.Tensor:
    """The rows of `rank` of a full sequence along dim."""
    return t.index_select(dim, positions(rank, sp, t.shape[dim] // sp, zigzag).to(t.device))


def place(shards: List[torch.Tensor], sp: int, zigzag: bool, dim: int = 1) -> torch.Tensor:
    """The full sequence from the per-rank shards, every row at its global position."""
    Sl = shards[0].shape[dim]
    shape = list(shards[0].shape)
    shape[dim] = Sl * sp
    full = torch.empty(shape, dtype=shards[0].dtype, device=shards[0].device)
    for r, s in enumerate(shards):
        full.index_copy_(dim, positions(r, sp, Sl, zigzag).to(s.device), s)
    return full


# ---- ring reference and model --------------------------------------------------------------------------------------------------
def _scale(D: int, k_prescaled: bool) -> float:
    return LN2 if k_prescaled else 1.0 / math.sqrt(D)


def ring_reference(q, k, v, *, causal=False, additive_mask=None, k_prescaled=False, device=None):
    """fp64 (o [B,S,H,D], lse [B,H,S]) of the full attention, nothing rounded (module docstring)."""
    return ac.reference(q, k, v, causal=causal, softmax_scale=_scale(q.shape[-1], k_prescaled), additive_mask=additive_mask,
                        device=device)


def ring_model(q, k, v, *, dtype, causal=False, additive_mask=None, k_prescaled=False, device=None):
    """The rounding model of the ring = of the dense attention (module docstring): fp64 [B,S,H,D] on the 16-bit grid."""
    A = mc._Arith(dtype, device)
    return A.r(mc._attention(A, A.f(q), A.f(k), A.f(v), _scale(q.shape[-1], k_prescaled), causal, additive=additive_mask,
                             chunk=1))


# ---- judgement -----------------------------------------------------------------------------------------------------------------
def ring_measure(o, ref, dtype, seg: int) -> dict:
    """dict(worst, mean, tile, seq) in u of o [B,S,H,D] against ref: tile = the worst mean over 16 consecutive queries of one
    query segment (seg rows; S is a multiple of it), seq = the worst mean over one query segment of one (batch, head)."""
    e = ac.row_errors(o, ref) / mc.U[dtype]                     # [B, H, S]
    B, H, S = e.shape
    assert S % seg == 0, (S, seg)
    es = e.view(B, H, S // seg, seg)
    pad = (-seg) % GROUP
    n = torch.full((seg + pad,), 1.0, dtype=e.dtype, device=e.device)
    n[seg:] = 0.0
    eg = torch.nn.functional.pad(es, (0, pad)).view(B, H, S // seg, -1, GROUP).sum(-1) / n.view(-1, GROUP).sum(-1)
    return {"worst": e.max().item(), "mean": e.mean().item(), "tile": eg.max().item(), "seq": es.mean(-1).max().item()}


def _verdict(st, ms, tag, dtype, family, record):
    bar = {k_: max(mc.MARGINS[k_] * ms[k_], mc.FLOOR) for k_ in mc.MARGINS}
    if record:
        rec = mc.STATS.setdefault((dtype, family), {"n": 0, "ratio": 0.0, **{k_: 0.0 for k_ in mc.MARGINS},
                                                    **{"model_" + k_: 0.0 for k_ in mc.MARGINS}})
        rec["n"] += 1
        for k_ in mc.MARGINS:
            rec[k_] = max(rec[k_], st[k_])
            rec["model_" + k_] = max(rec["model_" + k_], ms[k_])
            rec["ratio"] = max(rec["ratio"], st[k_] / bar[k_])
    assert all(st[k_] <= bar[k_] for k_ in mc.MARGINS), (
        f"{tag}: " + "; ".join(f"{k_} {st[k_]:.3f} u (bar {bar[k_]:.3f}, model {ms[k_]:.3f})" for k_ in mc.MARGINS))
    return st


def judge_ring(o, ref, model_o, dtype, seg: int, family: str, what: str = "", record: bool = True) -> dict:
    """Assert the ring output o [B,S,H,D] (all ranks' rows at their global positions, 16-bit) against the fp64 reference within
    the bars taken from model_o; seg = rows of a query segment."""
    tag = f"{what} [{family} {str(dtype).split('.')[-1]}]"
    assert tuple(o.shape) == tuple(ref.shape), f"{tag}: {tuple(o.shape)} vs {tuple(ref.shape)}"
    bad = ~torch.isfinite(o.detach().float())
    assert not bad.any(), f"{tag}: non-finite output ({int(bad.sum())} values)"
    return _verdict(ring_measure(o, ref, dtype, seg), ring_measure(model_o, ref, dtype, seg), tag, dtype, family, record)


# ---- loopback and recorder -----------------------------------------------------------------------------------------------------
class _Done:
    def wait(self):
        pass

    def wait_chunk(self, i):
        pass


class _Over:
    """`real` with the attributes `over` replaced."""

    def __init__(self, real, **over):
        self._real = real
        self.__dict__.update(over)

    def __getattr__(self, name):
        return getattr(self._real, name)


@contextlib.contextmanager
def loopback(rank: int, sp: int, shards):
    """sequence_parallel.ring_attention as rank `rank` of `sp` in this process (module docstring); shards[origin] = the (k, v)
    of every rank, in the layout of the call."""
    from mio.parallelism import sequence_parallel as spm
    passes = [0]

    def copies(origin):
        return [t.clone(memory_format=torch.contiguous_format) for t in shards[origin]]

    def mesh_exchange_start(tensors, group=None, buffers=None):
        return _Done(), [[t.contiguous() for t in tensors]] + [copies((rank - i) % sp) for i in range(1, sp)]

    def ring_exchange(*tensors, group=None, async_op=False, **kw):
        passes[0] += 1
        out = copies((rank - passes[0]) % sp)
        assert len(out) == len(tensors)
        return (_Done(), out) if async_op else out

    saved = spm.comm, spm.dist
    spm.comm = _Over(saved[0], get_world_size=lambda group=None: sp, get_rank=lambda group=None: rank,
                     mesh_exchange_start=mesh_exchange_start, ring_exchange=ring_exchange)
    spm.dist = _Over(saved[1], is_initialized=lambda: True)
    try:
        yield
    finally:
        spm.comm, spm.dist = saved


@contextlib.contextmanager
def steps(route: bool = True, hook: Optional[Callable] = None):
    """Record every _local.attention_step launch: dict(route, Sq, Sk, carry_in, write_out, q_offset, k_offset).  hook(i, q, k, v,
    kw, launch) -> None may change kw in place or launch further steps itself (launch = the unrecorded step function)."""
    from mio import ops
    from mio.parallelism import _local
    calls: List[dict] = []
    real = _local.attention_step

    def step(q, k, v, **kw):
        si = 2 if kw.get("layout", "bshd") == "bhsd" else 1
        if hook is not None:
            r = hook(len(calls), q, k, v, kw, real)
            if r is not None:
                q, k, v = r
        calls.append({"route": ops.fa3_route(q, k, v, **kw) if route else None, "Sq": q.shape[si], "Sk": k.shape[si],
                      "carry_in": bool(kw.get("carry_in")), "write_out": bool(kw.get("write_out", True)),
                      "q_offset": kw.get("q_offset", 0), "k_offset": kw.get("k_offset", 0)})
        return real(q, k, v, **kw)

    _local.attention_step = step
    try:
        yield calls
    finally:
        _local.attention_step = real


def run_ring(q, k, v, sp: int, *, layout="bshd", causal=False, zigzag=False, exchange="mesh", additive_mask=None,
             k_prescaled=False, route=True, hook=None, device=None):
    """ring_attention of every rank on the loopback, one rank after the other: (the full output [B,S,H,D] with every rank's rows
    at their global positions, the launch records per rank).  q [B,S,H,D], k / v [B,Sk,Hkv,D] and additive_mask [B,1|H,S,Sk] are
    the full tensors; hook(rank) -> a steps() hook."""
    from mio.parallelism.sequence_parallel import ring_attention
    Sl = q.shape[1] // sp

    def local(t, r):
        s = shard(t, r, sp, zigzag)
        s = s.permute(0, 2, 1, 3) if layout == "bhsd" else s
        return s.contiguous().to(device or t.device)

    kv = [(local(k, r), local(v, r)) for r in range(sp)]
    outs, records = [], []
    for r in range(sp):
        add = None
        if additive_mask is not None:
            add = shard(additive_mask, r, sp, zigzag, dim=2).contiguous().to(device or q.device)
        with loopback(r, sp, kv), steps(route, None if hook is None else hook(r)) as calls:
            o = ring_attention(local(q, r), kv[r][0], kv[r][1], None, layout=layout, causal=causal, zigzag=zigzag,
                               exchange=exchange, additive_mask=add, k_prescaled=k_prescaled)
        outs.append(o.permute(0, 2, 1, 3) if layout == "bhsd" else o)
        records.append(calls)
    assert outs[0].shape[1] == Sl
    return place(outs, sp, zigzag), records


# ---- the ring case table -------------------------------------------------------------------------------------------------------
RING_B = 2
MASKED_KEYS = 37                # the additive mask is -inf on the last 37 global keys of batch 1


def _ring(form, sp, heads, D, layout, Sl, Skl=None, mask_heads=None):
    """form: noncausal | causal | zigzag | mask | kpre_noncausal | kpre_causal | kpre_zigzag.  Sl / Skl: local query / key rows.
    The route every launch of every rank takes follows from the plan of csrc/fa3_route.h with the (o_acc, lse) carry: pre-scaled
    segments longer than 128 fwd5_kpre_carry, unmasked segments longer than 128 fwd3, segments of at most 128 fwd1, masked
    launches fwd1_add."""
    Skl = Sl if Skl is None else Skl
    zz = form.endswith("zigzag")
    seg = Sl // 2 if zz else Sl
    kpre = form.startswith("kpre")
    if form == "mask":
        route = "fwd1_add"
    elif seg <= 128:
        route = "fwd1"
    else:
        route = "fwd5_kpre_carry" if kpre else "fwd3"
    assert not kpre or (D == 64 and seg > 128)
    name = f"{form}_sp{sp}_h{heads[0]}kv{heads[1]}_d{D}_{layout}_s{Sl}" + (f"k{Skl}" if Skl != Sl else "")
    return dict(name=name, form=form, sp=sp, H=heads[0], Hkv=heads[1], D=D, layout=layout, Sl=Sl, Skl=Skl, zigzag=zz,
                causal=form.endswith("causal") and not form.endswith("noncausal") or zz, kpre=kpre, mask_heads=mask_heads,
                seg=seg, route=route, family="ring_" + form)


MHA, GQA = (4, 4), (4, 2)
RING_CASES: List[dict] = [
    # local length 200: the pipelined kernel with the carry, ragged
    _ring("noncausal", 2, MHA, 64, "bshd", 200), _ring("noncausal", 3, GQA, 128, "bhsd", 200),
    _ring("noncausal", 4, MHA, 80, "bshd", 200), _ring("noncausal", 8, GQA, 64, "bhsd", 200),
    _ring("causal", 2, GQA, 128, "bshd", 200), _ring("causal", 3, MHA, 64, "bhsd", 200),
    _ring("causal", 4, GQA, 64, "bshd", 200), _ring("causal", 8, MHA, 128, "bshd", 200),
    _ring("causal", 3, MHA, 80, "bhsd", 200),
    # local length 100: the fwd1 carry
    _ring("noncausal", 3, MHA, 64, "bshd", 100), _ring("noncausal", 4, GQA, 128, "bhsd", 100),
    _ring("causal", 2, MHA, 128, "bhsd", 100), _ring("causal", 4, GQA, 64, "bshd", 100),
    _ring("causal", 3, GQA, 80, "bshd", 100),
    # zig-zag 272: halves of 136
    _ring("zigzag", 2, MHA, 64, "bshd", 272), _ring("zigzag", 3, GQA, 128, "bhsd", 272),
    _ring("zigzag", 4, MHA, 128, "bshd", 272), _ring("zigzag", 8, GQA, 64, "bshd", 272),
    _ring("zigzag", 3, MHA, 80, "bhsd", 272),
    # zig-zag 128: halves of 64
    _ring("zigzag", 2, GQA, 128, "bhsd", 128), _ring("zigzag", 4, MHA, 64, "bshd", 128),
    _ring("zigzag", 3, MHA, 128, "bshd", 128),
    # non-causal cross: 200 local queries, 136 local keys
    _ring("noncausal", 3, GQA, 64, "bshd", 200, 136), _ring("noncausal", 4, MHA, 128, "bhsd", 200, 136),
    _ring("noncausal", 2, MHA, 80, "bshd", 200, 136),
    # additive mask
    _ring("mask", 2, MHA, 64, "bshd", 200, mask_heads=1), _ring("mask", 3, GQA, 128, "bhsd", 100, mask_heads=4),
    _ring("mask", 4, MHA, 64, "bshd", 200, 136, mask_heads=1), _ring("mask", 4, GQA, 128, "bshd", 200, mask_heads=4),
    # pre-scaled K at head dim 64, segments longer than 128
    _ring("kpre_noncausal", 3, MHA, 64, "bshd", 200), _ring("kpre_causal", 4, GQA, 64, "bhsd", 200),
    _ring("kpre_zigzag", 2, MHA, 64, "bshd", 272), _ring("kpre_zigzag", 4, GQA, 64, "bhsd", 272),
    _ring("kpre_noncausal", 2, MHA, 64, "bshd", 200, 136),
]


def ring_case(name: str) -> dict:
    return next(c for c in RING_CASES if c["name"] == name)


def ring_inputs(c: dict, dtype, B: int = RING_B):
    """(q [B,S,H,D], k, v [B,Sk,Hkv,D], additive mask or None) of a ring case on the CPU in dtype: q scaled so that the scores
    have a standard deviation of SCORE_STD; with kpre, k is K~ = K * log2(e) / sqrt(D) rounded once."""
    g = torch.Generator().manual_seed(mc.seed_of(c["name"], dtype))
    S, Sk, D = c["sp"] * c["Sl"], c["sp"] * c["Skl"], c["D"]
    q = (torch.randn(B, S, c["H"], D, generator=g) * SCORE_STD).to(dtype)
    k = torch.randn(B, Sk, c["Hkv"], D, generator=g)
    k = (k * (mc.LOG2E / math.sqrt(D))).to(dtype) if c["kpre"] else k.to(dtype)
    v = torch.randn(B, Sk, c["Hkv"], D, generator=g).to(dtype)
    add = None
    if c["form"] == "mask":
        add = torch.randn(B, c["mask_heads"], S, Sk, generator=g)
        add[B - 1, :, :, Sk - MASKED_KEYS:] = float("-inf")
    return q, k, v, add


def ring_kwargs(c: dict) -> dict:
    return dict(layout=c["layout"], causal=c["causal"], zigzag=c["zigzag"], k_prescaled=c["kpre"])


# ---- parameters of the parallel modules ----------------------------------------------------------------------------------------
def tp_params(spec, P: Dict[str, torch.Tensor], rank: int, tp: int) -> Dict[str, torch.Tensor]:
    """A rank's parameters of TensorParallelAttention (spec kind "self": P holds qkv_proj [3 d, d] and o_proj) or
    TensorParallelMLP (fc1, fc2) under the modules' own names."""
    out = {}
    if spec["op"] == "mlp":
        per = P["fc1.weight"].shape[0] // tp
        sl = slice(rank * per, (rank + 1) * per)
        out["dense_h_to_4h.weight"], out["dense_h_to_4h.bias"] = P["fc1.weight"][sl], P["fc1.bias"][sl]
        out["dense_4h_to_h.weight"], out["dense_4h_to_h.bias"] = P["fc2.weight"][:, sl], P["fc2.bias"]
        return out
    d = P["o_proj.weight"].shape[0]
    assert spec["kind"] == "self" and spec["Hkv"] == spec["H"]
    per = d // tp
    for i, name in enumerate(("query", "key", "value")):
        sl = slice(i * d + rank * per, i * d + (rank + 1) * per)
        out[name + ".weight"], out[name + ".bias"] = P["qkv_proj.weight"][sl], P["qkv_proj.bias"][sl]
    out["output.weight"], out["output.bias"] = P["o_proj.weight"][:, rank * per:(rank + 1) * per], P["o_proj.bias"]
    return out


def sp_params(spec, P: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The parameters of SequenceParallelAttention (spec kind "layer") or SequenceParallelMLP under the modules' own names."""
    names = ({"fc1": "dense_h_to_4h", "fc2": "dense_4h_to_h"} if spec["op"] == "mlp" else
             {"q_proj": "query", "k_proj": "key", "v_proj": "value", "o_proj": "output"})
    return {names[k_.split(".")[0]] + "." + k_.split(".")[1]: t for k_, t in P.items()}


def _sp_sublayer(A, spec, P, x, sp, mode, norm, residual):
    """SequenceParallelAttention on the full sequence x [B, S, d] (contiguous placement of the rows in `local` mode)."""
    B, S, d = x.shape
    x2 = A.load(x)
    xin = x2
    if norm is not None:
        n = dict(kind="layernorm", eps=norm["eps"], weight=A.load(norm["weight"]), bias=A.load(norm["bias"]))
        xin = A.r(mc._norm_rows(x2.reshape(-1, d), n)).view(B, S, d)        # _local.prenorm: the norm output is stored
    if mode == "local":
        xin = xin.reshape(B * sp, S // sp, d)
    branch = mc._sublayer(A, spec, P, xin, None, False, False)[1].reshape(B, S, d)
    return A.r(branch + x2 if residual else branch)


def sp_reference(spec, P, x, *, sp, mode, norm=None, residual=True, device=None):
    return _sp_sublayer(mc._Arith(None, device), spec, P, x, sp, mode, norm, residual)


def sp_model(spec, P, x, *, dtype, sp, mode, norm=None, residual=True, device=None):
    return _sp_sublayer(mc._Arith(dtype, device), spec, P, x, sp, mode, norm, residual)


# ---- the module case table -----------------------------------------------------------------------------------------------------
# rows: _module_check.SHAPES "small" (2 x 300) and "hd64" (63 x 257 = 16 191 rows); the sequence-parallel attention keeps hd64's
# 63 sequences at a local length of 258 (zig-zag halves of 129: longer than 128, so K stays pre-scaled)
D_MODEL, HEADS, TP_I, SP_LOCAL = 1024, 16, 2048, 258
WORLD = 2


def _mod(name, module, family, shape, routes, norms, **kw):
    """routes: per rank, what every launch with a route must be, in order -- "gemm:<route>" (+cs: with a column scale) and
    "attn:<route>"; norms: norm kernel launches per rank."""
    return dict(name=name, module=module, family=family, shape=shape, routes=routes, norms=norms, **kw)


def _tp_attn(shape, chunks, full):
    """TensorParallelAttention, tp = 2, causal; full: with residual and a LayerNorm pre_norm."""
    big = shape == "hd64"
    B, S = mc.SHAPES[shape][2:]
    n = max(1, min(chunks, B * S // 256 if B * S >= 512 else 1))
    head = ("gemm:p8w+cs", "attn:fwd5_kpre") if big else ("gemm:t128", "attn:fwd5")
    if big and n == 1:
        tails = (("gemm:p8w_res",) if full else ("gemm:p8w",), ("gemm:p8w",))
    else:
        tails = (("gemm:t128",) * n,) * 2
    return _mod(f"tp_attn_{shape}_chunks{chunks}_{'full' if full else 'bare'}", "tp_attn", "tp_attn_" + shape, shape,
                tuple(head + t for t in tails), int(full), spawn="tp_attn", spec=mc.attn_spec(kpre=big), chunks=chunks,
                residual=full, norm=full,
                n_chunks=n)


def _tp_mlp(shape, act, chunks):
    big = shape == "hd64"
    B, S = mc.SHAPES[shape][2:]
    n = max(1, min(chunks, B * S // 256 if B * S >= 512 else 1))
    head = ("gemm:p8w",) if big else ("gemm:t128",)
    tails = (("gemm:p8w_res",), ("gemm:p8w",)) if big and n == 1 else (("gemm:t128",) * n,) * 2
    return _mod(f"tp_mlp_{shape}_{act}_chunks{chunks}", "tp_mlp", "tp_mlp_" + shape, shape, tuple(head + t for t in tails), 1,
                spawn="tp_mlp", spec=mc.mlp_spec(act, TP_I), chunks=chunks, residual=True, norm=True, n_chunks=n)


def _sp_attn(mode, exchange, zigzag, causal, attn_routes, kpre):
    pro = ("gemm:p8w", "gemm:p8w+cs" if kpre else "gemm:p8w", "gemm:p8w")
    return _mod(f"sp_attn_{mode}" + (f"_{exchange}" + ("_zigzag" if zigzag else "") if mode == "ring" else ""), "sp_attn",
                "sp_attn_" + mode, "sp", tuple(pro + tuple("attn:" + r for r in ar) + ("gemm:p8w_res",) for ar in attn_routes), 1,
                spawn="sp_" + exchange, spec=mc.attn_spec("layer", causal=causal, kpre=kpre), mode=mode, exchange=exchange,
                zigzag=zigzag, residual=True,
                norm=True)


_KC = "fwd5_kpre_carry"
MODULE_CASES: List[dict] = [
    _tp_attn("small", 3, True), _tp_attn("small", 1, False), _tp_attn("hd64", 3, True), _tp_attn("hd64", 1, True),
    _tp_attn("hd64", 1, False),
    _tp_mlp("small", "gelu", 3), _tp_mlp("hd64", "gelu", 3), _tp_mlp("hd64", "silu", 1),
    # causal ring, contiguous: rank 0 drops the launch on rank 1's (future) keys
    _sp_attn("ring", "mesh", False, True, ((_KC,), (_KC, _KC)), True),
    # causal ring, zig-zag blocks (0, 3) and (1, 2): five launches on either rank
    _sp_attn("ring", "ring", True, True, ((_KC,) * 5, (_KC,) * 5), True),
    _sp_attn("full", "ring", False, True, (("fwd5",), ("fwd5",)), False),
    _sp_attn("local", "mesh", False, False, (("fwd5",), ("fwd5",)), False),
    _mod("sp_mlp_small_gelu", "sp_mlp", "sp_mlp_small", "small", (("gemm:t128", "gemm:t128"),) * 2, 1,
         spawn="sp_mesh", spec=mc.mlp_spec("gelu", TP_I), residual=True, norm=True),
]
# one spawn per entry and dtype serves all of its cases; the two ring cases sit in different spawns because gloo moves their K / V
# shards (2 x 33 MB per rank) through the host in 4.6 s, against 3.4 s for a whole spawn without them
SPAWNS = ("tp_attn", "tp_mlp", "sp_mesh", "sp_ring")


def module_case(name: str) -> dict:
    return next(c for c in MODULE_CASES if c["name"] == name)


def module_shape(c: dict):
    """(B, S_local) of the rows a rank of the case works on."""
    if c["shape"] == "sp":
        return mc.SHAPES["hd64"][2], SP_LOCAL
    return mc.SHAPES[c["shape"]][2:]


def module_inputs(c: dict, dtype, B: Optional[int] = None):
    """(parameters under the spec names, the pre_norm's parameters or None, the full input rows) of a module case on the CPU in
    dtype: the same on every rank.  The sequence-parallel attention's input is the full sequence [B, 2 * 258, d]."""
    Bc, S = module_shape(c)
    B = Bc if B is None else B
    g = torch.Generator().manual_seed(mc.seed_of(c["name"], dtype))
    P = mc.draw_params(c["spec"], D_MODEL, g, dtype)
    n = mc.draw_norm("layernorm", D_MODEL, g, dtype) if c["norm"] else None
    x = mc.draw_rows(B, S * (WORLD if c["module"] == "sp_attn" else 1), D_MODEL, g, dtype)
    return P, n, x


def module_truth(c: dict, P, n, x, dtype, device=None, defect=None):
    """(fp64 reference, rounding model) of a module case on the full rows x."""
    if c["module"] == "sp_attn":
        kw = dict(sp=WORLD, mode=c["mode"], norm=n, residual=c["residual"], device=device)
        return sp_reference(c["spec"], P, x, **kw), sp_model(c["spec"], P, x, dtype=dtype, **kw)
    tp = WORLD if c["module"].startswith("tp") else 1
    kw = dict(norm=n, residual=c["residual"], device=device)
    return (mc.reference(c["spec"], P, x, **kw), mc.model(c["spec"], P, x, dtype=dtype, tp=tp, defect=defect, **kw))

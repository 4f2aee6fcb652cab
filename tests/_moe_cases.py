"""The case tables of tests/test_gpu_moe.py (a plain helper module): the smallest shapes that reach each seam of the grouped
decode-step GEMMs under the plan of csrc/moe_plan.h.  What they reach is asserted on the CPU by
tests/test_moe_host.py::test_case_tables_reach_the_seams through the library's host queries, so a retune of the plan fails
there, not on the GPU.

A GEMM case is one grouped GEMM: N output columns, K the reduction (up: N = I, K = d; down: N = d, K = I).  `split` says
whether the plan cuts K; `chunks` is the chunk count of the longest slice (chunk: 256 k, SwiGLU 128)."""
from dataclasses import dataclass
from typing import Optional

import torch

ACTS = ["none", "gelu", "gelu_erf", "relu", "silu", "swiglu"]
KSTEP, CHUNK, CHUNK_GLU = 32, 256, 128


@dataclass(frozen=True)
class Case:
    what: str
    T: int
    k: int
    E: int
    N: int
    K: int
    act: str = "none"
    split: Optional[bool] = False   # None: not asserted
    bias: bool = True
    res: bool = False          # down only
    chunks: Optional[int] = None
    routing: str = "random"    # random | same (all tokens pick experts 1 .. k) | mixed (MIXED_COUNTS)
    seed: int = 0

    @property
    def glu(self):
        return self.act == "swiglu"


def slices(K: int, nsplit: int):
    """[(k_begin, k_end)] of the plan's slices: whole 32-k steps, the last cut at K (include/mio_hip.h)."""
    steps = (K + KSTEP - 1) // KSTEP
    return [(s * steps // nsplit * KSTEP, min(K, (s + 1) * steps // nsplit * KSTEP)) for s in range(nsplit)]


def max_chunks(K: int, nsplit: int, glu: bool) -> int:
    c = CHUNK_GLU if glu else CHUNK
    return max((e - b + c - 1) // c for b, e in slices(K, nsplit)) if K else 0


# ---- routings written as logits -------------------------------------------------------------------------------------------------
def logits_for(choice: torch.Tensor, E: int, dtype=torch.float32) -> torch.Tensor:
    """Router logits [T, E] under which ids == choice [T, k] (distinct experts per token) exactly: slot j gets 4 - j / 2, every
    other expert -10 (all exact in bf16 and fp16; the k-th and (k+1)-th logit are at least 10 apart)."""
    T, k = choice.shape
    x = torch.full((T, E), -10.0)
    x.scatter_(1, choice.long(), (4.0 - 0.5 * torch.arange(k, dtype=torch.float32)).expand(T, k).contiguous())
    return x.to(dtype)


# T 64, k 3, E 10: experts with exactly 64, 33, 17, 14, 16, 15, 1, 0, 32 and 0 rows
MIXED = dict(T=64, k=3, E=10)
MIXED_COUNTS = (64, 33, 17, 14, 16, 15, 1, 0, 32, 0)


def mixed_choice() -> torch.Tensor:
    t = torch.arange(64)
    s0 = torch.zeros(64, dtype=torch.int64)
    s1 = torch.where(t < 14, 3, torch.where(t < 47, 1, 2))
    s2 = torch.where((t >= 14) & (t < 30), 4, torch.where((t >= 30) & (t < 45), 5, torch.where(t == 45, 6, 8)))
    return torch.stack([s0, s1, s2], 1)


def choice_of(c: Case) -> torch.Tensor:
    """The experts of every token of case c, [T, k] int64."""
    if c.routing == "same":
        return (torch.arange(c.k) + 1).expand(c.T, c.k).contiguous() % c.E
    if c.routing == "mixed":
        assert (c.T, c.k, c.E) == (64, 3, 10)
        return mixed_choice()
    g = torch.Generator().manual_seed(1000 + c.seed)
    return torch.stack([torch.randperm(c.E, generator=g)[:c.k] for _ in range(c.T)])


# ---- rows per expert: 0, 1, 15, 16, 17, 33 and 64 rows, at two small weights ----------------------------------------------------
ROWS = [Case(f"{r} ({d}, {I}) {side}", T, k, E, N, K, act, routing=r, split=None, bias=True, res=side == "down", seed=i)
        for i, (r, T, k, E) in enumerate([("mixed", 64, 3, 10), ("same", 64, 2, 8), ("random", 1, 1, 256)])
        for d, I in [(40, 72), (264, 136)]
        for side, N, K, act in [("up", I, d, "swiglu"), ("up", I, d, "gelu"), ("down", d, I, "none")]]

# ---- K and N seams: T 4, k 2, E 8 aims the split at 8 experts, so K 1032 splits at every N here and K <= 40 never does -----------
_S = dict(T=4, k=2, E=8)
N_EDGES = [Case(f"N {N} K {K} {act} {side}", N=N, K=K, act=act, split=K > 40, res=side == "down", seed=N + K, **_S)
           for N in (1, 15, 72, 1000) for K in (8, 40, 1032)
           for side, act in (("up", "silu"), ("up", "swiglu"), ("down", "none")) if not (N == 1000 and K == 8)]
EVERY_ACTIVATION = [Case(f"{act} K {K} bias {b}", N=72, K=K, act=act, split=K > 40, bias=b, seed=7 + K, **_S)
                    for act in ACTS for K in (40, 1032) for b in (True, False)]
DOWN_OPTIONS = [Case(f"down K {K} bias {b} res {r}", N=72, K=K, split=K > 40, bias=b, res=r, seed=9 + K, **_S)
                for K in (40, 1032) for b in (True, False) for r in (True, False)]

# ---- deep slices: 3, 4 and >= 5 chunks.  T 64, k 2, E 128, N 136: 128 experts x 3 column tiles ask for two slices; the K of a
# table are column prefixes of one weight, so ldw > K in all but the longest ------------------------------------------------------
_D = dict(T=64, k=2, E=128, N=136, split=True)
DEEP = [Case("gelu 3 chunks", K=1400, act="gelu", chunks=3, seed=21, **_D),
        Case("gelu 4 chunks", K=2000, act="gelu", chunks=4, seed=22, **_D),
        Case("gelu 6 chunks", K=2600, act="gelu", chunks=6, seed=23, **_D),
        Case("swiglu 3 chunks", K=704, act="swiglu", chunks=3, seed=24, **_D),
        Case("swiglu 4 chunks", K=960, act="swiglu", chunks=4, seed=25, **_D),
        Case("swiglu 6 chunks", K=1400, act="swiglu", chunks=6, seed=26, **_D)]
DEEP_LDW = 2600
# one slice of many chunks: 256 aimed experts x 2 column tiles are the 512 workgroups already
DEEP_UNSPLIT = [Case("none 5 chunks unsplit", 64, 8, 256, 72, 1032, "none", chunks=5, seed=27),
                Case("swiglu 9 chunks unsplit", 64, 8, 256, 72, 1032, "swiglu", chunks=9, seed=28)]

# ---- hostile memory, row independence, workspace, reruns: one unsplit and one split shape, each with idle experts -------------
HOSTILE = [Case("unsplit", 5, 2, 8, 72, 40, "swiglu", seed=31), Case("split", 5, 2, 8, 72, 1032, "swiglu", split=True, seed=32),
           Case("mixed rows", 64, 3, 10, 136, 264, "gelu", routing="mixed", seed=33)]
# (d, I) of the whole-MLP cases of HOSTILE: up is N = I, K = d and down N = d, K = I
HOSTILE_DI = {"unsplit": (40, 72), "split": (1032, 72), "mixed rows": (264, 136)}



def poison_idle(emb, active: torch.Tensor, fill: str) -> torch.Tensor:
    """After emb.fill(fill): the slices of the idle experts (dim 0 of the view, ~active) of an input operand embedded with
    tests/_hostile_gemm.Embedded := `fill` as well.  Embedded.fill() writes the whole value back into the view, the idle experts'
    part included, so without this only the bytes AROUND the view are hostile.  benign leaves the value's finite numbers.  The
    snapshot untouched() compares with is retaken.  Returns the mask of the idle elements over the buffer."""
    import _hostile_gemm as hg
    idle = torch.zeros_like(emb.owned)
    idle[emb.idx][~active.to(idle.device)] = True
    hg.poison(emb.buf.view(-1), idle.view(-1), fill, emb.sign)
    emb.snap = hg.bits(emb.buf.view(-1)).clone()
    return idle


def idle_is_hostile(emb, active: torch.Tensor, fill: str) -> bool:
    """Every element of the idle experts' slices holds NaN (fill nan) or +-finfo.max / 8 (fill huge); the active experts' slices hold
    the value."""
    v, act = emb.view, active.to(emb.buf.device)
    if not torch.equal(v[act], emb.value[act]):
        return False
    idle = v[~act].float()
    if fill == "nan":
        return bool(torch.isnan(idle).all())
    if fill == "huge":
        return bool((idle.abs() == float(torch.finfo(v.dtype).max / 8)).all()) if idle.numel() else True
    return bool(torch.isfinite(idle).all())


ALL_TABLES = {"ROWS": ROWS, "N_EDGES": N_EDGES, "EVERY_ACTIVATION": EVERY_ACTIVATION, "DOWN_OPTIONS": DOWN_OPTIONS, "DEEP": DEEP,
              "DEEP_UNSPLIT": DEEP_UNSPLIT, "HOSTILE": HOSTILE}

# ---- router ----------------------------------------------------------------------------------------------------------------------
ROUTER_E = [1, 3, 8, 60, 64, 65, 128, 256]
ROUTER_T = [1, 5, 64]


def router_ks(E: int):
    return sorted({k for k in (1, 2, 8, E if E <= 8 else None) if k is not None and k <= min(E, 8)})

"""The shapes of the GPU tests of the decode-step GEMM on weight-only FP8 (tests/test_gpu_gemm_skinny_w8.py), as plain tables: a
helper module, not a conftest, and free of torch so that the CPU suite can read it.

Which seams of csrc/gemm_skinny_w8.hip a shape reaches is decided by the plan (gemm_skinny_plan.h, SKINNY_W8): the row fragments MF =
ceil(M / 16), the slices of K in whole 64-k steps (mio_gemm_skinny_w8_splits / _slice: at least 16 M k each) and, inside a slice,
the chunks of the kernel's loop (mio_gemm_skinny_w8_chunk_k) over a ring of mio_gemm_skinny_w8_depth register sets.  The first
depth - 1 chunks of a slice fill the ring before the loop; the loop body is unrolled depth times, so the refill of every set, the
rewrite of an LDS buffer one barrier after its last read and the exits at each position of the unrolled body need slices of
depth + 1, depth + 2 and depth + 3 chunks.  CHUNK_K and DEPTH below are the values these tables were laid out for;
tests/test_gemm_skinny_w8_host.py::test_case_tables_reach_the_seams asks the loaded library and fails, naming the cases, when a
retune moves a table off what it is here to reach.

A case is (M, N, K, act, split, ...): split is what the plan must say (several slices or one), asserted on the CPU for every
case and again where the GPU test runs it."""
from typing import NamedTuple, Optional

ACTS = ["none", "gelu", "gelu_erf", "relu", "silu", "swiglu"]
CHUNK_K = {False: 256, True: 128}  # plain / SwiGLU
DEPTH = {False: 3, True: 4}


class Case(NamedTuple):
    M: int
    N: int
    K: int
    act: str
    split: bool                # the plan splits K: both launches run, the reduction's epilogue writes y
    bias: bool = True
    res: bool = False
    bias_gate: bool = True     # (SwiGLU only)
    ldx: Optional[int] = None  # x rows this far apart (None: K)
    ldw: Optional[int] = None  # weight rows this many bytes apart (None: K)
    ldr: Optional[int] = None  # the residual as a view of rows this wide
    guard: bool = False        # the output as a view inside a filled buffer
    rows: Optional[int] = None  # the weight and its scales are the first N rows of a weight of this many rows
    zero_scale: bool = False   # the scales of columns 3 .. 5 (those below N) are 0
    seed: int = 0

    @property
    def mf(self) -> int:
        return max(1, (self.M + 15) // 16)

    @property
    def glu(self) -> bool:
        return self.act == "swiglu"

    @property
    def what(self) -> str:
        return f"{self.act} {self.M}x{self.N}x{self.K}" + ("" if self.bias or self.res else " bare")


# ---- below the ring's depth: fragments, tails, edges, activations, strides ------------------------------------------------------------
ROW_FRAGMENTS = [Case(M, 72, 48, "gelu", False, res=True, seed=M) for M in (1, 5, 16, 17, 33, 48, 64)]  # K below one step

# K 16; K % 64 in {32, 48, 16} behind many steps, several slices
K_TAILS_AND_SPLITS = [Case(37, 72, 16, "none", False, res=True, seed=16),
                      Case(21, 264, 1056, "none", True, res=True, seed=1056),
                      Case(3, 8, 2096, "none", True, res=True, seed=2096),
                      Case(37, 72, 4112, "none", True, bias=False, res=True, seed=4112)]

N_EDGES = [Case(17, N, 272, "silu", False, guard=True, seed=N) for N in (1, 8, 15, 72, 1000)]

# fp32 partials in rows of N % 4 != 0: the scalar path of both kernels
N_EDGES_SPLIT = [Case(17, N, 1040, act, True, guard=True, seed=N) for act in ("silu", "swiglu") for N in (1, 15, 63, 71, 1001)]


def _activation_calls(act, K, split):
    """With bias and a residual, with neither, and (SwiGLU) the gate's bias alone with a residual."""
    calls = [Case(21, 72, K, act, split, bias=True, res=True, seed=1),
             Case(21, 72, K, act, split, bias=False, res=False, bias_gate=False, seed=2)]
    if act == "swiglu":
        calls.append(Case(21, 72, K, act, split, bias=False, res=True, bias_gate=True, seed=3))
    return calls


EVERY_ACTIVATION = [c for act in ACTS for K, split in ((48, False), (1040, True)) for c in _activation_calls(act, K, split)]

STRIDES = [Case(21, 72, K, act, split, res=True, ldx=K + 8, ldw=K + 16, ldr=88, guard=True, seed=K)
           for act in ("gelu", "swiglu") for K, split in ((48, False), (1040, True))]

# the first 40 of 72 rows of a weight and of its scale vector (the query rows of a fused projection)
ROW_SLICE = [Case(21, 40, K, act, split, res=True, rows=72, seed=K + 1)
             for act in ("none", "swiglu") for K, split in ((48, False), (1040, True))]

# a zero scale in a few columns: act(bias) there, whatever the sums
ZERO_SCALE = [Case(21, 72, K, act, split, res=True, zero_scale=True, seed=K + 2)
              for act in ("gelu", "swiglu") for K, split in ((48, False), (1040, True))]

WORKSPACE = [Case(19, 136, 1040, act, True, res=True, seed=9) for act in ("none", "swiglu")]

# ---- past the ring's depth ---------------------------------------------------------------------------------------------------------
# One slice: N 32776 is 513 column tiles, more workgroups than the split aims for, so the whole K is one slice and K alone sets
# the chunk count: depth + 1, + 2, + 3 chunks, the last one a 16-k tail.  The K are column prefixes of one [DEEP_N, DEEP_LDW] weight.
DEEP_N = 32776
DEEP_M = (5, 21, 37, 64)  # MF 1 .. 4, ragged and full
DEEP_K = {glu: tuple((DEPTH[glu] + i - 1) * CHUNK_K[glu] + 16 for i in (1, 2, 3)) for glu in (False, True)}
DEEP_LDW = max(max(v) for v in DEEP_K.values())
DEEP_UNSPLIT = [Case(M, DEEP_N, K, act, False, res=True, seed=K + M)
                for act in ("gelu", "swiglu") for K in DEEP_K[act == "swiglu"] for M in DEEP_M]

# Several slices (N 8200: 129 column tiles, four slices where 16 M allows), each of more chunks than the ring is deep, not all of
# the same count.  Per MF a full and a ragged last fragment; M 1 is MF 1's ragged one.  Column prefixes of one weight again.
DEEP_SPLIT_N = 8200
DEEP_SPLIT_M = (1, 16, 21, 32, 37, 48, 53, 64)
DEEP_SPLIT_K = {False: 4112, True: 2576}
DEEP_SPLIT = [Case(M, DEEP_SPLIT_N, DEEP_SPLIT_K[act == "swiglu"], act, True, res=True, seed=M)
              for act in ("gelu", "swiglu") for M in DEEP_SPLIT_M]

# operands inside NaN-filled buffers (test_poisoned_paddings): everything next to what the kernel may read is poison
POISONED = [Case(M, 72, K, act, split, res=True, ldx=K + 24, ldw=K + 16, ldr=88, guard=True, seed=M + K)
            for act in ("gelu", "swiglu") for M, K, split in ((37, 48, False), (5, 48, False), (37, 2096, True), (5, 1040, True))]

K_ZERO = [Case(21, 72, 0, act, False, res=True, seed=5) for act in ("gelu", "swiglu")]

DETERMINISTIC = [Case(33, 200, 2096, "gelu", True, res=True, seed=4), Case(37, DEEP_SPLIT_N, 4112, "gelu", True, res=True, seed=6)]

# the quantiser: (N, K, ldw of the source in elements or None)
QUANT = [(1, 16, None), (73, 1040, None), (73, 528, 544), (8, 4112, None)]

TABLES = {"ROW_FRAGMENTS": ROW_FRAGMENTS, "K_TAILS_AND_SPLITS": K_TAILS_AND_SPLITS, "N_EDGES": N_EDGES,
          "N_EDGES_SPLIT": N_EDGES_SPLIT, "EVERY_ACTIVATION": EVERY_ACTIVATION, "STRIDES": STRIDES, "ROW_SLICE": ROW_SLICE,
          "ZERO_SCALE": ZERO_SCALE, "WORKSPACE": WORKSPACE, "DEEP_UNSPLIT": DEEP_UNSPLIT, "DEEP_SPLIT": DEEP_SPLIT,
          "POISONED": POISONED, "K_ZERO": K_ZERO, "DETERMINISTIC": DETERMINISTIC}

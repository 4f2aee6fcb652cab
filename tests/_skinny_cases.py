"""The shapes of the decode-step GEMM's GPU tests (tests/test_gpu_gemm_skinny.py), as plain tables: a helper module, not a conftest,
and free of torch so that the CPU suite can read it.

Which seams of csrc/gemm_skinny.hip a shape reaches is decided by the plan (gemm_skinny_plan.h): the row fragments MF =
ceil(M / 16), the slices of K (mio_gemm_skinny_splits / _slice) and, inside a slice, the chunks of the kernel's double-buffered
loop (mio_gemm_skinny_chunk_k: 256 k, SwiGLU 128).  Chunks 0 and 1 of a slice fill the two register sets and the two LDS buffers
for x; everything from chunk 2 on -- the reload of the first register set, the rewrite of an LDS buffer one barrier after it was
read, the exits after a reload at an odd and at an even count -- needs a slice of 3, 4 and 5 chunks.  The split target and the
chunk length are tuning values: tests/test_gemm_skinny_host.py::test_case_tables_reach_the_seams asks the loaded library for every
case's slices and chunks and fails, naming the cases, when a retune moves a table off what it is here to reach.

A case is (M, N, K, act, split, ...): split is what the plan must say (several slices or one), asserted on the CPU for every case
and again where the GPU test runs it."""
from typing import NamedTuple, Optional

ACTS = ["none", "gelu", "gelu_erf", "relu", "silu", "swiglu"]


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
    ldr: Optional[int] = None  # the residual as a view of rows this wide
    guard: bool = False        # the output as a view inside a filled buffer
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


# ---- one or two chunks per slice: fragments, tails, edges, activations, strides ------------------------------------------------------
ROW_FRAGMENTS = [Case(M, 72, 40, "gelu", False, res=True, seed=M) for M in (1, 5, 16, 17, 33, 48, 64)]

K_TAILS_AND_SPLITS = [Case(37, 72, 8, "none", False, res=True, seed=8),
                      Case(37, 72, 4104, "none", True, bias=False, res=True, seed=4104),
                      Case(64, 264, 1024, "none", True, res=True, seed=1024),
                      Case(3, 8, 2056, "none", True, res=True, seed=2056)]

N_EDGES = [Case(17, N, 264, "silu", False, guard=True, seed=N) for N in (1, 8, 15, 72, 1000)]


def _activation_calls(act, K, split):
    """With bias and a residual, with neither, and (SwiGLU) the gate's bias alone with a residual."""
    calls = [Case(21, 72, K, act, split, bias=True, res=True, seed=1),
             Case(21, 72, K, act, split, bias=False, res=False, bias_gate=False, seed=2)]
    if act == "swiglu":
        calls.append(Case(21, 72, K, act, split, bias=False, res=True, bias_gate=True, seed=3))
    return calls


EVERY_ACTIVATION = [c for act in ACTS for K, split in ((40, False), (1032, True)) for c in _activation_calls(act, K, split)]

STRIDES = [Case(37, 72, K, "gelu", split, res=True, ldx=K + 8, guard=True, ldr=88, seed=K) for K, split in ((40, False), (1032, True))]

WORKSPACE = [Case(19, 136, 1032, act, True, res=True, seed=9) for act in ("none", "swiglu")]

# ---- three and more chunks per slice -----------------------------------------------------------------------------------------------
# One slice: N 32776 is 513 column tiles, more workgroups than the split aims for at any target up to 512, so the whole K is one
# slice and K alone sets the chunk count.  The K below are column prefixes of one [DEEP_N, DEEP_LDW] weight (ldw != K).
DEEP_N, DEEP_LDW = 32776, 1032
DEEP_M = (5, 21, 37, 64)                                  # MF 1 .. 4, ragged and full
DEEP_K = {False: (520, 776, 1032), True: (264, 392, 520)}  # plain / SwiGLU: 3, 4 and 5 chunks (each K % 32 == 8: a tail step)
DEEP_UNSPLIT = [Case(M, DEEP_N, K, act, False, res=True, seed=K + M)
                for act in ("gelu", "swiglu") for K in DEEP_K[act == "swiglu"] for M in DEEP_M]

# Several slices, each of 3 or more chunks, not all of the same count.  Per MF a full and a ragged last fragment; M 1 is MF 1's
# ragged one.
DEEP_SPLIT_N = 8200
DEEP_SPLIT_M = (1, 16, 21, 32, 37, 48, 53, 64)
DEEP_SPLIT = ([Case(M, DEEP_SPLIT_N, 3080, "gelu", True, res=True, seed=M) for M in DEEP_SPLIT_M] +      # 3, 3, 3, 4 chunks
              # SwiGLU: 4, 4, 4, 5 chunks at K 2056; K 1544 (3, 3, 3, 4) cuts into four slices up to M 48 only
              [Case(M, DEEP_SPLIT_N, 1544 if M == 48 else 2056, "swiglu", True, res=True, seed=M) for M in DEEP_SPLIT_M])

# fp32 partials in rows of N % 4 != 0: the scalar path of both kernels (N_EDGES above is one slice and writes no partials)
N_EDGES_SPLIT = [Case(17, N, 1032, act, True, guard=True, seed=N) for act in ("silu", "swiglu") for N in (1, 15, 63, 71, 1001)]

# SwiGLU at every count of row fragments, through either kernel's epilogue, with both biases and the residual and with none
SWIGLU_FRAGMENTS = [Case(M, 72, K, "swiglu", split, bias=full, res=full, bias_gate=full, seed=M + full)
                    for M in (5, 16, 21, 37, 64) for K, split in ((40, False), (1032, True)) for full in (True, False)]

# operands inside NaN-filled buffers (test_poisoned_paddings): everything next to what the kernel may read is poison
POISONED = [Case(M, 72, K, act, split, res=True, ldx=K + 24, ldr=88, guard=True, seed=M + K)
            for act in ("gelu", "swiglu") for M in (37, 5) for K, split in ((40, False), (1032, True))]
POISONED_LDW_PAD = 16  # w and w_gate rows K + 16 apart

K_ZERO = [Case(21, 72, 0, act, False, res=True, seed=5) for act in ("gelu", "swiglu")]

DETERMINISTIC = [Case(33, 200, 2056, "gelu", True, res=True, seed=4), Case(37, DEEP_SPLIT_N, 3080, "gelu", True, res=True, seed=6)]

TABLES = {"ROW_FRAGMENTS": ROW_FRAGMENTS, "K_TAILS_AND_SPLITS": K_TAILS_AND_SPLITS, "N_EDGES": N_EDGES,
          "EVERY_ACTIVATION": EVERY_ACTIVATION, "STRIDES": STRIDES, "WORKSPACE": WORKSPACE, "DEEP_UNSPLIT": DEEP_UNSPLIT,
          "DEEP_SPLIT": DEEP_SPLIT, "N_EDGES_SPLIT": N_EDGES_SPLIT, "SWIGLU_FRAGMENTS": SWIGLU_FRAGMENTS, "POISONED": POISONED,
          "K_ZERO": K_ZERO, "DETERMINISTIC": DETERMINISTIC}

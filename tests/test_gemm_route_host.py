"""CPU-only tests of the GEMM route query: mio_gemm_route names the kernel every benchmark GEMM takes, each rule of
csrc/gemm_route.h flips on exactly its boundary, ops.gemm_route / ops.fused_mlp_route read the same shapes the launches do,
and mio_gemm_ln_ok refuses a LayerNorm consumer wider than the weights mio_ln_fold_weight prepares (K > 8192)."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIDE_MAX = 0x7fffffff // 512 // 8 * 8  # the longest row stride (elements, multiple of 8) the 32-bit per-tile offsets take


def _lib():
    from mio import _lib
    return _lib


def _route(M, N, K, ldx=None, ldw=None, ldy=None, ldr=0, act=0, res=False, w=0, fold_in=False, stats_out=False):
    L = _lib()
    r = L.lib.mio_gemm_route(M, N, K, K if ldx is None else ldx, K if ldw is None else ldw, N if ldy is None else ldy,
                             (N if ldr == 0 else ldr) if res else 0, act, int(res), w, int(fold_in), int(stats_out))
    return L.GEMM_ROUTES[r] if r >= 0 else None


def _err():
    return _lib().lib.mio_last_error().decode()


def test_gemm_route_symbol_and_table_match_header():
    L = _lib()
    assert "mio_gemm_route" in L.EXPORTS and len(L.lib.mio_gemm_route.argtypes) == 12
    assert L.lib.mio_version() == 106  # additive: the ABI version stays
    hdr = open(os.path.join(ROOT, "include", "mio_hip.h")).read()
    enum = {int(v): k.lower() for k, v in re.findall(r"MIO_GEMM_ROUTE_([A-Z0-9_]+) = (\d+)", hdr)}
    assert enum == L.GEMM_ROUTES


C2_M, C5_M = 8 * 4096, 8 * 4096
NONE, GELU, SWIGLU = 0, 1, 5
# (M, N, K, act, residual, weight layout, fold_in, stats_out) -> route: every GEMM of the benchmark stacks
BENCH = {
    "c2_qkv_col_scale": ((C2_M, 3072, 1024, NONE, False, 1, False, False), "p8w"),
    "c2_qkv_ln_fold": ((C2_M, 3072, 1024, NONE, False, 1, True, False), "p8w_fold"),
    "c2_out_proj": ((C2_M, 1024, 1024, NONE, True, 1, False, False), "p8w_res"),
    "c2_out_proj_stats": ((C2_M, 1024, 1024, NONE, True, 1, False, True), "p8w_stats"),
    "c2_fc1": ((C2_M, 4096, 1024, GELU, False, 1, False, False), "p8w"),
    "c2_fc1_ln_fold": ((C2_M, 4096, 1024, GELU, False, 1, True, False), "p8w_fold"),
    "c2_fc2": ((C2_M, 1024, 4096, NONE, True, 1, False, False), "p8w_res"),
    "c2_fc2_stats": ((C2_M, 1024, 4096, NONE, True, 1, False, True), "p8w_stats"),
    "c2_swiglu_fc1": ((C2_M, 4096, 1024, SWIGLU, False, 2, False, False), "p8w_glu"),
    "c2_swiglu_fc1_ln_fold": ((C2_M, 4096, 1024, SWIGLU, False, 2, True, False), "p8w_glu_fold"),
    "c5_qkv": ((C5_M, 3 * 1280, 1280, NONE, False, 1, False, False), "p8w"),
    "c5_q_ln_fold": ((C5_M, 1280, 1280, NONE, False, 1, True, False), "p8w_fold"),
    "c5_out_proj_stats": ((C5_M, 1280, 1280, NONE, True, 1, False, True), "p8w_stats"),
    "c5_fc1": ((C5_M, 5120, 1280, GELU, False, 1, False, False), "p8w"),
    "c5_fc1_ln_fold": ((C5_M, 5120, 1280, GELU, False, 1, True, False), "p8w_fold"),
    "c5_fc2": ((C5_M, 1280, 5120, NONE, True, 1, False, False), "p8w_res"),
    "c5_fc2_stats": ((C5_M, 1280, 5120, NONE, True, 1, False, True), "p8w_stats"),
    # the same GEMMs on plain weights (blocked weights off): the persistent kernel still
    "c2_qkv_plain": ((C2_M, 3072, 1024, NONE, False, 0, False, False), "p8w"),
    "c2_fc2_plain": ((C2_M, 1024, 4096, NONE, True, 0, False, False), "p8w_res"),
}


@pytest.mark.parametrize("case", sorted(BENCH))
def test_gemm_route_benchmark_shapes(case):
    (M, N, K, act, res, w, fold, stats), want = BENCH[case]
    assert _route(M, N, K, act=act, res=res, w=w, fold_in=fold, stats_out=stats) == want, _err()


def test_gemm_route_tile_count_boundary():
    # 256x256 tiles: 255 of them -> 128x128; 256 -> the persistent kernel (one row more than 255 row tiles also makes 256)
    assert _route(255 * 256, 256, 1024) == "t128"
    assert _route(256 * 256, 256, 1024) == "p8w"
    assert _route(255 * 256 + 1, 256, 1024) == "p8w"
    assert _route(16 * 256, 16 * 256 - 248, 1024) == "p8w"     # N ragged by 248: still 16 column tiles
    assert _route(16 * 256, 15 * 256 + 8, 1024) == "p8w"       # N ragged by 8: 16 column tiles
    assert _route(16 * 256, 15 * 256, 1024) == "t128"          # 240 tiles
    assert _route(1, 65536, 1024) == "p8w" and _route(1, 65536 - 256, 1024) == "t128"  # one row tile
    assert _route(65536, 8, 1024) == "p8w" and _route(65536 - 256, 8, 1024) == "t128"  # one column tile
    assert _route(0, 1024, 1024) == "empty"


def test_gemm_route_k_rules():
    M, N = 256 * 16, 256 * 16  # 256 tiles
    assert _route(M, N, 96) == "t256" and _route(M, N, 128) == "p8w"  # four K-tiles of 32 at least
    assert _route(M, N, 64) == "t256" and _route(M, N, 8) == "t256" and _route(M, N, 40) == "t256"
    assert _route(M, N, 264) == "t256" and _route(M, N, 256) == "p8w"  # K % 32
    assert _route(M, N, 136) == "t256" and _route(M, N, 160) == "p8w"
    for act in range(5):
        assert _route(M, N, 264, act=act) == "t256" and _route(M, N, 264, act=act, res=True) == "t256"
        assert _route(M, N, 256, act=act, res=True) == "p8w_res"
    assert _route(255 * 256, 256, 40) == "t128"  # below 256 tiles K does not matter


def test_gemm_route_stride_limit():
    M, N, K = 256 * 16, 256 * 16, 1024
    big = STRIDE_MAX + 8
    assert _route(M, N, K, ldx=STRIDE_MAX) == "p8w" and _route(M, N, K, ldx=big) == "t256"
    assert _route(M, N, K, ldw=STRIDE_MAX) == "p8w" and _route(M, N, K, ldw=big) == "t256"
    assert _route(M, N, K, ldy=STRIDE_MAX) == "p8w" and _route(M, N, K, ldy=big) == "t256"
    assert _route(M, N, K, res=True, ldr=STRIDE_MAX) == "p8w_res" and _route(M, N, K, res=True, ldr=big) == "t256"
    assert _route(M, N, K, ldr=big) == "p8w"  # no residual: its stride is not read
    # the blocked-weight entry points refuse such strides instead
    assert _route(M, N, K, ldx=big, w=1) is None and "row stride" in _err()


def test_gemm_route_swiglu_rules():
    M = 256 * 16
    assert _route(M, 2048, 1024, act=SWIGLU) == "glu_t256x128"          # 16 x 16 tiles of 256 x 128
    assert _route(M, 2048 - 8, 1024, act=SWIGLU) == "glu_t256x128"      # ragged: still 16 column tiles
    assert _route(M, 1920, 1024, act=SWIGLU) == "glu_t128x64"           # 240
    assert _route(M, 4096 + 8, 40, act=SWIGLU) == "glu_t256x128"        # no K rule for the gated 256x128 kernel
    assert _route(37, 72, 40, act=SWIGLU) == "glu_t128x64"
    assert _route(M, 2048, 1024, act=SWIGLU, w=1) is None               # no plain blocked weight for SwiGLU
    assert _route(M, 2048, 1024, act=NONE, w=2) is None                 # the interleaved weight is SwiGLU's


def test_gemm_route_refusals():
    M = 256 * 16
    assert _route(M, 1020, 1024) is None and "multiples of 8" in _err()
    assert _route(M, 1024, 1024, ldx=1000) is None and "strides" in _err()
    assert _route(M, 1024, 1024, act=6) is None and "activation" in _err()
    assert _route(M, 1024, 1024, w=3) is None
    assert _route(M, 1024, 1024, fold_in=True) is None and "blocked weight" in _err()
    assert _route(1024, 1024, 1024, w=1) is None and "blocked-weight" in _err()  # 16 tiles
    assert _route(C2_M, 1024, 1024, w=1, fold_in=True, res=True) is None          # the consumer takes no residual
    assert _route(C2_M, 1024, 1024, w=1, stats_out=True) is None                   # the producer is the residual epilogue


def test_gemm_ln_ok_refuses_fold_beyond_the_prepared_weight_width():
    """mio_ln_fold_weight prepares rows of at most 8192: a consumer with a wider K used to pass mio_gemm_ln_ok, so a model
    chose the folded path and its first forward raised in the weight preparation instead of falling back."""
    L = _lib()
    M = 8 * 4096
    assert L.lib.mio_gemm_ln_ok(M, 8192, 8192, NONE, 1, 0) == 1
    assert L.lib.mio_gemm_ln_ok(M, 8192, 8192 + 256, NONE, 1, 0) == 0
    assert L.lib.mio_gemm_ln_ok(M, 8192, 16384, GELU, 1, 0) == 0
    assert L.lib.mio_gemm_ln_ok(M, 8192, 8192 + 256, SWIGLU, 1, 0) == 0
    assert L.lib.mio_gemm_ln_ok(M, 8192, 8192 + 256, SWIGLU, 0, 0) == 1  # the gated stage without the fold is not limited
    assert L.lib.mio_gemm_ln_ok(M, 8192 + 256, 8192, NONE, 0, 1) == 1    # the producer is not limited either
    assert _route(M, 8192, 8192 + 256, w=1, fold_in=True) is None and "mio_gemm_ln_ok" in _err()
    from mio import ops
    assert not ops.gemm_ln_ok(M, 8192, 8192 + 256, "none", fold_in=True)


def _meta(*shape, dtype=torch.bfloat16):
    return torch.empty(*shape, dtype=dtype, device="meta")


def test_ops_gemm_route_reads_the_call():
    from mio import ops
    x, w = _meta(37, 40), _meta(72, 40)
    assert ops.gemm_route(x, w) == "t128"
    assert ops.gemm_route(_meta(0, 40), w) == "empty"
    M, N, K = 256 * 16, 256 * 16, 1024
    x, w, r = _meta(M, K), _meta(N, K), _meta(M, N)
    wb = _meta(N, K)
    assert ops.gemm_route(x, w, activation="gelu") == "p8w"
    assert ops.gemm_route(x, w, residual=r) == "p8w_res"
    assert ops.gemm_route(x, w, residual=r, w_blocked=wb) == "p8w_res"
    assert ops.gemm_route(x, w, w_blocked=wb, col_scale=(0, N, 0.5)) == "p8w"
    # x as a view of rows 4 Mi elements apart: the generic 256x256 kernel (gemm_bias_act keeps the plain weight then)
    xs = torch.empty(M, STRIDE_MAX + 8, dtype=torch.bfloat16, device="meta")[:, :K]
    assert ops.gemm_route(xs, w) == "t256" and ops.gemm_route(xs, w, w_blocked=wb) == "t256"
    assert ops.gemm_route(_meta(M, 96), _meta(N, 96), activation="relu") == "t256"
    assert ops.gemm_route(x, w, activation="swiglu", w_gate=w) == "glu_t256x128"
    # the gemm_ln signature (keyword-only M, N, K)
    st = _meta(4, 65536, 2, dtype=torch.float32)
    assert ops.gemm_route(x, wb, None, M=M, N=N, K=K, ln_stats=st) == "p8w_fold"
    assert ops.gemm_route(x, wb, None, M=M, N=N, K=K, residual=r, stats_out=True) == "p8w_stats"
    assert ops.gemm_route(x, wb, None, "swiglu", M=M, N=N, K=K) == "p8w_glu"
    with pytest.raises(ValueError):
        ops.gemm_route(_meta(1024, K), wb, None, M=1024, N=N, K=K, residual=r, stats_out=True)


def test_ops_fused_mlp_route():
    from mio import ops
    M, d, I = 8 * 4096, 1024, 4096
    x, w1, w2, r = _meta(8, 4096, d), _meta(I, d), _meta(d, I), _meta(8, 4096, d)
    b1, b2 = _meta(I), _meta(d)
    assert ops.fused_mlp_route(x, w1, b1, w2, b2, "gelu", residual=r, fc1_blocked=w1, fc2_blocked=w2) == \
        {"path": "blocked", "stage1": "p8w", "stage2": "p8w_res"}
    assert ops.fused_mlp_route(x, w1, b1, w2, b2, "gelu") == {"path": "blocked", "stage1": "p8w", "stage2": "p8w"}
    g = _meta(2 * I, d)
    assert ops.fused_mlp_route(x, w1, b1, w2, b2, "swiglu", w1, b1, residual=r, fc1_blocked=g, fc2_blocked=w2) == \
        {"path": "blocked", "stage1": "p8w_glu", "stage2": "p8w_res"}
    # SwiGLU on plain weights: two launches of the gated 256x128 kernel and the persistent one
    assert ops.fused_mlp_route(x, w1, b1, w2, b2, "swiglu", w1, b1) == \
        {"path": "two_launch", "stage1": "glu_t256x128", "stage2": "p8w"}
    xs = _meta(1, 300, 256)
    assert ops.fused_mlp_route(xs, _meta(1024, 256), None, _meta(256, 1024), None, "relu", residual=xs) == \
        {"path": "two_launch", "stage1": "t128", "stage2": "t128"}
    assert ops.fused_mlp_route(_meta(1, 0, 256), _meta(1024, 256), None, _meta(256, 1024), None, "silu") == \
        {"path": "two_launch", "stage1": "empty", "stage2": "empty"}


def test_gemm_bias_act_with_no_rows_takes_null_operands():
    """M == 0 (route "empty"): x and y hold no element, and torch hands an empty tensor over as a null pointer; the entry point
    used to refuse that before it reached its own M == 0 return."""
    L = _lib()
    W = 1 << 20  # a fake aligned weight address: nothing is launched, nothing dereferenced
    assert L.lib.mio_gemm_bias_act(None, W, None, None, None, None, None, 0, 128, 64, 64, 64, 128, 0, 1, 0, None) == 0, _err()
    assert L.lib.mio_gemm_bias_act(None, None, None, None, None, None, None, 0, 128, 64, 64, 64, 128, 0, 1, 0, None) != 0
    assert L.lib.mio_gemm_bias_act(None, W, None, None, None, None, None, 5, 128, 64, 64, 64, 128, 0, 1, 0, None) != 0

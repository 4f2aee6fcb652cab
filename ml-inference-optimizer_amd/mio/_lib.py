"""ctypes binding of libmio_hip.so (the C ABI declared in include/mio_hip.h).

There is no fallback: if the shared library is missing or a symbol is absent, importing this
module raises.  PyTorch is only used by the callers for device memory and streams.
"""
from __future__ import annotations

import ctypes as C
import os

# PyTorch must be loaded first: it ships its own HIP runtime (torch/lib/libamdhip64.so, SONAME
# libamdhip64.so.7).  With it already mapped, libmio_hip.so's NEEDED libamdhip64.so.7 binds to that same
# runtime, so torch's streams/events/allocations and our launches live in ONE HIP runtime.  (Loaded the other
# way round, /opt/rocm's copy would be pulled in first and the process would hold two runtimes.)
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
# MIO_LIB_DBG=1 (tools/ only): the diagnostic build (`make dbg`), which carries the A/B switches and the in-kernel
# stamp instantiations; the product library reads no environment variable and has neither.
LIB_PATH = os.path.join(_HERE, "libmio_hip_dbg.so" if os.environ.get("MIO_LIB_DBG") == "1" else "libmio_hip.so")

MIO_BF16, MIO_FP16 = 0, 1
MIO_FP32 = 2  # mio_sample_tokens' logits only
ACT_NONE, ACT_GELU_TANH, ACT_GELU_ERF, ACT_RELU, ACT_SILU, ACT_SWIGLU = range(6)
MASK_NONE, MASK_KEEP_U8, MASK_ADD_F32 = range(3)
# mio_fa3_route_t: the kernel mio_fa3_fwd launches (include/mio_hip.h)
FA3_ROUTES = {
    0: "empty",
    1: "fwd5",
    2: "fwd5_kpre",
    3: "fwd5_kpre_carry",
    4: "fwd5_kpre_oblk",
    5: "fwd3",
    6: "fwd3_kpre",
    7: "fwd1",
    8: "fwd1_keep",
    9: "fwd1_add",
}
# mio_fa3_varlen_route_t: the kernel mio_fa3_fwd_varlen launches (a table of its own: FA3_ROUTES is mio_fa3_fwd's)
FA3_VARLEN_ROUTES = {
    0: "empty",
    1: "fwd5",
    2: "fwd3",
}
# mio_fa3_paged_route_t: the kernel mio_fa3_fwd_paged launches
FA3_PAGED_ROUTES = {
    0: "empty",
    1: "fwd5",
    2: "fwd3",
}
# mio_decode_route_t: the kernel mio_fa3_decode_paged(_window) launches
DECODE_ROUTES = {
    0: "head",
    1: "rows",
    2: "gqa",
}

# mio_gemm_route_t: the kernel a GEMM launch takes (include/mio_hip.h, csrc/gemm_route.h)
GEMM_ROUTES = {
    0: "empty",
    1: "t128",
    2: "t256",
    3: "p8w",
    4: "p8w_res",
    5: "p8w_fold",
    6: "p8w_stats",
    7: "glu_t128x64",
    8: "glu_t256x128",
    9: "p8w_glu",
    10: "p8w_glu_fold",
}
# weight layouts mio_gemm_route takes
W_PLAIN, W_BLOCKED, W_GLU = range(3)

# every symbol include/mio_hip.h declares
EXPORTS = (
    "mio_version",
    "mio_last_error",
    "mio_fa3_fwd",
    "mio_fa3_k_prescaled_ok",
    "mio_fa3_o_blocked_ok",
    "mio_fa3_route",
    "mio_fa3_fwd_varlen",
    "mio_fa3_varlen_route",
    "mio_fa3_fwd_paged",
    "mio_fa3_paged_route",
    "mio_fa3_fwd_window",
    "mio_fa3_route_window",
    "mio_fa3_fwd_varlen_window",
    "mio_fa3_varlen_route_window",
    "mio_fa3_fwd_paged_window",
    "mio_fa3_paged_route_window",
    "mio_attn_merge",
    "mio_gemm_bias_act",
    "mio_fused_mlp_workspace_bytes",
    "mio_fused_mlp_fwd",
    "mio_weight_blocked_bytes",
    "mio_weight_block",
    "mio_gemm_blocked_weight_ok",
    "mio_gemm_bias_act_bw",
    "mio_gemm_col_scale_ok",
    "mio_gemm_bias_act_bw_cs",
    "mio_fused_mlp_blocked_weight_ok",
    "mio_fused_mlp_fwd_bw",
    "mio_weight_blocked_glu_bytes",
    "mio_weight_block_glu",
    "mio_fused_mlp_glu_fwd_bw",
    "mio_gemm_route",
    "mio_gemm_skinny_workspace_bytes",
    "mio_gemm_skinny_splits",
    "mio_gemm_skinny_slice",
    "mio_gemm_skinny_chunk_k",
    "mio_gemm_skinny_ok",
    "mio_gemm_skinny",
    "mio_weight_quant_w8",
    "mio_gemm_skinny_w8_workspace_bytes",
    "mio_gemm_skinny_w8_splits",
    "mio_gemm_skinny_w8_slice",
    "mio_gemm_skinny_w8_chunk_k",
    "mio_gemm_skinny_w8_depth",
    "mio_gemm_skinny_w8_ok",
    "mio_gemm_skinny_w8",
    "mio_layernorm_fwd_bx",
    "mio_ln_stats_bytes",
    "mio_gemm_ln_ok",
    "mio_ln_fold_weight",
    "mio_gemm_ln_bw",
    "mio_ln_stats_reduce",
    "mio_layernorm_fwd",
    "mio_gemm_rms_bw",
    "mio_rmsnorm_fwd",
    "mio_fa3_decode_workspace_bytes",
    "mio_fa3_decode_paged",
    "mio_fa3_decode_paged_window",
    "mio_fa3_decode_window_route",
    "mio_reshape_and_cache",
    "mio_reshape_and_cache_varlen",
    "mio_reshape_and_cache_kv8",
    "mio_reshape_and_cache_varlen_kv8",
    "mio_fa3_decode_paged_kv8",
    "mio_fa3_decode_kv8_route",
    "mio_fa3_fwd_paged_kv8",
    "mio_fa3_paged_kv8_route",
    "mio_rope_and_cache_varlen",
    "mio_rope_and_cache_varlen_kv8",
    "mio_rope_rows",
    "mio_qknorm_rope_and_cache_varlen",
    "mio_qknorm_rope_and_cache_varlen_kv8",
    "mio_qknorm_rope_rows",
    "mio_sample_tokens",
    "mio_moe_route",
    "mio_moe_up_splits",
    "mio_moe_up_workspace_bytes",
    "mio_moe_down_splits",
    "mio_moe_down_workspace_bytes",
    "mio_moe_up",
    "mio_moe_down",
)


class FaParams(C.Structure):
    """mio_fa3_fwd_params_t"""

    _fields_ = [
        ("q", C.c_void_p),
        ("k", C.c_void_p),
        ("v", C.c_void_p),
        ("o", C.c_void_p),
        ("lse", C.c_void_p),
        ("o_acc", C.c_void_p),
        ("mask", C.c_void_p),
        ("q_stride", C.c_int64 * 3),
        ("k_stride", C.c_int64 * 3),
        ("v_stride", C.c_int64 * 3),
        ("o_stride", C.c_int64 * 3),
        ("mask_stride", C.c_int64 * 4),
        ("B", C.c_int32),
        ("Sq", C.c_int32),
        ("Sk", C.c_int32),
        ("H", C.c_int32),
        ("Hkv", C.c_int32),
        ("D", C.c_int32),
        ("dtype", C.c_int32),
        ("causal", C.c_int32),
        ("mask_kind", C.c_int32),
        ("carry_in", C.c_int32),
        ("q_offset", C.c_int32),
        ("k_offset", C.c_int32),
        ("softmax_scale", C.c_float),
        ("k_prescaled", C.c_int32),
        ("o_blocked", C.c_int32),
    ]


class FaVarlenParams(C.Structure):
    """mio_fa3_varlen_params_t"""

    _fields_ = [
        ("q", C.c_void_p),
        ("k", C.c_void_p),
        ("v", C.c_void_p),
        ("o", C.c_void_p),
        ("lse", C.c_void_p),
        ("cu_seqlens_q", C.c_void_p),
        ("cu_seqlens_k", C.c_void_p),
        ("q_stride", C.c_int64 * 2),
        ("k_stride", C.c_int64 * 2),
        ("v_stride", C.c_int64 * 2),
        ("o_stride", C.c_int64 * 2),
        ("B", C.c_int32),
        ("total_q", C.c_int32),
        ("total_k", C.c_int32),
        ("max_seqlen_q", C.c_int32),
        ("max_seqlen_k", C.c_int32),
        ("H", C.c_int32),
        ("Hkv", C.c_int32),
        ("D", C.c_int32),
        ("dtype", C.c_int32),
        ("causal", C.c_int32),
        ("softmax_scale", C.c_float),
    ]


class FaPagedParams(C.Structure):
    """mio_fa3_paged_params_t"""

    _fields_ = [
        ("q", C.c_void_p),
        ("k_cache", C.c_void_p),
        ("v_cache", C.c_void_p),
        ("o", C.c_void_p),
        ("lse", C.c_void_p),
        ("cu_seqlens_q", C.c_void_p),
        ("seqused_k", C.c_void_p),
        ("block_tables", C.c_void_p),
        ("q_stride", C.c_int64 * 2),
        ("o_stride", C.c_int64 * 2),
        ("B", C.c_int32),
        ("total_q", C.c_int32),
        ("max_seqlen_q", C.c_int32),
        ("max_seqlen_k", C.c_int32),
        ("H", C.c_int32),
        ("Hkv", C.c_int32),
        ("D", C.c_int32),
        ("num_blocks", C.c_int32),
        ("num_layers", C.c_int32),
        ("layer_idx", C.c_int32),
        ("block_size", C.c_int32),
        ("max_blocks_per_seq", C.c_int32),
        ("dtype", C.c_int32),
        ("causal", C.c_int32),
        ("softmax_scale", C.c_float),
    ]


def _load() -> C.CDLL:
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: the HIP extension is not built. Run `make -C ml-inference-optimizer_amd/csrc` "
            "(or __graft_entry__.build()). There is no CPU or PyTorch fallback for this path."
        )
    lib = C.CDLL(LIB_PATH)
    missing = [s for s in EXPORTS if not hasattr(lib, s)]
    if missing:
        raise ImportError(f"{LIB_PATH} lacks symbols {missing}; rebuild the extension")
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    lib.mio_version.restype = i32
    lib.mio_last_error.restype = C.c_char_p
    lib.mio_fa3_fwd.argtypes = [C.POINTER(FaParams), vp]
    lib.mio_fa3_fwd.restype = i32
    lib.mio_fa3_k_prescaled_ok.argtypes = [C.POINTER(FaParams)]
    lib.mio_fa3_k_prescaled_ok.restype = i32
    lib.mio_fa3_o_blocked_ok.argtypes = [C.POINTER(FaParams)]
    lib.mio_fa3_o_blocked_ok.restype = i32
    lib.mio_fa3_route.argtypes = [C.POINTER(FaParams)]
    lib.mio_fa3_route.restype = i32
    lib.mio_fa3_fwd_varlen.argtypes = [C.POINTER(FaVarlenParams), vp]
    lib.mio_fa3_fwd_varlen.restype = i32
    lib.mio_fa3_varlen_route.argtypes = [C.POINTER(FaVarlenParams)]
    lib.mio_fa3_varlen_route.restype = i32
    lib.mio_fa3_fwd_paged.argtypes = [C.POINTER(FaPagedParams), vp]
    lib.mio_fa3_fwd_paged.restype = i32
    lib.mio_fa3_paged_route.argtypes = [C.POINTER(FaPagedParams)]
    lib.mio_fa3_paged_route.restype = i32
    for name, params in (("mio_fa3_fwd_window", FaParams), ("mio_fa3_fwd_varlen_window", FaVarlenParams),
                         ("mio_fa3_fwd_paged_window", FaPagedParams)):
        getattr(lib, name).argtypes = [C.POINTER(params), i32, i32, vp]
        getattr(lib, name).restype = i32
    for name, params in (("mio_fa3_route_window", FaParams), ("mio_fa3_varlen_route_window", FaVarlenParams),
                         ("mio_fa3_paged_route_window", FaPagedParams)):
        getattr(lib, name).argtypes = [C.POINTER(params), i32, i32]
        getattr(lib, name).restype = i32
    lib.mio_attn_merge.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]
    lib.mio_attn_merge.restype = i32
    lib.mio_gemm_bias_act.argtypes = [vp, vp, vp, vp, vp, vp, vp, i64, i32, i32, i64, i64, i64, i64, i32, i32, vp]
    lib.mio_gemm_bias_act.restype = i32
    # the decode-step GEMM's host queries, one family per weight form: the same signatures under both names
    for fam in ("mio_gemm_skinny", "mio_gemm_skinny_w8"):
        for query, restype in (("workspace_bytes", C.c_size_t), ("splits", i32), ("ok", i32)):
            getattr(lib, f"{fam}_{query}").argtypes = [i64, i32, i32, i32]
            getattr(lib, f"{fam}_{query}").restype = restype
        getattr(lib, f"{fam}_slice").argtypes = [i64, i32, i32, i32, i32, C.POINTER(i32), C.POINTER(i32)]
        getattr(lib, f"{fam}_slice").restype = i32
    for name in ("mio_gemm_skinny_chunk_k", "mio_gemm_skinny_w8_chunk_k", "mio_gemm_skinny_w8_depth"):
        getattr(lib, name).argtypes = [i32]
        getattr(lib, name).restype = i32
    lib.mio_gemm_skinny.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i64, i32, i32, i64, i64, i64, i64, i32, i32, vp]
    lib.mio_gemm_skinny.restype = i32
    lib.mio_weight_quant_w8.argtypes = [vp, i64, vp, i64, vp, i32, i32, i32, vp]
    lib.mio_weight_quant_w8.restype = i32
    lib.mio_gemm_skinny_w8.argtypes = [vp] * 10 + [i64, i32, i32, i64, i64, i64, i64, i32, i32, vp]
    lib.mio_gemm_skinny_w8.restype = i32
    lib.mio_fused_mlp_workspace_bytes.argtypes = [i64, i32, i32, i32]
    lib.mio_fused_mlp_workspace_bytes.restype = C.c_size_t
    lib.mio_fused_mlp_fwd.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i32, i32, i32, i32, vp]
    lib.mio_fused_mlp_fwd.restype = i32
    lib.mio_weight_blocked_bytes.argtypes = [i32, i32]
    lib.mio_weight_blocked_bytes.restype = C.c_size_t
    lib.mio_weight_block.argtypes = [vp, i64, vp, i32, i32, i32, vp]
    lib.mio_weight_block.restype = i32
    lib.mio_gemm_blocked_weight_ok.argtypes = [i64, i32, i32, i32]
    lib.mio_gemm_blocked_weight_ok.restype = i32
    lib.mio_gemm_bias_act_bw.argtypes = [vp, vp, vp, vp, vp, i64, i32, i32, i64, i64, i64, i32, i32, i32, vp]
    lib.mio_gemm_bias_act_bw.restype = i32
    lib.mio_gemm_col_scale_ok.argtypes = [i64, i32, i32, i32]
    lib.mio_gemm_col_scale_ok.restype = i32
    lib.mio_gemm_bias_act_bw_cs.argtypes = [vp, vp, vp, vp, i64, i32, i32, i64, i64, i32, i32, i32, i32, i32, f32, vp]
    lib.mio_gemm_bias_act_bw_cs.restype = i32
    lib.mio_fused_mlp_blocked_weight_ok.argtypes = [i64, i32, i32, i32]
    lib.mio_fused_mlp_blocked_weight_ok.restype = i32
    lib.mio_fused_mlp_fwd_bw.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i64, i32, i32, i32, i32, i32, vp]
    lib.mio_fused_mlp_fwd_bw.restype = i32
    lib.mio_weight_blocked_glu_bytes.argtypes = [i32, i32]
    lib.mio_weight_blocked_glu_bytes.restype = C.c_size_t
    lib.mio_weight_block_glu.argtypes = [vp, vp, i64, vp, i32, i32, i32, vp]
    lib.mio_weight_block_glu.restype = i32
    lib.mio_fused_mlp_glu_fwd_bw.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i32, i32, i32, i32, vp]
    lib.mio_fused_mlp_glu_fwd_bw.restype = i32
    lib.mio_gemm_route.argtypes = [i64, i32, i32, i64, i64, i64, i64, i32, i32, i32, i32, i32]
    lib.mio_gemm_route.restype = i32
    lib.mio_ln_stats_bytes.argtypes = [i64, i32]
    lib.mio_ln_stats_bytes.restype = C.c_size_t
    lib.mio_gemm_ln_ok.argtypes = [i64, i32, i32, i32, i32, i32]
    lib.mio_gemm_ln_ok.restype = i32
    lib.mio_ln_fold_weight.argtypes = [vp, i64, vp, vp, vp, vp, vp, i32, i32, i32, vp]
    lib.mio_ln_fold_weight.restype = i32
    lib.mio_gemm_ln_bw.argtypes = [vp, vp, vp, vp, vp, vp, i64, i32, i32, i64, i64, i64, i32, i32, i32, vp, i32, f32, vp, i32, i32, f32, vp]
    lib.mio_ln_stats_reduce.argtypes = [vp, i32, vp, i32, i64, vp]
    lib.mio_ln_stats_reduce.restype = i32
    lib.mio_gemm_ln_bw.restype = i32
    lib.mio_gemm_rms_bw.argtypes = list(lib.mio_gemm_ln_bw.argtypes)
    lib.mio_gemm_rms_bw.restype = i32
    lib.mio_rmsnorm_fwd.argtypes = [vp, vp, vp, vp, vp, i64, i32, f32, f32, i32, i32, vp]
    lib.mio_rmsnorm_fwd.restype = i32
    lib.mio_layernorm_fwd.argtypes = [vp, vp, vp, vp, vp, vp, i64, i32, f32, f32, i32, vp]
    lib.mio_layernorm_fwd.restype = i32
    lib.mio_layernorm_fwd_bx.argtypes = [vp, vp, vp, vp, vp, vp, i64, i32, f32, f32, i32, vp]
    lib.mio_layernorm_fwd_bx.restype = i32
    lib.mio_fa3_decode_workspace_bytes.argtypes = [i32, i32, i32, i32, i32]
    lib.mio_fa3_decode_workspace_bytes.restype = C.c_size_t
    lib.mio_fa3_decode_paged.argtypes = [vp, vp, vp, vp, vp, vp, C.POINTER(i64), C.POINTER(i64), i32, i32, i32, i32,
                                         i32, i32, i32, i32, i32, i32, f32, i32, vp, vp]
    lib.mio_fa3_decode_paged.restype = i32
    for name in ("mio_fa3_decode_paged_window", "mio_fa3_decode_window_route"):
        getattr(lib, name).argtypes = [vp, vp, vp, vp, vp, vp, C.POINTER(i64), C.POINTER(i64), i32, i32, i32, i32, i32,
                                       i32, i32, i32, i32, i32, f32, i32, i32, i32, vp, vp]
        getattr(lib, name).restype = i32
    lib.mio_reshape_and_cache.argtypes = [vp, vp, vp, vp, vp, vp, C.POINTER(i64), C.POINTER(i64), i32, i32, i32, i32,
                                          i32, i32, i32, i32, vp]
    lib.mio_reshape_and_cache.restype = i32
    lib.mio_reshape_and_cache_varlen.argtypes = [vp, vp, vp, vp, vp, vp, vp, C.POINTER(i64), C.POINTER(i64), i32, i32,
                                                 i32, i32, i32, i32, i32, i32, i32, i32, vp]
    lib.mio_reshape_and_cache_varlen.restype = i32
    # fp8 (e4m3fn) cache: the 16-bit forms' arguments with the two scale pointers after v_cache
    lib.mio_reshape_and_cache_kv8.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(i64), C.POINTER(i64), i32, i32,
                                              i32, i32, i32, i32, i32, i32, vp]
    lib.mio_reshape_and_cache_kv8.restype = i32
    lib.mio_reshape_and_cache_varlen_kv8.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(i64),
                                                     C.POINTER(i64), i32, i32, i32, i32, i32, i32, i32, i32, i32, i32,
                                                     vp]
    lib.mio_reshape_and_cache_varlen_kv8.restype = i32
    for name in ("mio_fa3_decode_paged_kv8", "mio_fa3_decode_kv8_route"):
        getattr(lib, name).argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(i64), C.POINTER(i64), i32, i32, i32,
                                       i32, i32, i32, i32, i32, i32, i32, f32, i32, i32, vp, vp]
        getattr(lib, name).restype = i32
    lib.mio_fa3_fwd_paged_kv8.argtypes = [C.POINTER(FaPagedParams), vp, vp, i32, i32, vp]
    lib.mio_fa3_fwd_paged_kv8.restype = i32
    lib.mio_fa3_paged_kv8_route.argtypes = [C.POINTER(FaPagedParams), vp, vp, i32, i32]
    lib.mio_fa3_paged_kv8_route.restype = i32
    # rotary: q, q_out, key, value, caches, (fp8: the two scales,) block_tables, cu_seqlens_new, context_lengths, positions, cos,
    # sin, four (token, head) stride pairs, then the sizes
    p64 = C.POINTER(i64)
    lib.mio_rope_and_cache_varlen.argtypes = [vp] * 12 + [p64] * 4 + [i32] * 14 + [vp]
    lib.mio_rope_and_cache_varlen.restype = i32
    lib.mio_rope_and_cache_varlen_kv8.argtypes = [vp] * 14 + [p64] * 4 + [i32] * 14 + [vp]
    lib.mio_rope_and_cache_varlen_kv8.restype = i32
    lib.mio_rope_rows.argtypes = [vp] * 5 + [p64] * 2 + [i32] * 7 + [vp]
    lib.mio_rope_rows.restype = i32
    # QK-norm: the rotary forms' arguments with the norm weight(s) after sin and eps after dtype
    lib.mio_qknorm_rope_and_cache_varlen.argtypes = [vp] * 14 + [p64] * 4 + [i32] * 14 + [f32, vp]
    lib.mio_qknorm_rope_and_cache_varlen.restype = i32
    lib.mio_qknorm_rope_and_cache_varlen_kv8.argtypes = [vp] * 16 + [p64] * 4 + [i32] * 14 + [f32, vp]
    lib.mio_qknorm_rope_and_cache_varlen_kv8.restype = i32
    lib.mio_qknorm_rope_rows.argtypes = [vp] * 6 + [p64] * 2 + [i32] * 7 + [f32, vp]
    lib.mio_qknorm_rope_rows.restype = i32
    # sampling: logits, ld, temperature, top_k, top_p, min_p, u, tokens_out, kept_out, probs_out, ld_probs, B, V, dtype, stream
    lib.mio_sample_tokens.argtypes = [vp, i64] + [vp] * 8 + [i64, i32, i32, i32, vp]
    lib.mio_sample_tokens.restype = i32
    # mixture of experts: logits, ld, the five outputs, T, E, top_k, renormalize, dtype, stream
    lib.mio_moe_route.argtypes = [vp, i64] + [vp] * 5 + [i32] * 5 + [vp]
    lib.mio_moe_route.restype = i32
    # the grouped GEMMs' plan queries: T, top_k, E, N, K (up: and act)
    lib.mio_moe_up_splits.argtypes = [i32] * 6
    lib.mio_moe_up_splits.restype = i32
    lib.mio_moe_up_workspace_bytes.argtypes = [i32] * 6
    lib.mio_moe_up_workspace_bytes.restype = C.c_size_t
    lib.mio_moe_down_splits.argtypes = [i32] * 5
    lib.mio_moe_down_splits.restype = i32
    lib.mio_moe_down_workspace_bytes.argtypes = [i32] * 5
    lib.mio_moe_down_workspace_bytes.restype = C.c_size_t
    # x, w_up, b_up, w_gate, b_gate, expert_offsets, sorted_rows, h, workspace, T, top_k, E, I, d, ldx, ldw, expert_stride, ldh, act,
    # dtype, stream
    lib.mio_moe_up.argtypes = [vp] * 9 + [i32] * 5 + [i64] * 4 + [i32, i32, vp]
    lib.mio_moe_up.restype = i32
    # h, w_down, b_down, ids, weights, expert_offsets, row_pos, residual, y, workspace, T, top_k, E, d, I, ldh, ldw, expert_stride,
    # ldy, ldr, dtype, stream
    lib.mio_moe_down.argtypes = [vp] * 10 + [i32] * 5 + [i64] * 5 + [i32, vp]
    lib.mio_moe_down.restype = i32
    return lib


lib = _load()


def check(rc: int) -> None:
    """Non-zero C return -> RuntimeError(mio_last_error()); no silent fallback."""
    if rc != 0:
        raise RuntimeError(lib.mio_last_error().decode("utf-8", "replace"))

/*
 * mio_hip.h -- C ABI of libmio_hip.so, the MI355X (gfx950 / CDNA4) implementation of the
 * transformer-inference hot path of aslitaser/ml-inference-optimizer.
 *
 * Every entry point replaces one Python->Triton launch boundary of the reference (cited per
 * function as reference file:line).  Conventions:
 *   - plain C: pointers, sizes, strides; no C++ or torch types.
 *   - every function returns 0 on success, <0 on error; mio_last_error() gives the message
 *     (thread-local).  Nothing is allocated, no ownership changes hands: outputs and workspaces
 *     are caller-owned device buffers.
 *   - asynchronous on the given HIP stream (`stream` is a hipStream_t passed as void*); safe to
 *     call concurrently from several threads/streams; graph-capturable (no sync, no malloc).
 *   - strides are in ELEMENTS of the tensor's dtype.  The innermost (head_dim / feature)
 *     dimension must be contiguous (stride 1) and every row start must be 16-byte aligned.
 */
#ifndef MIO_HIP_H
#define MIO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIO_VERSION 106 /* 0.1.0 */

typedef enum { MIO_BF16 = 0, MIO_FP16 = 1, MIO_FP32 = 2 /* mio_sample_tokens' logits only */ } mio_dtype_t;

typedef enum {
  MIO_ACT_NONE = 0,
  MIO_ACT_GELU_TANH = 1, /* kernels/triton/mlp_kernels.py:144-161, kernels/mlp/fused_mlp.py:227-231 */
  MIO_ACT_GELU_ERF = 2,  /* kernels/triton/mlp_kernels.py:782-783, kernels/mlp/fused_mlp.py:162-163 */
  MIO_ACT_RELU = 3,      /* kernels/triton/mlp_kernels.py:233-414 */
  MIO_ACT_SILU = 4,      /* kernels/mlp/fused_mlp.py:166-167 */
  MIO_ACT_SWIGLU = 5     /* kernels/triton/mlp_kernels.py:417-641 */
} mio_act_t;

typedef enum {
  MIO_MASK_NONE = 0,
  MIO_MASK_KEEP_U8 = 1, /* 1 = attend, 0 -> score := -1e9  (flash_attention_kernels.py:257-273) */
  MIO_MASK_ADD_F32 = 2  /* score += max(mask, -1e30)       (attention_kernels.py:1565-1566)      */
} mio_mask_kind_t;

int mio_version(void);
const char* mio_last_error(void);

/* ------------------------------------------------------------------------------------------
 * FlashAttention-3 style tiled attention forward (prefill), online softmax, fp32 accumulators.
 * Replaces: triton_flash_attention -> _flash_attention_forward_kernel launch
 *           (kernels/triton/flash_attention_kernels.py:1291-1310; kernel :38-325) and
 *           triton_ring_attention_forward -> _ring_attention_forward_kernel launch
 *           (kernels/triton/attention_kernels.py:979-995; kernel :35-202).
 *
 * q [B,Sq,H,D], k/v [B,Sk,Hkv,D], o [B,Sq,H,D] given by (b, s, h) strides (d stride is 1), so
 * both the reference's seq-major [B,S,H,D] (flash) and head-major [B,H,S,D] (ring) layouts are
 * accepted.  H % Hkv == 0 (GQA: kv head = h / (H/Hkv), flash_attention.py:894-912).
 * D in [8,128], D % 8 == 0.
 *
 * causal: key position (k_offset + j) > query position (q_offset + i) is excluded.  Without a
 *   user mask excluded blocks are skipped (exact: the reference's -1e9 fill underflows to 0).
 * mask: kind KEEP_U8 (uint8) or ADD_F32 (float), addressed with 4 element strides
 *   (b, h, q, k); 0 strides broadcast.  With a user mask, causal-excluded keys get the
 *   reference's finite -1e9 fill (not -inf).  ADD_F32 entries below -1e30 (-inf,
 *   finfo(float32).min, finfo(bfloat16).min) count as -1e30: a key at the floor gets weight 0
 *   next to any key above it, and a row whose every key is at the floor -- also a row of
 *   -inf only -- gets the uniform average of its keys, as a finite fill gives in
 *   softmax(scores + mask); never NaN.  A keep-mask row with no kept key likewise averages
 *   every key (-1e9 fill).
 * lse (nullable): [B,H,Sq] fp32, natural-log softmax denominator (m + log l of
 *   flash_attention_kernels.py:308-325).  Rows with no visible key get lse=-inf, o=0.
 * Ring carry (nullable o_acc): fp32 [B,Sq,H,D] contiguous running output state.
 *   carry_in != 0: start from (o_acc, lse) instead of empty;  o_acc != NULL: the normalised
 *   fp32 output is also written to o_acc (and lse must be non-NULL).  `o` may be NULL when
 *   o_acc is given (intermediate ring steps).
 * Sk == 0: no key is read; o = 0, lse = -inf (carry_in: the carried state is written back).
 * Memory the launch does not own may hold anything, NaN bit patterns included, and does not influence the
 *   result -- here and in the varlen, paged and windowed forms below: the bytes between D and the head stride,
 *   heads / rows / batch entries of a larger buffer around q, k, v, o or the mask, and, without a user mask,
 *   every 64-key tile (counted from key 0) that holds no key visible to any query row < Sq; o / lse / o_acc
 *   are written at rows < Sq only (a blocked o: its padding rows past B*Sq stay untouched).
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  const void* q;
  const void* k;
  const void* v;
  void* o;
  float* lse;
  float* o_acc;
  const void* mask;
  int64_t q_stride[3]; /* b, s, h */
  int64_t k_stride[3];
  int64_t v_stride[3];
  int64_t o_stride[3];
  int64_t mask_stride[4]; /* b, h, q, k */
  int32_t B, Sq, Sk, H, Hkv, D;
  int32_t dtype;     /* mio_dtype_t */
  int32_t causal;    /* 0/1 */
  int32_t mask_kind; /* mio_mask_kind_t */
  int32_t carry_in;  /* 0/1 */
  int32_t q_offset, k_offset;
  float softmax_scale; /* > 0 */
  int32_t k_prescaled; /* 0/1: k already holds K * softmax_scale * log2(e), scaled in fp32 BEFORE its rounding to 16 bits
                          (mio_gemm_bias_act_bw col_scale: the epilogue of the projection that produced it).  Only for
                          launches mio_fa3_k_prescaled_ok() accepts; the kernel then skips the per-score multiply. */
  int32_t o_blocked;   /* 0/1: `o` is the [B*Sq, H*D] output in the blocked ACTIVATION layout of the GEMM entry points below
                          (ceil(B*Sq/256)*256 x H*D elements, o_stride ignored): the attention epilogue hands the output
                          projection contiguous K-tiles.  Only for launches mio_fa3_o_blocked_ok() accepts. */
} mio_fa3_fwd_params_t;

int mio_fa3_fwd(const mio_fa3_fwd_params_t* p, void* stream);
/* Which kernel mio_fa3_fwd launches for these parameters (nothing is launched or dereferenced; no device needed).
 * Returns a mio_fa3_route_t, or < 0 (mio_last_error()) where mio_fa3_fwd would refuse the arguments.  The rule: without a
 * user mask, Sq > 128, Sk > 0 and K / V rows within 4 GiB of their (batch, head) base, the pipelined kernels --
 * fa3_fwd5_kernel at padded head dim 64 (plain output; k_prescaled also with the ring carry or a blocked output),
 * fa3_fwd3_kernel otherwise (k_prescaled at padded head dim 96, plain output only); every other launch goes to
 * fa3_fwd_kernel, templated on the mask kind. */
typedef enum {
  MIO_FA3_ROUTE_INVALID = -1,
  MIO_FA3_ROUTE_EMPTY = 0,            /* Sq == 0: nothing to launch */
  MIO_FA3_ROUTE_FWD5 = 1,             /* fa3_fwd5_kernel, plain K (scale applied in fp32) */
  MIO_FA3_ROUTE_FWD5_KPRE = 2,        /* fa3_fwd5_kernel, k_prescaled */
  MIO_FA3_ROUTE_FWD5_KPRE_CARRY = 3,  /* fa3_fwd5_kernel, k_prescaled, (o_acc, lse) carry */
  MIO_FA3_ROUTE_FWD5_KPRE_OBLK = 4,   /* fa3_fwd5_kernel, k_prescaled, blocked output */
  MIO_FA3_ROUTE_FWD3 = 5,             /* fa3_fwd3_kernel, plain K (with or without the carry) */
  MIO_FA3_ROUTE_FWD3_KPRE = 6,        /* fa3_fwd3_kernel, k_prescaled */
  MIO_FA3_ROUTE_FWD1 = 7,             /* fa3_fwd_kernel, no user mask (Sq <= 128, Sk == 0, K / V spans >= 4 GiB) */
  MIO_FA3_ROUTE_FWD1_KEEP = 8,        /* fa3_fwd_kernel, KEEP_U8 mask */
  MIO_FA3_ROUTE_FWD1_ADD = 9          /* fa3_fwd_kernel, ADD_F32 mask */
} mio_fa3_route_t;
int32_t mio_fa3_route(const mio_fa3_fwd_params_t* p);
/* 1 iff a launch with these parameters (k_prescaled ignored) may set k_prescaled = 1: no user mask, Sq > 128, Sk > 0, K / V
 * rows within 4 GiB of their (batch, head) base, head dim <= 96; with the (o_acc, lse) ring carry (o_acc and lse given,
 * carry_in 0 / 1, o optional) only at head dim <= 64. */
int32_t mio_fa3_k_prescaled_ok(const mio_fa3_fwd_params_t* p);
/* 1 iff a launch with these parameters (o_blocked ignored) may set o_blocked = 1: a k_prescaled launch without the ring
 * carry at head dim <= 64 with (H * D) % 32 == 0. */
int32_t mio_fa3_o_blocked_ok(const mio_fa3_fwd_params_t* p);

/* ------------------------------------------------------------------------------------------
 * Packed variable-length attention forward (prefill of sequences of different lengths; the
 * form of flash-attn's flash_attn_varlen_func), on the pipelined kernels of routes FWD5 / FWD3.
 *
 * q [total_q,H,D], k/v [total_k,Hkv,D], o [total_q,H,D] given by (token, head) strides (d
 * stride is 1; k/v may be strided views into a fused QKV buffer).  Sequence b (0 <= b < B)
 * owns rows cu_seqlens_q[b] .. cu_seqlens_q[b+1]-1 of q / o and rows cu_seqlens_k[b] ..
 * cu_seqlens_k[b+1]-1 of k / v; cu_seqlens_* are int32 DEVICE arrays of B+1 entries, never
 * read on the host.  The kernel clamps every sequence into [0,total_q) / [0,total_k) and to
 * max_seqlen_q / max_seqlen_k: offsets that disagree with the totals give wrong numbers, never
 * an access outside the buffers.  Rows of o outside every sequence are not written.
 * causal: bottom-right aligned per sequence -- query i of sequence b sees key j iff
 *   j <= i + Lk_b - Lq_b (a dense mio_fa3_fwd call on that sequence with q_offset = Lk_b - Lq_b,
 *   k_offset = 0; chunked prefill against a contiguous prefix).  Rows with no visible key, and
 *   every row of a sequence with Lk_b == 0, get o = 0, lse = -inf.
 * lse (nullable): fp32 [H,total_q], natural-log softmax denominator.
 * H % Hkv == 0; D in [8,128], D % 8 == 0 (padded head dim 64: fa3_fwd5_kernel, 96 / 128:
 * fa3_fwd3_kernel); plain K, softmax_scale applied in fp32.  K / V rows of one sequence must span
 * less than 4 GiB: max_seqlen_k * k/v token stride * 2 < 2^32.  No host sync; graph-capturable.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  const void* q;
  const void* k;
  const void* v;
  void* o;
  float* lse;                  /* nullable, fp32 [H, total_q] */
  const int32_t* cu_seqlens_q; /* device, B+1 entries */
  const int32_t* cu_seqlens_k; /* device, B+1 entries */
  int64_t q_stride[2];         /* token, head */
  int64_t k_stride[2];
  int64_t v_stride[2];
  int64_t o_stride[2];
  int32_t B, total_q, total_k, max_seqlen_q, max_seqlen_k, H, Hkv, D;
  int32_t dtype;       /* mio_dtype_t */
  int32_t causal;      /* 0/1 */
  float softmax_scale; /* > 0 */
} mio_fa3_varlen_params_t;

int mio_fa3_fwd_varlen(const mio_fa3_varlen_params_t* p, void* stream);
/* Which kernel mio_fa3_fwd_varlen launches (nothing is launched or dereferenced; no device needed).  Returns a
 * mio_fa3_varlen_route_t, or < 0 (mio_last_error()) where mio_fa3_fwd_varlen would refuse the arguments. */
typedef enum {
  MIO_FA3_VARLEN_ROUTE_INVALID = -1,
  MIO_FA3_VARLEN_ROUTE_EMPTY = 0, /* B == 0 or total_q == 0: nothing to launch */
  MIO_FA3_VARLEN_ROUTE_FWD5 = 1,  /* fa3_fwd5_kernel's varlen form (padded head dim 64), plain K */
  MIO_FA3_VARLEN_ROUTE_FWD3 = 2   /* fa3_fwd3_kernel's varlen form (padded head dim 96 / 128), plain K */
} mio_fa3_varlen_route_t;
int32_t mio_fa3_varlen_route(const mio_fa3_varlen_params_t* p);

/* ------------------------------------------------------------------------------------------
 * Attention forward over the paged KV cache (chunked prefill, shared prefixes, multi-token
 * verify against a cached context), on the pipelined kernels of routes FWD5 / FWD3.
 *
 * q/o [total_q,H,D] packed as in mio_fa3_fwd_varlen (cu_seqlens_q, (token, head) strides, d
 * stride 1).  k_cache/v_cache [num_blocks, num_layers, block_size, Hkv, D] contiguous (the
 * layout of mio_fa3_decode_paged), read at layer_idx.  Sequence b sees keys 0 .. Lk_b-1,
 * Lk_b = min(seqused_k[b], max_seqlen_k, max_blocks_per_seq * block_size); key j lives in page
 * block_tables[b, j / block_size] at slot j % block_size.  cu_seqlens_q [B+1], seqused_k [B]
 * and block_tables [B, max_blocks_per_seq] are int32 DEVICE arrays, never read on the host.
 * The kernel clamps cu_seqlens_q as mio_fa3_fwd_varlen does, every logical block into
 * [0, max_blocks_per_seq) and every page into [0, num_blocks): a bad table gives wrong numbers,
 * never an access outside the buffers.  Rows of o outside every sequence are not written.
 * No cache slot at or past Lk_b, no other layer, no page outside the tables, no 64-key tile without a visible
 * key and no table entry of a logical block that holds no such tile influences the result: they may hold
 * anything (NaN bit patterns too), as for mio_fa3_decode_paged.
 * causal: bottom-right aligned per sequence (query i sees key j iff j <= i + Lk_b - Lq_b).  Rows
 * with no visible key, and every row of a sequence with Lk_b == 0, get o = 0, lse = -inf.
 * lse (nullable): fp32 [H,total_q].  block_size must be a multiple of 64 (a 64-key tile never
 * spans two pages); num_blocks * num_layers * block_size < 2^32.  H % Hkv == 0; D in [8,128],
 * D % 8 == 0; plain K, softmax_scale applied in fp32.  No host sync; graph-capturable.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  const void* q;
  const void* k_cache;
  const void* v_cache;
  void* o;
  float* lse;                  /* nullable, fp32 [H, total_q] */
  const int32_t* cu_seqlens_q; /* device, B+1 entries */
  const int32_t* seqused_k;    /* device, B entries: keys of each sequence in the cache */
  const int32_t* block_tables; /* device, [B, max_blocks_per_seq] */
  int64_t q_stride[2];         /* token, head */
  int64_t o_stride[2];
  int32_t B, total_q, max_seqlen_q, max_seqlen_k, H, Hkv, D;
  int32_t num_blocks, num_layers, layer_idx, block_size, max_blocks_per_seq;
  int32_t dtype;       /* mio_dtype_t */
  int32_t causal;      /* 0/1 */
  float softmax_scale; /* > 0 */
} mio_fa3_paged_params_t;

int mio_fa3_fwd_paged(const mio_fa3_paged_params_t* p, void* stream);
/* Which kernel mio_fa3_fwd_paged launches (nothing is launched or dereferenced; no device needed).  Returns a
 * mio_fa3_paged_route_t, or < 0 (mio_last_error()) where mio_fa3_fwd_paged would refuse the arguments. */
typedef enum {
  MIO_FA3_PAGED_ROUTE_INVALID = -1,
  MIO_FA3_PAGED_ROUTE_EMPTY = 0, /* B == 0 or total_q == 0: nothing to launch */
  MIO_FA3_PAGED_ROUTE_FWD5 = 1,  /* fa3_fwd5_paged_kernel (padded head dim 64) */
  MIO_FA3_PAGED_ROUTE_FWD3 = 2   /* fa3_fwd3_paged_kernel (padded head dim 96 / 128) */
} mio_fa3_paged_route_t;
int32_t mio_fa3_paged_route(const mio_fa3_paged_params_t* p);

/* Merge two normalised partial attention states over disjoint key sets (ring / split-KV):
 * o = w_a*o_a + w_b*o_b, lse = logaddexp(lse_a, lse_b), w_x = exp(lse_x - lse).
 * Restates the (alpha, beta) update of kernels/triton/attention_kernels.py:1573-1585.
 * o_* fp32 [rows, D] contiguous with rows = B*Sq*H laid out [B,Sq,H]; lse_* fp32 [B,H,Sq].
 * Result in (o_a, lse_a); if o_out != NULL the merged output is also written there in `dtype`.
 * Memory the launch does not own may hold anything, NaN bit patterns included, and does not influence the result: the
 * bytes around the five operands are neither read into it nor written; o_b and lse_b are not written. */
int mio_attn_merge(float* o_a, float* lse_a, const float* o_b, const float* lse_b, void* o_out,
                   int32_t B, int32_t Sq, int32_t H, int32_t D, int32_t dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * y[M,N] = epilogue( x[M,K] @ w[N,K]^T ), bf16/fp16 in, fp32 accumulate on MFMA.
 *   act != SWIGLU:  y = act(x w^T + bias) (+ residual)
 *   act == SWIGLU:  y = silu(x w_gate^T + bias_gate) * (x w^T + bias)
 * This is the GEMM under both FusedMLP stages and the q/k/v/o projections
 * (F.linear call sites: kernels/mlp/fused_mlp.py:159,176,225,236,265-266,274;
 *  kernels/attention/flash_attention.py:629-631,654-657).
 * ldx/ldw/ldy/ldr: row strides in elements (multiples of 8); K % 8 == 0; bias/residual nullable.
 * Memory the launch does not own may hold anything, NaN bit patterns included, and does not influence the result -- here
 *   and in every entry point below that ends in a GEMM (the *_bw forms, mio_gemm_ln_bw / mio_gemm_rms_bw, the three
 *   FusedMLP forwards, mio_gemm_skinny, mio_gemm_skinny_w8) and in the weight preparations.  A launch owns x[m, k], m < M,
 *   k < K; w[n, k] and w_gate[n, k], n < N, k < K (a prepared weight: the whole prepared buffer, whose padding the library
 *   wrote); bias[n], bias_gate[n], w_scale[n], w_scale_gate[n], n < N; residual[m, n], m < M, n < N; and of the statistics
 *   ln_stats[s][m], s < ln_slots, m < M.  Not owned: the columns K .. ld of x, w, w_gate (bytes K .. ldw of an fp8 weight),
 *   the columns N .. ld of the residual and of y, the elements in front of element 0 and at and past N of a bias or scale,
 *   the rows in front of row 0 and the rows >= M (x, residual, y) or >= N (weights) of a larger buffer, the rows
 *   M .. ceil(M/256)*256 of a blocked x or residual and of every statistics slot, the statistics slots >= ln_slots, and a
 *   workspace's contents before the launch.  The K tail, the rows a tile has past M or N and the idle stages of the
 *   persistent kernel are zero-filled, clamped to an owned row or discarded: none of them reaches a stored value.
 *   y is written at m < M, n < N only: the bytes between N and ldy, the rows around y and, of a blocked y
 *   (MIO_GEMM_Y_BLOCKED), the padding rows M .. ceil(M/256)*256 keep what they held.
 *   Inputs are never written.
 * ------------------------------------------------------------------------------------------ */
int mio_gemm_bias_act(const void* x, const void* w, const void* bias, const void* w_gate,
                      const void* bias_gate, const void* residual, void* y, int64_t M, int32_t N,
                      int32_t K, int64_t ldx, int64_t ldw, int64_t ldy, int64_t ldr, int32_t act,
                      int32_t dtype, void* stream);

/* FusedMLP forward: y = fc2(act(fc1(x))) (+ residual).
 * Replaces: triton_fused_mlp -> _fused_mlp_{gelu,relu,swiglu}_kernel launch
 *           (kernels/triton/mlp_kernels.py:648-756, launch :711) and FusedMLP._forward_triton's
 *           fused_mlp_forward call (kernels/mlp/fused_mlp.py:131-141).
 * x [M,d], w1/wg [I,d], w2 [d,I], biases nullable; workspace >= mio_fused_mlp_workspace_bytes()
 * holds the bf16/fp16 [M,I] activation (written once by stage 1's epilogue, read once by stage 2; rows rounded up
 * to whole 256-row blocks: at sizes where both GEMMs run the 256x256-tile kernels the library keeps it in a blocked
 * layout of contiguous 16 KiB K-tiles).  What the workspace holds before the launch does not matter (stage 2 reads only what
 * stage 1 wrote for rows < M), nothing outside its mio_fused_mlp_workspace_bytes() is touched, and what it holds afterwards is
 * unspecified.  x, the weights and the residual are contiguous rows here: the ownership rule of mio_gemm_bias_act holds for the
 * rows around them, for the elements around the biases and for y. */
size_t mio_fused_mlp_workspace_bytes(int64_t M, int32_t d, int32_t I, int32_t act);
int mio_fused_mlp_fwd(const void* x, const void* w1, const void* b1, const void* wg, const void* bg,
                      const void* w2, const void* b2, const void* residual, void* y, void* workspace,
                      int64_t M, int32_t d, int32_t I, int32_t act, int32_t dtype, void* stream);

/* Blocked weights: a one-time repack of an nn.Linear weight [N, K] (K % 32 == 0) so that every (256-row, 32-column)
 * K-tile the 256x256-tile GEMM kernels fetch is one contiguous 16 KiB block instead of 256 pieces of 64 B at a stride of
 * 2 K bytes:   wb[((n / 256) * (K / 32) + k / 32) * 256 + n % 256][k % 32],  rows padded with zeros to a multiple of 256
 * (mio_weight_blocked_bytes).  The reference has no counterpart (its weights stay nn.Linear tensors read by tl.load,
 * kernels/triton/mlp_kernels.py:91-126); the plain-weight entry points above remain the drop-in boundary.
 * *_ok() == 0: the shape does not take those kernels -- keep the plain weight and call the plain entry point
 * (the *_bw entry points return an error then).
 * The preparations (mio_weight_block, mio_weight_block_glu, mio_ln_fold_weight, mio_weight_quant_w8) read w[n, k], n < N,
 * k < K of their source and nothing else of it: the columns K .. ldw and the rows around it may hold anything.  The padding
 * rows of a blocked weight are written as zeros whatever lies behind row N - 1 of the source. */
size_t mio_weight_blocked_bytes(int32_t N, int32_t K);
int mio_weight_block(const void* w, int64_t ldw, void* wb, int32_t N, int32_t K, int32_t dtype, void* stream);
int32_t mio_gemm_blocked_weight_ok(int64_t M, int32_t N, int32_t K, int32_t act);
int mio_gemm_bias_act_bw(const void* x, const void* wb, const void* bias, const void* residual, void* y, int64_t M,
                         int32_t N, int32_t K, int64_t ldx, int64_t ldy, int64_t ldr, int32_t act, int32_t dtype,
                         int32_t x_blocked, void* stream);
/* The same (no residual) with output columns [cs_lo, cs_hi) multiplied by cs_val in fp32 after bias / activation and before
 * the rounding to 16 bits (cs_lo, cs_hi multiples of 128).  The fused q/k/v projection uses it to hand mio_fa3_fwd a K that
 * already carries softmax_scale * log2(e) with a single rounding (k_prescaled).  Only where mio_gemm_col_scale_ok() != 0
 * (the persistent 256x256-tile kernel takes the launch). */
int32_t mio_gemm_col_scale_ok(int64_t M, int32_t N, int32_t K, int32_t act);
int mio_gemm_bias_act_bw_cs(const void* x, const void* wb, const void* bias, void* y, int64_t M, int32_t N, int32_t K,
                            int64_t ldx, int64_t ldy, int32_t act, int32_t dtype, int32_t x_blocked, int32_t cs_lo,
                            int32_t cs_hi, float cs_val, void* stream);
int32_t mio_fused_mlp_blocked_weight_ok(int64_t M, int32_t d, int32_t I, int32_t act);
int mio_fused_mlp_fwd_bw(const void* x, const void* w1b, const void* b1, const void* w2b, const void* b2,
                         const void* residual, void* y, void* workspace, int64_t M, int32_t d, int32_t I, int32_t act,
                         int32_t dtype, int32_t x_blocked, void* stream);
/* SwiGLU on the 256x256-tile kernels (reference kernels/triton/mlp_kernels.py:417-641 _fused_mlp_swiglu_kernel;
 * kernels/mlp/fused_mlp.py:262-275): the gate and up weights [I, K] are repacked ONCE into one blocked weight whose 256-row
 * tiles interleave, per 64-row wave slice, 32 gate rows and the 32 up rows of the same output columns
 *   row (tn * 256 + wn * 64 + h * 32 + j)  <-  (h ? w_up : w_gate)[tn * 128 + wn * 32 + j],   rows padded with zeros,
 * so that silu(gate) * up is local to a lane of the accumulator and stage 1 writes act once.  Use where
 * mio_fused_mlp_blocked_weight_ok(M, d, I, MIO_ACT_SWIGLU) != 0; w2b is mio_weight_block(w2). */
size_t mio_weight_blocked_glu_bytes(int32_t I, int32_t K);
int mio_weight_block_glu(const void* w_gate, const void* w_up, int64_t ldw, void* wb, int32_t I, int32_t K, int32_t dtype,
                         void* stream);
int mio_fused_mlp_glu_fwd_bw(const void* x, const void* wgu_b, const void* b_up, const void* b_gate, const void* w2b,
                             const void* b2, const void* residual, void* y, void* workspace, int64_t M, int32_t d, int32_t I,
                             int32_t dtype, int32_t x_blocked, void* stream);
/* Which GEMM kernel a launch with these arguments takes (host-only: no pointer is dereferenced).  The same rule the launch
 * switches on (csrc/gemm_route.h), for every entry point that ends in a GEMM (mio_gemm_bias_act, *_bw, *_bw_cs, mio_gemm_ln_bw
 * and both stages of the FusedMLP forwards).  ld*: row strides in elements (a blocked operand: its row length, K or N);
 * has_residual: a residual is added; w_layout: 0 row-major, 1 blocked (mio_weight_block), 2 gate / up interleaved
 * (mio_weight_block_glu); fold_in / stats_out: the LayerNorm consumer / producer forms of mio_gemm_ln_bw.  The column scale
 * is an argument of the persistent kernel, not a route.  Returns a mio_gemm_route_t, or < 0 (mio_last_error()) for
 * arguments no entry point takes (sizes, strides, an activation or weight layout the form does not have). */
typedef enum {
  MIO_GEMM_ROUTE_EMPTY = 0,         /* M == 0: nothing is launched                                                 */
  MIO_GEMM_ROUTE_T128 = 1,          /* gemm_bias_act_kernel, 128x128 tiles (fewer than 256 tiles of 256x256)       */
  MIO_GEMM_ROUTE_T256 = 2,          /* gemm_bias_act_kernel, 256x256 tiles (K % 32 != 0, K < 128 or a long stride)  */
  MIO_GEMM_ROUTE_P8W = 3,           /* gemm8w_kernel, persistent, no residual (column scale here)                  */
  MIO_GEMM_ROUTE_P8W_RES = 4,       /* gemm8w_kernel with the residual epilogue                                   */
  MIO_GEMM_ROUTE_P8W_FOLD = 5,      /* gemm8w_kernel, LayerNorm consumer (fold_in)                                */
  MIO_GEMM_ROUTE_P8W_STATS = 6,     /* gemm8w_kernel, residual epilogue + row statistics (stats_out)              */
  MIO_GEMM_ROUTE_GLU_T128X64 = 7,   /* gemm_bias_act_kernel SwiGLU, 128x64 tiles                                  */
  MIO_GEMM_ROUTE_GLU_T256X128 = 8,  /* gemm_bias_act_kernel SwiGLU, 256x128 tiles (>= 256 of them)                */
  MIO_GEMM_ROUTE_P8W_GLU = 9,       /* gemm8w_kernel SwiGLU on the interleaved blocked weight                     */
  MIO_GEMM_ROUTE_P8W_GLU_FOLD = 10  /* the same, LayerNorm consumer                                               */
} mio_gemm_route_t;
int32_t mio_gemm_route(int64_t M, int32_t N, int32_t K, int64_t ldx, int64_t ldw, int64_t ldy, int64_t ldr, int32_t act,
                       int32_t has_residual, int32_t w_layout, int32_t fold_in, int32_t stats_out);

/* The decode-step GEMM: mio_gemm_bias_act's contraction and epilogue for 1 <= M <= 64 rows (M = the batch of a decode step), on
 * a kernel that streams the row-major [N, K] weight from HBM once, straight into registers (csrc/gemm_skinny.hip).  The
 * reference has no such kernel: its decode step runs the projections and the MLP through F.linear
 * (kernels/attention/flash_attention.py:629-631,654-657; kernels/mlp/fused_mlp.py:159,176).
 *   arguments as mio_gemm_bias_act (ld*: multiples of 8 elements, K % 8 == 0, pointers 16-byte aligned, bias / residual
 *   nullable, w_gate iff act == SWIGLU), but any N >= 1, and a workspace.
 * K is cut into mio_gemm_skinny_splits() slices of whole 32-k steps (mio_gemm_skinny_slice: the k range of one) so that the
 * launch fills the chip; with more than one slice the kernel writes fp32 partials [splits][M][N] (SwiGLU: twice, up then gate)
 * into `workspace` (>= mio_gemm_skinny_workspace_bytes(), 0 with one slice) and a second small kernel sums them in slice order,
 * applies bias / activation / residual and rounds once.  No workgroup waits for another: the result is bit-reproducible, and
 * the launch neither allocates nor synchronises (graph-capturable).  The ownership rule of mio_gemm_bias_act holds here and
 * in mio_gemm_skinny_w8 (the rows M .. 63 behind x that pad the last row fragment, the columns K .. ld, the elements around
 * bias and scales are not owned); what the workspace holds before the launch does not matter and nothing outside its
 * mio_gemm_skinny_workspace_bytes() is touched.
 * mio_gemm_skinny runs every legal shape; M == 0 returns 0 and launches nothing.  mio_gemm_skinny_ok only advises the module
 * layer: 1 where the shape is legal AND measured at most 0.9 x the time of mio_gemm_bias_act's route (profiles/skinny_gemm.md).
 * mio_gemm_skinny_splits / _slice return < 0 (mio_last_error()) on a shape the launch refuses.
 * Inside a slice a workgroup runs a double-buffered loop over chunks of mio_gemm_skinny_chunk_k(act) k (256, SwiGLU 128; < 0 on
 * an unknown activation): ceil(slice length / chunk) chunks, which is what the tests ask to know which parts of that loop a
 * shape reaches. */
size_t mio_gemm_skinny_workspace_bytes(int64_t M, int32_t N, int32_t K, int32_t act);
int mio_gemm_skinny_splits(int64_t M, int32_t N, int32_t K, int32_t act);
int mio_gemm_skinny_slice(int64_t M, int32_t N, int32_t K, int32_t act, int32_t slice, int32_t* k_begin, int32_t* k_end);
int mio_gemm_skinny_chunk_k(int32_t act);
int mio_gemm_skinny_ok(int64_t M, int32_t N, int32_t K, int32_t act);
int mio_gemm_skinny(const void* x, const void* w, const void* bias, const void* w_gate, const void* bias_gate,
                    const void* residual, void* y, void* workspace, int64_t M, int32_t N, int32_t K, int64_t ldx,
                    int64_t ldw, int64_t ldy, int64_t ldr, int32_t act, int32_t dtype, void* stream);

/* The decode-step GEMM on weight-only FP8: mio_gemm_skinny with the weight stored as OCP e4m3fn bytes (torch.float8_e4m3fn,
 * row-major [N, K], ldw in bytes) and one fp32 scale per output column (csrc/gemm_skinny_w8.hip):
 *   y = act(w_scale[n] * (x w8^T) + bias[n]) (+ residual)
 *   SwiGLU: silu(w_scale_gate[n] * (x w8_gate^T) + bias_gate[n]) * (w_scale[n] * (x w8^T) + bias[n])
 * It replaces the same F.linear sites of the reference as mio_gemm_skinny (kernels/attention/flash_attention.py:629-631,654-657;
 * kernels/mlp/fused_mlp.py:159,176).  The reference has no quantised weights: this storage form, the kernel and the quantiser
 * below have no counterpart there.  FP8 is how the weights are stored, not a compute precision: the bytes are widened exactly
 * in registers and multiplied on the 16-bit MFMA, x / bias / residual / y stay bf16 or fp16 (dtype), and the result is the
 * 16-bit kernel's on the dequantised weight plus one fp32 fma per output.
 *   1 <= M <= 64, any N >= 1, K % 16 == 0, ldw % 16 == 0 (bytes) and >= K, ldx / ldy / ldr multiples of 8 elements, every
 *   pointer 16-byte aligned; bias / residual nullable; w8_gate and w_scale_gate together iff act == SWIGLU; scales any finite
 *   fp32 (a zero scale gives act(bias)).  M == 0 or N == 0 returns 0 and launches nothing; K == 0 is an empty sum.
 * K is cut into mio_gemm_skinny_w8_splits() slices of whole 64-k steps (mio_gemm_skinny_w8_slice), partials and workspace as
 * mio_gemm_skinny (mio_gemm_skinny_w8_workspace_bytes); bit-reproducible, graph-capturable.  Inside a slice a workgroup walks
 * chunks of mio_gemm_skinny_w8_chunk_k(act) k with a ring of mio_gemm_skinny_w8_depth(act) register sets, depth - 1 chunks of
 * weight loads in flight: both are tuning values the tests ask for (< 0 on an unknown activation).
 * mio_gemm_skinny_w8_ok only advises the module layer: 1 where the shape is legal AND the kernel measured at most 0.9 x the
 * time of the faster of mio_gemm_skinny and mio_gemm_bias_act on the 16-bit weight (profiles/skinny_gemm_w8.md).
 * mio_weight_quant_w8 is the one-time preparation, per row n of a 16-bit weight w [N, K] (ldw in elements, K % 16 == 0):
 *   a = max |w[n, :]| in fp32 (NaN elements ignored), scale[n] = a / 448 (1.0 where a == 0),
 *   w8[n, k] = e4m3(clamp(float(w[n, k]) * (1.0f / scale[n]), -448, 448)), round to nearest even; a NaN element -> sign | 0x7f
 * (the formula and NaN rule of mio_reshape_and_cache_kv8).  ldw8 in bytes, a multiple of 16. */
int mio_weight_quant_w8(const void* w, int64_t ldw, void* w8, int64_t ldw8, float* scale, int32_t N, int32_t K, int32_t dtype,
                        void* stream);
size_t mio_gemm_skinny_w8_workspace_bytes(int64_t M, int32_t N, int32_t K, int32_t act);
int mio_gemm_skinny_w8_splits(int64_t M, int32_t N, int32_t K, int32_t act);
int mio_gemm_skinny_w8_slice(int64_t M, int32_t N, int32_t K, int32_t act, int32_t slice, int32_t* k_begin, int32_t* k_end);
int mio_gemm_skinny_w8_chunk_k(int32_t act);
int mio_gemm_skinny_w8_depth(int32_t act);
int mio_gemm_skinny_w8_ok(int64_t M, int32_t N, int32_t K, int32_t act);
int mio_gemm_skinny_w8(const void* x, const void* w8, const float* w_scale, const void* bias, const void* w8_gate,
                       const float* w_scale_gate, const void* bias_gate, const void* residual, void* y, void* workspace,
                       int64_t M, int32_t N, int32_t K, int64_t ldx, int64_t ldw, int64_t ldy, int64_t ldr, int32_t act,
                       int32_t dtype, void* stream);
/* x_blocked != 0: the activation operand x is in the same blocked layout (m in the place of n; ceil(M/256)*256 x K
 * elements, ldx ignored) -- what mio_layernorm_fwd_bx writes, so that LayerNorm -> GEMM hands over contiguous K-tiles. */
int mio_layernorm_fwd_bx(const void* x, const void* residual, const void* weight, const void* bias, void* yb,
                         void* sum_out, int64_t rows, int32_t cols, float eps, float alpha, int32_t dtype, void* stream);

/* LayerNorm folded into the GEMMs on either side of it.  Replaces the reference's LayerNorm -> QKV prologue
 * fusion (kernels/triton/fused_layernorm_qkv.py:37-420, triton_fused_layernorm_qkv) and its residual + LayerNorm pass
 * (kernels/triton/layernorm_kernels.py:35-188) between two GEMMs of a transformer block:
 *   producer = the GEMM that writes the residual stream (out-proj / fc2 with the residual epilogue): stats_out != NULL makes it
 *     also write, per output row and 256-column tile, (sum, sum of squares) of the ROUNDED row: [N / 256][ceil(M/256)*256][2]
 *     fp32 (mio_ln_stats_bytes(M, N)); deterministic (fixed summation order, no atomics).  The kernel stores all 256 rows of
 *     a row tile: the rows M .. ceil(M/256)*256 of every slot ARE written, with the statistics of rows it recomputes from
 *     clamped (owned) rows of x and the residual -- values without meaning that depend on nothing the launch does not own;
 *   consumer = the projection behind the LayerNorm: ln_stats (a producer's stats_out of width K) != NULL: x is the raw stream,
 *     wb = mio_weight_block of the gamma-scaled, row-centred weight and bias the beta-folded bias (both from mio_ln_fold_weight:
 *     (x - mean 1) . w = x . (w - mean(w) 1), so centring the weight rows makes the plain product the centred one); the
 *     read-out computes rstd * acc + bias, then act / column scale.  Rounding: mio_ln_fold_weight chooses the rounding direction
 *     of a few elements per row so that the 16-bit row sums to zero within an ulp or two (plain rounding would leave ~sqrt(K/12)
 *     ulp, and the product would carry mean(x) times that); measured error equals the LayerNorm kernel + GEMM's (2.3e-3 bf16)
 *     for streams whose row mean is up to 4x their deviation.  The consumer owns ln_stats[s][m][0..1] for s < ln_slots and
 *     m < M (mio_gemm_rms_bw: only [1], the sum of squares): the rows M .. ceil(M/256)*256 of a slot (a producer's leftovers, or
 *     nothing at all) and the slots >= ln_slots of a larger buffer may hold anything, NaN bit patterns and values that survive
 *     the variance's fmaxf(., 0) included.
 * flags: the operands in the blocked activation layout ((256-row, 32-column) blocks of 16 KiB, rows padded to 256; ld* ignored
 * for a blocked operand): x (as mio_gemm_bias_act_bw's x_blocked), y (what the next GEMM takes as blocked x), residual.
 * Shapes: mio_gemm_ln_ok(M, N, K, act, fold_in, stats_out) != 0 (blocked-weight shapes; fold_in: K % 256 == 0, K <= 8192 (the
 * rows mio_ln_fold_weight prepares), act none / gelu_tanh / swiglu; stats_out: N % 256 == 0, act none).  Without ln_stats and stats_out it is
 * mio_gemm_bias_act_bw (+ column scale) with blocked y / residual.  act == MIO_ACT_SWIGLU: wb is mio_weight_block_glu of the two
 * folded weights (gate, up), bias the up bias, bias_gate the gate bias, N the number of OUTPUT columns (I). */
#define MIO_GEMM_X_BLOCKED 1
#define MIO_GEMM_Y_BLOCKED 2
#define MIO_GEMM_RES_BLOCKED 4
size_t mio_ln_stats_bytes(int64_t M, int32_t width);
int32_t mio_gemm_ln_ok(int64_t M, int32_t N, int32_t K, int32_t act, int32_t fold_in, int32_t stats_out);
/* w [N, K] (row stride ldw), gamma / beta [K] (beta nullable), bias [N] (nullable), all in dtype; w_scaled [N, K] contiguous
 * = w * gamma - mean_k(w * gamma) (rounded once), bias_out [N] = bias + w beta.  One-time weight preparation. */
int mio_ln_fold_weight(const void* w, int64_t ldw, const void* gamma, const void* beta, const void* bias, void* w_scaled,
                       void* bias_out, int32_t N, int32_t K, int32_t dtype, void* stream);
int mio_gemm_ln_bw(const void* x, const void* wb, const void* bias, const void* bias_gate, const void* residual, void* y, int64_t M, int32_t N, int32_t K,
                   int64_t ldx, int64_t ldy, int64_t ldr, int32_t act, int32_t dtype, int32_t flags, const float* ln_stats,
                   int32_t ln_slots, float ln_eps, float* stats_out, int32_t cs_lo, int32_t cs_hi, float cs_val, void* stream);
/* ln_slots: statistic slots in ln_stats (0: K / 256, what a producer of width K writes); at most 8.  A wider stream (K > 2048)
 * goes through mio_ln_stats_reduce first: stats_out[s'] = sum of slots_in / slots_out consecutive slots, same row padding:
 * the padding rows M .. ceil(M/256)*256 of stats_out are written with the sums of the input's padding rows, whatever those
 * hold (unspecified values, which the consumer does not own either); the rows < M depend on the rows < M of the slots_in
 * slots only. */
int mio_ln_stats_reduce(const float* stats_in, int32_t slots_in, float* stats_out, int32_t slots_out, int64_t M, void* stream);
/* The consumer form behind an RMSNorm(gamma): mio_gemm_ln_bw's arguments, kernels, routes (mio_gemm_route, mio_gemm_ln_ok answer
 * for both norms) and checks, with rstd = rsqrt(sum of squares / K + ln_eps): the statistics' sum entries are not used.  wb =
 * mio_weight_block (swiglu: mio_weight_block_glu) of the 16-bit rounding of w * gamma (no centring, nothing folded into the bias;
 * bias nullable).  ln_stats is required; residual and stats_out must be NULL (refused: the consumer form only). */
int mio_gemm_rms_bw(const void* x, const void* wb, const void* bias, const void* bias_gate, const void* residual, void* y, int64_t M, int32_t N, int32_t K,
                    int64_t ldx, int64_t ldy, int64_t ldr, int32_t act, int32_t dtype, int32_t flags, const float* ln_stats,
                    int32_t ln_slots, float ln_eps, float* stats_out, int32_t cs_lo, int32_t cs_hi, float cs_val, void* stream);

/* LayerNorm / residual+LayerNorm rows (the step either side of attention):
 * sum = x + alpha*residual (if residual), y = (sum-mean)/sqrt(var+eps)*weight + bias.
 * Replaces triton_layernorm -> _layernorm_fwd_kernel / _layernorm_residual_fwd_kernel
 * (kernels/triton/layernorm_kernels.py:191-276; kernels :35-188).  sum_out nullable.
 * x, residual, y and sum_out are `rows` contiguous rows of `cols` elements (there is no row stride).  Memory the launch does
 * not own may hold anything, NaN bit patterns included, and does not influence the result -- in mio_layernorm_fwd,
 * mio_layernorm_fwd_bx and mio_rmsnorm_fwd: the rows around x and the residual and the elements around weight and bias are
 * not read into it, the bytes around y and sum_out and the padding rows past `rows` of a blocked y are not written, inputs
 * are not written. */
int mio_layernorm_fwd(const void* x, const void* residual, const void* weight, const void* bias,
                      void* y, void* sum_out, int64_t rows, int32_t cols, float eps, float alpha,
                      int32_t dtype, void* stream);
/* RMSNorm / residual+RMSNorm rows (LLaMA-class decoders): s = x, or x + alpha*residual (with sum_out: rounded to dtype, stored
 * there, and the rounded value is what is normalised, as in mio_layernorm_fwd); y = s * rsqrt(mean(s^2) + eps) * weight.  No
 * bias.  cols % 8 == 0, cols <= 8192 (LayerNorm: 4096); y_blocked != 0: y in the blocked activation layout as
 * mio_layernorm_fwd_bx writes it (cols % 32 == 0).  residual, sum_out nullable; every given pointer 16-byte aligned.
 * rows == 0: returns 0 without a launch. */
int mio_rmsnorm_fwd(const void* x, const void* residual, const void* weight, void* y, void* sum_out, int64_t rows,
                    int32_t cols, float eps, float alpha, int32_t dtype, int32_t y_blocked, void* stream);

/* ------------------------------------------------------------------------------------------
 * Sliding-window attention forward (flash-attn's window_size = (left, right)): the params of
 * mio_fa3_fwd / mio_fa3_fwd_varlen / mio_fa3_fwd_paged unchanged, plus the window.  Each value is -1
 * (unbounded) or >= 0; query row i sees key j iff j >= i + off - window_left (left >= 0) and
 * j <= i + off + window_right (right >= 0) and the causal / length rules allow it, with
 * off = q_offset - k_offset (dense) or Lk_b - Lq_b (varlen, paged: bottom-right per sequence).
 * causal means window_right = 0 (-1 or 0 accepted).  Rows with no visible key get o = 0, lse = -inf.
 * (-1, -1) is the existing entry point exactly (same route, same output).  Any other window runs the
 * windowed fwd5 (head dim <= 64) / fwd3 kernels, which walk only the KV tiles inside each query
 * block's window; the routes report MIO_FA3_ROUTE_FWD5 / FWD3 / EMPTY for them (a dense launch with
 * Sk = 0 has no key to window and takes the unwindowed route).  Refused under a window: a window
 * value below -1, causal with window_right > 0, and for the dense form a mask, the ring carry
 * (o_acc / carry_in), k_prescaled, o_blocked, K / V spans of 4 GiB or more; lengths and offsets of
 * 2^28 or more.
 * ------------------------------------------------------------------------------------------ */
int mio_fa3_fwd_window(const mio_fa3_fwd_params_t* p, int32_t window_left, int32_t window_right, void* stream);
int32_t mio_fa3_route_window(const mio_fa3_fwd_params_t* p, int32_t window_left, int32_t window_right);
int mio_fa3_fwd_varlen_window(const mio_fa3_varlen_params_t* p, int32_t window_left, int32_t window_right,
                              void* stream);
int32_t mio_fa3_varlen_route_window(const mio_fa3_varlen_params_t* p, int32_t window_left, int32_t window_right);
int mio_fa3_fwd_paged_window(const mio_fa3_paged_params_t* p, int32_t window_left, int32_t window_right,
                             void* stream);
int32_t mio_fa3_paged_route_window(const mio_fa3_paged_params_t* p, int32_t window_left, int32_t window_right);

/* ------------------------------------------------------------------------------------------
 * Paged-KV decode attention.  Replaces triton_paged_attention_forward ->
 * _paged_attention_fwd_kernel (kernels/triton/attention_kernels.py:1206-1311; kernel :628-808).
 * q/o [B,H,q_len,D] (strides b,h,s; d contiguous); caches [num_blocks, L, block_size, Hkv, D]
 * contiguous; block_tables [B,max_blocks] int32; context_lengths [B] int32.  No causal mask
 * (the reference's is commented out, :774-776).  workspace: mio_fa3_decode_workspace_bytes().
 * Keys at positions >= max_blocks * block_size (a context longer than its block-table row) are
 * ignored.  No cache slot at or past context_lengths[b], and no table entry past the last needed
 * block, influences the result: such slots and entries may hold anything (NaN bit patterns too).
 * What a launch may read and write (tests/_hostile_decode.py holds every route to it, bit for bit,
 * under NaN and under huge finite values in everything else): of q the D elements of each
 * (b, h, qi) row; context_lengths[0..B); of the caches the slots of layer_idx at the positions
 * max(0, ctx_b - q_len - window_left) <= j < min(ctx_b, max_blocks * block_size) (from 0 without a
 * window) and the table entries of the blocks that hold one; with an fp8 cache the two scales of
 * layer_idx.  Keys in front of that range, the pages that hold only such keys and their table
 * entries may hold anything (a table entry must still name a block inside the cache), as may
 * the other layers, sequences and kv heads' data as far as one row of o is concerned.  What the
 * workspace holds before a launch does not matter, and nothing outside its
 * mio_fa3_decode_workspace_bytes() is written.  Of o the D elements of each (b, h, qi) row are
 * written; the bytes of q / o between D and the row stride are neither read nor written.
 * ------------------------------------------------------------------------------------------ */
size_t mio_fa3_decode_workspace_bytes(int32_t B, int32_t H, int32_t q_len, int32_t D, int32_t max_ctx);
int mio_fa3_decode_paged(const void* q, void* o, const void* k_cache, const void* v_cache,
                         const int32_t* block_tables, const int32_t* context_lengths,
                         const int64_t q_stride[3], const int64_t o_stride[3], int32_t B, int32_t H,
                         int32_t Hkv, int32_t q_len, int32_t D, int32_t num_layers, int32_t layer_idx,
                         int32_t block_size, int32_t max_blocks_per_seq, int32_t max_ctx, float scale,
                         int32_t dtype, void* workspace, void* stream);

/* Sliding-window decode (flash-attn's window_size = (left, right), decode form).  The arguments of
 * mio_fa3_decode_paged plus the window: row qi of q_len sees the cached keys j < ctx_b with
 * j >= ctx_b - q_len + qi - window_left; rows with no visible key get o = 0.  window_left is -1
 * (unbounded) or >= 0; window_right must be -1 (decode has no upper bound).  (-1, -1) is
 * mio_fa3_decode_paged exactly.  The splits cover [max(0, ctx_b - q_len - window_left), ctx_b) and
 * their count is sized from min(max_ctx, window_left + q_len), so mio_fa3_decode_workspace_bytes
 * for max_ctx covers every windowed launch as well.  Refused: a window value below -1, and
 * window_right != -1. */
int mio_fa3_decode_paged_window(const void* q, void* o, const void* k_cache, const void* v_cache,
                                const int32_t* block_tables, const int32_t* context_lengths,
                                const int64_t q_stride[3], const int64_t o_stride[3], int32_t B, int32_t H,
                                int32_t Hkv, int32_t q_len, int32_t D, int32_t num_layers, int32_t layer_idx,
                                int32_t block_size, int32_t max_blocks_per_seq, int32_t max_ctx, float scale,
                                int32_t window_left, int32_t window_right, int32_t dtype, void* workspace,
                                void* stream);

/* Which decode kernel a mio_fa3_decode_paged_window launch with these arguments takes (host-only: no
 * pointer is dereferenced, no stream is touched; the same argument checks).  Returns a
 * mio_decode_route_t, or <0 with mio_last_error() set when the launch would be refused.  The kernel
 * heuristics see the window span min(max_ctx, window_left + q_len) as the context length. */
typedef enum {
  MIO_DEC_ROUTE_HEAD = 0, /* decode_paged_kernel: one workgroup per (query row, split)              */
  MIO_DEC_ROUTE_ROWS = 1, /* decode_rows_kernel: whole token rows, one workgroup per (sequence, split) */
  MIO_DEC_ROUTE_GQA = 2   /* decode_gqa_kernel: matrix-core, one workgroup per (sequence, kv head, split) */
} mio_decode_route_t;
int mio_fa3_decode_window_route(const void* q, void* o, const void* k_cache, const void* v_cache,
                                const int32_t* block_tables, const int32_t* context_lengths,
                                const int64_t q_stride[3], const int64_t o_stride[3], int32_t B, int32_t H,
                                int32_t Hkv, int32_t q_len, int32_t D, int32_t num_layers, int32_t layer_idx,
                                int32_t block_size, int32_t max_blocks_per_seq, int32_t max_ctx, float scale,
                                int32_t window_left, int32_t window_right, int32_t dtype, void* workspace,
                                void* stream);

/* Scatter the current token's K/V into the paged cache at position context_len-1.
 * Replaces triton_reshape_and_cache -> _reshape_and_cache_kernel
 * (kernels/triton/attention_kernels.py:1314-1407; kernel :811-905).  key/value [B,1,Hkv,D]. */
int mio_reshape_and_cache(const void* key, const void* value, void* k_cache, void* v_cache,
                          const int32_t* block_tables, const int32_t* context_lengths,
                          const int64_t k_stride[2], const int64_t v_stride[2], /* b, h */
                          int32_t B, int32_t Hkv, int32_t D, int32_t num_layers, int32_t layer_idx,
                          int32_t block_size, int32_t max_blocks_per_seq, int32_t dtype, void* stream);

/* Scatter many new tokens per sequence into the paged cache (prompt chunks, multi-token appends).
 * key/value [total_new,Hkv,D] packed, given by (token, head) strides (d stride 1); sequence b's
 * tokens are rows cu_seqlens_new[b] .. cu_seqlens_new[b+1]-1 (clamped into [0,total_new)), and
 * context_lengths[b] is its length AFTER the append: token i of n_b goes to position
 * context_lengths[b] - n_b + i.  Both are int32 DEVICE arrays [B+1] / [B], never read on the host.
 * Positions that are negative or past the block-table row, and table entries outside
 * [0,num_blocks), are skipped.  Caches as in mio_fa3_decode_paged.  Byte-exact 16-byte copies;
 * no host sync; graph-capturable. */
int mio_reshape_and_cache_varlen(const void* key, const void* value, void* k_cache, void* v_cache,
                                 const int32_t* block_tables, const int32_t* cu_seqlens_new,
                                 const int32_t* context_lengths, const int64_t k_stride[2],
                                 const int64_t v_stride[2], /* token, head */
                                 int32_t B, int32_t total_new, int32_t Hkv, int32_t D, int32_t num_blocks,
                                 int32_t num_layers, int32_t layer_idx, int32_t block_size,
                                 int32_t max_blocks_per_seq, int32_t dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * FP8 paged KV cache (OCP e4m3fn, torch.float8_e4m3fn).  The caches are the layout above at one byte
 * per element; key/value, q and o stay bf16 / fp16 (dtype).  A cached byte x8 stands for
 * x8 * scale: k_scale / v_scale are DEVICE pointers to the fp32 scale of layer_idx's K and V, read
 * by the kernels (no host sync, graph-capturable; a scale may change between replays).  Both are
 * required (null is refused) and 4-byte aligned.  head_dim must be a multiple of 16.
 * Writes quantise: q = e4m3(clamp(float(x) * (1.0f / scale), -448, 448)), round to nearest even,
 * NaN stays NaN; otherwise as mio_reshape_and_cache / mio_reshape_and_cache_varlen (same skipping
 * rules, positions skipped leave the cache bytes untouched).
 * Decode is mio_fa3_decode_paged_window over K = x8 * k_scale, V = x8 * v_scale: window_left -1
 * (unbounded) or >= 0, the same routes (head / rows / gqa), the same workspace
 * (mio_fa3_decode_workspace_bytes); mio_fa3_decode_kv8_route is its host-only route query.
 * Paged prefill (chunked prefill, shared prefixes, multi-token verify) is mio_fa3_fwd_paged_kv8:
 * mio_fa3_fwd_paged_window over K = x8 * k_scale, V = x8 * v_scale (window (-1, -1) = none), the
 * same kernels (fwd5 at padded head dim 64, fwd3 at 96 / 128) widening the bytes exactly to 16 bits
 * in LDS; p->dtype is that of q / o, p->k_cache / p->v_cache address bytes.  Refused besides what
 * mio_fa3_fwd_paged(_window) refuses: null or misaligned scales, head_dim % 16 != 0.
 * mio_fa3_paged_kv8_route is its host-only route query (a mio_fa3_paged_route_t).
 * ------------------------------------------------------------------------------------------ */
int mio_reshape_and_cache_kv8(const void* key, const void* value, void* k_cache, void* v_cache,
                              const float* k_scale, const float* v_scale, const int32_t* block_tables,
                              const int32_t* context_lengths, const int64_t k_stride[2],
                              const int64_t v_stride[2], int32_t B, int32_t Hkv, int32_t D, int32_t num_layers,
                              int32_t layer_idx, int32_t block_size, int32_t max_blocks_per_seq, int32_t dtype,
                              void* stream);
int mio_reshape_and_cache_varlen_kv8(const void* key, const void* value, void* k_cache, void* v_cache,
                                     const float* k_scale, const float* v_scale, const int32_t* block_tables,
                                     const int32_t* cu_seqlens_new, const int32_t* context_lengths,
                                     const int64_t k_stride[2], const int64_t v_stride[2], int32_t B,
                                     int32_t total_new, int32_t Hkv, int32_t D, int32_t num_blocks,
                                     int32_t num_layers, int32_t layer_idx, int32_t block_size,
                                     int32_t max_blocks_per_seq, int32_t dtype, void* stream);
int mio_fa3_decode_paged_kv8(const void* q, void* o, const void* k_cache, const void* v_cache,
                             const float* k_scale, const float* v_scale, const int32_t* block_tables,
                             const int32_t* context_lengths, const int64_t q_stride[3], const int64_t o_stride[3],
                             int32_t B, int32_t H, int32_t Hkv, int32_t q_len, int32_t D, int32_t num_layers,
                             int32_t layer_idx, int32_t block_size, int32_t max_blocks_per_seq, int32_t max_ctx,
                             float scale, int32_t window_left, int32_t dtype, void* workspace, void* stream);
/* a mio_decode_route_t, or <0 with mio_last_error() set where mio_fa3_decode_paged_kv8 would refuse */
int mio_fa3_decode_kv8_route(const void* q, void* o, const void* k_cache, const void* v_cache,
                             const float* k_scale, const float* v_scale, const int32_t* block_tables,
                             const int32_t* context_lengths, const int64_t q_stride[3], const int64_t o_stride[3],
                             int32_t B, int32_t H, int32_t Hkv, int32_t q_len, int32_t D, int32_t num_layers,
                             int32_t layer_idx, int32_t block_size, int32_t max_blocks_per_seq, int32_t max_ctx,
                             float scale, int32_t window_left, int32_t dtype, void* workspace, void* stream);
int mio_fa3_fwd_paged_kv8(const mio_fa3_paged_params_t* p, const float* k_scale, const float* v_scale,
                          int32_t window_left, int32_t window_right, void* stream);
int32_t mio_fa3_paged_kv8_route(const mio_fa3_paged_params_t* p, const float* k_scale, const float* v_scale,
                                int32_t window_left, int32_t window_right);

/* ------------------------------------------------------------------------------------------
 * Rotary position embedding (csrc/rope.hip).  The first rot_dim elements of every head are rotated
 * by the angles of the token's position: y1 = x1 c - x2 s, y2 = x2 c + x1 s, evaluated in fp32 and
 * rounded once to the stored format.  c / s are read from the caller's tables cos / sin, fp32
 * DEVICE arrays [max_position, rot_dim / 2] contiguous and 16-byte aligned, never computed by the
 * kernels (a scaled, YaRN or Llama-3 frequency schedule is the caller's table).  interleaved 0 is
 * the neox pairing (element i with i + rot_dim / 2), 1 the GPT-J one (element 2i with 2i + 1).
 * rot_dim is a multiple of 16 in [16, D]; D a multiple of 8 (16 for an fp8 cache) and <= 128; for
 * an fp8 cache with the neox pairing rot_dim is a multiple of 32.  Elements [rot_dim, D) pass
 * through unchanged.
 *
 * mio_rope_and_cache_varlen: mio_reshape_and_cache_varlen (same packed-token form, same positions,
 * same skipping rules, V and K's elements past rot_dim written exactly as it writes them) with K
 * rotated on the way into the cache and the token's H query heads rotated into q_out.  q / q_out
 * [total_new, H, D] by (token, head) strides each (d stride 1); q_out may be q.  The rotation's
 * position is the token's cache position context_lengths[b] - n_b + i, or positions[t] where
 * positions (int32 DEVICE [total_new], may be null) is given; the cache row does not depend on it.
 * A token outside every sequence's clamped range, or whose rotation position is outside
 * [0, max_position), writes nothing to the caches and its q_out row is zeros.  A token whose cache
 * row is skipped (position before the sequence, past the table row, block id outside
 * [0, num_blocks)) but whose rotation position is valid still gets its q_out row.
 * context_lengths is the caller's and is only read: a sequence whose length goes on growing past
 * max_position, or past its block-table row, keeps the cache bytes it had.  A decode launch over
 * such a sequence counts the unwritten positions below the table row's end as keys and reads what
 * their slots hold (they must hold finite values for a finite result), ignores the positions past
 * it, and a zero q_out row weighs every key it sees alike (tests/_step_check.py).
 * mio_rope_and_cache_varlen_kv8: the same into an fp8 (e4m3fn) cache with the layer's scales as in
 * mio_reshape_and_cache_varlen_kv8: K is e4m3(clamp(rot(k) * (1.0f / k_scale), -448, 448)), one
 * rounding from fp32; NaN stays NaN.
 * mio_rope_rows: the standalone form: x [tokens, heads, D] by (token, head) strides rotated at
 * positions[token] (int32 DEVICE [tokens]) into out (own strides, may be x); a position outside
 * [0, max_position) writes the row as zeros.
 * All three: no host sync, graph-capturable; B == 0 / total_new == 0 / tokens == 0 return 0 without
 * a launch.  Refused before any launch: null pointers (positions of the cache forms excepted), a
 * pointer off 16-byte alignment, strides negative or not multiples of 8, bad geometry, dtype,
 * rot_dim, max_position <= 0.
 * ------------------------------------------------------------------------------------------ */
int mio_rope_and_cache_varlen(const void* q, void* q_out, const void* key, const void* value, void* k_cache,
                              void* v_cache, const int32_t* block_tables, const int32_t* cu_seqlens_new,
                              const int32_t* context_lengths, const int32_t* positions, const float* cos,
                              const float* sin, const int64_t q_stride[2], const int64_t q_out_stride[2],
                              const int64_t k_stride[2], const int64_t v_stride[2], /* token, head */
                              int32_t B, int32_t total_new, int32_t H, int32_t Hkv, int32_t D, int32_t rot_dim,
                              int32_t max_position, int32_t interleaved, int32_t num_blocks, int32_t num_layers,
                              int32_t layer_idx, int32_t block_size, int32_t max_blocks_per_seq, int32_t dtype,
                              void* stream);
int mio_rope_and_cache_varlen_kv8(const void* q, void* q_out, const void* key, const void* value, void* k_cache,
                                  void* v_cache, const float* k_scale, const float* v_scale,
                                  const int32_t* block_tables, const int32_t* cu_seqlens_new,
                                  const int32_t* context_lengths, const int32_t* positions, const float* cos,
                                  const float* sin, const int64_t q_stride[2], const int64_t q_out_stride[2],
                                  const int64_t k_stride[2], const int64_t v_stride[2], int32_t B, int32_t total_new,
                                  int32_t H, int32_t Hkv, int32_t D, int32_t rot_dim, int32_t max_position,
                                  int32_t interleaved, int32_t num_blocks, int32_t num_layers, int32_t layer_idx,
                                  int32_t block_size, int32_t max_blocks_per_seq, int32_t dtype, void* stream);
int mio_rope_rows(const void* x, void* out, const int32_t* positions, const float* cos, const float* sin,
                  const int64_t x_stride[2], const int64_t out_stride[2], /* token, head */
                  int32_t tokens, int32_t heads, int32_t D, int32_t rot_dim, int32_t max_position,
                  int32_t interleaved, int32_t dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * QK-norm (csrc/qknorm_rope.hip): the per-head RMSNorm of q and k (Qwen3, Gemma 3) in front of the
 * rotation above, in one pass.  A head row x[0 .. D) becomes n[d] = x[d] * r * w[d] with
 * r = rsqrt(mean_{d < D}(x[d]^2) + eps) -- the mean over the whole head_dim, not over rot_dim -- in
 * fp32, in mio_rmsnorm_fwd's order; the first rot_dim elements of n are rotated exactly as the
 * rotary entry points rotate, the others are n itself, and the result is rounded ONCE into the
 * stored format (16 bits; e4m3(clamp(y * (1.0f / k_scale), -448, 448)) for K into an fp8 cache):
 * nothing is rounded between the norm and the rotation.  w is a DEVICE array [D] of the rows'
 * dtype, 16-byte aligned, shared by all heads of its kind (q_weight for the query heads, k_weight
 * for the key heads).  Gemma's (1 + w) form is the caller's: pass 1 + w.  A zero row gives zeros
 * (eps > 0), a NaN in a head makes that head NaN; there is no other special case.
 *
 * mio_qknorm_rope_and_cache_varlen(_kv8): mio_rope_and_cache_varlen(_kv8) with the norm: the same
 * arguments, token placement, liveness and skipping rules (a dead token writes nothing to the
 * caches and gets a zero q_out row; a token whose cache row is skipped still gets its q), with
 * q_weight / k_weight after sin and eps after dtype.  V is not normalised: its bytes are those of
 * mio_reshape_and_cache_varlen(_kv8).
 * mio_qknorm_rope_rows: mio_rope_rows with the norm (weight after sin, eps after dtype); out may be x.
 * The fused write's q_out is bit-equal to mio_qknorm_rope_rows of the same q: one device function
 * computes both.
 * Refused before any launch, next to every refusal of the rotary entry points (D, rot_dim and the
 * rest as above): eps negative or not finite, and -- where there is work -- a null norm weight or
 * one off 16-byte alignment.
 * ------------------------------------------------------------------------------------------ */
int mio_qknorm_rope_and_cache_varlen(const void* q, void* q_out, const void* key, const void* value, void* k_cache,
                                     void* v_cache, const int32_t* block_tables, const int32_t* cu_seqlens_new,
                                     const int32_t* context_lengths, const int32_t* positions, const float* cos,
                                     const float* sin, const void* q_weight, const void* k_weight,
                                     const int64_t q_stride[2], const int64_t q_out_stride[2],
                                     const int64_t k_stride[2], const int64_t v_stride[2], /* token, head */
                                     int32_t B, int32_t total_new, int32_t H, int32_t Hkv, int32_t D, int32_t rot_dim,
                                     int32_t max_position, int32_t interleaved, int32_t num_blocks, int32_t num_layers,
                                     int32_t layer_idx, int32_t block_size, int32_t max_blocks_per_seq, int32_t dtype,
                                     float eps, void* stream);
int mio_qknorm_rope_and_cache_varlen_kv8(const void* q, void* q_out, const void* key, const void* value, void* k_cache,
                                         void* v_cache, const float* k_scale, const float* v_scale,
                                         const int32_t* block_tables, const int32_t* cu_seqlens_new,
                                         const int32_t* context_lengths, const int32_t* positions, const float* cos,
                                         const float* sin, const void* q_weight, const void* k_weight,
                                         const int64_t q_stride[2], const int64_t q_out_stride[2],
                                         const int64_t k_stride[2], const int64_t v_stride[2], int32_t B,
                                         int32_t total_new, int32_t H, int32_t Hkv, int32_t D, int32_t rot_dim,
                                         int32_t max_position, int32_t interleaved, int32_t num_blocks,
                                         int32_t num_layers, int32_t layer_idx, int32_t block_size,
                                         int32_t max_blocks_per_seq, int32_t dtype, float eps, void* stream);
int mio_qknorm_rope_rows(const void* x, void* out, const int32_t* positions, const float* cos, const float* sin,
                         const void* weight, const int64_t x_stride[2], const int64_t out_stride[2], /* token, head */
                         int32_t tokens, int32_t heads, int32_t D, int32_t rot_dim, int32_t max_position,
                         int32_t interleaved, int32_t dtype, float eps, void* stream);

/* ------------------------------------------------------------------------------------------
 * Token sampling (csrc/sampling.hip): [B, V] logits to token ids in one launch -- greedy,
 * temperature, top-k, top-p and min-p, every parameter per row and read from DEVICE memory, the
 * uniforms supplied by the caller (no RNG state in the kernel: graph-capturable, reproducible).
 *
 * Per row b: x[b, 0..V) the stored logits (bf16, fp16 or fp32 -- dtype MIO_FP32 is accepted here
 * and nowhere else), row stride ld >= V in elements; T_b temperature, k_b top-k, p_b top-p, q_b
 * min-p, u_b a uniform in [0, 1).  temperature, top_p, min_p, u are fp32 [B], top_k is int32 [B]; a
 * null top_k, top_p or min_p turns that filter off for every row.
 *
 * Order.  A NaN logit counts as -inf, a +inf logit as the largest finite fp32.  Tokens are totally
 * ordered: i before j iff x_i > x_j, or x_i == x_j and i < j.  The order is exact on the stored
 * values; temperature does not change it.
 * Greedy.  T_b NaN or T_b <= 0: the first token of the order (the argmax, lowest index on ties).
 * Otherwise, with m = max x and w_i = exp((x_i - m) / T_b):
 *   1. top-k: S1 = the first k_b tokens of the order; k_b <= 0 or k_b >= V means all tokens.
 *   2. top-p over the renormalised top-k set: Z1 = sum_{S1} w,
 *      S2 = { i in S1 : sum_{j in S1, j before i} w_j < p_b * Z1 }; p_b >= 1 or NaN means off; the
 *      first token is always kept, also for p_b <= 0.
 *   3. min-p: S3 = { i in S2 : w_i >= q_b } (the ratio to the most likely token: w_max = 1);
 *      q_b <= 0 or NaN means off; the first token is always kept.
 *   4. draw: Z = sum_{S3} w, C_i = sum_{j in S3, j <= i} w_j (ascending token index); the result is
 *      the token i of S3 with C_i - w_i <= u_b * Z < C_i, u_b first clamped into [0, 1).  Should
 *      rounding carry the search past the end, the result is the last token of S3: never a token
 *      outside S3, never an index >= V.
 * A row with no finite logit returns token -1, kept count 0 and a zero probability row; it does
 * not fault and produces no NaN.
 *
 * Outputs, each optional, at least one required: tokens_out int64 [B]; kept_out int32 [B] = |S3|
 * (1 on a greedy row); probs_out fp32 [B, V] by its own row stride ld_probs >= V: w_i / Z on S3 and
 * exactly 0.0f elsewhere (one-hot on a greedy row); bytes between its rows are left alone.
 *
 * Masses are summed in 64-bit fixed point (quantum 2^-40 of w_max = 1), so every sum is exactly
 * associative and reruns are bit-identical whatever the scheduling.
 * Limits: 1 <= V <= 2^20; B >= 0 (B == 0 returns 0 without a launch); logits 16-byte aligned; ld
 * arbitrary (rows may start off a 16-byte boundary: the kernel peels heads and tails itself and
 * reads nothing outside [row, row + V)).  Asynchronous on stream; allocates nothing; no workspace.
 * Parameter values live on the device and are not validated: every out-of-range value has the
 * meaning given above.
 * Refused (< 0) before any launch: null logits, temperature or u (u may be null only when
 * tokens_out is null: nothing is drawn then), every output null, V < 1 or V > 2^20, B < 0, ld < V,
 * probs_out with ld_probs < V, an unknown dtype, logits off 16-byte alignment (or a parameter or
 * output array off its element's alignment).
 * ------------------------------------------------------------------------------------------ */
int mio_sample_tokens(const void* logits, int64_t ld, const float* temperature, const int32_t* top_k,
                      const float* top_p, const float* min_p, const float* u, int64_t* tokens_out,
                      int32_t* kept_out, float* probs_out, int64_t ld_probs, int32_t B, int32_t V,
                      int32_t dtype /* MIO_BF16 | MIO_FP16 | MIO_FP32 */, void* stream);

/* ------------------------------------------------------------------------------------------
 * Mixture-of-experts MLP for decode steps (csrc/moe.hip, csrc/moe_plan.h): a router
 * and two grouped GEMMs over stacked expert weights, the routing device data from start to end.
 *
 * Shapes.  T tokens (0 <= T <= 64), E experts (1 <= E <= 256), top_k = k (1 <= k <= min(E, 8)),
 * hidden size d, expert intermediate size I.  Activations bf16 or fp16.  Expert weights 16-bit,
 * row-major and stacked: w_up [E, I, d], w_gate [E, I, d] (SwiGLU only), w_down [E, d, I]; ldw the
 * row stride (a multiple of 8 elements, >= the row's length), expert_stride the distance between
 * experts (elements, a multiple of 8, at least one expert's extent).  Biases optional, contiguous
 * [E, I] and [E, d].  A routed row is r = t k + j: token t, slot j.
 *
 * mio_moe_route.  logits [T, E] (bf16, fp16 or fp32 -- MIO_FP32 is accepted here), row stride
 * ld >= E.  Per token:
 *   Order.  As mio_sample_tokens orders tokens: a NaN logit counts as -inf, -0 as +0.  a before b
 *     iff x_a > x_b, or x_a == x_b and a < b; exact on the STORED values, so a +inf logit sorts
 *     before every finite one (before a stored largest finite fp32 too: fp32 logits only).
 *   Choice.  ids[t, j] is the j-th expert of that order, j = 0 .. k - 1.
 *   Weights.  In the weights, and only there, a +inf logit counts as the largest finite fp32 (so
 *     x - m is never inf - inf).  m = max x, p_e = exp(x_e - m) / sum over ALL E of exp(x - m); w[t, j] = p_{ids[t, j]};
 *     with renormalize that value divided by sum_j p_{ids[t, j]} (slot order).  renormalize = 1 is
 *     Mixtral and Qwen3-MoE, 0 is OLMoE and Qwen2-MoE.  fp32.
 *   Degenerate row.  No finite logit: ids = 0 .. k - 1, all weights exactly 0; no NaN, no fault.
 * Outputs (device): ids int32 [T, k]; weights fp32 [T, k]; expert_offsets int32 [E + 1]
 * (offsets[e] = routed rows whose expert is < e; offsets[E] = T k); sorted_rows int32 [T k]
 * (positions offsets[e] .. offsets[e + 1] hold expert e's routed rows in ascending r); row_pos
 * int32 [T k], the inverse: sorted_rows[row_pos[r]] = r.  ids, offsets, sorted_rows and row_pos are
 * exactly determined by the input.
 *
 * mio_moe_up.  For sorted position p of expert e, token t = sorted_rows[p] / k:
 *   h[p, :] = silu(x[t] Wgate_e^T + bg_e) * (x[t] Wup_e^T + bu_e)       (act == SWIGLU)
 *   h[p, :] = act(x[t] Wup_e^T + bu_e)                                  (none, gelu, gelu_erf, relu, silu)
 * fp32 accumulation, one rounding to the 16-bit dtype.  Only rows p < T k of h [T k, ldh] are written.
 *
 * mio_moe_down.  y[t, :] = sum_{j = 0 .. k-1} weights[t, j] (h[row_pos[t k + j]] Wdown_e^T + bd_e)
 * + residual[t], e = ids[t, j]: fp32, the K slices in slice order, then the slots in slot order
 * j = 0, 1, ..., one rounding.  residual is optional (also where a shared expert's output goes in).
 *
 * All three: no float atomics, no counters or barriers between workgroups, the same bits on every
 * rerun; nothing allocated, nothing read back to the host; graph-capturable on one stream; T == 0
 * returns 0 and launches nothing.  Ownership: rows of x (of h) are read only for the tokens routed
 * to the expert at hand; the weights and biases of an expert with no routed row are never read;
 * nothing past [row, row + K) of any operand is read; of a workspace only the first
 * _workspace_bytes are touched.
 * K (d for up, I for down) is cut into mio_moe_{up,down}_splits(T, k, E, N, K[, act]) slices of
 * whole 32-k steps, N the output columns (I for up, d for down).  The plan is a pure function of
 * these sizes: no device value is consulted.  Up with one slice finishes in its first kernel and
 * needs no workspace; otherwise fp32 partials [splits][T k][N] (SwiGLU: two such) go to `workspace`
 * (>= mio_moe_up_workspace_bytes).  Down always runs through partials: workspace
 * >= mio_moe_down_workspace_bytes = splits * T k * N * 4 is required whenever T > 0.
 * Refused (< 0, mio_last_error() names the entry point) before any launch: T > 64 (decode steps
 * only), E or top_k out of range, K not a multiple of 8, strides short or not multiples of 8,
 * pointers off 16-byte alignment (the route's int32 / fp32 arrays: off 4), w_gate without SWIGLU or
 * SWIGLU without it, a missing workspace, an unknown dtype or activation.  The queries return < 0
 * (_splits) or 0 with the message set (_workspace_bytes) on a shape the launch refuses.
 * ------------------------------------------------------------------------------------------ */
int mio_moe_route(const void* logits, int64_t ld, int32_t* ids, float* weights, int32_t* expert_offsets,
                  int32_t* sorted_rows, int32_t* row_pos, int32_t T, int32_t E, int32_t top_k,
                  int32_t renormalize, int32_t dtype /* MIO_BF16 | MIO_FP16 | MIO_FP32 */, void* stream);
int mio_moe_up_splits(int32_t T, int32_t top_k, int32_t E, int32_t N, int32_t K, int32_t act);
size_t mio_moe_up_workspace_bytes(int32_t T, int32_t top_k, int32_t E, int32_t N, int32_t K, int32_t act);
int mio_moe_down_splits(int32_t T, int32_t top_k, int32_t E, int32_t N, int32_t K);
size_t mio_moe_down_workspace_bytes(int32_t T, int32_t top_k, int32_t E, int32_t N, int32_t K);
int mio_moe_up(const void* x, const void* w_up, const void* b_up, const void* w_gate, const void* b_gate,
               const int32_t* expert_offsets, const int32_t* sorted_rows, void* h, void* workspace,
               int32_t T, int32_t top_k, int32_t E, int32_t I, int32_t d, int64_t ldx, int64_t ldw,
               int64_t expert_stride, int64_t ldh, int32_t act, int32_t dtype, void* stream);
int mio_moe_down(const void* h, const void* w_down, const void* b_down, const int32_t* ids,
                 const float* weights, const int32_t* expert_offsets, const int32_t* row_pos,
                 const void* residual, void* y, void* workspace, int32_t T, int32_t top_k, int32_t E,
                 int32_t d, int32_t I, int64_t ldh, int64_t ldw, int64_t expert_stride, int64_t ldy,
                 int64_t ldr, int32_t dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MIO_HIP_H */

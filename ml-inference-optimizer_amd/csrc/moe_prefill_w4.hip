// Mixture-of-experts MLP for tall inputs on MXFP4 expert weights (1 <= T <= 8192 tokens): the tiled grouped GEMM of moe_prefill.hip
// over e2m1 nibbles with one e8m0 scale byte per expert, output channel and 32 k; the C-ABI entry points mio_moe_prefill_up_w4 and
// mio_moe_prefill_down_w4 (semantics: include/mio_hip.h).  Weight-only: x, h, the biases, the residual and y are bf16,
// the weights are widened EXACTLY to bf16 on their way into LDS (v_cvt_scalef32_pk_bf16_fp4, the block scale 2^(b - 127) as the
// conversion's fp32 operand b << 23, as gemm_skinny_w4_loop.inc does it) and multiplied on the bf16 v_mfma_f32_16x16x32: the
// arithmetic of the decode units (gemm_skinny_w4.hip, moe_w4.hip), so prefill and decode of one model see the same effective weights,
// and the result equals moe_prefill.hip's on the bf16 dequantisation bit for bit (the same 32-k steps in the same order per
// accumulator).  The router, the tile map, the grid (max_tiles x ceil(N / BN)), the tile (128 x 128 x 64, SwiGLU 64 up + 64 gate
// rows), the 2 x 2 waves, the x staging, the fragment reads, the MFMA loop and both read-outs are moe_prefill_common.h's, shared
// with the 16-bit unit; the plan is moe_prefill_plan.h's.  This file owns the weight staging.
//
// Weight staging.  A chunk of BK = 64 k is two MX blocks per tile row, and 128 rows x 2 blocks are 256 (row, block) pairs: one per
// thread, thread tid -> (row tid >> 1, block tid & 1).  Per chunk a thread issues one 16-byte load (the block's 32 nibbles) and one
// byte load (its scale), prefetched a chunk ahead into 5 registers where the 16-bit unit holds 16 for its weight pieces.  Behind the
// MFMAs of the current chunk it widens dword j (elements 8 j .. 8 j + 7 of the block, low nibble first) with four conversions
// into the 16-byte piece 4 block + j of the row's 128 bytes, stored at the swizzled position (4 block + j) ^ ((row >> 1) & 7): 16
// conversions and four 16-byte LDS stores per thread and chunk.  Converting at the stash and not at the fragment read matters:
// every weight fragment is read by the two waves that share its columns, so conversions on the read side would double the VALU
// work that competes with the MFMAs for issue slots.
//
// LDS store conflicts of this map, by arithmetic.  A 16-byte store is served 16 lanes at a time and is free of conflicts when
// those lanes hit 16 different 16-byte columns of the 256-byte bank line; row r of 128 bytes covers columns 8 (r & 1) .. + 7.  Lanes
// 16 g .. 16 g + 15 of wave w hold rows 8 G .. 8 G + 7 (G = 4 w + g) x both blocks b.  Write the row as
// 8 G + 2 i + o (i = 0 .. 3 the row pair, o its parity): (row >> 1) & 7 = (4 G + i) & 7 = 4 (G & 1) | i, so store j lands on column
// 8 o + ((4 b + j) ^ (4 (G & 1) | i)) = 8 o + (4 (b ^ (G & 1)) | (j ^ i)).  Over b in {0, 1} and i in {0 .. 3} the second term takes all
// 8 values once, and o picks the half: 16 lanes, 16 columns, no conflict, for every j.  (Thread -> (row tid & 127, block tid >> 7),
// which would make the global loads of a wave 64 rows apart, puts rows r .. r + 15 of ONE block on a store: 8 row pairs with
// pieces (4 b + j) ^ i, i = 0 .. 7 -- also 16 columns; the map above was chosen for its loads: the two lanes of a row read 32
// adjacent bytes.)
//
// 32 bytes per row and chunk, not 64 per row every second chunk: a row's 32 bytes are a quarter of a 128-byte line, and the three
// chunks that follow read the rest of that line out of L2; a 64-byte fetch every second chunk would halve the number of requests
// per line at the price of a second register set and a stash that differs between odd and even chunks.  Not measured against
// each other; profiles/moe_prefill_w4.md holds what was measured.
//
// What keeps every load in bounds: a block at k >= K is not loaded (its nibbles are 0x00, its scale 1.0, whatever byte lies
// there: a 0xff would make the zeros NaN) and K % 32 == 0 puts every other block inside [0, K / 2) <= ldw of its row; a tile row
// whose column is >= N has no source; expert e < E is the clamped entry of the tile map, and only experts with rows have tiles,
// so an idle expert's nibbles and scale bytes are never read; x rows as in the 16-bit unit.  No split of K, no atomics: the same
// bits on every rerun, and a captured graph replays under any routing.
#include "moe_gemm_common.h"
#include "moe_prefill_common.h"

struct MoePfW4Dev : MoePfDev {
  const uint8_t* scale;    // e8m0 [E][N, lds], experts sstride apart (bytes)
  const uint8_t* scale_g;  // SwiGLU: the gate weight's, same strides
  int64_t lds, sstride;
};

// the 8 e2m1 elements of a dword as bf16, times the block scale: a 16-byte piece of a tile row, k ascending
__device__ __forceinline__ u32x4_t moe_pf_w4_widen(uint32_t w, float sc) {
  typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
  const bf16x2_t a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 0), b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 1),
                 c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 2), d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 3);
  return (u32x4_t){__builtin_bit_cast(uint32_t, a), __builtin_bit_cast(uint32_t, b), __builtin_bit_cast(uint32_t, c),
                   __builtin_bit_cast(uint32_t, d)};
}

template <bool GLU, bool GATHER>
__global__ __launch_bounds__(MOE_PF_NT, 2) void moe_prefill_w4_gemm_kernel(const MoePfW4Dev p) {
  using T = __bf16;
  __shared__ __attribute__((aligned(16))) unsigned char lds[MOE_PF_LDS_BYTES];
  // the tile: BM sorted positions of one expert.  Past the map: nothing else is read and no barrier is met, all threads alike.
  MoePfTile t;
  if (!moe_pf_tile(p, t)) return;
  constexpr int BN = GLU ? MOE_PF_BN_GLU : MOE_PF_BN;
  const int n0 = blockIdx.y * BN;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, q = lane >> 4, wm = wave & 1, wn = wave >> 1;

  const MoePfStage st = moe_pf_stage(tid);
  const T* xsrc[MOE_PF_PPT];  // null: a row past the tile's count, zeros
  moe_pf_x_sources<T, GATHER>(p, t, st, xsrc);

  // weight staging: this thread's (tile row, MX block) of every chunk.  Tile row -> column as in the 16-bit unit: n0 + row; SwiGLU:
  // rows 0 .. 63 the up weight's columns n0 .., rows 64 .. 127 the gate weight's.  Null: a column past N, zeros.
  const int wrow = tid / MOE_PF_W4_BLOCKS, wblk = tid % MOE_PF_W4_BLOCKS;
  const uint8_t* wsrc = nullptr;  // the row's nibbles at block wblk of chunk 0 ...
  const uint8_t* ssrc = nullptr;  // ... and that block's scale byte
  {
    const int n = n0 + (GLU ? (wrow & (MOE_PF_BN_GLU - 1)) : wrow);
    const bool gate = GLU && wrow >= MOE_PF_BN_GLU;
    if (n < p.N) {
      wsrc = (const uint8_t*)(gate ? p.wg : p.w) + (int64_t)t.e * p.estride + (int64_t)n * p.ldw + 16 * wblk;
      ssrc = (gate ? p.scale_g : p.scale) + (int64_t)t.e * p.sstride + (int64_t)n * p.lds + wblk;
    }
  }
  const int woff = wrow * MOE_PF_ROWB, wswz = (wrow >> 1) & 7;

  u32x4_t rx[MOE_PF_PPT], rw;
  uint32_t rs;
  const auto fetch = [&](int k0) {
    moe_pf_fetch<T>(xsrc, k0, k0 + st.spk < p.K, rx);
    rw = (u32x4_t){0u, 0u, 0u, 0u};
    rs = 0x7fu;  // (1.0)
    if (wsrc && k0 + 32 * wblk < p.K) {
      rw = *(const u32x4_t*)(wsrc + (k0 >> 1));
      rs = ssrc[k0 >> 5];
    }
  };
  const auto stash = [&](int buf) {
    unsigned char* xt = lds + buf * 2 * MOE_PF_TILE_BYTES;
    moe_pf_stash(xt, st, rx);
    unsigned char* wt = xt + MOE_PF_TILE_BYTES + woff;
    const float sc = __uint_as_float(rs << 23);
#pragma unroll
    for (int j = 0; j < 4; ++j) *(u32x4_t*)(wt + (((4 * wblk + j) ^ wswz) * 16)) = moe_pf_w4_widen(rw[j], sc);
  };

  f32x4_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  const int nchunks = (p.K + MOE_PF_BK - 1) / MOE_PF_BK;  // (workgroup-uniform, as every barrier below)
  if (nchunks > 0) {
    fetch(0);
    stash(0);
  }
  __syncthreads();
  for (int ch = 0; ch < nchunks; ++ch) {
    const bool more = ch + 1 < nchunks;
    if (more) fetch((ch + 1) * MOE_PF_BK);
    const unsigned char* xt = lds + (ch & 1) * 2 * MOE_PF_TILE_BYTES;
    moe_pf_mma_chunk<T, GLU>(xt, xt + MOE_PF_TILE_BYTES, wm, wn, c, q, acc);
    if (more) stash((ch + 1) & 1);  // (the buffer chunk ch - 1 was read from, a barrier ago)
    __syncthreads();
  }
  // (no scale in either read-out: it went in inside the conversion)
  moe_pf_read_out<T, GLU, GATHER>(p, t, n0, wm, wn, c, q, acc);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
// What both entry points check alike: the tall-input shape rule with whole MX blocks, then the half-byte form's operand rules as
// the decode unit states them (moe_gemm_checks under SKINNY_W4 -- its T cap is the decode step's, so it is handed T 0: T was
// judged the line before) and the block scales' strides.
static int moe_pf_w4_checks(const std::string& fn, int64_t T, int32_t k, int32_t E, int32_t N, int32_t K, int32_t act, int32_t dtype,
                            int64_t ldx, int64_t ldw, int64_t estride, int64_t lds, int64_t sstride, int64_t ldy) {
  std::string err;
  if (!moe_prefill_w4_shape_ok(fn.c_str(), T, k, E, N, K, act, err)) return mio_fail(err);
  if (int rc = moe_gemm_checks(SKINNY_W4, fn, 0, k, E, N, K, act, dtype, ldx, ldw, estride, ldy)) return rc;
  return moe_block_scale_checks(fn, N, K, lds, sstride);
}

static MoePfW4Dev moe_pf_w4_args(const MoePfDev& base, const void* scale, const void* scale_g, int64_t lds, int64_t sstride) {
  MoePfW4Dev p = {};
  static_cast<MoePfDev&>(p) = base;
  p.scale = (const uint8_t*)scale; p.scale_g = (const uint8_t*)scale_g; p.lds = lds; p.sstride = sstride;
  return p;
}

extern "C" int mio_moe_prefill_up_w4(const void* x, const void* w4_up, const void* s_up, const void* b_up, const void* w4_gate,
                                     const void* s_gate, const void* b_gate, const int32_t* expert_offsets, const int32_t* sorted_rows,
                                     const int32_t* tile_expert, const int32_t* tile_row0, const int32_t* num_tiles, void* h, int32_t T,
                                     int32_t top_k, int32_t E, int32_t I, int32_t d, int64_t ldx, int64_t ldw, int64_t expert_stride,
                                     int64_t lds, int64_t scale_expert_stride, int64_t ldh, int32_t act, int32_t dtype, void* stream) {
  const std::string fn = "mio_moe_prefill_up_w4";
  if (int rc = moe_pf_w4_checks(fn, T, top_k, E, I, d, act, dtype, ldx, ldw, expert_stride, lds, scale_expert_stride, ldh)) return rc;
  const bool glu = act == MIO_ACT_SWIGLU;
  MIO_CHECK(glu == (w4_gate != nullptr) && glu == (s_gate != nullptr), fn + SKINNY_W4.moe.gate);
  MIO_CHECK(s_up != nullptr, fn + SKINNY_W4.moe.up_scale);
  if (int rc = moe_pf_up_pointer_checks(fn, x, w4_up, b_up, w4_gate, b_gate, expert_offsets, sorted_rows, tile_expert, tile_row0, num_tiles,
                                        h, T, glu, ": x, w4_up, h, expert_offsets, sorted_rows and the tile map must be non-null"))
    return rc;
  MIO_CHECK(moe_pf_aligned4(s_up) && moe_pf_aligned4(s_gate), fn + ": the block scales must be 4-byte aligned");
  if (T == 0 || I == 0) return 0;
  MoePfDev b = moe_pf_args(x, w4_up, expert_offsets, sorted_rows, tile_expert, tile_row0, num_tiles, ldx, ldw, expert_stride, T, top_k, E, I, d);
  b.wg = w4_gate; b.bias = b_up; b.bias_g = b_gate; b.y = h; b.ldy = ldh; b.act = act;
  const MoePfW4Dev p = moe_pf_w4_args(b, s_up, s_gate, lds, scale_expert_stride);
  const int bn = moe_prefill_bn(glu);
  const dim3 grid((unsigned)p.max_tiles, (unsigned)((I + bn - 1) / bn));
  if (glu) hipLaunchKernelGGL((moe_prefill_w4_gemm_kernel<true, true>), grid, dim3(MOE_PF_NT), 0, (hipStream_t)stream, p);
  else hipLaunchKernelGGL((moe_prefill_w4_gemm_kernel<false, true>), grid, dim3(MOE_PF_NT), 0, (hipStream_t)stream, p);
  return moe_launched(fn);
}

extern "C" int mio_moe_prefill_down_w4(const void* h, const void* w4_down, const void* s_down, const void* b_down, const int32_t* ids,
                                       const float* weights, const int32_t* expert_offsets, const int32_t* row_pos,
                                       const int32_t* tile_expert, const int32_t* tile_row0, const int32_t* num_tiles, const void* residual,
                                       void* y, void* workspace, int32_t T, int32_t top_k, int32_t E, int32_t d, int32_t I, int64_t ldh,
                                       int64_t ldw, int64_t expert_stride, int64_t lds, int64_t scale_expert_stride, int64_t ldy,
                                       int64_t ldr, int32_t dtype, void* stream) {
  const std::string fn = "mio_moe_prefill_down_w4";
  if (int rc = moe_pf_w4_checks(fn, T, top_k, E, d, I, MIO_ACT_NONE, dtype, ldh, ldw, expert_stride, lds, scale_expert_stride, ldy)) return rc;
  MIO_CHECK(s_down != nullptr, fn + SKINNY_W4.moe.down_scale);
  if (int rc = moe_pf_down_pointer_checks(fn, h, w4_down, b_down, ids, weights, expert_offsets, row_pos, tile_expert, tile_row0, num_tiles,
                                          residual, y, workspace, T, d, ldr,
                                          ": h, w4_down, y, ids, weights, expert_offsets, row_pos and the tile map must be non-null"))
    return rc;
  MIO_CHECK(moe_pf_aligned4(s_down), fn + ": the block scales must be 4-byte aligned");
  if (T == 0 || d == 0) return 0;
  MIO_CHECK(workspace != nullptr, fn + ": workspace required (mio_moe_prefill_down_workspace_bytes)");
  MoePfDev b = moe_pf_args(h, w4_down, expert_offsets, nullptr, tile_expert, tile_row0, num_tiles, ldh, ldw, expert_stride, T, top_k, E, d, I);
  b.ws = (float*)workspace;
  const MoePfW4Dev p = moe_pf_w4_args(b, s_down, nullptr, lds, scale_expert_stride);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL((moe_prefill_w4_gemm_kernel<false, false>), dim3((unsigned)p.max_tiles, (unsigned)((d + MOE_PF_BN - 1) / MOE_PF_BN)),
                     dim3(MOE_PF_NT), 0, st, p);
  moe_pf_launch_down_finish(dtype, p, b_down, ids, weights, row_pos, residual, y, ldy, ldr, st);
  return moe_launched(fn);
}

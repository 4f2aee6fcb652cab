// Mixture-of-experts MLP for tall inputs (1 <= T <= 8192 tokens, E <= 256 experts, top_k <= 8): a router in three launches and a
// tiled grouped GEMM; the C-ABI entry points mio_moe_prefill_route, mio_moe_prefill_up, mio_moe_prefill_down and their host
// queries (semantics: include/mio_hip.h).  The plan (tile, bound on the tile map, shape checks, workspace) is
// moe_prefill_plan.h.  The decode unit (moe.hip) streams an expert's weight once past at most 64 rows held in LDS; here a
// 128 x 64 weight tile is staged once per 128 rows of its expert, so the weight traffic of a tall input no longer grows with
// ceil(T / 64).
//
// Router.  (a) moe_prefill_tokens_kernel: a grid of 4-wave workgroups, a wave per token, moe_common.h's moe_route_token -- the
// decode router's order, choice and weights, the same text -- writes ids and weights.  (b) moe_prefill_offsets_kernel: workgroup
// e counts the routed rows whose expert is below e, which IS expert_offsets[e]; every workgroup writes one final value, so no
// launch ever reads a count another workgroup of the same launch writes.  (c) moe_prefill_place_kernel: workgroup e walks ids in
// routed-row order, 1024 rows a step, an integer prefix over the matches (wave scan, four wave totals through LDS) placing its
// rows at offsets[e] + rank: ascending by construction; it also writes its ceil(c_e / BM) tiles at the prefix of the tile counts
// of the experts below it (<= 256 offsets, read by thread).  Integers only, no atomic of any kind, no counter or barrier between
// workgroups.
//
// Grouped GEMM.  Grid max_tiles x ceil(N / BN).  A workgroup reads num_tiles and returns when its tile index is not below it:
// before any other load and before any barrier, all threads alike.  Tile: BM = 128 sorted positions of one expert x BN = 128
// output columns (SwiGLU: 64 up columns and their 64 gate columns, which fill the same 128-row weight tile, so the activation
// meets both halves in registers), BK = 64, 256 threads as 2 x 2 waves of 64 x 64 each, v_mfma_f32_16x16x32 with the weight
// fragment as the A operand: lane (c, q) then owns row c, columns 4 q .. 4 q + 3 of a 16 x 16 block, four adjacent outputs of a row.
// Both operands go through LDS in rows of 128 bytes (8 pieces of 16); piece p of row r lies at p ^ ((r >> 1) & 7), so the 16 lanes
// of a fragment read (rows r .. r + 15, one p) land on 16 different 16-byte columns of the 256-byte bank line, and so do the 16
// lanes of a store (two rows, eight pieces).  Two LDS buffers: chunk i + 1 is fetched into registers before the MFMAs of chunk
// i, stored into the other buffer behind them, one barrier per chunk.  x rows are gathered (up: x[sorted_rows[p] / k]; down:
// h[p]); rows past the tile's count, columns past N and k past K are zeros that are never read from memory.  No split of K.
// Up's epilogue is the decode units' skinny_finish (bias, activation, one rounding) into h by sorted position; down stores fp32
// rows by sorted position into the workspace and moe_common.h's moe_down_finish_kernel, at one slice, is where a token's slots
// meet.
#include "moe_prefill_common.h"

// ---- router ------------------------------------------------------------------------------------------------------------------
struct MoePfRouteDev {
  const void* logits;
  int64_t ld;
  int32_t* ids;
  float* weights;
  int32_t* offsets;
  int32_t* sorted_rows;
  int32_t* row_pos;
  int32_t* tile_expert;
  int32_t* tile_row0;
  int32_t* num_tiles;
  int T, E, topk, renorm, max_tiles;
};

constexpr int MOE_PF_RT_NT = 256, MOE_PF_RT_NW = MOE_PF_RT_NT / 64;
static_assert(MOE_E_MAX <= MOE_PF_RT_NT, "a thread per expert in the tile prefix");

template <typename L>
__global__ __launch_bounds__(MOE_PF_RT_NT) void moe_prefill_tokens_kernel(const MoePfRouteDev a) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * MOE_PF_RT_NW + (threadIdx.x >> 6);
  if (t >= a.T) return;  // (wave-uniform; no barrier in this kernel)
  int my_id;
  float my_w;
  moe_route_token((const L*)a.logits + (int64_t)t * a.ld, a.E, a.topk, a.renorm, lane, my_id, my_w);
  if (lane < a.topk) {
    a.ids[t * a.topk + lane] = my_id;
    a.weights[t * a.topk + lane] = my_w;
  }
}

// the sum of v over the workgroup's 256 threads, for every thread (s: four ints of LDS, free again on return)
__device__ __forceinline__ int moe_pf_block_sum(int v, int* s) {
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  const int sum = s[0] + s[1] + s[2] + s[3];
  __syncthreads();
  return sum;
}

__global__ __launch_bounds__(MOE_PF_RT_NT) void moe_prefill_offsets_kernel(const MoePfRouteDev a) {
  __shared__ int s_sum[MOE_PF_RT_NW];
  const int e = blockIdx.x, rows = a.T * a.topk;
  int below = 0;
  for (int r = threadIdx.x; r < rows; r += MOE_PF_RT_NT) below += a.ids[r] < e;
  below = moe_pf_block_sum(below, s_sum);
  if (threadIdx.x == 0) {
    a.offsets[e] = below;
    if (e == 0) a.offsets[a.E] = rows;
  }
}

__global__ __launch_bounds__(MOE_PF_RT_NT) void moe_prefill_place_kernel(const MoePfRouteDev a) {
  __shared__ int s_sum[MOE_PF_RT_NW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int e = blockIdx.x, rows = a.T * a.topk;
  // the tile map: this expert's tiles start at the tile counts of the experts below it
  const int mine = tid < a.E ? (a.offsets[tid + 1] - a.offsets[tid] + MOE_PF_BM - 1) / MOE_PF_BM : 0;
  const int tile0 = moe_pf_block_sum(tid < e ? mine : 0, s_sum);
  if (e == 0) {  // (workgroup-uniform)
    const int total = moe_pf_block_sum(mine, s_sum);
    if (tid == 0) *a.num_tiles = min(total, a.max_tiles);
  }
  const int lo = a.offsets[e], cnt = a.offsets[e + 1] - lo;
  for (int i = tid; i * MOE_PF_BM < cnt; i += MOE_PF_RT_NT)
    if (tile0 + i < a.max_tiles) {  // (always: moe_prefill_max_tiles bounds the sum)
      a.tile_expert[tile0 + i] = e;
      a.tile_row0[tile0 + i] = lo + i * MOE_PF_BM;
    }
  if (cnt <= 0) return;  // (workgroup-uniform)
  // this expert's rows in ascending routed-row order: thread tid looks at rows base + 4 tid .. + 3, its rank is the matches before
  int placed = 0;
  for (int base = 0; base < rows && placed < cnt; base += 4 * MOE_PF_RT_NT) {  // (workgroup-uniform)
    const int r0 = base + 4 * tid;
    bool hit[4];
    int c = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      hit[i] = r0 + i < rows && a.ids[r0 + i] == e;
      c += hit[i];
    }
    int inc = c;
    for (int o = 1; o < 64; o <<= 1) {
      const int u = __shfl_up(inc, o, 64);
      if (lane >= o) inc += u;
    }
    if (lane == 63) s_sum[wave] = inc;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < MOE_PF_RT_NW; ++w) {
      const int v = s_sum[w];
      before += w < wave ? v : 0;
      total += v;
    }
    int pos = lo + placed + before + inc - c;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (hit[i] && pos < rows) {  // (pos < lo + cnt <= rows: the offsets were counted from these ids)
        a.sorted_rows[pos] = r0 + i;
        a.row_pos[r0 + i] = pos;
        ++pos;
      }
    placed += total;
    __syncthreads();
  }
}

// ---- grouped GEMM -------------------------------------------------------------------------------------------------------------
// (the launch's arguments, the tile, the x staging, a chunk's MFMAs and the read-out: moe_prefill_common.h, shared with the MXFP4 unit)
template <typename T, bool GLU, bool GATHER>
__global__ __launch_bounds__(MOE_PF_NT, 2) void moe_prefill_gemm_kernel(const MoePfDev p) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[MOE_PF_LDS_BYTES];
  // the tile: BM sorted positions of one expert.  Past the map: nothing else is read and no barrier is met, all threads alike.
  MoePfTile t;
  if (!moe_pf_tile(p, t)) return;
  constexpr int BN = GLU ? MOE_PF_BN_GLU : MOE_PF_BN;
  const int n0 = blockIdx.y * BN;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, q = lane >> 4, wm = wave & 1, wn = wave >> 1;

  // staging: piece i of this thread is (row srow + 32 i, k 8 (tid & 7) .. + 7) of both tiles
  const MoePfStage st = moe_pf_stage(tid);
  const T* xsrc[MOE_PF_PPT];  // null: a row past the tile's count / a column past N, zeros
  const T* wsrc[MOE_PF_PPT];
  moe_pf_x_sources<T, GATHER>(p, t, st, xsrc);
#pragma unroll
  for (int i = 0; i < MOE_PF_PPT; ++i) {
    // weight tile row: column n0 + row; SwiGLU: rows 0 .. 63 the up weight's columns n0 .., rows 64 .. 127 the gate weight's
    const int row = st.srow + 32 * i;
    const int n = n0 + (GLU ? (row & (MOE_PF_BN_GLU - 1)) : row);
    const T* wb = (const T*)((GLU && row >= MOE_PF_BN_GLU) ? p.wg : p.w);
    wsrc[i] = n < p.N ? wb + (int64_t)t.e * p.estride + (int64_t)n * p.ldw + st.spk : nullptr;
  }

  u32x4_t rx[MOE_PF_PPT], rw[MOE_PF_PPT];
  const auto fetch = [&](int k0) {
    const bool kin = k0 + st.spk < p.K;
    moe_pf_fetch<T>(xsrc, k0, kin, rx);
    moe_pf_fetch<T>(wsrc, k0, kin, rw);
  };
  const auto stash = [&](int buf) {
    unsigned char* xt = lds + buf * 2 * MOE_PF_TILE_BYTES;
    moe_pf_stash(xt, st, rx);
    moe_pf_stash(xt + MOE_PF_TILE_BYTES, st, rw);
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
  moe_pf_read_out<T, GLU, GATHER>(p, t, n0, wm, wn, c, q, acc);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
using MoePfKernel = void (*)(const MoePfDev);
// [MIO_BF16 / MIO_FP16][up SwiGLU / up plain / down]
static const MoePfKernel MOE_PF_TABLE[2][3] = {
    {moe_prefill_gemm_kernel<__bf16, true, true>, moe_prefill_gemm_kernel<__bf16, false, true>, moe_prefill_gemm_kernel<__bf16, false, false>},
    {moe_prefill_gemm_kernel<_Float16, true, true>, moe_prefill_gemm_kernel<_Float16, false, true>,
     moe_prefill_gemm_kernel<_Float16, false, false>}};

extern "C" int mio_moe_prefill_max_tiles(int32_t T, int32_t top_k, int32_t E) {
  std::string err;
  if (!moe_prefill_route_shape_ok("mio_moe_prefill_max_tiles", T, top_k, E, err)) return mio_fail(err);
  return (int)moe_prefill_max_tiles(T, top_k, E);
}

extern "C" size_t mio_moe_prefill_down_workspace_bytes(int32_t T, int32_t top_k, int32_t E, int32_t N, int32_t K) {
  std::string err;
  if (!moe_prefill_shape_ok("mio_moe_prefill_down_workspace_bytes", T, top_k, E, N, K, MIO_ACT_NONE, err)) {
    mio_set_error(err);
    return 0;
  }
  return moe_prefill_down_workspace_bytes(T, top_k, N);
}

extern "C" int mio_moe_prefill_route(const void* logits, int64_t ld, int32_t* ids, float* weights, int32_t* expert_offsets,
                                     int32_t* sorted_rows, int32_t* row_pos, int32_t* tile_expert, int32_t* tile_row0,
                                     int32_t* num_tiles, int32_t T, int32_t E, int32_t top_k, int32_t renormalize, int32_t dtype,
                                     void* stream) {
  const std::string fn = "mio_moe_prefill_route";
  std::string err;
  if (!moe_prefill_route_shape_ok(fn.c_str(), T, top_k, E, err)) return mio_fail(err);
  MIO_CHECK(dtype == MIO_BF16 || dtype == MIO_FP16 || dtype == MIO_FP32, fn + ": dtype must be bf16, fp16 or fp32");
  MIO_CHECK(ld >= E, fn + ": ld < E");
  if (T == 0) return 0;
  MIO_CHECK(logits && ids && weights && expert_offsets && sorted_rows && row_pos && tile_expert && tile_row0 && num_tiles,
            fn + ": null logits or output");
  MIO_CHECK(mio_aligned16(logits), fn + ": logits must be 16-byte aligned");
  MIO_CHECK(moe_pf_aligned4(ids) && moe_pf_aligned4(weights) && moe_pf_aligned4(expert_offsets) && moe_pf_aligned4(sorted_rows) &&
                moe_pf_aligned4(row_pos) && moe_pf_aligned4(tile_expert) && moe_pf_aligned4(tile_row0) && moe_pf_aligned4(num_tiles),
            fn + ": outputs must be aligned to their element size");
  const MoePfRouteDev a = {logits, ld, ids, weights, expert_offsets, sorted_rows, row_pos, tile_expert, tile_row0, num_tiles,
                           T, E, top_k, renormalize ? 1 : 0, (int)moe_prefill_max_tiles(T, top_k, E)};
  hipStream_t st = (hipStream_t)stream;
  const dim3 tg((unsigned)((T + MOE_PF_RT_NW - 1) / MOE_PF_RT_NW)), nt(MOE_PF_RT_NT);
  if (dtype == MIO_BF16) hipLaunchKernelGGL(moe_prefill_tokens_kernel<__bf16>, tg, nt, 0, st, a);
  else if (dtype == MIO_FP16) hipLaunchKernelGGL(moe_prefill_tokens_kernel<_Float16>, tg, nt, 0, st, a);
  else hipLaunchKernelGGL(moe_prefill_tokens_kernel<float>, tg, nt, 0, st, a);
  hipLaunchKernelGGL(moe_prefill_offsets_kernel, dim3((unsigned)E), nt, 0, st, a);
  hipLaunchKernelGGL(moe_prefill_place_kernel, dim3((unsigned)E), nt, 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mio_fail(fn + " launch: " + hipGetErrorString(e));
  return 0;
}

// what mio_moe_prefill_up and mio_moe_prefill_down check alike: the grouped GEMM's operands (x rows of K, weights [E][N, ldw],
// outputs of N) and the route's arrays
static int moe_pf_gemm_checks(const std::string& fn, int64_t T, int32_t k, int32_t E, int32_t N, int32_t K, int32_t act, int32_t dtype,
                              int64_t ldx, int64_t ldw, int64_t estride, int64_t ldy) {
  std::string err;
  if (!moe_prefill_shape_ok(fn.c_str(), T, k, E, N, K, act, err)) return mio_fail(err);
  MIO_CHECK(dtype == MIO_BF16 || dtype == MIO_FP16, fn + ": dtype must be bf16 or fp16");
  MIO_CHECK(ldx % 8 == 0 && ldw % 8 == 0 && ldy % 8 == 0 && estride % 8 == 0, fn + ": row and expert strides must be multiples of 8 elements");
  MIO_CHECK(ldx >= K && ldw >= K && ldy >= N, fn + ": row stride smaller than row length");
  MIO_CHECK(N == 0 || estride >= (int64_t)(N - 1) * ldw + K, fn + ": expert_stride smaller than one expert's weight");
  return 0;
}

void moe_pf_launch_down_finish(int32_t dtype, const MoePfDev& p, const void* b_down, const int32_t* ids, const float* weights,
                               const int32_t* row_pos, const void* residual, void* y, int64_t ldy, int64_t ldr, hipStream_t st) {
  const MoeDownDev f = {p.ws, nullptr, b_down, residual, y, ids, weights, row_pos, ldy, ldr, p.T, p.topk, p.E, p.rows, p.N, 1};
  const int64_t threads = (int64_t)p.T * ((p.N + 3) / 4);
  if (dtype == MIO_BF16) hipLaunchKernelGGL((moe_down_finish_kernel<__bf16, 1>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, f);
  else hipLaunchKernelGGL((moe_down_finish_kernel<_Float16, 1>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, f);
}

extern "C" int mio_moe_prefill_up(const void* x, const void* w_up, const void* b_up, const void* w_gate, const void* b_gate,
                                  const int32_t* expert_offsets, const int32_t* sorted_rows, const int32_t* tile_expert,
                                  const int32_t* tile_row0, const int32_t* num_tiles, void* h, int32_t T, int32_t top_k, int32_t E,
                                  int32_t I, int32_t d, int64_t ldx, int64_t ldw, int64_t expert_stride, int64_t ldh, int32_t act,
                                  int32_t dtype, void* stream) {
  const std::string fn = "mio_moe_prefill_up";
  if (int rc = moe_pf_gemm_checks(fn, T, top_k, E, I, d, act, dtype, ldx, ldw, expert_stride, ldh)) return rc;
  const bool glu = act == MIO_ACT_SWIGLU;
  MIO_CHECK(glu == (w_gate != nullptr), fn + ": w_gate is required iff act == SWIGLU");
  if (int rc = moe_pf_up_pointer_checks(fn, x, w_up, b_up, w_gate, b_gate, expert_offsets, sorted_rows, tile_expert, tile_row0, num_tiles, h,
                                        T, glu, ": x, w_up, h, expert_offsets, sorted_rows and the tile map must be non-null"))
    return rc;
  if (T == 0 || I == 0) return 0;
  MoePfDev p = moe_pf_args(x, w_up, expert_offsets, sorted_rows, tile_expert, tile_row0, num_tiles, ldx, ldw, expert_stride, T, top_k, E, I, d);
  p.wg = w_gate; p.bias = b_up; p.bias_g = b_gate; p.y = h; p.ldy = ldh; p.act = act;
  const int bn = moe_prefill_bn(glu);
  hipLaunchKernelGGL(MOE_PF_TABLE[dtype == MIO_BF16 ? 0 : 1][glu ? 0 : 1], dim3((unsigned)p.max_tiles, (unsigned)((I + bn - 1) / bn)),
                     dim3(MOE_PF_NT), 0, (hipStream_t)stream, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mio_fail(fn + " launch: " + hipGetErrorString(e));
  return 0;
}

extern "C" int mio_moe_prefill_down(const void* h, const void* w_down, const void* b_down, const int32_t* ids, const float* weights,
                                    const int32_t* expert_offsets, const int32_t* row_pos, const int32_t* tile_expert,
                                    const int32_t* tile_row0, const int32_t* num_tiles, const void* residual, void* y, void* workspace,
                                    int32_t T, int32_t top_k, int32_t E, int32_t d, int32_t I, int64_t ldh, int64_t ldw,
                                    int64_t expert_stride, int64_t ldy, int64_t ldr, int32_t dtype, void* stream) {
  const std::string fn = "mio_moe_prefill_down";
  if (int rc = moe_pf_gemm_checks(fn, T, top_k, E, d, I, MIO_ACT_NONE, dtype, ldh, ldw, expert_stride, ldy)) return rc;
  if (int rc = moe_pf_down_pointer_checks(fn, h, w_down, b_down, ids, weights, expert_offsets, row_pos, tile_expert, tile_row0, num_tiles,
                                          residual, y, workspace, T, d, ldr,
                                          ": h, w_down, y, ids, weights, expert_offsets, row_pos and the tile map must be non-null"))
    return rc;
  if (T == 0 || d == 0) return 0;
  MIO_CHECK(workspace != nullptr, fn + ": workspace required (mio_moe_prefill_down_workspace_bytes)");
  MoePfDev p = moe_pf_args(h, w_down, expert_offsets, nullptr, tile_expert, tile_row0, num_tiles, ldh, ldw, expert_stride, T, top_k, E, d, I);
  p.ws = (float*)workspace;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(MOE_PF_TABLE[dtype == MIO_BF16 ? 0 : 1][2], dim3((unsigned)p.max_tiles, (unsigned)((d + MOE_PF_BN - 1) / MOE_PF_BN)),
                     dim3(MOE_PF_NT), 0, st, p);
  moe_pf_launch_down_finish(dtype, p, b_down, ids, weights, row_pos, residual, y, ldy, ldr, st);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mio_fail(fn + " launch: " + hipGetErrorString(e));
  return 0;
}

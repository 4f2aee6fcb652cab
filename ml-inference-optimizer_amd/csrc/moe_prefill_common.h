// What the tiled grouped GEMMs for tall inputs share (moe_prefill.hip: 16-bit expert weights; moe_prefill_w4.hip: MXFP4 expert
// weights), in the manner of moe_gemm_common.h.  On the device: the launch's arguments, a workgroup's tile of the map, the x
// staging (gathered through sorted_rows for up, by position for down), the MFMAs of one staged chunk and the read-out (up:
// skinny_finish into h; down: fp32 rows into the workspace).  A unit keeps its weight staging, its kernel and its extern "C"
// entry points.  On the host (the end of this file): the operand checks both units make alike, the launch's arguments, down's
// finishing launch.  The LDS layout and why it is free of bank conflicts: the header of moe_prefill.hip.
#pragma once
#include <string>

#include "moe_common.h"
#include "moe_prefill_plan.h"

struct MoePfDev {
  const void* x;     // up: the tokens [T, ldx]; down: h by sorted position [T k, ldx]
  const void* w;     // [E][N, ldw], experts expert_stride apart (16-bit: elements; MXFP4: bytes)
  const void* wg;    // SwiGLU: the gate weight, same strides
  const void* bias;  // up: [E, N] or null
  const void* bias_g;
  void* y;           // up: h [T k, ldy]
  float* ws;         // down: fp32 rows [T k][N] by sorted position
  const int32_t* offsets;
  const int32_t* sorted_rows;
  const int32_t* tile_expert;
  const int32_t* tile_row0;
  const int32_t* num_tiles;
  int64_t ldx, ldw, estride, ldy;
  int T, topk, E, rows, N, K, act, max_tiles;
};

constexpr int MOE_PF_ROWB = MOE_PF_BK * 2;                    // bytes of a tile row in LDS
constexpr int MOE_PF_PPT = MOE_PF_BM * 8 / MOE_PF_NT;         // 16-byte pieces of one 16-bit operand's chunk per thread
static_assert(MOE_PF_ROWB == 128 && MOE_PF_PPT == 4 && MOE_PF_NT / 8 * MOE_PF_PPT == MOE_PF_BM, "staging pattern: thread -> (row, piece)");

// The workgroup's tile: BM sorted positions [row0, row0 + cnt) of expert e.  False past the map or on an empty tile: the caller
// returns, having read nothing else and met no barrier, all threads alike.
struct MoePfTile {
  int e, row0, cnt;
};
__device__ __forceinline__ bool moe_pf_tile(const MoePfDev& p, MoePfTile& t) {
  const int tile = blockIdx.x;
  if (tile >= min(*p.num_tiles, p.max_tiles)) return false;
  t.e = min(max(p.tile_expert[tile], 0), p.E - 1);
  t.row0 = min(max(p.tile_row0[tile], 0), p.rows);
  t.cnt = min(MOE_PF_BM, min(p.offsets[t.e + 1], p.rows) - t.row0);
  return t.cnt > 0;
}

// Staging of a 16-bit operand: piece i of a thread is (row srow + 32 i, k 8 (tid & 7) .. + 7) of the tile, stored at soff + i * 32
// rows; the swizzle does not depend on i.
struct MoePfStage {
  int srow, spk, soff;
};
__device__ __forceinline__ MoePfStage moe_pf_stage(int tid) {
  const int srow = tid >> 3;
  return {srow, (tid & 7) * 8, srow * MOE_PF_ROWB + (((tid & 7) ^ ((srow >> 1) & 7)) * 16)};
}

// the x rows a thread stages: null for a row past the tile's count (zeros, never read)
template <typename T, bool GATHER>
__device__ __forceinline__ void moe_pf_x_sources(const MoePfDev& p, const MoePfTile& t, const MoePfStage& s, const T* (&xsrc)[MOE_PF_PPT]) {
#pragma unroll
  for (int i = 0; i < MOE_PF_PPT; ++i) {
    const int row = s.srow + 32 * i;
    xsrc[i] = nullptr;
    if (row < t.cnt) {
      const int pos = t.row0 + row;
      const int src = GATHER ? min(max(p.sorted_rows[pos] / p.topk, 0), p.T - 1) : pos;
      xsrc[i] = (const T*)p.x + (int64_t)src * p.ldx + s.spk;
    }
  }
}

// a thread's pieces of a 16-bit operand at k0 (K % 8 == 0: a piece lies inside [0, K) or past it; kin: inside)
template <typename T>
__device__ __forceinline__ void moe_pf_fetch(const T* const (&src)[MOE_PF_PPT], int k0, bool kin, u32x4_t (&r)[MOE_PF_PPT]) {
#pragma unroll
  for (int i = 0; i < MOE_PF_PPT; ++i) {
    r[i] = (u32x4_t){0u, 0u, 0u, 0u};
    if (kin && src[i]) r[i] = *(const u32x4_t*)(src[i] + k0);
  }
}
__device__ __forceinline__ void moe_pf_stash(unsigned char* tile, const MoePfStage& s, const u32x4_t (&r)[MOE_PF_PPT]) {
#pragma unroll
  for (int i = 0; i < MOE_PF_PPT; ++i) *(u32x4_t*)(tile + s.soff + i * 32 * MOE_PF_ROWB) = r[i];
}

// The MFMAs of one staged chunk: the x tile at xt, the weight tile at wt, both as 16-bit rows of 128 bytes.  Wave (wm, wn), lane
// (c, q): x rows wm 64 + 16 i + c; weight tile rows wrow(j) + c (plain: wn 64 + 16 j; SwiGLU: j < 2 up, j >= 2 gate).  Every
// accumulator sees the chunk's two 32-k steps in ascending order.
template <typename T, bool GLU>
__device__ __forceinline__ void moe_pf_mma_chunk(const unsigned char* xt, const unsigned char* wt, int wm, int wn, int c, int q,
                                                 f32x4_t (&acc)[4][4]) {
  using X8 = typename DT<T>::x8;
  constexpr int WN = (GLU ? MOE_PF_BN_GLU : MOE_PF_BN) / 2;  // output columns of a wave
  const auto wrow = [&](int j) { return GLU ? (j >> 1) * MOE_PF_BN_GLU + wn * WN + 16 * (j & 1) : wn * WN + 16 * j; };
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    const int lro = c * MOE_PF_ROWB + (((ks * 4 + q) ^ (c >> 1)) * 16);
    X8 a[4], b[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) b[i] = __builtin_bit_cast(X8, *(const u32x4_t*)(xt + (wm * 64 + 16 * i) * MOE_PF_ROWB + lro));
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] = __builtin_bit_cast(X8, *(const u32x4_t*)(wt + wrow(j) * MOE_PF_ROWB + lro));
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = DT<T>::mfma16(a[j], b[i], acc[i][j]);
  }
}

// The read-out.  Lane (c, q): rows wm 64 + 16 i + c of the tile, i.e. sorted positions row0 + that, columns n .. n + 3.  Up
// (GATHER): bias, activation and the one rounding into h; down: fp32 rows into the workspace.
template <typename T, bool GLU, bool GATHER>
__device__ __forceinline__ void moe_pf_read_out(const MoePfDev& p, const MoePfTile& t, int n0, int wm, int wn, int c, int q,
                                                const f32x4_t (&acc)[4][4]) {
  constexpr int WN = (GLU ? MOE_PF_BN_GLU : MOE_PF_BN) / 2;
  SkinnyFinish f = {};
  if constexpr (GATHER) {
    f.bias = p.bias ? (const char*)p.bias + (int64_t)t.e * p.N * 2 : nullptr;
    f.bias_g = p.bias_g ? (const char*)p.bias_g + (int64_t)t.e * p.N * 2 : nullptr;
    f.y = p.y;
    f.ldy = p.ldy;
    f.N = p.N;
    f.act = p.act;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = wm * 64 + 16 * i + c;
    if (m >= t.cnt) continue;
    const int pos = t.row0 + m;
#pragma unroll
    for (int j = 0; j < (GLU ? 2 : 4); ++j) {
      const int n = n0 + wn * WN + 16 * j + 4 * q;
      if (n >= p.N) continue;
      if constexpr (GATHER) {
        const float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
        float g[4] = {0.f, 0.f, 0.f, 0.f};
        if constexpr (GLU) {
#pragma unroll
          for (int u = 0; u < 4; ++u) g[u] = acc[i][j + 2][u];
        }
        skinny_finish<T, GLU, false>(f, pos, n, v, g);
      } else {
        float* dst = p.ws + (int64_t)pos * p.N + n;
        if ((p.N & 3) == 0) {  // (n + 3 < N then, and the rows are 16-byte aligned)
          *(f32x4_t*)dst = acc[i][j];
        } else {
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (n + u < p.N) dst[u] = acc[i][j][u];
        }
      }
    }
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
static inline bool moe_pf_aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

static inline MoePfDev moe_pf_args(const void* x, const void* w, const int32_t* offsets, const int32_t* sorted_rows, const int32_t* tile_expert,
                                   const int32_t* tile_row0, const int32_t* num_tiles, int64_t ldx, int64_t ldw, int64_t estride, int32_t T,
                                   int32_t k, int32_t E, int32_t N, int32_t K) {
  MoePfDev p = {};
  p.x = x; p.w = w;
  p.offsets = offsets; p.sorted_rows = sorted_rows; p.tile_expert = tile_expert; p.tile_row0 = tile_row0; p.num_tiles = num_tiles;
  p.ldx = ldx; p.ldw = ldw; p.estride = estride;
  p.T = T; p.topk = k; p.E = E; p.rows = T * k; p.N = N; p.K = K; p.act = MIO_ACT_NONE;
  p.max_tiles = (int)moe_prefill_max_tiles(T, k, E);
  return p;
}

// What up checks behind its unit's shape and stride checks, whatever the weight form: the gate rule's bias half, the pointers a
// launch needs, the alignment of everything but the weights' scales.
static inline int moe_pf_up_pointer_checks(const std::string& fn, const void* x, const void* w_up, const void* b_up, const void* w_gate,
                                           const void* b_gate, const int32_t* expert_offsets, const int32_t* sorted_rows,
                                           const int32_t* tile_expert, const int32_t* tile_row0, const int32_t* num_tiles, const void* h,
                                           int32_t T, bool glu, const char* names) {
  MIO_CHECK(glu || b_gate == nullptr, fn + ": b_gate belongs to act == SWIGLU");
  MIO_CHECK(w_up && (T == 0 || (x && h && expert_offsets && sorted_rows && tile_expert && tile_row0 && num_tiles)), fn + names);
  MIO_CHECK(mio_aligned16(x) && mio_aligned16(w_up) && mio_aligned16(w_gate) && mio_aligned16(b_up) && mio_aligned16(b_gate) &&
                mio_aligned16(h) && moe_pf_aligned4(expert_offsets) && moe_pf_aligned4(sorted_rows) && moe_pf_aligned4(tile_expert) &&
                moe_pf_aligned4(tile_row0) && moe_pf_aligned4(num_tiles),
            fn + ": pointers must be 16-byte aligned (the route's arrays: 4-byte)");
  return 0;
}

// the same for down; the workspace is asked for by the caller behind the empty call
static inline int moe_pf_down_pointer_checks(const std::string& fn, const void* h, const void* w_down, const void* b_down, const int32_t* ids,
                                             const float* weights, const int32_t* expert_offsets, const int32_t* row_pos,
                                             const int32_t* tile_expert, const int32_t* tile_row0, const int32_t* num_tiles,
                                             const void* residual, const void* y, const void* workspace, int32_t T, int32_t d, int64_t ldr,
                                             const char* names) {
  MIO_CHECK(!residual || (ldr % 8 == 0 && ldr >= d), fn + ": ldr must be a multiple of 8 elements and at least d");
  MIO_CHECK(w_down && (T == 0 || (h && y && ids && weights && expert_offsets && row_pos && tile_expert && tile_row0 && num_tiles)), fn + names);
  MIO_CHECK(mio_aligned16(h) && mio_aligned16(w_down) && mio_aligned16(b_down) && mio_aligned16(residual) && mio_aligned16(y) &&
                mio_aligned16(workspace) && moe_pf_aligned4(ids) && moe_pf_aligned4(weights) && moe_pf_aligned4(expert_offsets) &&
                moe_pf_aligned4(row_pos) && moe_pf_aligned4(tile_expert) && moe_pf_aligned4(tile_row0) && moe_pf_aligned4(num_tiles),
            fn + ": pointers must be 16-byte aligned (the route's arrays: 4-byte)");
  return 0;
}

// Down's finishing launch behind a unit's grouped GEMM, on the fp32 rows p.ws: moe_down_finish_kernel<T, 1> at one slice.  Defined
// in moe_prefill.hip, which owns that kernel's symbol; the MXFP4 unit calls it, so the library carries one instance.
void moe_pf_launch_down_finish(int32_t dtype, const MoePfDev& p, const void* b_down, const int32_t* ids, const float* weights,
                               const int32_t* row_pos, const void* residual, void* y, int64_t ldy, int64_t ldr, hipStream_t st);

// Mixture-of-experts decode step on weight-only FP8 expert weights (T <= 64 tokens, E <= 256 experts, top_k <= 8): the grouped
// GEMM of moe.hip over e4m3fn weight bytes with one fp32 scale per expert and output channel; the C-ABI entry points
// mio_moe_up_w8, mio_moe_down_w8 and their host queries (semantics: include/mio_hip.h).  The router is moe.hip's:
// the routing arrays are read as mio_moe_route wrote them.  The plan is moe_plan.h under the form SKINNY_W8; the slice range, the
// slice sum, the partial store and the epilogue are gemm_skinny_plan.h's skinny_slice_range and gemm_skinny_common.h's
// skinny_slice_sum, skinny_write and skinny_finish<.., SCALED = true>, the ones the FP8 decode-step GEMM (gemm_skinny_w8.hip) runs.
// Every e4m3fn value is exact in bf16 and fp16: the bytes are widened in registers at scale 1 (kv8_to_x8) and multiplied on the
// 16-bit MFMA.  FP8 is a storage form of the expert weights here, not a compute precision.
//
// The kernel is two designs put together.
//   From the 16-bit grouped kernel (moe.hip).  Grid (ceil(N / 64), slices, E).  A workgroup reads offsets[e], offsets[e + 1],
//   clamped into [0, T k], and returns at once when its expert has no rows: before any weight load and before any barrier, the
//   same for all its threads.  The x stage gathers rows through sorted_rows (up: routed row / top_k is the token) or by sorted
//   position (down: h is stored that way); each thread resolves the rows behind its XPT pieces once, before the loop.  Rows past
//   the expert's count are zeros that are never read from memory.  The kernel is built for the host's bound on an expert's rows,
//   MF = ceil(T / 16) fragments; a workgroup stores to LDS and multiplies only the nf = ceil(count / 16) fragments its expert reaches.
//   From the FP8 decode-step GEMM (gemm_skinny_w8.hip).  Lane (c, q) = (lane & 15, lane >> 4) loads the 16 bytes of weight row
//   n0 + c at k0 + 16 q, k0 the begin of a 64-k step; that one load feeds two v_mfma_f32_16x16x32: MFMA j takes bytes 8 j .. 8 j + 7
//   as the lane's 8 A elements and the 16-byte piece k0 / 8 + 2 q + j of x row c, read from LDS, as its B operand.  x is staged
//   through LDS in whole rows, piece p of row r at p ^ (r & 15), two buffers, one barrier per chunk.  The weight registers are a
//   ring of SKINNY_W8.sets(GLU) chunks; the x pieces of a chunk are requested immediately BEFORE that chunk's weight loads and
//   stored to LDS only when the chunk is due: the vector memory counter retires loads in issue order, so waiting for an x load
//   issued behind younger weight loads would drain the ring.
//   Its own part: the scales.  They stay out of the K loop; partials are unscaled fp32 sums by sorted position.  The epilogues
//   apply z = fma(sum, scale[e, n], bias[e, n]): up's in the first kernel with one slice, up's reduce launch, and down's
//   finishing launch, where the scale of the slot's expert goes in before the routing weight (slot order and the one rounding as
//   in moe_down_finish_kernel).
//
// What keeps every load in bounds (K % 16 == 0, ldw % 16 == 0 and expert_stride % 16 == 0 in bytes, ldw >= K):
//   * a weight load is issued only for k < ke <= K, k a multiple of 16: its 16 bytes end at or before K;
//   * the weight row is min(n0 + c, N - 1) of expert e < E: a lane past the last column computes a copy of the last row and
//     stores nothing;
//   * x rows past the expert's count and x pieces at k >= ke are zeros written to LDS, never read from memory; a gathered row
//     index is clamped into [0, T - 1] (up) or is a sorted position < T k (down); weight bytes not loaded are 0x00, which is +0.0,
//     so no padding byte of any operand reaches a product;
//   * scales and biases are read at (e, min(n, N - 1)) of an expert that has rows.
#include "gemm_skinny_common.h"
#include "kv8_cvt.h"
#include "moe_plan.h"

constexpr SkinnyForm W8 = SKINNY_W8;  // this unit's weight form (gemm_skinny_plan.h)
constexpr int MOEW8_KSTEP = W8.kstep;

struct MoeW8Dev {
  const void* x;         // up: the tokens [T, ldx]; down: h by sorted position [T k, ldx]
  const void* w;         // e4m3fn bytes [E][N, ldw], experts expert_stride bytes apart
  const void* wg;        // SwiGLU: the gate weight, same strides
  const float* scale;    // [E, N] fp32
  const float* scale_g;  // SwiGLU: the gate weight's
  const void* bias;      // [E, N] or null
  const void* bias_g;
  void* y;               // up with one slice: h [T k, ldy]
  float* ws;             // fp32 partials [nsplit][T k][N] by sorted position (SwiGLU: then the gate half); null: finish in the kernel
  const int32_t* offsets;
  const int32_t* sorted_rows;  // up: routed row of a sorted position; null (down): x rows ARE sorted positions
  int64_t ldx, ldw, estride, ldy;
  int T, topk, E, rows, N, K, act, nsplit, steps;
};

// the epilogue's arguments for expert e: its scales and biases, no residual
__device__ __forceinline__ SkinnyFinish moe_w8_finish_args(const MoeW8Dev& p, int e) {
  SkinnyFinish f = {};
  f.bias = p.bias ? (const char*)p.bias + (int64_t)e * p.N * 2 : nullptr;
  f.bias_g = p.bias_g ? (const char*)p.bias_g + (int64_t)e * p.N * 2 : nullptr;
  f.y = p.y;
  f.ldy = p.ldy;
  f.N = p.N;
  f.act = p.act;
  f.scale = p.scale + (int64_t)e * p.N;
  f.scale_g = p.scale_g ? p.scale_g + (int64_t)e * p.N : nullptr;
  return f;
}

template <typename T, int MF, bool GLU>
__global__ __launch_bounds__(256) void moe_gemm_w8_kernel(const MoeW8Dev p) {
  using X8 = typename DT<T>::x8;
  constexpr int SKC = W8.chunk(GLU);  // k per chunk
  constexpr int D = W8.sets(GLU);     // register sets in the ring
  constexpr int KS = SKC / MOEW8_KSTEP, PCS = SKC / 8, ROWS = MF * 16, ROWB = SKC * 2;
  constexpr int XPT = ROWS * PCS / 256;  // 16-byte pieces of the x chunk per thread
  static_assert(PCS >= 16 && ROWS * PCS % 256 == 0 && SKC % MOEW8_KSTEP == 0 && D >= 2, "chunk shape");
  __shared__ __attribute__((aligned(16))) char sx[2][ROWS * ROWB];

  // the expert's rows: sorted positions [r0, r0 + cnt).  No rows: nothing of this expert is read and no barrier is met, the same
  // for all the workgroup's threads.
  const int e = blockIdx.z;
  const int r0 = max(0, min(p.offsets[e], p.rows));
  const int cnt = min(min(p.offsets[e + 1], p.rows) - r0, MF * 16);  // (an expert has at most T <= 16 MF rows)
  if (cnt <= 0) return;
  const int nf = (cnt + 15) >> 4;  // live row fragments (workgroup-uniform)

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, q = lane >> 4;
  const int n0 = blockIdx.x * SKINNY_BN + wave * 16;
  const bool active = n0 < p.N;  // (a wave past the last column stages x and keeps the barriers, nothing else)
  const int s = blockIdx.y;
  int kb, ke;
  skinny_slice_range(p.steps, p.nsplit, MOEW8_KSTEP, p.K, s, kb, ke);
  const int nc = (ke - kb + SKC - 1) / SKC;

  const int nrow = min(n0 + c, p.N - 1);
  const int64_t woff = (int64_t)e * p.estride + (int64_t)nrow * p.ldw;
  const uint8_t* wrow = (const uint8_t*)p.w + woff;
  const uint8_t* grow = GLU ? (const uint8_t*)p.wg + woff : nullptr;
  const T* xg = (const T*)p.x;

  // the x row behind each piece this thread stages (the same for every chunk); -1: a row past the expert's count
  int xsrc[XPT];
#pragma unroll
  for (int i = 0; i < XPT; ++i) {
    const int row = (tid + i * 256) / PCS;
    xsrc[i] = -1;
    if (row < cnt) {
      const int pos = r0 + row;
      xsrc[i] = p.sorted_rows ? min(max(p.sorted_rows[pos] / p.topk, 0), p.T - 1) : pos;
    }
  }

  auto load_w = [&](u32x4_t (&wr)[KS], u32x4_t (&gr)[GLU ? KS : 1], int ch) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int k = kb + ch * SKC + ks * MOEW8_KSTEP + 16 * q;
      const bool ok = active && k < ke;
      wr[ks] = (u32x4_t){0u, 0u, 0u, 0u};
      if (ok) wr[ks] = *(const u32x4_t*)(wrow + k);
      if constexpr (GLU) {
        gr[ks] = (u32x4_t){0u, 0u, 0u, 0u};
        if (ok) gr[ks] = *(const u32x4_t*)(grow + k);
      }
    }
  };
  auto load_x = [&](u32x4_t (&v)[XPT], int ch) {
#pragma unroll
    for (int i = 0; i < XPT; ++i) {
      const int k = kb + ch * SKC + ((tid + i * 256) % PCS) * 8;
      v[i] = (u32x4_t){0u, 0u, 0u, 0u};
      if (xsrc[i] >= 0 && k < ke) v[i] = *(const u32x4_t*)(xg + (int64_t)xsrc[i] * p.ldx + k);
    }
  };
  auto put_x = [&](const u32x4_t (&v)[XPT], int buf) {
#pragma unroll
    for (int i = 0; i < XPT; ++i) {
      const int idx = tid + i * 256, row = idx / PCS, pc = idx % PCS;
      if (row < nf * 16) *(u32x4_t*)(sx[buf] + row * ROWB + ((pc ^ (row & 15)) * 16)) = v[i];
    }
  };

  f32x4_t acc[MF], accg[GLU ? MF : 1];
#pragma unroll
  for (int mf = 0; mf < MF; ++mf) {
    acc[mf] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    if constexpr (GLU) accg[mf] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  }
  auto compute = [&](const u32x4_t (&wr)[KS], const u32x4_t (&gr)[GLU ? KS : 1], int buf) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {  // bytes 8 j .. 8 j + 7 of the piece: k0 + 16 q + 8 j, x piece ks * 8 + 2 q + j
        const X8 wf = kv8_to_x8<T>((u32x2_t){wr[ks][2 * j], wr[ks][2 * j + 1]});
        X8 gf;
        if constexpr (GLU) gf = kv8_to_x8<T>((u32x2_t){gr[ks][2 * j], gr[ks][2 * j + 1]});
#pragma unroll
        for (int mf = 0; mf < MF; ++mf) {
          if (mf < nf) {  // (workgroup-uniform)
            const X8 xf = __builtin_bit_cast(X8, *(const u32x4_t*)(sx[buf] + (mf * 16 + c) * ROWB + (((ks * 8 + 2 * q + j) ^ c) * 16)));
            acc[mf] = DT<T>::mfma16(wf, xf, acc[mf]);
            if constexpr (GLU) accg[mf] = DT<T>::mfma16(gf, xf, accg[mf]);
          }
        }
      }
    }
  };

  // A ring of D register sets.  Chunk ch lives in set ch % D: its x pieces and then its weight bytes are requested D - 1 chunks
  // ahead, into the set the chunk before the current one has just left.  One barrier per chunk: the x buffer written for chunk
  // ch was last read for chunk ch - 2, before the barrier of chunk ch - 1.
  u32x4_t wr[D][KS], gr[D][GLU ? KS : 1], xr[D][XPT];
#pragma unroll
  for (int j = 0; j < D - 1; ++j)
    if (j < nc) {
      load_x(xr[j], j);
      load_w(wr[j], gr[j], j);
    }
  for (int ch = 0; ch < nc; ch += D) {
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const int cur = ch + j;
      if (cur < nc) {  // (the same in every thread of the workgroup)
        put_x(xr[j], cur & 1);
        __syncthreads();
        if (cur + D - 1 < nc) {
          load_x(xr[(j + D - 1) % D], cur + D - 1);
          load_w(wr[(j + D - 1) % D], gr[(j + D - 1) % D], cur + D - 1);
        }
        compute(wr[j], gr[j], cur & 1);
      }
    }
  }

  if (!active) return;
  const int n = n0 + 4 * q;
  if (n >= p.N) return;
  // lane (c, q): rows 16 mf + c of the expert, i.e. sorted positions r0 + 16 mf + c, columns n .. n + 3: unscaled partials, or
  // the scaled epilogue with the expert's scale and bias rows
  skinny_write<T, MF, GLU, true>(moe_w8_finish_args(p, e), p.ws, p.nsplit, p.rows, s, c, n, r0, cnt, acc, accg);
}

// Up's second launch: one thread per (sorted position, 4 columns) sums the slices' partials in index order and runs the scaled
// epilogue with the scales and biases of the position's expert: the e with offsets[e] <= pos < offsets[e + 1].
template <typename T, bool GLU>
__global__ __launch_bounds__(256) void moe_up_w8_reduce_kernel(const MoeW8Dev p) {
  const int ngrp = (p.N + 3) / 4;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)p.rows * ngrp) return;
  const int pos = (int)(idx / ngrp), n = (int)(idx % ngrp) * 4;
  int lo = 0, hi = p.E - 1;
  while (lo < hi) {  // the largest e with offsets[e] <= pos (offsets[0] = 0; empty experts repeat an offset)
    const int mid = (lo + hi + 1) >> 1;
    if (p.offsets[mid] <= pos) lo = mid;
    else hi = mid - 1;
  }
  float v[4], g[4];
  skinny_slice_sum<GLU>(p.ws, p.nsplit, (int64_t)p.rows * p.N, p.N, pos, n, v, g);
  skinny_finish<T, GLU, true>(moe_w8_finish_args(p, lo), pos, n, v, g);
}

// Down's second launch, the scaled sibling of moe_common.h's moe_down_finish_kernel: one thread per (token, 4 columns).  Per slot
// j in order: the slices' partials of the slot's sorted position in slice order, z = fma(sum, scale[e, n], bias[e, n]) with the
// slot's expert e, times the routing weight; then the residual and the one rounding.
struct MoeDownW8Dev {
  const float* ws;
  const float* scale;  // [E, N] fp32
  const void* bias;    // [E, N] or null
  const void* res;
  void* y;
  const int32_t* ids;
  const float* weights;
  const int32_t* row_pos;
  int64_t ldy, ldr;
  int T, topk, E, rows, N, nsplit;
};

template <typename T>
__global__ __launch_bounds__(256) void moe_down_w8_finish_kernel(const MoeDownW8Dev p) {
  const int ngrp = (p.N + 3) / 4;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)p.T * ngrp) return;
  const int t = (int)(idx / ngrp), n = (int)(idx % ngrp) * 4;
  const int64_t plane = (int64_t)p.rows * p.N;
  const T* bias = (const T*)p.bias;
  float o[4] = {0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < p.topk; ++j) {
    const int r = t * p.topk + j;
    const int e = min(max(p.ids[r], 0), p.E - 1);
    const int pos = min(max(p.row_pos[r], 0), p.rows - 1);
    const float wj = p.weights[r];
    float z[4], unused[4];
    skinny_slice_sum<false>(p.ws, p.nsplit, plane, p.N, pos, n, z, unused);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int nn = n + i < p.N ? n + i : p.N - 1;  // (clamped: computed, not stored)
      const int64_t at = (int64_t)e * p.N + nn;
      const float zz = __builtin_fmaf(z[i], p.scale[at], bias ? (float)bias[at] : 0.f);
      o[i] = j == 0 ? wj * zz : o[i] + wj * zz;
    }
  }
  const T* rrow = p.res ? (const T*)p.res + (int64_t)t * p.ldr : nullptr;
  T* yrow = (T*)p.y + (int64_t)t * p.ldy;
  if (rrow) {
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] += (float)rrow[n + i < p.N ? n + i : p.N - 1];
  }
  if (n + 3 < p.N) {
    *(u32x2_t*)(yrow + n) = (u32x2_t){pack2<T>(o[0], o[1]), pack2<T>(o[2], o[3])};
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (n + i < p.N) yrow[n + i] = (T)o[i];
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
using MoeW8Kernel = void (*)(const MoeW8Dev);
struct MoeW8Kernels {
  MoeW8Kernel main[4], reduce;
};
#define MOE_W8_KERNELS(T, GLU)                                                                                                 \
  {{moe_gemm_w8_kernel<T, 1, GLU>, moe_gemm_w8_kernel<T, 2, GLU>, moe_gemm_w8_kernel<T, 3, GLU>, moe_gemm_w8_kernel<T, 4, GLU>}, \
   moe_up_w8_reduce_kernel<T, GLU>}
// [MIO_BF16 / MIO_FP16][SwiGLU / plain]
static const MoeW8Kernels MOE_W8_TABLE[2][2] = {{MOE_W8_KERNELS(__bf16, true), MOE_W8_KERNELS(__bf16, false)},
                                                {MOE_W8_KERNELS(_Float16, true), MOE_W8_KERNELS(_Float16, false)}};
#undef MOE_W8_KERNELS

static inline bool moe_w8_aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

// what mio_moe_up_w8 and mio_moe_down_w8 check alike: the grouped GEMM's operands (x rows of K 16-bit elements, weights [E][N, ldw]
// in bytes, outputs of N)
static int moe_w8_gemm_checks(const std::string& fn, int64_t T, int32_t k, int32_t E, int32_t N, int32_t K, int32_t act, int32_t dtype,
                              int64_t ldx, int64_t ldw, int64_t estride, int64_t ldy) {
  std::string err;
  if (!moe_shape_ok(W8, fn.c_str(), T, k, E, N, K, act, err)) return mio_fail(err);
  MIO_CHECK(dtype == MIO_BF16 || dtype == MIO_FP16, fn + ": dtype must be bf16 or fp16 (the activations'; the weights are e4m3fn bytes)");
  MIO_CHECK(ldw % W8.ldw_multiple == 0 && estride % W8.ldw_multiple == 0, fn + ": ldw and expert_stride must be multiples of 16 bytes");
  MIO_CHECK(ldx % 8 == 0 && ldy % 8 == 0, fn + ": activation row strides must be multiples of 8 elements");
  MIO_CHECK(ldx >= K && ldw >= K && ldy >= N, fn + ": row stride smaller than row length");
  MIO_CHECK(N == 0 || estride >= (int64_t)(N - 1) * ldw + K, fn + ": expert_stride smaller than one expert's weight");
  return 0;
}

static int moe_w8_query_splits(const char* who, int32_t T, int32_t k, int32_t E, int32_t N, int32_t K, int32_t act) {
  std::string err;
  if (!moe_shape_ok(W8, who, T, k, E, N, K, act, err)) return mio_fail(err);
  return moe_plan(W8, T, k, E, N, K, act).nsplit;
}

extern "C" int mio_moe_up_w8_splits(int32_t T, int32_t top_k, int32_t E, int32_t N, int32_t K, int32_t act) {
  return moe_w8_query_splits("mio_moe_up_w8_splits", T, top_k, E, N, K, act);
}

extern "C" size_t mio_moe_up_w8_workspace_bytes(int32_t T, int32_t top_k, int32_t E, int32_t N, int32_t K, int32_t act) {
  std::string err;
  if (!moe_shape_ok(W8, "mio_moe_up_w8_workspace_bytes", T, top_k, E, N, K, act, err)) {
    mio_set_error(err);
    return 0;
  }
  return moe_up_workspace_bytes(moe_plan(W8, T, top_k, E, N, K, act), N);
}

extern "C" int mio_moe_down_w8_splits(int32_t T, int32_t top_k, int32_t E, int32_t N, int32_t K) {
  return moe_w8_query_splits("mio_moe_down_w8_splits", T, top_k, E, N, K, MIO_ACT_NONE);
}

extern "C" size_t mio_moe_down_w8_workspace_bytes(int32_t T, int32_t top_k, int32_t E, int32_t N, int32_t K) {
  std::string err;
  if (!moe_shape_ok(W8, "mio_moe_down_w8_workspace_bytes", T, top_k, E, N, K, MIO_ACT_NONE, err)) {
    mio_set_error(err);
    return 0;
  }
  return moe_down_workspace_bytes(moe_plan(W8, T, top_k, E, N, K, MIO_ACT_NONE), N);
}

extern "C" int mio_moe_up_w8(const void* x, const void* w8_up, const float* s_up, const void* b_up, const void* w8_gate,
                             const float* s_gate, const void* b_gate, const int32_t* expert_offsets, const int32_t* sorted_rows,
                             void* h, void* workspace, int32_t T, int32_t top_k, int32_t E, int32_t I, int32_t d, int64_t ldx,
                             int64_t ldw, int64_t expert_stride, int64_t ldh, int32_t act, int32_t dtype, void* stream) {
  const std::string fn = "mio_moe_up_w8";
  if (int rc = moe_w8_gemm_checks(fn, T, top_k, E, I, d, act, dtype, ldx, ldw, expert_stride, ldh)) return rc;
  const bool glu = act == MIO_ACT_SWIGLU;
  MIO_CHECK(glu == (w8_gate != nullptr) && glu == (s_gate != nullptr), fn + ": w8_gate and s_gate are required together iff act == SWIGLU");
  MIO_CHECK(glu || b_gate == nullptr, fn + ": b_gate belongs to act == SWIGLU");
  MIO_CHECK(s_up != nullptr, fn + ": s_up (the fp32 scales [E, I]) must be non-null");
  MIO_CHECK(w8_up && (T == 0 || (x && h && expert_offsets && sorted_rows)), fn + ": x, w8_up, h, expert_offsets, sorted_rows must be non-null");
  MIO_CHECK(mio_aligned16(x) && mio_aligned16(w8_up) && mio_aligned16(w8_gate) && mio_aligned16(b_up) && mio_aligned16(b_gate) &&
                mio_aligned16(h) && mio_aligned16(workspace) && moe_w8_aligned4(s_up) && moe_w8_aligned4(s_gate) &&
                moe_w8_aligned4(expert_offsets) && moe_w8_aligned4(sorted_rows),
            fn + ": pointers must be 16-byte aligned (the scales and the route's arrays: 4-byte)");
  const MoePlan pl = moe_plan(W8, T, top_k, E, I, d, act);
  if (T == 0 || I == 0) return 0;
  MIO_CHECK(pl.nsplit == 1 || workspace != nullptr, fn + ": workspace required (mio_moe_up_w8_workspace_bytes) when the plan splits K");
  MoeW8Dev p;
  p.x = x; p.w = w8_up; p.wg = w8_gate; p.scale = s_up; p.scale_g = s_gate; p.bias = b_up; p.bias_g = b_gate; p.y = h;
  p.ws = pl.nsplit > 1 ? (float*)workspace : nullptr;
  p.offsets = expert_offsets; p.sorted_rows = sorted_rows;
  p.ldx = ldx; p.ldw = ldw; p.estride = expert_stride; p.ldy = ldh;
  p.T = T; p.topk = top_k; p.E = E; p.rows = pl.rows; p.N = I; p.K = d; p.act = act; p.nsplit = pl.nsplit; p.steps = pl.steps;
  const MoeW8Kernels& k = MOE_W8_TABLE[dtype == MIO_BF16 ? 0 : 1][glu ? 0 : 1];
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k.main[pl.mf - 1], dim3((unsigned)pl.tiles_n, (unsigned)pl.nsplit, (unsigned)E), dim3(256), 0, st, p);
  if (pl.nsplit > 1) {
    const int64_t threads = (int64_t)pl.rows * ((I + 3) / 4);
    hipLaunchKernelGGL(k.reduce, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, p);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mio_fail(fn + " launch: " + hipGetErrorString(e));
  return 0;
}

extern "C" int mio_moe_down_w8(const void* h, const void* w8_down, const float* s_down, const void* b_down, const int32_t* ids,
                               const float* weights, const int32_t* expert_offsets, const int32_t* row_pos, const void* residual,
                               void* y, void* workspace, int32_t T, int32_t top_k, int32_t E, int32_t d, int32_t I, int64_t ldh,
                               int64_t ldw, int64_t expert_stride, int64_t ldy, int64_t ldr, int32_t dtype, void* stream) {
  const std::string fn = "mio_moe_down_w8";
  if (int rc = moe_w8_gemm_checks(fn, T, top_k, E, d, I, MIO_ACT_NONE, dtype, ldh, ldw, expert_stride, ldy)) return rc;
  MIO_CHECK(!residual || (ldr % 8 == 0 && ldr >= d), fn + ": ldr must be a multiple of 8 elements and at least d");
  MIO_CHECK(s_down != nullptr, fn + ": s_down (the fp32 scales [E, d]) must be non-null");
  MIO_CHECK(w8_down && (T == 0 || (h && y && ids && weights && expert_offsets && row_pos)),
            fn + ": h, w8_down, y, ids, weights, expert_offsets, row_pos must be non-null");
  MIO_CHECK(mio_aligned16(h) && mio_aligned16(w8_down) && mio_aligned16(b_down) && mio_aligned16(residual) && mio_aligned16(y) &&
                mio_aligned16(workspace) && moe_w8_aligned4(s_down) && moe_w8_aligned4(ids) && moe_w8_aligned4(weights) &&
                moe_w8_aligned4(expert_offsets) && moe_w8_aligned4(row_pos),
            fn + ": pointers must be 16-byte aligned (the scales and the route's arrays: 4-byte)");
  const MoePlan pl = moe_plan(W8, T, top_k, E, d, I, MIO_ACT_NONE);
  if (T == 0 || d == 0) return 0;
  MIO_CHECK(workspace != nullptr, fn + ": workspace required (mio_moe_down_w8_workspace_bytes)");
  MoeW8Dev p;
  p.x = h; p.w = w8_down; p.wg = nullptr; p.scale = s_down; p.scale_g = nullptr; p.bias = nullptr; p.bias_g = nullptr; p.y = nullptr;
  p.ws = (float*)workspace;
  p.offsets = expert_offsets; p.sorted_rows = nullptr;
  p.ldx = ldh; p.ldw = ldw; p.estride = expert_stride; p.ldy = 0;
  p.T = T; p.topk = top_k; p.E = E; p.rows = pl.rows; p.N = d; p.K = I; p.act = MIO_ACT_NONE; p.nsplit = pl.nsplit; p.steps = pl.steps;
  const MoeDownW8Dev f = {(const float*)workspace, s_down, b_down, residual, y, ids, weights, row_pos, ldy, ldr, T, top_k, E, pl.rows, d, pl.nsplit};
  const MoeW8Kernels& k = MOE_W8_TABLE[dtype == MIO_BF16 ? 0 : 1][1];
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k.main[pl.mf - 1], dim3((unsigned)pl.tiles_n, (unsigned)pl.nsplit, (unsigned)E), dim3(256), 0, st, p);
  const int64_t threads = (int64_t)T * ((d + 3) / 4);
  if (dtype == MIO_BF16) hipLaunchKernelGGL(moe_down_w8_finish_kernel<__bf16>, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, f);
  else hipLaunchKernelGGL(moe_down_w8_finish_kernel<_Float16>, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, f);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mio_fail(fn + " launch: " + hipGetErrorString(e));
  return 0;
}

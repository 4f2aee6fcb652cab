// Mixture-of-experts MLP for decode steps (T <= 64 tokens, E <= 256 experts, top_k <= 8) on 16-bit expert weights: the router and
// the grouped GEMM's kernel; the C-ABI entry points mio_moe_route, mio_moe_up, mio_moe_down and their host queries (semantics:
// include/mio_hip.h).  This file owns the router, the K-loop kernel of the 16-bit form and the entry points'
// argument marshalling.  Shared with the FP8 unit (moe_w8.hip) and owned by moe_gemm_common.h: the launch's arguments, the checks,
// the host queries, both launches and up's reduction; by moe_rows_head.inc / moe_rows_gather.inc: an expert's rows description;
// by moe_common.h: down's finishing launch (and the per-token routing, shared with moe_prefill.hip); by moe_plan.h: the plan
// (shape checks, split of K, workspaces).  The K loop is the decode-step GEMM's (gemm_skinny_w16_head.inc,
// gemm_skinny_w16_loop.inc); the slice range, the slice sum and the epilogue arithmetic are gemm_skinny_plan.h's
// skinny_slice_range and gemm_skinny_common.h's skinny_slice_sum and skinny_finish, the ones the decode-step GEMM runs.
//
// Router: ONE workgroup of 16 waves, a wave per token (tokens wave, wave + 16, ...).  A lane holds the logits of experts lane,
// lane + 64, lane + 128, lane + 192 as fp32 (exact for bf16 / fp16) and their order-preserving keys; top_k rounds of a wave max
// over (key, ~index) pick the experts in the stated order, and the softmax sums run in a fixed shape (a lane's four in index
// order, then the xor butterfly), so reruns give the same bits.  Then a counting sort in LDS with integers only: thread e walks
// the <= 512 chosen ids in routed-row order, which yields its count, and -- behind a prefix over the counts -- its rows in
// ascending order by construction.  No atomic of any kind.
//
// Grouped GEMM: the decode-step GEMM's K loop (gemm_skinny_w16_loop.inc: a 16 x 32 weight fragment as the MFMA A operand straight from
// the row-major weight into VGPRs, x rows staged through LDS with the p ^ (r & 15) swizzle, two register sets, one barrier per
// chunk, v_mfma_f32_16x16x32) with the expert as the grid's third dimension.  A workgroup reads offsets[e], offsets[e + 1] and
// returns at once when its expert has no rows: before any weight load and before any barrier, and the same for all its threads.
// The x stage gathers rows through sorted_rows (up: routed row / top_k is the token) or by sorted position (down: h is stored
// that way); rows past the expert's count are zeros that are never read from memory.  The kernel is instantiated for the host's
// bound on an expert's rows, ceil(T / 16) fragments, and a workgroup stages and multiplies only the fragments its expert's
// count reaches.  Split-K as in the decode-step GEMM: fp32 partials by sorted position, a second launch that sums them in slice
// order.  Up finishes in the first kernel when there is one slice; down always goes through the partials, because its second
// launch is where the top_k slots of a token meet: slice sum, bias, routing weight, slot sum in slot order, residual, one
// rounding.  No atomics, counters or barriers between workgroups.
#include "moe_gemm_common.h"

constexpr SkinnyForm FORM = SKINNY_W16;  // this unit's weight form (gemm_skinny_plan.h)

// ---- router ------------------------------------------------------------------------------------------------------------------
struct MoeRouteDev {
  const void* logits;
  int64_t ld;
  int32_t* ids;
  float* weights;
  int32_t* offsets;
  int32_t* sorted_rows;
  int32_t* row_pos;
  int T, E, topk, renorm;
};

constexpr int MOE_RT_NT = 1024, MOE_RT_NW = MOE_RT_NT / 64;
static_assert(MOE_E_MAX <= 4 * 64 && MOE_E_MAX <= MOE_RT_NT, "four logits per lane; one sorting thread per expert");

template <typename L>
__global__ __launch_bounds__(MOE_RT_NT) void moe_route_kernel(const MoeRouteDev a) {
  __shared__ int32_t s_ids[MOE_T_MAX * MOE_TOPK_MAX];
  __shared__ int32_t s_cnt[MOE_E_MAX];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  for (int t = wave; t < a.T; t += MOE_RT_NW) {  // (wave-uniform)
    const L* row = (const L*)a.logits + (int64_t)t * a.ld;
    int my_id;  // lane j < top_k: slot j
    float my_w;
    moe_route_token(row, a.E, a.topk, a.renorm, lane, my_id, my_w);
    if (lane < a.topk) {
      const int r = t * a.topk + lane;
      a.ids[r] = my_id;
      a.weights[r] = my_w;
      s_ids[r] = my_id;
    }
  }
  __syncthreads();

  // counting sort: thread e owns expert e
  const int rows = a.T * a.topk;
  int cnt = 0;
  if (tid < a.E)
    for (int r = 0; r < rows; ++r) cnt += s_ids[r] == tid;
  if (tid < MOE_E_MAX) s_cnt[tid] = cnt;
  __syncthreads();
  if (tid < a.E) {
    int off = 0;
    for (int e = 0; e < tid; ++e) off += s_cnt[e];
    a.offsets[tid] = off;
    if (tid == a.E - 1) a.offsets[a.E] = off + cnt;
    for (int r = 0; r < rows; ++r)
      if (s_ids[r] == tid) {
        a.sorted_rows[off] = r;
        a.row_pos[r] = off;
        ++off;
      }
  }
}

// ---- grouped GEMM -------------------------------------------------------------------------------------------------------------
// The K loop is gemm_skinny_w16_head.inc + gemm_skinny_w16_loop.inc, the decode-step GEMM's, under an expert's rows description
// (moe_rows_head.inc, moe_rows_gather.inc).
template <typename T, int MF, bool GLU>
__global__ __launch_bounds__(256) void moe_gemm_kernel(const MoeDev<MOE_SCALES_NONE> p) {
#include "moe_rows_head.inc"
#include "gemm_skinny_w16_head.inc"
#include "moe_rows_gather.inc"
#include "gemm_skinny_w16_loop.inc"

  if (!active) return;
  const int n = n0 + 4 * q;
  if (n >= p.N) return;
  // lane (c, q): rows 16 mf + c of the expert, i.e. sorted positions r0 + 16 mf + c, columns n .. n + 3.  This is skinny_write
  // (gemm_skinny_common.h) at (r0, cnt), written out: through the call these kernels compile to other instructions, not these.
  const SkinnyFinish sd = moe_finish_args<false>(p, e);
#pragma unroll
  for (int mf = 0; mf < MF; ++mf) {
    const int m = mf * 16 + c;
    if (m >= cnt) continue;
    const int pos = r0 + m;
    if (p.ws == nullptr) {
      const float v[4] = {acc[mf][0], acc[mf][1], acc[mf][2], acc[mf][3]};
      float g[4] = {0.f, 0.f, 0.f, 0.f};
      if constexpr (GLU) {
#pragma unroll
        for (int i = 0; i < 4; ++i) g[i] = accg[mf][i];
      }
      skinny_finish<T, GLU, false>(sd, pos, n, v, g);
    } else {
      const int64_t plane = (int64_t)p.rows * p.N;
      float* dst = p.ws + (int64_t)s * plane + (int64_t)pos * p.N + n;
      if ((p.N & 3) == 0) {  // (n + 3 < N then, and the partial rows are 16-byte aligned)
        *(f32x4_t*)dst = acc[mf];
        if constexpr (GLU) *(f32x4_t*)(dst + (int64_t)p.nsplit * plane) = accg[mf];
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (n + i < p.N) {
            dst[i] = acc[mf][i];
            if constexpr (GLU) dst[(int64_t)p.nsplit * plane + i] = accg[mf][i];
          }
      }
    }
  }
}

static const MoeKernelTable<MOE_SCALES_NONE> KERNELS = MOE_KERNEL_TABLE(moe_gemm_kernel, 0, MOE_SCALES_NONE);

// ---- the C ABI -----------------------------------------------------------------------------------------------------------------
extern "C" int mio_moe_route(const void* logits, int64_t ld, int32_t* ids, float* weights, int32_t* expert_offsets,
                             int32_t* sorted_rows, int32_t* row_pos, int32_t T, int32_t E, int32_t top_k, int32_t renormalize,
                             int32_t dtype, void* stream) {
  const std::string fn = "mio_moe_route";
  std::string err;
  if (!moe_route_shape_ok(fn.c_str(), T, top_k, E, err)) return mio_fail(err);
  MIO_CHECK(dtype == MIO_BF16 || dtype == MIO_FP16 || dtype == MIO_FP32, fn + ": dtype must be bf16, fp16 or fp32");
  MIO_CHECK(ld >= E, fn + ": ld < E");
  if (T == 0) return 0;
  MIO_CHECK(logits && ids && weights && expert_offsets && sorted_rows && row_pos, fn + ": null logits or output");
  MIO_CHECK(mio_aligned16(logits), fn + ": logits must be 16-byte aligned");
  MIO_CHECK(moe_aligned4(ids) && moe_aligned4(weights) && moe_aligned4(expert_offsets) && moe_aligned4(sorted_rows) &&
                moe_aligned4(row_pos),
            fn + ": outputs must be aligned to their element size");
  const MoeRouteDev a = {logits, ld, ids, weights, expert_offsets, sorted_rows, row_pos, T, E, top_k, renormalize ? 1 : 0};
  hipStream_t st = (hipStream_t)stream;
  if (dtype == MIO_BF16) hipLaunchKernelGGL(moe_route_kernel<__bf16>, dim3(1), dim3(MOE_RT_NT), 0, st, a);
  else if (dtype == MIO_FP16) hipLaunchKernelGGL(moe_route_kernel<_Float16>, dim3(1), dim3(MOE_RT_NT), 0, st, a);
  else hipLaunchKernelGGL(moe_route_kernel<float>, dim3(1), dim3(MOE_RT_NT), 0, st, a);
  return moe_launched(fn);
}

// the grouped GEMMs: argument marshalling over moe_gemm_common.h's host side
extern "C" int mio_moe_up_splits(int32_t T, int32_t top_k, int32_t E, int32_t N, int32_t K, int32_t act) {
  return moe_query_splits(FORM, "mio_moe_up_splits", T, top_k, E, N, K, act);
}

extern "C" size_t mio_moe_up_workspace_bytes(int32_t T, int32_t top_k, int32_t E, int32_t N, int32_t K, int32_t act) {
  return moe_query_workspace_bytes(FORM, "mio_moe_up_workspace_bytes", false, T, top_k, E, N, K, act);
}

extern "C" int mio_moe_down_splits(int32_t T, int32_t top_k, int32_t E, int32_t N, int32_t K) {
  return moe_query_splits(FORM, "mio_moe_down_splits", T, top_k, E, N, K, MIO_ACT_NONE);
}

extern "C" size_t mio_moe_down_workspace_bytes(int32_t T, int32_t top_k, int32_t E, int32_t N, int32_t K) {
  return moe_query_workspace_bytes(FORM, "mio_moe_down_workspace_bytes", true, T, top_k, E, N, K, MIO_ACT_NONE);
}

extern "C" int mio_moe_up(const void* x, const void* w_up, const void* b_up, const void* w_gate, const void* b_gate,
                          const int32_t* expert_offsets, const int32_t* sorted_rows, void* h, void* workspace, int32_t T,
                          int32_t top_k, int32_t E, int32_t I, int32_t d, int64_t ldx, int64_t ldw, int64_t expert_stride,
                          int64_t ldh, int32_t act, int32_t dtype, void* stream) {
  return moe_run_up(FORM, KERNELS, "mio_moe_up", x, w_up, nullptr, b_up, w_gate, nullptr, b_gate, expert_offsets, sorted_rows, h,
                    workspace, T, top_k, E, I, d, ldx, ldw, expert_stride, ldh, act, dtype, stream);
}

extern "C" int mio_moe_down(const void* h, const void* w_down, const void* b_down, const int32_t* ids, const float* weights,
                            const int32_t* expert_offsets, const int32_t* row_pos, const void* residual, void* y, void* workspace,
                            int32_t T, int32_t top_k, int32_t E, int32_t d, int32_t I, int64_t ldh, int64_t ldw,
                            int64_t expert_stride, int64_t ldy, int64_t ldr, int32_t dtype, void* stream) {
  return moe_run_down(FORM, KERNELS, "mio_moe_down", h, w_down, nullptr, b_down, ids, weights, expert_offsets, row_pos, residual, y,
                      workspace, T, top_k, E, d, I, ldh, ldw, expert_stride, ldy, ldr, dtype, stream);
}

// One translation unit per dtype: compiled with -DGEMM_TYPE_ID={0,1}.
// The product library reads no environment variable; A/B switches and stamp instantiations: -DMIO_DIAG (make dbg).
#include <cstdlib>
#include <mutex>
#include <string>

#include "gemm8w_kernel.h"

#if GEMM_TYPE_ID == 0
using GT = __bf16;
#else
using GT = _Float16;
#endif

template <int BM, int BN, int WM, int WN, int ACT>
static int launch_cfg(GemmDev p, hipStream_t stream) {
  constexpr bool GATE = (ACT == MIO_ACT_SWIGLU);
  constexpr size_t smem = 2 * (size_t)(BM * GEMM_BK * 2 + BN * GEMM_BK * 2 * (GATE ? 2 : 1));
  p.tiles_m = (int)((p.M + BM - 1) / BM);
  p.tiles_n = (p.N + BN - 1) / BN;
  auto kern = gemm_bias_act_kernel<GT, BM, BN, WM, WN, ACT>;
  static std::once_flag once;  // > 64 KiB dynamic LDS needs the opt-in once per kernel
  static hipError_t ea = hipSuccess;
  std::call_once(once, [&] { ea = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem); });
  if (ea != hipSuccess) return mio_fail(std::string("gemm: hipFuncSetAttribute: ") + hipGetErrorString(ea));
  hipLaunchKernelGGL(kern, dim3(p.tiles_m * p.tiles_n), dim3(WM * WN * 64), smem, stream, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mio_fail(std::string("gemm launch: ") + hipGetErrorString(e));
  return 0;
}

// eight-wave ping-pong kernel (gemm8w_kernel.h), persistent; `one_tile`: one workgroup per tile instead (A/B only)
template <int ACT, bool RES, int VAR = 0, int FOLD = 0>
static int launch_8w(GemmDev p, hipStream_t stream, bool one_tile = false) {
  constexpr int BN = (ACT == MIO_ACT_SWIGLU) ? 128 : 256;
  constexpr int G8_SMEM = FOLD ? G8_SMEM_FOLD : ::G8_SMEM;  // (shadows the namespace-scope constant for this launcher)
  p.tiles_m = (int)((p.M + 255) / 256);
  p.tiles_n = (p.N + BN - 1) / BN;
  auto kern = gemm8w_kernel<GT, ACT, RES, VAR, FOLD>;
  static std::once_flag once;
  static hipError_t ea = hipSuccess;
  static int ncu = 256;
  std::call_once(once, [&] {
    ea = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, G8_SMEM);
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0)
      ncu = n & ~7;  // whole XCD groups, so tile % 8 keeps naming the XCD
  });
  if (ea != hipSuccess) return mio_fail(std::string("gemm8w: hipFuncSetAttribute: ") + hipGetErrorString(ea));
  const int tiles = p.tiles_m * p.tiles_n;
  int wgs = ncu;
#ifdef MIO_DIAG  // mio_dbg_set(7, n): a workgroup budget below the CU count, for co-running with another stream's kernel
  if (mio_dbg_get(7) >= 8 && mio_dbg_get(7) < ncu) wgs = mio_dbg_get(7) & ~7;  // (tools/overlap_probe.py)
#endif
  hipLaunchKernelGGL(kern, dim3((one_tile || tiles < wgs) ? tiles : wgs), dim3(G8_THREADS), G8_SMEM, stream, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mio_fail(std::string("gemm8w launch: ") + hipGetErrorString(e));
  return 0;
}
template <int ACT, int VAR = 0>
static int launch_8w_res(const GemmDev& p, hipStream_t stream, bool one_tile = false) {
  if constexpr (ACT != MIO_ACT_SWIGLU && VAR == 0) {
    if (p.res != nullptr) return launch_8w<ACT, true>(p, stream, one_tile);
  }
  return launch_8w<ACT, false, VAR>(p, stream, one_tile);
}

// `route`: the kernel gemm_plan (gemm_api.hip) chose with gemm_pick_route, the same answer mio_gemm_route reports.  The
// diagnostic build's overrides (mio_gemm_impl: MIO_GEMM_IMPL, mio_dbg_set(4, .)) replace it here by a variant of that route.
template <int ACT>
static int launch_act(const GemmDev& p, int route, hipStream_t stream) {
  if constexpr (ACT == MIO_ACT_SWIGLU) {
    switch (route) {
      case MIO_GEMM_ROUTE_P8W_GLU_FOLD: return launch_8w<ACT, false, 0, 1>(p, stream);  // LayerNorm applied in the read-out
      case MIO_GEMM_ROUTE_P8W_GLU: return launch_8w<ACT, false>(p, stream);
      case MIO_GEMM_ROUTE_GLU_T256X128: return launch_cfg<256, 128, 2, 4, ACT>(p, stream);
      case MIO_GEMM_ROUTE_GLU_T128X64: return launch_cfg<128, 64, 2, 2, ACT>(p, stream);
    }
  } else {
#ifdef MIO_DIAG
    // A/B: the generic 256x256 kernel in place of the persistent one
    if (mio_gemm_impl() == 1 && route != MIO_GEMM_ROUTE_T128) return launch_cfg<256, 256, 2, 4, ACT>(p, stream);
#endif
    switch (route) {
      case MIO_GEMM_ROUTE_T128: return launch_cfg<128, 128, 2, 2, ACT>(p, stream);
      case MIO_GEMM_ROUTE_T256: return launch_cfg<256, 256, 2, 4, ACT>(p, stream);
      case MIO_GEMM_ROUTE_P8W_FOLD:
        if constexpr (ACT == MIO_ACT_NONE || ACT == MIO_ACT_GELU_TANH) return launch_8w<ACT, false, 0, 1>(p, stream);
        break;
      case MIO_GEMM_ROUTE_P8W_STATS:
        if constexpr (ACT == MIO_ACT_NONE) return launch_8w<ACT, true, 0, 2>(p, stream);
        break;
      case MIO_GEMM_ROUTE_P8W:
      case MIO_GEMM_ROUTE_P8W_RES:
#ifdef MIO_DIAG
        if constexpr (ACT == MIO_ACT_NONE) {
          if (mio_gemm_impl() == 8 && p.dbg != nullptr) return launch_8w<ACT, false, 128>(p, stream);  // stamps
          if (mio_gemm_impl() == 24) return launch_8w_res<ACT, 2048>(p, stream);
          if (mio_gemm_impl() == 10) return launch_8w_res<ACT, 4>(p, stream);
          if (mio_gemm_impl() == 13) return launch_8w_res<ACT, 16>(p, stream);
          if (mio_gemm_impl() == 16) return launch_8w_res<ACT, 64>(p, stream);
        }
        if constexpr (ACT == MIO_ACT_GELU_TANH) {
          if (mio_gemm_impl() == 20) return launch_8w<ACT, false, 256>(p, stream);  // scalar activation math
        }
        if (mio_gemm_impl() == 9) return launch_8w_res<ACT>(p, stream, true);  // one workgroup per tile
#endif
        return launch_8w_res<ACT>(p, stream);
    }
  }
  return mio_fail("gemm: no kernel for route " + std::to_string(route));
}

template <>
int gemm_launch<GT>(GemmDev p, int act, int route, hipStream_t stream) {
#ifdef MIO_DIAG
  static const char* dbg_ptr = std::getenv("MIO_GEMM_DBG_PTR");
  if (dbg_ptr != nullptr) p.dbg = (unsigned long long*)std::strtoull(dbg_ptr, nullptr, 0);
  static const char* gm = std::getenv("MIO_GEMM_GROUP_M");  // tile-order sweep (tools/dbg)
  if (gm != nullptr) p.group_m = std::atoi(gm);
  if (mio_dbg_get(5) > 0) p.group_m = mio_dbg_get(5);
#endif
  switch (act) {
    case MIO_ACT_NONE: return launch_act<MIO_ACT_NONE>(p, route, stream);
    case MIO_ACT_GELU_TANH: return launch_act<MIO_ACT_GELU_TANH>(p, route, stream);
    case MIO_ACT_GELU_ERF: return launch_act<MIO_ACT_GELU_ERF>(p, route, stream);
    case MIO_ACT_RELU: return launch_act<MIO_ACT_RELU>(p, route, stream);
    case MIO_ACT_SILU: return launch_act<MIO_ACT_SILU>(p, route, stream);
    case MIO_ACT_SWIGLU: return launch_act<MIO_ACT_SWIGLU>(p, route, stream);
  }
  return mio_fail("gemm: unknown activation");
}

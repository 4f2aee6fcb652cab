// The dense attention forward (mio_fa3_fwd): one translation unit per (dtype, padded head dim), see fa3_inst.h.
// The product library reads no environment variable and keeps no unsynchronised mutable state; the A/B switches and the
// in-kernel stamp instantiations exist only in the diagnostic build (make dbg: -DMIO_DIAG -> libmio_hip_dbg.so).
#include <cstdlib>

#include "fa3_inst.h"
#include "fa3_route.h"

template <bool CAUSAL, int MASK>
static int launch_one(const FaDev& p, hipStream_t stream) {
  return fa_launch<fa3_fwd_kernel<FaT, FA_D, CAUSAL, MASK>>("fa3_fwd", p.nqblk * p.B * p.H, 256, FaSmem<FA_D>::TOTAL,
                                                            stream, p);
}

// third structure (software-pipelined across KV tiles): no user mask
template <bool CAUSAL, bool KPRE = false>
static int launch_three(FaDev p, hipStream_t stream) {
  const int grid = (int)fa_grid<CAUSAL>(p, p.Sq, FA3_BM);
  const size_t smem = FA3_STAGES * FaSmem<FA_D>::STAGE;
#ifdef MIO_DIAG
#if FA_D == 64 && FA_TYPE_ID == 0
  if constexpr (CAUSAL && !KPRE) {  // timing-only ablations (tools/fa_ablate.py): mio_dbg_set(0, bits)
    const char* abl = "fa3_fwd3 (ablation)";
    switch (mio_dbg_get(0)) {
      case 1: return fa_launch<fa3_fwd3_kernel<FaT, FA_D, CAUSAL, false, 1>>(abl, grid, 256, smem, stream, p);
      case 2: return fa_launch<fa3_fwd3_kernel<FaT, FA_D, CAUSAL, false, 2>>(abl, grid, 256, smem, stream, p);
      case 3: return fa_launch<fa3_fwd3_kernel<FaT, FA_D, CAUSAL, false, 3>>(abl, grid, 256, smem, stream, p);
      case 4: return fa_launch<fa3_fwd3_kernel<FaT, FA_D, CAUSAL, false, 4>>(abl, grid, 256, smem, stream, p);
      case 8: return fa_launch<fa3_fwd3_kernel<FaT, FA_D, CAUSAL, false, 8>>(abl, grid, 256, smem, stream, p);
      case 16: return fa_launch<fa3_fwd3_kernel<FaT, FA_D, CAUSAL, false, 16>>(abl, grid, 256, smem, stream, p);
      case 32: return fa_launch<fa3_fwd3_kernel<FaT, FA_D, CAUSAL, false, 32>>(abl, grid, 256, smem, stream, p);
      case 48: return fa_launch<fa3_fwd3_kernel<FaT, FA_D, CAUSAL, false, 48>>(abl, grid, 256, smem, stream, p);
      case 57: return fa_launch<fa3_fwd3_kernel<FaT, FA_D, CAUSAL, false, 57>>(abl, grid, 256, smem, stream, p);
      case 59: return fa_launch<fa3_fwd3_kernel<FaT, FA_D, CAUSAL, false, 59>>(abl, grid, 256, smem, stream, p);
      case 63: return fa_launch<fa3_fwd3_kernel<FaT, FA_D, CAUSAL, false, 63>>(abl, grid, 256, smem, stream, p);
      default: break;
    }
  }
#endif
  static const char* dbg_ptr = std::getenv("MIO_FA_DBG_PTR");  // in-kernel phase stamps (tools/fa_stamps.py)
  if (dbg_ptr != nullptr && !KPRE) {
    p.mask = (const void*)std::strtoull(dbg_ptr, nullptr, 0);
    return fa_launch<fa3_fwd3_kernel<FaT, FA_D, CAUSAL, true>>("fa3_fwd3 (stamps)", grid, 256, smem, stream, p);
  }
#endif
  return fa_launch<fa3_fwd3_kernel<FaT, FA_D, CAUSAL, false, 0, KPRE>>("fa3_fwd3", grid, 256, smem, stream, p);
}

// fifth structure (two waves per SIMD on 16x16x32 MFMA tiles): head dim <= 64, no user mask
#if FA_D == 64
template <bool CAUSAL, bool CARRY = false, bool OBLK = false, bool KPRE = true>
static int launch_five(FaDev p, hipStream_t stream) {
  const int grid = (int)fa_grid<CAUSAL>(p, p.Sq, FA5_BM);
#if defined(MIO_DIAG) && FA_TYPE_ID == 0
  if constexpr (!CARRY && !OBLK && KPRE) {
  p.xcd_remap |= (mio_dbg_get(3) & 7) << 4;  // wave-priority probe (tools/fa5_ablate.py)
  static const char* dbg_ptr = std::getenv("MIO_FA_DBG_PTR");  // in-kernel phase stamps (tools/fa5_stamps.py)
  if (dbg_ptr != nullptr) {
    p.mask = (const void*)std::strtoull(dbg_ptr, nullptr, 0);
    return fa_launch<fa3_fwd5_kernel<FaT, CAUSAL, true>>("fa3_fwd5 (stamps)", grid, 512, FA5_SMEM, stream, p);
  }
  if constexpr (CAUSAL) {  // timing-only ablations (tools/fa5_ablate.py): mio_dbg_set(0, bits)
    const char* abl = "fa3_fwd5 (ablation)";
    switch (mio_dbg_get(0)) {
      case 1: return fa_launch<fa3_fwd5_kernel<FaT, CAUSAL, false, 1>>(abl, grid, 512, FA5_SMEM, stream, p);
      case 2: return fa_launch<fa3_fwd5_kernel<FaT, CAUSAL, false, 2>>(abl, grid, 512, FA5_SMEM, stream, p);
      case 4: return fa_launch<fa3_fwd5_kernel<FaT, CAUSAL, false, 4>>(abl, grid, 512, FA5_SMEM, stream, p);
      case 8: return fa_launch<fa3_fwd5_kernel<FaT, CAUSAL, false, 8>>(abl, grid, 512, FA5_SMEM, stream, p);
      case 15: return fa_launch<fa3_fwd5_kernel<FaT, CAUSAL, false, 15>>(abl, grid, 512, FA5_SMEM, stream, p);
      default: break;
    }
  }
  }
#endif
  return fa_launch<fa3_fwd5_kernel<FaT, CAUSAL, false, 0, CARRY, OBLK, KPRE>>("fa3_fwd5", grid, 512, FA5_SMEM, stream, p);
}
#endif

#ifdef MIO_DIAG
// A/B overrides of the diagnostic build on top of the route (plain-K launches without a user mask): MIO_FA_IMPL=1 forces
// the sequential kernel, MIO_FA_IMPL=3 or mio_dbg_set(1, 3) fwd3 where the route takes fwd5 (mio_dbg_set(1, 3) also for
// pre-scaled K).  Returns 1 with *rc set when it took the launch.
static int diag_launch(int route, const FaDev& p, int causal, hipStream_t stream, int* rc) {
  static const int impl = [] {
    const char* e = std::getenv("MIO_FA_IMPL");
    return e ? std::atoi(e) : 0;
  }();
  if ((route == MIO_FA3_ROUTE_FWD5 || route == MIO_FA3_ROUTE_FWD3) && impl == 1) {
    *rc = causal ? launch_one<true, 0>(p, stream) : launch_one<false, 0>(p, stream);
    return 1;
  }
#if FA_D == 64
  if (route == MIO_FA3_ROUTE_FWD5 && (impl == 3 || mio_dbg_get(1) == 3)) {
    *rc = causal ? launch_three<true>(p, stream) : launch_three<false>(p, stream);
    return 1;
  }
  if ((route == MIO_FA3_ROUTE_FWD5_KPRE || route == MIO_FA3_ROUTE_FWD5_KPRE_OBLK) && mio_dbg_get(1) == 3) {
    *rc = causal ? launch_three<true, true>(p, stream) : launch_three<false, true>(p, stream);
    return 1;
  }
#endif
  return 0;
}
#endif

template <>
int fa3_launch<FaT, FA_D>(const FaDev& p, int causal, int route, hipStream_t stream) {
  // The route is fa3_pick_route's (fa3_route.h), the rule mio_fa3_route reports.  Measured on MI355X, B8 S4096, random data:
  //   no user mask, Sq > 128: the software-pipelined kernels --
  //     D64 causal 0.359 ms (766 TFLOP/s) vs 0.442 two-waves-per-SIMD / 0.52 sequential one-wave; non-causal 0.626 vs 0.79;
  //     D128 causal 0.284 ms (967 TFLOP/s) vs 0.361 sequential one-wave; D80 non-causal 0.828 ms (830) vs 1.158;
  //   head dim <= 64, plain output: fa3_fwd5 (16x16x32 MFMA tiles).  Same box, interleaved, B8 S4096 H16 bf16, k_prescaled:
  //     causal 0.3047 ms vs 0.3305 fa3_fwd4 KPRE / 0.3401 fa3_fwd3 KPRE / 0.3570 fa3_fwd3; non-causal 0.5494 vs 0.6162 /
  //     0.5862 / 0.6273; with plain K the same structure applies the scale in fp32 on the way into exp2;
  //   k_prescaled at head dim 65 .. 96: fa3_fwd3's KPRE form (not at 128: the two reference tuples (32 VGPRs) do not fit
  //     beside the score / P / fragment registers there -- hipcc parks values in accumulator registers the kernel owns,
  //     tools/check_agpr.py catches it);
  //   user masks, Sq <= 128, Sk == 0 and K / V spans of 4 GiB or more: the sequential one-wave kernel.
#ifdef MIO_DIAG
  {
    int rc = 0;
    if (diag_launch(route, p, causal, stream, &rc)) return rc;
  }
#endif
  switch (route) {
#if FA_D == 64
    case MIO_FA3_ROUTE_FWD5:
      return causal ? launch_five<true, false, false, false>(p, stream) : launch_five<false, false, false, false>(p, stream);
    case MIO_FA3_ROUTE_FWD5_KPRE:
      return causal ? launch_five<true>(p, stream) : launch_five<false>(p, stream);
    case MIO_FA3_ROUTE_FWD5_KPRE_CARRY:
      return causal ? launch_five<true, true>(p, stream) : launch_five<false, true>(p, stream);
    case MIO_FA3_ROUTE_FWD5_KPRE_OBLK:
      return causal ? launch_five<true, false, true>(p, stream) : launch_five<false, false, true>(p, stream);
#endif
#if FA_D < 128
    case MIO_FA3_ROUTE_FWD3_KPRE:
      return causal ? launch_three<true, true>(p, stream) : launch_three<false, true>(p, stream);
#endif
    case MIO_FA3_ROUTE_FWD3:
      return causal ? launch_three<true>(p, stream) : launch_three<false>(p, stream);
    case MIO_FA3_ROUTE_FWD1:
      return causal ? launch_one<true, 0>(p, stream) : launch_one<false, 0>(p, stream);
    case MIO_FA3_ROUTE_FWD1_KEEP:
      return causal ? launch_one<true, 1>(p, stream) : launch_one<false, 1>(p, stream);
    case MIO_FA3_ROUTE_FWD1_ADD:
      return causal ? launch_one<true, 2>(p, stream) : launch_one<false, 2>(p, stream);
    default:
      return mio_fail("fa3_fwd: k_prescaled launch outside the kernels that support it");
  }
}

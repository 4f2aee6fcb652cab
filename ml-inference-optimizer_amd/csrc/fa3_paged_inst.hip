// Attention forward over the paged KV cache (mio_fa3_fwd_paged): one translation unit per (dtype, padded head dim),
// compiled with -DFA_TYPE_ID={0,1} -DFA_D={64,96,128} like fa3_varlen_inst.hip.  Padded head dim 64:
// fa3_fwd5_paged_kernel; 96 / 128: fa3_fwd3_paged_kernel.  Plain K, plain output.
#include <mutex>

#include "fa3_paged.h"

#if FA_TYPE_ID == 0
using FaT = __bf16;
#else
using FaT = _Float16;
#endif

template <bool CAUSAL>
static int launch(FaDev p, const FaPaged& pg, hipStream_t stream) {
#if FA_D == 64
  constexpr int BM = FA5_BM, NT = 512;
  constexpr size_t smem = FA5_SMEM;
  auto kern = fa3_fwd5_paged_kernel<FaT, CAUSAL>;
#else
  constexpr int BM = FA3_BM, NT = 256;
  constexpr size_t smem = FA3_STAGES * FaSmem<FA_D>::STAGE;
  auto kern = fa3_fwd3_paged_kernel<FaT, FA_D, CAUSAL>;
#endif
  // the grid of a dense [B, max_seqlen_q] launch; workgroups past their own sequence's blocks leave at once
  p.nqblk = (pg.max_q + BM - 1) / BM;
  p.qgrid = CAUSAL ? (p.nqblk + 1) / 2 : p.nqblk;
  const int64_t grid = (int64_t)p.qgrid * p.B * p.H;
  if (grid > 0x7fffffff) return mio_fail("fa3_fwd_paged: grid too large");
  static std::once_flag once;
  static hipError_t ea = hipSuccess;
  std::call_once(once, [&] { ea = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem); });
  if (ea != hipSuccess) return mio_fail(std::string("fa3_fwd_paged: hipFuncSetAttribute: ") + hipGetErrorString(ea));
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(NT), smem, stream, p, pg);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mio_fail(std::string("fa3_fwd_paged launch: ") + hipGetErrorString(e));
  return 0;
}

template <>
int fa3_paged_launch<FaT, FA_D>(const FaDev& p, const FaPaged& pg, int causal, hipStream_t stream) {
  return causal ? launch<true>(p, pg, stream) : launch<false>(p, pg, stream);
}

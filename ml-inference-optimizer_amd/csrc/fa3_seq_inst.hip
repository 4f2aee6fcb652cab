// The per-sequence attention forwards: packed variable-length (mio_fa3_fwd_varlen, fa3_varlen.h) and over the paged KV
// cache (mio_fa3_fwd_paged, fa3_paged.h).  One translation unit per (dtype, padded head dim), see fa3_inst.h.  Padded
// head dim 64: the fwd5 form of the sequence's kernel (route fwd5's kernel); 96 / 128: the fwd3 form (route fwd3's).
// Plain K, plain output.
#include <type_traits>

#include "fa3_inst.h"
#include "fa3_paged.h"

// the kernel for the sequence description V (FaVarlen / FaPaged)
template <typename V, bool CAUSAL>
constexpr auto seq_kernel() {
  constexpr bool VARLEN = std::is_same_v<V, FaVarlen>;
#if FA_D == 64
  if constexpr (VARLEN) return fa3_fwd5_varlen_kernel<FaT, CAUSAL>;
  else return fa3_fwd5_paged_kernel<FaT, CAUSAL>;
#else
  if constexpr (VARLEN) return fa3_fwd3_varlen_kernel<FaT, FA_D, CAUSAL>;
  else return fa3_fwd3_paged_kernel<FaT, FA_D, CAUSAL>;
#endif
}

template <typename V, bool CAUSAL>
static int launch(FaDev p, const V& s, hipStream_t stream) {
  const char* family = std::is_same_v<V, FaVarlen> ? "fa3_fwd_varlen" : "fa3_fwd_paged";
  return fa_grid_launch<seq_kernel<V, CAUSAL>(), CAUSAL>(family, p, s.max_q, stream, p, s);
}

template <>
int fa3_seq_launch<FaT, FA_D>(const FaDev& p, const FaVarlen& s, int causal, hipStream_t stream) {
  return causal ? launch<FaVarlen, true>(p, s, stream) : launch<FaVarlen, false>(p, s, stream);
}

template <>
int fa3_seq_launch<FaT, FA_D>(const FaDev& p, const FaPaged& s, int causal, hipStream_t stream) {
  return causal ? launch<FaPaged, true>(p, s, stream) : launch<FaPaged, false>(p, s, stream);
}

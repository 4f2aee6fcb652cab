// The OCP e4m3fn (torch.float8_e4m3fn) conversions of the fp8 KV cache, shared by its decode (decode_kv8.hip), its cache
// writes (cache_write.hip) and its paged prefill (fa3_kv8_inst.hip).  Every e4m3 value is exact in bf16 / fp16 / fp32, so the
// widening conversions run at scale 1 and round nothing; the narrowing one rounds to nearest even after an explicit clamp.
#pragma once
#include <type_traits>

#include "mio_common.h"

// two e4m3fn bytes (the low / high half of w) -> two packed T (exact, scale 1)
template <typename T, bool HI>
__device__ __forceinline__ uint32_t kv8_cvt2(uint32_t w) {
  if constexpr (std::is_same_v<T, __bf16>) return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, HI));
  else return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, HI));
}

// eight e4m3 (two dwords) -> the 8 x 16-bit MFMA operand (exact)
template <typename T>
__device__ __forceinline__ typename DT<T>::x8 kv8_to_x8(u32x2_t w) {
  const u32x4_t r = {kv8_cvt2<T, false>(w[0]), kv8_cvt2<T, true>(w[0]), kv8_cvt2<T, false>(w[1]), kv8_cvt2<T, true>(w[1])};
  return __builtin_bit_cast(typename DT<T>::x8, r);
}

// four e4m3 (one dword) -> fp32 (exact)
__device__ __forceinline__ void kv8_to_f32x4(uint32_t w, float* f) {
  const f32x2_t lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
  const f32x2_t hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
  f[0] = lo[0];
  f[1] = lo[1];
  f[2] = hi[0];
  f[3] = hi[1];
}

// x * inv clamped to the e4m3 range; a NaN passes the comparisons unchanged (the convert is not relied on to saturate)
__device__ __forceinline__ float kv8_clamp(float x) { return x > 448.f ? 448.f : (x < -448.f ? -448.f : x); }

// four clamped fp32 -> four e4m3 bytes (round to nearest even); NaN -> sign | 0x7f as torch's float8_e4m3fn cast
__device__ __forceinline__ uint32_t kv8_pack4(const float* x) {
  typedef __attribute__((ext_vector_type(2))) short s16x2_t;
  s16x2_t v = {0, 0};
  v = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(v, x[0], x[1], 1.0f, false);
  v = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(v, x[2], x[3], 1.0f, true);
  uint32_t w = __builtin_bit_cast(uint32_t, v);
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (__builtin_isnan(x[i])) w = (w & ~(0xffu << (8 * i))) | (((__float_as_uint(x[i]) >> 24) | 0x7fu) & 0xffu) << (8 * i);
  return w;
}

// sixteen 16-bit source elements (two 16-byte loads) -> one 16-byte chunk of e4m3
template <typename T>
__device__ __forceinline__ u32x4_t kv8_quant16(u32x4_t a, u32x4_t b, float inv) {
  const typename DT<T>::x8 va = __builtin_bit_cast(typename DT<T>::x8, a), vb = __builtin_bit_cast(typename DT<T>::x8, b);
  float f[16];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float xa = (float)va[i], xb = (float)vb[i];
    f[i] = __builtin_isnan(xa) ? xa : kv8_clamp(xa * inv);  // a NaN keeps its input's sign
    f[8 + i] = __builtin_isnan(xb) ? xb : kv8_clamp(xb * inv);
  }
  return (u32x4_t){kv8_pack4(f), kv8_pack4(f + 4), kv8_pack4(f + 8), kv8_pack4(f + 12)};
}

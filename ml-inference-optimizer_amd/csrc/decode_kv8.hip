// FP8 paged KV cache (OCP e4m3fn, torch.float8_e4m3fn) for CDNA4 (gfx950): the quantising cache writes and the three
// decode kernels of decode_paged.hip reading one byte per cached element.
//
// Same cache layout, one byte per element: [num_blocks, num_layers, block_size, Hkv, D].  A cached element x8 stands for
// x8 * scale with one fp32 scale per (K or V, layer), read by the kernels from device memory (no host sync: a scale may change
// between replays of a captured graph).  The host passes the address of the scale of layer_idx.
//   write:  q = e4m3(clamp(float(x) * (1 / scale), -448, 448)), round to nearest even; NaN stays NaN (sign | 0x7f)
//   decode: every e4m3 value is exact in bf16 / fp16 / fp32, so K and V enter the products unrounded; k_scale is folded into
//           the score scale, v_scale into the output of each split before its partial state is stored (the split merge,
//           decode_reduce_kernel, is linear in o and is the 16-bit one).  Q and the softmax weights stay 16-bit / fp32.
// The kernels are the 16-bit ones with 16 elements per 16-byte chunk:
//   decode_paged_kv8_kernel  (route head)  one workgroup per (query row, split), a lane owns one 16-element chunk of a head row
//   decode_rows_kv8_kernel   (route rows)  one workgroup per (sequence, split) over whole token rows of Hkv * D bytes
//   decode_gqa_kv8_kernel    (route gqa)   matrix core: K / V by DMA into a 32 * D-byte LDS image per 32-key half; the K
//                                          fragment is one ds_read_b64 + 4 v_cvt_scalef32_pk_{bf16,f16}_fp8, the V^T fragment
//                                          one ds_read_b64_tr_b8 + 4 conversions; the MFMAs stay 16x16x32 bf16 / fp16
// and their *_win_kernel forms take a sliding window as decode_paged.hip's do.
#include <algorithm>
#include <mutex>
#include <type_traits>

#include "mio_common.h"

#include "decode_plan.h"

// ---- e4m3fn conversions ---------------------------------------------------------------------------------------------------
// four e4m3 (one dword) -> fp32 (exact)
__device__ __forceinline__ void kv8_to_f32x4(uint32_t w, float* f) {
  const f32x2_t lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
  const f32x2_t hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
  f[0] = lo[0];
  f[1] = lo[1];
  f[2] = hi[0];
  f[3] = hi[1];
}

// eight e4m3 (two dwords) -> the 8 x 16-bit MFMA operand (exact; scale 1)
template <typename T>
__device__ __forceinline__ typename DT<T>::x8 kv8_to_x8(u32x2_t w) {
  uint32_t r[4];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    if constexpr (std::is_same_v<T, __bf16>) {
      r[2 * i] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w[i], 1.0f, false));
      r[2 * i + 1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w[i], 1.0f, true));
    } else {
      r[2 * i] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w[i], 1.0f, false));
      r[2 * i + 1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w[i], 1.0f, true));
    }
  }
  return __builtin_bit_cast(typename DT<T>::x8, (u32x4_t){r[0], r[1], r[2], r[3]});
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

// ---- route head: one workgroup per (query row, split) ----------------------------------------------------------------------
// decode_paged_body.inc with a lane on 16 one-byte elements: CPRP = 16-byte chunks per head row padded to a power of two
// (4 for D <= 64, 8 for D <= 128), 64 / CPRP tokens per wave-iteration, U wave-iterations per double-buffered batch.
template <typename T, int CPRP, int U, bool WIN>
__device__ __forceinline__ void dec_paged_kv8_body(const DecDev& p, const float* ksc, const float* vsc, int wleft) {
  constexpr int TPI = 64 / CPRP;
  constexpr int NSTATE = 4 * TPI;
  __shared__ float s_o[NSTATE][CPRP * 16 + 1];
  __shared__ float s_m[NSTATE], s_l[NSTATE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t = lane / CPRP, c = lane % CPRP;
  const int row = blockIdx.x;  // (b, h, qi)
  const int split = blockIdx.y;
  const int qi = row % p.q_len;
  const int h = (row / p.q_len) % p.H;
  const int b = row / (p.q_len * p.H);
  const int kvh = h / (p.H / p.Hkv);
  const int ctx = p.cl[b];
  int begin = split * p.split_len;
  if constexpr (WIN) begin += dec_win_begin(ctx, p.q_len, wleft);
  int end = begin + p.split_len;
  if (end > ctx) end = ctx;
  if constexpr (WIN) {
    const int lo = ctx - p.q_len + qi - wleft;  // this row's first visible key
    if (begin < lo) begin = lo;
  }
  const bool c_ok = (16 * c < p.D);

  float qf[16];
  {
    const float qs = p.scale * ksc[0];  // k_scale folded into the score scale
    u32x4_t raw[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    if (c_ok) {
      const T* qp = (const T*)p.q + b * p.qs_b + h * p.qs_h + (int64_t)qi * p.qs_s + 16 * c;
      raw[0] = *(const u32x4_t*)qp;
      raw[1] = *(const u32x4_t*)(qp + 8);
    }
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const typename DT<T>::x8 v = __builtin_bit_cast(typename DT<T>::x8, raw[hh]);
#pragma unroll
      for (int i = 0; i < 8; ++i) qf[8 * hh + i] = (float)v[i] * qs;
    }
  }

  float m = -INFINITY, l = 0.f, o[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) o[i] = 0.f;

  const int64_t tok_stride = (int64_t)p.Hkv * p.D;  // bytes
  const int64_t blk_stride = (int64_t)p.L * p.bs * tok_stride;
  constexpr int STEP = 4 * TPI;
  const int last = end - 1;
  const int coff = c_ok ? 16 * c : 0;
  const int64_t lay_off = (int64_t)p.layer * p.bs * tok_stride + (int64_t)kvh * p.D + coff;
  const int32_t* btrow = p.bt + (int64_t)b * p.max_blocks;
  const uint8_t* kc = (const uint8_t*)p.kc;
  const uint8_t* vc = (const uint8_t*)p.vc;
  auto load_pb = [&](int pos0, int (&pb)[U]) {
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const int pos = min(pos0 + j * STEP + t, last);
      pb[j] = btrow[min(pos / p.bs, p.max_blocks - 1)];
    }
  };
  auto load_kv = [&](int pos0, const int (&pb)[U], u32x4_t (&kr)[U], u32x4_t (&vr)[U]) {
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const int pos = min(pos0 + j * STEP + t, last);
      const int64_t off = (int64_t)pb[j] * blk_stride + lay_off + (int64_t)(pos % p.bs) * tok_stride;
      kr[j] = *(const u32x4_t*)(kc + off);
      vr[j] = *(const u32x4_t*)(vc + off);
    }
  };
  auto reduce = [&](int pos0, const u32x4_t (&kr)[U], const u32x4_t (&vr)[U]) {
    float sc[U];
    float m_new = m;
#pragma unroll
    for (int j = 0; j < U; ++j) {
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        float kf[4];
        kv8_to_f32x4(kr[j][w], kf);
#pragma unroll
        for (int i = 0; i < 4; ++i) s += qf[4 * w + i] * kf[i];  // qf = 0 in the padding chunks (c_ok false)
      }
#pragma unroll
      for (int x = 1; x < CPRP; x <<= 1) s += __shfl_xor(s, x, 64);
      const int pos = pos0 + j * STEP + t;
      sc[j] = (pos < end && pos / p.bs < p.max_blocks) ? s : -INFINITY;
      m_new = fmaxf(m_new, sc[j]);
    }
    const float m_ref = (m_new == -INFINITY) ? 0.f : m_new;
    const float alpha = __expf(m - m_ref);
    l *= alpha;
#pragma unroll
    for (int i = 0; i < 16; ++i) o[i] *= alpha;
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const float pe = __expf(sc[j] - m_ref);
      l += pe;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        float vf[4];
        kv8_to_f32x4(vr[j][w], vf);
#pragma unroll
        for (int i = 0; i < 4; ++i) o[4 * w + i] += pe * vf[i];
      }
    }
    m = m_new;
  };
  {
    constexpr int BATCH = U * STEP;
    int pbA[U], pbB[U], pbC[U];
    u32x4_t kA[U], vA[U], kB[U], vB[U];
    auto shift = [&]() {
#pragma unroll
      for (int j = 0; j < U; ++j) {
        pbA[j] = pbB[j];
        pbB[j] = pbC[j];
      }
    };
    int pos0 = begin + wave * TPI;
    if (begin >= end) pos0 = end;  // empty split: no loads at all
    else {
      load_pb(pos0, pbA);
      load_pb(pos0 + BATCH, pbB);
      load_kv(pos0, pbA, kA, vA);
    }
    while (pos0 < end) {
      load_pb(pos0 + 2 * BATCH, pbC);
      load_kv(pos0 + BATCH, pbB, kB, vB);
      reduce(pos0, kA, vA);
      pos0 += BATCH;
      if (pos0 >= end) break;
      shift();
      load_pb(pos0 + 2 * BATCH, pbC);
      load_kv(pos0 + BATCH, pbB, kA, vA);
      reduce(pos0, kB, vB);
      pos0 += BATCH;
      shift();
    }
  }

  const int g = wave * TPI + t;
#pragma unroll
  for (int i = 0; i < 16; ++i) s_o[g][16 * c + i] = o[i];
  if (c == 0) {
    s_m[g] = m;
    s_l[g] = l;
  }
  __syncthreads();
  if (tid < p.D) {
    float M = -INFINITY;
    for (int j = 0; j < NSTATE; ++j) M = fmaxf(M, s_m[j]);
    float Lsum = 0.f, acc = 0.f;
    if (M != -INFINITY) {
      for (int j = 0; j < NSTATE; ++j) {
        const float w = __expf(s_m[j] - M);
        Lsum += s_l[j] * w;
        acc += s_o[j][tid] * w;
      }
    }
    const float val = (Lsum > 0.f) ? acc / Lsum * vsc[0] : 0.f;  // v_scale on the split's own output
    if (p.nsplit == 1) {
      ((T*)p.o)[b * p.os_b + h * p.os_h + (int64_t)qi * p.os_s + tid] = (T)val;
    } else {
      p.ws_o[((int64_t)row * p.nsplit + split) * p.D + tid] = val;
      if (tid == 0) p.ws_lse[(int64_t)row * p.nsplit + split] = (Lsum > 0.f) ? M + __logf(Lsum) : -INFINITY;
    }
  }
}

template <typename T, int CPRP>
__global__ __launch_bounds__(256) void decode_paged_kv8_kernel(const DecDev p, const float* ksc, const float* vsc) {
  dec_paged_kv8_body<T, CPRP, 2, false>(p, ksc, vsc, 0);
}

template <typename T, int CPRP>
__global__ __launch_bounds__(256) void decode_paged_kv8_win_kernel(const DecDev p, const float* ksc, const float* vsc,
                                                                   int wleft) {
  dec_paged_kv8_body<T, CPRP, 2, true>(p, ksc, vsc, wleft);
}

// ---- route rows: whole token rows, one workgroup per (sequence, split), one query vector per key ---------------------------
// decode_rows_body.inc (QN = 1) with a lane on 16 one-byte elements: CPR = D / 16 chunks per head row, CPT = Hkv * CPR per
// token row (16 .. 256, a power of two: dec_rows_ok with esz 1).
template <typename T, int CPR, bool WIN>
__device__ __forceinline__ void dec_rows_kv8_body(const DecDev& p, const float* ksc, const float* vsc, int wleft) {
  constexpr int U = 2;
  __shared__ float s_st[4][64][18];  // per (wave, lane): o[16], m, l

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x, split = blockIdx.y;
  const int CPT = p.Hkv * CPR;
  const int npart = CPT >= 64 ? CPT / 64 : 1;
  const int tpl = CPT >= 64 ? 1 : 64 / CPT;
  const int part = wave % npart, tslot = wave / npart;
  const int wpp = 4 / npart;
  const int tl = CPT >= 64 ? 0 : lane / CPT;
  const int cidx = CPT >= 64 ? part * 64 + lane : lane % CPT;
  const int kvh = cidx / CPR, c = cidx % CPR;
  const int ctx = p.cl[b];
  int begin = split * p.split_len;
  if constexpr (WIN) begin += dec_win_begin(ctx, p.q_len, wleft);
  int end = begin + p.split_len;
  if (end > ctx) end = ctx;
  const int h = kvh;  // H == Hkv, q_len == 1

  float qf[16];
  {
    const float qs = p.scale * ksc[0];
    const T* qp = (const T*)p.q + b * p.qs_b + h * p.qs_h + 16 * c;
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const typename DT<T>::x8 v = __builtin_bit_cast(typename DT<T>::x8, *(const u32x4_t*)(qp + 8 * hh));
#pragma unroll
      for (int i = 0; i < 8; ++i) qf[8 * hh + i] = (float)v[i] * qs;
    }
  }
  float m = -INFINITY, l = 0.f, o[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) o[i] = 0.f;

  const int64_t tok_stride = (int64_t)p.Hkv * p.D;
  const int64_t blk_stride = (int64_t)p.L * p.bs * tok_stride;
  const int64_t lay_off = (int64_t)p.layer * p.bs * tok_stride + (int64_t)cidx * 16;
  const int32_t* btrow = p.bt + (int64_t)b * p.max_blocks;
  const uint8_t* kc = (const uint8_t*)p.kc;
  const uint8_t* vc = (const uint8_t*)p.vc;
  const int step = wpp * tpl;
  const int last = end - 1;
  auto tok = [&](int pos0, int j) { return pos0 + j * step + tl; };
  auto load_pb = [&](int pos0, int (&pb)[U]) {
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const int pos = min(tok(pos0, j), last);
      pb[j] = btrow[min(pos / p.bs, p.max_blocks - 1)];
    }
  };
  auto load_kv = [&](int pos0, const int (&pb)[U], u32x4_t (&kr)[U], u32x4_t (&vr)[U]) {
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const int pos = min(tok(pos0, j), last);
      const int64_t off = (int64_t)pb[j] * blk_stride + lay_off + (int64_t)(pos % p.bs) * tok_stride;
      kr[j] = *(const u32x4_t*)(kc + off);
      vr[j] = *(const u32x4_t*)(vc + off);
    }
  };
  auto reduce = [&](int pos0, const u32x4_t (&kr)[U], const u32x4_t (&vr)[U]) {
    float sc[U];
    float m_new = m;
#pragma unroll
    for (int j = 0; j < U; ++j) {
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        float kf[4];
        kv8_to_f32x4(kr[j][w], kf);
#pragma unroll
        for (int i = 0; i < 4; ++i) s += qf[4 * w + i] * kf[i];
      }
#pragma unroll
      for (int x = 1; x < CPR; x <<= 1) s += __shfl_xor(s, x, 64);
      const int pos = tok(pos0, j);
      sc[j] = (pos < end && pos / p.bs < p.max_blocks) ? s : -INFINITY;
      if constexpr (WIN) {
        if (pos < ctx - 1 - wleft) sc[j] = -INFINITY;
      }
      m_new = fmaxf(m_new, sc[j]);
    }
    const float m_ref = (m_new == -INFINITY) ? 0.f : m_new;
    const float alpha = __expf(m - m_ref);
    l *= alpha;
#pragma unroll
    for (int i = 0; i < 16; ++i) o[i] *= alpha;
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const float pe = __expf(sc[j] - m_ref);
      l += pe;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        float vf[4];
        kv8_to_f32x4(vr[j][w], vf);
#pragma unroll
        for (int i = 0; i < 4; ++i) o[4 * w + i] += pe * vf[i];
      }
    }
    m = m_new;
  };
  {
    const int BATCH = U * step;
    int pbA[U], pbB[U], pbC[U];
    u32x4_t kA[U], vA[U], kB[U], vB[U];
    auto shift = [&]() {
#pragma unroll
      for (int j = 0; j < U; ++j) {
        pbA[j] = pbB[j];
        pbB[j] = pbC[j];
      }
    };
    int pos0 = begin + tslot * tpl;
    if (begin >= end) pos0 = end;
    else {
      load_pb(pos0, pbA);
      load_pb(pos0 + BATCH, pbB);
      load_kv(pos0, pbA, kA, vA);
    }
    while (pos0 < end) {
      load_pb(pos0 + 2 * BATCH, pbC);
      load_kv(pos0 + BATCH, pbB, kB, vB);
      reduce(pos0, kA, vA);
      pos0 += BATCH;
      if (pos0 >= end) break;
      shift();
      load_pb(pos0 + 2 * BATCH, pbC);
      load_kv(pos0 + BATCH, pbB, kA, vA);
      reduce(pos0, kB, vB);
      pos0 += BATCH;
      shift();
    }
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) s_st[wave][lane][i] = o[i];
  s_st[wave][lane][16] = m;
  s_st[wave][lane][17] = l;
  __syncthreads();
  if (tslot == 0 && tl == 0) {
    float M = -INFINITY;
    for (int w = part; w < 4; w += npart)
      for (int t2 = 0; t2 < tpl; ++t2) M = fmaxf(M, s_st[w][(CPT >= 64 ? lane : t2 * CPT + cidx)][16]);
    float Ls = 0.f, acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    if (M != -INFINITY) {
      for (int w = part; w < 4; w += npart)
        for (int t2 = 0; t2 < tpl; ++t2) {
          const float* st = s_st[w][(CPT >= 64 ? lane : t2 * CPT + cidx)];
          const float wgt = __expf(st[16] - M);
          Ls += st[17] * wgt;
#pragma unroll
          for (int i = 0; i < 16; ++i) acc[i] += st[i] * wgt;
        }
    }
    const float inv = (Ls > 0.f) ? vsc[0] / Ls : 0.f;  // v_scale on the split's own output
    const int64_t row = (int64_t)b * p.H + h;
    if (p.nsplit == 1) {
      T* op = (T*)p.o + b * p.os_b + h * p.os_h + 16 * c;
#pragma unroll
      for (int i = 0; i < 16; ++i) op[i] = (T)(acc[i] * inv);
    } else {
      float* wo = p.ws_o + (row * p.nsplit + split) * p.D + 16 * c;
#pragma unroll
      for (int i = 0; i < 16; ++i) wo[i] = acc[i] * inv;
      if (c == 0) p.ws_lse[row * p.nsplit + split] = (Ls > 0.f) ? M + __logf(Ls) : -INFINITY;
    }
  }
}

template <typename T, int CPR>
__global__ __launch_bounds__(256) void decode_rows_kv8_kernel(const DecDev p, const float* ksc, const float* vsc) {
  dec_rows_kv8_body<T, CPR, false>(p, ksc, vsc, 0);
}

template <typename T, int CPR>
__global__ __launch_bounds__(256) void decode_rows_kv8_win_kernel(const DecDev p, const float* ksc, const float* vsc,
                                                                  int wleft) {
  dec_rows_kv8_body<T, CPR, true>(p, ksc, vsc, wleft);
}

// ---- route gqa: matrix core ----------------------------------------------------------------------------------------------
// decode_gqa_body.inc over a 1-byte cache.  Per 32-key half an LDS image of 32 rows x D bytes, 16-byte chunk `ch` of row r
// stored at chunk ch ^ sw(r) (applied on the DMA's source address).  sw makes both fragment reads conflict-free within each
// 32-lane half: the K read takes one chunk of 16 consecutive rows (keys 0-15 or 16-31), the V^T read one chunk of the 16
// rows 4g .. 4g+3, 16+4g .. 16+4g+3 for g in {0, 1} (or {2, 3}); with b the row's bits, sw = [b3^b4, b2, b1] (D 128, 8
// chunks, rows 2 apart share a 256-byte bank row) and [b3^b4, b2] (D 64, 4 chunks, rows 4 apart share it).
//   K fragment (A of S^T = K . Q^T): lane (c16, g) = K[key 16 kt + c16][32 ds + 8 g .. +7]: one ds_read_b64 + 4 conversions.
//   V^T fragment (A of O^T += V^T . P^T): lane (c16, g) = V[key(k)][16 dt + c16] for k = 8 g .. 8 g + 7, key(8 g + j) =
//   4 g + j (j < 4), 16 + 4 g + j - 4 (j >= 4): one ds_read_b64_tr_b8 (lane 2 q + p of a 16-lane group addresses row q's
//   bytes 8 p .. 8 p + 7; lane i receives byte i of the 8 rows) + 4 conversions.
constexpr int DGK_NST = 2;  // (K, V) stages per wave

template <int D>
constexpr int dgk_smem_bytes() {
  return 4 * DGK_NST * (2 * 32 * D) + DG_BT_MAX * 4;
}

template <int D>
__device__ __forceinline__ int dgk_sw(int r) {
  const int x = ((r >> 3) ^ (r >> 4)) & 1;
  if constexpr (D == 128) return (x << 2) | ((r >> 1) & 3);
  else return (x << 1) | ((r >> 2) & 1);
}

template <typename T, int D, bool WIN>
__device__ __forceinline__ void dec_gqa_kv8_body(const DecDev& p, const float* ksc, const float* vsc, int wleft) {
  using X8 = typename DT<T>::x8;
  constexpr int NDS = D / 32;
  constexpr int NDT = D / 16;
  constexpr int ROWB = D;           // bytes per cached head row
  constexpr int HALF = 32 * ROWB;   // bytes of a 32-key K (or V) image
  constexpr int STAGE = 2 * HALF;
  constexpr int LPR = ROWB / 16;    // lanes (16-byte chunks) per row: 8 / 4
  constexpr int RPI = 64 / LPR;     // rows per DMA instruction: 8 / 16
  constexpr int NDMA = 32 / RPI;    // DMA instructions per image: 4 / 2
  constexpr int NL = 2 * NDMA;      // vector-memory instructions per chunk
  constexpr float LOG2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ float s_m[4][16], s_l[4][16];
  MIO_LDS int* bt_s = (MIO_LDS int*)(smem + 4 * DGK_NST * STAGE);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c16 = lane & 15, g = lane >> 4;
  const int b = blockIdx.x / p.Hkv, kvh = blockIdx.x % p.Hkv, split = blockIdx.y;
  const int rep = p.H / p.Hkv, QN = rep * p.q_len;
  const int ctx = p.cl[b];
  int begin = split * p.split_len;
  if constexpr (WIN) begin += dec_win_begin(ctx, p.q_len, wleft);
  int end = begin + p.split_len;
  if (end > ctx) end = ctx;
  {
    const int64_t cap = (int64_t)p.max_blocks * p.bs;
    if (end > cap) end = (int)cap;
  }
  const int nkeys = end > begin ? end - begin : 0;
  const int nch = (nkeys + 31) >> 5;
  const int last = end - 1;
  const int blk0 = begin / p.bs;

  if (nkeys > 0) {
    const int nb = last / p.bs - blk0 + 1;  // <= DG_BT_MAX (launcher)
    const int32_t* btrow = p.bt + (int64_t)b * p.max_blocks;
    for (int i = tid; i < nb; i += 256) bt_s[i] = btrow[blk0 + i];
  }

  X8 qf[NDS];
  {
    const bool ok = c16 < QN;
    const int j = ok ? c16 : 0;
    const T* qp = (const T*)p.q + b * p.qs_b + (int64_t)(kvh * rep + j / p.q_len) * p.qs_h + (int64_t)(j % p.q_len) * p.qs_s;
#pragma unroll
    for (int ds = 0; ds < NDS; ++ds) {
      u32x4_t raw = {0, 0, 0, 0};
      if (ok) raw = *(const u32x4_t*)(qp + 32 * ds + 8 * g);
      qf[ds] = __builtin_bit_cast(X8, raw);
    }
  }
  const float sl2 = p.scale * ksc[0] * LOG2E;  // k_scale folded into the score scale
  const float vs = vsc[0];
  __syncthreads();  // bt_s visible
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
  for (int ds = 0; ds < NDS; ++ds) asm volatile("" : "+v"(qf[ds]));

  const int64_t tok_bytes = (int64_t)p.Hkv * D;
  const char* kbase = (const char*)p.kc + (int64_t)kvh * ROWB;
  const char* vbase = (const char*)p.vc + (int64_t)kvh * ROWB;
  char* ring = smem + wave * (DGK_NST * STAGE);
  const uint32_t ring_lds = (uint32_t)(size_t)((MIO_LDS char*)ring);

  const int drow = lane / LPR, dpos = lane % LPR;
  auto issue = [&](int j, int st) __attribute__((always_inline)) {
    const uint32_t lds = __builtin_amdgcn_readfirstlane(ring_lds + (uint32_t)(st * STAGE));
#pragma unroll
    for (int i = 0; i < NDMA; ++i) {
      const int key = RPI * i + drow;
      int pos = begin + 32 * j + key;
      pos = pos < last ? pos : last;
      const int blk = bt_s[pos / p.bs - blk0];
      const int64_t row = ((int64_t)blk * p.L + p.layer) * p.bs + pos % p.bs;
      const int ch = dpos ^ dgk_sw<D>(key);
      const char* ks = kbase + row * tok_bytes + 16 * ch;
      const char* vsrc = vbase + row * tok_bytes + 16 * ch;
      const uint32_t lk = lds + 1024 * i, lv = lds + HALF + 1024 * i;
      asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" : : "s"(lk), "v"(ks) : "memory", "m0");
      asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" : : "s"(lv), "v"(vsrc) : "memory", "m0");
    }
  };

  int k_rd[2][NDS], v_rd[NDT];
  {
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      const int r = 16 * kt + c16;
#pragma unroll
      for (int ds = 0; ds < NDS; ++ds) k_rd[kt][ds] = r * ROWB + 16 * ((2 * ds + (g >> 1)) ^ dgk_sw<D>(r)) + 8 * (g & 1);
    }
    const int q8 = c16 >> 1, p8 = c16 & 1;
    const int vkey = q8 < 4 ? 4 * g + q8 : 16 + 4 * g + q8 - 4;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) v_rd[dt] = HALF + vkey * ROWB + 16 * (dt ^ dgk_sw<D>(vkey)) + 8 * p8;
  }

  int qlo = 0;
  if constexpr (WIN) qlo = ctx - p.q_len + c16 % p.q_len - wleft;
  float m = -INFINITY, l = 0.f;
  f32x4_t o[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) o[dt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  int j = wave, st = 0;
  if (j < nch) issue(j, 0);
  if (j + 4 < nch) issue(j + 4, 1);
  for (; j < nch; j += 4, st ^= 1) {
    if (j + 4 < nch) asm volatile("s_waitcnt vmcnt(%0)" : : "n"(NL) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const char* sb = ring + st * STAGE;
    f32x4_t s2[2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ds = 0; ds < NDS; ++ds) {
        const X8 kf = kv8_to_x8<T>(*(const MIO_LDS u32x2_t*)(sb + k_rd[kt][ds]));
        acc = DT<T>::mfma16(kf, qf[ds], acc);
      }
      s2[kt] = acc;
    }
    const int kpos = begin + 32 * j + 4 * g;
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float v = (kpos + 16 * kt + i < end) ? s2[kt][i] * sl2 : -INFINITY;
        if constexpr (WIN) {
          if (kpos + 16 * kt + i < qlo) v = -INFINITY;
        }
        s2[kt][i] = v;
        mx = fmaxf(mx, v);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m, mx);
    const float m_ref = (m_new == -INFINITY) ? 0.f : m_new;
    const float alpha = fast_exp2(m - m_ref);
    m = m_new;
    uint32_t pk[4];
    float psum = 0.f;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int h2 = 0; h2 < 2; ++h2) {
        const float e0 = fast_exp2(s2[kt][2 * h2] - m_ref), e1 = fast_exp2(s2[kt][2 * h2 + 1] - m_ref);
        const typename DT<T>::x2 r = __builtin_convertvector((f32x2_t){e0, e1}, typename DT<T>::x2);
        psum += (float)r[0] + (float)r[1];
        pk[2 * kt + h2] = __builtin_bit_cast(uint32_t, r);
      }
    l = l * alpha + psum;
    const X8 pf = __builtin_bit_cast(X8, (u32x4_t){pk[0], pk[1], pk[2], pk[3]});
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) {
      typedef __attribute__((ext_vector_type(2))) int i32x2_t;
      const u32x2_t raw = __builtin_bit_cast(u32x2_t, __builtin_amdgcn_ds_read_tr8_b64_v2i32((MIO_LDS i32x2_t*)(sb + v_rd[dt])));
      const X8 vf = kv8_to_x8<T>(raw);
      f32x4_t acc = o[dt];
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] *= alpha;
      o[dt] = DT<T>::mfma16(vf, pf, acc);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (j + 8 < nch) issue(j + 8, st);
  }
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);

  __syncthreads();
  MIO_LDS float* ob = (MIO_LDS float*)smem;
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) *(MIO_LDS f32x4_t*)(ob + (wave * 16 + c16) * D + 16 * dt + 4 * g) = o[dt];
  if (g == 0) {
    s_m[wave][c16] = m;
    s_l[wave][c16] = l;
  }
  __syncthreads();
  constexpr int CPQ = D / 8;
  if (tid < 16 * CPQ) {
    const int qj = tid / CPQ, c8 = tid % CPQ;
    if (qj < QN) {
      float M = -INFINITY;
#pragma unroll
      for (int w = 0; w < 4; ++w) M = fmaxf(M, s_m[w][qj]);
      float Ls = 0.f, acc[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] = 0.f;
      if (M != -INFINITY) {
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const float wgt = fast_exp2(s_m[w][qj] - M);
          Ls += s_l[w][qj] * wgt;
          const MIO_LDS float* src = ob + (w * 16 + qj) * D + 8 * c8;
#pragma unroll
          for (int i = 0; i < 8; ++i) acc[i] += src[i] * wgt;
        }
      }
      const float inv = (Ls > 0.f) ? vs / Ls : 0.f;  // v_scale on the split's own output
      const int h = kvh * rep + qj / p.q_len, qi = qj % p.q_len;
      const int64_t row = ((int64_t)b * p.H + h) * p.q_len + qi;
      if (p.nsplit == 1) {
        uint32_t w4[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) w4[i] = pack2<T>(acc[2 * i] * inv, acc[2 * i + 1] * inv);
        *(u32x4_t*)((T*)p.o + b * p.os_b + h * p.os_h + (int64_t)qi * p.os_s + 8 * c8) = (u32x4_t){w4[0], w4[1], w4[2], w4[3]};
      } else {
        float* wo = p.ws_o + (row * p.nsplit + split) * p.D + 8 * c8;
#pragma unroll
        for (int i = 0; i < 8; ++i) wo[i] = acc[i] * inv;
        if (c8 == 0) p.ws_lse[row * p.nsplit + split] = (Ls > 0.f) ? (M + fast_log2(Ls)) * LN2 : -INFINITY;
      }
    }
  }
}

template <typename T, int D>
__global__ __launch_bounds__(256) void decode_gqa_kv8_kernel(const DecDev p, const float* ksc, const float* vsc) {
  dec_gqa_kv8_body<T, D, false>(p, ksc, vsc, 0);
}

template <typename T, int D>
__global__ __launch_bounds__(256) void decode_gqa_kv8_win_kernel(const DecDev p, const float* ksc, const float* vsc,
                                                                 int wleft) {
  dec_gqa_kv8_body<T, D, true>(p, ksc, vsc, wleft);
}

// ---- host: planning and launches -----------------------------------------------------------------------------------------
// The gqa kernel's LDS image is half the 16-bit one (72 KiB at D 128): two workgroups fit a CU, so the split aims at 512.
constexpr int DGK_TARGET = 512;

static int kv8_plan(DecDev& p, int& route, const std::string& fn, const void* q, void* o, const void* k_cache,
                    const void* v_cache, const float* k_scale, const float* v_scale, const int32_t* block_tables,
                    const int32_t* context_lengths, const int64_t q_stride[3], const int64_t o_stride[3], int32_t B,
                    int32_t H, int32_t Hkv, int32_t q_len, int32_t D, int32_t num_layers, int32_t layer_idx,
                    int32_t block_size, int32_t max_blocks_per_seq, int32_t max_ctx, float scale, int32_t wleft,
                    int32_t dtype) {
  MIO_CHECK(q && o && k_cache && v_cache && block_tables && context_lengths && q_stride && o_stride, fn + ": null pointer");
  MIO_CHECK(k_scale && v_scale, fn + ": k_scale and v_scale are required with an fp8 cache (null scale pointer)");
  MIO_CHECK(((uintptr_t)k_scale & 3) == 0 && ((uintptr_t)v_scale & 3) == 0, fn + ": scales must be 4-byte aligned fp32");
  MIO_CHECK(B > 0 && H > 0 && Hkv > 0 && H % Hkv == 0 && q_len > 0, fn + ": bad sizes");
  MIO_CHECK(D >= 16 && D <= 128 && D % 16 == 0, fn + ": head_dim must be a multiple of 16 in [16,128] for an fp8 cache");
  MIO_CHECK(layer_idx >= 0 && layer_idx < num_layers, fn + ": layer_idx out of range");
  MIO_CHECK(block_size > 0 && max_blocks_per_seq > 0 && max_ctx >= 0, fn + ": bad cache geometry");
  MIO_CHECK(dtype == MIO_BF16 || dtype == MIO_FP16, fn + ": dtype (of q and o) must be bf16 or fp16");
  MIO_CHECK(wleft >= -1, fn + ": window_left must be -1 (unbounded) or >= 0");
  MIO_CHECK(wleft < 0 || q_len < (1 << 29), fn + ": q_len must be below 2^29 under a window");
  MIO_CHECK(q_stride[0] % 8 == 0 && q_stride[1] % 8 == 0 && q_stride[2] % 8 == 0 && mio_aligned16(q) &&
                mio_aligned16(k_cache) && mio_aligned16(v_cache),
            fn + ": q/cache rows must be 16-byte aligned");
  p.q = q; p.o = o; p.kc = k_cache; p.vc = v_cache; p.bt = block_tables; p.cl = context_lengths;
  p.qs_b = q_stride[0]; p.qs_h = q_stride[1]; p.qs_s = q_stride[2];
  p.os_b = o_stride[0]; p.os_h = o_stride[1]; p.os_s = o_stride[2];
  p.B = B; p.H = H; p.Hkv = Hkv; p.q_len = q_len; p.D = D; p.L = num_layers; p.layer = layer_idx;
  p.bs = block_size; p.max_blocks = max_blocks_per_seq; p.scale = scale;
  const int span = (wleft >= 0 && (int64_t)wleft + q_len < max_ctx) ? wleft + q_len : max_ctx;
  const bool gqa_kernel = dec_gqa_ok(B, H, Hkv, q_len, D, span, block_size, o_stride, o);
  const bool rows_kernel = !gqa_kernel && dec_rows_ok(B, H, Hkv, q_len, D, span, 1);
  route = gqa_kernel ? MIO_DEC_ROUTE_GQA : rows_kernel ? MIO_DEC_ROUTE_ROWS : MIO_DEC_ROUTE_HEAD;
  p.nsplit = gqa_kernel ? dec_nsplit_gqa((int64_t)B * Hkv, span, block_size, D, DGK_TARGET)
                        : rows_kernel ? dec_nsplit_rows(B, span) : dec_nsplit(B, H, q_len, span);
  int sl = (span + p.nsplit - 1) / p.nsplit;
  const int gran = gqa_kernel ? 128 : 32;
  sl = (sl + gran - 1) / gran * gran;
  if (sl < gran) sl = gran;
  p.split_len = sl;
  return 0;
}

template <typename T, int D>
static hipError_t kv8_gqa_attr() {
  static std::once_flag once;
  static hipError_t ea = hipSuccess;
  std::call_once(once, [] {
    ea = hipFuncSetAttribute((const void*)decode_gqa_kv8_kernel<T, D>, hipFuncAttributeMaxDynamicSharedMemorySize,
                             dgk_smem_bytes<D>());
    if (ea == hipSuccess)
      ea = hipFuncSetAttribute((const void*)decode_gqa_kv8_win_kernel<T, D>, hipFuncAttributeMaxDynamicSharedMemorySize,
                               dgk_smem_bytes<D>());
  });
  return ea;
}

template <typename T>
static int kv8_run(const DecDev& p, int route, int wleft, const float* ks, const float* vs, hipStream_t st) {
  const int64_t rows = (int64_t)p.B * p.H * p.q_len;
  const bool win = wleft >= 0;
  if (route == MIO_DEC_ROUTE_GQA) {
    const hipError_t ea = p.D == 128 ? kv8_gqa_attr<T, 128>() : kv8_gqa_attr<T, 64>();
    if (ea != hipSuccess) return mio_fail(std::string("decode_gqa_kv8: hipFuncSetAttribute: ") + hipGetErrorString(ea));
    const dim3 grid((unsigned)(p.B * p.Hkv), (unsigned)p.nsplit);
    if (p.D == 128) {
      if (win) hipLaunchKernelGGL((decode_gqa_kv8_win_kernel<T, 128>), grid, dim3(256), dgk_smem_bytes<128>(), st, p, ks, vs, wleft);
      else hipLaunchKernelGGL((decode_gqa_kv8_kernel<T, 128>), grid, dim3(256), dgk_smem_bytes<128>(), st, p, ks, vs);
    } else {
      if (win) hipLaunchKernelGGL((decode_gqa_kv8_win_kernel<T, 64>), grid, dim3(256), dgk_smem_bytes<64>(), st, p, ks, vs, wleft);
      else hipLaunchKernelGGL((decode_gqa_kv8_kernel<T, 64>), grid, dim3(256), dgk_smem_bytes<64>(), st, p, ks, vs);
    }
  } else if (route == MIO_DEC_ROUTE_ROWS) {  // one query vector per key (dec_rows_ok)
    const dim3 grid((unsigned)p.B, (unsigned)p.nsplit);
    if (p.D == 64) {
      if (win) hipLaunchKernelGGL((decode_rows_kv8_win_kernel<T, 4>), grid, dim3(256), 0, st, p, ks, vs, wleft);
      else hipLaunchKernelGGL((decode_rows_kv8_kernel<T, 4>), grid, dim3(256), 0, st, p, ks, vs);
    } else {
      if (win) hipLaunchKernelGGL((decode_rows_kv8_win_kernel<T, 8>), grid, dim3(256), 0, st, p, ks, vs, wleft);
      else hipLaunchKernelGGL((decode_rows_kv8_kernel<T, 8>), grid, dim3(256), 0, st, p, ks, vs);
    }
  } else {
    const dim3 grid((unsigned)rows, (unsigned)p.nsplit);
    if (p.D <= 64) {
      if (win) hipLaunchKernelGGL((decode_paged_kv8_win_kernel<T, 4>), grid, dim3(256), 0, st, p, ks, vs, wleft);
      else hipLaunchKernelGGL((decode_paged_kv8_kernel<T, 4>), grid, dim3(256), 0, st, p, ks, vs);
    } else {
      if (win) hipLaunchKernelGGL((decode_paged_kv8_win_kernel<T, 8>), grid, dim3(256), 0, st, p, ks, vs, wleft);
      else hipLaunchKernelGGL((decode_paged_kv8_kernel<T, 8>), grid, dim3(256), 0, st, p, ks, vs);
    }
  }
  if (p.nsplit > 1) hipLaunchKernelGGL(decode_reduce_kernel<T>, dim3((unsigned)rows), dim3(128), 0, st, p);
  return 0;
}

// a window no shorter than max_ctx + q_len is the unbounded one: clamped, so the kernels' bounds stay in int
static int32_t kv8_window(int32_t window_left, int32_t max_ctx, int32_t q_len) {
  if (window_left < 0) return window_left;
  return (int32_t)std::min<int64_t>(std::min<int64_t>(window_left, (int64_t)max_ctx + q_len), 1 << 29);
}

extern "C" int mio_fa3_decode_paged_kv8(const void* q, void* o, const void* k_cache, const void* v_cache,
                                        const float* k_scale, const float* v_scale, const int32_t* block_tables,
                                        const int32_t* context_lengths, const int64_t q_stride[3],
                                        const int64_t o_stride[3], int32_t B, int32_t H, int32_t Hkv, int32_t q_len,
                                        int32_t D, int32_t num_layers, int32_t layer_idx, int32_t block_size,
                                        int32_t max_blocks_per_seq, int32_t max_ctx, float scale, int32_t window_left,
                                        int32_t dtype, void* workspace, void* stream) {
  const std::string fn = "mio_fa3_decode_paged_kv8";
  DecDev p;
  int route = 0;
  const int rc = kv8_plan(p, route, fn, q, o, k_cache, v_cache, k_scale, v_scale, block_tables, context_lengths, q_stride,
                          o_stride, B, H, Hkv, q_len, D, num_layers, layer_idx, block_size, max_blocks_per_seq, max_ctx,
                          scale, window_left, dtype);
  if (rc != 0) return rc;
  const int32_t wleft = kv8_window(window_left, max_ctx, q_len);
  MIO_CHECK(p.nsplit == 1 || workspace != nullptr, fn + ": workspace required");
  const int64_t rows = (int64_t)B * H * q_len;
  p.ws_o = (float*)workspace;
  p.ws_lse = p.ws_o ? p.ws_o + rows * p.nsplit * D : nullptr;
  hipStream_t st = (hipStream_t)stream;
  const int rl = (dtype == MIO_BF16) ? kv8_run<__bf16>(p, route, wleft, k_scale, v_scale, st)
                                     : kv8_run<_Float16>(p, route, wleft, k_scale, v_scale, st);
  if (rl != 0) return rl;
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mio_fail(std::string("decode_paged_kv8 launch: ") + hipGetErrorString(e));
  return 0;
}

extern "C" int mio_fa3_decode_kv8_route(const void* q, void* o, const void* k_cache, const void* v_cache,
                                        const float* k_scale, const float* v_scale, const int32_t* block_tables,
                                        const int32_t* context_lengths, const int64_t q_stride[3],
                                        const int64_t o_stride[3], int32_t B, int32_t H, int32_t Hkv, int32_t q_len,
                                        int32_t D, int32_t num_layers, int32_t layer_idx, int32_t block_size,
                                        int32_t max_blocks_per_seq, int32_t max_ctx, float scale, int32_t window_left,
                                        int32_t dtype, void* workspace, void* stream) {
  (void)workspace;
  (void)stream;
  DecDev p;
  int route = 0;
  const int rc = kv8_plan(p, route, "mio_fa3_decode_kv8_route", q, o, k_cache, v_cache, k_scale, v_scale, block_tables,
                          context_lengths, q_stride, o_stride, B, H, Hkv, q_len, D, num_layers, layer_idx, block_size,
                          max_blocks_per_seq, max_ctx, scale, kv8_window(window_left, max_ctx, q_len), dtype);
  return rc != 0 ? rc : route;
}

// ---- quantising cache writes ---------------------------------------------------------------------------------------------
// reshape_and_cache_kv8_kernel: one workgroup per sequence, the token at context_lengths[b] - 1; a thread owns one 16-byte
// chunk (16 elements) of the cached row: two 16-byte loads of each of K and V, one 16-byte store of each.
template <typename T>
__global__ __launch_bounds__(256) void reshape_and_cache_kv8_kernel(
    const T* __restrict__ key, const T* __restrict__ value, uint8_t* __restrict__ kc, uint8_t* __restrict__ vc,
    const float* __restrict__ ksc, const float* __restrict__ vsc, const int32_t* __restrict__ bt,
    const int32_t* __restrict__ cl, int64_t ks_b, int64_t ks_h, int64_t vs_b, int64_t vs_h, int Hkv, int D, int L,
    int layer, int bs, int max_blocks) {
  const int b = blockIdx.x;
  const int pos = cl[b] - 1;
  if (pos < 0 || pos / bs >= max_blocks) return;  // empty sequence / context longer than the block table row: nothing written
  const int pb = bt[(int64_t)b * max_blocks + pos / bs];
  const float kinv = 1.0f / ksc[0], vinv = 1.0f / vsc[0];
  const int64_t tok_stride = (int64_t)Hkv * D;
  const int64_t dst = ((int64_t)pb * L + layer) * bs * tok_stride + (int64_t)(pos % bs) * tok_stride;
  const int cpr = D >> 4;
  for (int i = threadIdx.x; i < Hkv * cpr; i += 256) {
    const int hh = i / cpr, c = i % cpr;
    const T* kp = key + b * ks_b + hh * ks_h + 16 * c;
    const T* vp = value + b * vs_b + hh * vs_h + 16 * c;
    const u32x4_t k0 = *(const u32x4_t*)kp, k1 = *(const u32x4_t*)(kp + 8);
    const u32x4_t v0 = *(const u32x4_t*)vp, v1 = *(const u32x4_t*)(vp + 8);
    *(u32x4_t*)(kc + dst + (int64_t)hh * D + 16 * c) = kv8_quant16<T>(k0, k1, kinv);
    *(u32x4_t*)(vc + dst + (int64_t)hh * D + 16 * c) = kv8_quant16<T>(v0, v1, vinv);
  }
}

// reshape_and_cache_varlen_kv8_kernel: reshape_and_cache_varlen_kernel with a thread per 16-byte chunk (16 elements) of the
// cached row; the same sequence search and skipping rules.
template <typename T>
__global__ __launch_bounds__(256) void reshape_and_cache_varlen_kv8_kernel(
    const T* __restrict__ key, const T* __restrict__ value, uint8_t* __restrict__ kc, uint8_t* __restrict__ vc,
    const float* __restrict__ ksc, const float* __restrict__ vsc, const int32_t* __restrict__ bt,
    const int32_t* __restrict__ cu, const int32_t* __restrict__ cl, int64_t ks_t, int64_t ks_h, int64_t vs_t,
    int64_t vs_h, int B, int total, int Hkv, int D, int num_blocks, int L, int layer, int bs, int max_blocks) {
  const int cpr = D >> 4, cpt = Hkv * cpr;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)total * cpt) return;
  const int t = (int)(i / cpt), c = (int)(i % cpt), hh = c / cpr, cc = c % cpr;
  auto cu_at = [&](int b) { const int x = cu[b]; return x < 0 ? 0 : (x > total ? total : x); };
  int lo = 0, hi = B;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (cu_at(mid) <= t) lo = mid; else hi = mid;
  }
  const int b = lo, s0 = cu_at(b), s1e = cu_at(b + 1), s1 = s1e > s0 ? s1e : s0;
  if (t < s0 || t >= s1) return;
  const int pos = cl[b] - (s1 - s0) + (t - s0);
  if (pos < 0 || pos / bs >= max_blocks) return;
  const int pb = bt[(int64_t)b * max_blocks + pos / bs];
  if (pb < 0 || pb >= num_blocks) return;
  const int64_t dst = (((int64_t)pb * L + layer) * bs + pos % bs) * ((int64_t)Hkv * D) + (int64_t)hh * D + 16 * cc;
  const T* kp = key + t * ks_t + hh * ks_h + 16 * cc;
  const T* vp = value + t * vs_t + hh * vs_h + 16 * cc;
  const u32x4_t k0 = *(const u32x4_t*)kp, k1 = *(const u32x4_t*)(kp + 8);
  const u32x4_t v0 = *(const u32x4_t*)vp, v1 = *(const u32x4_t*)(vp + 8);
  *(u32x4_t*)(kc + dst) = kv8_quant16<T>(k0, k1, 1.0f / ksc[0]);
  *(u32x4_t*)(vc + dst) = kv8_quant16<T>(v0, v1, 1.0f / vsc[0]);
}

static bool kv8_scales_ok(const float* k_scale, const float* v_scale) {
  return k_scale && v_scale && ((uintptr_t)k_scale & 3) == 0 && ((uintptr_t)v_scale & 3) == 0;
}

extern "C" int mio_reshape_and_cache_kv8(const void* key, const void* value, void* k_cache, void* v_cache,
                                         const float* k_scale, const float* v_scale, const int32_t* block_tables,
                                         const int32_t* context_lengths, const int64_t k_stride[2],
                                         const int64_t v_stride[2], int32_t B, int32_t Hkv, int32_t D,
                                         int32_t num_layers, int32_t layer_idx, int32_t block_size,
                                         int32_t max_blocks_per_seq, int32_t dtype, void* stream) {
  const char* fn = "mio_reshape_and_cache_kv8";
  MIO_CHECK(key && value && k_cache && v_cache && block_tables && context_lengths && k_stride && v_stride,
            std::string(fn) + ": null pointer");
  MIO_CHECK(kv8_scales_ok(k_scale, v_scale), std::string(fn) + ": k_scale and v_scale are required with an fp8 cache "
                                                               "(null scale pointer or not 4-byte aligned)");
  MIO_CHECK(B > 0 && Hkv > 0, std::string(fn) + ": bad sizes");
  MIO_CHECK(D >= 16 && D % 16 == 0, std::string(fn) + ": head_dim must be a multiple of 16 for an fp8 cache");
  MIO_CHECK(layer_idx >= 0 && layer_idx < num_layers && block_size > 0 && max_blocks_per_seq > 0,
            std::string(fn) + ": bad cache geometry");
  MIO_CHECK(dtype == MIO_BF16 || dtype == MIO_FP16, std::string(fn) + ": dtype (of key and value) must be bf16 or fp16");
  MIO_CHECK(k_stride[0] % 8 == 0 && k_stride[1] % 8 == 0 && v_stride[0] % 8 == 0 && v_stride[1] % 8 == 0 &&
                mio_aligned16(key) && mio_aligned16(value) && mio_aligned16(k_cache) && mio_aligned16(v_cache),
            std::string(fn) + ": 16-byte alignment");
  hipStream_t st = (hipStream_t)stream;
  if (dtype == MIO_BF16)
    hipLaunchKernelGGL(reshape_and_cache_kv8_kernel<__bf16>, dim3((unsigned)B), dim3(256), 0, st, (const __bf16*)key,
                       (const __bf16*)value, (uint8_t*)k_cache, (uint8_t*)v_cache, k_scale, v_scale, block_tables,
                       context_lengths, k_stride[0], k_stride[1], v_stride[0], v_stride[1], Hkv, D, num_layers,
                       layer_idx, block_size, max_blocks_per_seq);
  else
    hipLaunchKernelGGL(reshape_and_cache_kv8_kernel<_Float16>, dim3((unsigned)B), dim3(256), 0, st, (const _Float16*)key,
                       (const _Float16*)value, (uint8_t*)k_cache, (uint8_t*)v_cache, k_scale, v_scale, block_tables,
                       context_lengths, k_stride[0], k_stride[1], v_stride[0], v_stride[1], Hkv, D, num_layers,
                       layer_idx, block_size, max_blocks_per_seq);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mio_fail(std::string("reshape_and_cache_kv8 launch: ") + hipGetErrorString(e));
  return 0;
}

extern "C" int mio_reshape_and_cache_varlen_kv8(const void* key, const void* value, void* k_cache, void* v_cache,
                                                const float* k_scale, const float* v_scale,
                                                const int32_t* block_tables, const int32_t* cu_seqlens_new,
                                                const int32_t* context_lengths, const int64_t k_stride[2],
                                                const int64_t v_stride[2], int32_t B, int32_t total_new, int32_t Hkv,
                                                int32_t D, int32_t num_blocks, int32_t num_layers, int32_t layer_idx,
                                                int32_t block_size, int32_t max_blocks_per_seq, int32_t dtype,
                                                void* stream) {
  const char* fn = "mio_reshape_and_cache_varlen_kv8";
  MIO_CHECK(k_stride != nullptr && v_stride != nullptr, std::string(fn) + ": null strides");
  MIO_CHECK(kv8_scales_ok(k_scale, v_scale), std::string(fn) + ": k_scale and v_scale are required with an fp8 cache "
                                                               "(null scale pointer or not 4-byte aligned)");
  MIO_CHECK(B >= 0 && total_new >= 0 && Hkv > 0, std::string(fn) + ": bad sizes");
  MIO_CHECK(D >= 16 && D % 16 == 0, std::string(fn) + ": head_dim must be a multiple of 16 for an fp8 cache");
  MIO_CHECK(num_blocks > 0 && num_layers > 0 && layer_idx >= 0 && layer_idx < num_layers && block_size > 0 &&
                max_blocks_per_seq > 0,
            std::string(fn) + ": bad cache geometry");
  MIO_CHECK(dtype == MIO_BF16 || dtype == MIO_FP16, std::string(fn) + ": dtype (of key and value) must be bf16 or fp16");
  if (B == 0 || total_new == 0) return 0;
  MIO_CHECK(key && value && k_cache && v_cache && block_tables && cu_seqlens_new && context_lengths,
            std::string(fn) + ": null pointer");
  MIO_CHECK(k_stride[0] >= 0 && k_stride[1] >= 0 && v_stride[0] >= 0 && v_stride[1] >= 0 && k_stride[0] % 8 == 0 &&
                k_stride[1] % 8 == 0 && v_stride[0] % 8 == 0 && v_stride[1] % 8 == 0 && mio_aligned16(key) &&
                mio_aligned16(value) && mio_aligned16(k_cache) && mio_aligned16(v_cache),
            std::string(fn) + ": 16-byte alignment");
  const int64_t blocks = ((int64_t)total_new * Hkv * (D / 16) + 255) / 256;
  MIO_CHECK(blocks <= 0x7fffffff, std::string(fn) + ": too many tokens");
  hipStream_t st = (hipStream_t)stream;
  if (dtype == MIO_BF16)
    hipLaunchKernelGGL(reshape_and_cache_varlen_kv8_kernel<__bf16>, dim3((unsigned)blocks), dim3(256), 0, st,
                       (const __bf16*)key, (const __bf16*)value, (uint8_t*)k_cache, (uint8_t*)v_cache, k_scale, v_scale,
                       block_tables, cu_seqlens_new, context_lengths, k_stride[0], k_stride[1], v_stride[0],
                       v_stride[1], B, total_new, Hkv, D, num_blocks, num_layers, layer_idx, block_size,
                       max_blocks_per_seq);
  else
    hipLaunchKernelGGL(reshape_and_cache_varlen_kv8_kernel<_Float16>, dim3((unsigned)blocks), dim3(256), 0, st,
                       (const _Float16*)key, (const _Float16*)value, (uint8_t*)k_cache, (uint8_t*)v_cache, k_scale,
                       v_scale, block_tables, cu_seqlens_new, context_lengths, k_stride[0], k_stride[1], v_stride[0],
                       v_stride[1], B, total_new, Hkv, D, num_blocks, num_layers, layer_idx, block_size,
                       max_blocks_per_seq);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return mio_fail(std::string("reshape_and_cache_varlen_kv8 launch: ") + hipGetErrorString(e));
  return 0;
}

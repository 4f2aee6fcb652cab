// FlashAttention forward, third structure (head dim 64, no user mask): software-pipelined across KV tiles.
//
// The retired sequential structure (fa3_fwd2_kernel: one wave per SIMD, 64 query rows per wave) ran each tile as
// QK^T -> softmax -> PV in sequence, so the matrix core idled during the softmax and the vector ALU during the MFMAs:
// 2375 cycles per tile against 1024 of MFMA work (rocprofv3 SQ counters).  Here, per wave and tile t:
//   phase 1   S(t+1) = K(t+1) . Q^T                  16 MFMAs   ||   P(t) = exp2(S(t))                  64 v_exp + 32 v_cvt_pk
//   phase 2   O^T += V(t)^T . P(t)^T, L += ones . P(t)^T  24 MFMAs   ||   S(t+1) := S(t+1)*c - ref, row max    64 v_fma + 32 v_max3, DMA issue
// with S double-buffered in VGPRs.  What makes the two sides balance:
//   * the scale-and-subtract of tile t+1 (exp2 domain, against the CURRENT reference) and its row maximum ride in the
//     vector slack of the PV phase, so the exp phase is exp + convert only;
//   * row sums come from the matrix core: L^T += ones(32x16) . P^T into a 32x32 accumulator whose registers all hold
//     the row sum (no v_add per element);
//   * every MFMA is an asm statement on asm-owned registers: O^T, L, Q, ones live in the accumulator file (MFMA
//     A/B operands may come from there), which leaves the 256 architectural VGPRs to S (128), P (32) and the K / V
//     fragments -- and every phase is a fixed sequence of micro-steps (MFMA + its share of the vector work) pinned
//     with sched_barrier(0).  (Compiler-visible "+a"/"a" operands were tried: accumulator tuples get copied at branch
//     joins right behind an asm MFMA whose latency the compiler does not know -- lost updates -- and "a" inputs are
//     re-copied from VGPRs before every use.)
// The reference only moves when a row outgrows it by 2^FA_RESCALE_THR (flash_attention_kernels.py:276-298 is the
// algorithm: online softmax with running max / sum; exp -> exp2).  K/V tiles go global -> LDS by DMA through a 4-stage
// ring (K(t+1) and V(t) are read while tiles t+2 and t+3 are in flight: a tile has two iterations to land), one
// barrier per tile.
#pragma once
#include "fa3_varlen.h"

// Accumulator tile k (16 registers) = a[16k : 16k+15], asm-owned: every statement names its registers as clobbers, so
// hipcc allocates them in the kernel descriptor and never touches them itself.
template <typename T, int K>
struct Fa2Acc;
#define FA2_CL(B) "a" #B
#define FA2_DEF(K, R0, R1, R2, R3, R4, R5, R6, R7, R8, R9, R10, R11, R12, R13, R14, R15)                          \
  template <>                                                                                                     \
  struct Fa2Acc<__bf16, K> {                                                                                      \
    static __device__ __forceinline__ void mfma(bf16x8_t a, bf16x8_t b) {                                         \
      asm volatile("v_mfma_f32_32x32x16_bf16 a[" #R0 ":" #R15 "], %0, %1, a[" #R0 ":" #R15 "]"                     \
                   :                                                                                              \
                   : "v"(a), "v"(b)                                                                               \
                   : FA2_CL(R0), FA2_CL(R1), FA2_CL(R2), FA2_CL(R3), FA2_CL(R4), FA2_CL(R5), FA2_CL(R6), FA2_CL(R7), \
                     FA2_CL(R8), FA2_CL(R9), FA2_CL(R10), FA2_CL(R11), FA2_CL(R12), FA2_CL(R13), FA2_CL(R14),      \
                     FA2_CL(R15));                                                                                \
    }                                                                                                             \
  };                                                                                                              \
  template <>                                                                                                     \
  struct Fa2Acc<_Float16, K> {                                                                                    \
    static __device__ __forceinline__ void mfma(f16x8_t a, f16x8_t b) {                                           \
      asm volatile("v_mfma_f32_32x32x16_f16 a[" #R0 ":" #R15 "], %0, %1, a[" #R0 ":" #R15 "]"                      \
                   :                                                                                              \
                   : "v"(a), "v"(b)                                                                               \
                   : FA2_CL(R0), FA2_CL(R1), FA2_CL(R2), FA2_CL(R3), FA2_CL(R4), FA2_CL(R5), FA2_CL(R6), FA2_CL(R7), \
                     FA2_CL(R8), FA2_CL(R9), FA2_CL(R10), FA2_CL(R11), FA2_CL(R12), FA2_CL(R13), FA2_CL(R14),      \
                     FA2_CL(R15));                                                                                \
    }                                                                                                             \
  };                                                                                                              \
  template <>                                                                                                     \
  struct Fa2AccIO<K> {                                                                                            \
    template <int G>                                                                                              \
    static __device__ __forceinline__ f32x4_t read4() { /* registers 4G..4G+3 of the tile */                      \
      float x0, x1, x2, x3;                                                                                       \
      if constexpr (G == 0)                                                                                       \
        asm volatile("v_accvgpr_read_b32 %0, a" #R0 "\n\tv_accvgpr_read_b32 %1, a" #R1 "\n\tv_accvgpr_read_b32 %2, a" #R2 \
                     "\n\tv_accvgpr_read_b32 %3, a" #R3 : "=v"(x0), "=v"(x1), "=v"(x2), "=v"(x3));                    \
      else if constexpr (G == 1)                                                                                  \
        asm volatile("v_accvgpr_read_b32 %0, a" #R4 "\n\tv_accvgpr_read_b32 %1, a" #R5 "\n\tv_accvgpr_read_b32 %2, a" #R6 \
                     "\n\tv_accvgpr_read_b32 %3, a" #R7 : "=v"(x0), "=v"(x1), "=v"(x2), "=v"(x3));                    \
      else if constexpr (G == 2)                                                                                  \
        asm volatile("v_accvgpr_read_b32 %0, a" #R8 "\n\tv_accvgpr_read_b32 %1, a" #R9 "\n\tv_accvgpr_read_b32 %2, a" #R10 \
                     "\n\tv_accvgpr_read_b32 %3, a" #R11 : "=v"(x0), "=v"(x1), "=v"(x2), "=v"(x3));                   \
      else                                                                                                        \
        asm volatile("v_accvgpr_read_b32 %0, a" #R12 "\n\tv_accvgpr_read_b32 %1, a" #R13 "\n\tv_accvgpr_read_b32 %2, a" #R14 \
                     "\n\tv_accvgpr_read_b32 %3, a" #R15 : "=v"(x0), "=v"(x1), "=v"(x2), "=v"(x3));                   \
      return (f32x4_t){x0, x1, x2, x3};                                                                           \
    }                                                                                                             \
    template <int G>                                                                                              \
    static __device__ __forceinline__ void write4(f32x4_t v) {                                                    \
      if constexpr (G == 0)                                                                                       \
        asm volatile("v_accvgpr_write_b32 a" #R0 ", %0\n\tv_accvgpr_write_b32 a" #R1 ", %1\n\tv_accvgpr_write_b32 a" #R2 \
                     ", %2\n\tv_accvgpr_write_b32 a" #R3 ", %3" : : "v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3])          \
                     : FA2_CL(R0), FA2_CL(R1), FA2_CL(R2), FA2_CL(R3));                                            \
      else if constexpr (G == 1)                                                                                  \
        asm volatile("v_accvgpr_write_b32 a" #R4 ", %0\n\tv_accvgpr_write_b32 a" #R5 ", %1\n\tv_accvgpr_write_b32 a" #R6 \
                     ", %2\n\tv_accvgpr_write_b32 a" #R7 ", %3" : : "v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3])          \
                     : FA2_CL(R4), FA2_CL(R5), FA2_CL(R6), FA2_CL(R7));                                            \
      else if constexpr (G == 2)                                                                                  \
        asm volatile("v_accvgpr_write_b32 a" #R8 ", %0\n\tv_accvgpr_write_b32 a" #R9 ", %1\n\tv_accvgpr_write_b32 a" #R10 \
                     ", %2\n\tv_accvgpr_write_b32 a" #R11 ", %3" : : "v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3])         \
                     : FA2_CL(R8), FA2_CL(R9), FA2_CL(R10), FA2_CL(R11));                                          \
      else                                                                                                        \
        asm volatile("v_accvgpr_write_b32 a" #R12 ", %0\n\tv_accvgpr_write_b32 a" #R13 ", %1\n\tv_accvgpr_write_b32 a" #R14 \
                     ", %2\n\tv_accvgpr_write_b32 a" #R15 ", %3" : : "v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3])         \
                     : FA2_CL(R12), FA2_CL(R13), FA2_CL(R14), FA2_CL(R15));                                        \
    }                                                                                                             \
  };
template <int K>
struct Fa2AccIO;
FA2_DEF(0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)
FA2_DEF(1, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31)
FA2_DEF(2, 32, 33, 34, 35, 36, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 47)
FA2_DEF(3, 48, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58, 59, 60, 61, 62, 63)
FA2_DEF(4, 64, 65, 66, 67, 68, 69, 70, 71, 72, 73, 74, 75, 76, 77, 78, 79)
FA2_DEF(5, 80, 81, 82, 83, 84, 85, 86, 87, 88, 89, 90, 91, 92, 93, 94, 95)
FA2_DEF(6, 96, 97, 98, 99, 100, 101, 102, 103, 104, 105, 106, 107, 108, 109, 110, 111)
FA2_DEF(7, 112, 113, 114, 115, 116, 117, 118, 119, 120, 121, 122, 123, 124, 125, 126, 127)
// tiles 8..15 = a[128:255]: the top of the accumulator file, where fa3_fwd3 keeps its accumulators, out of
// the way of the low registers the allocator hands out first
FA2_DEF(8, 128, 129, 130, 131, 132, 133, 134, 135, 136, 137, 138, 139, 140, 141, 142, 143)
FA2_DEF(9, 144, 145, 146, 147, 148, 149, 150, 151, 152, 153, 154, 155, 156, 157, 158, 159)
FA2_DEF(10, 160, 161, 162, 163, 164, 165, 166, 167, 168, 169, 170, 171, 172, 173, 174, 175)
FA2_DEF(11, 176, 177, 178, 179, 180, 181, 182, 183, 184, 185, 186, 187, 188, 189, 190, 191)
FA2_DEF(12, 192, 193, 194, 195, 196, 197, 198, 199, 200, 201, 202, 203, 204, 205, 206, 207)
FA2_DEF(13, 208, 209, 210, 211, 212, 213, 214, 215, 216, 217, 218, 219, 220, 221, 222, 223)
FA2_DEF(14, 224, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 235, 236, 237, 238, 239)
FA2_DEF(15, 240, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250, 251, 252, 253, 254, 255)
#undef FA2_DEF

constexpr int FA3_BM = 256;     // query rows per workgroup (4 waves x 64)
constexpr int FA3_STAGES = 4;
// Accumulator-file map (all asm-owned, at the TOP of the file: the allocator hands out a0, a1, ... for its own
// values first; tests/test_host_logic.py verifies after every build that no compiler-generated instruction touches
// Fa3Map<D>::A_Q and up):
//   L tile qt = Fa2Acc tile 14 + qt = a[224:255]             O^T tile qt*DT+dt = Fa2Acc tile T_O + qt*DT+dt, right below
//   ones (A operand, all ones) = the 4 registers below O^T    Q fragment (qt, ks) = a[A_Q + 4 KS qt + 4 ks : +3], below
template <int D>
struct Fa3Map {
  static constexpr int KS = D / 16, DT = D / 32;
  static constexpr int T_L = 14, T_O = 14 - 2 * DT;
  static constexpr int A_ONES = 16 * T_O - 4, A_Q = A_ONES - 8 * KS;  // D = 64: 156 / 124, 96: 124 / 76, 128: 92 / 28
  static constexpr int CPRK = D / 8 + 1;          // 16-byte chunks per padded K row
  static constexpr int KU = CPRK, VU = D / 8;     // 1-KiB DMA units of the K / V tile of a stage
  static constexpr int NU = KU + VU, UPW = (NU + 3) / 4;  // units per stage, per wave
};

// write one accumulator register a[R] (R >= Fa3Map<D>::A_Q: the asm-owned range; the MFMA statements' clobber lists
// make the whole file part of the kernel's allocation)
template <int R>
struct Fa3AW {
  static __device__ __forceinline__ void w(uint32_t v) {
    asm volatile("v_accvgpr_write_b32 a[%1], %0" : : "v"(v), "n"(R));
  }
};

template <typename T>
struct Fa3Ops;
#define FA3_OPS(TY, SUF)                                                                                              \
  template <>                                                                                                         \
  struct Fa3Ops<TY> {                                                                                                 \
    using X8 = typename DT<TY>::x8;                                                                                   \
    /* S (+)= K fragment (VGPR) . Q fragment a[R:R+3]; FIRST: S = ... (C = 0) */                                     \
    template <int R, bool FIRST>                                                                                      \
    static __device__ __forceinline__ void qk(f32x16_t& acc, const X8& kf) {                                          \
      if constexpr (FIRST)                                                                                            \
        asm volatile("v_mfma_f32_32x32x16_" SUF " %0, %1, a[%2:%3], 0" : "=v"(acc) : "v"(kf), "n"(R), "n"(R + 3));    \
      else                                                                                                            \
        asm volatile("v_mfma_f32_32x32x16_" SUF " %0, %1, a[%2:%3], %0" : "+v"(acc) : "v"(kf), "n"(R), "n"(R + 3));   \
    }                                                                                                                 \
    /* first k-step with the running reference as the C operand: S = K fragment . Q fragment + c (KPRE) */           \
    template <int R>                                                                                                  \
    static __device__ __forceinline__ void qk_c(f32x16_t& acc, const X8& kf, const f32x16_t& c) {                    \
      asm volatile("v_mfma_f32_32x32x16_" SUF " %0, %1, a[%2:%3], %4" : "=&v"(acc) : "v"(kf), "n"(R), "n"(R + 3), "v"(c)); \
    }                                                                                                                 \
    template <int RO>                                                                                                 \
    static __device__ __forceinline__ void lsum0(const X8& pf) {                                                      \
      asm volatile("v_mfma_f32_32x32x16_" SUF " a[224:239], a[%1:%2], %0, a[224:239]"                                 \
                   :                                                                                                  \
                   : "v"(pf), "n"(RO), "n"(RO + 3)                                                                    \
                   : "a224", "a225", "a226", "a227", "a228", "a229", "a230", "a231", "a232", "a233", "a234", "a235",  \
                     "a236", "a237", "a238", "a239");                                                                 \
    }                                                                                                                 \
    template <int RO>                                                                                                 \
    static __device__ __forceinline__ void lsum1(const X8& pf) {                                                      \
      asm volatile("v_mfma_f32_32x32x16_" SUF " a[240:255], a[%1:%2], %0, a[240:255]"                                 \
                   :                                                                                                  \
                   : "v"(pf), "n"(RO), "n"(RO + 3)                                                                    \
                   : "a240", "a241", "a242", "a243", "a244", "a245", "a246", "a247", "a248", "a249", "a250", "a251",  \
                     "a252", "a253", "a254", "a255");                                                                 \
    }                                                                                                                 \
  };
FA3_OPS(__bf16, "bf16")
FA3_OPS(_Float16, "f16")
#undef FA3_OPS

// Phase 2 gives every micro-step (= one MFMA, 32 matrix-pipe cycles of which the issue port is held for 8) exactly ONE
// piece of side work, so that the step stays inside the MFMA's shadow: the V fragment read of the next k-step (3 steps,
// fixed by the fragment ring), one of the 16 scale / max groups (4 fma + 2 max3 = 24 issue cycles), or one DMA unit.
// Stacked on the same step (as they were: scale / max on steps 2..17, reads on 1 / 7 / 13, DMA on every fourth) the
// dense steps overflow the shadow and the matrix pipe waits.  role(j): 0 nothing, 1 + i scale / max group i,
// 32 + k DMA unit k.  Order: a DMA unit first, then four groups and a unit alternately, the remaining units last.
template <int NS2, int PS, int UPW>
struct Fa3P2Role {
  static constexpr int role(int j) {
    int n_v = 0, n_d = 0;
    for (int jj = 0; jj < NS2; ++jj) {
      const int s = jj / PS, m = jj % PS;
      const bool rd = (m == 1 && s + 1 < 4);
      int r = 0;
      if (!rd) {
        const bool want_d = n_d < UPW && (n_d == 0 || n_v >= 4 * n_d || n_v == 16);
        if (want_d) {
          r = 32 + n_d;
          ++n_d;
        } else if (n_v < 16) {
          r = 1 + n_v;
          ++n_v;
        }
      }
      if (jj == j) return r;
    }
    return 0;
  }
  static constexpr int count(int lo, int hi) {  // steps with a role in [lo, hi)
    int n = 0;
    for (int jj = 0; jj < NS2; ++jj) n += (role(jj) >= lo && role(jj) < hi) ? 1 : 0;
    return n;
  }
  static_assert(count(1, 17) == 16 && count(32, 32 + UPW) == UPW, "phase 2: not every scale/max group or DMA unit has a step");
};

// ABL (diagnostic build only, timing-only ablations with WRONG results -- what each piece of the tile loop costs):
//   1 no scale-and-subtract / max in phase 2     2 no exp (P = converted S)     4 no row-sum MFMAs
//   8 no DMA issue in the tile loop              16 no reference test / update  32 no edge masks
// KPRE (FaDev::k_prescaled; see fa3_fwd5_kernel.h): K carries softmax_scale * log2(e).  The reference enters the QK^T
// product as the C operand of its first k-step (one 16-register tuple per query sub-tile), phase 2 loses its 64 v_fma +
// 32 v_max3 per tile, and the rescale test is bit 14 of the OR of the tile's packed P words (move_ref below).
template <typename T>
struct Fa3Margin { static constexpr float value = 5.0f; };
template <>
struct Fa3Margin<_Float16> { static constexpr float value = 2.0f; };

template <typename T, int D, bool CAUSAL, bool STAMP = false, int ABL = 0, bool KPRE = false>
__global__ __launch_bounds__(256) void fa3_fwd3_kernel(const FaDev p) {
#define FA_KV_TILE FA_KV_TILE_STRIDED
#define FA_LSE_INDEX(b, head, row) (((int64_t)(b) * p.H + (head)) * p.Sq + (row))
#include "fa3_fwd3_body.inc"
#undef FA_LSE_INDEX
#undef FA_KV_TILE
}

// packed variable-length form (mio_fa3_fwd_varlen, fa3_varlen.h), plain K and output: the dense body on this workgroup's
// sequence
template <typename T, int D, bool CAUSAL>
__global__ __launch_bounds__(256) void fa3_fwd3_varlen_kernel(const FaDev pl, const FaVarlen vl) {
  constexpr bool STAMP = false, KPRE = false;
  constexpr int ABL = 0;
  FaDev p = pl;
  if (!fa_varlen_prepare<FA3_BM, 256, CAUSAL>(p, vl)) return;
#define FA_KV_TILE FA_KV_TILE_STRIDED
#define FA_LSE_INDEX(b, head, row) ((int64_t)(head) * vl.total_q + (row))
#include "fa3_fwd3_body.inc"
#undef FA_LSE_INDEX
#undef FA_KV_TILE
}

// The decode-step GEMM's K loop on 16-bit weights is written once, in two pieces of text that gemm_skinny_kernel (gemm_skinny.hip)
// and moe_gemm_kernel (moe.hip, the grouped GEMM of the mixture-of-experts unit) include inside their bodies, as the decode units
// include theirs: this set-up, and the loop (gemm_skinny_w16_loop.inc).  Text, and in two pieces, because each kernel then
// compiles to the very instructions it had with the loop written out in it; a function template over a rows type, a rows object
// with methods, or the expert's row lookup moved away from between the pieces each gave the compiler another order to work in.
//
// This piece: the tile's constants, the x stage in LDS, the lane's coordinates, the slice of K and the weight rows.  T, MF, GLU and
// the launch's arguments `p` (x, w, wg, ldw, N, K, steps, nsplit) come from the including kernel, and so does
//   wbase()   elements from p.w (and p.wg) to the weight this workgroup reads: 0, or expert * expert_stride.
// A kernel that leaves early (an expert without rows) does so in front of this piece: every thread that enters reaches every barrier.
  using X8 = typename DT<T>::x8;
  using Tile = SkinnyW16Tile<MF, GLU>;
  constexpr int SKC = Tile::SKC, KS = Tile::KS, PCS = Tile::PCS, ROWB = Tile::ROWB, XPT = Tile::XPT;
  __shared__ __attribute__((aligned(16))) char sx[2][Tile::ROWS * ROWB];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, q = lane >> 4;
  const int n0 = blockIdx.x * SKINNY_BN + wave * 16;
  const bool active = n0 < p.N;  // (a wave past the last column stages x and keeps the barriers, nothing else)
  const int s = blockIdx.y;
  int kb, ke;
  skinny_slice_range(p.steps, p.nsplit, SKINNY_KSTEP, p.K, s, kb, ke);
  const int nc = (ke - kb + SKC - 1) / SKC;

  const int nrow = min(n0 + c, p.N - 1);
  const T* wrow = (const T*)p.w + wbase() + (int64_t)nrow * p.ldw;
  const T* grow = GLU ? (const T*)p.wg + wbase() + (int64_t)nrow * p.ldw : nullptr;
  const T* xg = (const T*)p.x;

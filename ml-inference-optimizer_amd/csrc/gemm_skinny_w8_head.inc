// The decode-step GEMM's K loop on e4m3fn weights is written once, in two pieces of text that gemm_skinny_w8_kernel
// (gemm_skinny_w8.hip) and moe_gemm_w8_kernel (moe_w8.hip, the grouped GEMM on FP8 expert weights) include inside their bodies, as
// the 16-bit kernels include theirs: this set-up, and the loop (gemm_skinny_w8_loop.inc).  Text in two pieces for the reason
// gemm_skinny_w16_head.inc gives: each kernel then compiles to the very instructions it had with the loop written out in it.
//
// This piece: the tile's constants, the x stage in LDS, the lane's coordinates, the slice of K and the weight rows.  T, MF, GLU and
// the launch's arguments `p` (x, w, wg, ldw, N, K, steps, nsplit) come from the including kernel, and so does
//   wbase()   bytes from p.w (and p.wg) to the weight this workgroup reads: 0, or expert * expert_stride.
// A kernel that leaves early (an expert without rows) does so in front of this piece: every thread that enters reaches every barrier.
  using X8 = typename DT<T>::x8;
  using Tile = SkinnyW8Tile<MF, GLU>;
  constexpr int SKC = Tile::SKC, D = Tile::D, KS = Tile::KS, PCS = Tile::PCS, ROWB = Tile::ROWB, XPT = Tile::XPT;
  __shared__ __attribute__((aligned(16))) char sx[2][Tile::ROWS * ROWB];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, q = lane >> 4;
  const int n0 = blockIdx.x * SKINNY_BN + wave * 16;
  const bool active = n0 < p.N;  // (a wave past the last column stages x and keeps the barriers, nothing else)
  const int s = blockIdx.y;
  int kb, ke;
  skinny_slice_range(p.steps, p.nsplit, SKINNY_W8_KSTEP, p.K, s, kb, ke);
  const int nc = (ke - kb + SKC - 1) / SKC;

  const int nrow = min(n0 + c, p.N - 1);
  const int64_t woff = wbase() + (int64_t)nrow * p.ldw;
  const uint8_t* wrow = (const uint8_t*)p.w + woff;
  const uint8_t* grow = GLU ? (const uint8_t*)p.wg + woff : nullptr;
  const T* xg = (const T*)p.x;

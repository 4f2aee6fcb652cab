// The decode-step GEMM's K loop on MXFP4 weights is written once, in two pieces of text that gemm_skinny_w4_kernel
// (gemm_skinny_w4.hip) and moe_gemm_w4_kernel (moe_w4.hip, the grouped GEMM on MXFP4 expert weights) include inside their bodies, as
// the 16-bit and e4m3fn kernels include theirs: this set-up, and the loop (gemm_skinny_w4_loop.inc).  Text in two pieces for the
// reason gemm_skinny_w16_head.inc gives.
//
// This piece: the tile's constants, the x stage in LDS, the lane's coordinates, the slice of K, the weight rows and their block
// scale rows.  T (__bf16), MF, GLU and the launch's arguments `p` (x, w, wg, ldw, lds, N, K, steps, nsplit; lds the scale rows'
// stride in bytes) come from the including kernel, and so do
//   wbase()     bytes from p.w (and p.wg) to the weight this workgroup reads: 0, or expert * expert_stride
//   wscale()    that weight's e8m0 block scales (const uint8_t*): the launch's, or expert * the scales' expert stride behind them
//   wscale_g()  the gate weight's (read under GLU only)
// A kernel that leaves early (an expert without rows) does so in front of this piece: every thread that enters reaches every barrier.
  using X8 = typename DT<T>::x8;
  using Tile = SkinnyW4Tile<MF, GLU>;
  constexpr int SKC = Tile::SKC, D = Tile::D, PCS = Tile::PCS, ROWB = Tile::ROWB, XPT = Tile::XPT;
  __shared__ __attribute__((aligned(16))) char sx[2][Tile::ROWS * ROWB];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, q = lane >> 4;
  const int n0 = blockIdx.x * SKINNY_BN + wave * 16;
  const bool active = n0 < p.N;  // (a wave past the last column stages x and keeps the barriers, nothing else)
  const int s = blockIdx.y;
  int kb, ke;
  skinny_slice_range(p.steps, p.nsplit, SKINNY_W4_KSTEP, p.K, s, kb, ke);
  const int nc = (ke - kb + SKC - 1) / SKC;

  const int nrow = min(n0 + c, p.N - 1);
  const int64_t woff = wbase() + (int64_t)nrow * p.ldw;
  const uint8_t* wrow = (const uint8_t*)p.w + woff;
  const uint8_t* grow = GLU ? (const uint8_t*)p.wg + woff : nullptr;
  // the row's scale bytes: byte k / 32 is the block at k.  kb is a multiple of 128 and a chunk of 256, so the two bytes of lane
  // group q in a chunk start at an even byte of a row that starts on a dword (lds % 4 == 0, 4-byte aligned base and expert stride)
  const uint8_t* srow = wscale() + (int64_t)nrow * p.lds;
  const uint8_t* sgrow = GLU ? wscale_g() + (int64_t)nrow * p.lds : nullptr;
  const T* xg = (const T*)p.x;

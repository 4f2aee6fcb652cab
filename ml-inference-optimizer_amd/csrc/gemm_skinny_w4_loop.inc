// The K loop of the decode-step GEMM on MXFP4 weights, included behind gemm_skinny_w4_head.inc.  In a chunk of 256 k lane (c, q)
// owns the 64 k at 64 q of its weight row: two MX blocks.  Load t (0, 1) is the 16 bytes of block t, 32 e2m1 elements at k0 =
// chunk + 64 q + 32 t, and one 2-byte load fetches the two blocks' e8m0 scale bytes.  Dword j (0 .. 3) of a load holds the
// elements k0 + 8 j .. + 7, low nibble first: four v_cvt_scalef32_pk_bf16_fp4, one per byte, widen them to bf16 with the block's
// scale 2^(b - 127) applied in the conversion (the fp32 operand b << 23), exactly for 2 <= b <= 252, and they are the lane's 8 A
// elements of one MFMA.  Its B operand is the same true k of x: the 16-byte piece 8 q + 4 t + j of the chunk's row c, read from
// LDS.  (An MFMA sums over the 32 (lane group, element) slots; which k sits in a slot is free as long as A and B agree.)  The x
// rows of a chunk are staged once per workgroup through LDS, piece p of row r at p ^ (r & 15).
// No padding reaches a product: a block at k >= ke is not loaded, its bytes are 0x00 (+0) and its scale is 1.0 whatever byte
// the scale load brought along (a 0xff there would make the zeros NaN), and the x pieces at k >= ke are zeros.
// What varies between the including kernels is the rows description, which they define between the two pieces, under the
// contract of gemm_skinny_w16_loop.inc (nf, all_live, xhas, xrow).
// The loop leaves the slice's sums behind for skinny_write: acc, accg (lane (c, q): rows 16 mf + c, columns n0 + 4 q .. + 3).
  constexpr int GW = GLU ? 2 : 1;
  auto load_w = [&](u32x4_t (&wr)[2], u32x4_t (&gr)[GW], uint32_t& sr, uint32_t& sgr, int ch) {
    const int k = kb + ch * SKC + 64 * q;
    sr = 0x7f7fu;  // (both bytes 127: 1.0)
    if constexpr (GLU) sgr = 0x7f7fu;
    if (active && k < ke) {
      sr = *(const uint16_t*)(srow + (k >> 5));
      if constexpr (GLU) sgr = *(const uint16_t*)(sgrow + (k >> 5));
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int kt = k + 32 * t;
      const bool ok = active && kt < ke;
      wr[t] = (u32x4_t){0u, 0u, 0u, 0u};
      if (ok) wr[t] = *(const u32x4_t*)(wrow + (kt >> 1));
      if constexpr (GLU) {
        gr[t] = (u32x4_t){0u, 0u, 0u, 0u};
        if (ok) gr[t] = *(const u32x4_t*)(grow + (kt >> 1));
      }
      if (!ok) {  // the byte of a block that is not loaded is its neighbour's or padding: 1.0 in its place
        sr = (sr & ~(0xffu << (8 * t))) | (0x7fu << (8 * t));
        if constexpr (GLU) sgr = (sgr & ~(0xffu << (8 * t))) | (0x7fu << (8 * t));
      }
    }
  };
  auto load_x = [&](u32x4_t (&v)[XPT], int ch) {
#pragma unroll
    for (int i = 0; i < XPT; ++i) {
      const int idx = tid + i * 256, row = idx / PCS, pc = idx % PCS;
      const int k = kb + ch * SKC + pc * 8;
      v[i] = (u32x4_t){0u, 0u, 0u, 0u};
      if (xhas(i, row) && k < ke) v[i] = *(const u32x4_t*)(xg + (int64_t)xrow(i, row) * p.ldx + k);
    }
  };
  auto put_x = [&](const u32x4_t (&v)[XPT], int buf) {
#pragma unroll
    for (int i = 0; i < XPT; ++i) {
      const int idx = tid + i * 256, row = idx / PCS, pc = idx % PCS;
      if (all_live || row < nf * 16) *(u32x4_t*)(sx[buf] + row * ROWB + ((pc ^ (row & 15)) * 16)) = v[i];
    }
  };
  // the 8 e2m1 elements of a dword as bf16, times the block scale
  auto widen = [](uint32_t w, float sc) {
    typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
    const bf16x2_t a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 0), b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 1),
                   cc = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 2), d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 3);
    return __builtin_bit_cast(X8, (u32x4_t){__builtin_bit_cast(uint32_t, a), __builtin_bit_cast(uint32_t, b),
                                            __builtin_bit_cast(uint32_t, cc), __builtin_bit_cast(uint32_t, d)});
  };

  f32x4_t acc[MF], accg[GLU ? MF : 1];
#pragma unroll
  for (int mf = 0; mf < MF; ++mf) {
    acc[mf] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    if constexpr (GLU) accg[mf] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  }
  auto compute = [&](const u32x4_t (&wr)[2], const u32x4_t (&gr)[GW], uint32_t sr, uint32_t sgr, int buf) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const float sc = __uint_as_float(((sr >> (8 * t)) & 0xffu) << 23);
      float scg = 0.f;
      if constexpr (GLU) scg = __uint_as_float(((sgr >> (8 * t)) & 0xffu) << 23);
#pragma unroll
      for (int j = 0; j < 4; ++j) {  // dword j of block t: k = chunk + 64 q + 32 t + 8 j, x piece 8 q + 4 t + j
        const X8 wf = widen(wr[t][j], sc);
        X8 gf;
        if constexpr (GLU) gf = widen(gr[t][j], scg);
#pragma unroll
        for (int mf = 0; mf < MF; ++mf) {
          if (mf < nf) {  // (workgroup-uniform)
            const X8 xf = __builtin_bit_cast(X8, *(const u32x4_t*)(sx[buf] + (mf * 16 + c) * ROWB + (((8 * q + 4 * t + j) ^ c) * 16)));
            acc[mf] = DT<T>::mfma16(wf, xf, acc[mf]);
            if constexpr (GLU) accg[mf] = DT<T>::mfma16(gf, xf, accg[mf]);
          }
        }
      }
    }
  };

  // A ring of D register sets, run as the e4m3fn loop runs its own (gemm_skinny_w8_loop.inc): chunk ch lives in set ch % D; its x
  // pieces, then its scale bytes and weight bytes are requested D - 1 chunks ahead, into the set the chunk before the current one
  // has just left, because the vector memory counter retires loads in issue order.  The x pieces are stored to LDS only when their
  // chunk is due.  One barrier per chunk: the x buffer written for chunk ch was last read for chunk ch - 2, before the barrier of
  // chunk ch - 1.
  u32x4_t wr[D][2], gr[D][GW], xr[D][XPT];
  uint32_t sr[D], sgr[D];
#pragma unroll
  for (int j = 0; j < D - 1; ++j)
    if (j < nc) {
      load_x(xr[j], j);
      load_w(wr[j], gr[j], sr[j], sgr[j], j);
    }
  for (int ch = 0; ch < nc; ch += D) {
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const int cur = ch + j;
      if (cur < nc) {  // (the same in every thread of the workgroup)
        put_x(xr[j], cur & 1);
        __syncthreads();
        if (cur + D - 1 < nc) {
          load_x(xr[(j + D - 1) % D], cur + D - 1);
          load_w(wr[(j + D - 1) % D], gr[(j + D - 1) % D], sr[(j + D - 1) % D], sgr[(j + D - 1) % D], cur + D - 1);
        }
        compute(wr[j], gr[j], sr[j], sgr[j], cur & 1);
      }
    }
  }

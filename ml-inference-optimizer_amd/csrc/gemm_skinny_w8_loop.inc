// The K loop of the decode-step GEMM on e4m3fn weights, included behind gemm_skinny_w8_head.inc.  Lane (c, q) loads the 16 bytes
// of its weight row at k0 + 16 q, k0 the begin of a 64-k step; that one load feeds two MFMAs: MFMA j takes bytes 8 j .. 8 j + 7,
// widened at scale 1 (kv8_to_x8), as the lane's 8 A elements and the 16-byte piece k0 / 8 + 2 q + j of x row c, read from LDS, as
// its B operand.  The x rows of a chunk are staged once per workgroup through LDS, piece p of row r at p ^ (r & 15).
// What varies between the including kernels is the rows description, which they define between the two pieces, under the
// contract of gemm_skinny_w16_loop.inc:
//   nf, all_live   row fragments of 16 that are live: only these are stored to LDS and multiplied.  Workgroup-uniform.  The dense
//                  GEMM's is the constant MF, which all_live = true says at compile time; an expert's is ceil(its rows / 16).
//   xhas(i, r)     whether a row of x lies behind staged row r (piece i of this thread's XPT pieces); where none does the stage
//                  holds zeros that are never read from memory
//   xrow(i, r)     which row of x that is
// The loop leaves the slice's sums behind for skinny_write: acc, accg (lane (c, q): rows 16 mf + c, columns n0 + 4 q .. + 3).
  auto load_w = [&](u32x4_t (&wr)[KS], u32x4_t (&gr)[GLU ? KS : 1], int ch) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int k = kb + ch * SKC + ks * SKINNY_W8_KSTEP + 16 * q;
      const bool ok = active && k < ke;
      wr[ks] = (u32x4_t){0u, 0u, 0u, 0u};
      if (ok) wr[ks] = *(const u32x4_t*)(wrow + k);
      if constexpr (GLU) {
        gr[ks] = (u32x4_t){0u, 0u, 0u, 0u};
        if (ok) gr[ks] = *(const u32x4_t*)(grow + k);
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

  f32x4_t acc[MF], accg[GLU ? MF : 1];
#pragma unroll
  for (int mf = 0; mf < MF; ++mf) {
    acc[mf] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    if constexpr (GLU) accg[mf] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  }
  auto compute = [&](const u32x4_t (&wr)[KS], const u32x4_t (&gr)[GLU ? KS : 1], int buf) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {  // bytes 8 j .. 8 j + 7 of the piece: k0 + 16 q + 8 j, x piece ks * 8 + 2 q + j
        const X8 wf = kv8_to_x8<T>((u32x2_t){wr[ks][2 * j], wr[ks][2 * j + 1]});
        X8 gf;
        if constexpr (GLU) gf = kv8_to_x8<T>((u32x2_t){gr[ks][2 * j], gr[ks][2 * j + 1]});
#pragma unroll
        for (int mf = 0; mf < MF; ++mf) {
          if (mf < nf) {  // (workgroup-uniform)
            const X8 xf = __builtin_bit_cast(X8, *(const u32x4_t*)(sx[buf] + (mf * 16 + c) * ROWB + (((ks * 8 + 2 * q + j) ^ c) * 16)));
            acc[mf] = DT<T>::mfma16(wf, xf, acc[mf]);
            if constexpr (GLU) accg[mf] = DT<T>::mfma16(gf, xf, accg[mf]);
          }
        }
      }
    }
  };

  // A ring of D register sets.  Chunk ch lives in set ch % D: its x pieces and then its weight bytes are requested D - 1 chunks
  // ahead, into the set the chunk before the current one has just left: the vector memory counter retires loads in issue order,
  // so waiting for an x load issued behind younger weight loads would drain the ring.  The x pieces are stored to LDS only when
  // their chunk is due.  One barrier per chunk: the x buffer written for chunk ch was last read for chunk ch - 2, before the
  // barrier of chunk ch - 1.
  u32x4_t wr[D][KS], gr[D][GLU ? KS : 1], xr[D][XPT];
#pragma unroll
  for (int j = 0; j < D - 1; ++j)
    if (j < nc) {
      load_x(xr[j], j);
      load_w(wr[j], gr[j], j);
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
          load_w(wr[(j + D - 1) % D], gr[(j + D - 1) % D], cur + D - 1);
        }
        compute(wr[j], gr[j], cur & 1);
      }
    }
  }

// Body of decode_rows_kernel, decode_rows_win_kernel (decode_paged.hip) and their fp8-cache forms decode_rows_kv8_kernel,
// decode_rows_kv8_win_kernel (decode_kv8.hip), included inside each: T, CPR, QN, the DecDev `p`, WIN, `wleft`, KV8 and the
// scale pointers `ksc`, `vsc` come from the including kernel.  KV8: 16 one-byte elements per 16-byte chunk, k_scale in the
// score scale, v_scale on the split's own output.
  constexpr int EPC = KV8 ? 16 : 8;  // elements per 16-byte chunk
  using KT = std::conditional_t<KV8, uint8_t, T>;  // a cached element
  constexpr int U = 2;  // token slots per batch (U = 4 measured the same within 2 %)
  __shared__ float s_st[4][64][QN][EPC + 2];  // per (wave, lane, query): o[EPC], m, l

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x, split = blockIdx.y;
  const int CPT = p.Hkv * CPR;
  const int npart = CPT >= 64 ? CPT / 64 : 1;
  const int tpl = CPT >= 64 ? 1 : 64 / CPT;             // tokens per wave-load
  const int part = wave % npart, tslot = wave / npart;  // this wave's slice of the row / token slot
  const int wpp = 4 / npart;                            // waves per part
  const int tl = CPT >= 64 ? 0 : lane / CPT;            // token inside the wave-load
  const int cidx = CPT >= 64 ? part * 64 + lane : lane % CPT;  // 16-byte chunk of the token row
  const int kvh = cidx / CPR, c = cidx % CPR;
  // the fp8 kernel has QN = 1 with the query indexing folded: H == Hkv and q_len == 1 (dec_rows_ok)
  const int rep = KV8 ? 1 : p.H / p.Hkv, q_len = KV8 ? 1 : p.q_len;
  const int ctx = p.cl[b];
  int begin = split * p.split_len;
  if constexpr (WIN) begin += dec_win_begin(ctx, p.q_len, wleft);
  int end = begin + p.split_len;
  if (end > ctx) end = ctx;

  float qf[QN][EPC];
#pragma unroll
  for (int j = 0; j < QN; ++j) {
    const float qs = KV8 ? p.scale * ksc[0] : p.scale;
    const int h = kvh * rep + j / q_len, qi = j % q_len;
    const T* qp = (const T*)p.q + b * p.qs_b + h * p.qs_h + (int64_t)qi * p.qs_s + EPC * c;
#pragma unroll
    for (int hh = 0; hh < EPC / 8; ++hh) {
      const typename DT<T>::x8 v = __builtin_bit_cast(typename DT<T>::x8, *(const u32x4_t*)(qp + 8 * hh));
#pragma unroll
      for (int i = 0; i < 8; ++i) qf[j][8 * hh + i] = (float)v[i] * qs;
    }
  }
  float m[QN], l[QN], o[QN][EPC];
#pragma unroll
  for (int j = 0; j < QN; ++j) {
    m[j] = -INFINITY;
    l[j] = 0.f;
#pragma unroll
    for (int i = 0; i < EPC; ++i) o[j][i] = 0.f;
  }

  const int64_t tok_stride = (int64_t)p.Hkv * p.D;
  const int64_t blk_stride = (int64_t)p.L * p.bs * tok_stride;
  const int64_t lay_off = (int64_t)p.layer * p.bs * tok_stride + (int64_t)cidx * EPC;
  const int32_t* btrow = p.bt + (int64_t)b * p.max_blocks;
  const int step = wpp * tpl;  // tokens the workgroup covers per slot
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
      kr[j] = *(const u32x4_t*)((const KT*)p.kc + off);
      vr[j] = *(const u32x4_t*)((const KT*)p.vc + off);
    }
  };
  auto reduce = [&](int pos0, const u32x4_t (&kr)[U], const u32x4_t (&vr)[U]) {
#pragma unroll
    for (int q = 0; q < QN; ++q) {
      float sc[U];
      float m_new = m[q];
#pragma unroll
      for (int j = 0; j < U; ++j) {
        float s = 0.f;
        dec_chunk_each<T, KV8>(kr[j], [&](int i, float k) { s += qf[q][i] * k; });
#pragma unroll
        for (int x = 1; x < CPR; x <<= 1) s += __shfl_xor(s, x, 64);
        const int pos = tok(pos0, j);
        sc[j] = (pos < end && pos / p.bs < p.max_blocks) ? s : -INFINITY;
        if constexpr (WIN) {
          if (pos < ctx - q_len + q % q_len - wleft) sc[j] = -INFINITY;
        }
        m_new = fmaxf(m_new, sc[j]);
      }
      const float m_ref = (m_new == -INFINITY) ? 0.f : m_new;
      const float alpha = __expf(m[q] - m_ref);
      l[q] *= alpha;
#pragma unroll
      for (int i = 0; i < EPC; ++i) o[q][i] *= alpha;
#pragma unroll
      for (int j = 0; j < U; ++j) {
        const float pe = __expf(sc[j] - m_ref);
        l[q] += pe;
        dec_chunk_each<T, KV8>(vr[j], [&](int i, float v) { o[q][i] += pe * v; });
      }
      m[q] = m_new;
    }
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
  // ---- merge the states of one (chunk of the row, query) held by several waves / token slots
#pragma unroll
  for (int q = 0; q < QN; ++q) {
#pragma unroll
    for (int i = 0; i < EPC; ++i) s_st[wave][lane][q][i] = o[q][i];
    s_st[wave][lane][q][EPC] = m[q];
    s_st[wave][lane][q][EPC + 1] = l[q];
  }
  __syncthreads();
  if (tslot == 0 && tl == 0) {  // one lane per chunk of the row: its own state first, then the others'
#pragma unroll
    for (int q = 0; q < QN; ++q) {
      float M = -INFINITY;
      for (int w = part; w < 4; w += npart)
        for (int t2 = 0; t2 < tpl; ++t2) M = fmaxf(M, s_st[w][(CPT >= 64 ? lane : t2 * CPT + cidx)][q][EPC]);
      float Ls = 0.f, acc[EPC];
#pragma unroll
      for (int i = 0; i < EPC; ++i) acc[i] = 0.f;
      if (M != -INFINITY) {
        for (int w = part; w < 4; w += npart)
          for (int t2 = 0; t2 < tpl; ++t2) {
            const float* st = s_st[w][(CPT >= 64 ? lane : t2 * CPT + cidx)][q];
            const float wgt = __expf(st[EPC] - M);
            Ls += st[EPC + 1] * wgt;
#pragma unroll
            for (int i = 0; i < EPC; ++i) acc[i] += st[i] * wgt;
          }
      }
      // empty context -> 0 (attention_kernels.py:802); KV8: v_scale on the split's own output
      const float inv = (Ls > 0.f) ? (KV8 ? vsc[0] : 1.f) / Ls : 0.f;
      const int h = kvh * rep + q / q_len, qi = q % q_len;
      const int64_t row = ((int64_t)b * p.H + h) * q_len + qi;
      if (p.nsplit == 1) {
        T* op = (T*)p.o + b * p.os_b + h * p.os_h + (int64_t)qi * p.os_s + EPC * c;
#pragma unroll
        for (int i = 0; i < EPC; ++i) op[i] = (T)(acc[i] * inv);
      } else {
        float* wo = p.ws_o + (row * p.nsplit + split) * p.D + EPC * c;
#pragma unroll
        for (int i = 0; i < EPC; ++i) wo[i] = acc[i] * inv;
        if (c == 0) p.ws_lse[row * p.nsplit + split] = (Ls > 0.f) ? M + __logf(Ls) : -INFINITY;
      }
    }
  }

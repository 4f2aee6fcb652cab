// Body of decode_rows_kernel and decode_rows_win_kernel (decode_paged.hip), included inside each: T, CPR, QN, the
// DecDev `p`, WIN and `wleft` come from the including kernel.
  constexpr int U = 2;  // token slots per batch (U = 4 measured the same within 2 %)
  __shared__ float s_st[4][64][QN][10];  // per (wave, lane, query): o[8], m, l

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
  const int rep = p.H / p.Hkv;
  const int ctx = p.cl[b];
  int begin = split * p.split_len;
  if constexpr (WIN) begin += dec_win_begin(ctx, p.q_len, wleft);
  int end = begin + p.split_len;
  if (end > ctx) end = ctx;

  float qf[QN][8];
#pragma unroll
  for (int j = 0; j < QN; ++j) {
    const int h = kvh * rep + j / p.q_len, qi = j % p.q_len;
    const u32x4_t raw = *(const u32x4_t*)((const T*)p.q + b * p.qs_b + h * p.qs_h + (int64_t)qi * p.qs_s + 8 * c);
    const typename DT<T>::x8 v = __builtin_bit_cast(typename DT<T>::x8, raw);
#pragma unroll
    for (int i = 0; i < 8; ++i) qf[j][i] = (float)v[i] * p.scale;
  }
  float m[QN], l[QN], o[QN][8];
#pragma unroll
  for (int j = 0; j < QN; ++j) {
    m[j] = -INFINITY;
    l[j] = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) o[j][i] = 0.f;
  }

  const int64_t tok_stride = (int64_t)p.Hkv * p.D;
  const int64_t blk_stride = (int64_t)p.L * p.bs * tok_stride;
  const int64_t lay_off = (int64_t)p.layer * p.bs * tok_stride + (int64_t)cidx * 8;
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
      kr[j] = *(const u32x4_t*)((const T*)p.kc + off);
      vr[j] = *(const u32x4_t*)((const T*)p.vc + off);
    }
  };
  auto reduce = [&](int pos0, const u32x4_t (&kr)[U], const u32x4_t (&vr)[U]) {
#pragma unroll
    for (int q = 0; q < QN; ++q) {
      float sc[U];
      float m_new = m[q];
#pragma unroll
      for (int j = 0; j < U; ++j) {
        const typename DT<T>::x8 kv = __builtin_bit_cast(typename DT<T>::x8, kr[j]);
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) s += qf[q][i] * (float)kv[i];
#pragma unroll
        for (int x = 1; x < CPR; x <<= 1) s += __shfl_xor(s, x, 64);
        const int pos = tok(pos0, j);
        sc[j] = (pos < end && pos / p.bs < p.max_blocks) ? s : -INFINITY;
        if constexpr (WIN) {
          if (pos < ctx - p.q_len + q % p.q_len - wleft) sc[j] = -INFINITY;
        }
        m_new = fmaxf(m_new, sc[j]);
      }
      const float m_ref = (m_new == -INFINITY) ? 0.f : m_new;
      const float alpha = __expf(m[q] - m_ref);
      l[q] *= alpha;
#pragma unroll
      for (int i = 0; i < 8; ++i) o[q][i] *= alpha;
#pragma unroll
      for (int j = 0; j < U; ++j) {
        const typename DT<T>::x8 vv = __builtin_bit_cast(typename DT<T>::x8, vr[j]);
        const float pe = __expf(sc[j] - m_ref);
        l[q] += pe;
#pragma unroll
        for (int i = 0; i < 8; ++i) o[q][i] += pe * (float)vv[i];
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
    for (int i = 0; i < 8; ++i) s_st[wave][lane][q][i] = o[q][i];
    s_st[wave][lane][q][8] = m[q];
    s_st[wave][lane][q][9] = l[q];
  }
  __syncthreads();
  if (tslot == 0 && tl == 0) {  // one lane per chunk of the row: its own state first, then the others'
#pragma unroll
    for (int q = 0; q < QN; ++q) {
      float M = -INFINITY;
      for (int w = part; w < 4; w += npart)
        for (int t2 = 0; t2 < tpl; ++t2) M = fmaxf(M, s_st[w][(CPT >= 64 ? lane : t2 * CPT + cidx)][q][8]);
      float Ls = 0.f, acc[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] = 0.f;
      if (M != -INFINITY) {
        for (int w = part; w < 4; w += npart)
          for (int t2 = 0; t2 < tpl; ++t2) {
            const float* st = s_st[w][(CPT >= 64 ? lane : t2 * CPT + cidx)][q];
            const float wgt = __expf(st[8] - M);
            Ls += st[9] * wgt;
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i] += st[i] * wgt;
          }
      }
      const float inv = (Ls > 0.f) ? 1.f / Ls : 0.f;  // empty context -> 0 (attention_kernels.py:802)
      const int h = kvh * rep + q / p.q_len, qi = q % p.q_len;
      const int64_t row = ((int64_t)b * p.H + h) * p.q_len + qi;
      if (p.nsplit == 1) {
        T* op = (T*)p.o + b * p.os_b + h * p.os_h + (int64_t)qi * p.os_s + 8 * c;
#pragma unroll
        for (int i = 0; i < 8; ++i) op[i] = (T)(acc[i] * inv);
      } else {
        float* wo = p.ws_o + (row * p.nsplit + split) * p.D + 8 * c;
#pragma unroll
        for (int i = 0; i < 8; ++i) wo[i] = acc[i] * inv;
        if (c == 0) p.ws_lse[row * p.nsplit + split] = (Ls > 0.f) ? M + __logf(Ls) : -INFINITY;
      }
    }
  }

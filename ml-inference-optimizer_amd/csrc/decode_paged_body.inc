// Body of decode_paged_kernel, decode_paged_win_kernel (decode_paged.hip) and their fp8-cache forms decode_paged_kv8_kernel,
// decode_paged_kv8_win_kernel (decode_kv8.hip), included inside each: T, CPRP, U, the DecDev `p`, WIN, `wleft`, KV8 and the
// scale pointers `ksc`, `vsc` come from the including kernel.  KV8: a cached element is one e4m3fn byte, so a lane's 16-byte
// chunk holds 16 elements instead of 8; k_scale joins the score scale and v_scale the split's own output (only the fp8
// kernels read ksc / vsc).
  constexpr int EPC = KV8 ? 16 : 8;  // elements per 16-byte chunk
  using KT = std::conditional_t<KV8, uint8_t, T>;  // a cached element
  constexpr int TPI = 64 / CPRP;  // tokens per wave-iteration
  constexpr int NSTATE = 4 * TPI;
  __shared__ float s_o[NSTATE][CPRP * EPC + 1];
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
  const bool c_ok = (EPC * c < p.D);

  float qf[EPC];
  {
    const float qs = KV8 ? p.scale * ksc[0] : p.scale;
    u32x4_t raw[EPC / 8] = {};
    if (c_ok) {
      const T* qp = (const T*)p.q + b * p.qs_b + h * p.qs_h + (int64_t)qi * p.qs_s + EPC * c;
#pragma unroll
      for (int hh = 0; hh < EPC / 8; ++hh) raw[hh] = *(const u32x4_t*)(qp + 8 * hh);
    }
#pragma unroll
    for (int hh = 0; hh < EPC / 8; ++hh) {
      const typename DT<T>::x8 v = __builtin_bit_cast(typename DT<T>::x8, raw[hh]);
#pragma unroll
      for (int i = 0; i < 8; ++i) qf[8 * hh + i] = (float)v[i] * qs;
    }
  }

  float m = -INFINITY, l = 0.f, o[EPC];
#pragma unroll
  for (int i = 0; i < EPC; ++i) o[i] = 0.f;

  const int64_t tok_stride = (int64_t)p.Hkv * p.D;
  const int64_t blk_stride = (int64_t)p.L * p.bs * tok_stride;

  // U wave-iterations (U * TPI tokens per wave) per batch, two batches in flight: the K/V rows of batch i+1 and the
  // block-table entries of batch i+2 are requested before batch i is reduced, and one max / rescale serves the U
  // tokens of a batch.  Measured (tools/dbg/dec_sweep.sh): U = 1 .. 4 are within 2 % of each other, U = 8 is 3-5 %
  // slower -- the kernel is bound by the 128-byte-pieces-at-token-stride access pattern (5.2-5.4 TB/s at B 64), not
  // by loads in flight.
  constexpr int STEP = 4 * TPI;  // tokens the workgroup's four waves cover per iteration
  // Loads are unconditional (addresses clamped to the split's last token / the row's first chunk, values masked in
  // `reduce`): predicated loads become branches, and hipcc drains vmcnt at every join, which serialises the batches.
  const int last = end - 1;  // >= begin here: empty splits skip the loop
  const int coff = c_ok ? EPC * c : 0;
  const int64_t lay_off = (int64_t)p.layer * p.bs * tok_stride + (int64_t)kvh * p.D + coff;
  const int32_t* btrow = p.bt + (int64_t)b * p.max_blocks;
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
      kr[j] = *(const u32x4_t*)((const KT*)p.kc + off);
      vr[j] = *(const u32x4_t*)((const KT*)p.vc + off);
    }
  };
  auto reduce = [&](int pos0, const u32x4_t (&kr)[U], const u32x4_t (&vr)[U]) {
    float sc[U];
    float m_new = m;
#pragma unroll
    for (int j = 0; j < U; ++j) {
      float s = 0.f;
      dec_chunk_each<T, KV8>(kr[j], [&](int i, float k) { s += qf[i] * k; });  // qf = 0 in the padding chunks (c_ok false)
#pragma unroll
      for (int x = 1; x < CPRP; x <<= 1) s += __shfl_xor(s, x, 64);
      const int pos = pos0 + j * STEP + t;
      sc[j] = (pos < end && pos / p.bs < p.max_blocks) ? s : -INFINITY;  // uniform within the token's lane group
      m_new = fmaxf(m_new, sc[j]);
    }
    const float m_ref = (m_new == -INFINITY) ? 0.f : m_new;  // nothing seen yet: every weight below is exp(-inf) = 0
    const float alpha = __expf(m - m_ref);
    l *= alpha;
#pragma unroll
    for (int i = 0; i < EPC; ++i) o[i] *= alpha;
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const float pe = __expf(sc[j] - m_ref);
      l += pe;
      dec_chunk_each<T, KV8>(vr[j], [&](int i, float v) { o[i] += pe * v; });
    }
    m = m_new;
  };
  {
    constexpr int BATCH = U * STEP;
    int pbA[U], pbB[U], pbC[U];  // block ids of the batch being reduced, the next one, and the one after
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

  // ---- merge the NSTATE per-(wave, token-slot) states
  const int g = wave * TPI + t;
#pragma unroll
  for (int i = 0; i < EPC; ++i) s_o[g][EPC * c + i] = o[i];
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
    // empty context -> 0 (attention_kernels.py:802); KV8: v_scale on the split's own output
    const float val = (Lsum > 0.f) ? (KV8 ? acc / Lsum * vsc[0] : acc / Lsum) : 0.f;
    if (p.nsplit == 1) {
      ((T*)p.o)[b * p.os_b + h * p.os_h + (int64_t)qi * p.os_s + tid] = (T)val;
    } else {
      p.ws_o[((int64_t)row * p.nsplit + split) * p.D + tid] = val;
      if (tid == 0) p.ws_lse[(int64_t)row * p.nsplit + split] = (Lsum > 0.f) ? M + __logf(Lsum) : -INFINITY;
    }
  }

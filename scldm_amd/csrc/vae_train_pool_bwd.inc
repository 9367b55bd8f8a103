// Body of wide::enc_pool_bwd_kernel / enc_pool_bwd_rows_kernel (vae_train_wide.hpp), included once per kernel with `ROWS` defined as a
// constexpr bool in the enclosing function; `a` is the kernel's EncPoolBwdArgs.
  extern __shared__ __attribute__((aligned(16))) float S[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, tk = lane >> 4, j = lane & 15;
  const int chunk = blockIdx.x, cell = blockIdx.y, nch = gridDim.x;
  constexpr float kS2 = 1.4426950408889634f * 0.35355339059327373f;   // log2(e) / sqrt(8)
  constexpr float kScale = 0.35355339059327373f;
  {
    RowCopy<64> cw;
    cw.load(a.wkv, 64, tid);
    cw.store(S + PB_W, tid);
    for (int idx = tid; idx < 512; idx += kThreads) {
      S[PB_Q + (idx >> 5) * kP + (idx & 31)] = a.Q[idx];
      S[PB_DAO + (idx >> 5) * kP + (idx & 31)] = a.dao[(size_t)cell * 512 + idx];
    }
    if (tid < 64) { S[PB_LSE + tid] = a.lse2[(size_t)cell * 64 + tid]; S[PB_DG + tid] = a.dgq[(size_t)cell * 64 + tid]; }
  }
  __syncthreads();
  float* __restrict__ Wv = S + PB_WAVE + wave * PW_SIZE;
  const float lw0 = a.ln1_w[j], lw1 = a.ln1_w[j + 16], lb0 = a.ln1_b[j], lb1 = a.ln1_b[j + 16];
  const int begin = chunk * a.tiles * 64, end = min(a.S, begin + a.tiles * 64);
  const int h = j >> 2, iq = j & 3;
  f32x4 gw[8];          // d c_attn[o = (lane >> 3) + 8 m][4 (lane & 7) ..]
  f32x4 gqa = z4(), gqb = z4();   // dQ[(head, query) = lane][d = 0 .. 7 of that head]
  float gln = 0.f;      // lanes < 32: LN_1 weight gradient of feature lane; lanes >= 32: bias gradient of feature lane - 32
#pragma unroll
  for (int m = 0; m < 8; ++m) gw[m] = z4();
  for (int s0 = begin + wave * 4; s0 < end; s0 += 16) {
    const int s = s0 + tk;
    const bool valid = s < end;
    const size_t si = (size_t)cell * a.S + (valid ? s : end - 1);
    const long long gene = a.genes[si];
    const float lc = log1pf(a.counts[si]);
    const float* e = a.emb + (size_t)gene * 32;
    const Ln n = ln_own(e[j] * lc, e[j + 16] * lc, a.eps);
    Wv[PW_XN + tk * kP + j] = fmaf(n.h0, lw0, lb0);
    Wv[PW_XN + tk * kP + j + 16] = fmaf(n.h1, lw1, lb1);
    tsync();
    lin32<64>(S + PB_W, Wv + PW_XN + tk * kP, j, [&](int, int o, float v) { Wv[PW_KV + tk * kP64 + o] = v; });
    tsync();
    {
      const f32x4 ka = *v4(Wv + PW_KV + tk * kP64 + 8 * h), kb = *v4(Wv + PW_KV + tk * kP64 + 8 * h + 4);
      const f32x4 va = *v4(Wv + PW_KV + tk * kP64 + 32 + 8 * h), vb = *v4(Wv + PW_KV + tk * kP64 + 32 + 8 * h + 4);
      f32x4 dka = z4(), dkb = z4(), dva = z4(), dvb = z4();
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = 4 * iq + q;
        const f32x4 qa = *v4(S + PB_Q + i * kP + 8 * h), qb = *v4(S + PB_Q + i * kP + 8 * h + 4);
        const f32x4 da = *v4(S + PB_DAO + i * kP + 8 * h), db = *v4(S + PB_DAO + i * kP + 8 * h + 4);
        const float sc = dot4(qa, ka) + dot4(qb, kb), dp = dot4(da, va) + dot4(db, vb);
        const float pp = valid ? __builtin_amdgcn_exp2f(sc * kS2 - S[PB_LSE + h * 16 + i]) : 0.f;
        const float ds = pp * (dp - S[PB_DG + h * 16 + i]) * kScale;
        Wv[PW_DSV + tk * kP64 + h * 16 + i] = ds;
        dka = fma4(ds, qa, dka); dkb = fma4(ds, qb, dkb);
        dva = fma4(pp, da, dva); dvb = fma4(pp, db, dvb);
      }
      dka = quad_sum4(dka); dkb = quad_sum4(dkb); dva = quad_sum4(dva); dvb = quad_sum4(dvb);
      const f32x4 mine = iq == 0 ? dka : iq == 1 ? dkb : iq == 2 ? dva : dvb;
      *v4(Wv + PW_DKV + tk * kP64 + (iq >> 1) * 32 + 8 * h + 4 * (iq & 1)) = mine;
    }
    tsync();
    {
      f32x4 acc = z4();
      lin32_t_acc<64>(S + PB_W, Wv + PW_DKV + tk * kP64, j, acc);
      acc = half_sum4(acc);
      if (j < 8) *v4(Wv + PW_TX + tk * kP + 4 * j) = acc;
    }
    {   // token-axis contractions over this wave's four tokens
      const int i4 = lane & 7, oo = lane >> 3, hq = lane >> 4;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const f32x4 xv = *v4(Wv + PW_XN + t * kP + 4 * i4);
#pragma unroll
        for (int m = 0; m < 8; ++m) gw[m] = fma4(Wv[PW_DKV + t * kP64 + oo + 8 * m], xv, gw[m]);
        const float ds = Wv[PW_DSV + t * kP64 + lane];
        gqa = fma4(ds, *v4(Wv + PW_KV + t * kP64 + 8 * hq), gqa);
        gqb = fma4(ds, *v4(Wv + PW_KV + t * kP64 + 8 * hq + 4), gqb);
      }
    }
    tsync();
    const float g0 = Wv[PW_TX + tk * kP + j], g1 = Wv[PW_TX + tk * kP + j + 16];
    Wv[PW_T1 + tk * kP + j] = g0 * n.h0;
    Wv[PW_T1 + tk * kP + j + 16] = g1 * n.h1;
    float o0, o1;
    ln_back(n, g0 * lw0, g1 * lw1, o0, o1);
    if constexpr (ROWS) {
      if (valid) {
        float* row = a.g_emb + ((size_t)cell * a.S + s) * 32;
        row[j] = lc != 0.f ? o0 * lc : 0.f;
        row[j + 16] = lc != 0.f ? o1 * lc : 0.f;
      }
    } else if (valid && lc != 0.f) {
      float* ge = a.g_emb + (size_t)gene * 32;
      atomicAdd(ge + j, o0 * lc);
      atomicAdd(ge + j + 16, o1 * lc);
    }
    tsync();
    {
      const float* src = (lane < 32 ? Wv + PW_T1 : Wv + PW_TX) + (lane & 31);
      gln += (src[0] + src[kP]) + (src[2 * kP] + src[3 * kP]);
    }
    tsync();
  }
  // the four waves' sums -> one partial
  __syncthreads();
  {
    float* R = S + wave * PB_ACC;
    const int i4 = lane & 7, oo = lane >> 3;
#pragma unroll
    for (int m = 0; m < 8; ++m) *v4(R + (oo + 8 * m) * 32 + 4 * i4) = gw[m];
    *v4(R + 2048 + lane * 8) = gqa;
    *v4(R + 2048 + lane * 8 + 4) = gqb;
    R[2560 + lane] = gln;
  }
  __syncthreads();
  float* P = a.part + (size_t)(cell * nch + chunk) * EP_SIZE;
  for (int idx = tid; idx < PB_ACC; idx += kThreads) {
    const float v = ((S[idx] + S[PB_ACC + idx]) + S[2 * PB_ACC + idx]) + S[3 * PB_ACC + idx];
    if (idx < 2048) P[EP_WKV + idx] = v;
    else if (idx < 2560) { const int e = idx - 2048, hi = e >> 3, dd = e & 7; P[EP_DQ + hi * 32 + 8 * (hi >> 4) + dd] = v; }
    else P[EP_LN1W + idx - 2560] = v;
  }

// Body of the per-gene decoder backward kernels of vae_train_wide.hpp (the header there explains the phases).  The including kernel
// defines: `a` (DecBwdArgs), F16, ROWS, GAUSS (the Gaussian head: see dec_gene_bwd_gauss_kernel) and hln_w / hln_b (GAUSS only),
// NB2 (the unshared-theta NB head: see dec_gene_bwd_nb2_kernel) and dl2 (NB2 only).
  extern __shared__ __attribute__((aligned(16))) float S[];
  const int tid = threadIdx.x, tok = tid >> 4, j = tid & 15, chunk = blockIdx.x, cell = blockIdx.y, nch = gridDim.x;
  const int wave = tid >> 6, li = tid & 15, g4 = (tid & 63) >> 4;      // MFMA roles: lane = (li, g4)
  constexpr float kScale = 0.35355339059327373f;   // 1 / sqrt(8)
  const int H = a.mlp.H;
  // GAUSS: the head vector of the rank-one part is ub = u - mean(u), u = head_w * ln_w (NB: head_w itself)
  float umean = 0.f;
  if constexpr (GAUSS) {
    for (int i = 0; i < 32; ++i) umean = fmaf(a.head_w[i], hln_w[i], umean);
    umean *= (1.0f / 32);
  }
  auto head_vec = [&](int i) { return a.head_w[i] * hln_w[i] - umean; };
  if constexpr (GAUSS) {
    RowCopy<96> cc;      // Wc^T, rows = hidden units (rows >= H zero)
    cc.load(a.mlp.wct, H, tid);
    cc.store(S + X_WC, tid);
    if (tid < 96) {      // c0[u] = sum_i Wc[i][u] ub[i]
      float s = 0.f;
      if (tid < H)
        for (int i = 0; i < 32; ++i) s = fmaf(a.mlp.wct[tid * 32 + i], head_vec(i), s);
      S[M_C0 + tid] = s;
    }
  }
  {
    RowCopy<32> cq, cp;
    RowCopy<96> c1, c2;
    cq.load(a.wq, 32, tid); cp.load(a.wp, 32, tid); c1.load(a.mlp.w1, H, tid); c2.load(a.mlp.w2, H, tid);
    cq.store(S + G_WQ, tid); cp.store(S + G_WP, tid); c1.store(S + G_W1, tid); c2.store(S + G_W2, tid);
    for (int idx = tid; idx < kT * 64; idx += kThreads) S[G_KV + (idx >> 6) * kP64 + (idx & 63)] = a.kv[(size_t)cell * (kT * 64) + idx];
    if (!GAUSS && tid < 96) {      // c0[u] = sum_i Wc[i][u] w_head[i]
      float s = 0.f;
      if (tid < H)
        for (int i = 0; i < 32; ++i) s = fmaf(a.mlp.wct[tid * 32 + i], a.head_w[i], s);
      S[M_C0 + tid] = s;
    }
    if constexpr (NB2) {
      if (tid < 96) {      // c1[u] = sum_i Wc[i][u] w_head[1][i]
        float s = 0.f;
        if (tid < H)
          for (int i = 0; i < 32; ++i) s = fmaf(a.mlp.wct[tid * 32 + i], a.head_w[32 + i], s);
        S[G_DB + tid] = s;      // (passes through the DB rows into registers, see below)
      }
      if (tid < 32) S[N_W1 + tid] = a.head_w[32 + tid];
    }
  }
  const float l1w0 = a.ln1q_w[j], l1w1 = a.ln1q_w[j + 16], l1b0 = a.ln1q_b[j], l1b1 = a.ln1q_b[j + 16];
  const float l2w0 = a.ln2_w[j], l2w1 = a.ln2_w[j + 16], l2b0 = a.ln2_b[j], l2b1 = a.ln2_b[j + 16];
  const float hw0 = GAUSS ? head_vec(j) : a.head_w[j], hw1 = GAUSS ? head_vec(j + 16) : a.head_w[j + 16];
  __syncthreads();
  // NB2: a lane reads only the c1 entries of its two hidden-unit tiles, so they live in registers (the DB rows are first written in
  // phase A, barriers later); the second gradient row and head row 1 sit behind the NB map (N_DL2, N_W1)
  float c1u[2] = {0.f, 0.f};
  if constexpr (NB2) {
#pragma unroll
    for (int q = 0; q < 2; ++q)
      if (wave + 4 * q < 6) c1u[q] = S[G_DB + 16 * (wave + 4 * q) + li];
  }
  f32x4 gw1[3] = {z4(), z4(), z4()}, gw2[3] = {z4(), z4(), z4()}, gq = z4(), gp = z4(), gk = z4(), gv = z4();
  // GAUSS: sum (beta xhat) (x) hid, tiles D[feature 16 (wave & 1) + 4 g4 + r][unit 16 ((wave >> 1) + 2 n) + li]; a | b of phase A;
  // alpha of this lane's gene; the running sum Q of g
  f32x4 gwc[3] = {z4(), z4(), z4()}, ga_[2] = {z4(), z4()}, gb_[2] = {z4(), z4()};
  float alpha = 0.f, qsum = 0.f;
  float cacc[2] = {0.f, 0.f};   // c[u] partials of this lane's gene quad, hidden-unit tiles wave, wave + 4
  float cacc1[2] = {0.f, 0.f};  // NB2: C1 = sum d1 hid likewise
  constexpr int NV = NB2 ? 12 : 10;
  float vs[NV];                 // running sums of this lane's gene slot: ln1q w|b, ln2 w|b, head (two features each); NB2: head row 1
#pragma unroll
  for (int i = 0; i < NV; ++i) vs[i] = 0.f;
  const int half = wave & 1, kh = wave >> 1;     // the small products' roles: (output half, k half)
  // x W^T with k along both images' rows: partial over input features 16 kh .. + 15 of output half `half`, D[gene 4 g4 + r][16 half + li]
  auto lin_partial = [&](int x_rows, int w_rows, int dst_rows) {
    const float* X = S + x_rows + li * kP + 16 * kh + 2 * g4;
    const float* W = S + w_rows + (16 * half + li) * kP + 16 * kh + 2 * g4;
    const f32x2 x0 = *v2(X), x1 = *v2(X + 8), w0 = *v2(W), w1 = *v2(W + 8);
    f32x4 acc = z4();
    if constexpr (F16) {
      acc = mfma16h(h4(x0[0], x0[1], x1[0], x1[1]), h4(w0[0], w0[1], w1[0], w1[1]), acc);
    } else {
      acc = mfma16(x0[0], w0[0], acc);
      acc = mfma16(x0[1], w0[1], acc);
      acc = mfma16(x1[0], w1[0], acc);
      acc = mfma16(x1[1], w1[1], acc);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) S[dst_rows + (4 * g4 + r) * kP + 16 * half + li] = acc[r];
  };
  // dy W with k along the weight image's rows: partial over output rows 16 kq .. + 15, D[gene 4 g4 + r][input 16 it + li]
  auto lin_t_partial = [&](int dy_rows, int w_rows, int it, int kq, f32x4& acc) {
    const f32x4 d = *v4(S + dy_rows + li * kP + 16 * kq + 4 * g4);
    const float* W = S + w_rows + (16 * kq + 4 * g4) * kP + 16 * it + li;
    if constexpr (F16) {
      acc = mfma16h(h4(d[0], d[1], d[2], d[3]), h4(W[0], W[kP], W[2 * kP], W[3 * kP]), acc);
    } else {
      acc = mfma16(d[0], W[0], acc);
      acc = mfma16(d[1], W[kP], acc);
      acc = mfma16(d[2], W[2 * kP], acc);
      acc = mfma16(d[3], W[3 * kP], acc);
    }
  };
  const int begin = chunk * a.tiles * 64, end = min(a.G, begin + a.tiles * 64);
#if SCLDM_VAE_PHASE_CLOCKS
  long long clk[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, last = __builtin_readcyclecounter();
#define PHASE_MARK(i) { const long long t_ = __builtin_readcyclecounter(); clk[i] += t_ - last; last = t_; }
#else
#define PHASE_MARK(i)
#endif
  // this step's gene id, d logit and embedding row were requested one step earlier (the id two steps earlier): S0 no longer waits
  // for two dependent global loads
  auto slot = [&](int g0) { return (size_t)cell * a.G + min(g0 + tok, end - 1); };
  // The cells of a batch list their genes in the same order, so workgroups of different cells reach the same genes' dE rows at the
  // same time and their atomics serialise in the L2.  Each cell therefore starts its walk over the chunk's steps at its own offset
  // (measured: the step's first phase 2 000 -> 1 650 cycles; without any atomics 1 250, 13.5 -> 13.2 ms per batch-512 step).
  const int nsteps = (end - begin + 15) / 16;
  const int rot = nsteps > 0 ? (int)(((unsigned)cell * 37u) % (unsigned)nsteps) : 0;
  auto first_gene = [&](int step) { return begin + 16 * ((step + rot) % nsteps); };
  long long gene_nx = 0, gene_n2 = 0;
  float dl_nx = 0.f, dl2_nx = 0.f, e0_nx = 0.f, e1_nx = 0.f;
  // F16: dl enters scaled by the cell's 2^e (so that the gradient operands sit in the fp16 range); every output leaves times 2^-e
  float dl_sc = 1.f;
  bool bad = false;     // F16: a non-finite value in this workgroup's outputs
  if constexpr (F16) dl_sc = a.dl_scale[cell];
  if (nsteps > 0) {
    const int ga = first_gene(0);
    gene_nx = a.genes[slot(ga)];
    gene_n2 = a.genes[slot(first_gene(1))];
    dl_nx = ga + tok < end ? a.dl[slot(ga)] : 0.f;
    if constexpr (F16) dl_nx *= dl_sc;
    if constexpr (NB2) {
      dl2_nx = ga + tok < end ? dl2[slot(ga)] : 0.f;
      if constexpr (F16) dl2_nx *= dl_sc;
    }
    e0_nx = a.emb[(size_t)gene_nx * 32 + j];
    e1_nx = a.emb[(size_t)gene_nx * 32 + j + 16];
  }
  for (int step = 0; step < nsteps; ++step) {
    const int g0 = first_gene(step), g1 = first_gene(step + 1);
    // ---- S0: embeddings, LN_1q
    const bool valid = g0 + tok < end;
    const long long gene = gene_nx;
    const float dlog = dl_nx, q00 = e0_nx, q01 = e1_nx;
    gene_nx = gene_n2;
    e0_nx = a.emb[(size_t)gene_nx * 32 + j];
    e1_nx = a.emb[(size_t)gene_nx * 32 + j + 16];
    dl_nx = g1 + tok < end ? a.dl[slot(g1)] : 0.f;
    if constexpr (F16) dl_nx *= dl_sc;
    gene_n2 = a.genes[slot(first_gene(step + 2))];
    if (!GAUSS && j == 0) S[M_DL + tok] = dlog;      // (GAUSS: dlog is g = d loss / d mu; M_DL gets alpha in phase H)
    if constexpr (NB2) {
      if (j == 1) S[N_DL2 + tok] = dl2_nx;      // (d1 of this step is read back from the row where it is needed: one register less)
      dl2_nx = g1 + tok < end ? dl2[slot(g1)] : 0.f;
      if constexpr (F16) dl2_nx *= dl_sc;
    }
    const Ln n1 = ln_own(q00, q01, a.eps);
    S[G_QN + tok * kP + j] = fmaf(n1.h0, l1w0, l1b0);
    S[G_QN + tok * kP + j + 16] = fmaf(n1.h1, l1w1, l1b1);
    __syncthreads();
    PHASE_MARK(0);
    // ---- S1: q partials -> QQ (k half 0), TX (k half 1)
    lin_partial(G_QN, G_WQ, kh ? G_TX : G_QQ);
    __syncthreads();
    PHASE_MARK(1);
    // ---- S2: attention on the matrix pipe, wave = head (16 genes x 16 keys x 8 head dims): scores = q_h K_h^T as two MFMAs (k pairs of
    // head dims as ds_read_b64; q = the two partials), softmax over the 16 lanes of a DPP row (lane = key), p -> PP rows (phase C's
    // operand anyway), ao_h = P V_h as four MFMAs whose useful output columns are the head's 8 dims
    float p[4];
    {
      const f32x2 q2 = *v2(S + G_QQ + li * kP + 8 * wave + 2 * g4) + *v2(S + G_TX + li * kP + 8 * wave + 2 * g4);
      const f32x2 k2 = *v2(S + G_KV + li * kP64 + 8 * wave + 2 * g4);
      f32x4 sc = z4();
      if constexpr (F16) {
        sc = mfma16h(h4(q2[0], q2[1], 0.f, 0.f), h4(k2[0], k2[1], 0.f, 0.f), sc);
      } else {
        sc = mfma16(q2[0], k2[0], sc);
        sc = mfma16(q2[1], k2[1], sc);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = sc[r] * kScale, e = __expf(v - row16_max(v));
        p[r] = e * (1.0f / row16_sum(e));
        S[G_PP + (4 * g4 + r) * kP64 + 16 * wave + li] = p[r];
      }
      tsync();     // (this wave wrote the PP columns it reads)
      f32x4 ao = z4();
      if constexpr (F16) {
        const f32x2 p0 = *v2(S + G_PP + li * kP64 + 16 * wave + 2 * g4), p1 = *v2(S + G_PP + li * kP64 + 16 * wave + 8 + 2 * g4);
        const float* V = S + G_KV + (2 * g4) * kP64 + 32 + 8 * wave + (li & 7);
        ao = mfma16h(h4(p0[0], p0[1], p1[0], p1[1]), h4(V[0], V[kP64], V[8 * kP64], V[9 * kP64]), ao);
      } else {
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          const f32x2 p2 = *v2(S + G_PP + li * kP64 + 16 * wave + 8 * m + 2 * g4);
          const float* V = S + G_KV + (8 * m + 2 * g4) * kP64 + 32 + 8 * wave + (li & 7);   // (lanes li, li + 8 share an address: no conflict)
          ao = mfma16(p2[0], V[0], ao);
          ao = mfma16(p2[1], V[kP64], ao);
        }
      }
      if (li < 8) {
#pragma unroll
        for (int r = 0; r < 4; ++r) S[G_AO + (4 * g4 + r) * kP + 8 * wave + li] = ao[r];
      }
    }
    __syncthreads();
    PHASE_MARK(2);
    // ---- S3: c_proj partials -> DY (k half 0), DAO (k half 1)
    lin_partial(G_AO, G_WP, kh ? G_DAO : G_DY);
    S[G_QQ + tok * kP + j] += S[G_TX + tok * kP + j];               // the whole q: dK's operand in phase C (its partials' last readers
    S[G_QQ + tok * kP + j + 16] += S[G_TX + tok * kP + j + 16];     // were S2's MFMAs; TX is next written in phase B)
    __syncthreads();
    PHASE_MARK(3);
    // ---- S4: residual, LN_2
    const float y0 = q00 + (S[G_DY + tok * kP + j] + S[G_DAO + tok * kP + j]);
    const float y1 = q01 + (S[G_DY + tok * kP + j + 16] + S[G_DAO + tok * kP + j + 16]);
    const Ln n2 = ln_own(y0, y1, a.eps);
    S[G_H2 + tok * kP + j] = fmaf(n2.h0, l2w0, l2b0);
    S[G_H2 + tok * kP + j + 16] = fmaf(n2.h1, l2w1, l2b1);
    __syncthreads();
    PHASE_MARK(4);
    // ---- phase A: a | b tiles D[gene 4 g4 + r][unit 16 ot + li], SwiGLU gradient in place
    {
      f32x2 hk[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) hk[s] = *v2(S + G_H2 + li * kP + 8 * s + 2 * g4);
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int ot = wave + 4 * q;
        if (ot < 6) {
          f32x4 aa = z4(), bb = z4();
          if constexpr (F16) {
            f16x8 xh, xa, xb;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
              const f32x2 wa = *v2(S + G_W1 + (16 * ot + li) * kP + 8 * s + 2 * g4), wb = *v2(S + G_W2 + (16 * ot + li) * kP + 8 * s + 2 * g4);
              xh[2 * s] = (_Float16)hk[s][0]; xh[2 * s + 1] = (_Float16)hk[s][1];
              xa[2 * s] = (_Float16)wa[0]; xa[2 * s + 1] = (_Float16)wa[1];
              xb[2 * s] = (_Float16)wb[0]; xb[2 * s + 1] = (_Float16)wb[1];
            }
            aa = mfma32h(xh, xa, aa);
            bb = mfma32h(xh, xb, bb);
          } else {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
              const f32x2 wa = *v2(S + G_W1 + (16 * ot + li) * kP + 8 * s + 2 * g4), wb = *v2(S + G_W2 + (16 * ot + li) * kP + 8 * s + 2 * g4);
              aa = mfma16(hk[s][0], wa[0], aa);
              bb = mfma16(hk[s][0], wb[0], bb);
              aa = mfma16(hk[s][1], wa[1], aa);
              bb = mfma16(hk[s][1], wb[1], bb);
            }
          }
          if constexpr (GAUSS) {     // a | b stay in registers (the SwiGLU gradient follows d hid in phase D); hid -> HID rows
            ga_[q] = aa;
            gb_[q] = bb;
#pragma unroll
            for (int r = 0; r < 4; ++r) S[X_HID + (4 * g4 + r) * kQ + 16 * ot + li] = aa[r] * sigm(aa[r]) * bb[r];
          } else if constexpr (NB2) {     // d hid = d0 c0 + d1 c1; C0 | C1 running sums
          const float c0u = S[M_C0 + 16 * ot + li];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int tk = 4 * g4 + r;
            const float dl = S[M_DL + tk], dk = S[N_DL2 + tk], sg = sigm(aa[r]), sa = aa[r] * sg, dh = fmaf(dl, c0u, dk * c1u[q]);
            const float hd = sa * bb[r];
            cacc[q] = fmaf(dl, hd, cacc[q]);
            cacc1[q] = fmaf(dk, hd, cacc1[q]);
            S[G_DA + tk * kQ + 16 * ot + li] = dh * bb[r] * (sg * (1.0f + aa[r] * (1.0f - sg)));
            S[G_DB + tk * kQ + 16 * ot + li] = dh * sa;
          }
          } else {
          const float c0u = S[M_C0 + 16 * ot + li];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int tk = 4 * g4 + r;
            const float dl = S[M_DL + tk], sg = sigm(aa[r]), sa = aa[r] * sg, dh = dl * c0u;
            cacc[q] = fmaf(dl, sa * bb[r], cacc[q]);
            S[G_DA + tk * kQ + 16 * ot + li] = dh * bb[r] * (sg * (1.0f + aa[r] * (1.0f - sg)));
            S[G_DB + tk * kQ + 16 * ot + li] = dh * sa;
          }
          }
        }
      }
    }
    __syncthreads();
    PHASE_MARK(5);
    if constexpr (GAUSS) {
      // ---- phase M: mlp = Wc hid partials, wave = (feature half, unit slices 3 kh .. 3 kh + 2) -> DY (kh 0), DAO (kh 1): both rows'
      // last readers were S4's y partials, their next writers are S5 / S6
      {
        f32x4 acc = z4(), acc2 = z4();
#pragma unroll
        for (int sq = 3 * kh; sq < 3 * kh + 3; ++sq) {
          const f32x4 d = *v4(S + X_HID + li * kQ + 16 * sq + 4 * g4);
          const float* W = S + X_WC + (16 * sq + 4 * g4) * kP + 16 * half + li;
          acc = mfma16(d[0], W[0], acc);
          acc2 = mfma16(d[1], W[kP], acc2);
          acc = mfma16(d[2], W[2 * kP], acc);
          acc2 = mfma16(d[3], W[3 * kP], acc2);
        }
        acc += acc2;
        float* Pt = S + (kh ? G_DAO : G_DY);
#pragma unroll
        for (int r = 0; r < 4; ++r) Pt[(4 * g4 + r) * kP + 16 * half + li] = acc[r];
      }
      __syncthreads();
      // ---- phase H: the head's LayerNorm of this lane's gene (features j, j + 16): alpha, beta xhat -> XB rows, running P (vs[8], vs[9]), Q
      {
        const float yo0 = y0 + (S[G_DY + tok * kP + j] + S[G_DAO + tok * kP + j]);
        const float yo1 = y1 + (S[G_DY + tok * kP + j + 16] + S[G_DAO + tok * kP + j + 16]);
        const Ln nh = ln_own(yo0, yo1, a.eps);
        const float sm = row16_sum(fmaf(hw0, nh.h0, hw1 * nh.h1)) * (1.0f / 32);
        alpha = dlog * nh.r;
        const float beta = -alpha * sm;
        S[X_XB + tok * kP + j] = beta * nh.h0;
        S[X_XB + tok * kP + j + 16] = beta * nh.h1;
        if (j == 0) S[M_DL + tok] = alpha;
        vs[8] = fmaf(dlog, nh.h0, vs[8]);
        vs[9] = fmaf(dlog, nh.h1, vs[9]);
        qsum += dlog;
      }
      __syncthreads();
      // ---- phase D: d hid = alpha c0 + Wc^T (beta xhat) as phase A's tiles D[gene 4 g4 + r][unit 16 ot + li], SwiGLU gradient -> DA, DB
      {
        f32x2 xk[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) xk[s] = *v2(S + X_XB + li * kP + 8 * s + 2 * g4);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const int ot = wave + 4 * q;
          if (ot < 6) {
            f32x4 t = z4();
#pragma unroll
            for (int s = 0; s < 4; ++s) {
              const f32x2 wc = *v2(S + X_WC + (16 * ot + li) * kP + 8 * s + 2 * g4);
              t = mfma16(xk[s][0], wc[0], t);
              t = mfma16(xk[s][1], wc[1], t);
            }
            const float c0u = S[M_C0 + 16 * ot + li];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int tk = 4 * g4 + r;
              const float aa = ga_[q][r], bb = gb_[q][r];
              const float al = S[M_DL + tk], sg = sigm(aa), sa = aa * sg, dh = fmaf(al, c0u, t[r]);
              cacc[q] = fmaf(al, sa * bb, cacc[q]);
              S[G_DA + tk * kQ + 16 * ot + li] = dh * bb * (sg * (1.0f + aa * (1.0f - sg)));
              S[G_DB + tk * kQ + 16 * ot + li] = dh * sa;
            }
          }
        }
      }
      __syncthreads();
    }
    // ---- phase B: d h2 partials, wave = (feature half, matrix); W1's go to the TX rows, W2's to the DQQ rows (free until S7)
    {
      const float* Wm = S + (kh ? G_W2 : G_W1);
      const float* Dm = S + (kh ? G_DB : G_DA);
      f32x4 acc = z4(), acc2 = z4();
      if constexpr (F16) {
#pragma unroll
        for (int sp = 0; sp < 3; ++sp) {     // two 16-unit k slices per 16 x 16 x 32 MFMA
          f16x8 xd, xw;
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            const int sq = 2 * sp + u;
            const f32x4 d = *v4(Dm + li * kQ + 16 * sq + 4 * g4);
            const float* W = Wm + (16 * sq + 4 * g4) * kP + 16 * half + li;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              xd[4 * u + i] = (_Float16)d[i];
              xw[4 * u + i] = (_Float16)W[i * kP];
            }
          }
          acc = mfma32h(xd, xw, acc);
        }
      } else {
#pragma unroll
        for (int sq = 0; sq < 6; ++sq) {
          const f32x4 d = *v4(Dm + li * kQ + 16 * sq + 4 * g4);
          const float* W = Wm + (16 * sq + 4 * g4) * kP + 16 * half + li;
          acc = mfma16(d[0], W[0], acc);
          acc2 = mfma16(d[1], W[kP], acc2);
          acc = mfma16(d[2], W[2 * kP], acc);
          acc2 = mfma16(d[3], W[3 * kP], acc2);
        }
        acc += acc2;
      }
      float* Pt = S + (kh ? G_DQQ : G_TX);
#pragma unroll
      for (int r = 0; r < 4; ++r) Pt[(4 * g4 + r) * kP + 16 * half + li] = acc[r];
    }
    __syncthreads();
    PHASE_MARK(6);
    // ---- S5: LN_2 backward -> d y
    float d0, d1;
    {
      const float t0 = S[G_TX + tok * kP + j] + S[G_DQQ + tok * kP + j], t1 = S[G_TX + tok * kP + j + 16] + S[G_DQQ + tok * kP + j + 16];
      vs[4] = fmaf(t0, n2.h0, vs[4]); vs[5] = fmaf(t1, n2.h1, vs[5]); vs[6] += t0; vs[7] += t1;
      if constexpr (!GAUSS) { vs[8] = fmaf(dlog, y0, vs[8]); vs[9] = fmaf(dlog, y1, vs[9]); }
      ln_back(n2, t0 * l2w0, t1 * l2w1, d0, d1);
      if constexpr (GAUSS) {     // the residual path: d yo = alpha ub + beta xhat
        d0 += fmaf(alpha, hw0, S[X_XB + tok * kP + j]);
        d1 += fmaf(alpha, hw1, S[X_XB + tok * kP + j + 16]);
      } else {
      d0 = fmaf(dlog, hw0, d0);
      d1 = fmaf(dlog, hw1, d1);
      }
      if constexpr (NB2) {     // head row 1: d yo = d0 w0 + d1 w1, and its running sums
        const float dlog1 = S[N_DL2 + tok];
        vs[NV - 2] = fmaf(dlog1, y0, vs[NV - 2]); vs[NV - 1] = fmaf(dlog1, y1, vs[NV - 1]);
        d0 = fmaf(dlog1, S[N_W1 + j], d0);
        d1 = fmaf(dlog1, S[N_W1 + j + 16], d1);
      }
    }
    S[G_DY + tok * kP + j] = d0;
    S[G_DY + tok * kP + j + 16] = d1;
    __syncthreads();
    PHASE_MARK(7);
    // ---- S6: d ao = Wp^T d y (waves 0, 1: one input half each, all 32 rows - S7's MFMAs read the whole row, and no row set is free
    // for a finalised sum of two partials)
    if (wave < 2) {
      f32x4 acc = z4(), acc2 = z4();
      lin_t_partial(G_DY, G_WP, wave, 0, acc);
      lin_t_partial(G_DY, G_WP, wave, 1, acc2);
      acc += acc2;
#pragma unroll
      for (int r = 0; r < 4; ++r) S[G_DAO + (4 * g4 + r) * kP + 16 * wave + li] = acc[r];
    }
    __syncthreads();
    PHASE_MARK(8);
    // ---- S7: attention backward, wave = head: d p = d ao_h V_h^T (two MFMAs), d s = p (d p - sum_keys p d p) / sqrt(8) in the lanes
    // that hold p, -> DS rows (phase C's operand), d q_h = d S K_h (four MFMAs, 8 useful columns)
    {
      const f32x2 a2 = *v2(S + G_DAO + li * kP + 8 * wave + 2 * g4);
      const f32x2 v2v = *v2(S + G_KV + li * kP64 + 32 + 8 * wave + 2 * g4);
      f32x4 dp = z4();
      if constexpr (F16) {
        dp = mfma16h(h4(a2[0], a2[1], 0.f, 0.f), h4(v2v[0], v2v[1], 0.f, 0.f), dp);
      } else {
        dp = mfma16(a2[0], v2v[0], dp);
        dp = mfma16(a2[1], v2v[1], dp);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float dg = row16_sum(p[r] * dp[r]);
        S[G_DS + (4 * g4 + r) * kP64 + 16 * wave + li] = p[r] * (dp[r] - dg) * kScale;
      }
      tsync();
      f32x4 dq = z4();
      if constexpr (F16) {
        const f32x2 d0 = *v2(S + G_DS + li * kP64 + 16 * wave + 2 * g4), d1 = *v2(S + G_DS + li * kP64 + 16 * wave + 8 + 2 * g4);
        const float* K = S + G_KV + (2 * g4) * kP64 + 8 * wave + (li & 7);
        dq = mfma16h(h4(d0[0], d0[1], d1[0], d1[1]), h4(K[0], K[kP64], K[8 * kP64], K[9 * kP64]), dq);
      } else {
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          const f32x2 d2 = *v2(S + G_DS + li * kP64 + 16 * wave + 8 * m + 2 * g4);
          const float* K = S + G_KV + (8 * m + 2 * g4) * kP64 + 8 * wave + (li & 7);
          dq = mfma16(d2[0], K[0], dq);
          dq = mfma16(d2[1], K[kP64], dq);
        }
      }
      if (li < 8) {
#pragma unroll
        for (int r = 0; r < 4; ++r) S[G_DQQ + (4 * g4 + r) * kP + 8 * wave + li] = dq[r];
      }
    }
    __syncthreads();
    PHASE_MARK(9);
    // ---- S8: d qn = Wq^T d q (waves 0, 1: one input half each, all 32 rows) -> TX; then phase C on every wave
    if (wave < 2) {
      f32x4 acc = z4(), acc2 = z4();
      lin_t_partial(G_DQQ, G_WQ, wave, 0, acc);
      lin_t_partial(G_DQQ, G_WQ, wave, 1, acc2);
      acc += acc2;
#pragma unroll
      for (int r = 0; r < 4; ++r) S[G_TX + (4 * g4 + r) * kP + 16 * wave + li] = acc[r];
    }
    // ---- phase C: weight gradients, D[out 16 ot + 4 g4 + r][in 16 it + li] += sum_genes dy[gene][out] x[gene][in]
    // (d W1 | d W2 could run in phase B already - measured: B + 1 270 cycles, C - 890: the matrix pipe is shared with the CU's other workgroup)
    if constexpr (F16) {   // (the four genes 4 g4 .. + 3 of a lane are the k of one 16 x 16 x 16 MFMA)
      auto col4 = [&](int base, int ld) {
        const float* p = S + base + 4 * g4 * ld;
        return h4(p[0], p[ld], p[2 * ld], p[3 * ld]);
      };
#pragma unroll
      for (int n = 0; n < 3; ++n) {
        const int idx = wave + 4 * n, ot = idx >> 1, it = idx & 1;
        const f16x4 x = col4(G_H2 + 16 * it + li, kP);
        gw1[n] = mfma16h(col4(G_DA + 16 * ot + li, kQ), x, gw1[n]);
        gw2[n] = mfma16h(col4(G_DB + 16 * ot + li, kQ), x, gw2[n]);
      }
      const int ot = wave >> 1, it = wave & 1;
      gq = mfma16h(col4(G_DQQ + 16 * ot + li, kP), col4(G_QN + 16 * it + li, kP), gq);
      gp = mfma16h(col4(G_DY + 16 * ot + li, kP), col4(G_AO + 16 * it + li, kP), gp);
      gk = mfma16h(col4(G_DS + wave * 16 + li, kP64), col4(G_QQ + 16 * (wave >> 1) + li, kP), gk);
      gv = mfma16h(col4(G_PP + wave * 16 + li, kP64), col4(G_DAO + 16 * (wave >> 1) + li, kP), gv);
    } else {
#pragma unroll
      for (int n = 0; n < 3; ++n) {
        const int idx = wave + 4 * n, ot = idx >> 1, it = idx & 1;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int tk = s + 4 * g4;       // (k slot <-> gene: rows 4 apart = 16 banks apart within a 32-lane group: conflict-free)
          const float x = S[G_H2 + tk * kP + 16 * it + li];
          gw1[n] = mfma16(S[G_DA + tk * kQ + 16 * ot + li], x, gw1[n]);
          gw2[n] = mfma16(S[G_DB + tk * kQ + 16 * ot + li], x, gw2[n]);
        }
      }
      const int ot = wave >> 1, it = wave & 1;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int tk = s + 4 * g4;
        gq = mfma16(S[G_DQQ + tk * kP + 16 * ot + li], S[G_QN + tk * kP + 16 * it + li], gq);
        gp = mfma16(S[G_DY + tk * kP + 16 * ot + li], S[G_AO + tk * kP + 16 * it + li], gp);
        // head `wave` of the cell's keys: D[key 4 g4 + r][column 16 (wave >> 1) + li], useful where (li >> 3) == (wave & 1)
        gk = mfma16(S[G_DS + tk * kP64 + wave * 16 + li], S[G_QQ + tk * kP + 16 * (wave >> 1) + li], gk);
        gv = mfma16(S[G_PP + tk * kP64 + wave * 16 + li], S[G_DAO + tk * kP + 16 * (wave >> 1) + li], gv);
      }
    }
    if constexpr (GAUSS) {     // the rank-two part of d Wc: D[feature 16 half + 4 g4 + r][unit 16 it + li] += sum_genes XB[gene][feature] hid[gene][unit]
#pragma unroll
      for (int n = 0; n < 3; ++n) {
        const int it = kh + 2 * n;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int tk = s + 4 * g4;
          gwc[n] = mfma16(S[X_XB + tk * kP + 16 * half + li], S[X_HID + tk * kQ + 16 * it + li], gwc[n]);
        }
      }
    }
    __syncthreads();
    PHASE_MARK(10);
    // ---- S9: LN_1q backward, dE[gene] (runs into the next step's S0: neither touches a row the other does)
    {
      const float t0 = S[G_TX + tok * kP + j], t1 = S[G_TX + tok * kP + j + 16];
      vs[0] = fmaf(t0, n1.h0, vs[0]); vs[1] = fmaf(t1, n1.h1, vs[1]); vs[2] += t0; vs[3] += t1;
      float o0, o1;
      ln_back(n1, t0 * l1w0, t1 * l1w1, o0, o1);
      // (a gene whose gradients are zero adds nothing; NB2: the d1 row is next written by this wave's own S0, after this read)
      const bool live = NB2 ? (dlog != 0.f || S[N_DL2 + tok] != 0.f) : dlog != 0.f;
      if constexpr (ROWS) {
        if (valid) {
          float v0 = 0.f, v1 = 0.f;
          if (live) {
            v0 = d0 + o0;
            v1 = d1 + o1;
            if constexpr (F16) {
              v0 *= 1.0f / dl_sc;
              v1 *= 1.0f / dl_sc;
              bad |= !(__builtin_isfinite(v0) && __builtin_isfinite(v1));
            }
          }
          float* row = a.g_emb + ((size_t)cell * a.G + g0 + tok) * 32;
          row[j] = v0;
          row[j + 16] = v1;
        }
      } else if (valid && live) {
        float* ge = a.g_emb + (size_t)gene * 32;
        float v0 = d0 + o0, v1 = d1 + o1;
        if constexpr (F16) {
          v0 *= 1.0f / dl_sc;
          v1 *= 1.0f / dl_sc;
          bad |= !(__builtin_isfinite(v0) && __builtin_isfinite(v1));
        }
        atomicAdd(ge + j, v0);
        atomicAdd(ge + j + 16, v1);
      }
    }
    PHASE_MARK(11);
  }
#if SCLDM_VAE_PHASE_CLOCKS
  if (blockIdx.x == 0 && blockIdx.y == 3 && tid == 0)
    printf("phase clocks (S0 S1 S2 S3 S4 A B S5 S6 S7 S8+C S9): %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld steps %d\n", clk[0], clk[1], clk[2],
           clk[3], clk[4], clk[5], clk[6], clk[7], clk[8], clk[9], clk[10], clk[11], nsteps);
#endif
#undef PHASE_MARK
  __syncthreads();
  if constexpr (F16) {     // back to the unscaled gradient (exact: a power of two), and the overflow check of what leaves
    const float inv = 1.0f / dl_sc;
    auto fix = [&](f32x4& v) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        v[r] *= inv;
        bad |= !__builtin_isfinite(v[r]);
      }
    };
#pragma unroll
    for (int n = 0; n < 3; ++n) { fix(gw1[n]); fix(gw2[n]); }
    fix(gq); fix(gp); fix(gk); fix(gv);
#pragma unroll
    for (int i = 0; i < NV; ++i) vs[i] *= inv;
#pragma unroll
    for (int q = 0; q < 2; ++q) cacc[q] *= inv;
    if constexpr (NB2) {
      cacc1[0] *= inv; cacc1[1] *= inv;
    }
  }
  // ---- one partial per workgroup (as dec_gene_bwd_mfma_kernel)
  float* P = a.part + (size_t)(cell * nch + chunk) * (GAUSS ? GP_SIZE : NB2 ? NP_SIZE : DP_SIZE);
  {
#pragma unroll
    for (int n = 0; n < 3; ++n) {
      const int idx = wave + 4 * n, ot = idx >> 1, it = idx & 1;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        P[DP_W1 + (16 * ot + 4 * g4 + r) * 32 + 16 * it + li] = gw1[n][r];
        P[DP_W2 + (16 * ot + 4 * g4 + r) * 32 + 16 * it + li] = gw2[n][r];
      }
    }
    const int ot = wave >> 1, it = wave & 1;
    float* DK = a.dkv_part + (size_t)(cell * nch + chunk) * (kT * 64);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      P[DP_WQ + (16 * ot + 4 * g4 + r) * 32 + 16 * it + li] = gq[r];
      P[DP_WP + (16 * ot + 4 * g4 + r) * 32 + 16 * it + li] = gp[r];
      if ((li >> 3) == (wave & 1)) {
        DK[(4 * g4 + r) * 64 + 16 * (wave >> 1) + li] = gk[r];
        DK[(4 * g4 + r) * 64 + 32 + 16 * (wave >> 1) + li] = gv[r];
      }
    }
  }
  float* R = S;
  float* RC = S + 16 * NV * 16;
#pragma unroll
  for (int i = 0; i < NV; ++i) R[(tok * NV + i) * 16 + j] = vs[i];
#pragma unroll
  for (int q = 0; q < 2; ++q)
    if (wave + 4 * q < 6) RC[g4 * 96 + 16 * (wave + 4 * q) + li] = cacc[q];
  float* RQ = RC + 4 * 96;      // GAUSS: Q of the 16 gene slots
  if constexpr (GAUSS) {
    if (j == 0) RQ[tok] = qsum;
  }
  float* RC1 = RC + 4 * 96;     // NB2: C1 partials, then the four waves' partial bias sums
  float* RB = RC1 + 4 * 96;
  if constexpr (NB2) {
#pragma unroll
    for (int q = 0; q < 2; ++q)
      if (wave + 4 * q < 6) RC1[g4 * 96 + 16 * (wave + 4 * q) + li] = cacc1[q];
    // d b_k = sum over the chunk's slots of d_k as the head pass wrote them (unscaled under F16): one more pass over values the
    // L2 still holds, instead of two more registers across the gene loop
    float b0 = 0.f, b1 = 0.f;
    for (int g = begin + tid; g < end; g += kThreads) {
      b0 += a.dl[(size_t)cell * a.G + g];
      b1 += dl2[(size_t)cell * a.G + g];
    }
    b0 = wave_sum(b0);
    b1 = wave_sum(b1);
    if ((tid & 63) == 0) { RB[wave] = b0; RB[4 + wave] = b1; }
  }
  __syncthreads();
  float sum = 0.f;
  const int vi = tid >> 4;
  if (vi < NV) {
#pragma unroll
    for (int t = 0; t < kT; ++t) sum += R[(t * NV + vi) * 16 + j];
  }
  float cu = 0.f;
  if (tid < 96) cu = (RC[tid] + RC[96 + tid]) + (RC[192 + tid] + RC[288 + tid]);
  float cu1 = 0.f;
  if constexpr (NB2) {
    if (tid < 96) cu1 = (RC1[tid] + RC1[96 + tid]) + (RC1[192 + tid] + RC1[288 + tid]);
    if (vi == 12 && j < 2) {      // d b_0 | d b_1
      sum = (RB[4 * j] + RB[4 * j + 1]) + (RB[4 * j + 2] + RB[4 * j + 3]);
    }
    if constexpr (F16) bad |= !__builtin_isfinite(cu1);
  }
  if constexpr (F16) {
    bad |= !(__builtin_isfinite(sum) && __builtin_isfinite(cu));
    if (bad && a.found_inf) *a.found_inf = 1.0f;
  }
  __syncthreads();
  float* C = S;            // c[u]
  float* HD = S + 128;     // sum dlogit * y
  float* C1 = S + 160;     // NB2: c1[u], sum d1 * y
  float* HD1 = S + 256;
  if constexpr (NB2) {
    if (tid < 96) C1[tid] = cu1;
    if (vi == 10 || vi == 11) HD1[j + 16 * (vi & 1)] = sum;
    if (vi == 12 && j < 2) P[NP_HEADB + j] = sum;
  }
  if (tid < 96) C[tid] = cu;
  if (vi < 10) {
    const int f = j + 16 * (vi & 1);
    if (vi < 2) P[DP_LN1QW + f] = sum;
    else if (vi < 4) P[DP_LN1QB + f] = sum;
    else if (vi < 6) P[DP_LN2W + f] = sum;
    else if (vi < 8) P[DP_LN2B + f] = sum;
    else HD[f] = sum;
  }
  __syncthreads();
  if constexpr (GAUSS) {
    if (tid < 32) {      // the head's four gradients from P (HD) and Q
      float q = 0.f;
#pragma unroll
      for (int t = 0; t < kT; ++t) q += RQ[t];
      const float pf = HD[tid], hw = a.head_w[tid];
      P[DP_HEADW + tid] = fmaf(hln_w[tid], pf, hln_b[tid] * q);
      P[GP_HLNW + tid] = hw * pf;
      P[GP_HLNB + tid] = hw * q;
      P[GP_HEADB + tid] = tid == 0 ? q : 0.f;
    }
#pragma unroll
    for (int n = 0; n < 3; ++n) {      // d Wc = ub (x) c + sum (beta xhat) (x) hid
      const int it = kh + 2 * n;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int f = 16 * half + 4 * g4 + r;
        P[DP_WC + f * kHP + 16 * it + li] = fmaf(head_vec(f), C[16 * it + li], gwc[n][r]);
      }
    }
  } else if constexpr (NB2) {     // d w_k = sum d_k y + Wc C_k;  d Wc = w0 (x) C0 + w1 (x) C1
    if (tid < 64) {
      const int k = tid >> 5, f = tid & 31;
      const float* Ck = k ? C1 : C;
      float s2 = k ? HD1[f] : HD[f];
      for (int u = 0; u < H; ++u) s2 = fmaf(a.mlp.wct[u * 32 + f], Ck[u], s2);
      P[(k ? NP_HEADW1 : DP_HEADW) + f] = s2;
    }
    for (int idx = tid; idx < 32 * kHP; idx += kThreads)
      P[DP_WC + idx] = fmaf(a.head_w[idx / kHP], C[idx % kHP], a.head_w[32 + idx / kHP] * C1[idx % kHP]);
  } else {
  if (tid < 32) {
    float s2 = HD[tid];
    for (int u = 0; u < H; ++u) s2 = fmaf(a.mlp.wct[u * 32 + tid], C[u], s2);
    P[DP_HEADW + tid] = s2;
  }
  for (int idx = tid; idx < 32 * kHP; idx += kThreads) P[DP_WC + idx] = a.head_w[idx / kHP] * C[idx % kHP];
  }

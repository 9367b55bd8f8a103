// Record-free inference and sampling of the shapes outside the fused family (scldm_dit_infer_*; see include/scldm_hip.h).  Included at
// the end of train_api.hip: the GEMM and elementwise dispatch helpers there are file-local, and this path runs the training forward's
// kernels through them - conditioning rows -> trunk over a row index -> CFG blend + state update, as api.hip's cfg_cond / cfg_trunk /
// scldm_sample_ode do for the fused family.  What differs from scldm_dit_train_forward:
//   - no activation record: ONE layer's arrays, overwritten by the next layer; the residual stream alternates between two buffers;
//   - the conditioning runs over n_rows rows (1 + n_pass x unique label rows for a scalar t), the trunk reads them through row_index;
//   - the bf16 weight mirror is refreshed once per C call (its own cast-job table, no transposed copies), not once per evaluation.
// With one conditioning row per sample-forward the kernels, operands and split-K choices are the training forward's: same bits.

namespace {

constexpr int kInferEvalChunk = 256;   // evaluations whose timestep embeddings are formed by one pass of the timestep MLP

struct InferWs {
  float *tgrid, *freq, *th, *sth, *temb;   // max(n_rows, kInferEvalChunk when sampling) rows
  float *c, *sc;                           // n_rows
  float* mod;                              // n_rows x mod_w (only with n_fwd > 0: scldm_dit_infer_cond_rows writes to its caller's array)
  float *xa, *xb, *h, *qkv, *ao, *y, *a, *b, *hid;   // one layer of n_fwd x 16 tokens
  float* part;
  size_t part_floats;
  float* v;          // (n_fwd, S, Din) trunk outputs of a CFG evaluation
  int32_t* ridx;     // n_fwd
  float *dz, *k2, *ztmp;   // n_state samples each
  size_t bytes;
};

InferWs carve_infer(const scldm_dit* h, void* base, int n_fwd, int n_rows, int n_state) {
  const size_t T = (size_t)n_fwd * kS, H = h->cfg.hidden_dim, kD = h->cfg.n_embed, e = (size_t)kS * h->cfg.n_embed_input;
  const size_t t_rows = std::max<size_t>(n_rows, n_state > 0 ? kInferEvalChunk : 0);
  Carver c{reinterpret_cast<char*>(base)};
  InferWs s;
  s.tgrid = c.take(t_rows);
  s.freq = c.take(t_rows * 256);
  s.th = c.take(t_rows * kD);
  s.sth = c.take(t_rows * kD);
  s.temb = c.take(t_rows * kD);
  s.c = c.take((size_t)n_rows * kD);
  s.sc = c.take((size_t)n_rows * kD);
  s.mod = c.take(n_fwd > 0 ? (size_t)n_rows * h->mod_w : 0);
  s.xa = c.take(T * kD);
  s.xb = c.take(T * kD);
  s.h = c.take(T * kD);
  s.qkv = c.take(T * 3 * kD);
  s.ao = c.take(T * kD);
  s.y = c.take(T * kD);
  s.a = c.take(T * H);
  s.b = c.take(T * H);
  s.hid = c.take(T * H);
  s.part_floats = split_k_floats(h);
  s.part = c.take(s.part_floats);
  s.v = c.take(n_state > 0 || n_rows > 0 ? (size_t)n_fwd * e : 0);
  s.ridx = reinterpret_cast<int32_t*>(c.take(n_fwd));
  s.dz = c.take((size_t)n_state * e);
  s.k2 = c.take((size_t)n_state * e);
  s.ztmp = c.take((size_t)n_state * e);
  s.bytes = c.off;
  return s;
}

// the bf16 weight mirror of the handle from the live parameters, for this C call: w16 / ada16 / ada_ball as refresh_w16 fills them
// (same casts, same destinations), through a table of its own without transposed copies
int refresh_w16_infer(scldm_dit* h, const scldm_dit_weights* w, hipStream_t st) {
  if (h->cfg.n_layer == 0) return SCLDM_OK;
  TRY(alloc_w16(h));
  const std::vector<const void*> key = w16_key_of(h, w, false);
  if (key != h->infer_key || !h->d_infer_jobs) {
    const std::vector<CastJob> jobs = w16_cast_jobs(h, w, false);
    if (!h->d_infer_jobs) HIP_TRY(hipMalloc(&h->d_infer_jobs, jobs.size() * sizeof(CastJob)));
    HIP_TRY(hipStreamSynchronize(st));   // (synchronous copy of a pageable vector: only when the parameters' device pointers changed)
    HIP_TRY(hipMemcpy(h->d_infer_jobs, jobs.data(), jobs.size() * sizeof(CastJob), hipMemcpyHostToDevice));
    h->n_infer_jobs = (int)jobs.size();
    h->infer_key = key;
  }
  hipLaunchKernelGGL(cast_jobs_kernel, dim3(64, h->n_infer_jobs), dim3(256), 0, st, (const CastJob*)h->d_infer_jobs, h->n_infer_jobs);
  LAUNCH_CHECK();
  return SCLDM_OK;
}

// common argument checks; *precision becomes the policy that runs (train_precision) and g_bf16 is set for the call's GEMMs
int check_infer(const scldm_dit* h, const scldm_dit_weights* w, int n, int* precision, const void* ws, const char* fused_entry) {
  if (!h || !w || !ws) return fail(SCLDM_ERR_SHAPE, "null argument");
  if (h->fused) return fail(SCLDM_ERR_SHAPE, "this handle's shape is in the fused family: use %s (scldm_dit_infer_* serves the other shapes)", fused_entry);
  *precision = train_precision(h, n, *precision);
  return check_common(h, w, n, *precision, ws, ws);
}

Scratch split_k_scratch(const InferWs& s) {
  Scratch k{};
  k.part = s.part;
  k.part_floats = s.part_floats;
  return k;
}

template <typename E>
E embed_args(const scldm_dit* h, const scldm_dit_weights* w, const int64_t* const* labels, uint32_t mask) {
  E e{};
  e.n_classes = h->cfg.n_classes;
  for (int c = 0; c < h->cfg.n_classes; ++c) {
    e.table[c] = w->class_emb[c];
    e.labels[c] = (labels && ((mask >> c) & 1u)) ? labels[c] : nullptr;
    e.vocab[c] = h->tab_rows[c] - 1;   // last table row: the null token when the tables have one
  }
  return e;
}
int check_null_rows(const scldm_dit* h, const int64_t* const* labels, uint32_t mask) {
  if (!h->cfg.has_null_row)
    for (int c = 0; c < h->cfg.n_classes; ++c)
      if (!labels || !labels[c] || !((mask >> c) & 1u))
        return fail(SCLDM_ERR_SHAPE, "class %d needs its null token, but the class tables have no null row (cfg_dropout_prob == 0)", c);
  return SCLDM_OK;
}

// timestep embeddings of n_t device times: temb (n_t, D) = t_embedder(t)   (the training forward's kernels over n_t rows)
int infer_t_embed(const scldm_dit* h, const scldm_dit_weights* w, const float* t, int n_t, const InferWs& s, Scratch& k, hipStream_t st) {
  const int kD = h->cfg.n_embed;
  hipLaunchKernelGGL(t_freq_kernel, dim3(n_t), dim3(256), 0, st, t, n_t, s.freq);
  LAUNCH_CHECK();
  TRY(linear_fwd(st, s.freq, 256, w->t_w0, n_t, kD, 256, w->t_b0, s.th, kD, k));
  hipLaunchKernelGGL(silu_kernel<float>, dim3(ew_grid((long)n_t * kD)), dim3(256), 0, st, s.th, s.sth, (long)n_t * kD);
  LAUNCH_CHECK();
  return linear_fwd(st, s.sth, kD, w->t_w2, n_t, kD, kD, w->t_b2, s.temb, kD, k);
}

// c rows [row0, row0 + rows) = temb (row stride temb_stride: 0 shares one embedding) + the class embeddings of `labels` under `mask`
int infer_cond_sum(const scldm_dit* h, const scldm_dit_weights* w, const float* temb, long temb_stride, const int64_t* const* labels,
                   uint32_t mask, int row0, int rows, const InferWs& s, hipStream_t st) {
  if (rows <= 0) return SCLDM_OK;
  TRY(check_null_rows(h, labels, mask));
  const int kD = h->cfg.n_embed;
  return scldm_infer_cond_sum_rows(st, temb, temb_stride, embed_args<InferEmbed>(h, w, labels, mask), rows, kD, s.c + (size_t)row0 * kD);
}

// mod (rows, mod_w) = SiLU(c) W_adaLN^T + b for every block and the final layer: the training forward's choice of route for `rows`
// samples (the stacked bf16-source product over the weight mirror, or one Linear per layer)
int infer_adaln(scldm_dit* h, const scldm_dit_weights* w, int rows, int precision, const InferWs& s, float* mod, Scratch& k, hipStream_t st) {
  const int L = h->cfg.n_layer, kD = h->cfg.n_embed, mw = h->mod_w;
  if (ada16_eligible(h, rows, precision)) {
    hipLaunchKernelGGL(silu_kernel<__bf16>, dim3(ew_grid((long)rows * kD)), dim3(256), 0, st, s.c, reinterpret_cast<__bf16*>(s.sc), (long)rows * kD);
    LAUNCH_CHECK();
    return bgemm(st, reinterpret_cast<const __bf16*>(s.sc), kD, true, reinterpret_cast<const __bf16*>(h->ada16), kD, true, mod, mw, rows, mw, kD,
                 h->ada_ball, false, k.part, k.part_floats);
  }
  hipLaunchKernelGGL(silu_kernel<float>, dim3(ew_grid((long)rows * kD)), dim3(256), 0, st, s.c, s.sc, (long)rows * kD);
  LAUNCH_CHECK();
  for (int l = 0; l < L; ++l)
    TRY(linear_fwd(st, s.sc, kD, w->ada_w[l], rows, 6 * kD, kD, w->ada_b[l], mod + (long)l * 6 * kD, mw, k));
  return linear_fwd(st, s.sc, kD, w->fin_ada_w, rows, 2 * kD, kD, w->fin_ada_b, mod + (long)L * 6 * kD, mw, k);
}

// the row-indexed LayerNorm-modulate (infer_wide.hip) with the training forward's call shapes: h as an fp32 or a bf16 array, and the
// fused residual form over a bf16 branch output
int ln_rows(hipStream_t st, int D, const float* x, const float* mod, long mw, const int32_t* ridx, int sc_off, int sh_off, float eps, long T, float* h) {
  return scldm_infer_ln_rows(st, D, x, nullptr, false, 0, nullptr, mod, mw, ridx, sc_off, sh_off, eps, T, h, false);
}
int ln_rows(hipStream_t st, int D, const float* x, const float* mod, long mw, const int32_t* ridx, int sc_off, int sh_off, float eps, long T, __bf16* h) {
  return scldm_infer_ln_rows(st, D, x, nullptr, false, 0, nullptr, mod, mw, ridx, sc_off, sh_off, eps, T, h, true);
}
int ln_rows_res(hipStream_t st, int D, const float* x, const __bf16* y, int g_off, float* x_out, const float* mod, long mw, const int32_t* ridx,
                int sc_off, int sh_off, float eps, long T, float* h) {
  return scldm_infer_ln_rows(st, D, x, y, true, g_off, x_out, mod, mw, ridx, sc_off, sh_off, eps, T, h, false);
}
int ln_rows_res(hipStream_t st, int D, const float* x, const __bf16* y, int g_off, float* x_out, const float* mod, long mw, const int32_t* ridx,
                int sc_off, int sh_off, float eps, long T, __bf16* h) {
  return scldm_infer_ln_rows(st, D, x, y, true, g_off, x_out, mod, mw, ridx, sc_off, sh_off, eps, T, h, true);
}

// The trunk over n_fwd sample-forwards on prepared conditioning rows: scldm_dit_train_forward's sequence of launches from the input
// projection on, over one layer's arrays.  x holds n_direct samples; sample-forwards beyond them re-read the last `rep`.
int infer_trunk(scldm_dit* h, const scldm_dit_weights* w, const float* x, int n_direct, int rep, int n_fwd, const float* mod,
                const int32_t* ridx, float* out, int precision, const InferWs& s, hipStream_t st) {
  const scldm_dit_config& cfg = h->cfg;
  const int L = cfg.n_layer, din = cfg.n_embed_input, H = cfg.hidden_dim, kD = cfg.n_embed, kNH = cfg.n_head;
  const long mw = h->mod_w;
  const int n = n_fwd;
  const long T = (long)n * kS;
  Scratch k = split_k_scratch(s);
  const bool src16 = src16_eligible(h, n, precision);
  const int Hp = hidden16(h);
  // x_0 = input_proj(x) + pos_embed over the distinct samples, then the conditional passes' copies
  float *x_in = s.xa, *x_mid = s.xb;
  TRY(linear_fwd(st, x, din, w->in_w, n_direct * kS, kD, din, w->in_b, x_in, kD, k));
  hipLaunchKernelGGL(add_pos_kernel, dim3(ew_grid((long)n_direct * kS * kD)), dim3(256), 0, st, x_in, w->pos_embed, (long)n_direct * kS, kD);
  LAUNCH_CHECK();
  if (n_fwd > n_direct) {
    TRY(scldm_infer_rep_rows(st, x_in, n_direct, rep, n_fwd, (long)kS * kD));
  }
  const bool overlap = src16 && g_overlap;   // the two up-projections of the MLP side by side, as in the training forward
  Scratch k2 = k;
  if (overlap) {
    const size_t half = (k.part_floats / 2) & ~(size_t)63;
    k2.part = k.part + half;
    k2.part_floats = k.part_floats - half;
    k.part_floats = half;
  }
  const bool y16 = src16 && g_y16;
  const bool fuse_res = y16 && g_fuse_res;
  auto lin = [&](const float* xin, int ldx, const float* W, const __bf16* Wh, int out_f, int in_f, const float* b, float* y,
                 hipStream_t sx = nullptr, bool y16 = false) {
    return src16 ? linear_fwd16(sx ? sx : st, reinterpret_cast<const __bf16*>(xin), ldx, Wh, (int)T, out_f, in_f, b, y, out_f, sx ? k2 : k, y16)
                 : linear_fwd(st, xin, ldx, W, (int)T, out_f, in_f, b, y, out_f, k);
  };
  __bf16* h16 = reinterpret_cast<__bf16*>(s.h);
  const __bf16* y16p = reinterpret_cast<const __bf16*>(s.y);
  for (int l = 0; l < L; ++l) {
    const int o = l * 6 * kD;
    const W16 wh = src16 ? w16_layer(h, l) : W16{};
    float* x_next = x_in;   // the layer's input is dead once x_mid exists
    if (src16 && !(fuse_res && l > 0)) TRY(ln_rows(st, kD, x_in, mod, mw, ridx, o, o + kD, cfg.layernorm_eps, T, h16));
    else if (!src16) TRY(ln_rows(st, kD, x_in, mod, mw, ridx, o, o + kD, cfg.layernorm_eps, T, s.h));
    TRY(lin(s.h, kD, w->attn_w[l], wh.attn_w, 3 * kD, kD, w->attn_b[l], s.qkv, nullptr, src16));
    if (src16) TRY(attn_fwd(st, kD, kNH, n, reinterpret_cast<const __bf16*>(s.qkv), reinterpret_cast<__bf16*>(s.ao)));
    else TRY(attn_fwd(st, kD, kNH, n, (const float*)s.qkv, s.ao));
    TRY(lin(s.ao, kD, w->proj_w[l], wh.proj_w, kD, kD, w->proj_b[l], s.y, nullptr, y16));
    if (fuse_res) {
      TRY(ln_rows_res(st, kD, x_in, y16p, o + 2 * kD, x_mid, mod, mw, ridx, o + 3 * kD, o + 4 * kD, cfg.layernorm_eps, T, h16));
    } else {
      TRY(scldm_infer_gate_res_rows(st, x_in, s.y, y16, mod, mw, ridx, o + 2 * kD, T, kD, x_mid));
      if (src16) TRY(ln_rows(st, kD, x_mid, mod, mw, ridx, o + 3 * kD, o + 4 * kD, cfg.layernorm_eps, T, h16));
      else TRY(ln_rows(st, kD, x_mid, mod, mw, ridx, o + 3 * kD, o + 4 * kD, cfg.layernorm_eps, T, s.h));
    }
    hipStream_t s2 = nullptr;
    if (overlap) TRY(fused::fork_side(h, st, 2, &s2));
    TRY(lin(s.h, kD, w->w2[l], wh.w2, H, kD, nullptr, s.b, s2, src16));
    TRY(lin(s.h, kD, w->w1[l], wh.w1, H, kD, nullptr, s.a, nullptr, src16));
    if (overlap) TRY(fused::join_side(h, st, 2));
    if (src16) hipLaunchKernelGGL((swiglu_fwd_kernel<__bf16, __bf16>), dim3(ew_grid(T * H)), dim3(256), 0, st, reinterpret_cast<const __bf16*>(s.a),
                                  reinterpret_cast<const __bf16*>(s.b), reinterpret_cast<__bf16*>(s.hid), T * H, H, Hp);
    else hipLaunchKernelGGL((swiglu_fwd_kernel<float, float>), dim3(ew_grid(T * H)), dim3(256), 0, st, (const float*)s.a, (const float*)s.b, s.hid, T * H, H, H);
    LAUNCH_CHECK();
    TRY(lin(s.hid, src16 ? Hp : H, w->cproj[l], wh.cproj, kD, H, nullptr, s.y, nullptr, y16));
    if (fuse_res) {   // x_next = x_mid + a5 * y2 and the NEXT LayerNorm-modulate (the next layer's first, or the final layer's) in one pass
      const int on = (l + 1) * 6 * kD;
      if (l + 1 < L) TRY(ln_rows_res(st, kD, x_mid, y16p, o + 5 * kD, x_next, mod, mw, ridx, on, on + kD, cfg.layernorm_eps, T, h16));
      else TRY(ln_rows_res(st, kD, x_mid, y16p, o + 5 * kD, x_next, mod, mw, ridx, on + kD, on, cfg.layernorm_eps, T, s.h));
    } else {
      TRY(scldm_infer_gate_res_rows(st, x_mid, s.y, y16, mod, mw, ridx, o + 5 * kD, T, kD, x_next));
    }
  }
  // FinalLayerDit: [shift | scale] = adaLN(c); LN(x) * (1 + scale) + shift; Linear
  const int of = L * 6 * kD;
  if (!(fuse_res && L > 0)) TRY(ln_rows(st, kD, x_in, mod, mw, ridx, of + kD, of, cfg.layernorm_eps, T, s.h));
  return linear_fwd(st, s.h, kD, w->fin_w, (int)T, din, kD, w->fin_b, out, din, k);
}

// ---- one CFG evaluation (CfgPlan, make_plan: cfg_plan.hpp; this path always blends, whatever the plan's `direct` says) --------------------
// the conditioning rows of one evaluation from its timestep embedding(s): row(s) of the unconditional pass (every class null), then
// U rows per conditional pass.  temb_stride 0: one embedding for all rows; D: row i of the state's 2B (conditional rows: the second half)
int infer_cfg_cond(scldm_dit* h, const scldm_dit_weights* w, const CfgPlan& pl, const float* temb, long temb_stride, int precision,
                   const InferWs& s, Scratch& k, hipStream_t st) {
  TRY(infer_cond_sum(h, w, temb, temb_stride, nullptr, 0u, 0, pl.uncond_rows, s, st));
  for (int p = 0; p < pl.P; ++p)
    TRY(infer_cond_sum(h, w, temb + (size_t)pl.B * temb_stride, temb_stride, pl.ulabels, pl.mask[p], pl.uncond_rows + p * pl.U, pl.U, s, st));
  return infer_adaln(h, w, pl.n_rows, precision, s, s.mod, k, st);
}
// the state-dependent part: the trunk over every sample-forward, then the blend (with the caller's Euler step when euler_z is given)
int infer_cfg_trunk(scldm_dit* h, const scldm_dit_weights* w, const CfgPlan& pl, const float* z, float* dz, int precision, const InferWs& s,
                    hipStream_t st, float* euler_z = nullptr, float euler_h = 0.f) {
  TRY(infer_trunk(h, w, z, 2 * pl.B, pl.B, pl.n_fwd, s.mod, s.ridx, s.v, precision, s, st));
  return scldm_cfg_blend(s.v, dz, pl.B, kS * h->cfg.n_embed_input, pl.P, pl.scale, euler_z, euler_h, st);
}

}  // namespace

extern "C" size_t scldm_dit_infer_workspace_bytes(const scldm_dit* h, int n_fwd, int n_rows, int n_state, int precision) {
  (void)precision;   // (every policy carves fp32-sized slots, as the training record does)
  if (!h || h->fused || n_fwd < 0 || n_rows < 0 || n_state < 0) return 0;
  return carve_infer(h, nullptr, n_fwd, n_rows, n_state).bytes;
}

extern "C" int scldm_dit_infer_cond_rows(scldm_dit* h, const scldm_dit_weights* w, const float* t, int t_stride, const int64_t* const* labels,
                                         int n_rows, float* mod_out, int precision, void* ws, void* stream_) {
  TRY(check_infer(h, w, n_rows, &precision, ws, "scldm_dit_cond_rows"));
  if (!t || !mod_out) return fail(SCLDM_ERR_SHAPE, "null argument");
  if (t_stride != 0 && t_stride != 1) return fail(SCLDM_ERR_SHAPE, "t_stride must be 0 (one scalar t) or 1 (one t per row)");
  TRY(check_null_rows(h, labels, 0xffffffffu));
  hipStream_t st = (hipStream_t)stream_;
  const InferWs s = carve_infer(h, ws, 0, n_rows, 0);
  Scratch k = split_k_scratch(s);
  const int kD = h->cfg.n_embed;
  if (ada16_eligible(h, n_rows, precision)) TRY(refresh_w16_infer(h, w, st));
  TRY(infer_t_embed(h, w, t, t_stride ? n_rows : 1, s, k, st));
  if (t_stride) {   // one embedding per row: the training forward's own kernel
    hipLaunchKernelGGL(cond_sum_kernel, dim3(n_rows, kD / 256), dim3(256), 0, st, s.temb, embed_args<EmbedArgs>(h, w, labels, 0xffffffffu), n_rows, kD, s.c);
    LAUNCH_CHECK();
  } else {
    TRY(infer_cond_sum(h, w, s.temb, 0, labels, 0xffffffffu, 0, n_rows, s, st));
  }
  return infer_adaln(h, w, n_rows, precision, s, mod_out, k, st);
}

extern "C" int scldm_dit_infer_forward_rows(scldm_dit* h, const scldm_dit_weights* w, const float* x, int n_direct, int rep, int n_fwd,
                                            const float* mod, const int32_t* row_index, float* out, int precision, void* ws, void* stream_) {
  TRY(check_infer(h, w, n_fwd, &precision, ws, "scldm_dit_forward_rows"));
  if (n_direct <= 0 || n_direct > n_fwd || (n_fwd > n_direct && (rep <= 0 || rep > n_direct)))
    return fail(SCLDM_ERR_SHAPE, "bad n_fwd/n_direct/rep (%d,%d,%d)", n_fwd, n_direct, rep);
  if (!x || !mod || !out) return fail(SCLDM_ERR_SHAPE, "null pointer argument");
  hipStream_t st = (hipStream_t)stream_;
  const InferWs s = carve_infer(h, ws, n_fwd, 0, 0);
  if (src16_eligible(h, n_fwd, precision)) TRY(refresh_w16_infer(h, w, st));
  return infer_trunk(h, w, x, n_direct, rep > 0 ? rep : 1, n_fwd, mod, row_index, out, precision, s, st);
}

extern "C" int scldm_dit_infer_forward_cfg(scldm_dit* h, const scldm_dit_weights* w, const float* x, const float* t, int t_stride,
                                           const int64_t* const* ulabels, int n_urows, const int32_t* cell_row, int B, int n_pass,
                                           const uint32_t* pass_mask, const float* pass_scale, float* out, int precision, void* ws,
                                           void* stream_) {
  TRY(check_infer(h, w, B > 0 ? 2 * B + std::max(n_pass, 0) * B : 1, &precision, ws, "scldm_dit_forward_cfg"));
  if (!x || !t || !out) return fail(SCLDM_ERR_SHAPE, "null pointer argument");
  if (t_stride != 0 && t_stride != 1) return fail(SCLDM_ERR_SHAPE, "t_stride must be 0 (one scalar t) or 1 (one t per sample)");
  CfgPlan pl;
  TRY(make_plan(h, pl, ulabels, n_urows, cell_row, B, n_pass, pass_mask, pass_scale, t_stride));
  hipStream_t st = (hipStream_t)stream_;
  const InferWs s = carve_infer(h, ws, pl.n_fwd, pl.n_rows, 0);
  Scratch k = split_k_scratch(s);
  if (src16_eligible(h, pl.n_fwd, precision) || ada16_eligible(h, pl.n_rows, precision)) TRY(refresh_w16_infer(h, w, st));
  TRY(scldm_cfg_fill_row_index(s.ridx, cell_row, 2 * B, pl.uncond_rows, B, pl.U, pl.P, st));
  TRY(infer_t_embed(h, w, t, t_stride ? 2 * B : 1, s, k, st));
  TRY(infer_cfg_cond(h, w, pl, s.temb, t_stride ? h->cfg.n_embed : 0, precision, s, k, st));
  return infer_cfg_trunk(h, w, pl, x, out, precision, s, st);
}

extern "C" int scldm_dit_infer_sample_ode(scldm_dit* h, const scldm_dit_weights* w, float* z, const int64_t* const* ulabels, int n_urows,
                                          const int32_t* cell_row, int B, int n_pass, const uint32_t* pass_mask, const float* pass_scale,
                                          int n_steps, int method, int precision, void* ws, void* stream_) {
  TRY(check_infer(h, w, B > 0 ? 2 * B + std::max(n_pass, 0) * B : 1, &precision, ws, "scldm_sample_ode"));
  if (!z) return fail(SCLDM_ERR_SHAPE, "null pointer argument");
  if (n_steps < 1) return fail(SCLDM_ERR_SHAPE, "n_steps must be >= 1");
  if (method != SCLDM_METHOD_EULER && method != SCLDM_METHOD_HEUN) return fail(SCLDM_ERR_SHAPE, "unknown method %d", method);
  CfgPlan pl;
  TRY(make_plan(h, pl, ulabels, n_urows, cell_row, B, n_pass, pass_mask, pass_scale, 0));
  hipStream_t st = (hipStream_t)stream_;
  const InferWs s = carve_infer(h, ws, pl.n_fwd, pl.n_rows, 2 * B);
  Scratch k = split_k_scratch(s);
  // the weights do not move during a solve: ONE refresh of the mirror for every evaluation
  if (src16_eligible(h, pl.n_fwd, precision) || ada16_eligible(h, pl.n_rows, precision)) TRY(refresh_w16_infer(h, w, st));
  TRY(scldm_cfg_fill_row_index(s.ridx, cell_row, 2 * B, 1, B, pl.U, pl.P, st));
  const size_t n = (size_t)2 * B * kS * h->cfg.n_embed_input;
  const int steps = n_steps + 1, kD = h->cfg.n_embed;
  const bool heun = method == SCLDM_METHOD_HEUN;
  const int n_evals = heun ? 2 * n_steps : n_steps;
  // one evaluation; the timestep embeddings of kInferEvalChunk evaluations at a time come from one pass of the timestep MLP
  // (grid_times_kernel of infer_wide.hip computes grid::linspace's values)
  auto eval = [&](int e, const float* zin, float* dz, float* euler_z, float euler_h) -> int {
    const int j = e % kInferEvalChunk;
    if (j == 0) {
      const int m = std::min(kInferEvalChunk, n_evals - e);
      TRY(scldm_infer_grid_times(st, s.tgrid, steps, heun ? 1 : 0, e, m));
      TRY(infer_t_embed(h, w, s.tgrid, m, s, k, st));
    }
    TRY(infer_cfg_cond(h, w, pl, s.temb + (size_t)j * kD, 0, precision, s, k, st));
    return infer_cfg_trunk(h, w, pl, zin, dz, precision, s, st, euler_z, euler_h);
  };
  return grid::euler_heun(
      n_steps, 0.f, 1.f, heun, grid::Buffers{z, s.dz, s.k2, s.ztmp}, eval,
      [&](const float* x, const float* kk, float* out, float hs) { return scldm_ode_axpy(x, kk, out, hs, n, st); },
      [&](float* x, const float* k1, const float* k2, float half_hs) { return scldm_ode_heun(x, k1, k2, half_hs, n, st); });
}

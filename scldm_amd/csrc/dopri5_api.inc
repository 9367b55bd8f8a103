// scldm_sample_ode_dopri5: the reference's default sampler as one call (include/scldm_hip.h).  Part of api.hip's translation unit: it uses
// that file's plan, conditioning and trunk helpers.  The step loop and its decisions are dopri5_ctl.hpp (plain C++: solve(), shared with
// scldm_logp_ode_dopri5); this file is the problem that loop drives.  The state kernels are dopri5_fused.hpp.
//
// One attempted step = one batched conditioning pass over its six new evaluation times (time list -> t_embed_list_kernel ->
// cond_rows_kernel over (rows, 6) -> one adaLN projection over 6 x rows rows: api.hip's cond_batch with n_evals = 6), the first
// stage point (combine_kernel), six trunks each followed by ONE state kernel, error_final_kernel, and an 8-byte read of the error ratio.

struct D5Ws {
  float *h, *v, *mod, *silu;
  void* asplit;
  float *temb, *tlist;
  int32_t* ridx;
  float* k[7];
  float* y[2];
  float* c[4];
  double *red, *red2;   // 1 024 doubles each: [0, 1022) block partials | [1022] the mean
  size_t total;
};
static D5Ws d5_carve(const scldm_dit* h, void* base, int B, int n_pass, int n_urows) {
  D5Ws w;
  char* p = (char*)base;
  size_t off = 0;
  const size_t e = (size_t)16 * h->cfg.n_embed_input, n_state = (size_t)2 * B;
  const size_t n_fwd = (size_t)2 * B + (size_t)n_pass * B, n_rows = 1 + (size_t)n_pass * n_urows;   // one unconditional row + a row per pass and label row
  const size_t rows_all = scldm::dopri5::kStages * n_rows;
  auto take = [&](size_t bytes) { char* r = p + off; off += align256(bytes); return r; };
  w.h = (float*)take((size_t)pad8((int)n_fwd) * 16 * 256 * 4);
  w.v = (float*)take(n_fwd * e * 4);
  w.mod = (float*)take(rows_all * h->mod_w * 4);
  w.silu = (float*)take((rows_all + 1) * 256 * 4);
  w.asplit = take((rows_all + 31) / 32 * 32 * 256 * 4);
  w.temb = (float*)take((size_t)8 * 256 * 4);
  w.tlist = (float*)take(8 * 4);
  w.ridx = (int32_t*)take(n_fwd * 4);
  for (int i = 0; i < 7; ++i) w.k[i] = (float*)take(n_state * e * 4);
  for (int i = 0; i < 2; ++i) w.y[i] = (float*)take(n_state * e * 4);
  for (int i = 0; i < 4; ++i) w.c[i] = (float*)take(n_state * e * 4);
  w.red = (double*)take(1024 * 8);
  w.red2 = (double*)take(1024 * 8);
  w.total = off;
  return w;
}
extern "C" size_t scldm_sample_ode_dopri5_workspace_bytes(const scldm_dit* h, int B, int n_pass, int n_urows) {
  if (!h || !h->fused || B < 1 || n_pass < 0 || n_pass > SCLDM_MAX_CLASSES || n_urows < 0) return 0;
  return d5_carve(h, nullptr, B, n_pass, n_urows).total;
}

// save_times: host, num_save non-decreasing fp32 times, the first 0 (the state there is the initial z)
static int d5_solve(scldm_dit* h, float* z, const int64_t* const* ulabels, int n_urows, const int32_t* cell_row, int B, int n_pass,
                    const uint32_t* pass_mask, const float* pass_scale, int num_save, const float* save_times, double atol, double rtol,
                    double first_step, float* traj, scldm_dopri5_stats* stats, double* step_log, int step_log_cap, int precision, void* ws_,
                    void* stream_) {
  namespace d5 = scldm::dopri5;
  namespace rk = scldm::rk;
  if (stats) *stats = scldm_dopri5_stats{};
  // (the shape family first, before any HIP call: a handle of another shape holds no device memory at all)
  if (!h) return fail(SCLDM_ERR_SHAPE, "null handle");
  if (!h->fused)
    return fail(SCLDM_ERR_SHAPE, "scldm_sample_ode_dopri5: this handle's shape is outside the fused family (n_embed=256, n_head=8, seq_len=16, "
                "n_embed_input<=32; got %d,%d,%d,%d) - such shapes keep the host-driven solve", h->cfg.n_embed, h->cfg.n_head, h->cfg.seq_len, h->cfg.n_embed_input);
  if (!z || !ws_) return fail(SCLDM_ERR_SHAPE, "scldm_sample_ode_dopri5: null pointer argument (z / ws)");
  if (num_save < 2) return fail(SCLDM_ERR_SHAPE, "scldm_sample_ode_dopri5: num_save must be >= 2 (save points, the first at t = 0), got %d", num_save);
  if (save_times) {
    if (save_times[0] != 0.0f) return fail(SCLDM_ERR_SHAPE, "scldm_sample_ode_dopri5_at: the first save time must be 0 (got %g)", (double)save_times[0]);
    for (int i = 1; i < num_save; ++i)
      if (!(save_times[i] >= save_times[i - 1]) || !(save_times[i] <= 1e30f))
        return fail(SCLDM_ERR_SHAPE, "scldm_sample_ode_dopri5_at: save times must be finite and non-decreasing (entry %d)", i);
  }
  if (B < 1) return fail(SCLDM_ERR_SHAPE, "scldm_sample_ode_dopri5: B must be positive");
  int rc = dopri5_check_tolerances("scldm_sample_ode_dopri5", atol, rtol, step_log, step_log_cap);
  if (rc) return rc;
  if (((uintptr_t)z & 15) || ((uintptr_t)traj & 15) || ((uintptr_t)ws_ & 255)) return fail(SCLDM_ERR_SHAPE, "scldm_sample_ode_dopri5: z and traj must be 16-byte, ws 256-byte aligned");
  if ((rc = check_ready(h, precision))) return rc;
  CfgPlan pl;
  if ((rc = make_plan(h, pl, ulabels, n_urows, cell_row, B, n_pass, pass_mask, pass_scale, 0))) return rc;
  const int e_row = 16 * h->cfg.n_embed_input;
  const size_t n = (size_t)2 * B * e_row, n4 = n / 4;
  if (n4 > 0x7fffffffull) return fail(SCLDM_ERR_SHAPE, "scldm_sample_ode_dopri5: state too large (at most 2^33 elements)");
  hipStream_t st = (hipStream_t)stream_;
  if ((rc = dopri5_check_stream("scldm_sample_ode_dopri5", h->rk_host, st))) return rc;

  D5Ws w = d5_carve(h, ws_, B, pl.P, pl.U);
  const float atol_f = (float)atol, rtol_f = (float)rtol;
  const unsigned sblocks = (unsigned)cdiv(n4, 256);
  const unsigned eblocks = (unsigned)std::min<long long>(cdiv(n, 256 * 8), 1022);   // scldm_rk_error's grid
  fill_cfg_row_index_kernel<<<cdiv(pl.n_fwd, 256), 256, 0, st>>>(w.ridx, cell_row, 2 * B, 1, B, pl.U, pl.P, nullptr, pl.direct);
  LAUNCH_CHECK();
  if (traj) HIP_TRY(hipMemcpyAsync(traj, z, n * sizeof(float), hipMemcpyDeviceToDevice, st));

  d5::BlendGeom geom{};
  geom.v = w.v;
  geom.B = B;
  geom.e = e_row;
  geom.P = pl.P;
  geom.direct = pl.direct ? 1 : 0;
  fill_pass_scale(geom.scale, pl.P, pl.scale);

  float* K[7];
  for (int i = 0; i < 7; ++i) K[i] = w.k[i];
  // three state buffers in rotation: the start of the last accepted step (c0 of its interpolant), the current state, the stage point
  float *c0 = w.y[1], *y0 = z, *stg = w.y[0];

  // the adaLN vectors of `cnt` evaluations at the given fp32 times -> w.mod, evaluation j in rows [j n_rows, (j + 1) n_rows)
  auto conditioning = [&](const float* times, int cnt) -> int {
    d5::Times tt{};
    for (int j = 0; j < cnt; ++j) tt.t[j] = times[j];
    d5::set_times_kernel<<<1, 64, 0, st>>>(w.tlist, tt, cnt);
    sde::t_embed_list_kernel<<<cnt, 256, 0, st>>>(w.tlist, h->w0t, h->b0, h->w2t, h->b2, w.temb);
    return cond_batch(h, pl, w.temb, cnt, w.silu, w.mod, w.asplit, precision, st);
  };
  auto run_trunk = [&](const float* x, int slot) -> int {
    return trunk(h, x, 2 * B, B, pl.direct ? 2 * B : pl.n_fwd, w.mod + (size_t)slot * pl.n_rows * h->mod_w, w.ridx, w.h, w.v, precision, st);
  };
  // weights with their mask -> the compacted (pointer, coefficient) list the state kernels take
  auto comb = [&](const float* wt, unsigned mask) {
    rk::CombArgs a{};
    a.n_k = d5::compact(wt, mask, [&](int i, int j, float c) { a.k[i] = K[j]; a.c[i] = c; });
    return a;
  };
  // slope alone (out == nullptr) or slope + next stage point
  auto blend_stage = [&](float* k_new, float* out, const float* y_from, const rk::CombArgs& c) -> int {
    d5::StageArgs a{};
    a.g = geom;
    a.k_new = k_new;
    a.out = out;
    a.y0 = y_from;
    a.c = c;
    d5::blend_stage_kernel<<<sblocks, 256, 0, st>>>(a);
    LAUNCH_CHECK();
    return SCLDM_OK;
  };
  // mean of squares of (a - b) / (atol + rtol |y0|) -> red[1022]
  auto norm = [&](const float* a, const float* b, double* red) -> int {
    d5::scaled_norm_kernel<<<eblocks, 256, 0, st>>>(a, b, y0, (long)n4, atol_f, rtol_f, red);
    rk::error_final_kernel<<<1, 256, 0, st>>>(red, eblocks, (long)n, red + 1022);
    LAUNCH_CHECK();
    return SCLDM_OK;
  };
  // f(t, x) into slope k
  auto slope_at = [&](float t, const float* x, float* k) -> int {
    int rc;
    if ((rc = conditioning(&t, 1))) return rc;
    if ((rc = run_trunk(x, 0))) return rc;
    return blend_stage(k, nullptr, nullptr, rk::CombArgs{});
  };

  // what dopri5_ctl.hpp's solve() calls, each in the order it enqueues
  auto first_slope = [&]() -> int { return slope_at(0.0f, y0, K[0]); };
  auto start_norms = [&](double* ms) -> int {
    int rc;
    if ((rc = norm(y0, nullptr, w.red))) return rc;
    if ((rc = norm(K[0], nullptr, w.red2))) return rc;
    volatile double* host = h->rk_host;
    HIP_TRY(hipMemcpyAsync((void*)(host + 0), w.red + 1022, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync((void*)(host + 1), w.red2 + 1022, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    ms[0] = host[0];
    ms[1] = host[1];
    return SCLDM_OK;
  };
  auto probe = [&](double h0, double* ms) -> int {
    rk::CombArgs c1{};
    c1.n_k = 1;
    c1.k[0] = K[0];
    c1.c[0] = (float)h0;
    rk::combine_kernel<<<sblocks, 256, 0, st>>>(stg, y0, c1, (long)n4);   // y0 + h0 f0
    int rc;
    if ((rc = slope_at((float)(0.0 + h0), stg, K[1]))) return rc;
    if ((rc = norm(K[1], K[0], w.red))) return rc;
    return dopri5_read_back(h->rk_host, w.red + 1022, 1, ms, st);
  };
  auto save_time = [&](int si) { return (double)(save_times ? save_times[si] : grid::linspace(si, num_save, 0.f, 1.f)); };
  auto attempt = [&](const d5::Step& step, double* ms) -> int {
    const scldm_dopri5_plan& plan = step.plan;
    int rc;
    if ((rc = conditioning(plan.t_stage, d5::kStages))) return rc;
    rk::combine_kernel<<<sblocks, 256, 0, st>>>(stg, y0, comb(plan.a[0], plan.a_mask[0]), (long)n4);
    LAUNCH_CHECK();
    for (int i = 0; i < d5::kStages; ++i) {
      if ((rc = run_trunk(stg, i))) return rc;
      if (i + 1 < d5::kStages) {
        if ((rc = blend_stage(K[i + 1], stg, y0, comb(plan.a[i + 1], plan.a_mask[i + 1])))) return rc;
      } else {   // the last stage point is the 5th-order solution y1 (FSAL: K[6] = f(ta + h, y1))
        d5::ErrorArgs ea{};
        ea.g = geom;
        ea.k_new = K[6];
        ea.y0 = y0;
        ea.y1 = stg;
        ea.c = comb(plan.err, plan.err_mask);
        ea.n = (long)n;
        ea.atol = atol_f;
        ea.rtol = rtol_f;
        ea.partial = w.red;
        d5::blend_error_kernel<<<eblocks, 256, 0, st>>>(ea);
        rk::error_final_kernel<<<1, 256, 0, st>>>(w.red, eblocks, (long)n, w.red + 1022);
        LAUNCH_CHECK();
      }
    }
    return dopri5_read_back(h->rk_host, w.red + 1022, 1, ms, st);      // the step's one host read
  };
  auto accept = [&](const d5::Step& step, bool fit_dense) -> int {
    if (fit_dense) {
      rk::dense_kernel<<<cdiv(n, 256), 256, 0, st>>>(y0, stg, comb(step.plan.mid, step.plan.mid_mask), K[0], K[6], step.plan.h, step.plan.two_h, (long)n,
                                                     w.c[0], w.c[1], w.c[2], w.c[3]);
      LAUNCH_CHECK();
    }
    float* freed = c0;
    c0 = y0;
    y0 = stg;
    stg = freed;
    std::swap(K[0], K[6]);
    return SCLDM_OK;
  };
  auto emit = [&](int si, double s) -> int {
    const d5::Quartic q = d5::quartic_at(s);
    if (traj) rk::poly_kernel<<<sblocks, 256, 0, st>>>(traj + (size_t)si * n, c0, w.c[0], w.c[1], w.c[2], w.c[3], q.s1, q.s2, q.s3, q.s4, (long)n4);
    if (si == num_save - 1) {
      // (z may be the buffer c0 lives in: a thread writes the four elements it has just read, nothing else)
      rk::poly_kernel<<<sblocks, 256, 0, st>>>(z, c0, w.c[0], w.c[1], w.c[2], w.c[3], q.s1, q.s2, q.s3, q.s4, (long)n4);
    }
    LAUNCH_CHECK();
    return SCLDM_OK;
  };
  auto reached = [&]() -> int {   // what the solve had reached
    if (y0 != z) HIP_TRY(hipMemcpyAsync(z, y0, n * sizeof(float), hipMemcpyDeviceToDevice, st));
    return SCLDM_OK;
  };
  d5::Problem problem{first_slope, start_norms, probe, save_time, attempt, accept, emit, reached};
  // without a trajectory only the state at the last save time (t = 1) is formed: the steps do not depend on the save times
  return d5::solve(problem, first_step, traj ? 1 : num_save - 1, num_save, step_log, step_log_cap, 3, stats);
}

extern "C" int scldm_sample_ode_dopri5(scldm_dit* h, float* z, const int64_t* const* ulabels, int n_urows, const int32_t* cell_row, int B, int n_pass,
                                       const uint32_t* pass_mask, const float* pass_scale, int num_save, double atol, double rtol, double first_step,
                                       float* traj, scldm_dopri5_stats* stats, double* step_log, int step_log_cap, int precision, void* ws,
                                       void* stream) {
  return d5_solve(h, z, ulabels, n_urows, cell_row, B, n_pass, pass_mask, pass_scale, num_save, nullptr, atol, rtol, first_step, traj, stats, step_log,
                  step_log_cap, precision, ws, stream);
}
extern "C" int scldm_sample_ode_dopri5_at(scldm_dit* h, float* z, const int64_t* const* ulabels, int n_urows, const int32_t* cell_row, int B,
                                          int n_pass, const uint32_t* pass_mask, const float* pass_scale, int num_save, const float* save_times,
                                          double atol, double rtol, double first_step, float* traj, scldm_dopri5_stats* stats, double* step_log,
                                          int step_log_cap, int precision, void* ws, void* stream) {
  if (num_save >= 2 && !save_times) return fail(SCLDM_ERR_SHAPE, "scldm_sample_ode_dopri5_at: null pointer argument (save_times)");
  return d5_solve(h, z, ulabels, n_urows, cell_row, B, n_pass, pass_mask, pass_scale, num_save, save_times, atol, rtol, first_step, traj, stats,
                  step_log, step_log_cap, precision, ws, stream);
}

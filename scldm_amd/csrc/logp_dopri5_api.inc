// scldm_logp_ode_dopri5: the reference's default likelihood solve (Sampler.sample_ode_likelihood(sampling_method="dopri5")) as one call
// (include/scldm_hip.h).  Part of logp_api.hip's translation unit: it uses that file's workspace layout and logp.hpp's evaluation kernels.
// The step loop and its decisions are dopri5_ctl.hpp (plain C++: solve(), shared with scldm_sample_ode_dopri5); this file is the problem
// that loop drives.  The state kernels are logp_dopri5.hpp; the dense output of the accepted step that contains s = 1 goes through
// scldm_rk_dense / scldm_rk_poly (the delta_logp arrays are padded to a multiple of four with zeros for them).
//
// One attempted step = the first stage point (scldm_rk_combine on x and on delta_logp), then six evaluations - seed kernel, recording
// forward, input-gradient-only backward, ONE state kernel each - the row-sum kernel, and an 8-byte read of the mean squared error ratio.
#include <algorithm>

#include "dopri5_ctl.hpp"
#include "logp_dopri5.hpp"

namespace {

struct LogpD5Ws {
  LogpWs ev;          // the evaluation's buffers (train workspace in front)
  float* kx[7];       // (2B, e)
  float* kl[7];       // (R4) each: 2B rounded up to a multiple of 4, the tail zero
  float* yx[2];       // with z: start of the last accepted step, current state, stage point - in rotation
  float* yl[3];
  float* cx[4];       // the interpolant's coefficients c1..c4 (c0 is the step's start)
  float* cl[4];
  float* l_end;       // (R4) delta_logp at s = 1
  double* partial;    // (2B) row sums
  double* mean;       // 4 doubles
  size_t bytes;
};
LogpD5Ws carve_logp_d5(const scldm_dit* h, int B, int n_pass, int precision, void* base) {
  LogpD5Ws w{};
  w.ev = carve_logp(h, B, n_pass, precision, base);
  const size_t e = (size_t)16 * h->cfg.n_embed_input, R = (size_t)2 * B, R4 = (R + 3) / 4 * 4;
  size_t off = w.ev.bytes;
  auto take = [&](size_t bytes) {
    void* p = base ? reinterpret_cast<char*>(base) + off : nullptr;
    off += align256(bytes);
    return p;
  };
  for (int i = 0; i < 7; ++i) w.kx[i] = (float*)take(R * e * 4);
  for (int i = 0; i < 2; ++i) w.yx[i] = (float*)take(R * e * 4);
  for (int i = 0; i < 4; ++i) w.cx[i] = (float*)take(R * e * 4);
  // the small arrays in one block (zeroed by one memset at the start of a solve)
  for (int i = 0; i < 7; ++i) w.kl[i] = (float*)take(R4 * 4);
  for (int i = 0; i < 3; ++i) w.yl[i] = (float*)take(R4 * 4);
  for (int i = 0; i < 4; ++i) w.cl[i] = (float*)take(R4 * 4);
  w.l_end = (float*)take(R4 * 4);
  w.partial = (double*)take(R * 8);
  w.mean = (double*)take(4 * 8);
  w.bytes = off;
  return w;
}

}  // namespace

extern "C" size_t scldm_logp_ode_dopri5_workspace_bytes(const scldm_dit* h, int B, int n_pass, int precision) {
  if (!h || !h->fused || B < 1 || n_pass < 0 || n_pass > SCLDM_MAX_CLASSES) return 0;
  return carve_logp_d5(h, B, n_pass, precision, nullptr).bytes;
}

extern "C" int scldm_logp_ode_dopri5(scldm_dit* h, const scldm_dit_weights* w, float* z, const int64_t* const* ulabels, int n_urows,
                                     const int32_t* cell_row, int B, int n_pass, const uint32_t* pass_mask, const float* pass_scale, double atol,
                                     double rtol, double first_step, const float* probe, int probe_per_solve, unsigned long long seed,
                                     long long cell_offset, long long cells_total, float* logp_out, float* dlogp_out, scldm_dopri5_stats* stats,
                                     double* step_log, int step_log_cap, int precision, void* saved, void* ws_, void* stream_) {
  namespace d5 = scldm::dopri5;
  namespace ld = scldm::logp_d5;
  if (stats) *stats = scldm_dopri5_stats{};
  // (every argument check before any HIP call)
  if (!h || !w || !z || !logp_out || !saved || !ws_) return fail(SCLDM_ERR_SHAPE, "scldm_logp_ode_dopri5: null pointer argument (handle / weights / z / logp_out / saved / ws)");
  if (B < 1) return fail(SCLDM_ERR_SHAPE, "scldm_logp_ode_dopri5: B must be positive");
  int rc = dopri5_check_tolerances("scldm_logp_ode_dopri5", atol, rtol, step_log, step_log_cap);
  if (rc) return rc;
  if (cell_offset < 0 || cells_total < cell_offset + B)
    return fail(SCLDM_ERR_SHAPE, "scldm_logp_ode_dopri5: cells_total (%lld) < cell_offset (%lld) + B (%d)", cells_total, cell_offset, B);
  if (probe && !probe_per_solve)
    return fail(SCLDM_ERR_SHAPE, "scldm_logp_ode_dopri5: a given probe needs probe_per_solve (the number of evaluations of an adaptive solve is not known ahead)");
  if (n_pass < 0 || n_pass > SCLDM_MAX_CLASSES) return fail(SCLDM_ERR_SHAPE, "scldm_logp_ode_dopri5: n_pass out of range");
  if (n_pass > 0 && (!ulabels || !pass_mask || !pass_scale || n_urows <= 0)) return fail(SCLDM_ERR_SHAPE, "scldm_logp_ode_dopri5: conditional passes need labels/masks/scales");
  if (n_pass > 0 && !cell_row && n_urows != B) return fail(SCLDM_ERR_SHAPE, "scldm_logp_ode_dopri5: cell_row is NULL but n_urows (%d) != B (%d)", n_urows, B);
  if (((uintptr_t)z & 15) || ((uintptr_t)probe & 15) || ((uintptr_t)logp_out & 3) || ((uintptr_t)dlogp_out & 3) || ((uintptr_t)ws_ & 255))
    return fail(SCLDM_ERR_SHAPE, "scldm_logp_ode_dopri5: z and probe must be 16-byte, logp_out / dlogp_out 4-byte, ws 256-byte aligned");
  if (!h->fused)
    return fail(SCLDM_ERR_SHAPE, "scldm_logp_ode_dopri5: this handle's shape is outside the fused family (n_embed=256, n_head=8, seq_len=16, "
                "n_embed_input<=32; got %d,%d,%d,%d) - such shapes keep the host-driven solve", h->cfg.n_embed, h->cfg.n_head, h->cfg.seq_len, h->cfg.n_embed_input);
  const scldm_dit_config& c = h->cfg;
  if (!c.has_null_row && c.n_classes > 0)
    return fail(SCLDM_ERR_SHAPE, "classifier-free guidance needs the null rows of the class tables (model built with cfg_dropout_prob == 0)");
  const int e = 16 * c.n_embed_input, R = 2 * B;
  const long long N = (long long)(2 + n_pass) * B;
  if (c.seq_len != 16 || e % 4 || N * (e / 4) > 0x7fffffffll || N > 0x7fffffffll) return fail(SCLDM_ERR_SHAPE, "scldm_logp_ode_dopri5: state too large or unsupported shape");
  hipStream_t st = (hipStream_t)stream_;
  if ((rc = dopri5_check_stream("scldm_logp_ode_dopri5", h->rk_host, st))) return rc;

  const LogpD5Ws k = carve_logp_d5(h, B, n_pass, precision, ws_);
  const long long n = (long long)R * e, R4 = (R + 3) / 4 * 4;
  const float atol_f = (float)atol, rtol_f = (float)rtol;
  const unsigned rblocks = (unsigned)cdiv(R, 4);
  // kl[0] .. l_end are one contiguous block: delta_logp starts at zero and the padded tails stay zero through the solve
  HIP_TRY(hipMemsetAsync(k.kl[0], 0, (size_t)((char*)k.partial - (char*)k.kl[0]), st));

  // per-row labels of the forward (constant over the solve)
  logp::LabelArgs la{};
  const int64_t* lab_ptr[SCLDM_MAX_CLASSES] = {};
  for (int ci = 0; ci < c.n_classes; ++ci) {
    la.ulabels[ci] = (n_pass > 0 && ulabels) ? ulabels[ci] : nullptr;
    la.out[ci] = k.ev.labels + (size_t)ci * N;
    la.null_row[ci] = h->tab_rows[ci] - 1;
    lab_ptr[ci] = la.out[ci];
  }
  for (int p = 0; p < n_pass; ++p) la.mask[p] = pass_mask[p];
  la.cell_row = cell_row;
  la.n_classes = c.n_classes;
  la.B = B;
  la.P = n_pass;
  if (c.n_classes > 0) {
    logp::labels_kernel<<<cdiv(N, 256), 256, 0, st>>>(la);
    LAUNCH_CHECK();
  }

  logp::SeedArgs sa{};
  sa.xin = k.ev.xin; sa.dout = k.ev.dout; sa.eps = k.ev.eps; sa.t = k.ev.t;
  sa.B = B; sa.e = e; sa.P = n_pass;
  sa.coef_u = 1.0f;
  for (int p = 0; p < n_pass; ++p) {
    sa.scale[p] = pass_scale[p];
    sa.coef_u -= pass_scale[p];
  }
  sa.probe = probe;
  sa.g = logp::NoiseGeom{seed, cell_offset, cells_total, 0u};
  ld::Geom geom{};
  geom.out = k.ev.out; geom.dx = k.ev.dxr; geom.eps = k.ev.eps;
  geom.B = B; geom.e = e; geom.P = n_pass;
  for (int p = 0; p < n_pass; ++p) geom.scale[p] = pass_scale[p];

  float *KX[7], *KL[7];
  for (int i = 0; i < 7; ++i) { KX[i] = k.kx[i]; KL[i] = k.kl[i]; }
  // three state buffers in rotation: the start of the last accepted step (c0 of its interpolant), the current state, the stage point
  float *c0x = k.yx[1], *y0x = z, *stx = k.yx[0];
  float *c0l = k.yl[2], *y0l = k.yl[0], *stl = k.yl[1];

  // forward and seeded backward at state x and solver time s (the model sees t = 1 - s); `index` is the evaluation's place in execution
  // order (rejected steps included): it selects the probe, unless one probe serves the whole solve
  auto evaluate = [&](const float* x, float s, long long index) -> int {
    sa.x = x;
    sa.tval = 1.0f - s;
    sa.g.step = probe_per_solve ? 0u : (uint32_t)index;
    logp::seed_kernel<<<cdiv(N * (e / 4), 256), 256, 0, st>>>(sa);
    LAUNCH_CHECK();
    int rc = scldm_dit_train_forward(h, w, k.ev.xin, k.ev.t, c.n_classes > 0 ? lab_ptr : nullptr, (int)N, k.ev.out, precision, saved, ws_, st);
    if (rc) return rc;
    return scldm_dit_train_backward_dx(h, w, k.ev.xin, c.n_classes > 0 ? lab_ptr : nullptr, k.ev.dout, (int)N, k.ev.dxr, precision, saved, ws_, st);
  };
  // weights with their mask -> the compacted list the state kernels take
  auto comb = [&](const float* wt, unsigned mask) {
    ld::Comb a{};
    a.n_k = d5::compact(wt, mask, [&](int i, int j, float cj) { a.kx[i] = KX[j]; a.kl[i] = KL[j]; a.c[i] = cj; });
    return a;
  };
  auto slopes = [&](int slot, const float* y_fromx, const float* y_froml, float* outx, float* outl, const ld::Comb& cb) -> int {
    ld::StageArgs a{};
    a.g = geom;
    a.kx_new = KX[slot]; a.kl_new = KL[slot];
    a.y0x = y_fromx; a.y0l = y_froml; a.outx = outx; a.outl = outl;
    a.c = cb;
    ld::stage_kernel<<<rblocks, 256, 0, st>>>(a);
    LAUNCH_CHECK();
    return SCLDM_OK;
  };
  // mean over the packed state of ((a - b) / (atol + rtol |y0|))^2 -> mean[slot]
  auto norm = [&](const float* ax, const float* al, const float* bx, const float* bl, int slot) -> int {
    const ld::NormArgs a{ax, al, bx, bl, y0x, y0l, R, e, atol_f, rtol_f, k.partial};
    ld::norm_kernel<<<rblocks, 256, 0, st>>>(a);
    ld::mean_kernel<<<1, 256, 0, st>>>(k.partial, R, (double)R * (double)(e + 1), k.mean + slot);
    LAUNCH_CHECK();
    return SCLDM_OK;
  };

  // what dopri5_ctl.hpp's solve() calls, each in the order it enqueues
  auto first_slope = [&]() -> int {
    int rc;
    if ((rc = evaluate(y0x, 0.0f, 0))) return rc;
    return slopes(0, nullptr, nullptr, nullptr, nullptr, ld::Comb{});
  };
  auto start_norms = [&](double* ms) -> int {
    int rc;
    if ((rc = norm(y0x, y0l, nullptr, nullptr, 0))) return rc;
    if ((rc = norm(KX[0], KL[0], nullptr, nullptr, 1))) return rc;
    return dopri5_read_back(h->rk_host, k.mean, 2, ms, st);
  };
  auto trial = [&](double h0, double* ms) -> int {
    const float h0f = (float)h0;
    const float* kp[1] = {KX[0]};
    int rc;
    if ((rc = scldm_rk_combine(stx, y0x, kp, &h0f, 1, n, st))) return rc;   // y0 + h0 f0
    kp[0] = KL[0];
    if ((rc = scldm_rk_combine(stl, y0l, kp, &h0f, 1, R4, st))) return rc;
    if ((rc = evaluate(stx, (float)(0.0 + h0), 1))) return rc;
    if ((rc = slopes(1, nullptr, nullptr, nullptr, nullptr, ld::Comb{}))) return rc;
    if ((rc = norm(KX[1], KL[1], KX[0], KL[0], 0))) return rc;
    return dopri5_read_back(h->rk_host, k.mean, 1, ms, st);
  };
  auto save_time = [](int) { return 1.0; };   // the one save point that is formed (steps are never clipped to it)
  auto attempt = [&](const d5::Step& step, double* ms) -> int {
    const scldm_dopri5_plan& plan = step.plan;
    int rc;
    {   // the first stage point from the step's first slope (FSAL)
      const ld::Comb cb = comb(plan.a[0], plan.a_mask[0]);
      if ((rc = scldm_rk_combine(stx, y0x, cb.kx, cb.c, cb.n_k, n, st))) return rc;
      if ((rc = scldm_rk_combine(stl, y0l, cb.kl, cb.c, cb.n_k, R4, st))) return rc;
    }
    for (int i = 0; i < d5::kStages; ++i) {
      if ((rc = evaluate(stx, plan.t_stage[i], step.n_eval + i))) return rc;
      if (i + 1 < d5::kStages) {
        if ((rc = slopes(i + 1, y0x, y0l, stx, stl, comb(plan.a[i + 1], plan.a_mask[i + 1])))) return rc;
      } else {   // the last stage point is the 5th-order solution y1 (FSAL: K[6] = f(ta + h, y1))
        ld::ErrorArgs ea{};
        ea.g = geom;
        ea.kx_new = KX[6]; ea.kl_new = KL[6];
        ea.y0x = y0x; ea.y0l = y0l; ea.y1x = stx; ea.y1l = stl;
        ea.c = comb(plan.err, plan.err_mask);
        ea.atol = atol_f; ea.rtol = rtol_f;
        ea.partial = k.partial;
        ld::error_kernel<<<rblocks, 256, 0, st>>>(ea);
        ld::mean_kernel<<<1, 256, 0, st>>>(k.partial, R, (double)R * (double)(e + 1), k.mean);
        LAUNCH_CHECK();
      }
    }
    return dopri5_read_back(h->rk_host, k.mean, 1, ms, st);      // the step's one host read
  };
  auto accept = [&](const d5::Step& step, bool fit_dense) -> int {
    if (fit_dense) {   // s = 1 falls inside this step
      const scldm_dopri5_plan& plan = step.plan;
      const ld::Comb cb = comb(plan.mid, plan.mid_mask);
      int rc;
      if ((rc = scldm_rk_dense(y0x, stx, cb.kx, cb.c, cb.n_k, KX[0], KX[6], plan.h, plan.two_h, n, k.cx[0], k.cx[1], k.cx[2], k.cx[3], st))) return rc;
      if ((rc = scldm_rk_dense(y0l, stl, cb.kl, cb.c, cb.n_k, KL[0], KL[6], plan.h, plan.two_h, R4, k.cl[0], k.cl[1], k.cl[2], k.cl[3], st))) return rc;
    }
    float* freed = c0x;
    c0x = y0x; y0x = stx; stx = freed;
    freed = c0l;
    c0l = y0l; y0l = stl; stl = freed;
    std::swap(KX[0], KX[6]);
    std::swap(KL[0], KL[6]);
    return SCLDM_OK;
  };
  auto emit = [&](int, double s) -> int {
    const d5::Quartic q = d5::quartic_at(s);
    int rc;
    // (z may be the buffer c0 lives in: a thread writes the four elements it has just read, nothing else)
    if ((rc = scldm_rk_poly(z, c0x, k.cx[0], k.cx[1], k.cx[2], k.cx[3], q.s1, q.s2, q.s3, q.s4, n, st))) return rc;
    if ((rc = scldm_rk_poly(k.l_end, c0l, k.cl[0], k.cl[1], k.cl[2], k.cl[3], q.s1, q.s2, q.s3, q.s4, R4, st))) return rc;
    const float cz = (float)(-0.5 * (double)e * std::log(2.0 * 3.14159265358979323846));
    logp::final_kernel<<<rblocks, 256, 0, st>>>(z, k.l_end, R, e, cz, logp_out);
    LAUNCH_CHECK();
    if (dlogp_out) HIP_TRY(hipMemcpyAsync(dlogp_out, k.l_end, (size_t)R * sizeof(float), hipMemcpyDeviceToDevice, st));
    return SCLDM_OK;
  };
  auto reached = [&]() -> int {   // what the solve had reached
    if (y0x != z) HIP_TRY(hipMemcpyAsync(z, y0x, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (dlogp_out) HIP_TRY(hipMemcpyAsync(dlogp_out, y0l, (size_t)R * sizeof(float), hipMemcpyDeviceToDevice, st));
    return SCLDM_OK;
  };
  d5::Problem problem{first_slope, start_norms, trial, save_time, attempt, accept, emit, reached};
  return d5::solve(problem, first_step, 0, 1, step_log, step_log_cap, 4, stats);
}

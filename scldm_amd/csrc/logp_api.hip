// C ABI of the log-likelihood solve (scldm_logp_*; see include/scldm_hip.h and logp.hpp).  Host-side sequencing only: every
// evaluation is seed kernel -> scldm_dit_train_forward -> scldm_dit_train_backward_dx -> blend kernel, all launches on one stream.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <vector>

#include "api_common.hpp"
#include "cfg_plan.hpp"
#include "dit_handle.hpp"
#include "fixed_grid.hpp"
#include "logp.hpp"
#include "sde_transport.hpp"

using namespace scldm;

namespace {

struct LogpWs {
  float *xin, *t, *out, *dout, *dxr, *eps, *k1v, *ztmp, *k1l, *dl;
  int64_t* labels;   // [n_classes][N]
  size_t train_bytes, bytes;
};
LogpWs carve_logp(const scldm_dit* h, int B, int n_pass, int precision, void* base) {
  const size_t N = (size_t)(2 + n_pass) * B, e = (size_t)16 * h->cfg.n_embed_input, R = (size_t)2 * B;
  LogpWs w{};
  w.train_bytes = align256(scldm_dit_train_workspace_bytes_dx_for(h, (int)N, precision));
  size_t off = w.train_bytes;
  auto take = [&](size_t bytes) {
    void* p = base ? reinterpret_cast<char*>(base) + off : nullptr;
    off += align256(bytes);
    return p;
  };
  w.xin = (float*)take(N * e * 4);
  w.t = (float*)take(N * 4);
  w.labels = (int64_t*)take((size_t)SCLDM_MAX_CLASSES * N * 8);
  w.out = (float*)take(N * e * 4);
  w.dout = (float*)take(N * e * 4);
  w.dxr = (float*)take(N * e * 4);
  w.eps = (float*)take(R * e * 4);
  w.k1v = (float*)take(R * e * 4);
  w.ztmp = (float*)take(R * e * 4);
  w.k1l = (float*)take(R * 4);
  w.dl = (float*)take(R * 4);
  w.bytes = off;
  return w;
}

}  // namespace

extern "C" size_t scldm_logp_workspace_bytes(const scldm_dit* h, int B, int n_pass, int precision) {
  if (!h || B < 1 || n_pass < 0 || n_pass > SCLDM_MAX_CLASSES) return 0;
  return carve_logp(h, B, n_pass, precision, nullptr).bytes;
}

extern "C" int scldm_logp_probe(float* out, long long n_rows_local, int e, unsigned long long seed, int evaluation, int half,
                                long long cell_offset, long long cells_total, void* stream_) {
  if (!out || ((uintptr_t)out & 15)) return fail(SCLDM_ERR_SHAPE, "scldm_logp_probe: out must be a 16-byte aligned device pointer");
  if (n_rows_local < 1 || e < 4 || e % 4) return fail(SCLDM_ERR_SHAPE, "scldm_logp_probe: n_rows_local >= 1 and e a positive multiple of 4 (got %lld, %d)", n_rows_local, e);
  if (evaluation < 0 || (half != 0 && half != 1)) return fail(SCLDM_ERR_SHAPE, "scldm_logp_probe: evaluation >= 0 and half 0 | 1 (got %d, %d)", evaluation, half);
  if (cell_offset < 0 || cells_total < cell_offset + n_rows_local)
    return fail(SCLDM_ERR_SHAPE, "scldm_logp_probe: cells_total (%lld) < cell_offset (%lld) + n_rows_local (%lld)", cells_total, cell_offset, n_rows_local);
  const long long n4 = n_rows_local * (e / 4);
  if (n4 > 0x7fffffffll) return fail(SCLDM_ERR_SHAPE, "scldm_logp_probe: at most 2^33 elements per call");
  const logp::NoiseGeom g{seed, cell_offset, cells_total, (uint32_t)evaluation};
  logp::probe_kernel<<<cdiv(n4, 256), 256, 0, (hipStream_t)stream_>>>(out, n_rows_local, e, half, g);
  LAUNCH_CHECK();
  return SCLDM_OK;
}

// The fixed-grid likelihood solve.  tr == NULL: the default transport (Linear path, velocity model) over s in [0, 1] with blend_kernel;
// otherwise solver time runs over linspace(t0, t1, n_steps + 1), (t0, t1) = check_interval(sde=False, eval=True), and every
// evaluation ends in blend_transport_kernel with (a, b) of tpath::transport_coef at its model time t = fp32(1 - s).
static int logp_solve(scldm_dit* h, const scldm_dit_weights* w, float* z, const int64_t* const* ulabels, int n_urows,
                      const int32_t* cell_row, int B, int n_pass, const uint32_t* pass_mask, const float* pass_scale, int n_steps,
                      int method, const float* probe, unsigned long long seed, long long cell_offset, long long cells_total,
                      float* logp_out, float* dlogp_traj, int precision, void* saved, void* ws_, void* stream_, const scldm_transport* tr) {
  if (!h || !w || !z || !logp_out || !saved || !ws_) return fail(SCLDM_ERR_SHAPE, "scldm_logp_ode: null pointer argument");
  if (n_steps < 1) return fail(SCLDM_ERR_SHAPE, "n_steps must be >= 1");
  if (method != SCLDM_METHOD_EULER && method != SCLDM_METHOD_HEUN) return fail(SCLDM_ERR_SHAPE, "unknown method %d", method);
  if (cell_offset < 0 || cells_total < cell_offset + B) return fail(SCLDM_ERR_SHAPE, "cells_total (%lld) < cell_offset (%lld) + B (%d)", cells_total, cell_offset, B);
  CfgPlan pl;   // (the argument checks of every CFG entry; the solve blends in its own kernels and never takes the direct route)
  int rc = make_plan(h, pl, ulabels, n_urows, cell_row, B, n_pass, pass_mask, pass_scale, 0);
  if (rc) return rc;
  const scldm_dit_config& c = h->cfg;
  if (((uintptr_t)z & 15) || ((uintptr_t)probe & 15)) return fail(SCLDM_ERR_SHAPE, "z and probe must be 16-byte aligned");
  const int e = 16 * c.n_embed_input;
  const long long N = (long long)(2 + n_pass) * B;
  if (c.seq_len != 16 || e % 4 || N * (e / 4) > 0x7fffffffll || N > 0x7fffffffll) return fail(SCLDM_ERR_SHAPE, "state too large or unsupported shape");
  // the solver-time grid and, under a transport, every evaluation's (a, b, a e): formed and checked before anything is launched
  const int steps = n_steps + 1;
  float sa0 = 0.f, sb0 = 1.f;
  struct TCoef { float a, b, ae; };
  std::vector<TCoef> tc;
  if (tr) {
    if (tr->model != SCLDM_MODEL_VELOCITY && !(tr->sample_eps > 0.f))   // (as scldm_sample_ode_transport)
      return fail(SCLDM_ERR_SHAPE, "scldm_logp_ode_transport: a noise / score model needs sample_eps > 0: its drift is singular at t = 0 (alpha'/alpha) "
                  "and at t = 1 (noise: 1 / sigma)");
    double td0, td1;
    tpath::transport_interval(tr, true, &td0, &td1);
    sa0 = (float)td0;
    sb0 = (float)td1;
    const bool heun = method == SCLDM_METHOD_HEUN;
    for (int i = 0; i < n_steps; ++i)
      for (int j = 0; j < (heun ? 2 : 1); ++j) {
        const float t = 1.0f - grid::linspace(i + j, steps, sa0, sb0);
        scldm_transport_coef kc;
        tpath::transport_coef(tr->path, tr->model, tr->weight, (double)t, &kc);
        const double ae = kc.a * (double)e;
        if (!sdet::all_finite({kc.a, kc.b, ae}))
          return fail(SCLDM_ERR_SHAPE, "scldm_logp_ode_transport: %s", sdet::refusal((int)tc.size(), (double)t, "a, b of the probability-flow drift").c_str());
        tc.push_back(TCoef{(float)kc.a, (float)kc.b, (float)ae});
      }
  }
  hipStream_t st = (hipStream_t)stream_;
  const LogpWs k = carve_logp(h, B, n_pass, precision, ws_);
  const size_t row_e = (size_t)2 * B * e;

  // per-row labels of the forward (constant over the solve)
  logp::LabelArgs la{};
  const int64_t* lab_ptr[SCLDM_MAX_CLASSES] = {};
  for (int ci = 0; ci < c.n_classes; ++ci) {
    la.ulabels[ci] = (n_pass > 0 && ulabels) ? ulabels[ci] : nullptr;
    la.out[ci] = k.labels + (size_t)ci * N;
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
  HIP_TRY(hipMemsetAsync(k.dl, 0, (size_t)2 * B * sizeof(float), st));

  logp::SeedArgs sa{};
  sa.xin = k.xin; sa.dout = k.dout; sa.eps = k.eps; sa.t = k.t;
  sa.B = B; sa.e = e; sa.P = n_pass;
  sa.coef_u = 1.0f;
  for (int p = 0; p < n_pass; ++p) {
    sa.scale[p] = pass_scale[p];
    sa.coef_u -= pass_scale[p];
  }
  sa.g = logp::NoiseGeom{seed, cell_offset, cells_total, 0u};
  logp::BlendArgs ba{};
  ba.out = k.out; ba.dx = k.dxr; ba.eps = k.eps; ba.z = z; ba.ztmp = k.ztmp; ba.k1v = k.k1v; ba.k1l = k.k1l; ba.dl = k.dl;
  ba.B = B; ba.e = e; ba.P = n_pass;
  for (int p = 0; p < n_pass; ++p) ba.scale[p] = pass_scale[p];

  int e_idx = 0;
  // one evaluation at state `x` and solver time s: the model sees t = 1 - s
  auto eval = [&](const float* x, float s, int mode, float hs) -> int {
    const int ev = e_idx++;
    sa.x = x;
    sa.probe = probe ? probe + (size_t)ev * row_e : nullptr;
    sa.tval = 1.0f - s;
    sa.g.step = (uint32_t)ev;
    logp::seed_kernel<<<cdiv(N * (e / 4), 256), 256, 0, st>>>(sa);
    LAUNCH_CHECK();
    int rc = scldm_dit_train_forward(h, w, k.xin, k.t, c.n_classes > 0 ? lab_ptr : nullptr, (int)N, k.out, precision, saved, ws_, st);
    if (rc) return rc;
    rc = scldm_dit_train_backward_dx(h, w, k.xin, c.n_classes > 0 ? lab_ptr : nullptr, k.dout, (int)N, k.dxr, precision, saved, ws_, st);
    if (rc) return rc;
    ba.mode = mode;
    ba.hs = hs;
    ba.traj = dlogp_traj ? dlogp_traj + (size_t)ev * 2 * B : nullptr;
    if (tr) {
      const logp::BlendTransportArgs bt{ba, k.xin, tc[ev].a, tc[ev].b, tc[ev].ae};
      logp::blend_transport_kernel<<<cdiv(2 * B, 4), 256, 0, st>>>(bt);
    } else {
      logp::blend_kernel<<<cdiv(2 * B, 4), 256, 0, st>>>(ba);
    }
    LAUNCH_CHECK();
    return SCLDM_OK;
  };
  for (int i = 0; i < n_steps; ++i) {
    const float s0 = grid::linspace(i, steps, sa0, sb0), s1 = grid::linspace(i + 1, steps, sa0, sb0);
    const float hs = s1 - s0;
    if (method == SCLDM_METHOD_EULER) {
      if ((rc = eval(z, s0, logp::kEuler, hs))) return rc;
    } else {
      if ((rc = eval(z, s0, logp::kHeun1, hs))) return rc;
      if ((rc = eval(k.ztmp, s1, logp::kHeun2, 0.5f * hs))) return rc;
    }
  }
  const float c0 = (float)(-0.5 * (double)e * std::log(2.0 * 3.14159265358979323846));
  logp::final_kernel<<<cdiv(2 * B, 4), 256, 0, st>>>(z, k.dl, 2 * B, e, c0, logp_out);
  LAUNCH_CHECK();
  return SCLDM_OK;
}

extern "C" int scldm_logp_ode(scldm_dit* h, const scldm_dit_weights* w, float* z, const int64_t* const* ulabels, int n_urows,
                              const int32_t* cell_row, int B, int n_pass, const uint32_t* pass_mask, const float* pass_scale, int n_steps,
                              int method, const float* probe, unsigned long long seed, long long cell_offset, long long cells_total,
                              float* logp_out, float* dlogp_traj, int precision, void* saved, void* ws_, void* stream_) {
  return logp_solve(h, w, z, ulabels, n_urows, cell_row, B, n_pass, pass_mask, pass_scale, n_steps, method, probe, seed, cell_offset, cells_total,
                    logp_out, dlogp_traj, precision, saved, ws_, stream_, nullptr);
}

// ---- the same solve under any transport (sde_transport.hpp, transport_path.hpp) ---------------------------------------------------------
static bool is_default_transport(const scldm_transport* tr) { return tr->path == SCLDM_PATH_LINEAR && tr->model == SCLDM_MODEL_VELOCITY; }

extern "C" size_t scldm_logp_transport_workspace_bytes(const scldm_dit* h, int B, int n_pass, int precision, const scldm_transport* tr) {
  if (!tpath::transport_valid(tr)) return 0;
  return scldm_logp_workspace_bytes(h, B, n_pass, precision);   // the transport blend reads the forward's own input: no further buffer
}

extern "C" int scldm_logp_ode_transport(scldm_dit* h, const scldm_dit_weights* w, float* z, const int64_t* const* ulabels, int n_urows,
                                        const int32_t* cell_row, int B, int n_pass, const uint32_t* pass_mask, const float* pass_scale,
                                        int n_steps, int method, const float* probe, unsigned long long seed, long long cell_offset,
                                        long long cells_total, float* logp_out, float* dlogp_traj, int precision, void* saved, void* ws_,
                                        void* stream_, const scldm_transport* tr) {
  if (!tpath::transport_valid(tr))
    return fail(SCLDM_ERR_SHAPE, "scldm_logp_ode_transport: bad transport (Linear | GVP, velocity | noise | score, 0 <= eps < 0.5)");
  return logp_solve(h, w, z, ulabels, n_urows, cell_row, B, n_pass, pass_mask, pass_scale, n_steps, method, probe, seed, cell_offset, cells_total,
                    logp_out, dlogp_traj, precision, saved, ws_, stream_, is_default_transport(tr) ? nullptr : tr);
}

#include "logp_dopri5_api.inc"   // scldm_logp_ode_dopri5: the adaptive solve over the same evaluation

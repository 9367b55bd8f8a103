// Host side of the SDE sampler and the likelihood under any transport of transport_path.hpp (Linear | GVP x velocity | noise | score):
// plain C++, no HIP, no handle - the scalar algebra of one evaluation, in double, and the scan that refuses a solve before its first
// launch.  With m the CFG-blended model output at state x and model time t and (alpha, alpha', sigma, sigma', Dv, a, b) of
// tpath::transport_coef:
//   probability-flow drift   f_ode = a x + b m
//   score                    s = s_x x + s_m m:  velocity (-1/var, rr/var), rr = alpha / alpha', var = sigma^2 - rr sigma' sigma
//                                                score (0, 1)   noise (0, -1/sigma)                          (transport.py:185-202)
//   diffusion D(t)           SBDM norm Dv | sigma norm sigma | linear norm (1 - t) | constant norm | decreasing 0.25 (norm cos(pi t) + 1)^2
//                            | inccreasing-decreasing norm sin^2(pi t)                                       (path.py:52-77)
//   SDE drift                f = f_ode + D s = c_x x + c_m m
// so every update of a solve is x' = a_x x + a_m m + a_w w, the three scalars formed here and rounded to fp32 once by the caller.
// rr is formed from alpha and alpha' (never as 1 / ratio): it is 0 at t = 0.  At t = 1 the GVP path's sigma and alpha' are exactly 0;
// cos(pi / 2) in double is 6e-17, the rounding residue of pi, which would make a singular score look finite - the end point gets the
// exact zeros, so the refusal scan sees the singularity there.
#pragma once
#include <cmath>
#include <cstdio>
#include <initializer_list>
#include <string>

#include "transport_path.hpp"

namespace scldm {
namespace sdet {

struct Eval {   // what one evaluation at model time t contributes
  double D, a, b, s_x, s_m, c_x, c_m, alpha, sigma;
};

inline bool form_valid(int form) { return form >= SCLDM_SDE_FORM_SIGMA && form <= SCLDM_SDE_FORM_SBDM; }

inline Eval eval_at(const scldm_transport* tr, int form, double norm, double t) {
#pragma clang fp contract(off)
  const double pi = 3.14159265358979323846;
  scldm_transport_coef k;
  tpath::transport_coef(tr->path, tr->model, tr->weight, t, &k);
  if (tr->path == SCLDM_PATH_GVP && t >= 1.0) {   // the exact end point (see the head of this file)
    k.sigma = 0.0;
    k.d_alpha = 0.0;
    k.ratio = 0.0;
    k.dv = 0.0;
    if (tr->model != SCLDM_MODEL_VELOCITY) {
      k.a = 0.0;
      k.b = tr->model == SCLDM_MODEL_SCORE ? 0.0 : -k.dv / k.sigma;   // noise: 0 / 0
    }
  }
  Eval e{};
  e.alpha = k.alpha;
  e.sigma = k.sigma;
  e.a = k.a;
  e.b = k.b;
  switch (form) {
    case SCLDM_SDE_FORM_SBDM: e.D = norm * k.dv; break;
    case SCLDM_SDE_FORM_SIGMA: e.D = norm * k.sigma; break;
    case SCLDM_SDE_FORM_LINEAR: e.D = norm * (1.0 - t); break;
    case SCLDM_SDE_FORM_CONSTANT: e.D = norm; break;
    case SCLDM_SDE_FORM_DECREASING: { const double c = norm * cos(pi * t) + 1.0; e.D = 0.25 * c * c; break; }
    default: { const double s = sin(pi * t); e.D = norm * s * s; }   // SCLDM_SDE_FORM_INC_DEC
  }
  if (tr->model == SCLDM_MODEL_VELOCITY) {
    const double rr = k.alpha / k.d_alpha;
    const double var = k.sigma * k.sigma - rr * k.d_sigma * k.sigma;
    e.s_x = -1.0 / var;
    e.s_m = rr / var;
  } else if (tr->model == SCLDM_MODEL_SCORE) {
    e.s_x = 0.0;
    e.s_m = 1.0;
  } else {
    e.s_x = 0.0;
    e.s_m = -1.0 / k.sigma;
  }
  e.c_x = e.a + e.D * e.s_x;
  e.c_m = e.b + e.D * e.s_m;
  return e;
}

// the noise scale of a step at t: sqrt(2 D dt)
inline double noise_scale(const Eval& e, double dt) { return sqrt(2.0 * e.D * dt); }

// the last step x' = a_x x + a_m m at t1 (transport.py:240-267); false for an unknown last step (NONE included: no evaluation)
inline bool last_coef(const Eval& e, int last_step, double last_step_size, double* a_x, double* a_m) {
#pragma clang fp contract(off)
  switch (last_step) {
    case SCLDM_SDE_LAST_MEAN: *a_x = 1.0 + last_step_size * e.c_x; *a_m = last_step_size * e.c_m; return true;
    case SCLDM_SDE_LAST_EULER: *a_x = 1.0 + last_step_size * e.a; *a_m = last_step_size * e.b; return true;
    case SCLDM_SDE_LAST_TWEEDIE: {
      const double q = e.sigma * e.sigma / e.alpha;
      *a_x = 1.0 / e.alpha + q * e.s_x;
      *a_m = q * e.s_m;
      return true;
    }
    default: return false;
  }
}

// (t0, t1) of check_interval(..., sde=True, eval=True, last_step_size) in the fp32 the grid is built from (transport.py:69-95)
inline void sde_interval(const scldm_transport* tr, float last_step_size, float* t0, float* t1) {
  const bool vel = tr->model == SCLDM_MODEL_VELOCITY;
  *t0 = vel ? 0.f : tr->sample_eps;
  *t1 = (float)(1.0 - (double)((vel || last_step_size != 0.f) ? last_step_size : tr->sample_eps));
}

inline bool all_finite(std::initializer_list<double> v) {
  for (double x : v)
    if (!std::isfinite(x) || !std::isfinite((float)x)) return false;
  return true;
}
inline std::string refusal(int index, double t, const char* what) {
  char buf[256];
  std::snprintf(buf, sizeof buf, "evaluation %d of the solve, at t = %.9g, has a non-finite coefficient (%s): the transport is singular there", index, t, what);
  return buf;
}

}  // namespace sdet
}  // namespace scldm

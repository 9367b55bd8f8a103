// The interpolant paths of the reference's transport (src/scldm/transport/path.py:24-151 ICPlan, 190-208 GVPCPlan) and what its
// Transport derives from them (transport.py:69-202): the ONE place that knows the paths.  The training kernels call
// transport_coef once per batch row, the host calls it once per evaluation, scldm_transport_coef_at hands it to callers.
//
//            alpha         alpha'               sigma         sigma'                alpha'/alpha
//   Linear   t             1                    1 - t         -1                    1 / t
//   GVP      sin(pi t/2)   pi/2 cos(pi t/2)     cos(pi t/2)   -pi/2 sin(pi t/2)     pi / (2 tan(pi t/2))
//
//   Dv = (alpha'/alpha) sigma^2 - sigma sigma'                              compute_drift(...)[1]
//   loss row  w mean((c m - tgt)^2):  (c, tgt) = (1, ut) velocity | (1, x0) noise | (sigma, -x0) score
//             w = 1 | (Dv/sigma)^2 | Dv/sigma^2  for the weights none | velocity | likelihood; a velocity model ignores the weight
//   probability-flow drift  f = a x + b m:  (a, b) = (0, 1) velocity | (alpha'/alpha, Dv) score | (alpha'/alpha, -Dv/sigma) noise
// Everything is evaluated in double; a field the formula makes infinite at an end point (alpha'/alpha at t = 0) is returned as it
// comes, and a velocity model gets (a, b, c, w) = (0, 1, 1, 1) without reading one.
#pragma once
#include <cmath>

#include "../../include/scldm_hip.h"

#if defined(__HIPCC__)
#define SCLDM_HD __host__ __device__
#else
#define SCLDM_HD
#endif

namespace scldm {
namespace tpath {

// an unknown enum, the VP path, a negative eps or an eps >= 0.5 (the interval [eps, 1 - eps] would be empty) is refused
SCLDM_HD inline bool transport_valid(const scldm_transport* tr) {
  if (!tr) return false;
  if (tr->path != SCLDM_PATH_LINEAR && tr->path != SCLDM_PATH_GVP) return false;
  if (tr->model != SCLDM_MODEL_VELOCITY && tr->model != SCLDM_MODEL_NOISE && tr->model != SCLDM_MODEL_SCORE) return false;
  if (tr->weight != SCLDM_WEIGHT_NONE && tr->weight != SCLDM_WEIGHT_VELOCITY && tr->weight != SCLDM_WEIGHT_LIKELIHOOD) return false;
  if (!(tr->train_eps >= 0.f) || !(tr->train_eps < 0.5f) || !(tr->sample_eps >= 0.f) || !(tr->sample_eps < 0.5f)) return false;
  return true;
}

SCLDM_HD inline void transport_coef(int path, int model, int weight, double t, scldm_transport_coef* o) {
#pragma clang fp contract(off)   // the same doubles in every kernel and on the host, whatever the contraction mode of the including file
  const double half_pi = 1.5707963267948966;
  if (path == SCLDM_PATH_GVP) {
    const double s = sin(t * half_pi), c = cos(t * half_pi);
    o->alpha = s; o->d_alpha = half_pi * c; o->sigma = c; o->d_sigma = -half_pi * s;
    o->ratio = half_pi / tan(t * half_pi);
  } else {
    o->alpha = t; o->d_alpha = 1.0; o->sigma = 1.0 - t; o->d_sigma = -1.0;
    o->ratio = 1.0 / t;
  }
  o->dv = o->ratio * (o->sigma * o->sigma) - o->sigma * o->d_sigma;
  if (model == SCLDM_MODEL_VELOCITY) {
    o->a = 0.0; o->b = 1.0; o->c = 1.0; o->w = 1.0;
    return;
  }
  o->a = o->ratio;
  o->b = model == SCLDM_MODEL_SCORE ? o->dv : -o->dv / o->sigma;
  o->c = model == SCLDM_MODEL_SCORE ? o->sigma : 1.0;
  const double q = o->dv / o->sigma;
  o->w = weight == SCLDM_WEIGHT_VELOCITY ? q * q : weight == SCLDM_WEIGHT_LIKELIHOOD ? o->dv / (o->sigma * o->sigma) : 1.0;
}

// the time interval of check_interval (transport.py:69-95, sde=False): velocity models integrate and train over [0, 1]
inline void transport_interval(const scldm_transport* tr, bool eval, double* t0, double* t1) {
  const double eps = tr->model == SCLDM_MODEL_VELOCITY ? 0.0 : (double)(eval ? tr->sample_eps : tr->train_eps);
  *t0 = eps;
  *t1 = 1.0 - eps;
}

#if defined(__HIPCC__)
// What one batch row needs, rounded to fp32 once: xt = al x1 + sg x0, the loss target, and the row's {c, w}.
struct RowCoef { float al, sg, dal, dsg, c, w; };
__device__ __forceinline__ RowCoef row_coef(int path, int model, int weight, float t) {
  scldm_transport_coef k;
  transport_coef(path, model, weight, (double)t, &k);
  return RowCoef{(float)k.alpha, (float)k.sigma, (float)k.d_alpha, (float)k.d_sigma, (float)k.c, (float)k.w};
}
// every product rounded on its own, then the sum: the eager form's bits (fm_mix_kernel).  (__fmul_rn and its kin are plain operators to
// the compiler: each helper switches contraction off itself, so that it is the same instructions in every including file.)
__device__ __forceinline__ float plan_xt(const RowCoef& k, float x1, float x0) {
#pragma clang fp contract(off)
  const float p1 = k.al * x1, p0 = k.sg * x0;
  return p1 + p0;
}
__device__ __forceinline__ float plan_tgt(const RowCoef& k, int model, float x1, float x0) {
#pragma clang fp contract(off)
  if (model == SCLDM_MODEL_VELOCITY) {
    const float p1 = k.dal * x1, p0 = k.dsg * x0;
    return p1 + p0;
  }
  return model == SCLDM_MODEL_NOISE ? x0 : -x0;
}
// the weighted row loss w mean((c m - tgt)^2) and its gradient, the same roundings wherever they are formed
__device__ __forceinline__ float wl_diff(float c, float m, float tgt) {
#pragma clang fp contract(off)
  const float p = c * m;
  return p - tgt;
}
__device__ __forceinline__ float wl_row(float w, float sum, int e) {
#pragma clang fp contract(off)
  const float mean = sum / (float)e;
  return w * mean;
}
__device__ __forceinline__ float wl_grad(float gloss, float w, float k, float c, float d) {
#pragma clang fp contract(off)
  return gloss * w * k * c * d;      // left to right, each product rounded
}
#endif

}  // namespace tpath
}  // namespace scldm

// Host-side controller of the adaptive Dormand-Prince 5(4) solve (scldm_sample_ode_dopri5): plain C++, no HIP, no handle.  It restates, in
// the same float64 operations and the same order, what scldm_amd.transport.Sampler._sample_dopri5 does between its kernel launches - the
// tableau weights handed to the state kernels, the accept / next-step rule and the automatic initial step - so the fused solve and the
// host-composed one take identical decisions from identical error ratios.  The scldm_dopri5_stage_plan / _control / _initial_h0 /
// _initial_step entries of the C ABI are thin wrappers over these functions: the controller is testable on a machine without a GPU.
#pragma once
#include <cmath>

#include "../../include/scldm_hip.h"

#pragma clang fp contract(off)   // every product and sum rounded on its own, as Python's float arithmetic

namespace scldm {
namespace dopri5 {

// Dormand & Prince (1980) 5(4) with Shampine's error weights and torchdiffeq's mid-point weights: the literals of
// scldm_amd/transport/__init__.py (_DP_A, _DP_C, _DP_E, _DP_MID), written as the same quotients so they round to the same doubles
constexpr int kStages = 6;   // new evaluations per attempted step (FSAL: the first slope is the last one of the step before)
static const double kA[6][6] = {{1.0 / 5, 0, 0, 0, 0, 0},
                                {3.0 / 40, 9.0 / 40, 0, 0, 0, 0},
                                {44.0 / 45, -56.0 / 15, 32.0 / 9, 0, 0, 0},
                                {19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729, 0, 0},
                                {9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656, 0},
                                {35.0 / 384, 0.0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84}};
static const double kC[6] = {1.0 / 5, 3.0 / 10, 4.0 / 5, 8.0 / 9, 1.0, 1.0};
static const double kE[7] = {35.0 / 384 - 1951.0 / 21600, 0.0, 500.0 / 1113 - 22642.0 / 50085, 125.0 / 192 - 451.0 / 720,
                             -2187.0 / 6784 - -12231.0 / 42400, 11.0 / 84 - 649.0 / 6300, -1.0 / 60.0};
static const double kMid[7] = {6025192743.0 / 30085553152.0 / 2, 0.0, 51252292925.0 / 65400821598.0 / 2, -2691868925.0 / 45128329728.0 / 2,
                               187940372067.0 / 1594534317056.0 / 2, -1776094331.0 / 19743644256.0 / 2, 11237099.0 / 235043384.0 / 2};

// Everything the state kernels of one attempted step from t0 with size h are handed: stage i (0-based, the (i + 2)-th slope) is evaluated
// at fp32(t0 + c_i h) (t0 + h where c_i == 1) on the point y0 + sum_j a[i][j] k_j; each weight is (float)(h * w) formed in double, and a
// mask bit is clear where the tableau entry is a structural zero (such terms are skipped, not multiplied by zero)
inline void stage_plan(double t0, double h, scldm_dopri5_plan* p) {
  for (int i = 0; i < kStages; ++i) {
    p->t_stage[i] = (float)(kC[i] == 1.0 ? t0 + h : t0 + kC[i] * h);
    p->a_mask[i] = 0;
    for (int j = 0; j < 7; ++j) {
      const double w = (j <= i) ? kA[i][j] : 0.0;
      p->a[i][j] = (float)(h * w);
      if (w != 0.0) p->a_mask[i] |= 1u << j;
    }
  }
  p->err_mask = p->mid_mask = 0;
  for (int j = 0; j < 7; ++j) {
    p->err[j] = (float)(h * kE[j]);
    p->mid[j] = (float)(h * kMid[j]);
    if (kE[j] != 0.0) p->err_mask |= 1u << j;
    if (kMid[j] != 0.0) p->mid_mask |= 1u << j;
  }
  p->h = (float)h;
  p->two_h = (float)(2 * h);
}

// Python's min / max of two floats (they keep the FIRST argument unless the second compares smaller / larger: a NaN is handled as there)
inline double pymin(double a, double b) { return b < a ? b : a; }
inline double pymax(double a, double b) { return b > a ? b : a; }

// After an attempted step from t0 with size h whose mixed rms error ratio is `ratio`: accept iff ratio <= 1; the next step starts at
// t1 = t0 + h (accepted) or t0 again; its size is h * 10 for ratio == 0, otherwise h * min(10, max(0.9 / ratio^0.2, ratio < 1 ? 1 : 0.2));
// underflow: that next step cannot advance the time (t1 + h_next == t1), or is not a number
inline void control(double t0, double h, double ratio, scldm_dopri5_control_out* c) {
  c->accepted = ratio <= 1.0 ? 1 : 0;
  c->t1 = c->accepted ? t0 + h : t0;
  if (ratio == 0.0) c->h_next = h * 10.0;
  else c->h_next = h * pymin(10.0, pymax(0.9 / std::pow(ratio, 0.2), ratio < 1.0 ? 1.0 : 0.2));
  c->underflow = (c->t1 + c->h_next > c->t1) ? 0 : 1;
}

// Hairer / Norsett / Wanner II.4 with the rms norm and exponent 1 / 5.  d0 = rms(y0 / scale), d1 = rms(f0 / scale),
// scale = atol + rtol |y0|: the trial step h0; then d2 = rms((f(t0 + h0, y0 + h0 f0) - f0) / scale) / h0: the first step
inline double initial_h0(double d0, double d1) { return (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1; }
inline double initial_step(double h0, double d1, double d2) {
  const double h1 = (d1 <= 1e-15 && d2 <= 1e-15) ? pymax(1e-6, h0 * 1e-3) : std::pow(0.01 / pymax(d1, d2), 1.0 / 5.0);
  return pymin(100.0 * h0, h1);
}

}  // namespace dopri5
}  // namespace scldm

// Host side of the fused adaptive Dormand-Prince 5(4) solves (scldm_sample_ode_dopri5, scldm_logp_ode_dopri5): plain C++, no HIP, no
// handle.  It restates, in the same float64 operations and the same order, what scldm_amd.transport.Sampler._sample_dopri5 does between
// its kernel launches - the tableau weights handed to the state kernels, the accept / next-step rule, the automatic initial step and, in
// solve() at the end of this file, the step loop itself - so the fused solves and the host-composed one take identical decisions from
// identical error ratios.  The scldm_dopri5_stage_plan / _control / _initial_h0 / _initial_step entries of the C ABI are thin wrappers
// over these functions, and tests/dopri5_driver_shim.cpp gives solve() a C face: all of it is tested on a machine without a GPU.
#pragma once
#include <cmath>
#include <cstddef>

#include "../../include/scldm_hip.h"

int scldm_fail(int code, const char* fmt, ...);   // records the message of scldm_last_error() (api.hip; a test shim brings its own)

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

// libm's pow as a call the optimiser cannot rewrite (pow(x, 0.5) would become a square root: correctly rounded, where the host-composed
// solver's Python `x ** 0.5` is libm's pow - the two routes have to take the same decisions from the same doubles)
inline double libm_pow(double x, double y) {
  volatile double yv = y;
  return std::pow(x, yv);
}

// weights with their mask -> keep(i, j, w[j]) for the i-th slope j that is not a structural zero; the number kept.  The state kernels
// take such compacted (pointer, coefficient) lists, each solve in its own struct
template <class Keep>
inline int compact(const float* w, unsigned mask, Keep&& keep) {
  int n = 0;
  for (int j = 0; j < 7; ++j)
    if ((mask >> j) & 1u) keep(n++, j, w[j]);
  return n;
}

// where the quartic interpolant of an accepted step is evaluated: s in [0, 1] held in double, its powers rounded to fp32 once each
struct Quartic {
  float s1, s2, s3, s4;
};
inline Quartic quartic_at(double s) { return Quartic{(float)s, (float)(s * s), (float)(s * s * s), (float)(s * s * s * s)}; }

struct Step {               // one attempted step as the problem sees it
  double t0, h;             // float64, as the decisions hold them; the state kernels take the plan's fp32 roundings
  long long n_eval;         // evaluations made before this step, rejected steps included
  scldm_dopri5_plan plan;
};
// What differs between the solves, as callables (each entry passes its lambdas).  All but save_time return an SCLDM_* code.
template <class FirstSlope, class StartNorms, class Probe, class SaveTime, class Attempt, class Accept, class Emit, class Reached>
struct Problem {
  FirstSlope first_slope;   // ()                          f(0, y0) into slope 0
  StartNorms start_norms;   // (double ms[2])              the mean squares of y0 / scale and f0 / scale, scale = atol + rtol |y0|
  Probe probe;              // (double h0, double* ms)     y0 + h0 f0, its evaluation at (float)(0 + h0) into slope 1, the mean square of (f1 - f0) / scale
  SaveTime save_time;       // (int si) -> double
  Attempt attempt;          // (const Step&, double* ms)   the step's six evaluations and its one host read: the mean squared error ratio
  Accept accept;            // (const Step&, bool fit)     fit the interpolant (THIS step's weights) if asked, then end -> current state, last slope -> first
  Emit emit;                // (int si, double s)          save point si from the last accepted step's interpolant at s (quartic_at)
  Reached reached;          // ()                          the solve failed: hand out the current state
};
template <class... F>
Problem(F...) -> Problem<F...>;

// The step loop of both fused solves: the first step, attempted steps until every save time first_save .. num_save - 1 lies inside an
// accepted one (time runs from 0; steps are never clipped to a save time), the statistics and the step log (NULL, or step_log_cap rows
// of log_stride doubles: t0, h, accepted (1.0 / 0.0) and, with 4, the error ratio).  The float64 decisions are Sampler._sample_dopri5's,
// in its order.  A problem's non-zero code ends the solve and is returned as it is, stats untouched; SCLDM_ERR_SOLVER comes with stats.
template <class P>
int solve(P& p, double first_step, int first_save, int num_save, double* step_log, int step_log_cap, int log_stride, scldm_dopri5_stats* stats) {
  int rc;
  scldm_dopri5_stats n{};   // the counters, in the struct they are reported in
  if ((rc = p.first_slope())) return rc;
  n.evaluations = 1;
  double hstep = first_step;
  if (!(first_step > 0.0)) {
    double ms[2];
    if ((rc = p.start_norms(ms))) return rc;
    const double dn0 = std::sqrt(ms[0]), dn1 = std::sqrt(ms[1]);
    const double h0 = initial_h0(dn0, dn1);
    if ((rc = p.probe(h0, ms))) return rc;
    ++n.evaluations;
    hstep = initial_step(h0, dn1, std::sqrt(ms[0]) / h0);
  }
  n.first_step = hstep;
  double t0 = 0.0, t1 = 0.0;
  bool underflow = !(t1 + hstep > t1);
  for (int si = first_save; si < num_save && n.status == SCLDM_DOPRI5_OK; ++si) {
    const double next_t = p.save_time(si);
    while (next_t > t1) {   // advance until the save time lies inside the last accepted step
      if (underflow) { n.status = SCLDM_DOPRI5_UNDERFLOW; break; }
      if (n.evaluations > 100000) { n.status = SCLDM_DOPRI5_MAX_EVALS; break; }
      Step step{t1, hstep, n.evaluations, {}};
      stage_plan(step.t0, step.h, &step.plan);
      double ms;
      if ((rc = p.attempt(step, &ms))) return rc;
      n.evaluations += kStages;
      const double ratio = libm_pow(ms, 0.5);
      scldm_dopri5_control_out co;
      control(step.t0, step.h, ratio, &co);
      if (step_log && n.step_log_len < step_log_cap) {
        double* row = step_log + (size_t)log_stride * n.step_log_len++;
        row[0] = step.t0;
        row[1] = step.h;
        row[2] = co.accepted ? 1.0 : 0.0;
        if (log_stride > 3) row[3] = ratio;
      }
      if (co.accepted) {
        ++n.accepted;
        if ((rc = p.accept(step, next_t <= co.t1))) return rc;
        t0 = step.t0;
        t1 = co.t1;
      } else ++n.rejected;
      hstep = co.h_next;
      underflow = co.underflow != 0;
    }
    if (n.status != SCLDM_DOPRI5_OK) break;
    if ((rc = p.emit(si, (next_t - t0) / (t1 - t0)))) return rc;
  }
  if (n.status != SCLDM_DOPRI5_OK && (rc = p.reached())) return rc;
  if (stats) *stats = n;
  if (n.status == SCLDM_DOPRI5_UNDERFLOW) return scldm_fail(SCLDM_ERR_SOLVER, "dopri5: step size underflow / too many evaluations (t = %.17g, h = %.3g)", t1, hstep);
  if (n.status == SCLDM_DOPRI5_MAX_EVALS) return scldm_fail(SCLDM_ERR_SOLVER, "dopri5: step size underflow / too many evaluations (%lld evaluations)", n.evaluations);
  return SCLDM_OK;
}

}  // namespace dopri5
}  // namespace scldm


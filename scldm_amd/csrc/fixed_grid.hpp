// Host side of the fixed-grid solves (scldm_sample_ode, scldm_sample_sde / _transport, scldm_sample_ode_transport, scldm_logp_ode / _transport,
// scldm_dit_infer_sample_ode): plain C++, no HIP, no handle - the fp32 time grid, the list of a solve's evaluation times and the
// Euler / Heun step loop over caller-supplied launches.  tests/fixed_grid_shim.cpp gives it a C face, so all of it is tested on a
// machine without a GPU (a sibling of dopri5_ctl.hpp).
#pragma once
#include <cstddef>
#include <vector>

namespace scldm {
namespace grid {

// torch.linspace(a, b, steps)[idx] in fp32 (integrators.py:23-24, :95): step = (b - a) / (steps - 1), the lower half filled upwards from
// a and the upper half downwards from b, every product and sum rounded on its own.  With a == 0 this is bit for bit the (0, b) form
// step * idx of a grid that starts at zero, so one function serves [0, 1], [0, 1 - last_step_size] and [eps, 1 - eps].
inline float linspace(int idx, int steps, float a, float b) {
#pragma clang fp contract(off)
  const float step = (b - a) / (float)(steps - 1);
  return (idx < steps / 2) ? a + step * (float)idx : b - step * (float)(steps - idx - 1);
}

// Where a step's second evaluation sits.
enum Second {
  kNone = 0,     // Euler: one evaluation per step, at t[i]
  kNext = 1,     // Heun: t[i], t[i + 1]
  kPlusDt = 2,   // the SDE's Heun (integrators.py:40-57): t[i], fp32(t[i] + dt) with dt = t[1] - t[0] for every step
};

// The time of every evaluation of a solve of n_steps steps over linspace(a, b, n_steps + 1), in the order they run; `last` (optional)
// appends the time of one trailing evaluation (the SDE's last step).
inline std::vector<float> eval_times(int n_steps, float a, float b, Second second, const float* last = nullptr) {
#pragma clang fp contract(off)
  const int steps = n_steps + 1;
  const float dt = linspace(1, steps, a, b) - linspace(0, steps, a, b);
  std::vector<float> tl;
  tl.reserve((std::size_t)(second == kNone ? 1 : 2) * n_steps + (last ? 1 : 0));
  for (int i = 0; i < n_steps; ++i) {
    const float t = linspace(i, steps, a, b);
    tl.push_back(t);
    if (second == kNext) tl.push_back(linspace(i + 1, steps, a, b));
    else if (second == kPlusDt) tl.push_back(t + dt);
  }
  if (last) tl.push_back(*last);
  return tl;
}

// The state buffers of the loop below: z is the state (updated in place), the rest is scratch of the same size (Heun only).
struct Buffers {
  float *z, *k1, *k2, *ztmp;
};

// Euler / Heun over linspace(a, b, n_steps + 1), hs = t[i + 1] - t[i] in fp32.  The caller supplies the launches, each returning 0 or an
// error code that ends the loop:
//   eval(e, zin, out, euler_z, hs)   evaluation e (the index into eval_times' list) at the state zin, slope -> out; with euler_z given the
//                                    same launch also applies euler_z += hs * slope (Euler: one launch less per step)
//   axpy(z, k, out, hs)              out = z + hs k
//   heun(z, k1, k2, half_hs)         z += half_hs (k1 + k2)
template <class Eval, class Axpy, class Heun>
int euler_heun(int n_steps, float a, float b, bool second_order, const Buffers& s, Eval&& eval, Axpy&& axpy, Heun&& heun) {
#pragma clang fp contract(off)
  const int steps = n_steps + 1;
  int rc;
  for (int i = 0; i < n_steps; ++i) {
    const float hs = linspace(i + 1, steps, a, b) - linspace(i, steps, a, b);
    if (!second_order) {
      if ((rc = eval(i, s.z, s.k1, s.z, hs))) return rc;
    } else {
      if ((rc = eval(2 * i, s.z, s.k1, nullptr, 0.f))) return rc;
      if ((rc = axpy(s.z, s.k1, s.ztmp, hs))) return rc;
      if ((rc = eval(2 * i + 1, s.ztmp, s.k2, nullptr, 0.f))) return rc;
      if ((rc = heun(s.z, s.k1, s.k2, 0.5f * hs))) return rc;
    }
  }
  return 0;
}

}  // namespace grid
}  // namespace scldm

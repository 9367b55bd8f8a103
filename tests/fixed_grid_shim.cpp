// A C face for the host side of the fixed-grid solves (scldm_amd/csrc/fixed_grid.hpp: linspace, eval_times, euler_heun), for
// tests/test_fixed_grid_cpu.py: the test reads the shipped grid and drives the shipped step loop with recording callbacks on a
// machine without a GPU.  Not part of the library.
#include "../scldm_amd/csrc/fixed_grid.hpp"

extern "C" {

float fixed_grid_linspace(int idx, int steps, float a, float b) { return scldm::grid::linspace(idx, steps, a, b); }

// out: room for 2 * n_steps + 1 floats; returns the number of evaluation times written
int fixed_grid_eval_times(int n_steps, float a, float b, int second, int has_last, float last, float* out) {
  const std::vector<float> tl = scldm::grid::eval_times(n_steps, a, b, (scldm::grid::Second)second, has_last ? &last : nullptr);
  for (std::size_t i = 0; i < tl.size(); ++i) out[i] = tl[i];
  return (int)tl.size();
}

struct shim_ops {
  int (*eval)(int e, const float* zin, float* out, float* euler_z, float hs);
  int (*axpy)(const float* z, const float* k, float* out, float hs);
  int (*heun)(float* z, const float* k1, const float* k2, float half_hs);
};

int fixed_grid_euler_heun(int n_steps, float a, float b, int second_order, float* z, float* k1, float* k2, float* ztmp, const shim_ops* ops) {
  return scldm::grid::euler_heun(n_steps, a, b, second_order != 0, scldm::grid::Buffers{z, k1, k2, ztmp}, ops->eval, ops->axpy, ops->heun);
}

}  // extern "C"

// A C face for the step loop of the fused dopri5 solves (scldm::dopri5::solve in scldm_amd/csrc/dopri5_ctl.hpp), for
// tests/test_dopri5_fused_cpu.py: a problem whose members are function pointers, so the test drives the shipped loop with float64
// numpy state arithmetic on a machine without a GPU.  Not part of the library.
#include <cstdarg>
#include <cstdio>

#include "../scldm_amd/csrc/dopri5_ctl.hpp"

static char g_message[256];
int scldm_fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(g_message, sizeof g_message, fmt, ap);
  va_end(ap);
  return code;
}

extern "C" {

struct shim_callbacks {
  int (*first_slope)();
  int (*start_norms)(double* ms);
  int (*probe)(double h0, double* ms);
  double (*save_time)(int si);
  int (*attempt)(const scldm::dopri5::Step* step, double* ms);
  int (*accept)(const scldm::dopri5::Step* step, int fit_dense);
  int (*emit)(int si, double s);
  int (*reached)();
};

const char* dopri5_shim_message() { return g_message; }

int dopri5_shim_solve(const shim_callbacks* cb, double first_step, int first_save, int num_save, double* step_log, int step_log_cap,
                      int log_stride, scldm_dopri5_stats* stats) {
  namespace d5 = scldm::dopri5;
  d5::Problem p{cb->first_slope, cb->start_norms, cb->probe, cb->save_time,
                [cb](const d5::Step& step, double* ms) { return cb->attempt(&step, ms); },
                [cb](const d5::Step& step, bool fit_dense) { return cb->accept(&step, fit_dense ? 1 : 0); }, cb->emit, cb->reached};
  g_message[0] = 0;
  return d5::solve(p, first_step, first_save, num_save, step_log, step_log_cap, log_stride, stats);
}

}  // extern "C"

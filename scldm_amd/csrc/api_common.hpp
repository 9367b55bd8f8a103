// Shared host-side helpers of the C ABI translation units.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstddef>
#include <cstdio>

#include "../../include/scldm_hip.h"

int scldm_fail(int code, const char* fmt, ...);   // records the thread-local message returned by scldm_last_error()
#define fail scldm_fail
#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess) return fail(SCLDM_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)
#define LAUNCH_CHECK()                                                                             \
  do {                                                                                             \
    hipError_t e_ = hipGetLastError();                                                             \
    if (e_ != hipSuccess) return fail(SCLDM_ERR_HIP, "kernel launch failed: %s (%s:%d)", hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

static inline size_t align256(size_t v) { return (v + 255) & ~size_t(255); }
static inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

// What the two fused dopri5 entries (dopri5_api.inc, logp_dopri5_api.inc) check alike, under the entry's name: first without a HIP call,
static inline int dopri5_check_tolerances(const char* entry, double atol, double rtol, const double* step_log, int step_log_cap) {
  if (!(atol > 0.0) || !(rtol >= 0.0)) return fail(SCLDM_ERR_SHAPE, "%s: atol must be > 0 and rtol >= 0 (got %g, %g)", entry, atol, rtol);
  if (step_log && step_log_cap < 0) return fail(SCLDM_ERR_SHAPE, "%s: step_log_cap must be >= 0", entry);
  return SCLDM_OK;
}
// then, last of all checks, the handle's pinned read-back slot and the stream
static inline int dopri5_check_stream(const char* entry, const volatile double* slot, hipStream_t st) {
  if (!slot) return fail(SCLDM_ERR_STATE, "%s: the handle has no read-back slot", entry);
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  HIP_TRY(hipStreamIsCapturing(st, &cap));
  if (cap != hipStreamCaptureStatusNone)
    return fail(SCLDM_ERR_SHAPE, "%s: the stream is capturing - the solve reads its error ratio once per step and cannot be captured into a graph", entry);
  return SCLDM_OK;
}
// `count` consecutive device doubles -> out through that slot: one copy, one stream synchronise
static inline int dopri5_read_back(volatile double* slot, const double* dev, int count, double* out, hipStream_t st) {
  HIP_TRY(hipMemcpyAsync((void*)slot, dev, (size_t)count * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  for (int i = 0; i < count; ++i) out[i] = slot[i];
  return SCLDM_OK;
}

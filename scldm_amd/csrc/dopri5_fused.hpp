// State kernels of the fused adaptive Dormand-Prince 5(4) solve (scldm_sample_ode_dopri5 in dopri5_api.inc).  The host-composed solver
// (scldm_amd/transport: Sampler._sample_dopri5 over DiT.forward_with_cfg) runs, after the trunk of every evaluation, cfg_blend_kernel and
// then - as separate launches through ctypes - rk::combine_kernel for the next stage point, or rk::error_kernel after the seventh slope.
// Here the blend rides in the kernel that consumes it:
//   blend_stage_kernel  k_i = CFG blend of the trunk output;  next stage point = ((y0 + c0 k0) + c1 k1) + ... + c_i k_i
//   blend_error_kernel  k_7 = CFG blend;  per-block double partials of sum((err / (atol + rtol max(|y0|, |y1|)))^2)
// Every value is produced by the operations of the kernels they replace, in their order: the blend through cfg_blend_term (dit_aux.hpp,
// that header's contraction mode), everything else with each product and sum rounded on its own (contraction off, as ode_rk.hpp), the
// error sum with error_kernel's grid, element-to-thread map and reduction tree - so rk::error_final_kernel returns scldm_rk_error's bits.
#pragma once
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "dit_aux.hpp"
#include "ode_rk.hpp"

#pragma clang fp contract(off)

namespace scldm {
namespace dopri5 {

// where the trunk left its output: 2B unconditional rows, then P conditional passes of B rows (direct: 2B rows, the result itself)
struct BlendGeom {
  const float* v;
  int B, e, P, direct;
  float scale[kMaxClasses];
};

// the blended slope of elements [4q, 4q + 4) of the (2B, e) state; e % 4 == 0, so the four never straddle the two halves
__device__ __forceinline__ f32x4 blend4(const BlendGeom& g, size_t q, size_t half4) {
  const f32x4* v4 = reinterpret_cast<const f32x4*>(g.v);
  f32x4 r = v4[q];
  if (!g.direct && q >= half4) {
    const f32x4* vc = v4 + 2 * half4 + (q - half4);   // pass 0 of these elements; pass p is p * half4 further
    const f32x4 u = r;
    for (int p = 0; p < g.P; ++p) r = cfg_blend_term(r, vc[(size_t)p * half4], u, g.scale[p]);
  }
  return r;
}

// c: the slopes of the next stage point in tableau order, structural zeros left out; its LAST entry is the slope this kernel forms (taken
// from the register, c.k of it is not read).  out == nullptr: the slope alone (the first evaluation of a solve, the initial-step probe)
struct StageArgs {
  BlendGeom g;
  float* k_new;
  float* out;
  const float* y0;
  rk::CombArgs c;
};
__global__ __launch_bounds__(256) void blend_stage_kernel(const StageArgs a) {
  const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t half4 = ((size_t)a.g.B * a.g.e) >> 2;
  if (q >= 2 * half4) return;
  const f32x4 r = blend4(a.g, q, half4);
  reinterpret_cast<f32x4*>(a.k_new)[q] = r;
  if (!a.out) return;
  f32x4 acc = reinterpret_cast<const f32x4*>(a.y0)[q];
#pragma unroll
  for (int j = 0; j < rk::kMaxK; ++j)
    if (j < a.c.n_k) {
      const f32x4 kv = (j == a.c.n_k - 1) ? r : reinterpret_cast<const f32x4*>(a.c.k[j])[q];
      acc = acc + kv * a.c.c[j];    // (combine_kernel's statement)
    }
  reinterpret_cast<f32x4*>(a.out)[q] = acc;
}

// The seventh slope and the error partials.  The double sum of a thread, of a wave and of a workgroup is the contract here (floating-point
// addition is not associative), so the kernel keeps error_kernel's map - element i belongs to thread i mod (256 gridDim.x), visited in
// rising order - and with it that kernel's 4-byte accesses (a wave still touches 256 consecutive bytes per instruction).
struct ErrorArgs {
  BlendGeom g;
  float* k_new;
  const float* y0;
  const float* y1;
  rk::CombArgs c;      // error weights, structural zeros left out, the new slope last
  long n;
  float atol, rtol;
  double* partial;
};
__global__ __launch_bounds__(256) void blend_error_kernel(const ErrorArgs a) {
  __shared__ double red[4];
  const size_t half = (size_t)a.g.B * a.g.e;
  double s = 0.0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (long)gridDim.x * 256) {
    float r = a.g.v[i];
    if (!a.g.direct && (size_t)i >= half) {
      const float u = r;
      for (int p = 0; p < a.g.P; ++p) r = cfg_blend_term(r, a.g.v[2 * half + (size_t)p * half + ((size_t)i - half)], u, a.g.scale[p]);
    }
    a.k_new[i] = r;
    float e = 0.f;
#pragma unroll
    for (int j = 0; j < rk::kMaxK; ++j)
      if (j < a.c.n_k) {
        const float t = ((j == a.c.n_k - 1) ? r : a.c.k[j][i]) * a.c.c[j];
        e = j == 0 ? t : e + t;
      }
    const float den = a.atol + a.rtol * fmaxf(fabsf(a.y0[i]), fabsf(a.y1[i]));
    const double q = (double)(e / den);
    s += q * q;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) a.partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// The three norms of the automatic initial step: partial[block] = sum(((a - b) / (atol + rtol |y0|))^2) in double (b == nullptr: a alone);
// rk::error_final_kernel then leaves the mean.  One fp32 difference and one fp32 quotient per element, as the composed expressions
// (f1 - f0) / scale and y0 / scale; the order of the double sum is this kernel's own (the composed route leaves it to a library reduction)
__global__ __launch_bounds__(256) void scaled_norm_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ y0, long n4,
                                                          float atol, float rtol, double* __restrict__ partial) {
  __shared__ double red[4];
  double s = 0.0;
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < n4; q += (long)gridDim.x * 256) {
    f32x4 x = reinterpret_cast<const f32x4*>(a)[q];
    if (b) x = x - reinterpret_cast<const f32x4*>(b)[q];
    const f32x4 y = reinterpret_cast<const f32x4*>(y0)[q];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const double r = (double)(x[c] / (atol + rtol * fabsf(y[c])));
      s += r * r;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// the fp32 times of up to eight evaluations, handed over by value (no host-to-device copy between the launches of a step)
struct Times { float t[8]; };
__global__ void set_times_kernel(float* __restrict__ tlist, const Times c, int n) {
  if ((int)threadIdx.x < n) tlist[threadIdx.x] = c.t[threadIdx.x];
}

}  // namespace dopri5
}  // namespace scldm
// (contraction stays off past this header, as ode_rk.hpp and sde.hpp leave it)

// State kernels of the adaptive log-likelihood solve (scldm_logp_ode_dopri5 in logp_dopri5_api.inc): Dormand-Prince 5(4) over the augmented
// state (x (2B, e), delta_logp (2B)) with the slopes (-v, logp_grad) of logp.hpp's evaluation.  After the recording forward and the
// input-gradient-only backward of an evaluation ONE kernel consumes their outputs, one wave per state row as logp::blend_kernel:
//   stage_kernel   k = (-v, logp_grad) of the row;  when asked, the next stage point ((y0 + c0 k0) + c1 k1) + ... for the row's x
//                  elements and its delta_logp (rk::combine_kernel's statement, stage_plan's weights, structural zeros left out)
//   error_kernel   the seventh slope;  the row's sum of (err / (atol + rtol max(|y0|, |y1|)))^2 in double over its e elements and its
//                  delta_logp - one double per row;  mean_kernel (ONE workgroup, the next launch) adds the 2B row sums in a fixed order
//                  and leaves the mean over the 2B (e + 1) components where the host reads it
//   norm_kernel    the norms of the automatic first step: the same shape with (a - b) / (atol + rtol |y0|)
// The norm is the mixed rms norm over the PACKED state (n, e + 1) that Sampler.sample_ode_likelihood hands its Dormand-Prince driver (the
// reference passes torchdiffeq a tuple state, which it flattens): one atol / rtol for both components.
// Arithmetic: the CFG blend is logp::cfg_blend_pass (cfg_blend_kernel's contracted statement); every other product and sum is rounded on
// its own.  Every reduction runs in a fixed order (lane-strided partial sums, a butterfly over the wave, rows in rising order): no
// atomics, run-to-run identical.  All results leave through plain vector stores.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.hpp"
#include "logp.hpp"

namespace scldm {
namespace logp_d5 {

#pragma clang fp contract(off)

constexpr int kMaxK = 7;
// the slopes of a combination in tableau order, structural zeros left out; the LAST entry is the slope the kernel itself forms (taken
// from its registers: kx / kl of that entry are not read)
struct Comb {
  const float* kx[kMaxK];   // (2B, e) each
  const float* kl[kMaxK];   // (2B) each
  float c[kMaxK];           // h * tableau weight, rounded to fp32 by the host
  int n_k;
};
// where an evaluation left its results (logp.hpp's row layout: 2B state rows, then P conditional passes of B rows)
struct Geom {
  const float* out;   // (N, e) forward outputs
  const float* dx;    // (N, e) input gradients of the seeded backward
  const float* eps;   // (2B, e)
  int B, e, P;
  float scale[logp::kMaxClasses];
};

// -v of four elements of state row r (the blend of logp::blend_kernel, term by term), and the row's probe . dx partial sum continued
__device__ __forceinline__ f32x4 slope4(const Geom& g, int r, size_t row4, size_t half4, int c4, float& acc) {
  const f32x4* out = reinterpret_cast<const f32x4*>(g.out);
  const f32x4* dx = reinterpret_cast<const f32x4*>(g.dx);
  f32x4 v = out[row4 + c4], d = dx[row4 + c4];
  if (r >= g.B) {
    const f32x4 u = v;
    for (int p = 0; p < g.P; ++p) {
      v = logp::cfg_blend_pass(v, out[row4 + half4 + (size_t)p * half4 + c4], u, g.scale[p]);
      d = d + dx[row4 + half4 + (size_t)p * half4 + c4];
    }
  }
  const f32x4 ep = reinterpret_cast<const f32x4*>(g.eps)[row4 + c4];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc = acc + ep[i] * d[i];
  return -v;
}

struct StageArgs {
  Geom g;
  float* kx_new;      // (2B, e) the slope -v
  float* kl_new;      // (2B) the slope logp_grad
  const float* y0x;   // start of the step (read when outx is given)
  const float* y0l;
  float* outx;        // the next stage point, or NULL: the slopes alone (the first evaluation of a solve, the initial-step probe)
  float* outl;
  Comb c;
};
__global__ __launch_bounds__(256) void stage_kernel(const StageArgs a) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= 2 * a.g.B) return;   // (whole waves leave: the shuffles below see full waves)
  const int e4 = a.g.e >> 2;
  const size_t half4 = (size_t)a.g.B * e4, row4 = (size_t)r * e4;
  float acc = 0.f;
  for (int c4 = lane; c4 < e4; c4 += 64) {
    const f32x4 nv = slope4(a.g, r, row4, half4, c4, acc);
    reinterpret_cast<f32x4*>(a.kx_new)[row4 + c4] = nv;
    if (a.outx) {
      f32x4 s = reinterpret_cast<const f32x4*>(a.y0x)[row4 + c4];
#pragma unroll
      for (int j = 0; j < kMaxK; ++j)
        if (j < a.c.n_k) {
          const f32x4 kv = (j == a.c.n_k - 1) ? nv : reinterpret_cast<const f32x4*>(a.c.kx[j])[row4 + c4];
          s = s + kv * a.c.c[j];    // (combine_kernel's statement)
        }
      reinterpret_cast<f32x4*>(a.outx)[row4 + c4] = s;
    }
  }
  const float lg = logp::wave_sum_fixed(acc);
  if (lane == 0) {
    a.kl_new[r] = lg;
    if (a.outx) {
      float s = a.y0l[r];
#pragma unroll
      for (int j = 0; j < kMaxK; ++j)
        if (j < a.c.n_k) s = s + ((j == a.c.n_k - 1) ? lg : a.c.kl[j][r]) * a.c.c[j];
      a.outl[r] = s;
    }
  }
}

__device__ __forceinline__ double wave_sum_fixed_f64(double v) {   // butterfly over the 64 lanes: every lane ends with the same bits
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o);
  return v;
}

struct ErrorArgs {
  Geom g;
  float* kx_new;
  float* kl_new;
  const float* y0x;
  const float* y0l;
  const float* y1x;   // the 5th-order solution: the last stage point
  const float* y1l;
  Comb c;             // error weights, structural zeros left out, the new slope last
  float atol, rtol;
  double* partial;    // (2B) row sums
};
__global__ __launch_bounds__(256) void error_kernel(const ErrorArgs a) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= 2 * a.g.B) return;
  const int e4 = a.g.e >> 2;
  const size_t half4 = (size_t)a.g.B * e4, row4 = (size_t)r * e4;
  float acc = 0.f;
  double s = 0.0;
  for (int c4 = lane; c4 < e4; c4 += 64) {
    const f32x4 nv = slope4(a.g, r, row4, half4, c4, acc);
    reinterpret_cast<f32x4*>(a.kx_new)[row4 + c4] = nv;
    f32x4 err = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < kMaxK; ++j)
      if (j < a.c.n_k) {
        const f32x4 t = ((j == a.c.n_k - 1) ? nv : reinterpret_cast<const f32x4*>(a.c.kx[j])[row4 + c4]) * a.c.c[j];
        err = j == 0 ? t : err + t;    // (rk::error_kernel's statement: the first term exact)
      }
    const f32x4 y0 = reinterpret_cast<const f32x4*>(a.y0x)[row4 + c4], y1 = reinterpret_cast<const f32x4*>(a.y1x)[row4 + c4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float den = a.atol + a.rtol * fmaxf(fabsf(y0[i]), fabsf(y1[i]));
      const double q = (double)(err[i] / den);
      s = s + q * q;
    }
  }
  const float lg = logp::wave_sum_fixed(acc);
  s = wave_sum_fixed_f64(s);
  if (lane == 0) {
    a.kl_new[r] = lg;
    float err = 0.f;
#pragma unroll
    for (int j = 0; j < kMaxK; ++j)
      if (j < a.c.n_k) {
        const float t = ((j == a.c.n_k - 1) ? lg : a.c.kl[j][r]) * a.c.c[j];
        err = j == 0 ? t : err + t;
      }
    const float den = a.atol + a.rtol * fmaxf(fabsf(a.y0l[r]), fabsf(a.y1l[r]));
    const double q = (double)(err / den);
    a.partial[r] = s + q * q;      // the row's e elements first, its delta_logp last
  }
}

// partial[r] = sum over the row's x elements, then its delta_logp, of ((a - b) / (atol + rtol |y0|))^2 in double (b NULL: a alone): one
// fp32 difference and one fp32 quotient per component, as the composed expressions (f1 - f0) / scale and y0 / scale
struct NormArgs {
  const float *ax, *al, *bx, *bl, *y0x, *y0l;
  int rows, e;
  float atol, rtol;
  double* partial;
};
__global__ __launch_bounds__(256) void norm_kernel(const NormArgs a) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= a.rows) return;
  const int e4 = a.e >> 2;
  const size_t row4 = (size_t)r * e4;
  double s = 0.0;
  for (int c4 = lane; c4 < e4; c4 += 64) {
    f32x4 x = reinterpret_cast<const f32x4*>(a.ax)[row4 + c4];
    if (a.bx) x = x - reinterpret_cast<const f32x4*>(a.bx)[row4 + c4];
    const f32x4 y = reinterpret_cast<const f32x4*>(a.y0x)[row4 + c4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const double q = (double)(x[i] / (a.atol + a.rtol * fabsf(y[i])));
      s = s + q * q;
    }
  }
  s = wave_sum_fixed_f64(s);
  if (lane == 0) {
    float x = a.al[r];
    if (a.bl) x = x - a.bl[r];
    const double q = (double)(x / (a.atol + a.rtol * fabsf(a.y0l[r])));
    a.partial[r] = s + q * q;
  }
}

// *out = (sum of the n_part row sums) / count.  One workgroup: thread t adds rows t, t + 256, ... in rising order, thread 0 then adds the
// 256 thread sums in thread order - a fixed order for any number of rows
__global__ __launch_bounds__(256) void mean_kernel(const double* __restrict__ partial, int n_part, double count, double* __restrict__ out) {
  __shared__ double p[256];
  double t = 0.0;
  for (int b = threadIdx.x; b < n_part; b += 256) t = t + partial[b];
  p[threadIdx.x] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int b = 0; b < 256; ++b) s = s + p[b];
    *out = s / count;
  }
}

}  // namespace logp_d5
}  // namespace scldm
// (contraction stays off past this header, as ode_rk.hpp and dopri5_fused.hpp leave it: the solve's host code follows)

// Training kernels of the scVI-style baseline VAE (ScviVAE; the reference trains it with VAEScvi.training_step, models.py:942-1113):
// BatchNorm1d in training mode forward and backward, the dropout mask, the two heads' backward and the products a backward needs.
// The products run on exact fp32 operands (scvi::F32Operands) or on fp16 operands (scvi::F16Operands, the reference's TF32 class);
// everything else is fp32 in both.  The training forward takes its raw products from scvi::gemm_kernel (MODE_PARTIAL, launched by
// scvi_api.hip).  Philox4x32-10 is the project's, from fm_step_common.hpp.
//
// prod_kernel (in scvi_prod.hpp with sum_slots_kernel: the wide TransformerVAE's backward instantiates the two as well) is the tile
// product of scvi_tile.hpp with the loaders a backward needs:
//   TN  C[M, N] = A[K, M]^T B[K, N]   weight gradients, K = batch: both operands k-strided
//   NN  C[M, N] = A[M, K] B[K, N]     data gradients dY W with W as torch stores it: A k-contiguous, B k-strided
// log1p is applied to the B operand while staging (dW_0 = da_0^T log1p(X)).  K above kScviSplit is cut into blockIdx.z splits of that
// many k-values - a function of K alone - written as slots of a partial buffer which sum_slots_kernel adds in slot order.  No float
// atomics anywhere: every sum below has one fixed order.
//
// fp16 operands: a gradient tensor that is an operand (always A: dlogit, the theta logits' gradient, every layer's da, dloc_t,
// dlog_scale) carries one power of two per TENSOR - K is the batch in a weight gradient, so a per-cell scale would not factor out of
// the sum.  The kernel that produces the tensor (template parameter F16 of lik_backward_kernel, bn_backward_kernel and
// post_backward_kernel) leaves the maximum of its magnitude bits in a slot of the workspace (unsigned integer maximum: exact in any
// order); prod_kernel<F16Operands, ...> reads the slot, multiplies A by 2^e while staging (scvi::scale_exponent) and its result by
// 2^-e, both exact.  The host never reads a slot.  The same instantiations raise the caller's overflow flag (found_inf) on a
// non-finite maximum or result.  The F16 = false instantiations are the fp32 kernels, instruction for instruction.
#pragma once
#include <type_traits>

#include "fm_step_common.hpp"
#include "scvi_prod.hpp"
#include "scvi_tile.hpp"

namespace scldm {
namespace scvi_train {

constexpr uint32_t kTagDrop = 0x64726f70u;   // "drop": keeps the mask draws apart from the project's other Philox streams

// the block's maximum of `m` (every thread of the block calls it) into *slot
__device__ __forceinline__ void block_max_to_slot(uint32_t m, uint32_t* slot) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o));
  if ((threadIdx.x & 63) == 0 && m != 0u) atomicMax(slot, m);
}
// ------------------------------------------------------------------------------------------------
// Column reductions over the batch.  A workgroup owns kColTile columns; thread (column tid % kColTile, row group tid / kColTile) adds
// its rows rg, rg + kRowGroups, ... in ascending order, then every thread adds the group sums of its column in group order: the
// order is a function of B alone, whatever the grid.  Eight columns per workgroup (32-byte row segments) rather than a full 128-byte
// line: at hidden 512 that is 64 workgroups with 16 rows per thread at 512 cells instead of 16 workgroups with 64.
// ------------------------------------------------------------------------------------------------
constexpr int kColTile = 8, kRowGroups = 256 / kColTile;

__device__ __forceinline__ float col_total(float (*red)[kColTile], float v) {
  const int cl = threadIdx.x % kColTile, rg = threadIdx.x / kColTile;
  red[rg][cl] = v;
  __syncthreads();
  float s = red[0][cl];
#pragma unroll
  for (int q = 1; q < kRowGroups; ++q) s += red[q][cl];
  __syncthreads();
  return s;
}

__device__ __forceinline__ float sigmoid_f(float x) { return 1.f / (1.f + expf(-x)); }

struct BnFwdArgs {
  const float* part;     // (splits, B, H) raw products of the Linear
  int splits;
  const float *bias, *gamma, *beta;
  float *run_mean, *run_var;
  float momentum, eps, p;
  int B, H;
  unsigned long long seed;
  uint32_t layer_tag;    // MLP * 8 + layer
  uint8_t* mask;         // (B, H) keep bytes, p > 0 only
  int draw;              // 1: draw the mask and record it, 0: read the given one
  float *xhat, *h, *rstd;   // record: (B, H), (B, H), (H)
};

// a = sum of the splits in order + bias;  mean, biased variance (two passes: mean first, then the centred second moment);  running
// statistics in place (running_var takes the unbiased variance);  xhat = (a - mean) rstd, h = SiLU(gamma xhat + beta) keep / (1 - p).
__global__ __launch_bounds__(256) void bn_forward_kernel(const BnFwdArgs a) {
  __shared__ float red[kRowGroups][kColTile];
  const int c = blockIdx.x * kColTile + threadIdx.x % kColTile, rg = threadIdx.x / kColTile;
  const bool ok = c < a.H;
  const size_t plane = (size_t)a.B * a.H;
  float s = 0.f;
  if (ok) {
    const float b = a.bias[c];
    for (int r = rg; r < a.B; r += kRowGroups) {
      const size_t i = (size_t)r * a.H + c;
      float v = a.part[i];
      for (int z = 1; z < a.splits; ++z) v += a.part[z * plane + i];
      v += b;
      a.xhat[i] = v;
      s += v;
    }
  }
  const float mean = col_total(red, s) / (float)a.B;
  s = 0.f;
  if (ok)
    for (int r = rg; r < a.B; r += kRowGroups) {
      const float d = a.xhat[(size_t)r * a.H + c] - mean;
      s += d * d;
    }
  const float var = col_total(red, s) / (float)a.B;
  if (!ok) return;
  const float rstd = 1.f / sqrtf(var + a.eps);
  if (rg == 0) {
    a.rstd[c] = rstd;
    a.run_mean[c] = (1.f - a.momentum) * a.run_mean[c] + a.momentum * mean;
    a.run_var[c] = (1.f - a.momentum) * a.run_var[c] + a.momentum * (var * ((float)a.B / (float)(a.B - 1)));
  }
  const float g = a.gamma[c], be = a.beta[c], inv_keep = 1.f / (1.f - a.p);
  for (int r = rg; r < a.B; r += kRowGroups) {
    const size_t i = (size_t)r * a.H + c;
    const float xh = (a.xhat[i] - mean) * rstd;
    float v = silu_f(g * xh + be);
    if (a.p > 0.f) {
      uint8_t keep;
      if (a.draw) {
        const fmstep::U4 u = fmstep::philox4((uint32_t)c, (uint32_t)r, a.layer_tag, kTagDrop, (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
        keep = fmstep::u01_closed0(u.x) >= a.p;
        a.mask[i] = keep;
      } else {
        keep = a.mask[i] != 0;
      }
      v = keep ? v * inv_keep : 0.f;
    }
    a.xhat[i] = xh;
    a.h[i] = v;
  }
}

struct BnBwdArgs {
  float* d;              // (B, H): dh on entry, da on exit
  const float *xhat, *rstd, *gamma, *beta;
  const uint8_t* mask;   // p > 0 only
  float p;
  int B, H;
  float *dgamma, *dbeta, *dbias;
  uint32_t* da_max;      // F16: slot of da's magnitude-bit maximum
  float* found_inf;      // F16: set to 1 on a non-finite dgamma / dbeta; may be NULL
};

// dy = dh keep / (1 - p) SiLU'(gamma xhat + beta);  dbeta = sum dy, dgamma = sum dy xhat;  da = gamma rstd (dy - mean(dy) - xhat
// mean(dy xhat));  the Linear bias in front of a training-mode BatchNorm has the gradient zero, written as such.
template <bool F16>
__global__ __launch_bounds__(256) void bn_backward_kernel(const BnBwdArgs a) {
  __shared__ float red[kRowGroups][kColTile];
  const int c = blockIdx.x * kColTile + threadIdx.x % kColTile, rg = threadIdx.x / kColTile;
  const bool ok = c < a.H;
  float s1 = 0.f, s2 = 0.f, g = 0.f;
  if (ok) {
    g = a.gamma[c];
    const float be = a.beta[c], inv_keep = 1.f / (1.f - a.p);
    for (int r = rg; r < a.B; r += kRowGroups) {
      const size_t i = (size_t)r * a.H + c;
      const float xh = a.xhat[i], y = g * xh + be, sg = sigmoid_f(y);
      float dy = a.d[i] * (sg * (1.f + y * (1.f - sg)));
      if (a.p > 0.f) dy = a.mask[i] ? dy * inv_keep : 0.f;
      a.d[i] = dy;
      s1 += dy;
      s2 += dy * xh;
    }
  }
  s1 = col_total(red, s1);
  s2 = col_total(red, s2);
  if constexpr (!F16) {
    if (!ok) return;
    if (rg == 0) {
      a.dbeta[c] = s1;
      a.dgamma[c] = s2;
      a.dbias[c] = 0.f;
    }
    const float m1 = s1 / (float)a.B, m2 = s2 / (float)a.B, gr = g * a.rstd[c];
    for (int r = rg; r < a.B; r += kRowGroups) {
      const size_t i = (size_t)r * a.H + c;
      a.d[i] = gr * (a.d[i] - m1 - a.xhat[i] * m2);
    }
  } else {      // the same, every thread staying for the block's maximum of |da|
    uint32_t mx = 0u;
    if (ok) {
      if (rg == 0) {
        a.dbeta[c] = s1;
        a.dgamma[c] = s2;
        a.dbias[c] = 0.f;
        if (a.found_inf && !(finite_f(s1) && finite_f(s2))) *a.found_inf = 1.0f;
      }
      const float m1 = s1 / (float)a.B, m2 = s2 / (float)a.B, gr = g * a.rstd[c];
      for (int r = rg; r < a.B; r += kRowGroups) {
        const size_t i = (size_t)r * a.H + c;
        const float da = gr * (a.d[i] - m1 - a.xhat[i] * m2);
        a.d[i] = da;
        mx = max(mx, scvi::magnitude_bits(da));
      }
    }
    block_max_to_slot(mx, a.da_max);
  }
}

// out[c] = sum over the B rows of X[., c]
template <bool F16>
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ X, int B, int N, float* __restrict__ out, float* found_inf) {
  __shared__ float red[kRowGroups][kColTile];
  const int c = blockIdx.x * kColTile + threadIdx.x % kColTile, rg = threadIdx.x / kColTile;
  float s = 0.f;
  if (c < N)
    for (int r = rg; r < B; r += kRowGroups) s += X[(size_t)r * N + c];
  s = col_total(red, s);
  if (c < N && rg == 0) out[c] = s;
  if (F16 && c < N && rg == 0 && found_inf && !finite_f(s)) *found_inf = 1.0f;
}

// ------------------------------------------------------------------------------------------------
// Posterior head.  Forward: the two raw products (their k-splits added in split order) -> loc, pre-clamp log-scale (recorded for the hardtanh gate), scale, z.
// Backward: dloc += dz, dscale += dz eps, dlog_scale = dscale scale strictly inside (-7, 5), else 0 (torch's hardtanh backward).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void post_forward_kernel(const float* __restrict__ raw_loc, const float* __restrict__ raw_ls,
                                                           const float* __restrict__ loc_b, const float* __restrict__ scale_b,
                                                           const float* __restrict__ eps, int splits, int n, int L,
                                                           float* __restrict__ loc, float* __restrict__ ls_pre,
                                                           float* __restrict__ scale, float* __restrict__ z) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int j = i % L;
  float lo = raw_loc[i], ls = raw_ls[i];
  for (int s = 1; s < splits; ++s) {      // (splits, B, L) each: n_hidden above kScviSplit is cut like every other product
    lo += raw_loc[(size_t)s * n + i];
    ls += raw_ls[(size_t)s * n + i];
  }
  lo += loc_b[j];
  ls += scale_b[j];
  const float sc = expf(fminf(fmaxf(ls, -7.f), 5.f));
  loc[i] = lo;
  ls_pre[i] = ls;
  scale[i] = sc;
  z[i] = lo + eps[i] * sc;
}

template <bool F16>
__global__ __launch_bounds__(256) void post_backward_kernel(const float* __restrict__ dz, const float* __restrict__ dz_dec,
                                                            const float* __restrict__ dloc, const float* __restrict__ dscale,
                                                            const float* __restrict__ eps, const float* __restrict__ scale,
                                                            const float* __restrict__ ls_pre, int n, float* __restrict__ dloc_t,
                                                            float* __restrict__ dls, uint32_t* dloc_max, uint32_t* dls_max,
                                                            float* found_inf) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if constexpr (!F16) {
    if (i >= n) return;
    float g = dz ? dz[i] : 0.f;
    if (dz_dec) g += dz_dec[i];
    const float dl = (dloc ? dloc[i] : 0.f) + g;
    const float ds = (dscale ? dscale[i] : 0.f) + g * eps[i];
    const float ls = ls_pre[i];
    dloc_t[i] = dl;
    dls[i] = (ls > -7.f && ls < 5.f) ? ds * scale[i] : 0.f;
  } else {      // the same, every thread staying for the two maxima; an upstream gradient behind a closed hardtanh gate is checked too
    uint32_t m_dl = 0u, m_ds = 0u;
    if (i < n) {
      float g = dz ? dz[i] : 0.f;
      if (dz_dec) g += dz_dec[i];
      const float dl = (dloc ? dloc[i] : 0.f) + g;
      const float ds = (dscale ? dscale[i] : 0.f) + g * eps[i];
      const float ls = ls_pre[i];
      const float dv = (ls > -7.f && ls < 5.f) ? ds * scale[i] : 0.f;
      dloc_t[i] = dl;
      dls[i] = dv;
      m_dl = scvi::magnitude_bits(dl);
      m_ds = scvi::magnitude_bits(dv);
      if (found_inf && !finite_f(ds)) *found_inf = 1.0f;
    }
    block_max_to_slot(m_dl, dloc_max);
    block_max_to_slot(m_ds, dls_max);
  }
}

// ------------------------------------------------------------------------------------------------
// Likelihood head backward, one workgroup per row: s_b = sum_g mu dmu (thread-strided partial sums, then the wave's xor tree, then
// the four waves in order: a fixed order), dlogit = mu dmu - (mu / library) s_b (zeros for library 0); unshared theta:
// dtheta_logit = dtheta softplus'(.) with softplus'(x) = 1 - exp(-theta) (= sigmoid(x); 1 above torch's threshold 20).  Workgroup 0
// also forms the shared theta's dtheta_param = dtheta softplus'(theta_param).
// ------------------------------------------------------------------------------------------------
template <bool F16>
__global__ __launch_bounds__(256) void lik_backward_kernel(const float* __restrict__ mu, const float* __restrict__ theta,
                                                           const float* __restrict__ dmu, const float* __restrict__ dtheta,
                                                           const float* __restrict__ library, int G, int shared_theta,
                                                           const float* __restrict__ theta_param, float* __restrict__ dlogit,
                                                           float* __restrict__ dtlogit, float* __restrict__ dtheta_param,
                                                           uint32_t* dlogit_max, uint32_t* dtlogit_max, float* found_inf) {
  __shared__ float red[4];
  const int row = blockIdx.x, tid = threadIdx.x;
  const size_t o = (size_t)row * G;
  float s = 0.f;
  if (dmu)
    for (int g = tid; g < G; g += 256) s += mu[o + g] * dmu[o + g];
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m);
  if ((tid & 63) == 0) red[tid >> 6] = s;
  __syncthreads();
  s = ((red[0] + red[1]) + red[2]) + red[3];
  const float lib = library[row];
  uint32_t m_dl = 0u, m_dt = 0u;      // (F16 only)
  for (int g = tid; g < G; g += 256) {
    const float m = mu[o + g];
    const float dl = (dmu && lib != 0.f) ? m * dmu[o + g] - (m / lib) * s : 0.f;
    dlogit[o + g] = dl;
    if (F16) m_dl = max(m_dl, scvi::magnitude_bits(dl));
    if (!shared_theta) {
      const float t = theta[o + g];
      const float dt = dtheta ? dtheta[o + g] * (t > 20.f ? 1.f : -expm1f(-t)) : 0.f;
      dtlogit[o + g] = dt;
      if (F16) m_dt = max(m_dt, scvi::magnitude_bits(dt));
    }
  }
  if (shared_theta && row == 0)
    for (int g = tid; g < G; g += 256) {
      const float x = theta_param[g];
      const float dp = dtheta ? dtheta[g] * (x > 20.f ? 1.f : sigmoid_f(x)) : 0.f;
      dtheta_param[g] = dp;
      if (F16 && found_inf && !finite_f(dp)) *found_inf = 1.0f;
    }
  if constexpr (F16) {
    block_max_to_slot(m_dl, dlogit_max);
    if (!shared_theta) block_max_to_slot(m_dt, dtlogit_max);
  }
}

}  // namespace scvi_train
}  // namespace scldm

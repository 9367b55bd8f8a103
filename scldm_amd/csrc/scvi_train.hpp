// Training kernels of the scVI-style baseline VAE (ScviVAE; the reference trains it with VAEScvi.training_step, models.py:942-1113):
// BatchNorm1d in training mode forward and backward, the dropout mask, the two heads' backward and the products a backward needs.
// Exact fp32 (OpF32) like scvi.hpp, whose forward tile kernel (NT: X[M, K] W[N, K]^T) the training forward reuses as it is
// (MODE_PARTIAL: the raw products, launched by scvi_api.hip).  These kernels live in a translation unit of their own
// (scvi_train_api.hip): the eval kernels' device module is what it was.  Philox4x32-10 is the project's, from fm_step_common.hpp.
//
// prod_kernel is scvi::gemm_kernel's tile (64 x 64 per workgroup of four waves, K in stages of 32 through LDS, one accumulator per
// element walked in ascending k, the next stage's loads in flight during the MFMAs) with the two loaders a backward needs:
//   TN  C[M, N] = A[K, M]^T B[K, N]   weight gradients, K = batch: both operands k-STRIDED, so a thread walks the row axis (64
//                                     consecutive rows per 256-byte request) and four k-values per stage pass
//   NN  C[M, N] = A[M, K] B[K, N]     data gradients dY W with W as torch stores it: A k-contiguous (gemm_kernel's loader), B k-strided
// Loads are masked scalar dwords (17 002-float rows are 8-byte aligned), log1p is applied to the B operand while staging (dW_0 =
// da_0^T log1p(X)).  K above scvi_host::kScviSplit is cut into blockIdx.z splits of that many k-values - a function of K alone - written as slots of a
// partial buffer which sum_slots_kernel adds in slot order.  No float atomics anywhere: every sum below has one fixed order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.hpp"
#include "fm_step_common.hpp"

namespace scldm {
namespace scvi_train {

constexpr int kBM = 64, kBN = 64, kBK = 32, kLd = kBK + 4;   // scvi::gemm_kernel's tile
constexpr uint32_t kTagDrop = 0x64726f70u;   // "drop": keeps the mask draws apart from the project's other Philox streams

struct ProdArgs {
  const float* A;        // AT: (K, M) with row stride lda | else (M, K) with row stride lda
  const float* Bm;       // (K, N) with row stride ldb
  long long lda, ldb;
  int M, N, K;
  int k_per_split;       // k-values per blockIdx.z (multiple of kBK)
  float* out;            // (slots, M, N); this launch writes slots slot0 + blockIdx.z
  int slot0;
};

template <bool AT, bool LOG1P_B>
__global__ __launch_bounds__(256) void prod_kernel(const ProdArgs a) {
  __shared__ __attribute__((aligned(16))) float smem[2 * kBM * kLd];
  float* As = smem;
  float* Bs = smem + kBM * kLd;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.y * kBM, n0 = blockIdx.x * kBN;
  const int k_lo = blockIdx.z * a.k_per_split;
  const int k_hi = min(a.K, k_lo + a.k_per_split);
  // k-contiguous loader: thread -> k offset tid & 31 of rows (tid >> 5) + 8 j;  k-strided loader: row tid & 63 at k offsets (tid >> 6) + 4 j
  const int lk = tid & 31, lr = tid >> 5, tr = tid & 63, tk = tid >> 6;
  float xa[8], wb[8];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (AT) {
        const int k = k0 + tk + 4 * j, m = m0 + tr;
        xa[j] = (k < k_hi && m < a.M) ? a.A[(size_t)k * a.lda + m] : 0.f;
      } else {
        const int k = k0 + lk, m = m0 + lr + 8 * j;
        xa[j] = (k < k_hi && m < a.M) ? a.A[(size_t)m * a.lda + k] : 0.f;
      }
      const int k = k0 + tk + 4 * j, n = n0 + tr;
      wb[j] = (k < k_hi && n < a.N) ? a.Bm[(size_t)k * a.ldb + n] : 0.f;
    }
  };
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  if (k_lo < k_hi) fetch(k_lo);
  const int hh = lane >> 5, l31 = lane & 31;
  for (int k0 = k_lo; k0 < k_hi; k0 += kBK) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (AT) As[tr * kLd + tk + 4 * j] = xa[j];
      else As[(lr + 8 * j) * kLd + lk] = xa[j];
      Bs[tr * kLd + tk + 4 * j] = LOG1P_B ? log1pf(wb[j]) : wb[j];
    }
    __syncthreads();
    if (k0 + kBK < k_hi) fetch(k0 + kBK);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const float* ap = As + (wm * 32 + l31) * kLd + u * 16 + 8 * hh;
      const float* bp = Bs + (wn * 32 + l31) * kLd + u * 16 + 8 * hh;
      const f32x4 a0 = *reinterpret_cast<const f32x4*>(ap), a1 = *reinterpret_cast<const f32x4*>(ap + 4);
      const f32x4 b0 = *reinterpret_cast<const f32x4*>(bp), b1 = *reinterpret_cast<const f32x4*>(bp + 4);
      const f32x8 af = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
      const f32x8 bf = {b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
      acc = OpF32::mma(af, bf, acc);
    }
    __syncthreads();
  }
  // lane holds column wn * 32 + l31 of the tile, register r row wm * 32 + acc_row(r, hh)
  const int n = n0 + wn * 32 + l31;
  if (n >= a.N) return;
  float* out = a.out + (size_t)(a.slot0 + blockIdx.z) * a.M * a.N;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = m0 + wm * 32 + acc_row(r, hh);
    if (m < a.M) out[(size_t)m * a.N + n] = acc[r];
  }
}

// out = slot 0 + slot 1 + ... in slot order
__global__ __launch_bounds__(256) void sum_slots_kernel(const float* __restrict__ part, int slots, size_t plane, float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= plane) return;
  float v = part[i];
  for (int z = 1; z < slots; ++z) v += part[z * plane + i];
  out[i] = v;
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
};

// dy = dh keep / (1 - p) SiLU'(gamma xhat + beta);  dbeta = sum dy, dgamma = sum dy xhat;  da = gamma rstd (dy - mean(dy) - xhat
// mean(dy xhat));  the Linear bias in front of a training-mode BatchNorm has the gradient zero, written as such.
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
}

// out[c] = sum over the B rows of X[., c]
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ X, int B, int N, float* __restrict__ out) {
  __shared__ float red[kRowGroups][kColTile];
  const int c = blockIdx.x * kColTile + threadIdx.x % kColTile, rg = threadIdx.x / kColTile;
  float s = 0.f;
  if (c < N)
    for (int r = rg; r < B; r += kRowGroups) s += X[(size_t)r * N + c];
  s = col_total(red, s);
  if (c < N && rg == 0) out[c] = s;
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

__global__ __launch_bounds__(256) void post_backward_kernel(const float* __restrict__ dz, const float* __restrict__ dz_dec,
                                                            const float* __restrict__ dloc, const float* __restrict__ dscale,
                                                            const float* __restrict__ eps, const float* __restrict__ scale,
                                                            const float* __restrict__ ls_pre, int n, float* __restrict__ dloc_t,
                                                            float* __restrict__ dls) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float g = dz ? dz[i] : 0.f;
  if (dz_dec) g += dz_dec[i];
  const float dl = (dloc ? dloc[i] : 0.f) + g;
  const float ds = (dscale ? dscale[i] : 0.f) + g * eps[i];
  const float ls = ls_pre[i];
  dloc_t[i] = dl;
  dls[i] = (ls > -7.f && ls < 5.f) ? ds * scale[i] : 0.f;
}

// ------------------------------------------------------------------------------------------------
// Likelihood head backward, one workgroup per row: s_b = sum_g mu dmu (thread-strided partial sums, then the wave's xor tree, then
// the four waves in order: a fixed order), dlogit = mu dmu - (mu / library) s_b (zeros for library 0); unshared theta:
// dtheta_logit = dtheta softplus'(.) with softplus'(x) = 1 - exp(-theta) (= sigmoid(x); 1 above torch's threshold 20).  Workgroup 0
// also forms the shared theta's dtheta_param = dtheta softplus'(theta_param).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lik_backward_kernel(const float* __restrict__ mu, const float* __restrict__ theta,
                                                           const float* __restrict__ dmu, const float* __restrict__ dtheta,
                                                           const float* __restrict__ library, int G, int shared_theta,
                                                           const float* __restrict__ theta_param, float* __restrict__ dlogit,
                                                           float* __restrict__ dtlogit, float* __restrict__ dtheta_param) {
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
  for (int g = tid; g < G; g += 256) {
    const float m = mu[o + g];
    dlogit[o + g] = (dmu && lib != 0.f) ? m * dmu[o + g] - (m / lib) * s : 0.f;
    if (!shared_theta) {
      const float t = theta[o + g];
      dtlogit[o + g] = dtheta ? dtheta[o + g] * (t > 20.f ? 1.f : -expm1f(-t)) : 0.f;
    }
  }
  if (shared_theta && row == 0)
    for (int g = tid; g < G; g += 256) {
      const float x = theta_param[g];
      dtheta_param[g] = dtheta ? dtheta[g] * (x > 20.f ? 1.f : sigmoid_f(x)) : 0.f;
    }
}

}  // namespace scvi_train
}  // namespace scldm

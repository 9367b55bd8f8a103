// Kernels of the scVI-style baseline VAE (ScviVAE: src/scldm/nnets.py:19-73, stochastic_layers.py:38-70,123-158, vae.py:90-128),
// inference only, exact fp32 on the matrix pipe (OpF32: 8 x v_mfma_f32_32x32x2_f32 per 16 k-values).
//
// One tile kernel serves every dense product of the model, Y[M, N] = act(X[M, K]) W[N, K]^T with both operands row-major and K
// contiguous (torch's Linear layout, used as it is: nothing but the folded BatchNorm vectors is packed):
//   * a workgroup of four waves owns a 64 x 64 output tile, wave (wm, wn) its 32 x 32 quadrant; K is walked in stages of 32 through
//     LDS (rows padded to 36 floats: 16-byte aligned fragments), the next stage's global loads are in flight during the MFMAs;
//   * K, M and N are arbitrary: loads are scalar dwords (a row of 17 002 floats is only 8-byte aligned) masked to zero outside the
//     matrix - log1p(0) = 0, so the masked first-layer operand is zero as well;
//   * every output element accumulates its k-values in ascending stage order in ONE accumulator, and the k range of a split is a
//     function of K alone (kScviSplitK), so an element's bits depend neither on the run nor on the other rows of the batch.
// Epilogues (MODE):
//   LAYER    y = SiLU(s[n] acc + c[n])                        BatchNorm1d(eval) and the Linear bias folded into (s, c)
//   PARTIAL  partial[split][m, n] = acc                       K > kScviSplitK; merge_kernel sums the splits in order
//   POST     columns [0, 32) of a tile are loc, [32, 64) the log-scale of the SAME 32 latents:  loc, scale = exp(hardtanh(., -7, 5)),
//            z = loc + eps scale
//   LIK      logits (+ the theta product in the same pass when theta is unshared: columns [32, 64) of a tile are the theta logits of
//            the 32 genes in columns [0, 32)), written to mu, with one (max, sum exp) pair per (row, tile); softmax_finalize_kernel
//            merges a row's pairs in tile order and rewrites mu in place.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.hpp"

namespace scldm {
namespace scvi {

constexpr int kBM = 64, kBN = 64, kBK = 32, kLd = kBK + 4;
constexpr int kScviSplitK = 1024;          // k-values per split of the layer product (a multiple of kBK)
constexpr int kMaxLayers = 8;              // per MLP
constexpr int kOutLd = kBN + 1;            // LDS row stride of a staged output tile
constexpr int kSmemFloats = kBM * kOutLd + 2 * kBM * 4;   // the epilogues' staged output tile + softmax partials; the operand stages reuse it
static_assert(2 * kBM * kLd <= kSmemFloats, "the two operand stages fit the epilogue's LDS");

enum : int { MODE_LAYER = 0, MODE_PARTIAL = 1, MODE_POST = 2, MODE_LIK = 3, MODE_LIK2 = 4 };   // LIK2: unshared theta

struct GemmArgs {
  const float* X;      // (M, K)
  const float* W0;     // (N0, K)
  const float* W1;     // second weight of POST (log-scale) / LIK2 (theta), same shape as W0
  const float* b0;     // bias of W0 (POST, LIK) | s (LAYER)
  const float* b1;     // bias of W1             | c (LAYER)
  int M, N0, K;
  int k_per_split;     // k-values per blockIdx.z (multiple of kBK); >= K when there is one split
  float* out0;         // LAYER: Y (M, N0) | PARTIAL: partials (splits, M, N0) | POST: loc (M, N0) | LIK: mu (M, N0)
  float* out1;         // POST: scale | LIK2: theta (M, N0)
  float* out2;         // POST: z, or NULL
  const float* eps;    // POST: (M, N0) or NULL
  float* pairs;        // LIK: (M, tiles, 2)
};

__device__ __forceinline__ float softplus_f(float x) { return x > 20.f ? x : log1pf(expf(x)); }   // torch's threshold-20 form

template <int MODE>
struct Traits {
  static constexpr bool kDual = MODE == MODE_POST || MODE == MODE_LIK2;   // a tile's columns [32, 64) come from W1
  static constexpr int kCols = kDual ? 32 : 64;                            // columns of the N0 axis one tile covers
};

// scvi_train::prod_kernel (scvi_train.hpp) is a second copy of this kernel's stage loop and MFMA loop with the TN / NN loaders of the
// backward: a change to the tile, the LDS stride or the fragment layout here has to be made there as well.
template <int MODE, bool LOG1P>
__global__ __launch_bounds__(256) void gemm_kernel(const GemmArgs a) {
  using T = Traits<MODE>;
  __shared__ __attribute__((aligned(16))) float smem[kSmemFloats];
  float* As = smem;
  float* Bs = smem + kBM * kLd;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.y * kBM, n0 = blockIdx.x * T::kCols;
  const int k_lo = blockIdx.z * a.k_per_split;
  const int k_hi = min(a.K, k_lo + a.k_per_split);
  // loader: thread -> k offset tid & 31 of rows (tid >> 5) + 8 j
  const int lk = tid & 31, lr = tid >> 5;
  const float* xrow[8];
  const float* wrow[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int r = lr + 8 * j;
    const int m = m0 + r;
    xrow[j] = m < a.M ? a.X + (size_t)m * a.K : nullptr;
    int n;
    const float* w;
    if (T::kDual) { n = n0 + (r & 31); w = r < 32 ? a.W0 : a.W1; }
    else { n = n0 + r; w = a.W0; }
    wrow[j] = n < a.N0 ? w + (size_t)n * a.K : nullptr;
  }
  float xa[8], wb[8];
  auto fetch = [&](int k0) {
    const int k = k0 + lk;
    const bool ok = k < k_hi;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      xa[j] = (ok && xrow[j]) ? xrow[j][k] : 0.f;
      wb[j] = (ok && wrow[j]) ? wrow[j][k] : 0.f;
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
      As[(lr + 8 * j) * kLd + lk] = LOG1P ? log1pf(xa[j]) : xa[j];
      Bs[(lr + 8 * j) * kLd + lk] = wb[j];
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
  // ---- epilogues: lane holds column wn * 32 + l31 of the tile, register r row wm * 32 + acc_row(r, hh)
  if (MODE == MODE_LAYER || MODE == MODE_PARTIAL) {
    const int n = n0 + wn * 32 + l31;
    if (n >= a.N0) return;
    float s = 1.f, c = 0.f;
    if (MODE == MODE_LAYER) { s = a.b0[n]; c = a.b1[n]; }
    float* out = a.out0 + (MODE == MODE_PARTIAL ? (size_t)blockIdx.z * a.M * a.N0 : 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + wm * 32 + acc_row(r, hh);
      if (m < a.M) out[(size_t)m * a.N0 + n] = MODE == MODE_LAYER ? silu_f(s * acc[r] + c) : acc[r];
    }
    return;
  } else {
    // stage the tile (+ bias) in LDS so that a thread can see the two halves of a column pair / a whole row
    float* tile = smem;
    {
      const int c = wn * 32 + l31;
      const int n = n0 + (T::kDual ? l31 : c);
      const float* bias = (T::kDual && wn) ? a.b1 : a.b0;
      const float bv = n < a.N0 ? bias[n] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) tile[(wm * 32 + acc_row(r, hh)) * kOutLd + c] = acc[r] + bv;
    }
    __syncthreads();
    if (MODE == MODE_POST) {
      for (int idx = tid; idx < kBM * 32; idx += 256) {
        const int r = idx >> 5, j = idx & 31, m = m0 + r, n = n0 + j;
        if (m >= a.M || n >= a.N0) continue;
        const float loc = tile[r * kOutLd + j];
        const float ls = fminf(fmaxf(tile[r * kOutLd + 32 + j], -7.f), 5.f);
        const float sc = expf(ls);
        const size_t o = (size_t)m * a.N0 + n;
        a.out0[o] = loc;
        a.out1[o] = sc;
        if (a.out2) a.out2[o] = loc + a.eps[o] * sc;
      }
    } else {
      constexpr int C = T::kCols;   // logit columns of the tile
      for (int idx = tid; idx < kBM * C; idx += 256) {
        const int r = idx / C, j = idx % C, m = m0 + r, n = n0 + j;
        if (m >= a.M || n >= a.N0) continue;
        const size_t o = (size_t)m * a.N0 + n;
        a.out0[o] = tile[r * kOutLd + j];
        if (MODE == MODE_LIK2) a.out1[o] = softplus_f(tile[r * kOutLd + 32 + j]);
      }
      // (max, sum exp) of the row's logits in this tile: four threads per row take C / 4 consecutive columns each, then the
      // first merges the four in column order
      float* pm = smem + kBM * kOutLd;
      float* ps = pm + kBM * 4;
      const int r = tid >> 2, part = tid & 3;
      const int c_lo = part * (C / 4), c_hi = min(c_lo + C / 4, a.N0 - n0);
      float mx = -INFINITY, sm = 0.f;
      for (int c = c_lo; c < c_hi; ++c) mx = fmaxf(mx, tile[r * kOutLd + c]);
      for (int c = c_lo; c < c_hi; ++c) sm += expf(tile[r * kOutLd + c] - mx);
      pm[r * 4 + part] = mx;
      ps[r * 4 + part] = sm;
      __syncthreads();
      if (part == 0 && m0 + r < a.M) {
        const float M4 = fmaxf(fmaxf(pm[r * 4], pm[r * 4 + 1]), fmaxf(pm[r * 4 + 2], pm[r * 4 + 3]));
        float S = 0.f;
#pragma unroll
        for (int p = 0; p < 4; ++p) S += ps[r * 4 + p] > 0.f ? ps[r * 4 + p] * expf(pm[r * 4 + p] - M4) : 0.f;
        float* pr = a.pairs + ((size_t)(m0 + r) * gridDim.x + blockIdx.x) * 2;
        pr[0] = M4;
        pr[1] = S;
      }
    }
  }
}

// Y = SiLU(s (sum over splits, in split order) + c)
__global__ __launch_bounds__(256) void merge_kernel(const float* __restrict__ part, int splits, size_t plane, int N, const float* __restrict__ s,
                                                    const float* __restrict__ c, float* __restrict__ Y) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= plane) return;
  float v = part[i];
  for (int z = 1; z < splits; ++z) v += part[(size_t)z * plane + i];
  const int n = (int)(i % N);
  Y[i] = silu_f(s[n] * v + c[n]);
}

// One workgroup per row: the row's (max, sum exp) pairs -> (M, S) in tile order, then mu = library exp(l - M) / S in place.
// Workgroup 0 also writes the shared theta = softplus(theta_param) when there is one.
constexpr int kFinChunk = 1024;
__global__ __launch_bounds__(256) void softmax_finalize_kernel(float* __restrict__ mu, const float* __restrict__ pairs, int tiles, int G,
                                                               const float* __restrict__ library, const float* __restrict__ theta_param,
                                                               float* __restrict__ theta) {
  __shared__ float term[kFinChunk];
  __shared__ float red[4];
  __shared__ float ms[2];
  const int row = blockIdx.x, tid = threadIdx.x;
  const float* pr = pairs + (size_t)row * tiles * 2;
  float mx = -INFINITY;
  for (int t = tid; t < tiles; t += 256) mx = fmaxf(mx, pr[2 * t]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));      // max is exact in any order
  if ((tid & 63) == 0) red[tid >> 6] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  float S = 0.f;                                                            // (thread 0's)
  for (int t0 = 0; t0 < tiles; t0 += kFinChunk) {
    const int n = min(kFinChunk, tiles - t0);
    for (int t = tid; t < n; t += 256) term[t] = pr[2 * (t0 + t) + 1] * expf(pr[2 * (t0 + t)] - mx);
    __syncthreads();
    if (tid == 0)
      for (int t = 0; t < n; ++t) S += term[t];
    __syncthreads();
  }
  if (tid == 0) { ms[0] = mx; ms[1] = S; }
  __syncthreads();
  mx = ms[0];
  S = ms[1];
  const float lib = library[row];
  float* mrow = mu + (size_t)row * G;
  for (int g = tid; g < G; g += 256) mrow[g] = lib * (expf(mrow[g] - mx) / S);
  if (row == 0 && theta_param)
    for (int g = tid; g < G; g += 256) theta[g] = softplus_f(theta_param[g]);
}

// ------------------------------------------------------------------------------------------------
// Folding BatchNorm1d(eval) and the Linear bias into y = s x + c per output column, s = gamma / sqrt(running_var + eps),
// c = beta + (b - running_mean) s, for every layer of both MLPs in ONE single-workgroup launch, guarded by a fingerprint of the
// five source vectors of every layer (the position-dependent wrapping sum of dit_aux.hpp): the launch re-packs only when the
// fingerprint moved or `force` is set, so an in-place change of a parameter or a buffer is picked up by the next call in stream order.
// ------------------------------------------------------------------------------------------------
struct PackLayer { const float *b, *gamma, *beta, *mean, *var; };
struct PackArgs {
  PackLayer layer[2 * kMaxLayers];
  int n_layers, H, force;
  float bn_eps;
  float* s;                       // (n_layers, H)
  float* c;
  unsigned long long* fp_state;   // [0] fingerprint of the packed vectors, [1] valid
};
__global__ __launch_bounds__(256) void pack_kernel(const PackArgs a) {
  __shared__ unsigned long long wsum[4];
  __shared__ int dirty;
  const int tid = threadIdx.x;
  unsigned long long hsum = 0;
  for (int l = 0; l < a.n_layers; ++l) {
    const uint32_t* src[5] = {(const uint32_t*)a.layer[l].b, (const uint32_t*)a.layer[l].gamma, (const uint32_t*)a.layer[l].beta,
                              (const uint32_t*)a.layer[l].mean, (const uint32_t*)a.layer[l].var};
#pragma unroll
    for (int q = 0; q < 5; ++q)
      for (int i = tid; i < a.H; i += 256) {
        const unsigned long long v = src[q][i], pos = ((unsigned long long)(l * 5 + q) * a.H + i) + 1;
        hsum += (v + 0x9E3779B97F4A7C15ull * pos) * 0xBF58476D1CE4E5B9ull ^ (v << 29);
      }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) hsum += __shfl_xor(hsum, o);
  if ((tid & 63) == 0) wsum[tid >> 6] = hsum;
  __syncthreads();
  if (tid == 0) {
    const unsigned long long fp = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
    dirty = a.force || a.fp_state[1] == 0 || a.fp_state[0] != fp;
    a.fp_state[0] = fp;
    a.fp_state[1] = 1;
  }
  __syncthreads();
  if (!dirty) return;
  for (int l = 0; l < a.n_layers; ++l)
    for (int i = tid; i < a.H; i += 256) {
      const PackLayer& p = a.layer[l];
      const float s = p.gamma[i] / sqrtf(p.var[i] + a.bn_eps);
      a.s[l * a.H + i] = s;
      a.c[l * a.H + i] = p.beta[i] + (p.b[i] - p.mean[i]) * s;
    }
}

}  // namespace scvi
}  // namespace scldm

// Inference kernels of the scVI-style baseline VAE (ScviVAE: src/scldm/nnets.py:19-73, stochastic_layers.py:38-70,123-158,
// vae.py:90-128).  gemm_kernel serves every dense product of the model, Y[M, N] = act(X[M, K]) W[N, K]^T with both operands fp32,
// row-major and K contiguous (torch's Linear layout, read where the parameters live: nothing but the folded BatchNorm vectors is
// packed), on the tile, the operand policies (exact fp32 or fp16 operands) and the epilogues of scvi_tile.hpp.
#pragma once
#include "scvi_tile.hpp"

namespace scldm {
namespace scvi {

template <class P, int MODE, bool LOG1P>
__global__ __launch_bounds__(256) void gemm_kernel(const GemmArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[kSmemBytes<P>];
  RowLoader<P, LOG1P> la(a.X, blockIdx.y * kBM, a.M, a.K);
  RowLoader<P, false> lb(a.W0, a.W1, Traits<MODE>::kDual, blockIdx.x * Traits<MODE>::kCols, a.N0, a.K);
  const int k_lo = blockIdx.z * a.k_per_split;
  const int k_hi = min(a.K, k_lo + a.k_per_split);
  const f32x16 acc = tile_product<P>(la, lb, smem, k_lo, k_hi);
  tile_epilogue<MODE>(a, acc, reinterpret_cast<float*>(smem), blockIdx.z);
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
  PackLayer layer[2 * kScviMaxLayers];
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

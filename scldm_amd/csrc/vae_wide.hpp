// Kernels of the shape-generic TransformerVAE inference route (vae_wide_api.hip: the scldm_vaew_* entries): every shape of the
// family include/scldm_hip.h lists that is not the 32-wide vae_base shape, whose route and kernels (mcab.hpp) stay as they are.
//
// The model is walked as a chain of launches over plain row-major fp32 buffers in the caller's workspace:
//   gemm_kernel<P, EPI>   Y[M, N] = X[M, K] W[N, K]^T for every n x n / n x 2n / n x 3n / n x hidden product, on the product core of
//                         scvi_tile.hpp (64 x 64 tile, masked loads: M, N, K arbitrary; one accumulator per element walked in ascending
//                         k, so a row's bits depend neither on the other rows nor on how the cells were chunked).  P = F32Operands
//                         (v_mfma_f32_32x32x2_f32, exact) or F16Operands (v_mfma_f32_32x32x16_f16, operands rounded while they are
//                         staged: the reference's TF32 class).  The weights are read where the parameters live, in torch's Linear
//                         layout: nothing derived from them is kept between calls, so nothing can go stale.
//                         Epilogues: STORE | RESID (+ a residual row: the same row, a row modulo the inducing points, or a gathered
//                         table row, and optionally a second modulo row: pos_embed) | SWIGLU (the tile's columns [0, 32) come from w1,
//                         [32, 64) from w2 for the SAME 32 hidden units; SiLU(a) b leaves through LDS).
//   ln_rows_kernel        one wave per row: (gathered table row x log1p(count) | plain row) -> LayerNorm, affine or not; fp32
//                         statistics, two passes over registers, cross-lane sums.
//   attn_kernel           softmax(q k^T / sqrt(hd)) v per (cell, head), fp32 on the VALU: a workgroup stages a chunk of keys and
//                         values of its head in LDS, a wave owns four queries at a time, lane j scores key j, lane d accumulates
//                         output feature d.  Key chunks have a fixed size (a function of the head dim alone) and are folded into the
//                         running (max, sum, acc) in ascending chunk order: online softmax, no atomics.  A key axis longer than
//                         kAttnSplitChunks chunks (the pooling's S) is split over workgroups, each leaving its (max, sum, acc) per
//                         query; attn_merge_kernel folds them in split order.  The same kernel pools (n_inducing queries, S keys),
//                         runs the trunk's self-attention and unpools (G queries, n_inducing keys: one chunk, staged once per
//                         workgroup).
//   nb_logits_kernel      the n -> 1 | 2 head: logits (+ theta) and one (max, sum exp) pair per 256 genes;
//   nb_finalize_kernel    merges a row's pairs in chunk order and rewrites mu = library_size * softmax in place.
#pragma once
#include "scvi_tile.hpp"

namespace scldm {
namespace vaew {

using scvi::F16Operands;
using scvi::F32Operands;
using scvi::kBM;
using scvi::kBN;

constexpr int kMaxEmbed = 1024;            // a lane of a row kernel carries kMaxEmbed / 64 values
constexpr int kRowVals = kMaxEmbed / 64;
constexpr int kAttnGroup = 16;             // queries a workgroup handles at a time: four per wave
constexpr int kAttnQueriesPerBlock = 256;  // queries per workgroup (the decoder's gene axis)
constexpr int kAttnLdsFloats = 4096;       // keys per chunk = min(64, kAttnLdsFloats / head_dim)
constexpr int kAttnSplitChunks = 8;        // key chunks per workgroup: longer key axes (the pooling's S) are split over workgroups
constexpr int kNbChunk = 256;              // genes per (max, sum exp) pair
constexpr int kNbFinal = 1024;             // genes per workgroup of the finalize pass

enum : int { EPI_STORE = 0, EPI_RESID = 1, EPI_SWIGLU = 2 };

struct GemmArgs {
  const float* X;        // (M, K)
  const float* W0;       // (N, K)
  const float* W1;       // SWIGLU: w2, same shape as W0 (= w1)
  float* out;            // (M, N)
  int M, N, K;
  const float* R;        // RESID: residual rows of width N
  const int64_t* ridx;   // RESID: row m adds R[clamp(ridx[m])] (the gene table), else
  int rmod;              // RESID: > 0: row m adds R[m % rmod]; 0: R[m] (out may alias R)
  int ridx_max;          // largest valid table row
  const float* R2;       // RESID: optional second residual, row m % r2mod
  int r2mod;
};

template <class P, int EPI>
__global__ __launch_bounds__(256) void gemm_kernel(const GemmArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[scvi::kSmemBytes<P>];
  constexpr bool kDual = EPI == EPI_SWIGLU;
  constexpr int kCols = kDual ? 32 : 64;
  scvi::RowLoader<P, false> la(a.X, blockIdx.x * kBM, a.M, a.K);
  scvi::RowLoader<P, false> lb(a.W0, a.W1, kDual, blockIdx.y * kCols, a.N, a.K);
  const f32x16 acc = scvi::tile_product<P>(la, lb, smem, 0, a.K);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1, hh = lane >> 5, l31 = lane & 31;
  const int m0 = blockIdx.x * kBM, n0 = blockIdx.y * kCols;
  if (EPI == EPI_SWIGLU) {
    float* tile = reinterpret_cast<float*>(smem);   // (64, 33): the w1 half of the tile
    if (wn == 0) {
#pragma unroll
      for (int r = 0; r < 16; ++r) tile[(wm * 32 + acc_row(r, hh)) * 33 + l31] = acc[r];
    }
    __syncthreads();
    const int n = n0 + l31;
    if (wn == 1 && n < a.N) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = wm * 32 + acc_row(r, hh), m = m0 + row;
        if (m < a.M) a.out[(size_t)m * a.N + n] = silu_f(tile[row * 33 + l31]) * acc[r];
      }
    }
  } else {
    const int n = n0 + wn * 32 + l31;
    if (n >= a.N) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + wm * 32 + acc_row(r, hh);
      if (m >= a.M) continue;
      float v = acc[r];
      if (EPI == EPI_RESID) {
        size_t rr = m;
        if (a.ridx) {
          const int64_t g = a.ridx[m];
          rr = (size_t)(g < 0 ? 0 : (g > a.ridx_max ? a.ridx_max : g));
        } else if (a.rmod > 0) {
          rr = m % a.rmod;
        }
        v += a.R[rr * a.N + n];
        if (a.R2) v += a.R2[(size_t)(m % a.r2mod) * a.N + n];
      }
      a.out[(size_t)m * a.N + n] = v;
    }
  }
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// ---- row kernel: out[row] = LayerNorm(scale * src_row) (* w + b).  src_row = src[clamp(gidx[row])] when gidx is given (a table of
// idx_max + 1 rows), else src[row]; scale = log1p(counts[row]) when counts is given.  w == NULL: no affine.  n in [1, kMaxEmbed].
struct LnArgs {
  const float* src;
  const int64_t* gidx;
  int idx_max;
  const float* counts;
  const float* w;
  const float* b;
  float* out;
  long long rows;
  int n;
  float eps;
};

__global__ __launch_bounds__(256) void ln_rows_kernel(const LnArgs a) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.rows) return;
  size_t sr = (size_t)row;
  if (a.gidx) {
    const int64_t g = a.gidx[row];
    sr = (size_t)(g < 0 ? 0 : (g > a.idx_max ? a.idx_max : g));
  }
  const float* x = a.src + sr * a.n;
  const float sc = a.counts ? log1pf(a.counts[row]) : 1.f;
  float v[kRowVals];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < kRowVals; ++i) {
    const int d = lane + 64 * i;
    v[i] = d < a.n ? x[d] * sc : 0.f;
    s += v[i];
  }
  const float mean = wave_sum(s) / (float)a.n;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < kRowVals; ++i) {
    const int d = lane + 64 * i;
    v[i] = d < a.n ? v[i] - mean : 0.f;
    q += v[i] * v[i];
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)a.n + a.eps);
  float* o = a.out + (size_t)row * a.n;
#pragma unroll
  for (int i = 0; i < kRowVals; ++i) {
    const int d = lane + 64 * i;
    if (d < a.n) {
      float y = v[i] * rstd;
      if (a.w) y = y * a.w[d] + a.b[d];
      o[d] = y;
    }
  }
}

// ---- attention.  Query (b, m) of head h is Q[b q_bs + m q_ld + h hd ..], key / value s of cell b K / V[b kv_bs + s kv_ld + h hd ..],
// the output O[(b M + m) o_ld + h hd ..].  grid (query blocks, heads, cells); dynamic LDS attn_lds_bytes(hd).
struct AttnArgs {
  const float* Q;
  size_t q_bs;
  int q_ld;
  const float* K;
  const float* V;
  size_t kv_bs;
  int kv_ld;
  float* O;
  int o_ld;
  int M, S, hd, kc;
  float scale;
  int splits, keys_per_split;   // splits > 1: workgroup (query block, split) writes part[((b heads + h) M + m) splits + split][hd + 2]
  float* part;                  //             = acc[hd] | max | sum, unnormalised
};
static inline int attn_key_chunk(int hd) { return kAttnLdsFloats / hd < 64 ? kAttnLdsFloats / hd : 64; }
static inline int attn_keys_per_split(int hd) { return kAttnSplitChunks * attn_key_chunk(hd); }
static inline size_t attn_lds_bytes(int hd) {
  const int kc = attn_key_chunk(hd);
  return ((size_t)kc * (hd + 1) + (size_t)kc * hd + (size_t)kAttnGroup * hd + 4 * 64) * sizeof(float);
}

__global__ __launch_bounds__(256) void attn_kernel(const AttnArgs a) {
  extern __shared__ float attn_sm[];
  const int hd = a.hd, kc = a.kc, ldk = hd + 1;
  float* Ks = attn_sm;                    // (kc, hd + 1): lane j walks row j, the odd stride keeps the 64 rows on different banks
  float* Vs = Ks + kc * ldk;              // (kc, hd)
  float* Qs = Vs + kc * hd;               // (kAttnGroup, hd)
  float* Ps = Qs + kAttnGroup * hd;       // (4, 64): a wave's probabilities of the chunk
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int head = blockIdx.y, b = blockIdx.z;
  const float* Qb = a.Q + (size_t)b * a.q_bs + (size_t)head * hd;
  const float* Kb = a.K + (size_t)b * a.kv_bs + (size_t)head * hd;
  const float* Vb = a.V + (size_t)b * a.kv_bs + (size_t)head * hd;
  const int split = blockIdx.x % a.splits, qblock = blockIdx.x / a.splits;
  const int k_lo = split * a.keys_per_split, k_hi = min(a.S, k_lo + a.keys_per_split);
  const bool single = k_hi - k_lo <= kc;  // one chunk: staged once for every query group of the workgroup
  bool staged = false;
  const int q_lo = qblock * kAttnQueriesPerBlock;
  const int q_hi = min(a.M, q_lo + kAttnQueriesPerBlock);
  float* P = Ps + wave * 64;
  for (int q0 = q_lo; q0 < q_hi; q0 += kAttnGroup) {
    __syncthreads();                      // the previous group's queries (and chunk) are consumed
    for (int i = tid; i < kAttnGroup * hd; i += 256) {
      const int qi = i / hd, d = i - qi * hd, m = q0 + qi;
      Qs[i] = m < q_hi ? Qb[(size_t)m * a.q_ld + d] : 0.f;
    }
    float mx[4], l[4], acc[4][4];
#pragma unroll
    for (int qi = 0; qi < 4; ++qi) {
      mx[qi] = -INFINITY;
      l[qi] = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[qi][i] = 0.f;
    }
    for (int c0 = k_lo; c0 < k_hi; c0 += kc) {
      const int nk = min(kc, k_hi - c0);
      if (!(single && staged)) {
        if (c0 > k_lo) __syncthreads();   // the previous chunk is consumed
        for (int i = tid; i < nk * hd; i += 256) {
          const int j = i / hd, d = i - j * hd;
          const size_t g = (size_t)(c0 + j) * a.kv_ld + d;
          Ks[j * ldk + d] = Kb[g];
          Vs[j * hd + d] = Vb[g];
        }
        staged = true;
      }
      __syncthreads();
#pragma unroll
      for (int qi = 0; qi < 4; ++qi) {
        const float* q = Qs + (wave * 4 + qi) * hd;
        float s = -INFINITY;
        if (lane < nk) {
          const float* k = Ks + lane * ldk;
          float t = 0.f;
          for (int d = 0; d < hd; ++d) t = fmaf(q[d], k[d], t);
          s = t * a.scale;
        }
        const float mnew = fmaxf(mx[qi], wave_max(s));      // finite: a chunk holds at least one key
        const float p = lane < nk ? expf(s - mnew) : 0.f;
        const float corr = expf(mx[qi] - mnew);             // 0 at the first chunk
        l[qi] = l[qi] * corr + wave_sum(p);
        mx[qi] = mnew;
        P[lane] = p;                                        // read back by this wave only: LDS operations of a wave stay in order
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int d = lane + 64 * i;
          if (d < hd) {
            float t = acc[qi][i] * corr;
            for (int j = 0; j < nk; ++j) t = fmaf(P[j], Vs[j * hd + d], t);
            acc[qi][i] = t;
          }
        }
      }
    }
#pragma unroll
    for (int qi = 0; qi < 4; ++qi) {
      const int m = q0 + wave * 4 + qi;
      if (m >= q_hi) continue;
      if (a.splits > 1) {
        float* pr = a.part + ((((size_t)b * gridDim.y + head) * a.M + m) * a.splits + split) * (hd + 2);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int d = lane + 64 * i;
          if (d < hd) pr[d] = acc[qi][i];
        }
        if (lane == 0) { pr[hd] = mx[qi]; pr[hd + 1] = l[qi]; }
        continue;
      }
      float* o = a.O + ((size_t)b * a.M + m) * a.o_ld + (size_t)head * hd;
      const float inv = 1.0f / l[qi];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int d = lane + 64 * i;
        if (d < hd) o[d] = acc[qi][i] * inv;
      }
    }
  }
}

// one wave per (cell, head, query): the splits' (acc, max, sum) folded in split order.  grid cdiv(cells heads M, 4)
__global__ __launch_bounds__(256) void attn_merge_kernel(const float* __restrict__ part, float* __restrict__ O, int o_ld, long long rows, int heads,
                                                         int M, int hd, int splits) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);   // (b heads + h) M + m
  if (row >= rows) return;
  const float* pr = part + (size_t)row * splits * (hd + 2);
  float mx = -INFINITY;
  for (int s = 0; s < splits; ++s) mx = fmaxf(mx, pr[(size_t)s * (hd + 2) + hd]);
  float acc[4] = {0.f, 0.f, 0.f, 0.f}, l = 0.f;
  for (int s = 0; s < splits; ++s) {
    const float* p = pr + (size_t)s * (hd + 2);
    const float w = expf(p[hd] - mx);
    l += p[hd + 1] * w;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int d = lane + 64 * i;
      if (d < hd) acc[i] = fmaf(p[d], w, acc[i]);
    }
  }
  const int m = (int)(row % M), h = (int)((row / M) % heads);
  const long long b = row / ((long long)M * heads);
  float* o = O + ((size_t)b * M + m) * o_ld + (size_t)h * hd;
  const float inv = 1.0f / l;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int d = lane + 64 * i;
    if (d < hd) o[d] = acc[i] * inv;
  }
}

// ---- negative-binomial head (NegativeBinomialTransformerLayer, stochastic_layers.py:102-116).  grid (gene chunks of kNbChunk, cells)
struct NbArgs {
  const float* h;          // (cells, G, n): the decoder's per-gene output
  const float* head_w;     // decoder_head.params.weight (1 | 2, n)
  const float* head_b;     // (1 | 2)
  const float* theta_tab;  // decoder_head.theta.weight (n_genes + 1) or NULL: unshared theta, the second logit
  const int64_t* genes;    // (cells, G)
  int idx_max;
  float* mu;               // (cells, G): receives logit / t
  float* theta;            // (cells, G)
  float* pairs;            // (cells, chunks, 2)
  int G, n, chunks;
  float inv_temp;
};

__global__ __launch_bounds__(256) void nb_logits_kernel(const NbArgs a) {
  __shared__ float pm[4], ps[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int chunk = blockIdx.x, b = blockIdx.y;
  const bool two = a.theta_tab == nullptr;
  float w0[kRowVals], w1[kRowVals];
#pragma unroll
  for (int i = 0; i < kRowVals; ++i) {
    const int d = lane + 64 * i;
    w0[i] = d < a.n ? a.head_w[d] : 0.f;
    w1[i] = (two && d < a.n) ? a.head_w[a.n + d] : 0.f;
  }
  const int g0 = chunk * kNbChunk + wave * 64;
  float logit = -INFINITY, logit2 = 0.f;
  for (int t = 0; t < 64; ++t) {
    const int g = g0 + t;
    if (g >= a.G) break;
    const float* x = a.h + ((size_t)b * a.G + g) * a.n;
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int i = 0; i < kRowVals; ++i) {
      const int d = lane + 64 * i;
      const float xv = d < a.n ? x[d] : 0.f;
      s0 = fmaf(xv, w0[i], s0);
      s1 = fmaf(xv, w1[i], s1);
    }
    s0 = wave_sum(s0);
    if (two) s1 = wave_sum(s1);
    if (lane == t) {
      logit = (s0 + a.head_b[0]) * a.inv_temp;
      logit2 = two ? s1 + a.head_b[1] : 0.f;
    }
  }
  const int g = g0 + lane;
  if (g < a.G) {
    const size_t o = (size_t)b * a.G + g;
    a.mu[o] = logit;
    if (two) {
      a.theta[o] = expf(logit2);
    } else {
      const int64_t gi = a.genes[o];
      a.theta[o] = expf(a.theta_tab[gi < 0 ? 0 : (gi > a.idx_max ? a.idx_max : gi)]);
    }
  }
  const float wmx = wave_max(logit);
  const float wsm = wave_sum(g < a.G ? expf(logit - wmx) : 0.f);   // (a wave past G holds no gene: wmx = -inf, the sum is 0)
  if (lane == 0) { pm[wave] = wmx; ps[wave] = wsm; }
  __syncthreads();
  if (tid == 0) {
    const float M4 = fmaxf(fmaxf(pm[0], pm[1]), fmaxf(pm[2], pm[3]));
    float S = 0.f;
#pragma unroll
    for (int p = 0; p < 4; ++p) S += ps[p] > 0.f ? ps[p] * expf(pm[p] - M4) : 0.f;
    float* pr = a.pairs + ((size_t)b * a.chunks + chunk) * 2;
    pr[0] = M4;
    pr[1] = S;
  }
}

// grid (cdiv(G, kNbFinal), cells): every thread folds the row's pairs in chunk order (the same order in every thread), then rewrites
// its genes: mu = softmax(logit / t) * library_size
__global__ __launch_bounds__(256) void nb_finalize_kernel(float* __restrict__ mu, const float* __restrict__ pairs, const float* __restrict__ library,
                                                          int G, int chunks) {
  const int b = blockIdx.y;
  const float* pr = pairs + (size_t)b * chunks * 2;
  float M = -INFINITY;
  for (int c = 0; c < chunks; ++c) M = fmaxf(M, pr[2 * c]);
  float S = 0.f;
  for (int c = 0; c < chunks; ++c) S += pr[2 * c + 1] * expf(pr[2 * c] - M);
  const float lib = library[b];
  float* row = mu + (size_t)b * G;
  for (int g = blockIdx.x * kNbFinal + threadIdx.x; g < min(G, (int)(blockIdx.x + 1) * kNbFinal); g += 256) row[g] = expf(row[g] - M) / S * lib;
}

}  // namespace vaew
}  // namespace scldm

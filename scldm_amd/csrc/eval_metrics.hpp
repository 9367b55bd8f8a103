// Evaluation metrics of the validation step and the generation evaluation (src/scldm/models.py:315-331 and :892-928):
// mse, per-gene Pearson correlation (nanmean), zeros accuracy, r2 of the per-gene means and r2 of the per-gene variances
// of two count matrices pred (n_pred, G) and true (n_true, G) after U = log1p(x * target_sum / divisor).  All five are
// functions of per-gene first and second moments plus two global sums, so one streaming pass over both matrices yields
// them:
//   eval_row_scale_kernel   one workgroup per row: target_sum / (row sum), summed in a fixed order
//   eval_moments_kernel     grid (column tiles of 256 genes) x (row blocks); a lane owns one gene and walks its row block
//                           top to bottom with 8 rows of loads in flight, keeping fp32 Welford moments (two means, two
//                           M2 sums, the co-moment); the workgroup reduces sum (u - v)^2 and the zero-agreement count
//   eval_merge_kernel       per gene: the row-block partials combined in row-block order by the pairwise (Chan) update in
//                           double -> mean, unbiased variance, correlation
//   eval_finalize_kernel    one workgroup: fixed-order double sums over the genes -> the six outputs
// No atomics: every sum has one order that depends on (n_pred, n_true, G) only, so results are bit-reproducible.
// Element offsets are 64-bit (36 130 genes x 65 536 cells exceeds 2^31).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace scldm {

constexpr int kEvalTileG = 256;    // genes per workgroup of the moments pass (one per lane, 4 waves)
constexpr int kEvalMaxRB = 64;     // largest row block
constexpr int kEvalUnroll = 8;     // rows of loads in flight per lane
constexpr int kEvalMergeThreads = 64;   // one wave per workgroup: 36 130 genes still give 565 workgroups
constexpr int kEvalFinalThreads = 1024;

// rows per row block: a function of the row count alone (never of the device), so the summation order is too.  Small
// matrices get short blocks so that a validation batch still fills the chip.
__host__ __device__ inline int eval_row_block(int n) { return n >= 1024 ? 64 : (n >= 256 ? 32 : 16); }

// log1p for the scaled counts (x >= 0; NaN and +inf pass through, x < -1 gives NaN): log(u) + (x - (u - 1)) / u with
// u = fl(1 + x) - the correction term restores the bits 1 + x rounded away, which keeps small x at full relative
// precision - on the hardware log2 (1 ulp) instead of the library's polynomial: two of these per loaded pair decide
// whether the pass is bound by memory or by the VALU.
__device__ __forceinline__ float eval_log1p(float x) {
  const float u = 1.0f + x;
  const float c = (x - (u - 1.0f)) * __builtin_amdgcn_rcpf(u);
  const float r = fmaf(__builtin_amdgcn_logf(u), 0.693147180559945309f, c);
  return u == __builtin_inff() ? u : r;
}

// sum of one row in a fixed order: 256 strided fp32 lane sums, then a double tree.  All threads return the sum.
__device__ __forceinline__ double eval_block_row_sum(const float* __restrict__ row, int G, double* sh) {
  float s = 0.f;
  for (int g = threadIdx.x; g < G; g += 256) s += row[g];
  sh[threadIdx.x] = (double)s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  const double tot = sh[0];
  __syncthreads();
  return tot;
}

__global__ __launch_bounds__(256) void eval_row_scale_kernel(const float* __restrict__ x, int G, float target_sum, float* __restrict__ scale) {
  __shared__ double sh[256];
  const double tot = eval_block_row_sum(x + (size_t)blockIdx.x * G, G, sh);
  if (threadIdx.x == 0) scale[blockIdx.x] = target_sum / (float)tot;
}

// out = log1p(x * target_sum / divisor); one workgroup per row; div == NULL: the row's own sum (the second read of the
// row comes from cache).  target_sum <= 0: a copy.
__global__ __launch_bounds__(256) void eval_log1p_normalize_kernel(const float* __restrict__ x, int G, const float* __restrict__ div,
                                                                   float target_sum, float* __restrict__ out) {
  __shared__ double sh[256];
  const float* row = x + (size_t)blockIdx.x * G;
  float* orow = out + (size_t)blockIdx.x * G;
  if (!(target_sum > 0.f)) {
    for (int g = threadIdx.x; g < G; g += 256) orow[g] = row[g];
    return;
  }
  const float s = div ? target_sum / div[blockIdx.x] : target_sum / (float)eval_block_row_sum(row, G, sh);
  for (int g = threadIdx.x; g < G; g += 256) orow[g] = eval_log1p(row[g] * s);
}

// Reconstruction loss of the Gaussian head before .mean() (models.py:239-245 with distributions.py:45-62, sigma = None):
//   loss_rows[b] = sum_g (log1p(counts[b, g] / rowsum_b * target_sum) - mu[b, g])^2
// One workgroup per row, two passes over the row (its sum, then the squared error; the second read comes from cache), the
// scaled counts exactly those of eval_log1p_normalize_kernel (an all-zero row: 0 * inf = NaN, as there and as in the reference).
// 256 strided fp32 lane sums, then a double tree: one order, bit-reproducible.
__global__ __launch_bounds__(256) void gaussian_recon_loss_kernel(const float* __restrict__ counts, const float* __restrict__ mu, int G,
                                                                  float target_sum, float* __restrict__ loss_rows) {
  __shared__ double sh[256];
  const float* row = counts + (size_t)blockIdx.x * G;
  const float* mrow = mu + (size_t)blockIdx.x * G;
  const bool raw = !(target_sum > 0.f);
  const float s = raw ? 1.0f : target_sum / (float)eval_block_row_sum(row, G, sh);
  float acc = 0.f;
  for (int g = threadIdx.x; g < G; g += 256) {
    const float d = (raw ? row[g] : eval_log1p(row[g] * s)) - mrow[g];
    acc = fmaf(d, d, acc);
  }
  sh[threadIdx.x] = (double)acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss_rows[blockIdx.x] = (float)sh[0];
}
// ... and its gradient with respect to mu in one pass: dmu[b, g] = -2 (y[b, g] - mu[b, g]) gout_rows[b], y recomputed exactly as above
// (the training step of the Gaussian head: mu requires grad, counts do not)
__global__ __launch_bounds__(256) void gaussian_recon_loss_bwd_kernel(const float* __restrict__ counts, const float* __restrict__ mu,
                                                                      const float* __restrict__ gout_rows, int G, float target_sum,
                                                                      float* __restrict__ dmu) {
  __shared__ double sh[256];
  const float* row = counts + (size_t)blockIdx.x * G;
  const float* mrow = mu + (size_t)blockIdx.x * G;
  float* drow = dmu + (size_t)blockIdx.x * G;
  const bool raw = !(target_sum > 0.f);
  const float s = raw ? 1.0f : target_sum / (float)eval_block_row_sum(row, G, sh);
  const float go = -2.0f * gout_rows[blockIdx.x];
  for (int g = threadIdx.x; g < G; g += 256) drow[g] = ((raw ? row[g] : eval_log1p(row[g] * s)) - mrow[g]) * go;
}

// Partials: `part` holds 5 planes (mean_u, M2_u, mean_v, M2_v, C_uv) of (plane_rows, G) floats, row = row block.
// PAIRED: a and b are pred and true with the same n; all five planes and the workgroup's (sum (u-v)^2, zero agreement)
// pair are written.  !PAIRED: only `a` is read and planes slot, slot + 1 are written (the r2 metrics of two matrices
// with different row counts).  RAW: the inputs are already scaled (target_sum <= 0).
// sa / sb: per-row multiplier (is_div = 0) or divisor (is_div = 1: the multiplier is target_sum / divisor).
template <bool PAIRED, bool RAW>
__global__ __launch_bounds__(256) void eval_moments_kernel(const float* __restrict__ a, const float* __restrict__ b, int n, int G, int rb,
                                                           const float* __restrict__ sa, int sa_is_div, const float* __restrict__ sb,
                                                           int sb_is_div, float target_sum, float* __restrict__ part, size_t plane,
                                                           int slot, double* __restrict__ wg_out) {
  __shared__ float s_a[kEvalMaxRB], s_b[kEvalMaxRB];
  __shared__ double red[8];
  const int tid = threadIdx.x;
  const int g = blockIdx.x * kEvalTileG + tid;
  const bool live = g < G;
  const int gc = live ? g : G - 1;   // dead lanes re-read the last gene (in bounds) and write nothing
  const int r0 = blockIdx.y * rb;
  const int rows = min(rb, n - r0);
  if (!RAW) {
    if (tid < rows) {
      s_a[tid] = sa_is_div ? target_sum / sa[r0 + tid] : sa[r0 + tid];
      if (PAIRED) s_b[tid] = sb_is_div ? target_sum / sb[r0 + tid] : sb[r0 + tid];
    }
    __syncthreads();
  }
  const float* pa = a + (size_t)r0 * G + gc;
  const float* pb = PAIRED ? b + (size_t)r0 * G + gc : nullptr;
  float mu = 0.f, m2u = 0.f, mv = 0.f, m2v = 0.f, cuv = 0.f, sq = 0.f;
  int agree = 0;
  // one row: transform, Welford update of the five moments, the two global sums.  The row index is wave-uniform, so the
  // reciprocal of the count is computed once per row.
  auto update = [&](int row, float xav, float xbv) {
    const float inv = row == 0 ? 1.0f : __builtin_amdgcn_rcpf((float)(row + 1));
    const float u = RAW ? xav : eval_log1p(xav * s_a[row]);
    const float du = u - mu;
    mu = fmaf(du, inv, mu);
    m2u = fmaf(du, u - mu, m2u);
    if (PAIRED) {
      const float v = RAW ? xbv : eval_log1p(xbv * s_b[row]);
      const float dv = v - mv;
      mv = fmaf(dv, inv, mv);
      m2v = fmaf(dv, v - mv, m2v);
      cuv = fmaf(du, v - mv, cuv);
      const float d = u - v;
      sq = fmaf(d, d, sq);
      agree += ((xav == 0.f) == (xbv == 0.f)) ? 1 : 0;
    }
  };
  int r = 0;
  for (; r + kEvalUnroll <= rows; r += kEvalUnroll) {   // whole chunks: all loads issued before the first use
    float xa[kEvalUnroll], xb[kEvalUnroll];
#pragma unroll
    for (int k = 0; k < kEvalUnroll; ++k) {
      xa[k] = pa[(size_t)(r + k) * G];
      xb[k] = PAIRED ? pb[(size_t)(r + k) * G] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < kEvalUnroll; ++k) update(r + k, xa[k], xb[k]);
  }
  for (; r < rows; ++r) update(r, pa[(size_t)r * G], PAIRED ? pb[(size_t)r * G] : 0.f);   // the last block's ragged end
  if (live) {
    const size_t o = (size_t)blockIdx.y * G + g;
    part[(size_t)slot * plane + o] = mu;
    part[(size_t)(slot + 1) * plane + o] = m2u;
    if (PAIRED) {
      part[2 * plane + o] = mv;
      part[3 * plane + o] = m2v;
      part[4 * plane + o] = cuv;
    }
  }
  if (PAIRED) {
    double dsq = live ? (double)sq : 0.0, dag = live ? (double)agree : 0.0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      dsq += __shfl_xor(dsq, o);
      dag += __shfl_xor(dag, o);
    }
    if ((tid & 63) == 0) {
      red[tid >> 6] = dsq;
      red[4 + (tid >> 6)] = dag;
    }
    __syncthreads();
    if (tid == 0) {
      const size_t w = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
      wg_out[2 * w] = (red[0] + red[1]) + (red[2] + red[3]);
      wg_out[2 * w + 1] = (red[4] + red[5]) + (red[6] + red[7]);
    }
  }
}

// one matrix's row-block partials of gene g combined in row-block order (Chan et al.): mean and M2 in double
__device__ __forceinline__ void eval_merge_one(const float* __restrict__ pmean, const float* __restrict__ pm2, int g, int G, int n, int rb,
                                               double& mean, double& m2) {
  const int nrb = (n + rb - 1) / rb;
  double na = 0.0;
  mean = 0.0;
  m2 = 0.0;
#pragma unroll 4
  for (int k = 0; k < nrb; ++k) {
    const double nb = (double)min(rb, n - k * rb), nt = na + nb;
    const double mb = (double)pmean[(size_t)k * G + g], d = mb - mean;
    m2 += (double)pm2[(size_t)k * G + g] + d * d * (na * nb / nt);
    mean += d * (nb / nt);
    na = nt;
  }
}

// gene_d: 5 planes of G doubles (mean_p, var_p, mean_t, var_t, pcc) for the finalize pass
__global__ __launch_bounds__(kEvalMergeThreads) void eval_merge_kernel(const float* __restrict__ part, size_t plane, int G, int n_pred, int n_true, int paired,
                                                         double* __restrict__ gene_d, float* __restrict__ pcc_out, float* __restrict__ stats_out) {
  const int g = blockIdx.x * kEvalMergeThreads + threadIdx.x;
  if (g >= G) return;
  const double nan = __builtin_nan("");
  double mp, m2p, mt, m2t, pcc = nan;
  if (paired) {
    const int n = n_pred, rb = eval_row_block(n), nrb = (n + rb - 1) / rb;
    double na = 0.0, c = 0.0;
    mp = m2p = mt = m2t = 0.0;
#pragma unroll 4
    for (int k = 0; k < nrb; ++k) {   // unrolled: the partial loads of four row blocks are in flight, the order of the sums is unchanged
      const size_t o = (size_t)k * G + g;
      const double nb = (double)min(rb, n - k * rb), nt = na + nb, w = na * nb / nt;
      const double du = (double)part[o] - mp, dv = (double)part[2 * plane + o] - mt;
      m2p += (double)part[plane + o] + du * du * w;
      m2t += (double)part[3 * plane + o] + dv * dv * w;
      c += (double)part[4 * plane + o] + du * dv * w;
      mp += du * (nb / nt);
      mt += dv * (nb / nt);
      na = nt;
    }
    if (n >= 2 && m2p > 0.0 && m2t > 0.0) {   // a zero (or NaN) variance leaves the correlation undefined: NaN
      pcc = c / (sqrt(m2p) * sqrt(m2t));
      if (pcc > 1.0) pcc = 1.0;
      if (pcc < -1.0) pcc = -1.0;
    }
  } else {
    eval_merge_one(part, part + plane, g, G, n_pred, eval_row_block(n_pred), mp, m2p);
    eval_merge_one(part + 2 * plane, part + 3 * plane, g, G, n_true, eval_row_block(n_true), mt, m2t);
  }
  const double vp = m2p / (double)(n_pred - 1), vt = m2t / (double)(n_true - 1);   // n = 1: 0 / 0 = NaN, as torch's .var(0)
  gene_d[g] = mp;
  gene_d[(size_t)G + g] = vp;
  gene_d[2 * (size_t)G + g] = mt;
  gene_d[3 * (size_t)G + g] = vt;
  gene_d[4 * (size_t)G + g] = pcc;
  if (pcc_out) pcc_out[g] = (float)pcc;
  if (stats_out) {
    stats_out[g] = (float)mp;
    stats_out[(size_t)G + g] = (float)vp;
    stats_out[2 * (size_t)G + g] = (float)mt;
    stats_out[3 * (size_t)G + g] = (float)vt;
  }
}

// N sums over the workgroup in a fixed order (one tree over kEvalFinalThreads slots for all of them); every thread gets the totals
template <int N>
__device__ __forceinline__ void eval_final_sum(double (&v)[N], double (*sh)[kEvalFinalThreads]) {
#pragma unroll
  for (int i = 0; i < N; ++i) sh[i][threadIdx.x] = v[i];
  __syncthreads();
  for (int o = kEvalFinalThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
#pragma unroll
      for (int i = 0; i < N; ++i) sh[i][threadIdx.x] += sh[i][threadIdx.x + o];
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = sh[i][0];
  __syncthreads();
}

// out: SCLDM_EVAL_MSE, _PCC, _ZEROS, _R2_MEAN, _R2_VAR, _PCC_VALID.  r2(preds, target) = 1 - sum (target - preds)^2 /
// sum (target - mean(target))^2 with preds = pred's per-gene statistic and target = true's.
__global__ __launch_bounds__(kEvalFinalThreads) void eval_finalize_kernel(const double* __restrict__ gene_d, int G, const double* __restrict__ wg,
                                                                          int n_wg, double cells, int paired, double* __restrict__ out) {
  __shared__ double sh[6][kEvalFinalThreads];
  const int tid = threadIdx.x;
  const double *mp = gene_d, *vp = gene_d + G, *mt = gene_d + 2 * (size_t)G, *vt = gene_d + 3 * (size_t)G, *pc = gene_d + 4 * (size_t)G;
  double s_mt = 0.0, s_vt = 0.0, s_pc = 0.0, n_pc = 0.0, s_sq = 0.0, s_ag = 0.0;
  for (int g = tid; g < G; g += kEvalFinalThreads) {
    s_mt += mt[g];
    s_vt += vt[g];
    const double p = pc[g];
    if (p == p) {
      s_pc += p;
      n_pc += 1.0;
    }
  }
  if (paired)
    for (int w = tid; w < n_wg; w += kEvalFinalThreads) {
      s_sq += wg[2 * w];
      s_ag += wg[2 * w + 1];
    }
  double a6[6] = {s_mt, s_vt, s_pc, n_pc, s_sq, s_ag};
  eval_final_sum<6>(a6, sh);
  s_mt = a6[0], s_vt = a6[1], s_pc = a6[2], n_pc = a6[3], s_sq = a6[4], s_ag = a6[5];
  const double mean_mt = s_mt / G, mean_vt = s_vt / G;
  double rm = 0.0, tm = 0.0, rv = 0.0, tv = 0.0;
  for (int g = tid; g < G; g += kEvalFinalThreads) {
    const double a = mt[g] - mp[g], b = mt[g] - mean_mt, c = vt[g] - vp[g], d = vt[g] - mean_vt;
    rm += a * a;
    tm += b * b;
    rv += c * c;
    tv += d * d;
  }
  double a4[4] = {rm, tm, rv, tv};
  eval_final_sum<4>(a4, sh);
  rm = a4[0], tm = a4[1], rv = a4[2], tv = a4[3];
  if (tid == 0) {
    const double nan = __builtin_nan("");
    out[0] = paired ? s_sq / (cells * G) : nan;
    out[1] = n_pc > 0.0 ? s_pc / n_pc : nan;
    out[2] = paired ? s_ag / (cells * G) : nan;
    out[3] = 1.0 - rm / tm;
    out[4] = 1.0 - rv / tv;
    out[5] = n_pc;
  }
}

}  // namespace scldm

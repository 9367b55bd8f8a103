// Kernels of the training backward of the shape-generic TransformerVAE route (vae_wide_train_api.hip: scldm_vaew_train_backward).
// The forward record of a cell chunk is rebuilt with the inference kernels of vae_wide.hpp; what is here walks it back.  Everything is
// fp32, and every sum has one fixed order: no float atomics.
//
//   products              scvi_train::prod_kernel<F32Operands, AT, false> (TN: dW = dY^T X, NN: dX = dY W) into slots, then
//                         scvi_train::sum_slots_kernel (data gradients) or acc_slots_kernel (weight gradients: += the slots in slot
//                         order, so the chunks of a call accumulate in chunk order).
//   ln_bwd_kernel         one wave per row, values in registers: dx of LayerNorm (affine or not; the source row plain, or gathered
//                         from the gene table and scaled by log1p(count), its gradient scaled back), optionally + a carried gradient
//                         row.  A workgroup owns kColRows consecutive rows, a quarter per wave in ascending order; the waves' dgamma / dbeta
//                         sums are added in wave order and leave as one partial per workgroup, colpart_merge_kernel adds the partials
//                         in workgroup order.
//   nb_bwd_row_kernel     the NB head per cell: s = sum mu dmu (fixed order), dlogit, dlogit2 / the theta table's per-entry rows.
//   nb_bwd_h_kernel       per gene row: dh = dlogit (x) W_head in place of h, the head's weight / bias partials like ln_bwd_kernel's.
//   swiglu_fwd / _bwd     elementwise over the recorded pre-activations a, b.
//   attn_stats_kernel     first sweep of the attention backward: per query (max, 1 / sum exp) of its scores and D = dO . O.
//   attn_bwd_q_kernel     one wave per (query, key split): lane j scores key j of a 64-key chunk from the recorded Q, K, V, lane d
//                         accumulates dQ feature d over the keys in ascending order.
//   attn_bwd_kv_kernel    one wave per (key, query split): the same with the roles exchanged, dK and dV.
//                         Splits leave partials which sum_slots_kernel adds in split order.
//   cell_sum_acc_kernel   out += the cells' rows in cell order (the inducing points' residual and the shared queries' dQ).
//   table_rows_sum_kernel / theta_rows_sum_kernel   the fixed-order segmented sums of the two embedding tables' per-entry rows.
#pragma once
#include "scvi_prod.hpp"
#include "vae_wide_host.hpp"

namespace scldm {
namespace vaewt {

constexpr int kMaxEmbed = vaew_host::kWideMaxEmbed;   // a lane of a row kernel carries kMaxEmbed / 64 values
constexpr int kRowVals = kMaxEmbed / 64;

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

constexpr int kColRows = 64;          // rows per workgroup of a kernel that leaves column partials: kColRows / 4 per wave
constexpr int kAttnBwdQuerySplit = 256;   // queries per split of attn_bwd_kv_kernel (the decoder's gene axis)
constexpr int kMaxSlots = 16;         // k-splits of a weight gradient

// out += slot 0 + slot 1 + ... in slot order
__global__ __launch_bounds__(256) void acc_slots_kernel(const float* __restrict__ part, int slots, size_t plane, float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= plane) return;
  float v = part[i];
  for (int z = 1; z < slots; ++z) v += part[z * plane + i];
  out[i] += v;
}

// The four waves' column sums acc[a][i] (column lane + 64 i of array a) added in wave order through sm (NA * kMaxEmbed floats), then
// written to part (NA, n).  Every thread of the workgroup calls it.
template <int NA>
__device__ __forceinline__ void waves_to_part(const float (&acc)[NA][kRowVals], int n, float* sm, float* part) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int i = 0; i < kRowVals; ++i) {
          const int d = lane + 64 * i;
          if (d < n) sm[a * kMaxEmbed + d] = w ? sm[a * kMaxEmbed + d] + acc[a][i] : acc[a][i];
        }
    }
    __syncthreads();
  }
  for (int i = threadIdx.x; i < NA * n; i += 256) part[i] = sm[(i / n) * kMaxEmbed + i % n];
}

// out[k][o] += part[0][c] + part[1][c] + ... for column c = offset o of segment k (a NULL segment is skipped).  grid cdiv(width, 256)
struct MergeArgs {
  const float* part;   // (blocks, width)
  int blocks, width;
  float* out[4];
  int len[4];
};
__global__ __launch_bounds__(256) void colpart_merge_kernel(const MergeArgs a) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= a.width) return;
  float s = a.part[c];
  for (int b = 1; b < a.blocks; ++b) s += a.part[(size_t)b * a.width + c];
  int k = 0, o = c;
  while (k < 3 && o >= a.len[k]) o -= a.len[k++];
  if (a.out[k] && o < a.len[k]) a.out[k][o] += s;
}

// ---- LayerNorm backward.  x = scale * src_row as in vaew::ln_rows_kernel; dx[row] = (add ? add[row] : 0) + scale * dLN(dy[row]).
struct LnBwdArgs {
  const float* src;
  const int64_t* gidx;
  int idx_max;
  const float* counts;
  const float* w;        // gamma, or NULL: no affine
  const float* dy;       // (rows, n)
  const float* add;      // (rows, n) or NULL; may be dx
  float* dx;             // (rows, n)
  float* part;           // (workgroups, 2, n): dgamma | dbeta; NULL without affine
  long long rows;
  int n;
  float eps;
};

__global__ __launch_bounds__(256) void ln_bwd_kernel(const LnBwdArgs a) {
  __shared__ float sm[2 * kMaxEmbed];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float dg[2][kRowVals];
#pragma unroll
  for (int i = 0; i < kRowVals; ++i) dg[0][i] = dg[1][i] = 0.f;
  const long long r0 = (long long)blockIdx.x * kColRows + wave * (kColRows / 4);
  for (int t = 0; t < kColRows / 4; ++t) {
    const long long row = r0 + t;
    if (row >= a.rows) break;
    size_t sr = (size_t)row;
    if (a.gidx) {
      const int64_t g = a.gidx[row];
      sr = (size_t)(g < 0 ? 0 : (g > a.idx_max ? a.idx_max : g));
    }
    const float* x = a.src + sr * a.n;
    const float sc = a.counts ? log1pf(a.counts[row]) : 1.f;
    float v[kRowVals], g[kRowVals];
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
    const float* dy = a.dy + (size_t)row * a.n;
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < kRowVals; ++i) {
      const int d = lane + 64 * i;
      v[i] *= rstd;                                   // xhat
      const float y = d < a.n ? dy[d] : 0.f;
      dg[0][i] += y * v[i];
      dg[1][i] += y;
      g[i] = (a.w && d < a.n) ? y * a.w[d] : y;
      s1 += g[i];
      s2 += g[i] * v[i];
    }
    const float c1 = wave_sum(s1) / (float)a.n, c2 = wave_sum(s2) / (float)a.n;
    const float* ad = a.add ? a.add + (size_t)row * a.n : nullptr;
    float* o = a.dx + (size_t)row * a.n;
#pragma unroll
    for (int i = 0; i < kRowVals; ++i) {
      const int d = lane + 64 * i;
      if (d < a.n) {
        const float r = rstd * (g[i] - c1 - v[i] * c2) * sc;
        o[d] = ad ? ad[d] + r : r;
      }
    }
  }
  if (a.part) waves_to_part<2>(dg, a.n, sm, a.part + (size_t)blockIdx.x * 2 * a.n);
}

// ---- NB head backward.  grid (cells): mu = library softmax(logit / t), so dlogit_g = (mu_g dmu_g - (mu_g / library) s) / t with
// s = sum_j mu_j dmu_j (thread-strided sums, the wave's xor tree, the four waves in order); zeros for library 0.  theta = exp(.):
// d(.) = dtheta theta, the second logit's gradient (dl2) or the per-entry row of the theta table (trows).
struct NbRowArgs {
  const float *mu, *theta, *dmu, *dtheta, *library;   // (cells, G) x 4 (dmu / dtheta may be NULL), (cells)
  int G;
  float inv_temp;
  float *dl, *dl2, *trows;                            // (cells, G); dl2 (unshared theta) or trows (shared) is NULL
};
__global__ __launch_bounds__(256) void nb_bwd_row_kernel(const NbRowArgs a) {
  __shared__ float red[4];
  const int row = blockIdx.x, tid = threadIdx.x;
  const size_t o = (size_t)row * a.G;
  float s = 0.f;
  if (a.dmu)
    for (int g = tid; g < a.G; g += 256) s += a.mu[o + g] * a.dmu[o + g];
  s = wave_sum(s);
  if ((tid & 63) == 0) red[tid >> 6] = s;
  __syncthreads();
  s = ((red[0] + red[1]) + red[2]) + red[3];
  const float lib = a.library[row];
  for (int g = tid; g < a.G; g += 256) {
    const float m = a.mu[o + g];
    a.dl[o + g] = (a.dmu && lib != 0.f) ? (m * a.dmu[o + g] - (m / lib) * s) * a.inv_temp : 0.f;
    const float dt = a.dtheta ? a.dtheta[o + g] * a.theta[o + g] : 0.f;
    if (a.dl2) a.dl2[o + g] = dt;
    else a.trows[o + g] = dt;
  }
}

// one wave per gene row, rows as in ln_bwd_kernel: h[row] <- dl[row] W[0] (+ dl2[row] W[1]); partials (workgroups, 2 n + 2):
// dW[0] | dW[1] | db[0] | db[1] (the second logit's are zero under shared theta)
struct NbHArgs {
  float* h;              // (rows, n): the decoder's output on entry, its gradient on exit
  const float *dl, *dl2; // (rows); dl2 may be NULL
  const float* head_w;   // (1 | 2, n)
  float* part;
  long long rows;
  int n;
};
__global__ __launch_bounds__(256) void nb_bwd_h_kernel(const NbHArgs a) {
  __shared__ float sm[2 * kMaxEmbed];
  __shared__ float sb[4][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float dw[2][kRowVals], w0[kRowVals], w1[kRowVals];
#pragma unroll
  for (int i = 0; i < kRowVals; ++i) {
    const int d = lane + 64 * i;
    dw[0][i] = dw[1][i] = 0.f;
    w0[i] = d < a.n ? a.head_w[d] : 0.f;
    w1[i] = (a.dl2 && d < a.n) ? a.head_w[a.n + d] : 0.f;
  }
  float b0 = 0.f, b1 = 0.f;
  const long long r0 = (long long)blockIdx.x * kColRows + wave * (kColRows / 4);
  for (int t = 0; t < kColRows / 4; ++t) {
    const long long row = r0 + t;
    if (row >= a.rows) break;
    const float g0 = a.dl[row], g1 = a.dl2 ? a.dl2[row] : 0.f;
    float* x = a.h + (size_t)row * a.n;
    b0 += g0;
    b1 += g1;
#pragma unroll
    for (int i = 0; i < kRowVals; ++i) {
      const int d = lane + 64 * i;
      if (d < a.n) {
        const float xv = x[d];
        dw[0][i] = fmaf(g0, xv, dw[0][i]);
        dw[1][i] = fmaf(g1, xv, dw[1][i]);
        x[d] = fmaf(g1, w1[i], g0 * w0[i]);
      }
    }
  }
  float* part = a.part + (size_t)blockIdx.x * (2 * a.n + 2);
  waves_to_part<2>(dw, a.n, sm, part);
  if (lane == 0) { sb[wave][0] = b0; sb[wave][1] = b1; }
  __syncthreads();
  if (threadIdx.x < 2) part[2 * a.n + threadIdx.x] = ((sb[0][threadIdx.x] + sb[1][threadIdx.x]) + sb[2][threadIdx.x]) + sb[3][threadIdx.x];
}

// ---- SwiGLU over the recorded pre-activations
__global__ __launch_bounds__(256) void swiglu_fwd_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ hid, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) hid[i] = silu_f(a[i]) * b[i];
}
// a <- d hid b SiLU'(a), b <- d hid SiLU(a)
__global__ __launch_bounds__(256) void swiglu_bwd_kernel(float* __restrict__ a, float* __restrict__ b, const float* __restrict__ dhid, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float x = a[i], y = b[i], d = dhid[i];
  const float sg = 1.f / (1.f + expf(-x));
  a[i] = d * y * (sg * (1.f + x * (1.f - sg)));
  b[i] = d * (x * sg);
}

// out[i] += in[0][i] + in[1][i] + ... over the cells in cell order
__global__ __launch_bounds__(256) void cell_sum_acc_kernel(const float* __restrict__ in, int cells, size_t plane, float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= plane) return;
  float v = in[i];
  for (int b = 1; b < cells; ++b) v += in[b * plane + i];
  out[i] += v;
}

// ---- attention backward.  Addressing of Q, K, V, O as in vaew::AttnArgs; dO has O's layout; stats (cells, heads, M, 3) =
// max | 1 / sum exp | D.  With p_j = exp(s_j - max) / sum:  dp_j = dO . v_j, ds_j = p_j (dp_j - D) scale, dQ = sum_j ds_j k_j,
// dK_j = sum_m ds_mj q_m, dV_j = sum_m p_mj dO_m.
struct AttnBwdArgs {
  const float* Q;
  size_t q_bs;
  int q_ld;
  const float* K;
  const float* V;
  size_t kv_bs;
  int kv_ld;
  const float* O;
  const float* dO;
  int o_ld;
  float* stats;
  int cells, heads, M, S, hd;
  float scale;
  float* dQ;             // row (b M + m) dq_ld + h hd; split z adds z * q_plane
  int dq_ld;
  size_t q_plane;
  int keys_per_split;    // attn_bwd_q_kernel: grid.y splits of the key axis
  float* dK;             // row (b S + j) dkv_ld + h hd; split z adds z * kv_plane
  float* dV;
  int dkv_ld;
  size_t kv_plane;
  int queries_per_split; // attn_bwd_kv_kernel: grid.y splits of the query axis
};

__device__ __forceinline__ float dot_rows(const float* __restrict__ x, const float* __restrict__ y, int hd) {
  const f32x4* xv = reinterpret_cast<const f32x4*>(x);
  const f32x4* yv = reinterpret_cast<const f32x4*>(y);
  float t = 0.f;
  for (int d = 0; d < hd / 4; ++d) {
    const f32x4 p = xv[d], q = yv[d];
    t = fmaf(p[0], q[0], t);
    t = fmaf(p[1], q[1], t);
    t = fmaf(p[2], q[2], t);
    t = fmaf(p[3], q[3], t);
  }
  return t;
}

// one wave per (cell, head, query).  grid cdiv(cells heads M, 4)
__global__ __launch_bounds__(256) void attn_stats_kernel(const AttnBwdArgs a) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);   // (b heads + h) M + m
  if (row >= (long long)a.cells * a.heads * a.M) return;
  const int m = (int)(row % a.M), h = (int)((row / a.M) % a.heads);
  const size_t b = (size_t)(row / ((long long)a.M * a.heads));
  const float* q = a.Q + b * a.q_bs + (size_t)m * a.q_ld + (size_t)h * a.hd;
  const float* Kb = a.K + b * a.kv_bs + (size_t)h * a.hd;
  float mx = -INFINITY, l = 0.f;
  for (int j = lane; j < a.S; j += 64) {
    const float s = dot_rows(q, Kb + (size_t)j * a.kv_ld, a.hd) * a.scale;
    const float mnew = fmaxf(mx, s);
    l = l * expf(mx - mnew) + expf(s - mnew);
    mx = mnew;
  }
  const float M = wave_max(mx);
  l = wave_sum(l > 0.f ? l * expf(mx - M) : 0.f);
  const size_t o = (b * a.M + m) * a.o_ld + (size_t)h * a.hd;
  float D = 0.f;
  for (int d = lane; d < a.hd; d += 64) D = fmaf(a.dO[o + d], a.O[o + d], D);
  D = wave_sum(D);
  if (lane == 0) {
    float* st = a.stats + (size_t)row * 3;
    st[0] = M;
    st[1] = 1.0f / l;
    st[2] = D;
  }
}

// one wave per (cell, head, query) and key split.  grid (cdiv(cells heads M, 4), key splits)
__global__ __launch_bounds__(256) void attn_bwd_q_kernel(const AttnBwdArgs a) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (long long)a.cells * a.heads * a.M) return;
  const int m = (int)(row % a.M), h = (int)((row / a.M) % a.heads);
  const size_t b = (size_t)(row / ((long long)a.M * a.heads));
  const float* q = a.Q + b * a.q_bs + (size_t)m * a.q_ld + (size_t)h * a.hd;
  const float* Kb = a.K + b * a.kv_bs + (size_t)h * a.hd;
  const float* Vb = a.V + b * a.kv_bs + (size_t)h * a.hd;
  const float* dO = a.dO + (b * a.M + m) * a.o_ld + (size_t)h * a.hd;
  const float* st = a.stats + (size_t)row * 3;
  const float mx = st[0], inv = st[1], D = st[2];
  const int k_lo = blockIdx.y * a.keys_per_split, k_hi = min(a.S, k_lo + a.keys_per_split);
  float dq[4] = {0.f, 0.f, 0.f, 0.f};
  for (int c0 = k_lo; c0 < k_hi; c0 += 64) {
    const int j = c0 + lane, nk = min(64, k_hi - c0);
    float ds = 0.f;
    if (j < k_hi) {
      const float p = expf(dot_rows(q, Kb + (size_t)j * a.kv_ld, a.hd) * a.scale - mx) * inv;
      ds = p * (dot_rows(dO, Vb + (size_t)j * a.kv_ld, a.hd) - D) * a.scale;
    }
    for (int jj = 0; jj < nk; ++jj) {
      const float w = __shfl(ds, jj);
      const float* k = Kb + (size_t)(c0 + jj) * a.kv_ld;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int d = lane + 64 * i;
        if (d < a.hd) dq[i] = fmaf(w, k[d], dq[i]);
      }
    }
  }
  float* o = a.dQ + (size_t)blockIdx.y * a.q_plane + (b * a.M + m) * a.dq_ld + (size_t)h * a.hd;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int d = lane + 64 * i;
    if (d < a.hd) o[d] = dq[i];
  }
}

// one wave per (cell, head, key) and query split.  grid (cdiv(cells heads S, 4), query splits)
__global__ __launch_bounds__(256) void attn_bwd_kv_kernel(const AttnBwdArgs a) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);   // (b heads + h) S + j
  if (row >= (long long)a.cells * a.heads * a.S) return;
  const int j = (int)(row % a.S), h = (int)((row / a.S) % a.heads);
  const size_t b = (size_t)(row / ((long long)a.S * a.heads));
  const float* Qb = a.Q + b * a.q_bs + (size_t)h * a.hd;
  const float* k = a.K + b * a.kv_bs + (size_t)j * a.kv_ld + (size_t)h * a.hd;
  const float* v = a.V + b * a.kv_bs + (size_t)j * a.kv_ld + (size_t)h * a.hd;
  const float* dOb = a.dO + b * a.M * a.o_ld + (size_t)h * a.hd;
  const float* stb = a.stats + ((b * a.heads + h) * a.M) * 3;
  const int q_lo = blockIdx.y * a.queries_per_split, q_hi = min(a.M, q_lo + a.queries_per_split);
  float dk[4] = {0.f, 0.f, 0.f, 0.f}, dv[4] = {0.f, 0.f, 0.f, 0.f};
  for (int c0 = q_lo; c0 < q_hi; c0 += 64) {
    const int m = c0 + lane, nq = min(64, q_hi - c0);
    float ds = 0.f, p = 0.f;
    if (m < q_hi) {
      const float* st = stb + (size_t)m * 3;
      p = expf(dot_rows(Qb + (size_t)m * a.q_ld, k, a.hd) * a.scale - st[0]) * st[1];
      ds = p * (dot_rows(dOb + (size_t)m * a.o_ld, v, a.hd) - st[2]) * a.scale;
    }
    for (int mm = 0; mm < nq; ++mm) {
      const float w = __shfl(ds, mm), pw = __shfl(p, mm);
      const float* q = Qb + (size_t)(c0 + mm) * a.q_ld;
      const float* g = dOb + (size_t)(c0 + mm) * a.o_ld;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int d = lane + 64 * i;
        if (d < a.hd) {
          dk[i] = fmaf(w, q[d], dk[i]);
          dv[i] = fmaf(pw, g[d], dv[i]);
        }
      }
    }
  }
  const size_t o = (size_t)blockIdx.y * a.kv_plane + (b * a.S + j) * a.dkv_ld + (size_t)h * a.hd;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int d = lane + 64 * i;
    if (d < a.hd) {
      a.dK[o + d] = dk[i];
      a.dV[o + d] = dv[i];
    }
  }
}

// ---- the two embedding tables: table row r owns the entries order[seg[r] : seg[r + 1]) (scldm_amd.vae.table_order), added in that
// order.  rows (entries, n): decoder slots first, then encoder tokens.  grid (table rows)
__global__ __launch_bounds__(256) void table_rows_sum_kernel(const float* __restrict__ rows, const int* __restrict__ order, const int* __restrict__ seg,
                                                             int n, float* __restrict__ out) {
  const int r = blockIdx.x, e_lo = seg[r], e_hi = seg[r + 1];
  for (int c = threadIdx.x; c < n; c += 256) {
    float s = 0.f;
    for (int e = e_lo; e < e_hi; ++e) s += rows[(size_t)order[e] * n + c];
    out[(size_t)r * n + c] = s;
  }
}
// the theta table: the decoder slots (entries below `slots`) of a row.  grid cdiv(table rows, 256)
__global__ __launch_bounds__(256) void theta_rows_sum_kernel(const float* __restrict__ trows, const int* __restrict__ order, const int* __restrict__ seg,
                                                             int table_rows, int slots, float* __restrict__ out) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= table_rows) return;
  float s = 0.f;
  for (int e = seg[r]; e < seg[r + 1]; ++e) {
    const int ent = order[e];
    if (ent < slots) s += trows[ent];
  }
  out[r] = s;
}

}  // namespace vaewt
}  // namespace scldm

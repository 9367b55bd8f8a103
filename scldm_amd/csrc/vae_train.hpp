// Backward of the TransformerVAE training step on gfx950 (judge-added row V1 / BASELINE configs[0]):
//   TransformerVAE.forward                     src/scldm/vae.py:29-56
//   VAE.loss -> -log_nb_positive(counts, mu, theta)   src/scldm/models.py:243-249, src/scldm/distributions.py:6-42
// The reference differentiates that chain with torch autograd; here every gradient is hand-derived and fp32.
//
// This file holds what the kernels of the backward share: the argument structs and the layouts of the per-workgroup partials
// (DP_*, TP_*, dc_*, ec_*, EP_*), and the small kernels around the heavy ones - weight transposes, the encoder's cell-independent
// query branch (enc_q_*), the NB head backward, the partial reductions and the fused NB log-likelihood.  The heavy kernels (per-gene
// decoder chain in its NB and Gaussian-head forms, the two 16-token cell sides, the encoder pooling) are in vae_train_wide.hpp.
// Sums over TOKENS (weight gradients, the per-cell dK / dV of the decoder's cross attention, the encoder's dQ) are written as ONE
// partial per workgroup, and a final pass adds the partials in index order (deterministic).  Only the two embedding-table
// gradients (gene_embedding, theta: scatter by gene id) use float atomics by default, like torch's own embedding backward.  The
// ORDERED mode (scldm_vae_train_backward_ordered) replaces them: the ROWS instantiations store each slot's contribution at the
// slot's entry index and table_rows_reduce_kernel adds the entries of a table row in the order of the caller's index.  It guarantees
// run-to-run bit equality of every gradient on one build and one GPU model - not equality across SCLDM_VAE_GENE_WGS / _POOL_WGS
// settings, which change other partial sums too.
// Forward activations are recomputed from the saved inputs (per-gene chains) or from one saved (16, 32) state per trunk layer.
#pragma once
#include "common.hpp"

namespace scldm {
namespace vtrain {

constexpr int kT = 16;      // latent tokens per cell
constexpr int kSL = 36;     // floats per row of a 32-wide staging tile (16-byte aligned rows, conflict-free 16-byte stores)
constexpr int kHP = 96;     // SwiGLU hidden padded to three 32-wide chunks (88 in the reference)

__device__ __forceinline__ f32x16 z16() {
  f32x16 z = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  return z;
}
// single-wave workgroups: the barrier is free, the fences order this wave's LDS traffic for the compiler
__device__ __forceinline__ void wsync() { __syncthreads(); }

// ---- thread-local vector helpers of the one-wave enc_q_* kernels (weights: wave-uniform pointers -> scalar loads) ---------------
template <int N>
__device__ __forceinline__ float dotw(const float* __restrict__ w, const float (&x)[N]) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < N; ++i) s = fmaf(w[i], x[i], s);
  return s;
}
// y[o] = W[o][:] . x   (W row-major [OUT][IN])
template <int OUT, int IN>
__device__ __forceinline__ void matvec(const float* __restrict__ W, const float (&x)[IN], float (&y)[OUT]) {
#pragma unroll
  for (int o = 0; o < OUT; ++o) y[o] = dotw<IN>(W + o * IN, x);
}
// dx[i] += sum_o W[o][i] dy[o]
template <int OUT, int IN>
__device__ __forceinline__ void matvec_t_acc(const float* __restrict__ W, const float (&dy)[OUT], float (&dx)[IN]) {
#pragma unroll
  for (int o = 0; o < OUT; ++o)
#pragma unroll
    for (int i = 0; i < IN; ++i) dx[i] = fmaf(W[o * IN + i], dy[o], dx[i]);
}
template <int N>
__device__ __forceinline__ void ln_fwd(const float (&x)[N], float (&xhat)[N], float& rstd, float eps) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < N; ++i) s += x[i];
  const float mean = s * (1.0f / N);
  float v = 0.f;
#pragma unroll
  for (int i = 0; i < N; ++i) { const float d = x[i] - mean; xhat[i] = d; v = fmaf(d, d, v); }
  rstd = 1.0f / sqrtf(v * (1.0f / N) + eps);
#pragma unroll
  for (int i = 0; i < N; ++i) xhat[i] *= rstd;
}
// dx += rstd * (dxhat - mean(dxhat) - xhat * mean(dxhat * xhat))
template <int N>
__device__ __forceinline__ void ln_bwd_acc(const float (&dxhat)[N], const float (&xhat)[N], float rstd, float (&dx)[N]) {
  float a = 0.f, b = 0.f;
#pragma unroll
  for (int i = 0; i < N; ++i) { a += dxhat[i]; b = fmaf(dxhat[i], xhat[i], b); }
  a *= (1.0f / N);
  b *= (1.0f / N);
#pragma unroll
  for (int i = 0; i < N; ++i) dx[i] = fmaf(rstd, dxhat[i] - a - xhat[i] * b, dx[i]);
}
__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + __expf(-x)); }

// ---- staging + lane-axis contractions ------------------------------------------------------------------------------------------
// row `lane` of a [64][kSL] tile <- v (zeros for an invalid token)
__device__ __forceinline__ void stage32(float* __restrict__ buf, int lane, const float (&v)[32], bool valid) {
  f32x4* row = reinterpret_cast<f32x4*>(buf + lane * kSL);
#pragma unroll
  for (int q = 0; q < 8; ++q) row[q] = valid ? f32x4{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]} : f32x4{0.f, 0.f, 0.f, 0.f};
}
// acc[r] (lane l) += sum_tokens A[token][acc_row(r, l >> 5)] * B[token][l & 31]
__device__ __forceinline__ void wgrad32(f32x16& acc, const float* __restrict__ A, const float* __restrict__ B, int lane) {
  const int c = lane & 31, kh = lane >> 5;
#pragma unroll 8
  for (int k = 0; k < 32; ++k) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(A[(2 * k + kh) * kSL + c], B[(2 * k + kh) * kSL + c], acc, 0, 0, 0);
}
// lanes < 32: column sums of A; lanes >= 32: column sums of B  (feature = lane & 31)
__device__ __forceinline__ float colsum2(const float* __restrict__ A, const float* __restrict__ B, int lane) {
  const float* src = (lane < 32 ? A : B) + (lane & 31);
  float s = 0.f;
#pragma unroll 8
  for (int t = 0; t < 64; ++t) s += src[t * kSL];
  return s;
}
// partial tile store: dst[(row0 + acc_row(r, hh)) * ld + col0 + c32]
__device__ __forceinline__ void flush_tile(float* __restrict__ dst, const f32x16& acc, int lane, int row0, int col0, int ld) {
  const int c = lane & 31, hh = lane >> 5;
#pragma unroll
  for (int r = 0; r < 16; ++r) dst[(size_t)(row0 + acc_row(r, hh)) * ld + col0 + c] = acc[r];
}

// SwiGLU MLP weights: m = Wc (silu(W1 h2) * (W2 h2)); wct = Wc transposed ([H][32])
struct MlpW { const float* w1; const float* w2; const float* wct; int H; };

// =================================================================================================================================
// Small preparation kernels
// =================================================================================================================================
// WT[c][r] = W[r][c]
__global__ void transpose_kernel(const float* __restrict__ W, int R, int C, float* __restrict__ WT) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < R * C) WT[(i % C) * R + (i / C)] = W[i];
}
// the same for up to 34 matrices of one shape in ONE launch (blockIdx.y = matrix; WT of matrix m at dst + m * R * C... stride given)
struct TransposeJobs { const float* src[34]; };
__global__ void transpose_many_kernel(const TransposeJobs j, int R, int C, float* __restrict__ dst, long stride) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < R * C) dst[(size_t)blockIdx.y * stride + (i % C) * R + (i / C)] = j.src[blockIdx.y][i];
}
// Encoder queries (cell-independent): qn = LN_1q(inducing points), Q = c_attn_q qn  (layers.py:312-313,326; 248-253)
__global__ __launch_bounds__(64) void enc_q_fwd_kernel(const float* __restrict__ ind, const float* __restrict__ lnw, const float* __restrict__ lnb,
                                                       const float* __restrict__ wq, float eps, float* __restrict__ Q) {
  const int t = threadIdx.x;
  if (t >= kT) return;
  float x[32], xh[32], q[32], rstd;
#pragma unroll
  for (int i = 0; i < 32; ++i) x[i] = ind[t * 32 + i];
  ln_fwd<32>(x, xh, rstd, eps);
#pragma unroll
  for (int i = 0; i < 32; ++i) xh[i] = fmaf(xh[i], lnw[i], lnb[i]);
  matvec<32, 32>(wq, xh, q);
#pragma unroll
  for (int i = 0; i < 32; ++i) Q[t * 32 + i] = q[i];
}
// ... and its backward once dQ (sum over all cells and tokens) is known: d c_attn_q, d ln_1q, d inducing points (+= into gind)
__global__ __launch_bounds__(64) void enc_q_bwd_kernel(const float* __restrict__ ind, const float* __restrict__ lnw, const float* __restrict__ lnb,
                                                       const float* __restrict__ wq, float eps, const float* __restrict__ dQ,
                                                       float* __restrict__ g_wq, float* __restrict__ g_lnw, float* __restrict__ g_lnb,
                                                       float* __restrict__ g_ind) {
  __shared__ float A[64 * kSL], Bq[64 * kSL], Cn[64 * kSL];
  const int t = threadIdx.x;
  const bool valid = t < kT;
  const int tt = valid ? t : 0;
  float x[32], xh[32], qn[32], dq[32], dqn[32], rstd;
#pragma unroll
  for (int i = 0; i < 32; ++i) { x[i] = ind[tt * 32 + i]; dq[i] = dQ[tt * 32 + i]; dqn[i] = 0.f; }
  ln_fwd<32>(x, xh, rstd, eps);
#pragma unroll
  for (int i = 0; i < 32; ++i) qn[i] = fmaf(xh[i], lnw[i], lnb[i]);
  matvec_t_acc<32, 32>(wq, dq, dqn);
  float dxh[32], prod[32], dx[32];
#pragma unroll
  for (int i = 0; i < 32; ++i) { dxh[i] = dqn[i] * lnw[i]; prod[i] = dqn[i] * xh[i]; dx[i] = 0.f; }
  ln_bwd_acc<32>(dxh, xh, rstd, dx);
  if (valid)
#pragma unroll
    for (int i = 0; i < 32; ++i) g_ind[t * 32 + i] += dx[i];
  stage32(A, t, dq, valid);
  stage32(Bq, t, qn, valid);
  wsync();
  f32x16 acc = z16();
  wgrad32(acc, A, Bq, t);
  flush_tile(g_wq, acc, t, 0, 0, 32);
  wsync();
  stage32(A, t, prod, valid);
  stage32(Cn, t, dqn, valid);
  wsync();
  const float s = colsum2(A, Cn, t);
  if (t < 32) g_lnw[t] = s; else g_lnb[t - 32] = s;
}

// =================================================================================================================================
// NB head backward (stochastic_layers.py:102-116): mu = softmax_G(logit / T) lib, theta = exp(Theta[gene])
//   dlogit_g = mu_g (dmu_g - sum_j dmu_j mu_j / lib) / T ;  dTheta[gene] += dtheta theta (atomic scatter)
// One workgroup (256 threads) per cell.  dlogit overwrites `dl`; bsum[cell] = sum_g dlogit_g (the head bias gradient's partial).
// =================================================================================================================================
// SCALE (fp16 training backward): also records the cell's power of two 2^e with max |2^e dl| in [2^kDlScaleLog2, 2^(kDlScaleLog2 + 1))
// (1 for an all-zero row) in dl_scale[cell]; the fp16-operand per-gene kernel multiplies dl by it before rounding, and its fp32 outputs
// by 2^-e.  The gradient operands of the chain are dl times weight-sized factors (d a = dl (Wc^T w_head)_u b sigma'(a), ...: 1e-3 dl
// at the reference's initialisation), and most genes' dl lie orders of magnitude below the cell's maximum: at [8, 16) they fell into
// fp16's subnormal range (gradient error 1.7 x the TF32-operand oracle's on vae_train_small); [1024, 2048) keeps them normal and
// leaves 32 x headroom for d y = dl w_head + ... (|w_head| < 1).  An overflow still sets the found-inf flag.
constexpr int kDlScaleLog2 = 10;
// ROWS (ordered table gradients): `g_theta` is the (B, G) row buffer instead of the table - dtheta theta goes to g_theta[cell * G + slot]
// (0 where dtheta is NULL; every slot is written, the buffer needs no memset), `genes` is not read, and table_rows_reduce_kernel adds
// the slots of a table row in a fixed order.
template <bool SCALE, bool ROWS = false>
__global__ __launch_bounds__(256) void head_bwd_kernel(const float* __restrict__ mu, const float* __restrict__ theta, const float* __restrict__ dmu,
                                                       const float* __restrict__ dtheta, const float* __restrict__ lib,
                                                       const int64_t* __restrict__ genes, int G, float inv_temp, float* __restrict__ dl,
                                                       float* __restrict__ g_theta, float* __restrict__ bsum, float* __restrict__ dl_scale) {
  __shared__ float red[4];
  __shared__ float amax[4];
  const int cell = blockIdx.x, tid = threadIdx.x;
  const size_t base = (size_t)cell * G;
  float s = 0.f;
  for (int g = tid; g < G; g += 256) s = fmaf(dmu ? dmu[base + g] : 0.f, mu[base + g], s);
  s = wave_sum(s);
  if ((tid & 63) == 0) red[tid >> 6] = s;
  __syncthreads();
  const float sc = (red[0] + red[1] + red[2] + red[3]) / lib[cell];
  __syncthreads();
  float b = 0.f, m = 0.f;
  for (int g = tid; g < G; g += 256) {
    const float d = dmu ? mu[base + g] * (dmu[base + g] - sc) * inv_temp : 0.f;
    dl[base + g] = d;
    b += d;
    if constexpr (SCALE) m = fmaxf(m, fabsf(d));
    if constexpr (ROWS) {
      g_theta[base + g] = dtheta ? dtheta[base + g] * theta[base + g] : 0.f;
    } else if (dtheta) {
      const float dt = dtheta[base + g] * theta[base + g];
      if (dt != 0.f) atomicAdd(g_theta + genes[base + g], dt);
    }
  }
  b = wave_sum(b);
  if ((tid & 63) == 0) red[tid >> 6] = b;
  if constexpr (SCALE) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((tid & 63) == 0) amax[tid >> 6] = m;
  }
  __syncthreads();
  if (tid == 0) bsum[cell] = red[0] + red[1] + red[2] + red[3];
  if constexpr (SCALE) {
    if (tid == 0) {
      const float mx = fmaxf(fmaxf(amax[0], amax[1]), fmaxf(amax[2], amax[3]));
      int e = 0;
      if (mx > 0.f && mx <= 3.4e38f) {      // (a non-finite row keeps 2^0: the gene kernel's outputs then raise the flag)
        int ex;
        (void)frexpf(mx, &ex);             // mx = f 2^ex, f in [0.5, 1)  ->  mx 2^(kDlScaleLog2 + 1 - ex) in [2^kDlScaleLog2, 2^(kDlScaleLog2 + 1))
        e = min(max(kDlScaleLog2 + 1 - ex, -126), 126);
      }
      dl_scale[cell] = ldexpf(1.0f, e);
    }
  }
}

// Unshared-theta NB head (theta = exp(l1), one per cell and gene, no table): dl = d loss / d l0 as above, dl2 = d loss / d l1 =
// dtheta theta (zeros where dtheta is NULL); the two head bias gradients come out of the per-gene kernel's partial.  SCALE: the cell's
// power of two is taken from max(|dl|, |dl2|) over the cell and scales both streams (same window as head_bwd_kernel<true>).
template <bool SCALE>
__global__ __launch_bounds__(256) void head_bwd_nb2_kernel(const float* __restrict__ mu, const float* __restrict__ theta, const float* __restrict__ dmu,
                                                           const float* __restrict__ dtheta, const float* __restrict__ lib, int G, float inv_temp,
                                                           float* __restrict__ dl, float* __restrict__ dl2, float* __restrict__ dl_scale) {
  __shared__ float red[4];
  __shared__ float amax[4];
  const int cell = blockIdx.x, tid = threadIdx.x;
  const size_t base = (size_t)cell * G;
  float s = 0.f;
  for (int g = tid; g < G; g += 256) s = fmaf(dmu ? dmu[base + g] : 0.f, mu[base + g], s);
  s = wave_sum(s);
  if ((tid & 63) == 0) red[tid >> 6] = s;
  __syncthreads();
  const float sc = (red[0] + red[1] + red[2] + red[3]) / lib[cell];
  float m = 0.f;
  for (int g = tid; g < G; g += 256) {
    const float d = dmu ? mu[base + g] * (dmu[base + g] - sc) * inv_temp : 0.f;
    const float d2 = dtheta ? dtheta[base + g] * theta[base + g] : 0.f;
    dl[base + g] = d;
    dl2[base + g] = d2;
    if constexpr (SCALE) m = fmaxf(m, fmaxf(fabsf(d), fabsf(d2)));
  }
  if constexpr (SCALE) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((tid & 63) == 0) amax[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
      const float mx = fmaxf(fmaxf(amax[0], amax[1]), fmaxf(amax[2], amax[3]));
      int e = 0;
      if (mx > 0.f && mx <= 3.4e38f) {      // (a non-finite row keeps 2^0: the gene kernel's outputs then raise the flag)
        int ex;
        (void)frexpf(mx, &ex);
        e = min(max(kDlScaleLog2 + 1 - ex, -126), 126);
      }
      dl_scale[cell] = ldexpf(1.0f, e);
    }
  }
}

// =================================================================================================================================
// Decoder MCAB, per-gene chain backward (layers.py:305-330 with q = gene embeddings, nnets.py:206-208; NB logit head)
//   q0 = E[gene]; qn = LN_1q(q0); qq = Wq qn; ao = softmax(qq K^T / sqrt 8) V (4 heads x 8, 16 latent keys of the cell);
//   y = q0 + Wp ao; h2 = LN_2(y); yo = y + MLP(h2); logit = w_head . yo + b
// grid = (chunks, B), `tiles` 64-gene tiles per workgroup (wide::dec_gene_bwd_mfma2_kernel).
// Partial per workgroup (floats): see DP_* below; dK|dV of the cell: dkv_part[(cell * chunks + chunk)][16][64].
// =================================================================================================================================
enum : int { DP_WQ = 0, DP_WP = 1024, DP_W1 = 2048, DP_W2 = DP_W1 + kHP * 32, DP_WC = DP_W2 + kHP * 32, DP_LN1QW = DP_WC + 32 * kHP,
             DP_LN1QB = DP_LN1QW + 32, DP_LN2W = DP_LN1QB + 32, DP_LN2B = DP_LN2W + 32, DP_HEADW = DP_LN2B + 32, DP_SIZE = DP_HEADW + 32 };
struct DecBwdArgs {
  const int64_t* genes;    // (B, G)
  const float* emb;        // (n_genes + 1, 32)
  const float* dl;         // (B, G) dlogit
  const float* kv;         // (B, 16, 64): K | V of the cell's latent tokens
  const float *ln1q_w, *ln1q_b, *wq, *wp, *ln2_w, *ln2_b, *head_w;
  MlpW mlp;
  float* g_emb;            // (n_genes + 1, 32), atomically accumulated; ROWS instantiations: the (B * G, 32) row buffer of the ordered mode
  float* part;             // (B * chunks, DP_SIZE)
  float* dkv_part;         // (B * chunks, 16, 64)
  int G, tiles;
  float eps;
  // fp16-operand per-gene kernel only (dec_gene_bwd_mfma2_kernel<true>): per-cell power-of-two scale of dl (head_bwd_kernel<true>) and
  // the caller's found-inf flag (may be null)
  const float* dl_scale;
  float* found_inf;
};
// Gaussian head (wide::dec_gene_bwd_gauss_kernel): `nb.dl` is d loss / d mu as the caller gives it, `nb.head_w` the (1, 32) params
// weight; the partial is the NB layout followed by the head LayerNorm's vectors and the head bias (a layout of its own: DP_SIZE
// and the NB kernels' argument block stay what they were)
enum : int { GP_HLNW = DP_SIZE, GP_HLNB = GP_HLNW + 32, GP_HEADB = GP_HLNB + 32, GP_SIZE = GP_HEADB + 32 };
struct DecBwdGaussArgs {
  DecBwdArgs nb;
  const float *hln_w, *hln_b;   // decoder_head.ln.weight / .bias (32)
};
// Unshared-theta NB head (wide::dec_gene_bwd_nb2_kernel): `nb.head_w` is the (2, 32) params weight (row 1 at + 32), `nb.dl` is
// d loss / d l0 and `dl2` d loss / d l1 = dtheta theta (head_bwd_nb2_kernel); the partial is the NB layout followed by head row 1 and
// the two bias sums (a layout of its own, as GP_*)
enum : int { NP_HEADW1 = DP_SIZE, NP_HEADB = NP_HEADW1 + 32, NP_SIZE = NP_HEADB + 32 };
struct DecBwdNb2Args {
  DecBwdArgs nb;
  const float* dl2;             // (B, G)
};

// =================================================================================================================================
// The 16-token side of a cell: trunk Blocks (layers.py:222-226: x += c_proj(attn(LN_1 x)); x += MLP(LN_2 x); 8 heads x 4) and the
// per-cell ends of the two MCABs: arguments and partial layouts of the wide:: cell kernels.
// =================================================================================================================================
struct BlockW { const float *ln1_w, *ln1_b, *wqkv, *wp, *ln2_w, *ln2_b; MlpW mlp; };
struct BlockWArr { BlockW b[16]; };   // up to 16 layers per side
constexpr float kTScale = 0.5f;   // 1 / sqrt(4)

// Partial layout of one trunk layer (floats)
enum : int { TP_WQKV = 0, TP_WP = 3072, TP_W1 = 4096, TP_W2 = TP_W1 + kHP * 32, TP_WC = TP_W2 + kHP * 32, TP_LN1W = TP_WC + 32 * kHP,
             TP_LN1B = TP_LN1W + 32, TP_LN2W = TP_LN1B + 32, TP_LN2B = TP_LN2W + 32, TP_SIZE = TP_LN2B + 32 };

// ---- decoder cell side ----------------------------------------------------------------------------------------------------------
// forward with saved layer inputs: z (16 x n_lat) -> LN (no affine) -> Linear -> n_layer Blocks -> h_lat; kv = c_attn(LN_1 h_lat)
// xsave: (B, n_layer + 1, 16, 32)
struct DecCellTrainArgs {
  const float* z;          // (B, 16, n_lat)
  const float* w_in;       // decoder_latent_input.1.weight (32, n_lat)
  BlockWArr blocks;
  const float *cln1_w, *cln1_b, *wkv;   // decoder_cross_attention.ln_1, attn.c_attn (64, 32)
  float* xsave;
  float* kv;               // (B, 16, 64)
  // backward only
  const float* dkv_part;   // (B * chunks, 16, 64)
  int chunks;
  float* dz;               // (B, 16, n_lat): gradient w.r.t. z from the decoder
  float* part;             // (workgroups, DC_SIZE)
  int B, n_lat, n_layer;
  float eps;
};
// partial of the decoder cell kernel: n_layer trunk layers, then the cross-attention's K/V side and the latent input Linear
__host__ __device__ constexpr int dc_off_wkv(int n_layer) { return n_layer * TP_SIZE; }
__host__ __device__ constexpr int dc_off_cln1w(int n_layer) { return dc_off_wkv(n_layer) + 64 * 32; }
__host__ __device__ constexpr int dc_off_cln1b(int n_layer) { return dc_off_cln1w(n_layer) + 32; }
__host__ __device__ constexpr int dc_off_win(int n_layer) { return dc_off_cln1b(n_layer) + 32; }      // stored as [32][32] (cols >= n_lat zero)
__host__ __device__ constexpr int dc_size(int n_layer) { return dc_off_win(n_layer) + 1024; }

// ---- encoder cell side ----------------------------------------------------------------------------------------------------------
// y = P + Wp ao; y2 = y + MLP(LN_2 y); x0 = y2 + pos; n_layer Blocks -> hL; zl = W_lat hL; z = LN(zl)   (layers.py:326-330, nnets.py:139-144)
struct EncCellTrainArgs {
  const float* pooled;     // (B, 16, 32): attention output of the pooling (heads concatenated)
  const float* ind;        // inducing points (16, 32)
  const float *wp, *cln2_w, *cln2_b;
  MlpW cmlp;
  const float* pos;        // (16, 32) or nullptr
  BlockWArr blocks;
  const float* w_lat;      // encoder_latent_input.0.weight (n_lat, 32)
  float* xsave;            // (B, n_layer + 1, 16, 32)
  float* ysave;            // (B, 16, 32): y (input of LN_2)
  // backward
  const float* dz_a;       // (B, 16, n_lat) or nullptr: gradient w.r.t. z from the decoder
  const float* dz_b;       // (B, 16, n_lat) or nullptr: gradient w.r.t. the returned z
  float* dao;              // (B, 16, 32): gradient w.r.t. the pooled attention output
  float* dgq;              // (B, 4, 16): sum_d dao[i, h, d] * ao[i, h, d]
  float* part;
  int B, n_lat, n_layer;
  float eps;
};
__host__ __device__ constexpr int ec_off_wp(int n_layer) { return n_layer * TP_SIZE; }
__host__ __device__ constexpr int ec_off_w1(int n_layer) { return ec_off_wp(n_layer) + 1024; }
__host__ __device__ constexpr int ec_off_w2(int n_layer) { return ec_off_w1(n_layer) + kHP * 32; }
__host__ __device__ constexpr int ec_off_wc(int n_layer) { return ec_off_w2(n_layer) + kHP * 32; }
__host__ __device__ constexpr int ec_off_ln2w(int n_layer) { return ec_off_wc(n_layer) + 32 * kHP; }
__host__ __device__ constexpr int ec_off_ln2b(int n_layer) { return ec_off_ln2w(n_layer) + 32; }
__host__ __device__ constexpr int ec_off_wlat(int n_layer) { return ec_off_ln2b(n_layer) + 32; }     // [32][32], rows >= n_lat zero
__host__ __device__ constexpr int ec_off_ind(int n_layer) { return ec_off_wlat(n_layer) + 1024; }    // [16][32]
__host__ __device__ constexpr int ec_size(int n_layer) { return ec_off_ind(n_layer) + 512; }

// =================================================================================================================================
// Encoder MCAB pooling backward, key side (layers.py:111-118, 248-264, 325-326): wide::enc_pool_bwd_kernel
//   x = E[gene] log1p(count); xn = LN_1(x); k | v = c_attn xn; p[i][h] = exp2(log2e / sqrt 8 * Q[i][h] . k[h] - lse2[i][h])
// grid = (chunks, B).  Partial per workgroup: EP_* ; gene-embedding gradient by atomics.
// =================================================================================================================================
enum : int { EP_WKV = 0, EP_LN1W = 2048, EP_LN1B = 2080, EP_DQ = 2112, EP_SIZE = EP_DQ + 64 * 32 };
struct EncPoolBwdArgs {
  const float* counts;     // (B, S)
  const int64_t* genes;    // (B, S)
  const float* emb;
  const float *ln1_w, *ln1_b, *wkv;
  const float* Q;          // (16, 32) = c_attn_q(LN_1q(inducing))
  const float* lse2;       // (B, 4, 16): log2-domain log-sum-exp of the scaled scores
  const float* dao;        // (B, 16, 32)
  const float* dgq;        // (B, 4, 16)
  float* g_emb;            // enc_pool_bwd_rows_kernel: the (B * S, 32) row buffer of the ordered mode
  float* part;             // (B * chunks, EP_SIZE)
  int S, tiles;
  float eps;
};

// =================================================================================================================================
// Partial reduction: dst[i] (+)= sum_p part[p * stride + off + i]   (index order: deterministic)
// =================================================================================================================================
struct RedJob { float* dst; int off, n, accumulate; int rows, ld_src, ld_dst; };   // rows > 1: a [rows][ld_src] block copied to [rows][ld_dst] (n = cols)
constexpr int kMaxRedJobs = 96;   // (3 KB of kernel arguments; a cell side of 8 layers is 76-84 jobs: one launch)
struct RedArgs { const float* part; int n_part; long stride; int n_jobs; RedJob job[kMaxRedJobs]; };
// sum over the partials of one element, eight independent running sums (memory-level parallelism; fixed order: deterministic)
__device__ __forceinline__ float sum_partials(const float* __restrict__ src, int n_part, long stride) {
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int p = 0;
  for (; p + 8 <= n_part; p += 8)
#pragma unroll
    for (int u = 0; u < 8; ++u) s[u] += src[(size_t)(p + u) * stride];
  for (; p < n_part; ++p) s[p & 7] += src[(size_t)p * stride];
  return ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
}
__global__ __launch_bounds__(256) void reduce_jobs_kernel(const RedArgs a) {
  const RedJob& j = a.job[blockIdx.y];
  const int total = j.rows * j.n;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int r = i / j.n, c = i % j.n;
    const float s = sum_partials(a.part + j.off + (size_t)r * j.ld_src + c, a.n_part, a.stride);
    float* d = j.dst + (size_t)r * j.ld_dst + c;
    *d = j.accumulate ? *d + s : s;
  }
}
// dQ (16, 32) from the pooling partial's [h*16 + i][32] block-diagonal rows: dQ[i][d] = row(head(d), i)[d]
__global__ __launch_bounds__(64) void fold_dq_kernel(const float* __restrict__ part, int n_part, long stride, float* __restrict__ dQ) {
  const int idx = blockIdx.x * 64 + threadIdx.x;
  if (idx >= 16 * 32) return;
  const int i = idx >> 5, d = idx & 31, h = d >> 3;
  dQ[idx] = sum_partials(part + EP_DQ + (h * 16 + i) * 32 + d, n_part, stride);
}

// =================================================================================================================================
// Ordered table gradients (scldm_vae_train_backward_ordered): g[r][f] = sum over order[seg[r] .. seg[r + 1]) of rows[entry][f], in the
// order the caller's index lists the entries - no float atomics, so the two embedding tables are bit-reproducible run to run like every
// other gradient.  256 threads = 8 interleaved running sums (sum u takes the entries u, u + 8, ... of the segment, four loads in
// flight, added in index order) x 32 columns, combined in the fixed tree of sum_partials.  A table row with an empty segment is
// written as exact zeros: the tables need no memset.
//   F = 32 (table_rows_reduce_kernel, gene_embedding): one workgroup per table row, column = feature; rows = the decoder slots' and
//           the encoder tokens' 32-float contributions (entry = cell * G + slot, or B * G + cell * S + token).
//   F = 1  (table_scalars_reduce_kernel, theta): one workgroup per 32 table rows, column = table row; rows = one float per decoder
//           slot, and only the entries below `n_valid` = B * G (the decoder slots of the same index) are taken.
// Entries outside [0, n_valid) and offsets outside [0, n_order] are skipped / clamped, never dereferenced.
// (Two plain kernels over one body, not two instantiations of a template kernel: with the template, head_bwd_kernel<false> of the default
// mode compiled to one instruction more - tools/kernel_isa_digest.py.)
// =================================================================================================================================
template <int F>
__device__ __forceinline__ void table_rows_reduce(float (&part)[8][33], const float* __restrict__ rows, const int32_t* __restrict__ order,
                                                  const int32_t* __restrict__ seg, int n_table, int n_order, int n_valid,
                                                  float* __restrict__ dst) {
  const int u = threadIdx.x >> 5, c = threadIdx.x & 31;
  const int r = F == 32 ? (int)blockIdx.x : (int)blockIdx.x * 32 + c;
  const int f = F == 32 ? c : 0;
  float s = 0.f;
  if (r < n_table) {
    const int beg = min(max(seg[r], 0), n_order), end = min(max(seg[r + 1], beg), n_order);
    auto val = [&](int i) {
      const int e = i < end ? order[i] : -1;
      return (unsigned)e < (unsigned)n_valid ? rows[(size_t)e * F + f] : 0.f;
    };
    for (int i = beg + u; i < end; i += 32) {
      const float v0 = val(i), v1 = val(i + 8), v2 = val(i + 16), v3 = val(i + 24);
      s += v0;
      s += v1;
      s += v2;
      s += v3;
    }
  }
  part[u][c] = s;
  __syncthreads();
  if (u == 0 && r < n_table)
    dst[(size_t)r * F + f] = ((part[0][c] + part[1][c]) + (part[2][c] + part[3][c])) + ((part[4][c] + part[5][c]) + (part[6][c] + part[7][c]));
}
__global__ __launch_bounds__(256) void table_rows_reduce_kernel(const float* __restrict__ rows, const int32_t* __restrict__ order,
                                                                const int32_t* __restrict__ seg, int n_table, int n_order, int n_valid,
                                                                float* __restrict__ dst) {
  __shared__ float part[8][33];
  table_rows_reduce<32>(part, rows, order, seg, n_table, n_order, n_valid, dst);
}
__global__ __launch_bounds__(256) void table_scalars_reduce_kernel(const float* __restrict__ rows, const int32_t* __restrict__ order,
                                                                   const int32_t* __restrict__ seg, int n_table, int n_order, int n_valid,
                                                                   float* __restrict__ dst) {
  __shared__ float part[8][33];
  table_rows_reduce<1>(part, rows, order, seg, n_table, n_order, n_valid, dst);
}

// =================================================================================================================================
// log_nb_positive with its gradient (src/scldm/distributions.py:6-42), elementwise
// =================================================================================================================================
__device__ __forceinline__ float digammaf_dev(float x) {
  // psi(x) for x > 0: recurrence up to x >= 6, then the asymptotic series
  float r = 0.f;
  while (x < 6.0f) { r -= 1.0f / x; x += 1.0f; }
  const float f = 1.0f / (x * x);
  return r + logf(x) - 0.5f / x - f * (1.0f / 12.0f - f * (1.0f / 120.0f - f * (1.0f / 252.0f - f * (1.0f / 240.0f - f * (1.0f / 132.0f)))));
}
__global__ __launch_bounds__(256) void nb_loglik_kernel(const float* __restrict__ x, const float* __restrict__ mu, const float* __restrict__ theta,
                                                        float eps, float* __restrict__ out, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const float xv = x[i], m = mu[i], th = theta[i];
    const float ltm = logf(th + m + eps);
    out[i] = th * (logf(th + eps) - ltm) + xv * (logf(m + eps) - ltm) + lgammaf(xv + th) - lgammaf(th) - lgammaf(xv + 1.0f);
  }
}
__global__ __launch_bounds__(256) void nb_loglik_bwd_kernel(const float* __restrict__ x, const float* __restrict__ mu, const float* __restrict__ theta,
                                                            const float* __restrict__ gout, float eps, float* __restrict__ dmu,
                                                            float* __restrict__ dtheta, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const float xv = x[i], m = mu[i], th = theta[i], g = gout[i];
    const float inv = 1.0f / (th + m + eps);
    if (dmu) dmu[i] = g * (xv / (m + eps) - (th + xv) * inv);
    if (dtheta)
      dtheta[i] = g * (logf(th + eps) - logf(th + m + eps) + th / (th + eps) - (th + xv) * inv + digammaf_dev(xv + th) - digammaf_dev(th));
  }
}

}  // namespace vtrain
}  // namespace scldm

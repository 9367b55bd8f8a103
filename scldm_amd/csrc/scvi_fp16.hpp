// The tile kernel of the scVI-style baseline VAE on fp16 operands (the reference's TF32 class: 10 explicit mantissa bits, fp32
// accumulate), inference only: scvi16::gemm_kernel is scvi::gemm_kernel (scvi.hpp) with the operands rounded to fp16 while they are
// written to LDS and one v_mfma_f32_32x32x16_f16 per 16 k-values in place of 8 x v_mfma_f32_32x32x2_f32.  It lives in its own
// header and translation unit (scvi_fp16_api.hip) so that the device module of scvi.hpp compiles exactly as before; pack_kernel,
// merge_kernel and softmax_finalize_kernel are reached through the host launchers of scvi_handle.hpp.
//
// Y[M, N] = act(X[M, K]) W[N, K]^T, both operands fp32 in torch's layout (K contiguous), read where the parameters live:
//   * a workgroup of four waves owns a 64 x 64 output tile, wave (wm, wn) its 32 x 32 quadrant; K is walked in stages of 64 through
//     LDS, the next stage's global loads are in flight during the MFMAs;
//   * loads are scalar dwords masked to zero outside M, N and K (a row of 17 002 floats is only 8-byte aligned; log1p(0) = 0 keeps the
//     masked first-layer operand zero); a thread loads the two consecutive k-values 2 (tid & 31), + 1 of eight rows per operand and
//     stores them as one packed dword;
//   * conversion: log1pf in fp32 first (first layer), then a clamp to +-65 504 (the saturation of the MCAB fp16 weight policy) and a
//     plain round-to-nearest-even cast.  NaN operands are outside the contract.  There is no packed fp16 copy of the weights;
//   * LDS holds halfs, rows padded to kLd = 72 halfs = 144 bytes = 36 dwords: a lane's fragment (8 consecutive k-values of its row,
//     k = 16 u + 8 (lane >> 5) + i) is one 16-byte aligned ds_read_b128, and the 16 lanes one LDS cycle serves (rows l, dword
//     36 l mod 64 = 0, 36, 8, 44, ... : sixteen different multiples of 4) cover the 64 banks once; the packed stores of a half-wave
//     are 32 consecutive dwords;
//   * every output element accumulates its k-values in ascending stage order in ONE accumulator, and the k range of a split is a
//     function of K alone (kSplitK), so an element's bits depend neither on the run nor on the other rows of the batch.
// The epilogues (MODE) are those of scvi.hpp, in fp32, word for word.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.hpp"

namespace scldm {
namespace scvi16 {

constexpr int kBM = 64, kBN = 64, kBK = 64, kLd = kBK + 8;   // kLd in halfs
constexpr int kSplitK = 1024;              // k-values per split of a product (a multiple of kBK; = scvi::kScviSplitK)
constexpr int kOutLd = kBN + 1;            // LDS row stride (floats) of a staged output tile
constexpr int kEpiBytes = (kBM * kOutLd + 2 * kBM * 4) * 4;   // the epilogues' staged output tile + softmax partials
constexpr int kStageBytes = 2 * kBM * kLd * 2;                // the two operand stages, which the epilogue reuses
constexpr int kSmemBytes = kEpiBytes > kStageBytes ? kEpiBytes : kStageBytes;
static_assert(kSplitK % kBK == 0 && (kLd * 2) % 16 == 0, "whole stages per split, 16-byte aligned fragment rows");

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

typedef __attribute__((ext_vector_type(2))) _Float16 f16x2;
// fp32 -> fp16 operand: saturate at the largest finite half, then round to nearest even (v_cvt_f16_f32 under the default mode)
__device__ __forceinline__ _Float16 to_operand(float x) { return (_Float16)__builtin_amdgcn_fmed3f(x, -65504.f, 65504.f); }

template <int MODE>
struct Traits {
  static constexpr bool kDual = MODE == MODE_POST || MODE == MODE_LIK2;   // a tile's columns [32, 64) come from W1
  static constexpr int kCols = kDual ? 32 : 64;                            // columns of the N0 axis one tile covers
};

template <int MODE, bool LOG1P>
__global__ __launch_bounds__(256) void gemm_kernel(const GemmArgs a) {
  using T = Traits<MODE>;
  __shared__ __attribute__((aligned(16))) unsigned char smem_raw[kSmemBytes];
  float* smem = reinterpret_cast<float*>(smem_raw);
  _Float16* As = reinterpret_cast<_Float16*>(smem_raw);
  _Float16* Bs = As + kBM * kLd;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.y * kBM, n0 = blockIdx.x * T::kCols;
  const int k_lo = blockIdx.z * a.k_per_split;
  const int k_hi = min(a.K, k_lo + a.k_per_split);
  // loader: thread -> k offsets lk, lk + 1 of rows (tid >> 5) + 8 j
  const int lk = (tid & 31) * 2, lr = tid >> 5;
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
  float xa[8][2], wb[8][2];
  auto fetch = [&](int k0) {
    const int k = k0 + lk;
    const bool ok0 = k < k_hi, ok1 = k + 1 < k_hi;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      xa[j][0] = (ok0 && xrow[j]) ? xrow[j][k] : 0.f;
      xa[j][1] = (ok1 && xrow[j]) ? xrow[j][k + 1] : 0.f;
      wb[j][0] = (ok0 && wrow[j]) ? wrow[j][k] : 0.f;
      wb[j][1] = (ok1 && wrow[j]) ? wrow[j][k + 1] : 0.f;
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
      const float x0 = LOG1P ? log1pf(xa[j][0]) : xa[j][0], x1 = LOG1P ? log1pf(xa[j][1]) : xa[j][1];
      *reinterpret_cast<f16x2*>(As + (lr + 8 * j) * kLd + lk) = f16x2{to_operand(x0), to_operand(x1)};
      *reinterpret_cast<f16x2*>(Bs + (lr + 8 * j) * kLd + lk) = f16x2{to_operand(wb[j][0]), to_operand(wb[j][1])};
    }
    __syncthreads();
    if (k0 + kBK < k_hi) fetch(k0 + kBK);
#pragma unroll
    for (int u = 0; u < kBK / 16; ++u) {
      const f16x8 af = *reinterpret_cast<const f16x8*>(As + (wm * 32 + l31) * kLd + u * 16 + 8 * hh);
      const f16x8 bf = *reinterpret_cast<const f16x8*>(Bs + (wn * 32 + l31) * kLd + u * 16 + 8 * hh);
      acc = OpFP16::mma(af, bf, acc);
    }
    __syncthreads();
  }
  // ---- epilogues (scvi.hpp's): lane holds column wn * 32 + l31 of the tile, register r row wm * 32 + acc_row(r, hh)
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

}  // namespace scvi16
}  // namespace scldm

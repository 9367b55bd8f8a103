// The tile product of the scVI-style baseline VAE (ScviVAE), defined once for its inference kernels in both operand precisions
// (scvi.hpp: gemm_kernel) and for the products of its backward (scvi_train.hpp: prod_kernel): the shared types, the operand policy,
// the product core and the epilogues.
//
// A workgroup of four waves owns a 64 x 64 output tile, wave (wm, wn) its 32 x 32 quadrant.  K is walked in stages of P::kBK through
// LDS, the next stage's global loads are in flight during the MFMAs.  M, N and K are arbitrary: loads are scalar dwords (a row of
// 17 002 floats is only 8-byte aligned) masked to zero outside the matrix - log1p(0) = 0, so a masked log1p operand is zero as well.
// Every output element accumulates its k-values in ascending stage order in ONE accumulator, and the k range of a split is a
// function of K alone (kScviSplit), so an element's bits depend neither on the run nor on the other rows of the batch.
//
// Operand policy P (what differs between the precisions):
//   F32Operands  exact fp32 on the matrix pipe: LDS holds floats, stages of 32 in rows padded to 36 floats (16-byte aligned
//                fragments), 8 x v_mfma_f32_32x32x2_f32 per 16 k-values.
//   F16Operands  the reference's TF32 class (10 explicit mantissa bits, fp32 accumulate): operands are read as fp32 where the
//                parameters live - there is no packed fp16 copy of the weights - and converted while they are written to LDS: log1pf
//                in fp32 first, then a clamp to +-65 504 (the saturation of the MCAB fp16 weight policy) and a plain
//                round-to-nearest-even cast.  NaN operands are outside the contract.  A loader thread carries two consecutive
//                k-values and stores them as one packed dword.  LDS holds halfs, stages of 64 in rows padded to 72 halfs = 144 bytes
//                = 36 dwords: a lane's fragment (8 consecutive k-values of its row, k = 16 u + 8 (lane >> 5) + i) is one 16-byte
//                aligned ds_read_b128, and the 16 lanes one LDS cycle serves (rows l, dword 36 l mod 64 = 0, 36, 8, 44, ... : sixteen
//                different multiples of 4) cover the 64 banks once; the packed stores of a half-wave are 32 consecutive dwords.  One
//                v_mfma_f32_32x32x16_f16 per 16 k-values.
// Loaders (which of a matrix's axes is contiguous):
//   RowLoader      k contiguous (torch's Linear layout, used as it is): thread -> k offsets P::kPer (tid & 31) + i of rows
//                  (tid >> 5) + 8 j; the rows may come from two matrices (a tile whose columns [32, 64) belong to a second weight)
//   StridedLoader  k strided, the tile's row axis contiguous: thread -> row tid & 63 at k offsets (tid >> 6) + 4 j, so a wave reads
//                  64 consecutive rows per 256-byte request (one k-value per thread and pass: F32Operands)
//   StridedPairLoader  the same for a policy with two k-values per dword (F16Operands): thread -> one row, one k-pair per pass
//   ScaledRowLoader / StridedPairLoader<., ., true>  multiply by the operand's power of two first (fp16 training: a gradient operand)
// Epilogues (MODE), all in fp32:
//   LAYER    y = SiLU(s[n] acc + c[n])                        BatchNorm1d(eval) and the Linear bias folded into (s, c)
//   PARTIAL  partial[slot][m, n] = acc                        the raw product of one k-split; the caller sums the slots in order
//   POST     columns [0, 32) of a tile are loc, [32, 64) the log-scale of the SAME 32 latents:  loc, scale = exp(hardtanh(., -7, 5)),
//            z = loc + eps scale
//   LIK      logits (+ the theta product in the same pass when theta is unshared, LIK2: columns [32, 64) of a tile are the theta
//            logits of the 32 genes in columns [0, 32)), written to mu, with one (max, sum exp) pair per (row, tile);
//            softmax_finalize_kernel merges a row's pairs in tile order and rewrites mu in place.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.hpp"

namespace scldm {
namespace scvi {

constexpr int kScviSplit = 1024;           // k-values per split of a product (a multiple of every policy's kBK)
constexpr int kScviMaxLayers = 8;          // per MLP
constexpr int kBM = 64, kBN = 64;
constexpr int kOutLd = kBN + 1;            // LDS row stride (floats) of a staged output tile
constexpr int kEpiBytes = (kBM * kOutLd + 2 * kBM * 4) * 4;   // the epilogues' staged output tile + softmax partials

enum : int { MODE_LAYER = 0, MODE_PARTIAL = 1, MODE_POST = 2, MODE_LIK = 3, MODE_LIK2 = 4 };   // LIK2: unshared theta

struct GemmArgs {
  const float* X;      // (M, K)
  const float* W0;     // (N0, K)
  const float* W1;     // second weight of POST (log-scale) / LIK2 (theta), same shape as W0
  const float* b0;     // bias of W0 (POST, LIK) | s (LAYER)
  const float* b1;     // bias of W1             | c (LAYER)
  int M, N0, K;
  int k_per_split;     // k-values per blockIdx.z (multiple of kBK); >= K when there is one split
  float* out0;         // LAYER: Y (M, N0) | PARTIAL: partials (slots, M, N0) | POST: loc (M, N0) | LIK: mu (M, N0)
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

// ---- operand policies: store() converts and writes the kPer consecutive k-values a loader thread carries, mma16() contracts the 16
// k-values at ap / bp (the lane's row, its 8 of them first)
struct F32Operands {
  using E = float;
  static constexpr int kBK = 32, kLd = kBK + 4, kPer = 1;
  static __device__ __forceinline__ void store(E* p, const float* x) { p[0] = x[0]; }
  static __device__ __forceinline__ f32x16 mma16(const E* ap, const E* bp, f32x16 acc) {
    const f32x4 a0 = *reinterpret_cast<const f32x4*>(ap), a1 = *reinterpret_cast<const f32x4*>(ap + 4);
    const f32x4 b0 = *reinterpret_cast<const f32x4*>(bp), b1 = *reinterpret_cast<const f32x4*>(bp + 4);
    const f32x8 af = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
    const f32x8 bf = {b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
    return OpF32::mma(af, bf, acc);
  }
};
struct F16Operands {
  using E = _Float16;
  static constexpr int kBK = 64, kLd = kBK + 8, kPer = 2;
  typedef __attribute__((ext_vector_type(2))) _Float16 f16x2;
  // saturate at the largest finite half, then round to nearest even (v_cvt_f16_f32 under the default mode)
  static __device__ __forceinline__ _Float16 to_operand(float x) { return (_Float16)__builtin_amdgcn_fmed3f(x, -65504.f, 65504.f); }
  static __device__ __forceinline__ void store(E* p, const float* x) { *reinterpret_cast<f16x2*>(p) = f16x2{to_operand(x[0]), to_operand(x[1])}; }
  static __device__ __forceinline__ f32x16 mma16(const E* ap, const E* bp, f32x16 acc) {
    return OpFP16::mma(*reinterpret_cast<const f16x8*>(ap), *reinterpret_cast<const f16x8*>(bp), acc);
  }
};
template <class P>
constexpr int kStageBytes = 2 * kBM * P::kLd * (int)sizeof(typename P::E);   // the two operand stages; the epilogues reuse them
template <class P>
constexpr int kSmemBytes = kEpiBytes > kStageBytes<P> ? kEpiBytes : kStageBytes<P>;
static_assert(kScviSplit % F32Operands::kBK == 0 && kScviSplit % F16Operands::kBK == 0, "whole stages per split");
static_assert((F32Operands::kLd * 4) % 16 == 0 && (F16Operands::kLd * 2) % 16 == 0, "16-byte aligned fragment rows");

// ---- loaders: prepare(j) once; per stage st = stage(k0, k_hi), then fetch(j, st) issues the global loads of pass j and store(S, j)
// writes them to the operand's LDS stage.  Three details below steer code generation - written otherwise, the compiler picks other
// address arithmetic and load predication for the stage loop (profiles/scvi_tile_isa_identity.txt): lane indices are signed ints (add nsw keeps the k index a plain induction variable),
// an LDS address is one integer index into the stage, and a stage's k / in-range flags are a by-value Stage local to the core's fetch.
template <class P, bool LOG1P>
struct RowLoader {
  // tile rows [0, 64) are rows r0 + r of `base` (row stride ld, n rows); dual: rows r0 + (r & 31) of `base` (r < 32) or of `base1`
  const float *base, *base1;
  bool dual;
  int r0, n;
  size_t ld;
  const float* row[8];   // NULL outside the matrix
  float v[8][P::kPer];
  struct Stage { int k; bool ok[P::kPer]; };
  static __device__ __forceinline__ int lk() { return ((int)threadIdx.x & 31) * P::kPer; }
  static __device__ __forceinline__ int lr() { return (int)threadIdx.x >> 5; }
  __device__ __forceinline__ RowLoader(const float* base_, const float* base1_, bool dual_, int r0_, int n_, size_t ld_)
      : base(base_), base1(base1_), dual(dual_), r0(r0_), n(n_), ld(ld_) {}
  __device__ __forceinline__ RowLoader(const float* base_, int r0_, int n_, size_t ld_) : RowLoader(base_, base_, false, r0_, n_, ld_) {}
  __device__ __forceinline__ void prepare(int j) {
    const int r = lr() + 8 * j;
    const int g = r0 + (dual ? r & 31 : r);
    row[j] = g < n ? ((!dual || r < 32) ? base : base1) + (size_t)g * ld : nullptr;
  }
  __device__ __forceinline__ Stage stage(int k0, int k_hi) const {
    Stage st;
    st.k = k0 + lk();
#pragma unroll
    for (int i = 0; i < P::kPer; ++i) st.ok[i] = st.k + i < k_hi;
    return st;
  }
  __device__ __forceinline__ void fetch(int j, const Stage& st) {
#pragma unroll
    for (int i = 0; i < P::kPer; ++i) v[j][i] = (st.ok[i] && row[j]) ? row[j][st.k + i] : 0.f;
  }
  __device__ __forceinline__ void store(typename P::E* S, int j) const {
    float x[P::kPer];
#pragma unroll
    for (int i = 0; i < P::kPer; ++i) x[i] = LOG1P ? log1pf(v[j][i]) : v[j][i];
    P::store(&S[(lr() + 8 * j) * P::kLd + lk()], x);
  }
};

template <class P, bool LOG1P>
struct StridedLoader {
  static_assert(P::kPer == 1, "one k-value per thread and pass");
  const float* base;     // (K, n) with row stride ld
  size_t ld;
  int r0, n;             // the thread's row is r0 + tr() of the n rows behind the tile
  float v[8];
  struct Stage { int k0, k_hi; };
  static __device__ __forceinline__ int tr() { return (int)threadIdx.x & 63; }
  static __device__ __forceinline__ int tk() { return (int)threadIdx.x >> 6; }
  __device__ __forceinline__ StridedLoader(const float* base_, int r0_, int n_, size_t ld_) : base(base_), ld(ld_), r0(r0_), n(n_) {}
  __device__ __forceinline__ void prepare(int) {}
  __device__ __forceinline__ Stage stage(int k0, int k_hi) const { return Stage{k0, k_hi}; }
  __device__ __forceinline__ void fetch(int j, const Stage& st) {
    const int k = st.k0 + tk() + 4 * j, r = r0 + tr();
    v[j] = (k < st.k_hi && r < n) ? base[(size_t)k * ld + r] : 0.f;
  }
  __device__ __forceinline__ void store(typename P::E* S, int j) const {
    const float x = LOG1P ? log1pf(v[j]) : v[j];
    P::store(&S[tr() * P::kLd + tk() + 4 * j], &x);
  }
};

// ---- the power-of-two scale of a gradient operand (fp16 training: fp16 has TF32's mantissa but five exponent bits).  `m` is the
// largest magnitude of the tensor as fp32 bits (sign cleared; an unsigned maximum, exact in any order).  e = 10 - floor(log2(max)),
// so max |2^e d| lies in [1024, 2048); zero and non-finite maxima take e = 0; |e| <= 126 keeps 2^e and 2^-e normal fp32.
__device__ __forceinline__ bool scale_max_finite(uint32_t m) { return m < 0x7f800000u; }
__device__ __forceinline__ int scale_exponent(uint32_t m) {
  if (m == 0u || !scale_max_finite(m)) return 0;
  const int e = 10 - ((int)(m >> 23) - 127);
  return min(max(e, -126), 126);
}
__device__ __forceinline__ float pow2_f(int e) { return __uint_as_float((uint32_t)(e + 127) << 23); }
__device__ __forceinline__ uint32_t magnitude_bits(float x) { return __float_as_uint(x) & 0x7fffffffu; }

// RowLoader whose values are multiplied by `mul` (a power of two: exact in fp32) before the policy's clamp and cast
template <class P>
struct ScaledRowLoader : RowLoader<P, false> {
  using Base = RowLoader<P, false>;
  float mul;
  __device__ __forceinline__ ScaledRowLoader(const float* base_, int r0_, int n_, size_t ld_, float mul_) : Base(base_, r0_, n_, ld_), mul(mul_) {}
  __device__ __forceinline__ void store(typename P::E* S, int j) const {
    float x[P::kPer];
#pragma unroll
    for (int i = 0; i < P::kPer; ++i) x[i] = this->v[j][i] * mul;
    P::store(&S[(Base::lr() + 8 * j) * P::kLd + Base::lk()], x);
  }
};

// StridedLoader for a policy that packs two consecutive k-values per dword (F16Operands).  A wave covers 32 consecutive rows of
// two neighbouring k-pairs: lanes [0, 16) and [32, 48) rows 0-15 / 16-31 of the wave's 32 at k-pair p, lanes [16, 32) and [48, 64)
// the same rows at k-pair p + 1, so each global load instruction reads two runs of 32 consecutive floats (128 bytes) per k-value.
// The packed ds_write_b32 of a 32-lane group (the unit that conflicts, bank = dword mod 32) goes to dwords 36 r + p: 16 rows
// give 4 r mod 32 = eight multiples of 4, each twice, and p, p + 1 land on neighbouring banks - 16 banks, two addresses each: a
// two-way conflict, which costs ds_write_b32 no extra cycle.  (One row per lane, the fp32 StridedLoader's shape, would be
// four-way: twice the cycles.)  A pair that straddles k_hi (an odd K) keeps its first half and zeroes the second.
template <class P, bool LOG1P, bool SCALED>
struct StridedPairLoader {
  static_assert(P::kPer == 2 && P::kBK == 64, "two k-values per thread and pass, 32 pairs per stage");
  const float* base;     // (K, n) with row stride ld
  size_t ld;
  int r0, n;
  float mul;             // SCALED: the operand's power of two
  float v[8][2];
  struct Stage { int k0, k_hi; };
  static __device__ __forceinline__ int tr() {
    const int lane = (int)threadIdx.x & 63, w = (int)threadIdx.x >> 6;
    return 32 * (w & 1) + 16 * (lane >> 5) + (lane & 15);
  }
  static __device__ __forceinline__ int tp() { return 2 * ((int)threadIdx.x >> 7) + (((int)threadIdx.x >> 4) & 1); }   // pass j: k-pair tp() + 4 j
  __device__ __forceinline__ StridedPairLoader(const float* base_, int r0_, int n_, size_t ld_, float mul_ = 1.f)
      : base(base_), ld(ld_), r0(r0_), n(n_), mul(mul_) {}
  __device__ __forceinline__ void prepare(int) {}
  __device__ __forceinline__ Stage stage(int k0, int k_hi) const { return Stage{k0, k_hi}; }
  __device__ __forceinline__ void fetch(int j, const Stage& st) {
    const int k = st.k0 + 2 * (tp() + 4 * j), r = r0 + tr();
#pragma unroll
    for (int i = 0; i < 2; ++i) v[j][i] = (k + i < st.k_hi && r < n) ? base[(size_t)(k + i) * ld + r] : 0.f;
  }
  __device__ __forceinline__ void store(typename P::E* S, int j) const {
    float x[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      x[i] = LOG1P ? log1pf(v[j][i]) : v[j][i];
      if (SCALED) x[i] *= mul;
    }
    P::store(&S[tr() * P::kLd + 2 * (tp() + 4 * j)], x);
  }
};

// ---- the product core: acc = sum over k in [k_lo, k_hi) of the tile's A rows times its B rows.  smem holds kStageBytes<P>.
template <class P, class LA, class LB>
__device__ __forceinline__ f32x16 tile_product(LA& la, LB& lb, unsigned char* smem, int k_lo, int k_hi) {
  using E = typename P::E;
  E* As = reinterpret_cast<E*>(smem);
  E* Bs = As + kBM * P::kLd;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    la.prepare(j);
    lb.prepare(j);
  }
  auto fetch = [&](int k0) {
    const auto sa = la.stage(k0, k_hi);
    const auto sb = lb.stage(k0, k_hi);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      la.fetch(j, sa);
      lb.fetch(j, sb);
    }
  };
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  if (k_lo < k_hi) fetch(k_lo);
  const int hh = lane >> 5, l31 = lane & 31;
  for (int k0 = k_lo; k0 < k_hi; k0 += P::kBK) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      la.store(As, j);
      lb.store(Bs, j);
    }
    __syncthreads();
    if (k0 + P::kBK < k_hi) fetch(k0 + P::kBK);
#pragma unroll
    for (int u = 0; u < P::kBK / 16; ++u)
      acc = P::mma16(&As[(wm * 32 + l31) * P::kLd + u * 16 + 8 * hh], &Bs[(wn * 32 + l31) * P::kLd + u * 16 + 8 * hh], acc);
    __syncthreads();
  }
  return acc;
}

// ---- the epilogues: lane holds column wn * 32 + l31 of the tile, register r row wm * 32 + acc_row(r, hh).  smem holds kEpiBytes
// (unused by LAYER and PARTIAL); PARTIAL writes slot `slot` of out0.
template <int MODE>
__device__ __forceinline__ void tile_epilogue(const GemmArgs& a, const f32x16& acc, float* smem, size_t slot) {
  using T = Traits<MODE>;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1, hh = lane >> 5, l31 = lane & 31;
  const int m0 = blockIdx.y * kBM, n0 = blockIdx.x * T::kCols;
  if (MODE == MODE_LAYER || MODE == MODE_PARTIAL) {
    const int n = n0 + wn * 32 + l31;
    if (n >= a.N0) return;
    float s = 1.f, c = 0.f;
    if (MODE == MODE_LAYER) { s = a.b0[n]; c = a.b1[n]; }
    float* out = a.out0 + (MODE == MODE_PARTIAL ? slot * a.M * a.N0 : 0);
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

}  // namespace scvi
}  // namespace scldm

// The backward products of scvi_train.hpp in a header of their own (prod_kernel and sum_slots_kernel, both templates, with the text they
// had there), so that another translation unit can instantiate them without that header's other kernels: the training backward of the
// wide TransformerVAE route (vae_wide_train_api.hip) does.  What they compute is described at the top of scvi_train.hpp.
#pragma once
#include <type_traits>

#include "scvi_tile.hpp"

namespace scldm {
namespace scvi_train {

struct ProdArgs {
  const float* A;        // AT: (K, M) with row stride lda | else (M, K) with row stride lda
  const float* Bm;       // (K, N) with row stride ldb
  long long lda, ldb;
  int M, N, K;
  int k_per_split;       // k-values per blockIdx.z (multiple of kBK)
  float* out;            // (slots, M, N); this launch writes slots slot0 + blockIdx.z
  int slot0;
  const uint32_t* a_max; // F16Operands: the magnitude-bit maximum of A (a gradient tensor)
  float* found_inf;      // F16Operands: set to 1 on a non-finite maximum or result; may be NULL
};

template <class P, bool AT, bool LOG1P_B>
__global__ __launch_bounds__(256) void prod_kernel(const ProdArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[scvi::kStageBytes<P>];
  if constexpr (std::is_same_v<P, scvi::F32Operands>) {      // statement for statement the fp32 kernel as it was (its code generation follows the order)
    using LA = std::conditional_t<AT, scvi::StridedLoader<P, false>, scvi::RowLoader<P, false>>;
    LA la(a.A, blockIdx.y * scvi::kBM, a.M, a.lda);
    scvi::StridedLoader<P, LOG1P_B> lb(a.Bm, blockIdx.x * scvi::kBN, a.N, a.ldb);
    const int k_lo = blockIdx.z * a.k_per_split;
    const int k_hi = min(a.K, k_lo + a.k_per_split);
    const f32x16 acc = scvi::tile_product<P>(la, lb, smem, k_lo, k_hi);
    scvi::GemmArgs g = {};
    g.M = a.M;
    g.N0 = a.N;
    g.out0 = a.out;
    scvi::tile_epilogue<scvi::MODE_PARTIAL>(g, acc, nullptr, a.slot0 + blockIdx.z);
  } else {
    using LA = std::conditional_t<AT, scvi::StridedPairLoader<P, false, true>, scvi::ScaledRowLoader<P>>;
    const uint32_t mx = *a.a_max;
    const int e = scvi::scale_exponent(mx);
    LA la(a.A, blockIdx.y * scvi::kBM, a.M, a.lda, scvi::pow2_f(e));
    scvi::StridedPairLoader<P, LOG1P_B, false> lb(a.Bm, blockIdx.x * scvi::kBN, a.N, a.ldb);
    const int k_lo = blockIdx.z * a.k_per_split;
    const int k_hi = min(a.K, k_lo + a.k_per_split);
    f32x16 acc = scvi::tile_product<P>(la, lb, smem, k_lo, k_hi);
    scvi::GemmArgs g = {};
    g.M = a.M;
    g.N0 = a.N;
    g.out0 = a.out;
    const float inv = scvi::pow2_f(-e);
    bool bad = !scvi::scale_max_finite(mx);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      acc[r] *= inv;
      bad |= !scvi::scale_max_finite(scvi::magnitude_bits(acc[r]));
    }
    if (bad && a.found_inf) *a.found_inf = 1.0f;
    scvi::tile_epilogue<scvi::MODE_PARTIAL>(g, acc, nullptr, a.slot0 + blockIdx.z);
  }
}

__device__ __forceinline__ bool finite_f(float x) { return scvi::scale_max_finite(scvi::magnitude_bits(x)); }

// out = slot 0 + slot 1 + ... in slot order
template <bool F16>
__global__ __launch_bounds__(256) void sum_slots_kernel(const float* __restrict__ part, int slots, size_t plane, float* __restrict__ out,
                                                        float* found_inf) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= plane) return;
  float v = part[i];
  for (int z = 1; z < slots; ++z) v += part[z * plane + i];
  out[i] = v;
  if (F16 && found_inf && !finite_f(v)) *found_inf = 1.0f;
}

}  // namespace scvi_train
}  // namespace scldm

// What the two batch-preparation kernels share (train_step.hip: the default transport; train_step_transport.hip: every other): the
// Philox4x32-10 generator, its uniforms, the counter tags and the argument block - one definition, so that both make the same draws.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#pragma clang fp contract(off)

namespace scldm {
namespace fmstep {

struct U4 { uint32_t x, y, z, w; };
__device__ __forceinline__ U4 philox4(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return U4{c0, c1, c2, c3};
}
__device__ __forceinline__ float u01(uint32_t w) { return ((w >> 8) + 0.5f) * (1.0f / 16777216.0f); }   // (0, 1), 24 bits
__device__ __forceinline__ float u01_closed0(uint32_t w) { return (float)(w >> 8) * (1.0f / 16777216.0f); }   // [0, 1): torch.rand's range

enum : uint32_t { TAG_X0 = 0x78300000u, TAG_ROW = 0x726f7700u, TAG_STEP = 0x73746570u };

struct PrepArgs {
  const float* x1;                  // (n, e)
  const int64_t* labels_in[8];      // per class (sorted-name order): (n) labels, or nullptr = class absent from `condition`
  int null_token[8];                // class vocabulary size = its null token
  int n_classes, strategy;          // strategy 0 mutually_exclusive, 1 joint
  int drop;                         // apply label dropout (training mode / force_drop_ids)
  float p_drop;
  const unsigned long long* rng;    // device: [0] seed, [1] step counter
  float* t;                         // (n)
  float* x0;                        // (n, e) or nullptr
  float* xt; float* ut;             // (n, e)
  int64_t* labels_out;              // (n_classes, n): what the model sees
  int n, e;
};

constexpr int kLossRows = 8;      // batch rows per workgroup of the loss kernels (one wave per row, two rounds)

}  // namespace fmstep
}  // namespace scldm

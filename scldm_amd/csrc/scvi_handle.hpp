// What the two translation units of the scVI-style baseline share (scvi_api.hip: handle, packing, eval entries; scvi_train_api.hip:
// training entries): the handle, the argument checks, and the three eval launches the training forward reuses, which scvi_api.hip
// defines.
#pragma once
#include <hip/hip_runtime.h>

#include "api_common.hpp"
#include "scvi_tile.hpp"

struct scldm_scvi {
  int n_enc, n_dec, G, H, L, shared_theta;
  float bn_eps;
  bool packed;
  scldm_scvi_layer enc[scldm::scvi::kScviMaxLayers], dec[scldm::scvi::kScviMaxLayers];
  scldm_scvi_params p;            // p.enc / p.dec point at the two arrays above
  float *d_s, *d_c;               // (n_enc + n_dec, H) folded BatchNorm scale / shift
  unsigned long long* d_fp;       // pack_kernel's fingerprint state
  float* found_inf;               // fp16 training backward: caller-owned device float (scldm_scvi_train_set_found_inf), may be NULL
};

namespace scldm {
namespace scvi_host {
using scvi::kScviMaxLayers;
using scvi::kScviSplit;

static inline bool misaligned(const void* p, size_t a) { return (reinterpret_cast<size_t>(p) & (a - 1)) != 0; }
static inline int splits_of(int K) { return cdiv(K, kScviSplit); }
// k-values per blockIdx.z of a product over K on operand policy P: a whole split, or all of K in whole stages
template <class P>
static inline int k_per_split(int K) { return splits_of(K) > 1 ? kScviSplit : cdiv(K, P::kBK) * P::kBK; }
static inline int lik_tiles(const scldm_scvi* h) { return cdiv(h->G, h->shared_theta ? 64 : 32); }

static inline int check_ptr(const char* entry, const char* name, const void* p, bool required) {
  if (!p) return required ? fail(SCLDM_ERR_SHAPE, "%s: %s is NULL", entry, name) : SCLDM_OK;
  if (misaligned(p, 4)) return fail(SCLDM_ERR_SHAPE, "%s: %s is not 4-byte aligned", entry, name);
  return SCLDM_OK;
}
#define CHECK_PTR(entry, p, required)                                          \
  do {                                                                         \
    const int rc_ = scldm::scvi_host::check_ptr(entry, #p, p, required);       \
    if (rc_ != SCLDM_OK) return rc_;                                           \
  } while (0)

static inline int check_packed(const char* entry, const scldm_scvi* h) {   // after every argument check
  if (!h->packed) return fail(SCLDM_ERR_STATE, "%s: scldm_scvi_pack has not been called", entry);
  return SCLDM_OK;
}

// defined in scvi_api.hip, on the kernels of scvi.hpp
void launch_pack(const scldm_scvi* h, int force, hipStream_t st);
// raw products X (B, K) W (N, K)^T on the operands of `precision` into slots [0, splits) of `part` (splits, B, N), log1p applied to X
// while staging; returns the splits
int launch_raw(const float* X, int K, bool log1p, const float* W, int N, int B, float* part, int precision, hipStream_t st);
// mu = library softmax_G(x W_mu^T + b), theta (shared: softplus of the parameter; else softplus(x W_theta^T + b)) of x (B, H), the
// products on the operands of `precision` (SCLDM_PREC_FP32 or SCLDM_PREC_FP16)
int lik_head_impl(const scldm_scvi* h, const float* x, const float* library, int B, float* mu, float* theta, float* pairs, int precision,
                  hipStream_t st);

}  // namespace scvi_host
}  // namespace scldm

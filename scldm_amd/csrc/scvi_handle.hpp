// What the translation units of the scVI-style baseline share (scvi_api.hip: handle, packing, eval entries; scvi_train_api.hip:
// training entries; scvi_fp16_api.hip: the eval entries with a precision argument): the handle, the argument checks, and the eval
// launches the other two reuse, which scvi_api.hip defines - its kernels (scvi.hpp) stay in one device module, so adding training or
// fp16 code cannot change how they compile.
#pragma once
#include <hip/hip_runtime.h>

#include "api_common.hpp"

namespace scldm {
namespace scvi_host {
constexpr int kScviMaxLayers = 8;       // per MLP (= scvi::kMaxLayers)
constexpr int kScviSplit = 1024;       // k-values per split of a product (= scvi::kScviSplitK)
}  // namespace scvi_host
}  // namespace scldm

struct scldm_scvi {
  int n_enc, n_dec, G, H, L, shared_theta;
  float bn_eps;
  bool packed;
  scldm_scvi_layer enc[scldm::scvi_host::kScviMaxLayers], dec[scldm::scvi_host::kScviMaxLayers];
  scldm_scvi_params p;            // p.enc / p.dec point at the two arrays above
  float *d_s, *d_c;               // (n_enc + n_dec, H) folded BatchNorm scale / shift
  unsigned long long* d_fp;       // pack_kernel's fingerprint state
};

namespace scldm {
namespace scvi_host {

static inline bool misaligned(const void* p, size_t a) { return (reinterpret_cast<size_t>(p) & (a - 1)) != 0; }
static inline int splits_of(int K) { return cdiv(K, kScviSplit); }
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
// raw products X (B, K) W (N, K)^T into slots [0, splits) of `part` (splits, B, N), log1p applied to X while staging; returns the splits
int launch_raw(const float* X, int K, bool log1p, const float* W, int N, int B, float* part, hipStream_t st);
// mu = library softmax_G(x W_mu^T + b), theta (shared: softplus of the parameter; else softplus(x W_theta^T + b)) of x (B, H)
int lik_head_impl(const scldm_scvi* h, const float* x, const float* library, int B, float* mu, float* theta, float* pairs, hipStream_t st);

// ---- what scvi_fp16_api.hip (the entries with a precision argument) shares, defined in scvi_api.hip as well
// the argument checks of scldm_scvi_encode / _decode / _forward under the caller's entry name (before check_packed)
int eval_check_encode(const char* entry, const scldm_scvi* h, const float* counts, int B, const float* eps, const float* hout,
                      const float* loc, const float* scale, const float* z, const void* ws);
int eval_check_decode(const char* entry, const scldm_scvi* h, const float* z, const float* library, int n_library, int B, const float* mu,
                      const float* theta, const void* ws);
int eval_check_forward(const char* entry, const scldm_scvi* h, const float* counts, const float* library, int n_library, int B,
                       const float* eps, const float* hout, const float* loc, const float* scale, const float* z, const float* mu,
                       const float* theta, const void* ws);
// the slots of the workspace of scldm_scvi_workspace_bytes
struct EvalWorkspace { float* act[2]; float* part; float* pairs; };
EvalWorkspace eval_workspace(const scldm_scvi* h, int B, char* ws);
// the launches of scldm_scvi_encode / _decode behind the fingerprint / pack launch
int encode_fp32(const scldm_scvi* h, const float* counts, int B, const float* eps, float* hout, float* loc, float* scale, float* z, char* ws,
                hipStream_t st);
int decode_fp32(const scldm_scvi* h, const float* z, const float* library, int B, float* mu, float* theta, char* ws, hipStream_t st);
// Y = SiLU(s (sum of the splits of `part`, in split order) + c)
void launch_merge(const float* part, int splits, size_t plane, int N, const float* s, const float* c, float* Y, hipStream_t st);
// mu = library softmax over the (max, sum exp) pairs of `tiles` = lik_tiles(h) tiles per row, in place; the shared theta's softplus
int launch_softmax_finalize(const scldm_scvi* h, const float* library, int B, float* mu, float* theta, const float* pairs, hipStream_t st);

}  // namespace scvi_host
}  // namespace scldm

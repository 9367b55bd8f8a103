// C ABI of the scVI-style baseline VAE with a precision argument (include/scldm_hip.h): scldm_scvi_encode_ex / _decode_ex /
// _forward_ex.  SCLDM_PREC_FP32 runs the launches of scvi_api.hip's entries (through scvi_handle.hpp), SCLDM_PREC_FP16 the tile kernel
// of scvi_fp16.hpp in their place; pack, merge and softmax-finalize are the fp32 path's own kernels in both.  Every entry checks its
// arguments before the first HIP call and makes launches only (no host read, no copy).
#include <hip/hip_runtime.h>

#include "scvi_fp16.hpp"
#include "scvi_handle.hpp"

using namespace scldm;
using namespace scldm::scvi16;
using namespace scldm::scvi_host;
static_assert(scvi_host::kScviSplit == kSplitK, "scvi_handle.hpp restates scvi_fp16.hpp");

namespace {

int check_precision(const char* entry, int precision) {
  if (precision != SCLDM_PREC_FP32 && precision != SCLDM_PREC_FP16)
    return fail(SCLDM_ERR_SHAPE, "%s: precision %d is not built for the scVI baseline (SCLDM_PREC_FP32 or SCLDM_PREC_FP16)", entry, precision);
  return SCLDM_OK;
}

// Y (B, H) = SiLU(s (act(X) W^T) + c), K split by kSplitK
void launch_layer(const scldm_scvi* h, const float* X, int K, bool log1p, const float* W, int layer, float* Y, int B, float* part,
                  hipStream_t st) {
  GemmArgs a = {};
  a.X = X;
  a.W0 = W;
  a.b0 = h->d_s + (size_t)layer * h->H;
  a.b1 = h->d_c + (size_t)layer * h->H;
  a.M = B;
  a.N0 = h->H;
  a.K = K;
  const int sp = splits_of(K);
  a.k_per_split = sp > 1 ? kSplitK : cdiv(K, kBK) * kBK;
  const dim3 grid(cdiv(h->H, kBN), cdiv(B, kBM), sp);
  if (sp == 1) {
    a.out0 = Y;
    if (log1p) hipLaunchKernelGGL((gemm_kernel<MODE_LAYER, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((gemm_kernel<MODE_LAYER, false>), grid, dim3(256), 0, st, a);
  } else {
    a.out0 = part;
    if (log1p) hipLaunchKernelGGL((gemm_kernel<MODE_PARTIAL, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((gemm_kernel<MODE_PARTIAL, false>), grid, dim3(256), 0, st, a);
    launch_merge(part, sp, (size_t)B * h->H, h->H, a.b0, a.b1, Y, st);
  }
}

int encode_fp16(const scldm_scvi* h, const float* counts, int B, const float* eps, float* hout, float* loc, float* scale, float* z,
                char* ws, hipStream_t st) {
  const EvalWorkspace l = eval_workspace(h, B, ws);
  const float* x = counts;
  for (int i = 0; i < h->n_enc; ++i) {
    float* y = i == h->n_enc - 1 ? hout : l.act[i & 1];
    launch_layer(h, x, i == 0 ? h->G : h->H, i == 0, h->enc[i].w, i, y, B, l.part, st);
    x = y;
  }
  LAUNCH_CHECK();
  GemmArgs a = {};
  a.X = hout;
  a.W0 = h->p.loc_w;
  a.W1 = h->p.scale_w;
  a.b0 = h->p.loc_b;
  a.b1 = h->p.scale_b;
  a.M = B;
  a.N0 = h->L;
  a.K = h->H;
  a.k_per_split = cdiv(h->H, kBK) * kBK;
  a.out0 = loc;
  a.out1 = scale;
  a.out2 = eps ? z : nullptr;
  a.eps = eps;
  hipLaunchKernelGGL((gemm_kernel<MODE_POST, false>), dim3(cdiv(h->L, 32), cdiv(B, kBM), 1), dim3(256), 0, st, a);
  LAUNCH_CHECK();
  return SCLDM_OK;
}

int decode_fp16(const scldm_scvi* h, const float* z, const float* library, int B, float* mu, float* theta, char* ws, hipStream_t st) {
  const EvalWorkspace l = eval_workspace(h, B, ws);
  const float* x = z;
  for (int i = 0; i < h->n_dec; ++i) {
    launch_layer(h, x, i == 0 ? h->L : h->H, false, h->dec[i].w, h->n_enc + i, l.act[i & 1], B, l.part, st);
    x = l.act[i & 1];
  }
  LAUNCH_CHECK();
  GemmArgs a = {};
  a.X = x;
  a.W0 = h->p.mu_w;
  a.b0 = h->p.mu_b;
  a.M = B;
  a.N0 = h->G;
  a.K = h->H;
  a.k_per_split = cdiv(h->H, kBK) * kBK;
  a.out0 = mu;
  a.pairs = l.pairs;
  const dim3 grid(lik_tiles(h), cdiv(B, kBM), 1);
  if (h->shared_theta) {
    hipLaunchKernelGGL((gemm_kernel<MODE_LIK, false>), grid, dim3(256), 0, st, a);
  } else {
    a.W1 = h->p.theta_w;
    a.b1 = h->p.theta_b;
    a.out1 = theta;
    hipLaunchKernelGGL((gemm_kernel<MODE_LIK2, false>), grid, dim3(256), 0, st, a);
  }
  LAUNCH_CHECK();
  return launch_softmax_finalize(h, library, B, mu, theta, l.pairs, st);
}

}  // namespace

extern "C" int scldm_scvi_encode_ex(scldm_scvi* h, const float* counts, int B, const float* eps, float* hout, float* loc, float* scale,
                                    float* z, int precision, void* ws, void* stream_) {
  const char* entry = "scldm_scvi_encode_ex";
  int rc = eval_check_encode(entry, h, counts, B, eps, hout, loc, scale, z, ws);
  if (rc == SCLDM_OK) rc = check_precision(entry, precision);
  if (rc == SCLDM_OK) rc = check_packed(entry, h);
  if (rc != SCLDM_OK) return rc;
  hipStream_t st = (hipStream_t)stream_;
  launch_pack(h, 0, st);
  if (precision == SCLDM_PREC_FP32) return encode_fp32(h, counts, B, eps, hout, loc, scale, z, (char*)ws, st);
  return encode_fp16(h, counts, B, eps, hout, loc, scale, z, (char*)ws, st);
}

extern "C" int scldm_scvi_decode_ex(scldm_scvi* h, const float* z, const float* library_size, int n_library, int B, float* mu, float* theta,
                                    int precision, void* ws, void* stream_) {
  const char* entry = "scldm_scvi_decode_ex";
  int rc = eval_check_decode(entry, h, z, library_size, n_library, B, mu, theta, ws);
  if (rc == SCLDM_OK) rc = check_precision(entry, precision);
  if (rc == SCLDM_OK) rc = check_packed(entry, h);
  if (rc != SCLDM_OK) return rc;
  hipStream_t st = (hipStream_t)stream_;
  launch_pack(h, 0, st);
  if (precision == SCLDM_PREC_FP32) return decode_fp32(h, z, library_size, B, mu, theta, (char*)ws, st);
  return decode_fp16(h, z, library_size, B, mu, theta, (char*)ws, st);
}

extern "C" int scldm_scvi_forward_ex(scldm_scvi* h, const float* counts, const float* library_size, int n_library, int B, const float* eps,
                                     float* hout, float* loc, float* scale, float* z, float* mu, float* theta, int precision, void* ws,
                                     void* stream_) {
  const char* entry = "scldm_scvi_forward_ex";
  int rc = eval_check_forward(entry, h, counts, library_size, n_library, B, eps, hout, loc, scale, z, mu, theta, ws);
  if (rc == SCLDM_OK) rc = check_precision(entry, precision);
  if (rc == SCLDM_OK) rc = check_packed(entry, h);
  if (rc != SCLDM_OK) return rc;
  hipStream_t st = (hipStream_t)stream_;
  launch_pack(h, 0, st);
  const bool f16 = precision == SCLDM_PREC_FP16;
  rc = f16 ? encode_fp16(h, counts, B, eps, hout, loc, scale, z, (char*)ws, st) : encode_fp32(h, counts, B, eps, hout, loc, scale, z, (char*)ws, st);
  if (rc != SCLDM_OK) return rc;
  return f16 ? decode_fp16(h, z, library_size, B, mu, theta, (char*)ws, st) : decode_fp32(h, z, library_size, B, mu, theta, (char*)ws, st);
}

// C ABI of the scVI-style baseline VAE (include/scldm_hip.h): scldm_scvi_create / _destroy / _pack / _workspace_bytes / _encode /
// _decode / _forward and their _ex forms with a precision argument; the training entries are in scvi_train_api.hip.  Every entry
// checks its arguments before the first HIP call and makes launches only (no host read, no copy).
#include <hip/hip_runtime.h>

#include <new>

#include "scvi.hpp"
#include "scvi_handle.hpp"

using namespace scldm;
using namespace scldm::scvi;
using namespace scldm::scvi_host;

namespace {

struct Layout { size_t act0, act1, part, pairs, total; };
Layout layout_of(const scldm_scvi* h, int B) {
  Layout l;
  size_t o = 0;
  auto take = [&](size_t bytes) { size_t r = o; o += align256(bytes); return r; };
  int sp = splits_of(h->G);
  if (splits_of(h->H) > sp) sp = splits_of(h->H);
  if (splits_of(h->L) > sp) sp = splits_of(h->L);
  l.act0 = take((size_t)B * h->H * 4);
  l.act1 = take((size_t)B * h->H * 4);
  l.part = take(sp > 1 ? (size_t)sp * B * h->H * 4 : 0);
  l.pairs = take((size_t)B * lik_tiles(h) * 2 * 4);
  l.total = o;
  return l;
}

int check_call(const char* entry, const scldm_scvi* h, int B, const void* ws) {
  if (!h) return fail(SCLDM_ERR_SHAPE, "%s: NULL handle", entry);
  if (B < 1) return fail(SCLDM_ERR_SHAPE, "%s: need B >= 1 (got %d)", entry, B);
  if (!ws) return fail(SCLDM_ERR_SHAPE, "%s: ws is NULL", entry);
  if (misaligned(ws, 256)) return fail(SCLDM_ERR_SHAPE, "%s: ws is not 256-byte aligned", entry);
  return SCLDM_OK;
}

// gemm_kernel<., MODE, LOG1P> on the operands of `precision` over the whole of a.out0's (M, N0); only PARTIAL splits K
template <int MODE, bool LOG1P = false>
void launch_gemm(int precision, GemmArgs a, hipStream_t st) {
  const bool f16 = precision == SCLDM_PREC_FP16;
  const int bk = f16 ? F16Operands::kBK : F32Operands::kBK;
  const int sp = MODE == MODE_PARTIAL ? splits_of(a.K) : 1;
  a.k_per_split = sp > 1 ? kScviSplit : cdiv(a.K, bk) * bk;
  const dim3 grid(cdiv(a.N0, Traits<MODE>::kCols), cdiv(a.M, kBM), sp);
  if (f16) hipLaunchKernelGGL((gemm_kernel<F16Operands, MODE, LOG1P>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((gemm_kernel<F32Operands, MODE, LOG1P>), grid, dim3(256), 0, st, a);
}

// Y (B, H) = SiLU(s (act(X) W^T) + c), K split by kScviSplit
void launch_layer(const scldm_scvi* h, int precision, const float* X, int K, bool log1p, const float* W, int layer, float* Y, int B,
                  float* part, hipStream_t st) {
  GemmArgs a = {};
  a.X = X;
  a.W0 = W;
  a.b0 = h->d_s + (size_t)layer * h->H;
  a.b1 = h->d_c + (size_t)layer * h->H;
  a.M = B;
  a.N0 = h->H;
  a.K = K;
  const int sp = splits_of(K);
  if (sp == 1) {
    a.out0 = Y;
    if (log1p) launch_gemm<MODE_LAYER, true>(precision, a, st);
    else launch_gemm<MODE_LAYER>(precision, a, st);
  } else {
    a.out0 = part;
    if (log1p) launch_gemm<MODE_PARTIAL, true>(precision, a, st);
    else launch_gemm<MODE_PARTIAL>(precision, a, st);
    const size_t plane = (size_t)B * h->H;
    hipLaunchKernelGGL(merge_kernel, dim3(cdiv((long long)plane, 256)), dim3(256), 0, st, part, sp, plane, h->H, a.b0, a.b1, Y);
  }
}

int encode_impl(const scldm_scvi* h, int precision, const float* counts, int B, const float* eps, float* hout, float* loc, float* scale,
                float* z, char* ws, hipStream_t st) {
  const Layout l = layout_of(h, B);
  float* act[2] = {(float*)(ws + l.act0), (float*)(ws + l.act1)};
  float* part = (float*)(ws + l.part);
  const float* x = counts;
  for (int i = 0; i < h->n_enc; ++i) {
    float* y = i == h->n_enc - 1 ? hout : act[i & 1];
    launch_layer(h, precision, x, i == 0 ? h->G : h->H, i == 0, h->enc[i].w, i, y, B, part, st);
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
  a.out0 = loc;
  a.out1 = scale;
  a.out2 = eps ? z : nullptr;
  a.eps = eps;
  launch_gemm<MODE_POST>(precision, a, st);
  LAUNCH_CHECK();
  return SCLDM_OK;
}

int decode_impl(const scldm_scvi* h, int precision, const float* z, const float* library, int B, float* mu, float* theta, char* ws,
                hipStream_t st) {
  const Layout l = layout_of(h, B);
  float* act[2] = {(float*)(ws + l.act0), (float*)(ws + l.act1)};
  float* part = (float*)(ws + l.part);
  const float* x = z;
  for (int i = 0; i < h->n_dec; ++i) {
    launch_layer(h, precision, x, i == 0 ? h->L : h->H, false, h->dec[i].w, h->n_enc + i, act[i & 1], B, part, st);
    x = act[i & 1];
  }
  LAUNCH_CHECK();
  return lik_head_impl(h, x, library, B, mu, theta, (float*)(ws + l.pairs), precision, st);
}

int check_encode(const char* entry, const scldm_scvi* h, const float* counts, int B, const float* eps, const float* hout, const float* loc,
                 const float* scale, const float* z, const void* ws) {
  int rc = check_call(entry, h, B, ws);
  if (rc != SCLDM_OK) return rc;
  CHECK_PTR(entry, counts, true);
  CHECK_PTR(entry, hout, true);
  CHECK_PTR(entry, loc, true);
  CHECK_PTR(entry, scale, true);
  CHECK_PTR(entry, eps, false);
  CHECK_PTR(entry, z, eps != nullptr);
  return SCLDM_OK;
}
int check_decode(const char* entry, const scldm_scvi* h, const float* z, const float* library, int n_library, int B, const float* mu,
                 const float* theta, const void* ws) {
  int rc = check_call(entry, h, B, ws);
  if (rc != SCLDM_OK) return rc;
  if (n_library != B) return fail(SCLDM_ERR_SHAPE, "%s: library_size has %d entries for %d cells", entry, n_library, B);
  CHECK_PTR(entry, z, true);
  CHECK_PTR(entry, library, true);
  CHECK_PTR(entry, mu, true);
  CHECK_PTR(entry, theta, true);
  return SCLDM_OK;
}
// the last two checks of every eval entry, after those of its arguments
int check_precision_packed(const char* entry, const scldm_scvi* h, int precision) {
  if (precision != SCLDM_PREC_FP32 && precision != SCLDM_PREC_FP16)
    return fail(SCLDM_ERR_SHAPE, "%s: precision %d is not built for the scVI baseline (SCLDM_PREC_FP32 or SCLDM_PREC_FP16)", entry, precision);
  return check_packed(entry, h);
}

// ---- the eval entries under the name of the C entry that forwards to them
int encode_entry(const char* entry, scldm_scvi* h, const float* counts, int B, const float* eps, float* hout, float* loc, float* scale,
                 float* z, int precision, void* ws, void* stream_) {
  int rc = check_encode(entry, h, counts, B, eps, hout, loc, scale, z, ws);
  if (rc == SCLDM_OK) rc = check_precision_packed(entry, h, precision);
  if (rc != SCLDM_OK) return rc;
  launch_pack(h, 0, (hipStream_t)stream_);
  return encode_impl(h, precision, counts, B, eps, hout, loc, scale, z, (char*)ws, (hipStream_t)stream_);
}

int decode_entry(const char* entry, scldm_scvi* h, const float* z, const float* library_size, int n_library, int B, float* mu, float* theta,
                 int precision, void* ws, void* stream_) {
  int rc = check_decode(entry, h, z, library_size, n_library, B, mu, theta, ws);
  if (rc == SCLDM_OK) rc = check_precision_packed(entry, h, precision);
  if (rc != SCLDM_OK) return rc;
  launch_pack(h, 0, (hipStream_t)stream_);
  return decode_impl(h, precision, z, library_size, B, mu, theta, (char*)ws, (hipStream_t)stream_);
}

int forward_entry(const char* entry, scldm_scvi* h, const float* counts, const float* library_size, int n_library, int B, const float* eps,
                  float* hout, float* loc, float* scale, float* z, float* mu, float* theta, int precision, void* ws, void* stream_) {
  int rc = check_call(entry, h, B, ws);
  if (rc != SCLDM_OK) return rc;
  if (!eps) return fail(SCLDM_ERR_SHAPE, "%s: eps is NULL (the caller draws it)", entry);
  rc = check_encode(entry, h, counts, B, eps, hout, loc, scale, z, ws);
  if (rc != SCLDM_OK) return rc;
  rc = check_decode(entry, h, z, library_size, n_library, B, mu, theta, ws);
  if (rc == SCLDM_OK) rc = check_precision_packed(entry, h, precision);
  if (rc != SCLDM_OK) return rc;
  launch_pack(h, 0, (hipStream_t)stream_);
  rc = encode_impl(h, precision, counts, B, eps, hout, loc, scale, z, (char*)ws, (hipStream_t)stream_);
  if (rc != SCLDM_OK) return rc;
  return decode_impl(h, precision, z, library_size, B, mu, theta, (char*)ws, (hipStream_t)stream_);
}
}  // namespace

// ---- the launches scvi_train_api.hip shares (scvi_handle.hpp)
namespace scldm {
namespace scvi_host {
void launch_pack(const scldm_scvi* h, int force, hipStream_t st) {
  PackArgs a;
  const int n = h->n_enc + h->n_dec;
  for (int i = 0; i < n; ++i) {
    const scldm_scvi_layer& l = i < h->n_enc ? h->enc[i] : h->dec[i - h->n_enc];
    a.layer[i] = PackLayer{l.b, l.bn_w, l.bn_b, l.bn_mean, l.bn_var};
  }
  a.n_layers = n;
  a.H = h->H;
  a.force = force;
  a.bn_eps = h->bn_eps;
  a.s = h->d_s;
  a.c = h->d_c;
  a.fp_state = h->d_fp;
  hipLaunchKernelGGL(pack_kernel, dim3(1), dim3(256), 0, st, a);
}

int launch_raw(const float* X, int K, bool log1p, const float* W, int N, int B, float* part, int precision, hipStream_t st) {
  GemmArgs a = {};
  a.X = X;
  a.W0 = W;
  a.M = B;
  a.N0 = N;
  a.K = K;
  a.out0 = part;
  if (log1p) launch_gemm<MODE_PARTIAL, true>(precision, a, st);
  else launch_gemm<MODE_PARTIAL>(precision, a, st);
  return splits_of(K);
}

int lik_head_impl(const scldm_scvi* h, const float* x, const float* library, int B, float* mu, float* theta, float* pairs, int precision,
                  hipStream_t st) {
  GemmArgs a = {};
  a.X = x;
  a.W0 = h->p.mu_w;
  a.b0 = h->p.mu_b;
  a.M = B;
  a.N0 = h->G;
  a.K = h->H;
  a.out0 = mu;
  a.pairs = pairs;
  if (h->shared_theta) {
    launch_gemm<MODE_LIK>(precision, a, st);
  } else {
    a.W1 = h->p.theta_w;
    a.b1 = h->p.theta_b;
    a.out1 = theta;
    launch_gemm<MODE_LIK2>(precision, a, st);
  }
  LAUNCH_CHECK();
  hipLaunchKernelGGL(softmax_finalize_kernel, dim3(B), dim3(256), 0, st, mu, pairs, lik_tiles(h), h->G, library,
                     h->shared_theta ? h->p.theta_w : nullptr, theta);
  LAUNCH_CHECK();
  return SCLDM_OK;
}
}  // namespace scvi_host
}  // namespace scldm

extern "C" int scldm_scvi_create(int n_enc_layers, int n_dec_layers, int n_genes, int n_hidden, int n_latent, int shared_theta,
                                 float bn_eps, scldm_scvi** out) {
  if (!out) return fail(SCLDM_ERR_SHAPE, "scldm_scvi_create: out is NULL");
  *out = nullptr;
  if (n_enc_layers < 1 || n_dec_layers < 1)
    return fail(SCLDM_ERR_SHAPE, "scldm_scvi_create: n_layers must be >= 1 (got encoder %d, decoder %d)", n_enc_layers, n_dec_layers);
  if (n_enc_layers > kScviMaxLayers || n_dec_layers > kScviMaxLayers)
    return fail(SCLDM_ERR_SHAPE, "scldm_scvi_create: at most %d layers per MLP (got encoder %d, decoder %d)", kScviMaxLayers, n_enc_layers, n_dec_layers);
  if (n_genes < 1 || n_hidden < 1 || n_latent < 1)
    return fail(SCLDM_ERR_SHAPE, "scldm_scvi_create: n_genes, n_hidden and n_latent must be positive (got %d, %d, %d)", n_genes, n_hidden, n_latent);
  if (!(bn_eps >= 0.f)) return fail(SCLDM_ERR_SHAPE, "scldm_scvi_create: the BatchNorm eps must be >= 0 (got %g)", (double)bn_eps);
  scldm_scvi* h = new (std::nothrow) scldm_scvi();
  if (!h) return fail(SCLDM_ERR_STATE, "scldm_scvi_create: out of host memory");
  h->n_enc = n_enc_layers;
  h->n_dec = n_dec_layers;
  h->G = n_genes;
  h->H = n_hidden;
  h->L = n_latent;
  h->shared_theta = shared_theta != 0;
  h->bn_eps = bn_eps;
  *out = h;
  return SCLDM_OK;
}

extern "C" void scldm_scvi_destroy(scldm_scvi* h) {
  if (!h) return;
  if (h->d_s) (void)hipFree(h->d_s);
  if (h->d_c) (void)hipFree(h->d_c);
  if (h->d_fp) (void)hipFree(h->d_fp);
  delete h;
}

extern "C" int scldm_scvi_pack(scldm_scvi* h, const scldm_scvi_params* p, void* stream_) {
  const char* entry = "scldm_scvi_pack";
  if (!h || !p) return fail(SCLDM_ERR_SHAPE, "%s: NULL argument", entry);
  if (!p->enc || !p->dec) return fail(SCLDM_ERR_SHAPE, "%s: the layer tables are NULL", entry);
  for (int side = 0; side < 2; ++side) {
    const scldm_scvi_layer* t = side ? p->dec : p->enc;
    for (int i = 0; i < (side ? h->n_dec : h->n_enc); ++i) {
      const float* q[6] = {t[i].w, t[i].b, t[i].bn_w, t[i].bn_b, t[i].bn_mean, t[i].bn_var};
      for (int k = 0; k < 6; ++k)
        if (!q[k] || misaligned(q[k], 4))
          return fail(SCLDM_ERR_SHAPE, "%s: %s layer %d has a NULL or misaligned pointer (field %d)", entry, side ? "decoder" : "encoder", i, k);
    }
  }
  CHECK_PTR(entry, p->loc_w, true);
  CHECK_PTR(entry, p->loc_b, true);
  CHECK_PTR(entry, p->scale_w, true);
  CHECK_PTR(entry, p->scale_b, true);
  CHECK_PTR(entry, p->mu_w, true);
  CHECK_PTR(entry, p->mu_b, true);
  CHECK_PTR(entry, p->theta_w, true);
  CHECK_PTR(entry, p->theta_b, !h->shared_theta);
  if (!h->d_s) {
    const size_t n = (size_t)(h->n_enc + h->n_dec) * h->H * 4;
    hipError_t e = hipMalloc((void**)&h->d_s, n);
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_c, n);
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_fp, 16);
    if (e == hipSuccess) e = hipMemsetAsync(h->d_fp, 0, 16, (hipStream_t)stream_);
    if (e != hipSuccess) {      // all three or none: a later pack starts over, and no launch ever sees a half-allocated handle
      if (h->d_s) (void)hipFree(h->d_s);
      if (h->d_c) (void)hipFree(h->d_c);
      if (h->d_fp) (void)hipFree(h->d_fp);
      h->d_s = h->d_c = nullptr;
      h->d_fp = nullptr;
      return fail(SCLDM_ERR_HIP, "%s: allocating the packed scale / shift vectors failed: %s", entry, hipGetErrorString(e));
    }
  }
  for (int i = 0; i < h->n_enc; ++i) h->enc[i] = p->enc[i];
  for (int i = 0; i < h->n_dec; ++i) h->dec[i] = p->dec[i];
  h->p = *p;
  h->p.enc = h->enc;
  h->p.dec = h->dec;
  launch_pack(h, 1, (hipStream_t)stream_);
  LAUNCH_CHECK();
  h->packed = true;
  return SCLDM_OK;
}

extern "C" size_t scldm_scvi_workspace_bytes(const scldm_scvi* h, int B) {
  if (!h || B < 1) return 0;
  return layout_of(h, B).total;
}

extern "C" int scldm_scvi_encode(scldm_scvi* h, const float* counts, int B, const float* eps, float* hout, float* loc, float* scale, float* z,
                                 void* ws, void* stream_) {
  return encode_entry("scldm_scvi_encode", h, counts, B, eps, hout, loc, scale, z, SCLDM_PREC_FP32, ws, stream_);
}
extern "C" int scldm_scvi_encode_ex(scldm_scvi* h, const float* counts, int B, const float* eps, float* hout, float* loc, float* scale,
                                    float* z, int precision, void* ws, void* stream_) {
  return encode_entry("scldm_scvi_encode_ex", h, counts, B, eps, hout, loc, scale, z, precision, ws, stream_);
}

extern "C" int scldm_scvi_decode(scldm_scvi* h, const float* z, const float* library_size, int n_library, int B, float* mu, float* theta,
                                 void* ws, void* stream_) {
  return decode_entry("scldm_scvi_decode", h, z, library_size, n_library, B, mu, theta, SCLDM_PREC_FP32, ws, stream_);
}
extern "C" int scldm_scvi_decode_ex(scldm_scvi* h, const float* z, const float* library_size, int n_library, int B, float* mu, float* theta,
                                    int precision, void* ws, void* stream_) {
  return decode_entry("scldm_scvi_decode_ex", h, z, library_size, n_library, B, mu, theta, precision, ws, stream_);
}

extern "C" int scldm_scvi_forward(scldm_scvi* h, const float* counts, const float* library_size, int n_library, int B, const float* eps,
                                  float* hout, float* loc, float* scale, float* z, float* mu, float* theta, void* ws, void* stream_) {
  return forward_entry("scldm_scvi_forward", h, counts, library_size, n_library, B, eps, hout, loc, scale, z, mu, theta, SCLDM_PREC_FP32, ws,
                       stream_);
}
extern "C" int scldm_scvi_forward_ex(scldm_scvi* h, const float* counts, const float* library_size, int n_library, int B, const float* eps,
                                     float* hout, float* loc, float* scale, float* z, float* mu, float* theta, int precision, void* ws,
                                     void* stream_) {
  return forward_entry("scldm_scvi_forward_ex", h, counts, library_size, n_library, B, eps, hout, loc, scale, z, mu, theta, precision, ws,
                       stream_);
}

// Training entries of the scVI-style baseline VAE (include/scldm_hip.h): scldm_scvi_train_record_bytes / _workspace_bytes / _forward /
// _backward, their _ex forms with a precision argument and scldm_scvi_train_set_found_inf.  A translation unit of its own: the handle, the argument checks and the three eval launches the forward reuses come from
// scvi_api.hip through scvi_handle.hpp.  Every entry checks its arguments before the first HIP call and makes launches only.
#include <hip/hip_runtime.h>

#include "scvi_handle.hpp"
#include "scvi_train.hpp"

using namespace scldm;
using namespace scldm::scvi_host;
using namespace scldm::scvi_train;

namespace {

// record: per MLP layer (encoder first) xhat (B, H), h (B, H), rstd (H); then the pre-clamp log-scale (B, L)
struct Record { size_t layer[2 * kScviMaxLayers][3], ls_pre, total; };
Record record_of(const scldm_scvi* h, int B) {
  Record r;
  size_t o = 0;
  auto take = [&](size_t bytes) { size_t q = o; o += align256(bytes); return q; };
  for (int i = 0; i < h->n_enc + h->n_dec; ++i) {
    r.layer[i][0] = take((size_t)B * h->H * 4);
    r.layer[i][1] = take((size_t)B * h->H * 4);
    r.layer[i][2] = take((size_t)h->H * 4);
  }
  r.ls_pre = take((size_t)B * h->L * 4);
  r.total = o;
  return r;
}

// workspace: the slot buffer of the split products, the softmax pairs, dlogit (and the theta logits' gradient), two (B, H) gradient
// buffers and three (B, L) ones; last, the magnitude-bit maxima of the gradient operands (fp16 backward): dlogit, the theta logits'
// gradient, dloc_t, dlog_scale, then every MLP layer's da
enum : int { SLOT_DLOGIT = 0, SLOT_DTLOGIT = 1, SLOT_DLOC = 2, SLOT_DLS = 3, SLOT_LAYER0 = 4, kSlots = SLOT_LAYER0 + 2 * kScviMaxLayers };
struct TrainLayout { size_t part, pairs, dlogit, dtlogit, d0, d1, dloc, dls, dzdec, slots, total; };
TrainLayout train_layout_of(const scldm_scvi* h, int B) {
  TrainLayout l;
  size_t o = 0;
  auto take = [&](size_t bytes) { size_t q = o; o += align256(bytes); return q; };
  const size_t BH = (size_t)B * h->H;
  const int heads = h->shared_theta ? 1 : 2;
  size_t part = 0;
  auto upd = [&](size_t floats) { if (floats > part) part = floats; };
  upd((size_t)splits_of(h->G) * BH);                      // first encoder layer; dlogit W_mu (+ dtheta_logit W_theta)
  upd((size_t)heads * splits_of(h->G) * BH);
  upd((size_t)splits_of(h->H) * B * (h->H > h->L ? h->H : h->L));
  upd((size_t)splits_of(h->L) * BH * 2);                  // dloc W_loc + dlog_scale W_scale
  upd((size_t)2 * splits_of(h->H) * B * h->L);            // the posterior head's two raw products, splits_of(H) planes each
  if (splits_of(B) > 1) {                                 // weight gradients of a batch above kScviSplit rows
    const size_t wide = h->G > h->H ? h->G : h->H;
    upd((size_t)splits_of(B) * wide * h->H);
  }
  l.part = take(part * 4);
  l.pairs = take((size_t)B * lik_tiles(h) * 2 * 4);
  l.dlogit = take((size_t)B * h->G * 4);
  l.dtlogit = take(h->shared_theta ? 0 : (size_t)B * h->G * 4);
  l.d0 = take(BH * 4);
  l.d1 = take(BH * 4);
  l.dloc = take((size_t)B * h->L * 4);
  l.dls = take((size_t)B * h->L * 4);
  l.dzdec = take((size_t)B * h->L * 4);
  l.slots = take(kSlots * sizeof(uint32_t));
  l.total = o;
  return l;
}

// The operand policy of a backward: fp32, or fp16 with the workspace's scale slots and the handle's overflow flag.  `a_slot` below
// names the slot of the product's A operand (always the gradient tensor).
struct Prec { bool f16; uint32_t* slots; float* found_inf; };
template <class P>
void launch_prod_on(const ProdArgs& a, bool at, bool log1p_b, dim3 grid, hipStream_t st) {
  if (!at) hipLaunchKernelGGL((prod_kernel<P, false, false>), grid, dim3(256), 0, st, a);
  else if (log1p_b) hipLaunchKernelGGL((prod_kernel<P, true, true>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((prod_kernel<P, true, false>), grid, dim3(256), 0, st, a);
}
// C (M, N) = A^T B (at) or A B, K split into slots slot0 ... of `dst`; returns the number of slots written
int launch_prod(const Prec& pr, int a_slot, const float* A, long long lda, bool at, const float* Bm, long long ldb, bool log1p_b, int M,
                int N, int K, float* dst, int slot0, hipStream_t st) {
  ProdArgs a;
  a.A = A;
  a.Bm = Bm;
  a.lda = lda;
  a.ldb = ldb;
  a.M = M;
  a.N = N;
  a.K = K;
  const int sp = splits_of(K);
  a.k_per_split = pr.f16 ? k_per_split<scvi::F16Operands>(K) : k_per_split<scvi::F32Operands>(K);
  a.out = dst;
  a.slot0 = slot0;
  a.a_max = pr.f16 ? pr.slots + a_slot : nullptr;
  a.found_inf = pr.found_inf;
  const dim3 grid(cdiv(N, scvi::kBN), cdiv(M, scvi::kBM), sp);
  if (pr.f16) launch_prod_on<scvi::F16Operands>(a, at, log1p_b, grid, st);
  else launch_prod_on<scvi::F32Operands>(a, at, log1p_b, grid, st);
  return sp;
}
void launch_sum(const Prec& pr, const float* part, int slots, size_t plane, float* out, hipStream_t st) {
  const dim3 grid(cdiv((long long)plane, 256));
  if (pr.f16) hipLaunchKernelGGL(sum_slots_kernel<true>, grid, dim3(256), 0, st, part, slots, plane, out, pr.found_inf);
  else hipLaunchKernelGGL(sum_slots_kernel<false>, grid, dim3(256), 0, st, part, slots, plane, out, (float*)nullptr);
}
void launch_colsum(const Prec& pr, const float* X, int B, int N, float* out, hipStream_t st) {
  const dim3 grid(cdiv(N, kColTile));
  if (pr.f16) hipLaunchKernelGGL(colsum_kernel<true>, grid, dim3(256), 0, st, X, B, N, out, pr.found_inf);
  else hipLaunchKernelGGL(colsum_kernel<false>, grid, dim3(256), 0, st, X, B, N, out, (float*)nullptr);
}
// dW (N_out, N_in) = dA (B, N_out)^T X (B, N_in), K = batch
void launch_wgrad(const Prec& pr, int a_slot, const float* dA, int n_out, const float* X, int n_in, bool log1p, int B, float* dW,
                  float* part, hipStream_t st) {
  if (splits_of(B) == 1) {
    launch_prod(pr, a_slot, dA, n_out, true, X, n_in, log1p, n_out, n_in, B, dW, 0, st);
  } else {
    const int sp = launch_prod(pr, a_slot, dA, n_out, true, X, n_in, log1p, n_out, n_in, B, part, 0, st);
    launch_sum(pr, part, sp, (size_t)n_out * n_in, dW, st);
  }
}
int check_train_precision(const char* entry, int precision) {
  if (precision != SCLDM_PREC_FP32 && precision != SCLDM_PREC_FP16)
    return fail(SCLDM_ERR_SHAPE, "%s: precision %d is not built for the scVI baseline (SCLDM_PREC_FP32 or SCLDM_PREC_FP16)", entry, precision);
  return SCLDM_OK;
}

int check_train_common(const char* entry, const scldm_scvi* h, int B, int n_library, const void* ws, float p_enc, float p_dec,
                       unsigned char* const* masks) {
  if (!h) return fail(SCLDM_ERR_SHAPE, "%s: NULL handle", entry);
  if (B < 2) return fail(SCLDM_ERR_SHAPE, "%s: BatchNorm1d in training mode needs B >= 2 (got %d)", entry, B);
  if (!ws) return fail(SCLDM_ERR_SHAPE, "%s: ws is NULL", entry);
  if (misaligned(ws, 256)) return fail(SCLDM_ERR_SHAPE, "%s: ws is not 256-byte aligned", entry);
  if (n_library != B) return fail(SCLDM_ERR_SHAPE, "%s: library_size has %d entries for %d cells", entry, n_library, B);
  if (!(p_enc >= 0.f && p_enc < 1.f) || !(p_dec >= 0.f && p_dec < 1.f))
    return fail(SCLDM_ERR_SHAPE, "%s: the dropout rates must lie in [0, 1) (got %g, %g)", entry, (double)p_enc, (double)p_dec);
  if ((p_enc > 0.f || p_dec > 0.f) && !masks) return fail(SCLDM_ERR_SHAPE, "%s: masks is NULL with a dropout rate above 0", entry);
  for (int i = 0; i < h->n_enc + h->n_dec; ++i)
    if ((i < h->n_enc ? p_enc : p_dec) > 0.f && !masks[i])
      return fail(SCLDM_ERR_SHAPE, "%s: the mask of %s layer %d is NULL", entry, i < h->n_enc ? "encoder" : "decoder", i < h->n_enc ? i : i - h->n_enc);
  return SCLDM_OK;
}
}  // namespace

extern "C" size_t scldm_scvi_train_record_bytes(const scldm_scvi* h, int B) {
  if (!h || B < 2) return 0;
  return record_of(h, B).total;
}

extern "C" size_t scldm_scvi_train_workspace_bytes(const scldm_scvi* h, int B) {
  if (!h || B < 2) return 0;
  return train_layout_of(h, B).total;
}

namespace {
// ---- the two training entries under the name of the C entry that forwards to them
int train_forward_entry(const char* entry, scldm_scvi* h, const float* counts, const float* library, int n_library, int B, const float* eps,
                        float p_enc, float p_dec, unsigned long long seed, unsigned char* const* masks, int masks_given, float momentum,
                        void* record, float* loc, float* scale, float* z, float* mu, float* theta, int precision, void* ws,
                        void* stream_) {
  int rc = check_train_common(entry, h, B, n_library, ws, p_enc, p_dec, masks);
  if (rc != SCLDM_OK) return rc;
  if (!(momentum >= 0.f && momentum <= 1.f)) return fail(SCLDM_ERR_SHAPE, "%s: momentum must lie in [0, 1] (got %g)", entry, (double)momentum);
  if (!record) return fail(SCLDM_ERR_SHAPE, "%s: record is NULL", entry);
  if (misaligned(record, 256)) return fail(SCLDM_ERR_SHAPE, "%s: record is not 256-byte aligned", entry);
  CHECK_PTR(entry, counts, true);
  CHECK_PTR(entry, library, true);
  CHECK_PTR(entry, eps, true);
  CHECK_PTR(entry, loc, true);
  CHECK_PTR(entry, scale, true);
  CHECK_PTR(entry, z, true);
  CHECK_PTR(entry, mu, true);
  CHECK_PTR(entry, theta, true);
  rc = check_train_precision(entry, precision);
  if (rc == SCLDM_OK) rc = check_packed(entry, h);
  if (rc != SCLDM_OK) return rc;
  hipStream_t st = (hipStream_t)stream_;
  const Record r = record_of(h, B);
  const TrainLayout l = train_layout_of(h, B);
  char* rec = (char*)record;
  float* part = (float*)((char*)ws + l.part);
  const int H = h->H, L = h->L;
  const float* x = counts;
  for (int i = 0; i < h->n_enc + h->n_dec; ++i) {
    const bool enc = i < h->n_enc;
    const int li = enc ? i : i - h->n_enc;
    const scldm_scvi_layer& lay = enc ? h->enc[li] : h->dec[li];
    if (i == h->n_enc) {      // posterior head between the two MLPs
      float* raw_ls = part + (size_t)splits_of(H) * B * L;       // behind the loc product's splits_of(H) planes
      const int sp = launch_raw(x, H, false, h->p.loc_w, L, B, part, precision, st);
      launch_raw(x, H, false, h->p.scale_w, L, B, raw_ls, precision, st);
      hipLaunchKernelGGL(post_forward_kernel, dim3(cdiv((long long)B * L, 256)), dim3(256), 0, st, part, raw_ls, h->p.loc_b,
                         h->p.scale_b, eps, sp, B * L, L, loc, (float*)(rec + r.ls_pre), scale, z);
      LAUNCH_CHECK();
      x = z;
    }
    const int K = li > 0 ? H : enc ? h->G : L;
    BnFwdArgs a;
    a.part = part;
    a.splits = launch_raw(x, K, i == 0, lay.w, H, B, part, precision, st);
    a.bias = lay.b;
    a.gamma = lay.bn_w;
    a.beta = lay.bn_b;
    a.run_mean = const_cast<float*>(lay.bn_mean);      // training updates the running statistics in place
    a.run_var = const_cast<float*>(lay.bn_var);
    a.momentum = momentum;
    a.eps = h->bn_eps;
    a.p = enc ? p_enc : p_dec;
    a.B = B;
    a.H = H;
    a.seed = seed;
    a.layer_tag = (uint32_t)((enc ? 0 : kScviMaxLayers) + li);
    a.mask = a.p > 0.f ? masks[i] : nullptr;
    a.draw = !masks_given;
    a.xhat = (float*)(rec + r.layer[i][0]);
    a.h = (float*)(rec + r.layer[i][1]);
    a.rstd = (float*)(rec + r.layer[i][2]);
    hipLaunchKernelGGL(bn_forward_kernel, dim3(cdiv(H, kColTile)), dim3(256), 0, st, a);
    LAUNCH_CHECK();
    x = a.h;
  }
  rc = lik_head_impl(h, x, library, B, mu, theta, (float*)((char*)ws + l.pairs), precision, st);
  if (rc != SCLDM_OK) return rc;
  launch_pack(h, 0, st);      // the fingerprint sees the new running statistics: eval calls after this step use them
  LAUNCH_CHECK();
  return SCLDM_OK;
}

int train_backward_entry(const char* entry, scldm_scvi* h, const float* counts, const float* library, int n_library, int B,
                         const float* eps, float p_enc, float p_dec, unsigned char* const* masks, const void* record, const float* scale,
                         const float* z, const float* mu, const float* theta, const float* dmu, const float* dtheta, const float* dloc,
                         const float* dscale, const float* dz, const scldm_scvi_grads* grads, int precision, void* ws, void* stream_) {
  int rc = check_train_common(entry, h, B, n_library, ws, p_enc, p_dec, masks);
  if (rc != SCLDM_OK) return rc;
  if (!record) return fail(SCLDM_ERR_SHAPE, "%s: record is NULL", entry);
  if (misaligned(record, 256)) return fail(SCLDM_ERR_SHAPE, "%s: record is not 256-byte aligned", entry);
  CHECK_PTR(entry, counts, true);
  CHECK_PTR(entry, library, true);
  CHECK_PTR(entry, eps, true);
  CHECK_PTR(entry, scale, true);
  CHECK_PTR(entry, z, true);
  CHECK_PTR(entry, mu, true);
  CHECK_PTR(entry, theta, true);
  CHECK_PTR(entry, dmu, false);
  CHECK_PTR(entry, dtheta, false);
  CHECK_PTR(entry, dloc, false);
  CHECK_PTR(entry, dscale, false);
  CHECK_PTR(entry, dz, false);
  if (!grads) return fail(SCLDM_ERR_SHAPE, "%s: grads is NULL", entry);
  if (!grads->enc || !grads->dec) return fail(SCLDM_ERR_SHAPE, "%s: the gradient layer tables are NULL", entry);
  for (int side = 0; side < 2; ++side) {
    const scldm_scvi_layer_grads* t = side ? grads->dec : grads->enc;
    for (int i = 0; i < (side ? h->n_dec : h->n_enc); ++i) {
      const float* q[4] = {t[i].dw, t[i].db, t[i].dgamma, t[i].dbeta};
      for (int k = 0; k < 4; ++k)
        if (!q[k] || misaligned(q[k], 4))
          return fail(SCLDM_ERR_SHAPE, "%s: %s layer %d has a NULL or misaligned gradient pointer (field %d)", entry, side ? "decoder" : "encoder", i, k);
    }
  }
  CHECK_PTR(entry, grads->loc_w, true);
  CHECK_PTR(entry, grads->loc_b, true);
  CHECK_PTR(entry, grads->scale_w, true);
  CHECK_PTR(entry, grads->scale_b, true);
  CHECK_PTR(entry, grads->mu_w, true);
  CHECK_PTR(entry, grads->mu_b, true);
  CHECK_PTR(entry, grads->theta_w, true);
  CHECK_PTR(entry, grads->theta_b, !h->shared_theta);
  rc = check_train_precision(entry, precision);
  if (rc == SCLDM_OK) rc = check_packed(entry, h);
  if (rc != SCLDM_OK) return rc;
  hipStream_t st = (hipStream_t)stream_;
  const Record r = record_of(h, B);
  const TrainLayout l = train_layout_of(h, B);
  const char* rec = (const char*)record;
  char* w = (char*)ws;
  float* part = (float*)(w + l.part);
  float* dlogit = (float*)(w + l.dlogit);
  float* dtlogit = (float*)(w + l.dtlogit);
  float* d[2] = {(float*)(w + l.d0), (float*)(w + l.d1)};
  float *dloc_t = (float*)(w + l.dloc), *dls = (float*)(w + l.dls), *dzdec = (float*)(w + l.dzdec);
  const int G = h->G, H = h->H, L = h->L, n_all = h->n_enc + h->n_dec;
  const size_t BH = (size_t)B * H;
  auto rec_h = [&](int i) { return (const float*)(rec + r.layer[i][1]); };
  int cur = 0;
  const Prec pr = {precision == SCLDM_PREC_FP16, (uint32_t*)(w + l.slots), precision == SCLDM_PREC_FP16 ? h->found_inf : nullptr};
  if (pr.f16) {      // the maxima start at zero, the overflow flag at 0.0
    HIP_TRY(hipMemsetAsync(pr.slots, 0, kSlots * sizeof(uint32_t), st));
    if (pr.found_inf) HIP_TRY(hipMemsetAsync(pr.found_inf, 0, sizeof(float), st));
  }

  // ---- likelihood head: dlogit (and the theta logits' gradient), the head's weights and biases, dg into d[cur]
  const float* g_dec = rec_h(n_all - 1);
  if (pr.f16)
    hipLaunchKernelGGL(lik_backward_kernel<true>, dim3(B), dim3(256), 0, st, mu, theta, dmu, dtheta, library, G, h->shared_theta,
                       h->p.theta_w, dlogit, dtlogit, grads->theta_w, pr.slots + SLOT_DLOGIT, pr.slots + SLOT_DTLOGIT, pr.found_inf);
  else
    hipLaunchKernelGGL(lik_backward_kernel<false>, dim3(B), dim3(256), 0, st, mu, theta, dmu, dtheta, library, G, h->shared_theta,
                       h->p.theta_w, dlogit, dtlogit, grads->theta_w, (uint32_t*)nullptr, (uint32_t*)nullptr, (float*)nullptr);
  LAUNCH_CHECK();
  launch_wgrad(pr, SLOT_DLOGIT, dlogit, G, g_dec, H, false, B, grads->mu_w, part, st);
  launch_colsum(pr, dlogit, B, G, grads->mu_b, st);
  if (!h->shared_theta) {
    launch_wgrad(pr, SLOT_DTLOGIT, dtlogit, G, g_dec, H, false, B, grads->theta_w, part, st);
    launch_colsum(pr, dtlogit, B, G, grads->theta_b, st);
  }
  LAUNCH_CHECK();
  {
    int slots = launch_prod(pr, SLOT_DLOGIT, dlogit, G, false, h->p.mu_w, H, false, B, H, G, part, 0, st);
    if (!h->shared_theta) slots += launch_prod(pr, SLOT_DTLOGIT, dtlogit, G, false, h->p.theta_w, H, false, B, H, G, part, slots, st);
    launch_sum(pr, part, slots, BH, d[cur], st);
    LAUNCH_CHECK();
  }

  // ---- the two MLPs, last layer first, with the posterior head between them
  for (int i = n_all - 1; i >= 0; --i) {
    const bool enc = i < h->n_enc;
    const int li = enc ? i : i - h->n_enc;
    const scldm_scvi_layer& lay = enc ? h->enc[li] : h->dec[li];
    const scldm_scvi_layer_grads& gl = enc ? grads->enc[li] : grads->dec[li];
    BnBwdArgs a;
    a.d = d[cur];
    a.xhat = (const float*)(rec + r.layer[i][0]);
    a.rstd = (const float*)(rec + r.layer[i][2]);
    a.gamma = lay.bn_w;
    a.beta = lay.bn_b;
    a.p = enc ? p_enc : p_dec;
    a.mask = a.p > 0.f ? masks[i] : nullptr;
    a.B = B;
    a.H = H;
    a.dgamma = gl.dgamma;
    a.dbeta = gl.dbeta;
    a.dbias = gl.db;
    a.da_max = pr.f16 ? pr.slots + SLOT_LAYER0 + i : nullptr;
    a.found_inf = pr.found_inf;
    if (pr.f16) hipLaunchKernelGGL(bn_backward_kernel<true>, dim3(cdiv(H, kColTile)), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(bn_backward_kernel<false>, dim3(cdiv(H, kColTile)), dim3(256), 0, st, a);
    LAUNCH_CHECK();
    const int K = li > 0 ? H : enc ? G : L;                       // the layer's input width
    const float* xin = li > 0 ? rec_h(i - 1) : enc ? counts : z;
    launch_wgrad(pr, SLOT_LAYER0 + i, d[cur], H, xin, K, i == 0, B, gl.dw, part, st);   // the first encoder layer stages log1p(counts)
    LAUNCH_CHECK();
    if (i == 0) break;                                            // no gradient with respect to counts
    // dx (B, K) = da W
    float* dx = li > 0 ? d[cur ^ 1] : dzdec;
    const int sp = splits_of(H);
    if (sp == 1) {
      launch_prod(pr, SLOT_LAYER0 + i, d[cur], H, false, lay.w, K, false, B, K, H, dx, 0, st);
    } else {
      launch_prod(pr, SLOT_LAYER0 + i, d[cur], H, false, lay.w, K, false, B, K, H, part, 0, st);
      launch_sum(pr, part, sp, (size_t)B * K, dx, st);
    }
    LAUNCH_CHECK();
    if (li > 0) { cur ^= 1; continue; }
    // ---- posterior head (i is the first decoder layer): dloc_t, dlog_scale, the four head gradients, dh into d[cur]
    const float* h_enc = rec_h(h->n_enc - 1);
    if (pr.f16)
      hipLaunchKernelGGL(post_backward_kernel<true>, dim3(cdiv((long long)B * L, 256)), dim3(256), 0, st, dz, dzdec, dloc, dscale, eps,
                         scale, (const float*)(rec + r.ls_pre), B * L, dloc_t, dls, pr.slots + SLOT_DLOC, pr.slots + SLOT_DLS, pr.found_inf);
    else
      hipLaunchKernelGGL(post_backward_kernel<false>, dim3(cdiv((long long)B * L, 256)), dim3(256), 0, st, dz, dzdec, dloc, dscale, eps,
                         scale, (const float*)(rec + r.ls_pre), B * L, dloc_t, dls, (uint32_t*)nullptr, (uint32_t*)nullptr, (float*)nullptr);
    LAUNCH_CHECK();
    launch_wgrad(pr, SLOT_DLOC, dloc_t, L, h_enc, H, false, B, grads->loc_w, part, st);
    launch_wgrad(pr, SLOT_DLS, dls, L, h_enc, H, false, B, grads->scale_w, part, st);
    launch_colsum(pr, dloc_t, B, L, grads->loc_b, st);
    launch_colsum(pr, dls, B, L, grads->scale_b, st);
    LAUNCH_CHECK();
    int slots = launch_prod(pr, SLOT_DLOC, dloc_t, L, false, h->p.loc_w, H, false, B, H, L, part, 0, st);
    slots += launch_prod(pr, SLOT_DLS, dls, L, false, h->p.scale_w, H, false, B, H, L, part, slots, st);
    launch_sum(pr, part, slots, BH, d[cur], st);
    LAUNCH_CHECK();
  }
  return SCLDM_OK;
}
}  // namespace

extern "C" int scldm_scvi_train_forward(scldm_scvi* h, const float* counts, const float* library, int n_library, int B, const float* eps,
                                        float p_enc, float p_dec, unsigned long long seed, unsigned char* const* masks, int masks_given,
                                        float momentum, void* record, float* loc, float* scale, float* z, float* mu, float* theta,
                                        void* ws, void* stream) {
  return train_forward_entry("scldm_scvi_train_forward", h, counts, library, n_library, B, eps, p_enc, p_dec, seed, masks, masks_given,
                             momentum, record, loc, scale, z, mu, theta, SCLDM_PREC_FP32, ws, stream);
}
extern "C" int scldm_scvi_train_forward_ex(scldm_scvi* h, const float* counts, const float* library, int n_library, int B, const float* eps,
                                           float p_enc, float p_dec, unsigned long long seed, unsigned char* const* masks, int masks_given,
                                           float momentum, void* record, float* loc, float* scale, float* z, float* mu, float* theta,
                                           int precision, void* ws, void* stream) {
  return train_forward_entry("scldm_scvi_train_forward_ex", h, counts, library, n_library, B, eps, p_enc, p_dec, seed, masks, masks_given,
                             momentum, record, loc, scale, z, mu, theta, precision, ws, stream);
}

extern "C" int scldm_scvi_train_backward(scldm_scvi* h, const float* counts, const float* library, int n_library, int B, const float* eps,
                                         float p_enc, float p_dec, unsigned char* const* masks, const void* record, const float* scale,
                                         const float* z, const float* mu, const float* theta, const float* dmu, const float* dtheta,
                                         const float* dloc, const float* dscale, const float* dz, const scldm_scvi_grads* grads, void* ws,
                                         void* stream) {
  return train_backward_entry("scldm_scvi_train_backward", h, counts, library, n_library, B, eps, p_enc, p_dec, masks, record, scale, z,
                              mu, theta, dmu, dtheta, dloc, dscale, dz, grads, SCLDM_PREC_FP32, ws, stream);
}
extern "C" int scldm_scvi_train_backward_ex(scldm_scvi* h, const float* counts, const float* library, int n_library, int B,
                                            const float* eps, float p_enc, float p_dec, unsigned char* const* masks, const void* record,
                                            const float* scale, const float* z, const float* mu, const float* theta, const float* dmu,
                                            const float* dtheta, const float* dloc, const float* dscale, const float* dz,
                                            const scldm_scvi_grads* grads, int precision, void* ws, void* stream) {
  return train_backward_entry("scldm_scvi_train_backward_ex", h, counts, library, n_library, B, eps, p_enc, p_dec, masks, record, scale, z,
                              mu, theta, dmu, dtheta, dloc, dscale, dz, grads, precision, ws, stream);
}

extern "C" int scldm_scvi_train_set_found_inf(scldm_scvi* h, float* found_inf) {
  if (!h) return fail(SCLDM_ERR_SHAPE, "scldm_scvi_train_set_found_inf: NULL handle");
  if (found_inf && misaligned(found_inf, 4)) return fail(SCLDM_ERR_SHAPE, "scldm_scvi_train_set_found_inf: found_inf is not 4-byte aligned");
  h->found_inf = found_inf;
  return SCLDM_OK;
}

// C ABI of the TransformerVAE training step (scldm_vae_train_*, scldm_vae_train_gaussian_*, scldm_nb_loglik*; see include/scldm_hip.h): host-side
// sequencing of the kernels in vae_train.hpp and vae_train_wide.hpp.  The forward is the inference path (mcab.hpp) with two extra outputs; the backward
// reads the parameters LIVE from the caller's tensors (PyTorch layouts) and writes every gradient in the same layout.
#include <algorithm>
#include <atomic>
#include <vector>

#include "vae_handle.hpp"
#include "vae_train_wide.hpp"

using namespace scldm;
using namespace scldm::vtrain;

namespace {

struct Carver {
  char* base;
  size_t off = 0;
  float* take(size_t floats) {
    float* p = base ? reinterpret_cast<float*>(base + off) : nullptr;
    off += align256(floats * sizeof(float));
    return p;
  }
};

// tiles of 64 tokens per workgroup / workgroups per cell of the two gene-axis kernels: about `wgs` workgroups in flight, so that
// one partial per workgroup stays small next to the work it summarises
void split_tiles(int n_tok, int B, int* tiles, int* chunks, int wgs) {
  const int per_cell = cdiv(n_tok, 64);
  const int want = std::max(1, std::min(per_cell, wgs / std::max(B, 1)));
  *tiles = cdiv(per_cell, want);
  *chunks = cdiv(per_cell, *tiles);
}

// the split of both kernels at batch B, S encoder tokens and G decoded genes: what carve_ws launches with and scldm_vae_train_split
// reports (the workgroups are four waves, two per CU: one full round of 512 measured best at batch 32 - per-gene kernel
// 606 us against 633-645 us with 1 024-4 096 workgroups, pooling 123 us against 130-138 us - and equal at batch 512;
// SCLDM_VAE_GENE_WGS / SCLDM_VAE_POOL_WGS override the target counts)
struct Split { int tilesD, chunksD, tilesE, chunksE; };
Split train_split(int B, int S, int G) {
  static const int wgs_d = [] { const char* e = getenv("SCLDM_VAE_GENE_WGS"); return e ? atoi(e) : 512; }();
  static const int wgs_e = [] { const char* e = getenv("SCLDM_VAE_POOL_WGS"); return e ? atoi(e) : 512; }();
  Split s;
  split_tiles(G, B, &s.tilesD, &s.chunksD, wgs_d);
  split_tiles(S, B, &s.tilesE, &s.chunksE, wgs_e);
  return s;
}

struct Saved { float *pooled, *lse2, *kv; size_t bytes; };
Saved carve_saved(int B, void* base) {
  Carver c{reinterpret_cast<char*>(base)};
  Saved s;
  s.pooled = c.take((size_t)B * kT * 32);
  s.lse2 = c.take((size_t)B * 64);
  s.kv = c.take((size_t)B * kT * 64);   // K | V of the cells' latent tokens (the decode's plain (B, 16, 64) copy), for the per-gene backward
  s.bytes = c.off;
  return s;
}

// the NB training entries refuse a handle that holds the Gaussian head, and the Gaussian ones an NB handle: the head's LayerNorm
// makes d(y + mlp) rank two per gene, which is a per-gene kernel of its own (wide::dec_gene_bwd_gauss_kernel)
const char* const kGaussNoTrain = "this entry trains the negative-binomial head; this handle holds a Gaussian head "
                                  "(GaussianTransformerLayer): use scldm_vae_train_gaussian_forward / _gaussian_backward";
const char* const kNbNoGaussTrain = "this entry trains the Gaussian head (GaussianTransformerLayer); this handle holds a negative-binomial "
                                    "head (NegativeBinomialTransformerLayer): use scldm_vae_train_forward / _backward";

// precision of a training step: fp32 (exact), or fp16 (fp16 operands of the per-gene MCAB contractions, forward and backward)
int check_train_precision(int precision) {
  if (precision != SCLDM_PREC_FP32 && precision != SCLDM_PREC_FP16)
    return fail(SCLDM_ERR_SHAPE, "unsupported VAE training precision %d (SCLDM_PREC_FP32 or SCLDM_PREC_FP16)", precision);
  return SCLDM_OK;
}

// the NB head without a theta table (decoder_head.params is Linear(32, 2), theta = exp of its second output): routed on the handle,
// as decode does
bool unshared_theta(const scldm_vae* h) { return h->loaded && !h->gaussian && !h->theta; }

struct Ws {
  float *wct, *Q, *dQ, *xs_enc, *xs_dec, *ysave, *kv, *dl, *dz_dec, *dao, *dgq, *bsum, *p_gene, *p_dkv, *p_dcell, *p_ecell, *p_pool, *dl_scale, *dl2;
  int tilesD, chunksD, tilesE, chunksE;
  size_t bytes;
};
Ws carve_ws(const scldm_vae* h, int B, int S, int G, void* base) {
  const scldm_vae_config& c = h->cfg;
  const int L = c.n_layer;
  Carver k{reinterpret_cast<char*>(base)};
  Ws w;
  const Split sp = train_split(B, S, G);
  w.tilesD = sp.tilesD; w.chunksD = sp.chunksD; w.tilesE = sp.tilesE; w.chunksE = sp.chunksE;
  w.wct = k.take((size_t)(2 + 2 * L) * kHP * 32);
  w.Q = k.take(512);
  w.dQ = k.take(512);
  w.xs_enc = k.take((size_t)B * (L + 1) * kT * 32);
  w.xs_dec = k.take((size_t)B * (L + 1) * kT * 32);
  w.ysave = k.take((size_t)B * kT * 32);
  w.kv = k.take((size_t)B * kT * 64);
  w.dl = k.take((size_t)B * G);
  w.dz_dec = k.take((size_t)B * kT * c.n_embed_latent);
  w.dao = k.take((size_t)B * kT * 32);
  w.dgq = k.take((size_t)B * 64);
  w.bsum = k.take((size_t)B);
  const bool nb2 = unshared_theta(h);
  w.p_gene = k.take((size_t)B * w.chunksD * (h->gaussian ? GP_SIZE : nb2 ? NP_SIZE : DP_SIZE));   // (the Gaussian / unshared partials carry the head rows)
  w.p_dkv = k.take((size_t)B * w.chunksD * kT * 64);
  w.p_dcell = k.take((size_t)B * dc_size(L));      // cell-side partials: one per cell
  w.p_ecell = k.take((size_t)B * ec_size(L));
  w.p_pool = k.take((size_t)B * w.chunksE * EP_SIZE);
  w.dl_scale = k.take((size_t)B);      // fp16: per-cell power of two of dl (head_bwd_kernel<true>)
  w.dl2 = k.take(nb2 ? (size_t)B * G : 0);      // unshared theta: d loss / d l1 per slot
  w.bytes = k.off;
  return w;
}

int check_train(const scldm_vae* h, const scldm_vae_weights* w, int B, int S, int G) {
  if (!h || !w) return fail(SCLDM_ERR_SHAPE, "null argument");
  if (!h->loaded) return fail(SCLDM_ERR_STATE, "scldm_vae_load_weights has not been called");
  if (B < 1 || S < 1 || G < 1) return fail(SCLDM_ERR_SHAPE, "need B, S, G >= 1 (got %d, %d, %d)", B, S, G);
  if (h->cfg.n_layer > 16) return fail(SCLDM_ERR_SHAPE, "the VAE training kernels take at most 16 trunk layers per side (got %d)", h->cfg.n_layer);
  if (h->cfg.hidden_dim > kHP) return fail(SCLDM_ERR_SHAPE, "SwiGLU hidden width %d exceeds %d", h->cfg.hidden_dim, kHP);
  if (B > 65535) return fail(SCLDM_ERR_SHAPE, "batch too large for one launch (%d)", B);
  return SCLDM_OK;
}

// row buffers of the ordered table gradients: the decoder slots' then the encoder tokens' 32-float gene-embedding contributions
// (contiguous: entry e of the caller's index is row e), then one theta contribution per decoder slot
struct Rows { float *emb, *theta; size_t bytes; };
Rows carve_rows(int B, int S, int G, void* base) {
  Carver c{reinterpret_cast<char*>(base)};
  Rows r;
  r.emb = c.take(((size_t)B * G + (size_t)B * S) * 32);
  r.theta = c.take((size_t)B * G);
  r.bytes = c.off;
  return r;
}

MlpW mlp_of(const float* w1, const float* w2, const float* wct, int H) { return MlpW{w1, w2, wct, H}; }

BlockWArr blocks_of(const scldm_vae_block* b, int L, const float* wct0, int H) {
  BlockWArr a{};
  for (int l = 0; l < L; ++l) {
    a.b[l].ln1_w = b[l].ln1_w; a.b[l].ln1_b = b[l].ln1_b; a.b[l].wqkv = b[l].attn_w; a.b[l].wp = b[l].proj_w;
    a.b[l].ln2_w = b[l].ln2_w; a.b[l].ln2_b = b[l].ln2_b;
    a.b[l].mlp = mlp_of(b[l].w1, b[l].w2, wct0 + (size_t)l * kHP * 32, H);
  }
  return a;
}

// reduction jobs of one partial array (launched in groups of at most kMaxRedJobs)
struct Jobs {
  std::vector<RedJob> v;
  void vec(float* dst, int off, int n, bool acc = false) { if (dst) v.push_back(RedJob{dst, off, n, acc ? 1 : 0, 1, 0, 0}); }
  void mat(float* dst, int off, int rows, int cols, int ld_src, int ld_dst, bool acc = false) {
    if (dst) v.push_back(RedJob{dst, off, cols, acc ? 1 : 0, rows, ld_src, ld_dst});
  }
  int run(const float* part, int n_part, long stride, hipStream_t st) {
    for (size_t i = 0; i < v.size(); i += kMaxRedJobs) {
      RedArgs a{};
      a.part = part; a.n_part = n_part; a.stride = stride;
      a.n_jobs = (int)std::min<size_t>(kMaxRedJobs, v.size() - i);
      for (int j = 0; j < a.n_jobs; ++j) a.job[j] = v[i + j];
      reduce_jobs_kernel<<<dim3(12, a.n_jobs), 256, 0, st>>>(a);   // (3 072 threads per job: one element each for the largest blocks)
      LAUNCH_CHECK();
    }
    return SCLDM_OK;
  }
};

// gradient pointer of a trunk layer's tensors, in the partial layout of block_bwd
void trunk_jobs(Jobs& j, const scldm_vae_block& g, int off0, int H) {
  j.mat(const_cast<float*>(g.attn_w), off0 + TP_WQKV, 96, 32, 32, 32);
  j.mat(const_cast<float*>(g.proj_w), off0 + TP_WP, 32, 32, 32, 32);
  j.mat(const_cast<float*>(g.w1), off0 + TP_W1, H, 32, 32, 32);
  j.mat(const_cast<float*>(g.w2), off0 + TP_W2, H, 32, 32, 32);
  j.mat(const_cast<float*>(g.cproj), off0 + TP_WC, 32, H, kHP, H);
  j.vec(const_cast<float*>(g.ln1_w), off0 + TP_LN1W, 32);
  j.vec(const_cast<float*>(g.ln1_b), off0 + TP_LN1B, 32);
  j.vec(const_cast<float*>(g.ln2_w), off0 + TP_LN2W, 32);
  j.vec(const_cast<float*>(g.ln2_b), off0 + TP_LN2B, 32);
}

}  // namespace

extern "C" size_t scldm_vae_train_saved_bytes(const scldm_vae* h, int B) {
  if (!h || B < 1) return 0;
  return carve_saved(B, nullptr).bytes;
}
extern "C" size_t scldm_vae_train_workspace_bytes(const scldm_vae* h, int B, int S, int G) {
  if (!h || B < 1 || S < 1 || G < 1) return 0;
  // the forward borrows the inference workspace layout; the backward carves its own
  return std::max(carve_ws(h, B, S, G, nullptr).bytes, scldm_vae_workspace_bytes(h, B, G));
}

extern "C" int scldm_vae_train_split(int B, int S, int G, int out[4]) {
  if (B < 1 || S < 1 || G < 1) return fail(SCLDM_ERR_SHAPE, "need B, S, G >= 1 (got %d, %d, %d)", B, S, G);
  if (!out) return fail(SCLDM_ERR_SHAPE, "scldm_vae_train_split: null output");
  const Split s = train_split(B, S, G);
  out[0] = s.tilesD; out[1] = s.chunksD; out[2] = s.tilesE; out[3] = s.chunksE;
  return SCLDM_OK;
}

extern "C" int scldm_vae_train_set_found_inf(scldm_vae* h, float* found_inf) {
  if (!h) return fail(SCLDM_ERR_SHAPE, "scldm_vae_train_set_found_inf: null handle");
  if (h->gaussian) return fail(SCLDM_ERR_SHAPE, "%s", kGaussNoTrain);
  h->found_inf = found_inf;
  return SCLDM_OK;
}

extern "C" int scldm_vae_train_forward_ex(scldm_vae* h, const float* counts_subset, const int64_t* genes_subset, int B, int S,
                                          const int64_t* genes, const float* library_size, int G, float* mu, float* theta, float* z,
                                          void* saved_, void* ws, int precision, void* stream_) {
  int rc = check_train_precision(precision);
  if (rc) return rc;
  if (!h || !counts_subset || !genes_subset || !genes || !library_size || !mu || !theta || !z || !saved_ || !ws)
    return fail(SCLDM_ERR_SHAPE, "null argument");
  if (B < 1 || S < 1 || G < 1) return fail(SCLDM_ERR_SHAPE, "need B, S, G >= 1");
  if (h->gaussian) return fail(SCLDM_ERR_SHAPE, "%s", kGaussNoTrain);
  hipStream_t st = (hipStream_t)stream_;
  Saved s = carve_saved(B, saved_);
  if (precision == SCLDM_PREC_FP16) {
    // fp16 operands in the per-token / per-gene MCAB kernels (pooling, per-gene decoder); the two 16-token trunks stay exact fp32, so
    // the backward's fp32 recompute of them reproduces the forward.  `saved` receives the cells' plain K | V directly.
    rc = scldm_vae_encode_ex(h, counts_subset, genes_subset, B, S, z, SCLDM_PREC_FP16, s.pooled, s.lse2, st, SCLDM_PREC_FP32);
    if (rc) return rc;
    return scldm_vae_decode_train_fp16(h, z, genes, library_size, B, G, mu, theta, s.kv, ws, st);
  }
  rc = scldm_vae_encode_ex(h, counts_subset, genes_subset, B, S, z, SCLDM_PREC_FP32, s.pooled, s.lse2, st);
  if (rc) return rc;
  rc = scldm_vae_decode(h, z, genes, library_size, B, G, mu, theta, SCLDM_PREC_FP32, ws, stream_);
  if (rc) return rc;
  // the decode's fp32 route leaves the cells' plain K | V at the start of its workspace (vae_api.hip: vae_decode_impl): keep a copy in
  // `saved` so that the per-gene backward does not wait for the recompute forward (4 KB per cell)
  HIP_TRY(hipMemcpyAsync(s.kv, ws, (size_t)B * kT * 64 * sizeof(float), hipMemcpyDeviceToDevice, st));
  return SCLDM_OK;
}

extern "C" int scldm_vae_train_forward(scldm_vae* h, const float* counts_subset, const int64_t* genes_subset, int B, int S,
                                       const int64_t* genes, const float* library_size, int G, float* mu, float* theta, float* z,
                                       void* saved_, void* ws, void* stream_) {
  return scldm_vae_train_forward_ex(h, counts_subset, genes_subset, B, S, genes, library_size, G, mu, theta, z, saved_, ws,
                                    SCLDM_PREC_FP32, stream_);
}

// Gaussian head: the inference path (the per-gene kernel writes mu itself, no finalize pass) and the same `saved` as the NB forward
extern "C" int scldm_vae_train_gaussian_forward(scldm_vae* h, const float* counts_subset, const int64_t* genes_subset, int B, int S,
                                                const int64_t* genes, int G, float* mu, float* z, void* saved_, void* ws, void* stream_) {
  if (!h || !counts_subset || !genes_subset || !genes || !mu || !z || !saved_ || !ws) return fail(SCLDM_ERR_SHAPE, "null argument");
  if (B < 1 || S < 1 || G < 1) return fail(SCLDM_ERR_SHAPE, "need B, S, G >= 1");
  if (!h->gaussian) return fail(SCLDM_ERR_SHAPE, "%s", kNbNoGaussTrain);
  hipStream_t st = (hipStream_t)stream_;
  Saved s = carve_saved(B, saved_);
  int rc = scldm_vae_encode_ex(h, counts_subset, genes_subset, B, S, z, SCLDM_PREC_FP32, s.pooled, s.lse2, st);
  if (rc) return rc;
  rc = scldm_vae_decode_gaussian(h, z, genes, B, G, mu, SCLDM_PREC_FP32, ws, stream_);
  if (rc) return rc;
  // (the fp32 decode leaves the cells' plain K | V at the start of its workspace, as scldm_vae_decode does)
  HIP_TRY(hipMemcpyAsync(s.kv, ws, (size_t)B * kT * 64 * sizeof(float), hipMemcpyDeviceToDevice, st));
  return SCLDM_OK;
}

namespace {
// the backward of both table-gradient modes: atomic (rows_ == nullptr; scldm_vae_train_backward_ex) or ordered
int train_backward_impl(scldm_vae* h, const scldm_vae_weights* w, const scldm_vae_weights* g, const float* counts_subset,
                        const int64_t* genes_subset, int B, int S, const int64_t* genes, const float* library_size, int G, const float* mu,
                        const float* theta, const float* z, const float* dmu, const float* dtheta, const float* dz, void* saved_, void* ws_,
                        int precision, const int32_t* order, const int32_t* seg, int n_entries, void* rows_, void* stream_,
                        bool gauss = false) {
  // gauss: the Gaussian head (scldm_vae_train_gaussian_backward) - library_size, theta, dtheta are NULL and unused, fp32 only
  int rc = check_train_precision(precision);
  if (rc) return rc;
  if (h && h->gaussian != gauss) return fail(SCLDM_ERR_SHAPE, "%s", gauss ? kNbNoGaussTrain : kGaussNoTrain);
  rc = check_train(h, w, B, S, G);
  if (rc) return rc;
  const bool f16 = precision == SCLDM_PREC_FP16;
  const bool nb2 = unshared_theta(h);      // (check_train: the handle is loaded)
  if (!g || !counts_subset || !genes_subset || !genes || !mu || !z || !saved_ || !ws_ || (!gauss && (!library_size || !theta)))
    return fail(SCLDM_ERR_SHAPE, "null argument");
  if (gauss) {
    if (!g->gene_embedding) return fail(SCLDM_ERR_SHAPE, "the gene_embedding gradient table is required");
    if (!w->head_ln_w || !w->head_ln_b || !w->head_w) return fail(SCLDM_ERR_SHAPE, "Gaussian head: head_ln_w, head_ln_b and head_w are required");
  } else if (nb2) {
    if (!g->gene_embedding) return fail(SCLDM_ERR_SHAPE, "the gene_embedding gradient table is required");
    if (!w->head_w || !g->head_w || !g->head_b)
      return fail(SCLDM_ERR_SHAPE, "unshared-theta head: head_w (2, 32) and the head_w / head_b (2) gradients are required");
  } else if (!g->gene_embedding || !g->theta) return fail(SCLDM_ERR_SHAPE, "the gene_embedding and theta gradient tables are required");
  hipStream_t st = (hipStream_t)stream_;
  const scldm_vae_config& c = h->cfg;
  const int L = c.n_layer, H = c.hidden_dim, nl = c.n_embed_latent;
  const float eps = c.layernorm_eps;
  Saved sv = carve_saved(B, saved_);
  Ws k = carve_ws(h, B, S, G, ws_);
  float* g_emb = const_cast<float*>(g->gene_embedding);
  float* g_theta = const_cast<float*>(g->theta);
  const bool ordered = rows_ != nullptr;
  const Rows rw = carve_rows(B, S, G, rows_);
  if (!ordered) {   // (the ordered reduction writes every table row, the untouched ones as zeros)
    HIP_TRY(hipMemsetAsync(g_emb, 0, (size_t)(c.n_genes + 1) * 32 * 4, st));
    if (!gauss && !nb2) HIP_TRY(hipMemsetAsync(g_theta, 0, (size_t)(c.n_genes + 1) * 4, st));
  }
  if (f16 && h->found_inf) HIP_TRY(hipMemsetAsync(h->found_inf, 0, sizeof(float), st));

  // ---- transposed c_proj copies (the streaming SwiGLU reads columns of c_proj as rows): enc cross, dec cross, enc layers, dec layers
  auto wct = [&](int i) { return k.wct + (size_t)i * kHP * 32; };
  {
    TransposeJobs tj{};     // slots: enc cross, dec cross, enc layers, dec layers (one launch)
    tj.src[0] = w->enc_cross.cproj;
    tj.src[1] = w->dec_cross.cproj;
    for (int l = 0; l < L; ++l) { tj.src[2 + l] = w->enc_blocks[l].cproj; tj.src[2 + L + l] = w->dec_blocks[l].cproj; }
    transpose_many_kernel<<<dim3(cdiv(32 * H, 256), 2 + 2 * L), 256, 0, st>>>(tj, 32, H, k.wct, (long)kHP * 32);
    enc_q_fwd_kernel<<<1, 64, 0, st>>>(w->inducing_points, w->enc_cross.ln1q_w, w->enc_cross.ln1q_b, w->enc_cross.attn_q, eps, k.Q);
    LAUNCH_CHECK();
  }
  // ---- recompute the 16-token sides with saved layer inputs
  EncCellTrainArgs ea{};
  ea.pooled = sv.pooled; ea.ind = w->inducing_points; ea.wp = w->enc_cross.attn_proj; ea.cln2_w = w->enc_cross.ln2_w; ea.cln2_b = w->enc_cross.ln2_b;
  ea.cmlp = mlp_of(w->enc_cross.w1, w->enc_cross.w2, wct(0), H);
  ea.pos = c.positional_encoding ? w->enc_pos_embed : nullptr;
  ea.blocks = blocks_of(w->enc_blocks, L, wct(2), H);
  ea.w_lat = w->enc_latent_w; ea.xsave = k.xs_enc; ea.ysave = k.ysave;
  ea.dz_a = k.dz_dec; ea.dz_b = dz; ea.dao = k.dao; ea.dgq = k.dgq; ea.part = k.p_ecell;
  ea.B = B; ea.n_lat = nl; ea.n_layer = L; ea.eps = eps;
  {   // (the attribute is per device: a process that drives several GPUs sets it on each)
    static std::atomic<bool> attr_set[64];
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64 || !attr_set[dev].load(std::memory_order_acquire)) {
      for (const void* f : {(const void*)wide::enc_cell_fwd_kernel, (const void*)wide::enc_cell_bwd_kernel, (const void*)wide::dec_cell_fwd_kernel,
                            (const void*)wide::dec_cell_bwd_kernel})
        HIP_TRY(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, wide::LDS_BYTES));
      HIP_TRY(hipFuncSetAttribute((const void*)wide::enc_pool_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, wide::PB_BYTES));
      HIP_TRY(hipFuncSetAttribute((const void*)wide::dec_gene_bwd_mfma2_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, wide::M_BYTES));
      HIP_TRY(hipFuncSetAttribute((const void*)wide::dec_gene_bwd_mfma2_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, wide::M_BYTES));
      HIP_TRY(hipFuncSetAttribute((const void*)wide::enc_pool_bwd_rows_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, wide::PB_BYTES));
      HIP_TRY(hipFuncSetAttribute((const void*)wide::dec_gene_bwd_mfma2_kernel<false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, wide::M_BYTES));
      HIP_TRY(hipFuncSetAttribute((const void*)wide::dec_gene_bwd_mfma2_kernel<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, wide::M_BYTES));
      HIP_TRY(hipFuncSetAttribute((const void*)wide::dec_gene_bwd_gauss_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, wide::MG_BYTES));
      HIP_TRY(hipFuncSetAttribute((const void*)wide::dec_gene_bwd_gauss_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, wide::MG_BYTES));
      HIP_TRY(hipFuncSetAttribute((const void*)wide::dec_gene_bwd_nb2_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, wide::N_BYTES));
      HIP_TRY(hipFuncSetAttribute((const void*)wide::dec_gene_bwd_nb2_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, wide::N_BYTES));
      HIP_TRY(hipFuncSetAttribute((const void*)wide::dec_gene_bwd_nb2_kernel<false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, wide::N_BYTES));
      HIP_TRY(hipFuncSetAttribute((const void*)wide::dec_gene_bwd_nb2_kernel<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, wide::N_BYTES));
      if (dev >= 0 && dev < 64) attr_set[dev].store(true, std::memory_order_release);
    }
  }
  // The recompute forwards of the two 16-token sides (B workgroups each) only feed the cell-side backward kernels: they run on a second
  // stream beside the head and per-gene backward, which take the cells' K | V from the copy the forward left in `saved`.
  static const bool overlap = [] { const char* e = getenv("SCLDM_VAE_TRAIN_OVERLAP"); return !(e && e[0] == '0'); }();
  hipStream_t s2 = st;
  if (overlap) {
    if (!h->side) {
      HIP_TRY(hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking));
      HIP_TRY(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
      HIP_TRY(hipEventCreateWithFlags(&h->ev_gene, hipEventDisableTiming));
      HIP_TRY(hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming));
    }
    s2 = h->side;
    HIP_TRY(hipEventRecord(h->ev_fork, st));
    HIP_TRY(hipStreamWaitEvent(s2, h->ev_fork, 0));
  }
  // whatever path leaves this function, the caller's stream waits for everything the second stream was given (the caller frees the
  // workspace in stream order of `st` only)
  struct JoinSide {
    scldm_vae* h; hipStream_t st; bool on;
    ~JoinSide() {
      if (!on) return;
      if (hipEventRecord(h->ev_fork, h->side) == hipSuccess) (void)hipStreamWaitEvent(st, h->ev_fork, 0);
    }
  } join_side{h, st, overlap};
  wide::enc_cell_fwd_kernel<<<B, wide::kThreads, wide::LDS_BYTES, s2>>>(ea);
  LAUNCH_CHECK();
  DecCellTrainArgs da{};
  da.z = z; da.w_in = w->dec_latent_w; da.blocks = blocks_of(w->dec_blocks, L, wct(2 + L), H);
  da.cln1_w = w->dec_cross.ln1_w; da.cln1_b = w->dec_cross.ln1_b; da.wkv = w->dec_cross.attn_kv;
  da.xsave = k.xs_dec; da.kv = k.kv; da.dkv_part = k.p_dkv; da.chunks = k.chunksD; da.dz = k.dz_dec; da.part = k.p_dcell;
  da.B = B; da.n_lat = nl; da.n_layer = L; da.eps = eps;
  wide::dec_cell_fwd_kernel<<<B, wide::kThreads, wide::LDS_BYTES, s2>>>(da);
  LAUNCH_CHECK();
  if (overlap) HIP_TRY(hipEventRecord(h->ev_join, s2));
  // ---- NB head, then the per-gene decoder chain (the Gaussian head has no head pass: d logit is d mu as given, the head bias
  // gradient comes out of the per-gene kernel's partial, and there is no theta)
  if (gauss) {
    if (!dmu) HIP_TRY(hipMemsetAsync(k.dl, 0, (size_t)B * G * sizeof(float), st));
  } else if (nb2) {      // d l0 | d l1 per slot; no theta table, and both bias sums come out of the per-gene kernel's partial
    if (f16) head_bwd_nb2_kernel<true><<<B, 256, 0, st>>>(mu, theta, dmu, dtheta, library_size, G, 1.0f / c.nb_temperature, k.dl, k.dl2, k.dl_scale);
    else head_bwd_nb2_kernel<false><<<B, 256, 0, st>>>(mu, theta, dmu, dtheta, library_size, G, 1.0f / c.nb_temperature, k.dl, k.dl2, nullptr);
  } else if (ordered) {
    if (f16) head_bwd_kernel<true, true><<<B, 256, 0, st>>>(mu, theta, dmu, dtheta, library_size, nullptr, G, 1.0f / c.nb_temperature, k.dl, rw.theta, k.bsum, k.dl_scale);
    else head_bwd_kernel<false, true><<<B, 256, 0, st>>>(mu, theta, dmu, dtheta, library_size, nullptr, G, 1.0f / c.nb_temperature, k.dl, rw.theta, k.bsum, nullptr);
  } else if (f16) head_bwd_kernel<true><<<B, 256, 0, st>>>(mu, theta, dmu, dtheta, library_size, genes, G, 1.0f / c.nb_temperature, k.dl, g_theta, k.bsum, k.dl_scale);
  else head_bwd_kernel<false><<<B, 256, 0, st>>>(mu, theta, dmu, dtheta, library_size, genes, G, 1.0f / c.nb_temperature, k.dl, g_theta, k.bsum, nullptr);
  LAUNCH_CHECK();
  DecBwdArgs ga{};
  ga.genes = genes; ga.emb = w->gene_embedding; ga.dl = gauss && dmu ? dmu : k.dl; ga.kv = overlap ? sv.kv : k.kv;
  ga.ln1q_w = w->dec_cross.ln1q_w; ga.ln1q_b = w->dec_cross.ln1q_b; ga.wq = w->dec_cross.attn_q; ga.wp = w->dec_cross.attn_proj;
  ga.ln2_w = w->dec_cross.ln2_w; ga.ln2_b = w->dec_cross.ln2_b; ga.head_w = w->head_w;
  ga.mlp = mlp_of(w->dec_cross.w1, w->dec_cross.w2, wct(1), H);
  ga.g_emb = ordered ? rw.emb : g_emb; ga.part = k.p_gene; ga.dkv_part = k.p_dkv; ga.G = G; ga.tiles = k.tilesD; ga.eps = eps;
  if (gauss) {
    DecBwdGaussArgs gg{ga, w->head_ln_w, w->head_ln_b};
    if (ordered) wide::dec_gene_bwd_gauss_kernel<true><<<dim3(k.chunksD, B), wide::kThreads, wide::MG_BYTES, st>>>(gg);
    else wide::dec_gene_bwd_gauss_kernel<false><<<dim3(k.chunksD, B), wide::kThreads, wide::MG_BYTES, st>>>(gg);
  } else if (nb2) {
    if (f16) {
      ga.dl_scale = k.dl_scale;
      ga.found_inf = h->found_inf;
    }
    DecBwdNb2Args gn{ga, k.dl2};
    const dim3 grid(k.chunksD, B);
    if (f16 && ordered) wide::dec_gene_bwd_nb2_kernel<true, true><<<grid, wide::kThreads, wide::N_BYTES, st>>>(gn);
    else if (f16) wide::dec_gene_bwd_nb2_kernel<true><<<grid, wide::kThreads, wide::N_BYTES, st>>>(gn);
    else if (ordered) wide::dec_gene_bwd_nb2_kernel<false, true><<<grid, wide::kThreads, wide::N_BYTES, st>>>(gn);
    else wide::dec_gene_bwd_nb2_kernel<false><<<grid, wide::kThreads, wide::N_BYTES, st>>>(gn);
  } else if (f16) {
    ga.dl_scale = k.dl_scale;
    ga.found_inf = h->found_inf;
    if (ordered) wide::dec_gene_bwd_mfma2_kernel<true, true><<<dim3(k.chunksD, B), wide::kThreads, wide::M_BYTES, st>>>(ga);
    else wide::dec_gene_bwd_mfma2_kernel<true><<<dim3(k.chunksD, B), wide::kThreads, wide::M_BYTES, st>>>(ga);
  } else if (ordered) wide::dec_gene_bwd_mfma2_kernel<false, true><<<dim3(k.chunksD, B), wide::kThreads, wide::M_BYTES, st>>>(ga);
  else wide::dec_gene_bwd_mfma2_kernel<false><<<dim3(k.chunksD, B), wide::kThreads, wide::M_BYTES, st>>>(ga);
  LAUNCH_CHECK();
  if (overlap) {
    HIP_TRY(hipEventRecord(h->ev_gene, st));
    HIP_TRY(hipStreamWaitEvent(st, h->ev_join, 0));
  }
  wide::dec_cell_bwd_kernel<<<B, wide::kThreads, wide::LDS_BYTES, st>>>(da);
  LAUNCH_CHECK();
  wide::enc_cell_bwd_kernel<<<B, wide::kThreads, wide::LDS_BYTES, st>>>(ea);
  LAUNCH_CHECK();
  EncPoolBwdArgs pa{};
  pa.counts = counts_subset; pa.genes = genes_subset; pa.emb = w->gene_embedding;
  pa.ln1_w = w->enc_cross.ln1_w; pa.ln1_b = w->enc_cross.ln1_b; pa.wkv = w->enc_cross.attn_kv; pa.Q = k.Q; pa.lse2 = sv.lse2;
  pa.dao = k.dao; pa.dgq = k.dgq; pa.g_emb = ordered ? rw.emb + (size_t)B * G * 32 : g_emb; pa.part = k.p_pool; pa.S = S; pa.tiles = k.tilesE; pa.eps = eps;
  if (ordered) wide::enc_pool_bwd_rows_kernel<<<dim3(k.chunksE, B), wide::kThreads, wide::PB_BYTES, st>>>(pa);
  else wide::enc_pool_bwd_kernel<<<dim3(k.chunksE, B), wide::kThreads, wide::PB_BYTES, st>>>(pa);
  LAUNCH_CHECK();
  if (ordered) {
    // both producers of the row buffers (head + per-gene kernel, pooling) ran on `st`: the two table sums follow them in stream order.
    // The theta table walks the same segments and takes the decoder entries (those below B * G) only.
    const int n_table = c.n_genes + 1, n_dec = B * G;
    table_rows_reduce_kernel<<<n_table, 256, 0, st>>>(rw.emb, order, seg, n_table, n_entries, n_dec + B * S, g_emb);
    if (!gauss && !nb2) table_scalars_reduce_kernel<<<cdiv(n_table, 32), 256, 0, st>>>(rw.theta, order, seg, n_table, n_entries, n_dec, g_theta);
    LAUNCH_CHECK();
  }

  // ---- partial sums -> parameter gradients
  auto G_ = [](const float* p) { return const_cast<float*>(p); };
  {
    Jobs j;   // per-gene decoder chain
    const scldm_vae_cross& gc = g->dec_cross;
    j.mat(G_(gc.attn_q), DP_WQ, 32, 32, 32, 32);
    j.mat(G_(gc.attn_proj), DP_WP, 32, 32, 32, 32);
    j.mat(G_(gc.w1), DP_W1, H, 32, 32, 32);
    j.mat(G_(gc.w2), DP_W2, H, 32, 32, 32);
    j.mat(G_(gc.cproj), DP_WC, 32, H, kHP, H);
    j.vec(G_(gc.ln1q_w), DP_LN1QW, 32);
    j.vec(G_(gc.ln1q_b), DP_LN1QB, 32);
    j.vec(G_(gc.ln2_w), DP_LN2W, 32);
    j.vec(G_(gc.ln2_b), DP_LN2B, 32);
    j.vec(G_(g->head_w), DP_HEADW, 32);
    // (on the second stream, beside the cell-side backward kernels: it only needs the per-gene kernel's partials)
    if (overlap) HIP_TRY(hipStreamWaitEvent(s2, h->ev_gene, 0));
    if (gauss) {
      j.vec(G_(g->head_ln_w), GP_HLNW, 32);
      j.vec(G_(g->head_ln_b), GP_HLNB, 32);
      j.vec(G_(g->head_b), GP_HEADB, 1);
      if ((rc = j.run(k.p_gene, B * k.chunksD, GP_SIZE, s2))) return rc;
    } else if (nb2) {
      j.vec(G_(g->head_w) + 32, NP_HEADW1, 32);
      j.vec(G_(g->head_b), NP_HEADB, 2);
      if ((rc = j.run(k.p_gene, B * k.chunksD, NP_SIZE, s2))) return rc;
    } else {
      if ((rc = j.run(k.p_gene, B * k.chunksD, DP_SIZE, s2))) return rc;
      Jobs jb;
      jb.vec(G_(g->head_b), 0, 1);
      if ((rc = jb.run(k.bsum, B, 1, s2))) return rc;
    }
  }
  {
    Jobs j;   // decoder cell side
    for (int l = 0; l < L; ++l) trunk_jobs(j, g->dec_blocks[l], l * TP_SIZE, H);
    j.mat(G_(g->dec_cross.attn_kv), dc_off_wkv(L), 64, 32, 32, 32);
    j.vec(G_(g->dec_cross.ln1_w), dc_off_cln1w(L), 32);
    j.vec(G_(g->dec_cross.ln1_b), dc_off_cln1b(L), 32);
    j.mat(G_(g->dec_latent_w), dc_off_win(L), 32, nl, 32, nl);
    if ((rc = j.run(k.p_dcell, B, dc_size(L), st))) return rc;
  }
  {
    Jobs j;   // encoder cell side
    for (int l = 0; l < L; ++l) trunk_jobs(j, g->enc_blocks[l], l * TP_SIZE, H);
    const scldm_vae_cross& gc = g->enc_cross;
    j.mat(G_(gc.attn_proj), ec_off_wp(L), 32, 32, 32, 32);
    j.mat(G_(gc.w1), ec_off_w1(L), H, 32, 32, 32);
    j.mat(G_(gc.w2), ec_off_w2(L), H, 32, 32, 32);
    j.mat(G_(gc.cproj), ec_off_wc(L), 32, H, kHP, H);
    j.vec(G_(gc.ln2_w), ec_off_ln2w(L), 32);
    j.vec(G_(gc.ln2_b), ec_off_ln2b(L), 32);
    j.mat(G_(g->enc_latent_w), ec_off_wlat(L), nl, 32, 32, 32);
    j.vec(G_(g->inducing_points), ec_off_ind(L), 512);
    if ((rc = j.run(k.p_ecell, B, ec_size(L), st))) return rc;
  }
  {
    Jobs j;   // encoder pooling
    j.mat(G_(g->enc_cross.attn_kv), EP_WKV, 64, 32, 32, 32);
    j.vec(G_(g->enc_cross.ln1_w), EP_LN1W, 32);
    j.vec(G_(g->enc_cross.ln1_b), EP_LN1B, 32);
    if ((rc = j.run(k.p_pool, B * k.chunksE, EP_SIZE, st))) return rc;
    fold_dq_kernel<<<8, 64, 0, st>>>(k.p_pool, B * k.chunksE, EP_SIZE, k.dQ);
    LAUNCH_CHECK();
    // (the inducing-point gradient was set by the encoder-cell reduction above; this adds the query-projection branch)
    if (!g->inducing_points || !g->enc_cross.attn_q || !g->enc_cross.ln1q_w || !g->enc_cross.ln1q_b)
      return fail(SCLDM_ERR_SHAPE, "the encoder query-branch gradient pointers are required");
    enc_q_bwd_kernel<<<1, 64, 0, st>>>(w->inducing_points, w->enc_cross.ln1q_w, w->enc_cross.ln1q_b, w->enc_cross.attn_q, eps, k.dQ,
                                       G_(g->enc_cross.attn_q), G_(g->enc_cross.ln1q_w), G_(g->enc_cross.ln1q_b), G_(g->inducing_points));
    LAUNCH_CHECK();
  }
  return SCLDM_OK;   // (join_side: `st` waits for the second stream)
}
}  // namespace

extern "C" size_t scldm_vae_train_rows_bytes(const scldm_vae* h, int B, int S, int G) {
  if (!h || B < 1 || S < 1 || G < 1) return 0;
  return carve_rows(B, S, G, nullptr).bytes;
}

extern "C" int scldm_vae_train_backward_ex(scldm_vae* h, const scldm_vae_weights* w, const scldm_vae_weights* g, const float* counts_subset,
                                           const int64_t* genes_subset, int B, int S, const int64_t* genes, const float* library_size, int G,
                                           const float* mu, const float* theta, const float* z, const float* dmu, const float* dtheta,
                                           const float* dz, void* saved_, void* ws_, int precision, void* stream_) {
  return train_backward_impl(h, w, g, counts_subset, genes_subset, B, S, genes, library_size, G, mu, theta, z, dmu, dtheta, dz, saved_, ws_,
                             precision, nullptr, nullptr, 0, nullptr, stream_);
}

extern "C" int scldm_vae_train_backward_ordered(scldm_vae* h, const scldm_vae_weights* w, const scldm_vae_weights* g,
                                                const float* counts_subset, const int64_t* genes_subset, int B, int S, const int64_t* genes,
                                                const float* library_size, int G, const float* mu, const float* theta, const float* z,
                                                const float* dmu, const float* dtheta, const float* dz, void* saved_, void* ws_, int precision,
                                                const int32_t* order, const int32_t* seg, int n_entries, void* rows, void* stream_) {
  if (!seg || !rows || (!order && n_entries != 0)) return fail(SCLDM_ERR_SHAPE, "scldm_vae_train_backward_ordered: null order / seg / rows");
  if (B < 1 || S < 1 || G < 1) return fail(SCLDM_ERR_SHAPE, "need B, S, G >= 1 (got %d, %d, %d)", B, S, G);
  const long long n_max = (long long)B * G + (long long)B * S;
  if (n_max > 0x7fffffffLL - 64) return fail(SCLDM_ERR_SHAPE, "B * (G + S) = %lld entries exceed the int32 entry index", n_max);
  if (n_entries < 0 || n_entries > n_max)
    return fail(SCLDM_ERR_SHAPE, "n_entries %d outside [0, B * G + B * S = %lld]", n_entries, n_max);
  return train_backward_impl(h, w, g, counts_subset, genes_subset, B, S, genes, library_size, G, mu, theta, z, dmu, dtheta, dz, saved_, ws_,
                             precision, order, seg, n_entries, rows, stream_);
}

// Gaussian head, both table-gradient modes: order == NULL is the atomic mode, otherwise the contract of scldm_vae_train_backward_ordered
extern "C" int scldm_vae_train_gaussian_backward(scldm_vae* h, const scldm_vae_weights* w, const scldm_vae_weights* g,
                                                 const float* counts_subset, const int64_t* genes_subset, int B, int S, const int64_t* genes,
                                                 int G, const float* mu, const float* z, const float* dmu, const float* dz, void* saved_,
                                                 void* ws_, const int32_t* order, const int32_t* seg, int n_entries, void* rows,
                                                 void* stream_) {
  if (h && !h->gaussian) return fail(SCLDM_ERR_SHAPE, "%s", kNbNoGaussTrain);
  if (order) {
    if (!seg || !rows) return fail(SCLDM_ERR_SHAPE, "scldm_vae_train_gaussian_backward: null order / seg / rows");
    if (B < 1 || S < 1 || G < 1) return fail(SCLDM_ERR_SHAPE, "need B, S, G >= 1 (got %d, %d, %d)", B, S, G);
    const long long n_max = (long long)B * G + (long long)B * S;
    if (n_max > 0x7fffffffLL - 64) return fail(SCLDM_ERR_SHAPE, "B * (G + S) = %lld entries exceed the int32 entry index", n_max);
    if (n_entries < 0 || n_entries > n_max)
      return fail(SCLDM_ERR_SHAPE, "n_entries %d outside [0, B * G + B * S = %lld]", n_entries, n_max);
  } else {
    rows = nullptr;
  }
  return train_backward_impl(h, w, g, counts_subset, genes_subset, B, S, genes, nullptr, G, mu, nullptr, z, dmu, nullptr, dz, saved_, ws_,
                             SCLDM_PREC_FP32, order, seg, n_entries, rows, stream_, true);
}

extern "C" int scldm_vae_train_backward(scldm_vae* h, const scldm_vae_weights* w, const scldm_vae_weights* g, const float* counts_subset,
                                        const int64_t* genes_subset, int B, int S, const int64_t* genes, const float* library_size, int G,
                                        const float* mu, const float* theta, const float* z, const float* dmu, const float* dtheta,
                                        const float* dz, void* saved_, void* ws_, void* stream_) {
  return scldm_vae_train_backward_ex(h, w, g, counts_subset, genes_subset, B, S, genes, library_size, G, mu, theta, z, dmu, dtheta, dz,
                                     saved_, ws_, SCLDM_PREC_FP32, stream_);
}

extern "C" int scldm_nb_loglik(const float* x, const float* mu, const float* theta, float eps, float* out, size_t n, void* stream_) {
  if (!x || !mu || !theta || !out) return fail(SCLDM_ERR_SHAPE, "null argument");
  if (n == 0) return SCLDM_OK;
  nb_loglik_kernel<<<(int)std::min<size_t>((n + 255) / 256, 256 * 32), 256, 0, (hipStream_t)stream_>>>(x, mu, theta, eps, out, n);
  LAUNCH_CHECK();
  return SCLDM_OK;
}
extern "C" int scldm_nb_loglik_bwd(const float* x, const float* mu, const float* theta, const float* gout, float eps, float* dmu,
                                   float* dtheta, size_t n, void* stream_) {
  if (!x || !mu || !theta || !gout) return fail(SCLDM_ERR_SHAPE, "null argument");
  if (n == 0) return SCLDM_OK;
  nb_loglik_bwd_kernel<<<(int)std::min<size_t>((n + 255) / 256, 256 * 32), 256, 0, (hipStream_t)stream_>>>(x, mu, theta, gout, eps, dmu, dtheta, n);
  LAUNCH_CHECK();
  return SCLDM_OK;
}

// C ABI of the shape-generic TransformerVAE inference route (include/scldm_hip.h: scldm_vaew_*; kernels in vae_wide.hpp).
#include <cstdlib>
#include <cstring>
#include <vector>

#include "api_common.hpp"
#include "vae_wide.hpp"
#include "vae_wide_host.hpp"

using namespace scldm;
using namespace scldm::vaew;
using namespace scldm::vaew_host;

static const size_t kDefaultCapMb = 1024;
static const long long kMaxChunkRows = 1ll << 30;   // rows of one chunk (cells x tokens): row indices stay ints

extern "C" int scldm_vaew_create(const scldm_vae_config* c, scldm_vaew** out) {
  if (!c || !out) return fail(SCLDM_ERR_SHAPE, "null argument");
  if (c->n_embed % 32 != 0) return fail(SCLDM_ERR_SHAPE, "wide VAE route: n_embed %% 32 == 0 is required (got n_embed=%d)", c->n_embed);
  if (c->n_embed < 64 || c->n_embed > kMaxEmbed)
    return fail(SCLDM_ERR_SHAPE, "wide VAE route: 64 <= n_embed <= %d is required (got n_embed=%d)", kMaxEmbed, c->n_embed);
  const int heads[2] = {c->n_head, c->n_head_cross};
  const char* names[2] = {"n_head", "n_head_cross"};
  for (int i = 0; i < 2; ++i) {
    if (heads[i] < 1 || c->n_embed % heads[i] != 0)
      return fail(SCLDM_ERR_SHAPE, "wide VAE route: n_embed %% %s == 0 is required (got n_embed=%d, %s=%d)", names[i], c->n_embed, names[i], heads[i]);
    const int hd = c->n_embed / heads[i];
    if (hd % 8 != 0 || hd < 8 || hd > 256)
      return fail(SCLDM_ERR_SHAPE, "wide VAE route: the head dim n_embed / %s must be a multiple of 8 in [8, 256] (got %d)", names[i], hd);
  }
  if (c->n_inducing < 1 || c->n_inducing > 64)
    return fail(SCLDM_ERR_SHAPE, "wide VAE route: 1 <= n_inducing_points <= 64 is required (got %d)", c->n_inducing);
  if (c->n_embed_latent < 1 || c->n_embed_latent > c->n_embed)
    return fail(SCLDM_ERR_SHAPE, "wide VAE route: 1 <= n_embed_latent <= n_embed is required (got n_embed_latent=%d, n_embed=%d)",
                c->n_embed_latent, c->n_embed);
  if (c->n_layer < 0) return fail(SCLDM_ERR_SHAPE, "wide VAE route: n_layer >= 0 is required (got %d)", c->n_layer);
  if (c->hidden_dim < 1) return fail(SCLDM_ERR_SHAPE, "wide VAE route: hidden_dim >= 1 is required (got %d)", c->hidden_dim);
  if (c->n_genes < 1) return fail(SCLDM_ERR_SHAPE, "wide VAE route: n_genes >= 1 is required (got %d)", c->n_genes);
  if (!(c->nb_temperature > 0.f)) return fail(SCLDM_ERR_SHAPE, "wide VAE route: nb_temperature > 0 is required");
  scldm_vaew* h = new scldm_vaew();
  h->cfg = *c;
  h->loaded = false;
  h->unshared_theta = false;
  memset(&h->w, 0, sizeof(h->w));
  size_t mb = kDefaultCapMb;
  if (const char* e = getenv("SCLDM_VAEW_WS_MB")) {
    const long long v = atoll(e);
    if (v < 1) {
      delete h;
      return fail(SCLDM_ERR_SHAPE, "SCLDM_VAEW_WS_MB must be a positive number of MiB (got '%s')", e);
    }
    mb = (size_t)v;
  }
  h->cap_bytes = mb << 20;
  *out = h;
  return SCLDM_OK;
}

extern "C" void scldm_vaew_destroy(scldm_vaew* h) { delete h; }

extern "C" int scldm_vaew_load_weights(scldm_vaew* h, const scldm_vae_weights* w, void* /*stream*/) {
  if (!h || !w) return fail(SCLDM_ERR_SHAPE, "null argument");
  const scldm_vae_config& c = h->cfg;
  if (w->head_ln_w || w->head_ln_b)
    return fail(SCLDM_ERR_SHAPE, "wide VAE route: the Gaussian head (GaussianTransformerLayer) is not built; it decodes the negative-binomial head only");
  if (c.positional_encoding && !w->enc_pos_embed) return fail(SCLDM_ERR_SHAPE, "positional_encoding set but enc_pos_embed is NULL");
  const void* need[] = {w->gene_embedding, w->inducing_points, w->enc_latent_w, w->dec_latent_w, w->head_w, w->head_b};
  for (const void* p : need)
    if (!p) return fail(SCLDM_ERR_SHAPE, "scldm_vaew_load_weights: a weight pointer is NULL");
  for (const scldm_vae_cross* cr : {&w->enc_cross, &w->dec_cross}) {
    const void* ps[] = {cr->ln1_w, cr->ln1_b, cr->ln1q_w, cr->ln1q_b, cr->attn_kv, cr->attn_q, cr->attn_proj, cr->ln2_w, cr->ln2_b, cr->w1, cr->w2, cr->cproj};
    for (const void* p : ps)
      if (!p) return fail(SCLDM_ERR_SHAPE, "scldm_vaew_load_weights: a cross-attention weight pointer is NULL");
  }
  if (c.n_layer > 0 && (!w->enc_blocks || !w->dec_blocks)) return fail(SCLDM_ERR_SHAPE, "scldm_vaew_load_weights: the block arrays are NULL");
  std::vector<scldm_vae_block> eb, db;
  for (int i = 0; i < c.n_layer; ++i)
    for (int side = 0; side < 2; ++side) {
      const scldm_vae_block& b = side ? w->dec_blocks[i] : w->enc_blocks[i];
      const void* ps[] = {b.ln1_w, b.ln1_b, b.attn_w, b.proj_w, b.ln2_w, b.ln2_b, b.w1, b.w2, b.cproj};
      for (const void* p : ps)
        if (!p) return fail(SCLDM_ERR_SHAPE, "scldm_vaew_load_weights: a weight pointer of trunk layer %d is NULL", i);
      (side ? db : eb).push_back(b);
    }
  h->w = *w;
  h->enc_blocks.swap(eb);
  h->dec_blocks.swap(db);
  h->w.enc_blocks = h->enc_blocks.data();
  h->w.dec_blocks = h->dec_blocks.data();
  h->unshared_theta = w->theta == nullptr;
  h->loaded = true;
  return SCLDM_OK;
}

// ---- workspace layout of one chunk of `cells` cells with T tokens each (encode: the S expressed genes, decode: the G genes)
namespace {
struct Layout {
  size_t h, t, att, qkv, hid;           // the inducing-point rows of the cells: (cells * n_inducing, n | n | n | 3 n | hidden)
  size_t qi, qq;                        // encode: LN_1q(inducing points), its projection (n_inducing, n)
  size_t xln, kv;                       // encode: (cells * S, n | 2 n)
  size_t part;                          // encode: the pooling's per-split (acc, max, sum): (cells, heads, n_inducing, splits, hd + 2)
  size_t zln, kvc;                      // decode: (rows, n_lat), (rows, 2 n)
  size_t ga, gb, ghid, pairs;           // decode: (cells * G, n | n | hidden), (cells, chunks, 2)
  size_t bytes;
};
Layout layout(const scldm_vae_config& c, bool decode, long long cells, long long T) {
  Layout L;
  memset(&L, 0, sizeof(L));
  size_t o = 0;
  auto take = [&](size_t floats) { const size_t r = o; o += align256(floats * sizeof(float)); return r; };
  const size_t n = c.n_embed, H = c.hidden_dim, rows = (size_t)cells * c.n_inducing, tok = (size_t)cells * T;
  L.h = take(rows * n); L.t = take(rows * n); L.att = take(rows * n); L.qkv = take(rows * 3 * n); L.hid = take(rows * H);
  if (!decode) {
    L.qi = take((size_t)c.n_inducing * n); L.qq = take((size_t)c.n_inducing * n);
    L.xln = take(tok * n); L.kv = take(tok * 2 * n);
    const int hd = c.n_embed / c.n_head_cross, splits = cdiv(T, attn_keys_per_split(hd));
    L.part = take(splits > 1 ? rows * c.n_head_cross * splits * (hd + 2) : 0);
  } else {
    L.zln = take(rows * c.n_embed_latent); L.kvc = take(rows * 2 * n);
    L.ga = take(tok * n); L.gb = take(tok * n); L.ghid = take(tok * H);
    L.pairs = take((size_t)cells * cdiv(T, kNbChunk) * 2);
  }
  L.bytes = o;
  return L;
}
int plan(const scldm_vaew* h, bool decode, int B, int T, size_t cap, int* cells, int* chunks, size_t* bytes) {
  if (!h) return fail(SCLDM_ERR_SHAPE, "null handle");
  if (B < 1 || T < 1) return fail(SCLDM_ERR_SHAPE, "scldm_vaew_plan: B and the token count must be >= 1 (got %d, %d)", B, T);
  if (cap == 0) cap = h->cap_bytes;
  const size_t one = layout(h->cfg, decode, 1, T).bytes;
  if (one > cap)
    return fail(SCLDM_ERR_SHAPE, "wide VAE route: one cell of %d tokens needs %zu workspace bytes, above the cap of %zu (SCLDM_VAEW_WS_MB)", T, one, cap);
  long long lo = 1, hi = B;                              // the largest chunk under the cap (the layout grows with the cells)
  if (hi > 65535) hi = 65535;                            // the cells are a grid's z extent
  if ((long long)T * hi > kMaxChunkRows) hi = kMaxChunkRows / T > 1 ? kMaxChunkRows / T : 1;
  while (lo < hi) {
    const long long mid = (lo + hi + 1) / 2;
    if (layout(h->cfg, decode, mid, T).bytes <= cap) lo = mid; else hi = mid - 1;
  }
  *cells = (int)lo;
  *chunks = cdiv(B, lo);
  *bytes = layout(h->cfg, decode, lo, T).bytes;
  return SCLDM_OK;
}
}  // namespace

extern "C" int scldm_vaew_plan(const scldm_vaew* h, int decode, int B, int tokens, size_t cap_bytes, int* cells_per_chunk, int* n_chunks,
                               size_t* ws_bytes) {
  if (!cells_per_chunk || !n_chunks || !ws_bytes) return fail(SCLDM_ERR_SHAPE, "null argument");
  return plan(h, decode != 0, B, tokens, cap_bytes, cells_per_chunk, n_chunks, ws_bytes);
}

extern "C" size_t scldm_vaew_workspace_bytes(const scldm_vaew* h, int B, int S, int G) {
  size_t need = 0;
  int cells, chunks;
  size_t bytes;
  if (S > 0) {
    if (plan(h, false, B, S, 0, &cells, &chunks, &bytes)) return 0;
    need = bytes;
  }
  if (G > 0) {
    if (plan(h, true, B, G, 0, &cells, &chunks, &bytes)) return 0;
    need = bytes > need ? bytes : need;
  }
  return need;
}

// ---- launch helpers (declared in vae_wide_host.hpp: the training backward rebuilds its record with them)
namespace {
template <int EPI>
void gemm(const Ctx& c, const GemmArgs& a) {
  const dim3 grid(cdiv(a.M, kBM), cdiv(a.N, EPI == EPI_SWIGLU ? 32 : 64));
  if (c.prec == SCLDM_PREC_FP16) gemm_kernel<F16Operands, EPI><<<grid, 256, 0, c.st>>>(a);
  else gemm_kernel<F32Operands, EPI><<<grid, 256, 0, c.st>>>(a);
}
GemmArgs gemm_args(const float* X, const float* W, float* out, long long M, int N, int K) {
  GemmArgs a;
  memset(&a, 0, sizeof(a));
  a.X = X; a.W0 = W; a.W1 = W; a.out = out; a.M = (int)M; a.N = N; a.K = K;
  return a;
}
}  // namespace
namespace scldm {
namespace vaew_host {
static_assert(kWideMaxEmbed == kMaxEmbed, "one width limit");
int wide_attn_keys_per_split(int hd) { return attn_keys_per_split(hd); }
void store(const Ctx& c, const float* X, const float* W, float* out, long long M, int N, int K) { gemm<EPI_STORE>(c, gemm_args(X, W, out, M, N, K)); }
void resid(const Ctx& c, const float* X, const float* W, float* out, long long M, int N, int K, const float* R, int rmod,
           const float* R2, int r2mod, const int64_t* ridx, int ridx_max) {
  GemmArgs a = gemm_args(X, W, out, M, N, K);
  a.R = R; a.rmod = rmod; a.R2 = R2; a.r2mod = r2mod; a.ridx = ridx; a.ridx_max = ridx_max;
  gemm<EPI_RESID>(c, a);
}
void swiglu(const Ctx& c, const float* X, const float* w1, const float* w2, float* out, long long M, int H, int K) {
  GemmArgs a = gemm_args(X, w1, out, M, H, K);
  a.W1 = w2;
  gemm<EPI_SWIGLU>(c, a);
}
void ln(const Ctx& c, const float* src, float* out, long long rows, int n, const float* w, const float* b, const int64_t* gidx,
        const float* counts) {
  LnArgs a;
  a.src = src; a.gidx = gidx; a.idx_max = c.h->cfg.n_genes; a.counts = counts; a.w = w; a.b = b; a.out = out; a.rows = rows; a.n = n;
  a.eps = c.h->cfg.layernorm_eps;
  ln_rows_kernel<<<cdiv(rows, 4), 256, 0, c.st>>>(a);
}
void attn(const Ctx& c, const float* Q, size_t q_bs, int q_ld, const float* K, const float* V, size_t kv_bs, int kv_ld, float* O, int cells,
          int M, int S, int heads, float* part) {
  AttnArgs a;
  const int n = c.h->cfg.n_embed;
  a.Q = Q; a.q_bs = q_bs; a.q_ld = q_ld; a.K = K; a.V = V; a.kv_bs = kv_bs; a.kv_ld = kv_ld; a.O = O; a.o_ld = n; a.M = M; a.S = S;
  a.hd = n / heads; a.kc = attn_key_chunk(a.hd); a.scale = 1.0f / sqrtf((float)a.hd);
  a.keys_per_split = attn_keys_per_split(a.hd);
  a.splits = part ? cdiv(S, a.keys_per_split) : 1;       // (without a partials buffer: the trunk and the unpooling, n_inducing keys)
  if (a.splits == 1) a.keys_per_split = S;
  a.part = part;
  attn_kernel<<<dim3(cdiv(M, kAttnQueriesPerBlock) * a.splits, heads, cells), 256, attn_lds_bytes(a.hd), c.st>>>(a);
  if (a.splits > 1) {
    const long long rows = (long long)cells * heads * M;
    attn_merge_kernel<<<cdiv(rows, 4), 256, 0, c.st>>>(part, O, n, rows, heads, M, a.hd, a.splits);
  }
}
}  // namespace vaew_host
}  // namespace scldm
namespace {
// the plain Blocks on the cells' inducing-point rows h (rows, n), in place (layers.py:222-226)
void trunk(const Ctx& c, const std::vector<scldm_vae_block>& blocks, const Layout& L, char* ws, int cells) {
  const scldm_vae_config& f = c.h->cfg;
  const int n = f.n_embed, ni = f.n_inducing, H = f.hidden_dim;
  const long long rows = (long long)cells * ni;
  float *h = (float*)(ws + L.h), *t = (float*)(ws + L.t), *att = (float*)(ws + L.att), *qkv = (float*)(ws + L.qkv), *hid = (float*)(ws + L.hid);
  for (const scldm_vae_block& b : blocks) {
    ln(c, h, t, rows, n, b.ln1_w, b.ln1_b);
    store(c, t, b.attn_w, qkv, rows, 3 * n, n);
    attn(c, qkv, (size_t)ni * 3 * n, 3 * n, qkv + n, qkv + 2 * n, (size_t)ni * 3 * n, 3 * n, att, cells, ni, ni, f.n_head);
    resid(c, att, b.proj_w, h, rows, n, n, h);
    ln(c, h, t, rows, n, b.ln2_w, b.ln2_b);
    swiglu(c, t, b.w1, b.w2, hid, rows, H, n);
    resid(c, hid, b.cproj, h, rows, n, H, h);
  }
}
int ready(const scldm_vaew* h, int precision) {
  if (!h) return fail(SCLDM_ERR_SHAPE, "null handle");
  if (!h->loaded) return fail(SCLDM_ERR_STATE, "scldm_vaew_load_weights has not been called");
  if (precision != SCLDM_PREC_FP32 && precision != SCLDM_PREC_FP16)
    return fail(SCLDM_ERR_SHAPE, "wide VAE route: unsupported precision %d (fp32 and fp16; bf16 operands are not built)", precision);
  return SCLDM_OK;
}
}  // namespace

extern "C" int scldm_vaew_encode(scldm_vaew* h, const float* counts, const int64_t* genes, int B, int S, float* z, int precision, void* ws_,
                                 void* stream_) {
  int rc = ready(h, precision);
  if (rc) return rc;
  if (B < 1 || S < 1 || !counts || !genes || !z || !ws_) return fail(SCLDM_ERR_SHAPE, "bad argument");
  int cells, chunks;
  size_t bytes;
  if ((rc = plan(h, false, B, S, 0, &cells, &chunks, &bytes))) return rc;
  const Ctx c{h, precision, (hipStream_t)stream_};
  const scldm_vae_config& f = h->cfg;
  const scldm_vae_weights& w = h->w;
  const scldm_vae_cross& ec = w.enc_cross;
  const int n = f.n_embed, ni = f.n_inducing, H = f.hidden_dim, nl = f.n_embed_latent;
  char* ws = (char*)ws_;
  const Layout L = layout(f, false, cells, S);
  float *hb = (float*)(ws + L.h), *t = (float*)(ws + L.t), *att = (float*)(ws + L.att), *hid = (float*)(ws + L.hid);
  float *qi = (float*)(ws + L.qi), *qq = (float*)(ws + L.qq), *xln = (float*)(ws + L.xln), *kv = (float*)(ws + L.kv);
  // the inducing-point queries are the same for every cell: LN_1q, then c_attn_q, once per call
  ln(c, w.inducing_points, qi, ni, n, ec.ln1q_w, ec.ln1q_b);
  store(c, qi, ec.attn_q, qq, ni, n, n);
  for (int b0 = 0; b0 < B; b0 += cells) {
    const int bc = B - b0 < cells ? B - b0 : cells;
    const long long rows = (long long)bc * ni, tok = (long long)bc * S;
    const size_t o = (size_t)b0 * S;
    ln(c, w.gene_embedding, xln, tok, n, ec.ln1_w, ec.ln1_b, genes + o, counts + o);       // LN_1(emb[g] log1p(count))
    store(c, xln, ec.attn_kv, kv, tok, 2 * n, n);                                           // k | v
    attn(c, qq, 0, n, kv, kv + n, (size_t)S * 2 * n, 2 * n, att, bc, ni, S, f.n_head_cross, (float*)(ws + L.part));
    resid(c, att, ec.attn_proj, hb, rows, n, n, w.inducing_points, ni);                     // the residual is the raw query (layers.py:327)
    ln(c, hb, t, rows, n, ec.ln2_w, ec.ln2_b);
    swiglu(c, t, ec.w1, ec.w2, hid, rows, H, n);
    resid(c, hid, ec.cproj, hb, rows, n, H, hb, 0, f.positional_encoding ? w.enc_pos_embed : nullptr, ni);
    trunk(c, h->enc_blocks, L, ws, bc);
    store(c, hb, w.enc_latent_w, t, rows, nl, n);
    ln(c, t, z + (size_t)b0 * ni * nl, rows, nl, nullptr, nullptr);
    LAUNCH_CHECK();
  }
  return SCLDM_OK;
}

extern "C" int scldm_vaew_decode(scldm_vaew* h, const float* z, const int64_t* genes, const float* library_size, int B, int G, float* mu,
                                 float* theta, int precision, void* ws_, void* stream_) {
  int rc = ready(h, precision);
  if (rc) return rc;
  if (B < 1 || G < 1 || !z || !genes || !library_size || !mu || !theta || !ws_) return fail(SCLDM_ERR_SHAPE, "bad argument");
  int cells, chunks;
  size_t bytes;
  if ((rc = plan(h, true, B, G, 0, &cells, &chunks, &bytes))) return rc;
  const Ctx c{h, precision, (hipStream_t)stream_};
  const scldm_vae_config& f = h->cfg;
  const scldm_vae_weights& w = h->w;
  const scldm_vae_cross& dc = w.dec_cross;
  const int n = f.n_embed, ni = f.n_inducing, H = f.hidden_dim, nl = f.n_embed_latent;
  char* ws = (char*)ws_;
  const Layout L = layout(f, true, cells, G);
  float *hb = (float*)(ws + L.h), *t = (float*)(ws + L.t), *zln = (float*)(ws + L.zln), *kvc = (float*)(ws + L.kvc);
  float *ga = (float*)(ws + L.ga), *gb = (float*)(ws + L.gb), *ghid = (float*)(ws + L.ghid), *pairs = (float*)(ws + L.pairs);
  const int nch = cdiv(G, kNbChunk);
  for (int b0 = 0; b0 < B; b0 += cells) {
    const int bc = B - b0 < cells ? B - b0 : cells;
    const long long rows = (long long)bc * ni, tok = (long long)bc * G;
    const size_t o = (size_t)b0 * G;
    ln(c, z + (size_t)b0 * ni * nl, zln, rows, nl, nullptr, nullptr);
    store(c, zln, w.dec_latent_w, hb, rows, n, nl);
    trunk(c, h->dec_blocks, L, ws, bc);
    ln(c, hb, t, rows, n, dc.ln1_w, dc.ln1_b);
    store(c, t, dc.attn_kv, kvc, rows, 2 * n, n);                                           // the cell's keys | values
    ln(c, w.gene_embedding, ga, tok, n, dc.ln1q_w, dc.ln1q_b, genes + o);                   // LN_1q(emb[g])
    store(c, ga, dc.attn_q, gb, tok, n, n);
    attn(c, gb, (size_t)G * n, n, kvc, kvc + n, (size_t)ni * 2 * n, 2 * n, ga, bc, G, ni, f.n_head_cross);
    resid(c, ga, dc.attn_proj, gb, tok, n, n, w.gene_embedding, 0, nullptr, 1, genes + o, f.n_genes);   // + the raw gene embedding
    ln(c, gb, ga, tok, n, dc.ln2_w, dc.ln2_b);
    swiglu(c, ga, dc.w1, dc.w2, ghid, tok, H, n);
    resid(c, ghid, dc.cproj, gb, tok, n, H, gb);
    NbArgs a;
    a.h = gb; a.head_w = w.head_w; a.head_b = w.head_b; a.theta_tab = w.theta; a.genes = genes + o; a.idx_max = f.n_genes;
    a.mu = mu + o; a.theta = theta + o; a.pairs = pairs; a.G = G; a.n = n; a.chunks = nch; a.inv_temp = 1.0f / f.nb_temperature;
    nb_logits_kernel<<<dim3(nch, bc), 256, 0, c.st>>>(a);
    nb_finalize_kernel<<<dim3(cdiv(G, kNbFinal), bc), 256, 0, c.st>>>(mu + o, pairs, library_size + b0, G, nch);
    LAUNCH_CHECK();
  }
  return SCLDM_OK;
}

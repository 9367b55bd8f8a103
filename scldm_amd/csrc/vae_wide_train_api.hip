// C ABI of the training backward of the shape-generic TransformerVAE route (include/scldm_hip.h: scldm_vaew_train_*; kernels in
// vae_wide_train.hpp, the forward's in vae_wide.hpp).  Exact fp32.
#include <cmath>
#include <cstring>

#include "vae_wide_host.hpp"
#include "vae_wide_train.hpp"

using namespace scldm;
using namespace scldm::vaew_host;
using namespace scldm::vaewt;
using scldm::scvi::F32Operands;
using scldm::scvi::kBM;
using scldm::scvi::kBN;
using scldm::scvi_train::ProdArgs;

namespace {
const long long kMaxTrainChunkRows = 4000000;   // rows of one chunk (cells x tokens): the row tiles are a grid's y extent

int round32(long long k) { return (int)((k + 31) / 32 * 32); }
// k-values per split of a weight gradient whose k axis has K rows: a function of K alone
int tn_k_per_split(long long K) {
  const int slots = cdiv(K, scvi::kScviSplit) < kMaxSlots ? cdiv(K, scvi::kScviSplit) : kMaxSlots;
  return round32(cdiv(K, slots));
}
int tn_slots(long long K) { return cdiv(K, tn_k_per_split(K)); }

// ---- the record of one chunk of `cells` cells (S encoder tokens, G decoded genes each): byte offsets into the workspace.  Every
// stage of the forward has a buffer of its own.  The decoder's and the encoder's per-token records share their bytes (the decoder is
// walked back before the encoder is rebuilt), and so do the two trunks'.
struct Rec { size_t t1, qkv, att, hmid, t2, a, b, hid; };   // one plain Block: (rows, n | 3 n | n | n | n | H | H | H)
struct TL {
  size_t qi, qq, dqq, dqi;                      // the shared inducing-point queries and their gradients: (n_inducing, n)
  size_t P, C, stats;                           // product / attention partials, column partials, the softmax statistics
  std::vector<size_t> hs;                       // the trunk's layer inputs and its output: (n_layer + 1) x (rows, n)
  std::vector<Rec> layer;
  size_t dh, dt, dqkv, dH;                      // the trunk's gradients: (rows, n | n | 3 n | H)
  size_t dzc;                                   // dz of the chunk: (rows, n_lat)
  // decoder
  size_t zln, dzln, t, kvc, dkvc;               // (rows, n_lat | n_lat | n | 2 n | 2 n)
  size_t ga, gq, gatt, y, gt2, hout, a, b, hid, g2, dl, dl2;   // (cells * G, n x 6 | H x 3 | n | 1 | 1)
  // encoder
  size_t xln, kv, dkv, gx, part;                // (cells * S, n | 2 n | 2 n | n), the pooling's forward partials
  size_t eatt, hb0, et2, ea, eb, ehid, tlat, dtlat, dqc;   // (rows, n | n | n | H | H | H | n_lat | n_lat | n)
  size_t bytes;
};
TL layout(const scldm_vae_config& c, long long cells, long long S, long long G) {
  TL L;
  size_t o = 0;
  auto take = [&](size_t floats) { const size_t r = o; o += align256(floats * sizeof(float)); return r; };
  const size_t n = c.n_embed, H = c.hidden_dim, nl = c.n_embed_latent, ni = c.n_inducing;
  const size_t rows = (size_t)cells * ni, tg = (size_t)cells * G, ts = (size_t)cells * S;
  const size_t hmax = c.n_head > c.n_head_cross ? c.n_head : c.n_head_cross;
  L.qi = take(ni * n); L.qq = take(ni * n); L.dqq = take(ni * n); L.dqi = take(ni * n);
  // the partials' scratch: k-splits of a weight gradient, the pair of a SwiGLU's two data gradients, the attention's splits
  const size_t big = tg > ts ? tg : ts, mrows = big > rows ? big : rows;
  size_t maxw = 3 * n * n;
  if (n * H > maxw) maxw = n * H;
  size_t p = (size_t)tn_slots((long long)mrows) * maxw;
  if (2 * mrows * n > p) p = 2 * mrows * n;
  const size_t unpool = (size_t)cdiv(G, kAttnBwdQuerySplit) * rows * 2 * n;
  const size_t pool = (size_t)cdiv(S, wide_attn_keys_per_split(c.n_embed / c.n_head_cross)) * rows * n;
  if (unpool > p) p = unpool;
  if (pool > p) p = pool;
  L.P = take(p);
  L.C = take((size_t)cdiv((long long)mrows, kColRows) * (2 * n + 2));
  L.stats = take(3 * (tg * c.n_head_cross > rows * hmax ? tg * c.n_head_cross : rows * hmax));
  L.hs.resize(c.n_layer + 1);
  L.layer.resize(c.n_layer);
  for (size_t& h : L.hs) h = take(rows * n);
  for (Rec& r : L.layer) {
    r.t1 = take(rows * n); r.qkv = take(rows * 3 * n); r.att = take(rows * n); r.hmid = take(rows * n); r.t2 = take(rows * n);
    r.a = take(rows * H); r.b = take(rows * H); r.hid = take(rows * H);
  }
  L.dh = take(rows * n); L.dt = take(rows * n); L.dqkv = take(rows * 3 * n); L.dH = take(rows * H);
  L.dzc = take(rows * nl);
  const size_t u = o;
  L.zln = take(rows * nl); L.dzln = take(rows * nl); L.t = take(rows * n); L.kvc = take(rows * 2 * n); L.dkvc = take(rows * 2 * n);
  L.ga = take(tg * n); L.gq = take(tg * n); L.gatt = take(tg * n); L.y = take(tg * n); L.gt2 = take(tg * n); L.hout = take(tg * n);
  L.a = take(tg * H); L.b = take(tg * H); L.hid = take(tg * H); L.g2 = take(tg * n); L.dl = take(tg); L.dl2 = take(tg);
  const size_t dec_end = o;
  o = u;
  L.xln = take(ts * n); L.kv = take(ts * 2 * n); L.dkv = take(ts * 2 * n); L.gx = take(ts * n);
  const int hd = c.n_embed / c.n_head_cross, splits = cdiv(S, wide_attn_keys_per_split(hd));
  L.part = take(splits > 1 ? rows * c.n_head_cross * splits * (hd + 2) : 0);
  L.eatt = take(rows * n); L.hb0 = take(rows * n); L.et2 = take(rows * n); L.ea = take(rows * H); L.eb = take(rows * H); L.ehid = take(rows * H);
  L.tlat = take(rows * nl); L.dtlat = take(rows * nl); L.dqc = take(rows * n);
  L.bytes = o > dec_end ? o : dec_end;
  return L;
}

int plan(const scldm_vaew* h, int B, int S, int G, size_t cap, int* cells, int* chunks, size_t* bytes) {
  if (!h) return fail(SCLDM_ERR_SHAPE, "null handle");
  if (B < 1 || S < 1 || G < 1) return fail(SCLDM_ERR_SHAPE, "scldm_vaew_train_plan: B, S and G must be >= 1 (got %d, %d, %d)", B, S, G);
  if (cap == 0) cap = h->cap_bytes;
  const size_t one = layout(h->cfg, 1, S, G).bytes;
  if (one > cap)
    return fail(SCLDM_ERR_SHAPE, "wide VAE training: the record of one cell of %d tokens and %d genes needs %zu workspace bytes, above the cap of %zu (SCLDM_VAEW_WS_MB)",
                S, G, one, cap);
  const long long T = S > G ? S : G;
  if (T > kMaxTrainChunkRows) return fail(SCLDM_ERR_SHAPE, "wide VAE training: at most %lld tokens per cell (got %lld)", kMaxTrainChunkRows, T);
  long long lo = 1, hi = B;                              // the largest chunk under the cap (the layout grows with the cells)
  if (hi > 65535) hi = 65535;
  if (T * hi > kMaxTrainChunkRows) hi = kMaxTrainChunkRows / T;
  while (lo < hi) {
    const long long mid = (lo + hi + 1) / 2;
    if (layout(h->cfg, mid, S, G).bytes <= cap) lo = mid; else hi = mid - 1;
  }
  *cells = (int)lo;
  *chunks = cdiv(B, lo);
  *bytes = layout(h->cfg, lo, S, G).bytes;
  return SCLDM_OK;
}

// ---- launch helpers of the backward
struct T {
  Ctx c;
  char* ws;
  const TL* L;
  float* P;
  float* C;
  float* f(size_t off) const { return (float*)(ws + off); }
};
// out[M, N] (slot `slot` of it) = A[M, K] B[K, N]: a data gradient dY W, W as torch stores it; one k-split
void nn(const T& t, const float* A, int lda, const float* Bm, int ldb, long long M, int N, int K, float* out, int slot = 0) {
  ProdArgs p = {};
  p.A = A; p.Bm = Bm; p.lda = lda; p.ldb = ldb; p.M = (int)M; p.N = N; p.K = K; p.k_per_split = round32(K); p.out = out; p.slot0 = slot;
  scvi_train::prod_kernel<F32Operands, false, false><<<dim3(cdiv(N, kBN), cdiv(M, kBM), 1), 256, 0, t.c.st>>>(p);
}
// grad[M, N] += A[K, M]^T B[K, N]: a weight gradient dY^T X over K rows, its k-splits added in split order
void tn(const T& t, const float* A, int lda, const float* Bm, int ldb, int M, int N, long long K, const float* grad) {
  ProdArgs p = {};
  p.A = A; p.Bm = Bm; p.lda = lda; p.ldb = ldb; p.M = M; p.N = N; p.K = (int)K; p.k_per_split = tn_k_per_split(K); p.out = t.P; p.slot0 = 0;
  const int slots = tn_slots(K);
  scvi_train::prod_kernel<F32Operands, true, false><<<dim3(cdiv(N, kBN), cdiv(M, kBM), slots), 256, 0, t.c.st>>>(p);
  const size_t plane = (size_t)M * N;
  acc_slots_kernel<<<cdiv(plane, 256), 256, 0, t.c.st>>>(t.P, slots, plane, const_cast<float*>(grad));
}
void sum_slots(const T& t, const float* part, int slots, size_t plane, float* out) {
  scvi_train::sum_slots_kernel<false><<<cdiv(plane, 256), 256, 0, t.c.st>>>(part, slots, plane, out, nullptr);
}
// dx = (add) + dLN(dy) at x = LayerNorm's input; the affine's gradients += when gamma is given
void ln_bwd(const T& t, const float* src, const float* dy, const float* add, float* dx, long long rows, int n, const float* gamma,
            const float* dgamma, const float* dbeta, const int64_t* gidx = nullptr, const float* counts = nullptr) {
  LnBwdArgs a;
  a.src = src; a.gidx = gidx; a.idx_max = t.c.h->cfg.n_genes; a.counts = counts; a.w = gamma; a.dy = dy; a.add = add; a.dx = dx;
  a.part = gamma ? t.C : nullptr; a.rows = rows; a.n = n; a.eps = t.c.h->cfg.layernorm_eps;
  const int blocks = cdiv(rows, kColRows);
  ln_bwd_kernel<<<blocks, 256, 0, t.c.st>>>(a);
  if (gamma) {
    MergeArgs m = {};
    m.part = t.C; m.blocks = blocks; m.width = 2 * n;
    m.out[0] = const_cast<float*>(dgamma); m.len[0] = n; m.out[1] = const_cast<float*>(dbeta); m.len[1] = n;
    colpart_merge_kernel<<<cdiv(m.width, 256), 256, 0, t.c.st>>>(m);
  }
}
void swiglu_fwd(const T& t, const float* a, const float* b, float* hid, size_t n) { swiglu_fwd_kernel<<<cdiv(n, 256), 256, 0, t.c.st>>>(a, b, hid, n); }
void swiglu_bwd(const T& t, float* a, float* b, const float* dhid, size_t n) { swiglu_bwd_kernel<<<cdiv(n, 256), 256, 0, t.c.st>>>(a, b, dhid, n); }
void cell_sum_acc(const T& t, const float* in, int cells, size_t plane, const float* out) {
  cell_sum_acc_kernel<<<cdiv(plane, 256), 256, 0, t.c.st>>>(in, cells, plane, const_cast<float*>(out));
}
// the attention backward of one geometry: the statistics, dQ (over key splits) and dK | dV (over query splits)
void attn_bwd(const T& t, const float* Q, size_t q_bs, int q_ld, const float* K, const float* V, size_t kv_bs, int kv_ld, const float* O,
              const float* dO, int cells, int M, int S, int heads, float* dQ, int dq_ld, float* dK, float* dV, int dkv_ld) {
  AttnBwdArgs a = {};
  const int n = t.c.h->cfg.n_embed;
  a.Q = Q; a.q_bs = q_bs; a.q_ld = q_ld; a.K = K; a.V = V; a.kv_bs = kv_bs; a.kv_ld = kv_ld; a.O = O; a.dO = dO; a.o_ld = n;
  a.stats = t.f(t.L->stats); a.cells = cells; a.heads = heads; a.M = M; a.S = S; a.hd = n / heads; a.scale = 1.0f / sqrtf((float)a.hd);
  const long long qrows = (long long)cells * heads * M, krows = (long long)cells * heads * S;
  attn_stats_kernel<<<cdiv(qrows, 4), 256, 0, t.c.st>>>(a);
  a.keys_per_split = wide_attn_keys_per_split(a.hd);
  const int ks = cdiv(S, a.keys_per_split);
  a.q_plane = (size_t)cells * M * dq_ld;
  a.dQ = ks > 1 ? t.P : dQ;
  a.dq_ld = dq_ld;
  attn_bwd_q_kernel<<<dim3(cdiv(qrows, 4), ks), 256, 0, t.c.st>>>(a);
  if (ks > 1) sum_slots(t, t.P, ks, a.q_plane, dQ);      // (split geometries own the whole of dQ's rows: dq_ld == n)
  a.queries_per_split = kAttnBwdQuerySplit;
  const int qs = cdiv(M, a.queries_per_split);
  a.kv_plane = (size_t)cells * S * dkv_ld;
  a.dK = qs > 1 ? t.P : dK;
  a.dV = qs > 1 ? t.P + (dV - dK) : dV;
  a.dkv_ld = dkv_ld;
  attn_bwd_kv_kernel<<<dim3(cdiv(krows, 4), qs), 256, 0, t.c.st>>>(a);
  if (qs > 1) sum_slots(t, t.P, qs, a.kv_plane, dK);     // (dK | dV are the whole of the rows: dkv_ld == 2 n)
}

// the plain Blocks on the cells' inducing-point rows, every stage recorded (vae_wide_api.hip: trunk)
void trunk_fwd(const T& t, const std::vector<scldm_vae_block>& blocks, int cells) {
  const Ctx& c = t.c;
  const scldm_vae_config& f = c.h->cfg;
  const int n = f.n_embed, ni = f.n_inducing, H = f.hidden_dim;
  const long long rows = (long long)cells * ni;
  for (size_t l = 0; l < blocks.size(); ++l) {
    const scldm_vae_block& b = blocks[l];
    const Rec& r = t.L->layer[l];
    float *hin = t.f(t.L->hs[l]), *hout = t.f(t.L->hs[l + 1]), *qkv = t.f(r.qkv);
    ln(c, hin, t.f(r.t1), rows, n, b.ln1_w, b.ln1_b);
    store(c, t.f(r.t1), b.attn_w, qkv, rows, 3 * n, n);
    attn(c, qkv, (size_t)ni * 3 * n, 3 * n, qkv + n, qkv + 2 * n, (size_t)ni * 3 * n, 3 * n, t.f(r.att), cells, ni, ni, f.n_head);
    resid(c, t.f(r.att), b.proj_w, t.f(r.hmid), rows, n, n, hin);
    ln(c, t.f(r.hmid), t.f(r.t2), rows, n, b.ln2_w, b.ln2_b);
    store(c, t.f(r.t2), b.w1, t.f(r.a), rows, H, n);
    store(c, t.f(r.t2), b.w2, t.f(r.b), rows, H, n);
    swiglu_fwd(t, t.f(r.a), t.f(r.b), t.f(r.hid), (size_t)rows * H);
    resid(c, t.f(r.hid), b.cproj, hout, rows, n, H, t.f(r.hmid));
  }
}
// a SwiGLU MLP y = x + c_proj(SiLU(w1 t2) w2 t2), t2 = LN_2(x), walked back: dh (the gradient of y) becomes the gradient of x
void mlp_bwd(const T& t, long long rows, float* dh, const float* x, float* t2, float* a, float* b, float* hid, float* dH, float* dt,
             const float* ln_w, const float* w1, const float* w2, const float* cproj, const float* g_ln_w, const float* g_ln_b, const float* g_w1,
             const float* g_w2, const float* g_cproj) {
  const scldm_vae_config& f = t.c.h->cfg;
  const int n = f.n_embed, H = f.hidden_dim;
  tn(t, dh, n, hid, H, n, H, rows, g_cproj);
  nn(t, dh, n, cproj, H, rows, H, n, dH);
  swiglu_bwd(t, a, b, dH, (size_t)rows * H);
  tn(t, a, H, t2, n, H, n, rows, g_w1);
  tn(t, b, H, t2, n, H, n, rows, g_w2);
  nn(t, a, H, w1, n, rows, n, H, t.P, 0);
  nn(t, b, H, w2, n, rows, n, H, t.P, 1);
  sum_slots(t, t.P, 2, (size_t)rows * n, dt);
  ln_bwd(t, x, dt, dh, dh, rows, n, ln_w, g_ln_w, g_ln_b);
}
// dh (rows, n): the gradient of the trunk's output on entry, of its input on exit
void trunk_bwd(const T& t, const std::vector<scldm_vae_block>& blocks, const scldm_vae_block* g, int cells) {
  const scldm_vae_config& f = t.c.h->cfg;
  const int n = f.n_embed, ni = f.n_inducing;
  const long long rows = (long long)cells * ni;
  float *dh = t.f(t.L->dh), *dt = t.f(t.L->dt), *dqkv = t.f(t.L->dqkv), *dH = t.f(t.L->dH);
  for (int l = (int)blocks.size() - 1; l >= 0; --l) {
    const scldm_vae_block& b = blocks[l];
    const Rec& r = t.L->layer[l];
    const float* qkv = t.f(r.qkv);
    mlp_bwd(t, rows, dh, t.f(r.hmid), t.f(r.t2), t.f(r.a), t.f(r.b), t.f(r.hid), dH, dt, b.ln2_w, b.w1, b.w2, b.cproj, g[l].ln2_w, g[l].ln2_b,
            g[l].w1, g[l].w2, g[l].cproj);
    tn(t, dh, n, t.f(r.att), n, n, n, rows, g[l].proj_w);
    nn(t, dh, n, b.proj_w, n, rows, n, n, dt);
    attn_bwd(t, qkv, (size_t)ni * 3 * n, 3 * n, qkv + n, qkv + 2 * n, (size_t)ni * 3 * n, 3 * n, t.f(r.att), dt, cells, ni, ni, f.n_head, dqkv,
             3 * n, dqkv + n, dqkv + 2 * n, 3 * n);
    tn(t, dqkv, 3 * n, t.f(r.t1), n, 3 * n, n, rows, g[l].attn_w);
    nn(t, dqkv, 3 * n, b.attn_w, n, rows, n, 3 * n, dt);
    ln_bwd(t, t.f(t.L->hs[l]), dt, dh, dh, rows, n, b.ln1_w, g[l].ln1_w, g[l].ln1_b);
  }
}
}  // namespace

extern "C" int scldm_vaew_train_plan(const scldm_vaew* h, int B, int S, int G, size_t cap_bytes, int* cells_per_chunk, int* n_chunks,
                                     size_t* ws_bytes) {
  if (!cells_per_chunk || !n_chunks || !ws_bytes) return fail(SCLDM_ERR_SHAPE, "null argument");
  return plan(h, B, S, G, cap_bytes, cells_per_chunk, n_chunks, ws_bytes);
}

extern "C" size_t scldm_vaew_train_workspace_bytes(const scldm_vaew* h, int B, int S, int G) {
  int cells, chunks;
  size_t bytes;
  if (plan(h, B, S, G, 0, &cells, &chunks, &bytes)) return 0;
  return bytes;
}

extern "C" size_t scldm_vaew_train_rows_bytes(const scldm_vaew* h, int B, int S, int G) {
  if (!h || B < 1 || S < 1 || G < 1) return 0;
  return ((size_t)B * ((size_t)G + S) * h->cfg.n_embed + (size_t)B * G) * sizeof(float);
}

extern "C" int scldm_vaew_train_backward(scldm_vaew* h, const scldm_vae_weights* g, const float* counts_subset, const int64_t* genes_subset,
                                         int B, int S, const int64_t* genes, const float* library_size, int G, const float* mu,
                                         const float* theta, const float* z, const float* dmu, const float* dtheta, const float* dz,
                                         const int32_t* order, const int32_t* seg, int n_order, void* rows_, void* ws_, void* stream_) {
  if (!h) return fail(SCLDM_ERR_SHAPE, "null handle");
  if (!h->loaded) return fail(SCLDM_ERR_STATE, "scldm_vaew_load_weights has not been called");
  if (B < 1 || S < 1 || G < 1 || !g || !counts_subset || !genes_subset || !genes || !library_size || !mu || !theta || !z || !order || !seg ||
      n_order < 0 || !rows_ || !ws_)
    return fail(SCLDM_ERR_SHAPE, "scldm_vaew_train_backward: bad argument");
  if ((long long)B * ((long long)G + S) > 2147483647ll - 65) return fail(SCLDM_ERR_SHAPE, "scldm_vaew_train_backward: B * (G + S) exceeds the int32 entry index");
  const scldm_vae_config& f = h->cfg;
  const scldm_vae_weights& w = h->w;
  const bool shared = !h->unshared_theta;
  const void* need[] = {g->gene_embedding, g->inducing_points, g->enc_latent_w, g->dec_latent_w, g->head_w, g->head_b};
  for (const void* p : need)
    if (!p) return fail(SCLDM_ERR_SHAPE, "scldm_vaew_train_backward: a gradient pointer is NULL");
  if (shared && !g->theta) return fail(SCLDM_ERR_SHAPE, "scldm_vaew_train_backward: the theta table's gradient pointer is NULL");
  if (f.n_layer > 0 && (!g->enc_blocks || !g->dec_blocks)) return fail(SCLDM_ERR_SHAPE, "scldm_vaew_train_backward: the gradient block arrays are NULL");
  int cells, chunks, rc;
  size_t bytes;
  if ((rc = plan(h, B, S, G, 0, &cells, &chunks, &bytes))) return rc;
  const TL L = layout(f, cells, S, G);
  T t;
  t.c = Ctx{h, SCLDM_PREC_FP32, (hipStream_t)stream_};
  t.ws = (char*)ws_;
  t.L = &L;
  t.P = t.f(L.P);
  t.C = t.f(L.C);
  const Ctx& c = t.c;
  const scldm_vae_cross &ec = w.enc_cross, &dc = w.dec_cross, &gec = g->enc_cross, &gdc = g->dec_cross;
  const int n = f.n_embed, ni = f.n_inducing, H = f.hidden_dim, nl = f.n_embed_latent, nlay = f.n_layer;
  float* grow = (float*)rows_;                                   // (B (G + S), n): the gene table's per-entry rows
  float* trows = grow + (size_t)B * ((size_t)G + S) * n;         // (B G): the theta table's
  float *qi = t.f(L.qi), *qq = t.f(L.qq), *dqq = t.f(L.dqq), *dqi = t.f(L.dqi);
  float *dh = t.f(L.dh), *dt = t.f(L.dt), *dH = t.f(L.dH), *dzc = t.f(L.dzc);
  float *hL = t.f(L.hs[nlay]), *h0 = t.f(L.hs[0]);
  // the inducing-point queries are the same for every cell: LN_1q, then c_attn_q, once per call; dqq collects their gradient
  ln(c, w.inducing_points, qi, ni, n, ec.ln1q_w, ec.ln1q_b);
  store(c, qi, ec.attn_q, qq, ni, n, n);
  hipError_t e = hipMemsetAsync(dqq, 0, (size_t)ni * n * sizeof(float), c.st);
  if (e != hipSuccess) return fail(SCLDM_ERR_HIP, "hipMemsetAsync failed: %s", hipGetErrorString(e));
  for (int b0 = 0; b0 < B; b0 += cells) {
    const int bc = B - b0 < cells ? B - b0 : cells;
    const long long rows = (long long)bc * ni, tg = (long long)bc * G, ts = (long long)bc * S;
    const size_t og = (size_t)b0 * G, os = (size_t)b0 * S, oz = (size_t)b0 * ni * nl;
    {  // ---- 1. the decoder's record from the saved z
      float *zln = t.f(L.zln), *tt = t.f(L.t), *kvc = t.f(L.kvc), *ga = t.f(L.ga), *gq = t.f(L.gq), *gatt = t.f(L.gatt), *y = t.f(L.y);
      float *gt2 = t.f(L.gt2), *hout = t.f(L.hout), *a = t.f(L.a), *b = t.f(L.b), *hid = t.f(L.hid), *g2 = t.f(L.g2);
      float *dl = t.f(L.dl), *dl2 = t.f(L.dl2), *dzln = t.f(L.dzln), *dkvc = t.f(L.dkvc);
      ln(c, z + oz, zln, rows, nl, nullptr, nullptr);
      store(c, zln, w.dec_latent_w, h0, rows, n, nl);
      trunk_fwd(t, h->dec_blocks, bc);
      ln(c, hL, tt, rows, n, dc.ln1_w, dc.ln1_b);
      store(c, tt, dc.attn_kv, kvc, rows, 2 * n, n);
      ln(c, w.gene_embedding, ga, tg, n, dc.ln1q_w, dc.ln1q_b, genes + og);
      store(c, ga, dc.attn_q, gq, tg, n, n);
      attn(c, gq, (size_t)G * n, n, kvc, kvc + n, (size_t)ni * 2 * n, 2 * n, gatt, bc, G, ni, f.n_head_cross);
      resid(c, gatt, dc.attn_proj, y, tg, n, n, w.gene_embedding, 0, nullptr, 1, genes + og, f.n_genes);
      ln(c, y, gt2, tg, n, dc.ln2_w, dc.ln2_b);
      store(c, gt2, dc.w1, a, tg, H, n);
      store(c, gt2, dc.w2, b, tg, H, n);
      swiglu_fwd(t, a, b, hid, (size_t)tg * H);
      resid(c, hid, dc.cproj, hout, tg, n, H, y);
      LAUNCH_CHECK();
      // ---- 2. the decoder walked back.  hout becomes the carried gradient g1, hid the SwiGLU's d hid, gt2 the queries' gradient
      NbRowArgs r;
      r.mu = mu + og; r.theta = theta + og; r.dmu = dmu ? dmu + og : nullptr; r.dtheta = dtheta ? dtheta + og : nullptr;
      r.library = library_size + b0; r.G = G; r.inv_temp = 1.0f / f.nb_temperature; r.dl = dl; r.dl2 = shared ? nullptr : dl2;
      r.trows = shared ? trows + og : nullptr;
      nb_bwd_row_kernel<<<bc, 256, 0, c.st>>>(r);
      NbHArgs hh;
      hh.h = hout; hh.dl = dl; hh.dl2 = shared ? nullptr : dl2; hh.head_w = w.head_w; hh.part = t.C; hh.rows = tg; hh.n = n;
      const int hblocks = cdiv(tg, kColRows);
      nb_bwd_h_kernel<<<hblocks, 256, 0, c.st>>>(hh);
      MergeArgs m = {};
      m.part = t.C; m.blocks = hblocks; m.width = 2 * n + 2;
      float* ghw = const_cast<float*>(g->head_w);
      float* ghb = const_cast<float*>(g->head_b);
      m.out[0] = ghw; m.len[0] = n; m.out[1] = shared ? nullptr : ghw + n; m.len[1] = n; m.out[2] = ghb; m.len[2] = 1;
      m.out[3] = shared ? nullptr : ghb + 1; m.len[3] = 1;
      colpart_merge_kernel<<<cdiv(m.width, 256), 256, 0, c.st>>>(m);
      float* g1 = hout;
      mlp_bwd(t, tg, g1, y, gt2, a, b, hid, /*dH=*/hid, g2, dc.ln2_w, dc.w1, dc.w2, dc.cproj, gdc.ln2_w, gdc.ln2_b, gdc.w1, gdc.w2, gdc.cproj);
      tn(t, g1, n, gatt, n, n, n, tg, gdc.attn_proj);
      nn(t, g1, n, dc.attn_proj, n, tg, n, n, g2);                                           // d gatt
      float* dgq = gt2;
      attn_bwd(t, gq, (size_t)G * n, n, kvc, kvc + n, (size_t)ni * 2 * n, 2 * n, gatt, g2, bc, G, ni, f.n_head_cross, dgq, n, dkvc, dkvc + n, 2 * n);
      tn(t, dgq, n, ga, n, n, n, tg, gdc.attn_q);
      nn(t, dgq, n, dc.attn_q, n, tg, n, n, g2);                                             // d LN_1q(emb[g])
      // the table row of decoder slot (cell, slot): the LN_1q path + the raw-embedding residual (g1)
      ln_bwd(t, w.gene_embedding, g2, g1, grow + og * n, tg, n, dc.ln1q_w, gdc.ln1q_w, gdc.ln1q_b, genes + og);
      tn(t, dkvc, 2 * n, tt, n, 2 * n, n, rows, gdc.attn_kv);
      nn(t, dkvc, 2 * n, dc.attn_kv, n, rows, n, 2 * n, dt);
      ln_bwd(t, hL, dt, nullptr, dh, rows, n, dc.ln1_w, gdc.ln1_w, gdc.ln1_b);
      trunk_bwd(t, h->dec_blocks, g->dec_blocks, bc);
      tn(t, dh, n, zln, nl, n, nl, rows, g->dec_latent_w);
      nn(t, dh, n, w.dec_latent_w, nl, rows, nl, n, dzln);
      // ---- 3. dz = the upstream gradient + the decoder's
      ln_bwd(t, z + oz, dzln, dz ? dz + oz : nullptr, dzc, rows, nl, nullptr, nullptr, nullptr);
      LAUNCH_CHECK();
    }
    {  // ---- 4. the encoder's record from the inputs
      float *xln = t.f(L.xln), *kv = t.f(L.kv), *dkv = t.f(L.dkv), *gx = t.f(L.gx), *att = t.f(L.eatt), *hb0 = t.f(L.hb0), *t2 = t.f(L.et2);
      float *a = t.f(L.ea), *b = t.f(L.eb), *hid = t.f(L.ehid), *tlat = t.f(L.tlat), *dtlat = t.f(L.dtlat), *dqc = t.f(L.dqc);
      ln(c, w.gene_embedding, xln, ts, n, ec.ln1_w, ec.ln1_b, genes_subset + os, counts_subset + os);
      store(c, xln, ec.attn_kv, kv, ts, 2 * n, n);
      attn(c, qq, 0, n, kv, kv + n, (size_t)S * 2 * n, 2 * n, att, bc, ni, S, f.n_head_cross, t.f(L.part));
      resid(c, att, ec.attn_proj, hb0, rows, n, n, w.inducing_points, ni);
      ln(c, hb0, t2, rows, n, ec.ln2_w, ec.ln2_b);
      store(c, t2, ec.w1, a, rows, H, n);
      store(c, t2, ec.w2, b, rows, H, n);
      swiglu_fwd(t, a, b, hid, (size_t)rows * H);
      resid(c, hid, ec.cproj, h0, rows, n, H, hb0, 0, f.positional_encoding ? w.enc_pos_embed : nullptr, ni);
      trunk_fwd(t, h->enc_blocks, bc);
      store(c, hL, w.enc_latent_w, tlat, rows, nl, n);
      LAUNCH_CHECK();
      // ---- 5. the encoder walked back
      ln_bwd(t, tlat, dzc, nullptr, dtlat, rows, nl, nullptr, nullptr, nullptr);
      tn(t, dtlat, nl, hL, n, nl, n, rows, g->enc_latent_w);
      nn(t, dtlat, nl, w.enc_latent_w, n, rows, n, nl, dh);
      trunk_bwd(t, h->enc_blocks, g->enc_blocks, bc);
      mlp_bwd(t, rows, dh, hb0, t2, a, b, hid, dH, dt, ec.ln2_w, ec.w1, ec.w2, ec.cproj, gec.ln2_w, gec.ln2_b, gec.w1, gec.w2, gec.cproj);
      cell_sum_acc(t, dh, bc, (size_t)ni * n, g->inducing_points);                           // the residual is the raw query
      tn(t, dh, n, att, n, n, n, rows, gec.attn_proj);
      nn(t, dh, n, ec.attn_proj, n, rows, n, n, dt);
      attn_bwd(t, qq, 0, n, kv, kv + n, (size_t)S * 2 * n, 2 * n, att, dt, bc, ni, S, f.n_head_cross, dqc, n, dkv, dkv + n, 2 * n);
      cell_sum_acc(t, dqc, bc, (size_t)ni * n, dqq);
      tn(t, dkv, 2 * n, xln, n, 2 * n, n, ts, gec.attn_kv);
      nn(t, dkv, 2 * n, ec.attn_kv, n, ts, n, 2 * n, gx);
      // the table row of encoder token (cell, tok): its LN_1 gradient times log1p(count)
      ln_bwd(t, w.gene_embedding, gx, nullptr, grow + ((size_t)B * G + os) * n, ts, n, ec.ln1_w, gec.ln1_w, gec.ln1_b, genes_subset + os,
             counts_subset + os);
      LAUNCH_CHECK();
    }
  }
  // ---- the batch-independent pieces: the shared queries' gradient, summed over the cells, goes back once
  tn(t, dqq, n, qi, n, n, n, ni, gec.attn_q);
  nn(t, dqq, n, ec.attn_q, n, ni, n, n, dqi);
  ln_bwd(t, w.inducing_points, dqi, g->inducing_points, const_cast<float*>(g->inducing_points), ni, n, ec.ln1q_w, gec.ln1q_w, gec.ln1q_b);
  // ---- the two tables: fixed-order segmented sums over the caller's index
  table_rows_sum_kernel<<<f.n_genes + 1, 256, 0, c.st>>>(grow, order, seg, n, const_cast<float*>(g->gene_embedding));
  if (shared)
    theta_rows_sum_kernel<<<cdiv(f.n_genes + 1, 256), 256, 0, c.st>>>(trows, order, seg, f.n_genes + 1, B * G, const_cast<float*>(g->theta));
  LAUNCH_CHECK();
  return SCLDM_OK;
}

// C ABI of libscldm_hip.so (see include/scldm_hip.h).  gfx950 only; no torch dependency.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <cmath>
#include "api_common.hpp"
#include "cfg_plan.hpp"
#include "dit_aux.hpp"
#include "dit_forward.hpp"
#include "dit_handle.hpp"
#include "ode_rk.hpp"
#include "sde.hpp"
#include "transport_path.hpp"
#include "sde_transport.hpp"
#include "dopri5_ctl.hpp"
#include "dopri5_fused.hpp"
#include "fixed_grid.hpp"

using namespace scldm;

static thread_local char g_err[512] = "";
int scldm_fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}
static inline int pad8(int n) { return (n + 7) & ~7; }  // sample-forwards per 128-token tile


extern "C" const char* scldm_last_error(void) { return g_err; }
// 3: SCLDM_PREC_FP16, scldm_dit_fp16_stats, scldm_dit_train_prepare, forward_cfg t_stride 2
// 4 (round 6): SCLDM_PREC_FP16 on the scldm_vae_* entry points, unshared-theta head (theta == NULL), scldm_dit_train_step / scldm_fm_prepare /
//    scldm_fm_loss_grad, the scldm_adamw_table_* family, scldm_vae_kernel_timing
// added under 5 (no prototype or struct offset moved, the ABI tests pin the number): the scldm_vae_train_* entries take a handle with
//    the unshared-theta head (they returned SCLDM_ERR_STATE for it)
extern "C" int scldm_version(void) { return 5; }
//   // 2: has_null_row in scldm_dit_config, SCLDM_PREC_BF16X3, refresh_weights / label_errors

static size_t esize(int prec) { return (prec == SCLDM_PREC_BF16 || prec == SCLDM_PREC_FP16) ? 2 : 4; }  // bytes per packed weight element (split-bf16: hi + lo)
static const int kNPrec = 4;

// Kernel shape: (token tiles of 32*NTT, FT feature tiles per wave => 8/FT waves per workgroup).
//   fp32   : NTT=2, FT=2 (4 waves, one per SIMD, 512-register budget)
//   bf16   : NTT=2, FT=2, two workgroups per CU by default; FT=1 (8 waves, one head each) stays selectable through SCLDM_FT
//            for A/B runs.  128-token tiles (NTT=4) were measured with both wave shapes and dropped: FT=2 needs the 512-register
//            budget of one wave per SIMD and loses the second workgroup (450 vs 337 us per layer, round 1), FT=1 keeps eight
//            lockstep waves and still spills (1594 vs 1270 us per 4-layer launch, round 2)
//   bf16x3 : NTT=2, FT=2 (one workgroup per CU: 155 KB of LDS); SCLDM_X3_FT=1 selects the 8-wave shape
static void pick_shape(const scldm_dit* h, int prec, int* ntt, int* ft) {
  *ntt = 2;
  *ft = 2;
  if (prec == SCLDM_PREC_BF16 || prec == SCLDM_PREC_FP16) {   // fp16: the bf16 kernel's shape, layout and schedule
    if (h->force_ft == 1 || h->force_ft == 2) *ft = h->force_ft;
  } else if (prec == SCLDM_PREC_BF16X3) {
    if (h->force_x3_ft == 1) *ft = 1;
    else if (h->force_x3_ntt == 1) *ntt = 1;   // 32-token tiles: 79 KB of LDS, two workgroups per CU
  }
}

extern "C" int scldm_dit_create(const scldm_dit_config* cfg, scldm_dit** out) {
  if (!cfg || !out) return fail(SCLDM_ERR_SHAPE, "null argument");
  if (cfg->n_embed < 1 || cfg->n_head < 1 || cfg->seq_len < 1) return fail(SCLDM_ERR_SHAPE, "bad n_embed / n_head / seq_len");
  // The fused inference layer is specialised to the reference's DiT shape family; any other shape gets a handle that only
  // serves the generic (GEMM-based) scldm_dit_train_* path, and the fused entry points report SCLDM_ERR_SHAPE.
  const bool fused = cfg->n_embed == 256 && cfg->n_head == 8 && cfg->seq_len == 16 && cfg->n_embed_input <= 32;
  if (cfg->n_embed_input < 1) return fail(SCLDM_ERR_SHAPE, "n_embed_input must be >= 1");
  if (!fused) {
    const int hd = cfg->n_embed % cfg->n_head == 0 ? cfg->n_embed / cfg->n_head : 0;
    if (cfg->n_embed % 256 != 0 || cfg->n_embed > 2048 || cfg->seq_len != 16 || (hd != 32 && hd != 64))
      return fail(SCLDM_ERR_SHAPE, "unsupported DiT shape: fused kernels need n_embed=256, n_head=8, seq_len=16; the generic path needs "
                  "n_embed %% 256 == 0 (<= 2048), seq_len=16, head_dim 32 or 64 (got n_embed=%d, n_head=%d, seq_len=%d)", cfg->n_embed,
                  cfg->n_head, cfg->seq_len);
  }
  if (cfg->n_layer < 1 || cfg->hidden_dim < 1) return fail(SCLDM_ERR_SHAPE, "bad n_layer / hidden_dim");
  if (cfg->n_classes < 0 || cfg->n_classes > SCLDM_MAX_CLASSES) return fail(SCLDM_ERR_SHAPE, "n_classes must be <= %d", SCLDM_MAX_CLASSES);
  if (cfg->has_null_row != 0 && cfg->has_null_row != 1) return fail(SCLDM_ERR_SHAPE, "has_null_row must be 0 or 1");
  for (int c = 0; c < cfg->n_classes; ++c)
    if (cfg->class_vocab[c] < 1) return fail(SCLDM_ERR_SHAPE, "class %d has an empty vocabulary", c);
  scldm_dit* h = new scldm_dit();   // value-initialised: every pointer NULL, every counter 0
  h->cfg = *cfg;
  h->fused = fused;
  h->mod_w = cfg->n_layer * 6 * cfg->n_embed + 2 * cfg->n_embed;
  for (int c = 0; c < cfg->n_classes; ++c) h->tab_rows[c] = cfg->class_vocab[c] + cfg->has_null_row;
  h->bf16_sources = true;   // (a knob of the generic training path: read for every shape)
  if (const char* e = getenv("SCLDM_TRAIN_BF16_SOURCES")) h->bf16_sources = atoi(e) != 0;
  h->wgrad_batch = true;
  if (const char* e = getenv("SCLDM_WGRAD_BATCH")) h->wgrad_batch = atoi(e) != 0;
  if (!fused) {
    *out = h;
    return SCLDM_OK;
  }
  // run-time knobs are read ONCE, here (they select kernel shapes and therefore which weight streams exist)
  if (const char* e = getenv("SCLDM_FWD_MFMA")) h->fwd_m16 = atoi(e) != 32;
  if (const char* e = getenv("SCLDM_FT")) h->force_ft = atoi(e);
  if (const char* e = getenv("SCLDM_X3_FT")) h->force_x3_ft = atoi(e);
  if (const char* e = getenv("SCLDM_X3_NTT")) h->force_x3_ntt = atoi(e);
  if (const char* e = getenv("SCLDM_SMALL_NTT")) h->small_ntt = atoi(e) != 0;
  h->lpl = kMaxLayersPerLaunch;   // layers per fused launch (SCLDM_LPL=1..kMaxLayersPerLaunch for A/B runs)
  if (const char* e = getenv("SCLDM_LPL")) h->lpl = std::min(kMaxLayersPerLaunch, std::max(1, atoi(e)));
  h->groups = 1;
  if (const char* e = getenv("SCLDM_ADALN_VALU")) h->adaln_valu = atoi(e) != 0;
  if (const char* e = getenv("SCLDM_ADALN_EXACT")) h->adaln_exact = atoi(e) != 0;
  if (const char* e = getenv("SCLDM_ADALN_ROWTILE")) h->adaln_rowtile = atoi(e) != 0;
  if (const char* e = getenv("SCLDM_COND_ALL")) h->cond_all_on = atoi(e) != 0;
  if (const char* e = getenv("SCLDM_GROUPS")) h->groups = std::min(4, std::max(1, atoi(e)));
  if (const char* e = getenv("SCLDM_TAIL_SPLIT")) h->tail_split = atoi(e) != 0;
  {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
      h->n_cu = prop.multiProcessorCount;
  }
  h->dbg_layer = -1;
  if (const char* e = getenv("SCLDM_DBG_LAYER")) h->dbg_layer = atoi(e);
  h->train_fused = true;
  if (const char* e = getenv("SCLDM_TRAIN_FUSED")) h->train_fused = atoi(e) != 0;
  if (const char* e = getenv("SCLDM_WGRAD_SPLITS")) h->wgrad_splits = atoi(e);
  h->bwd_dbg = getenv("SCLDM_BWD_DBG") != nullptr;
  h->n_chunks[0] = (cfg->hidden_dim + kHC - 1) / kHC;  // FT=1: pad the hidden dimension to whole chunks
  h->half[0] = 0;
  {
    int hp = (cfg->hidden_dim + 63) / 64 * 64;     // FT=2: pad to 64, last chunk may be a half chunk
    if (getenv("SCLDM_PAD128")) hp = (cfg->hidden_dim + 127) / 128 * 128;   // A/B switch: whole chunks only, no trailing half chunk
    h->n_chunks[1] = hp / kHC;
    h->half[1] = (hp % kHC) / 64;
  }
  auto alloc = [&](void** p, size_t bytes) { return hipMalloc(p, bytes); };
  const int L = cfg->n_layer, din = cfg->n_embed_input;
  hipError_t e = hipSuccess;
  for (int p = 0; p < kNPrec && e == hipSuccess; ++p) {
    const size_t es = esize(p);
    int ntt, ft;
    pick_shape(h, p, &ntt, &ft);   // only the stream of the shape this precision will run is packed
    const int f = ft - 1;
    const size_t elems = ((size_t)4 * L * units_per_layer(h->n_chunks[f], h->half[f]) + kMaxPF) * 1024;  // + ring over-read slack
    if ((e = alloc(&h->stream[p][f], elems * es)) != hipSuccess) break;
    if ((e = hipMemset(h->stream[p][f], 0, elems * es)) != hipSuccess) break;
    if ((e = alloc(&h->wfinal[p], 16 * 512 * es)) != hipSuccess) break;
  }
  if (e == hipSuccess && cfg->hidden_dim <= kBwdChunks * kBwdChunk) {   // backward weight stream of the fused training path (bf16, 23 MB at 8 layers)
    const size_t elems = ((size_t)L * 8 * kBwdUnitsLayer + kMaxPF) * 512;   // + ring over-read slack
    e = alloc(&h->bwd_stream, elems * 2);
    if (e == hipSuccess) e = hipMemset(h->bwd_stream, 0, elems * 2);
  }
  if (e == hipSuccess) e = alloc((void**)&h->b_qkv, (size_t)L * 768 * 4);
  if (e == hipSuccess) e = alloc((void**)&h->b_proj, (size_t)L * 256 * 4);
  int emb_rows = 0;
  for (int c = 0; c < cfg->n_classes; ++c) {
    h->emb_row0[c] = emb_rows;
    emb_rows += h->tab_rows[c];
  }
  if (e == hipSuccess) e = alloc((void**)&h->w0t, 256 * 256 * 4);
  if (e == hipSuccess) e = alloc((void**)&h->b0, 256 * 4);
  if (e == hipSuccess) e = alloc((void**)&h->w2t, 256 * 256 * 4);
  if (e == hipSuccess) e = alloc((void**)&h->b2, 256 * 4);
  if (e == hipSuccess) e = alloc((void**)&h->emb, (size_t)(emb_rows > 0 ? emb_rows : 1) * 256 * 4);
  if (e == hipSuccess) e = alloc((void**)&h->ada_t, (size_t)256 * h->mod_w * 4);
  if (e == hipSuccess) e = alloc((void**)&h->ada_b, (size_t)h->mod_w * 4);
  if (e == hipSuccess) e = alloc((void**)&h->ada_x3, (size_t)256 * h->mod_w * 4);
  if (e == hipSuccess) e = alloc((void**)&h->in_wt, (size_t)din * 256 * 4);
  if (e == hipSuccess) e = alloc((void**)&h->in_w, (size_t)din * 256 * 4);
  if (e == hipSuccess) e = alloc((void**)&h->in_b, 256 * 4);
  if (e == hipSuccess) e = alloc((void**)&h->pos, 16 * 256 * 4);
  if (e == hipSuccess) e = alloc((void**)&h->fin_b, (size_t)din * 4);
  if (e == hipSuccess) e = alloc((void**)&h->d_plan, 8);
  if (e == hipSuccess) e = alloc((void**)&h->d_fp16_stats, 16);
  if (e == hipSuccess) e = hipMemset(h->d_fp16_stats, 0, 16);
  if (e == hipSuccess) e = alloc((void**)&h->d_ls, 64);
  if (e == hipSuccess) e = hipMemset(h->d_ls, 0, 64);
  if (e == hipSuccess) e = alloc((void**)&h->label_err, 4);
  if (e == hipSuccess) e = hipMemset(h->label_err, 0, 4);
  if (e == hipSuccess) e = alloc((void**)&h->d_fp_state, 16);
  if (e == hipSuccess) e = hipMemset(h->d_fp_state, 0, 16);
  if (e == hipSuccess) e = alloc((void**)&h->d_dirty, 8);
  if (e == hipSuccess) e = hipMemset(h->d_dirty, 0, 8);
  if (e == hipSuccess) e = hipHostMalloc((void**)&h->rk_host, 32, hipHostMallocDefault);   // read-back slot of scldm_sample_ode_dopri5
  if (e != hipSuccess) {
    int rc = fail(SCLDM_ERR_HIP, "hipMalloc failed in scldm_dit_create: %s", hipGetErrorString(e));
    scldm_dit_destroy(h);
    return rc;
  }
  *out = h;
  return SCLDM_OK;
}

extern "C" void scldm_dit_destroy(scldm_dit* h) {
  if (!h) return;
  for (int p = 0; p < kNPrec; ++p) {
    for (int f = 0; f < 2; ++f)
      if (h->stream[p][f]) (void)hipFree(h->stream[p][f]);
    if (h->wfinal[p]) (void)hipFree(h->wfinal[p]);
  }
  void* ptrs[] = {h->ada_x3, h->w0t, h->b0, h->w2t, h->b2, h->emb, h->ada_t, h->ada_b, h->in_wt, h->in_w, h->in_b, h->pos, h->fin_b, h->b_qkv,
                  h->b_proj, h->label_err, h->d_plan, h->d_ls, h->d_fp16_stats, h->d_jobs, h->d_fp_src, h->d_fp_state, h->d_dirty, h->bwd_stream, h->d_tjobs, h->iota, h->w16, h->wt16, h->d_cast_jobs, h->ada16, h->ada_ball, h->d_infer_jobs};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  for (hipEvent_t ev : h->ev) (void)hipEventDestroy(ev);
  for (int g = 0; g < 2; ++g)
    if (h->wg_ev[g]) (void)hipEventDestroy(h->wg_ev[g]);
  for (int g = 0; g < 3; ++g) {
    if (h->side[g]) (void)hipStreamDestroy(h->side[g]);
    if (h->join_ev[g]) (void)hipEventDestroy(h->join_ev[g]);
  }
  if (h->fork_ev) (void)hipEventDestroy(h->fork_ev);
  if (h->bwd_pack_ev) (void)hipEventDestroy(h->bwd_pack_ev);
  if (h->cond_all) (void)hipFree(h->cond_all);
  if (h->rk_host) (void)hipHostFree(h->rk_host);
  delete h;
}

extern "C" int scldm_dit_mod_width(const scldm_dit* h) { return h ? h->mod_w : 0; }
extern "C" int scldm_dit_layers_per_launch(const scldm_dit* h) { return (h && h->fused) ? h->lpl : 0; }
extern "C" int scldm_dit_set_option(scldm_dit* h, int option, int value) {
  if (!h) return fail(SCLDM_ERR_SHAPE, "null handle");
  if (option == SCLDM_OPT_CFG1_DIRECT) { h->cfg1_direct = value != 0; return SCLDM_OK; }
  if (option == SCLDM_OPT_TAIL_SPLIT) { h->tail_split = value != 0; return SCLDM_OK; }
  return fail(SCLDM_ERR_SHAPE, "unknown option %d", option);
}

// fingerprint the parameter tensors, compare with the fingerprint of the packed copies, re-pack if they differ (all on
// device, in stream order; `force` makes the first pack after scldm_dit_load_weights unconditional)
// prec_mask: which streams to refresh (bit p: precision p's forward stream; 0x100: the backward stream); anything but "all"
// leaves the other streams stale, so the next full refresh is forced
static const unsigned kPackAll = 0x1ffu;   // bits 0..3: the four precisions' forward streams, bit 8: the backward stream
int scldm_run_pack(scldm_dit* h, bool force, unsigned prec_mask, hipStream_t st) {
  if (prec_mask == kPackAll && h->partial_pack) {
    force = true;
    h->partial_pack = false;
  }
  if (prec_mask != kPackAll) {
    // training step: only the streams it reads, from the dense training table, unconditionally (no fingerprint pass)
    h->partial_pack = true;
    pack_jobs_kernel<<<h->tjob_blocks, 256, 0, st>>>((const PackJob*)h->d_tjobs, h->n_tjobs, nullptr, prec_mask);
    LAUNCH_CHECK();
    return SCLDM_OK;
  }
  if (force) set_word_kernel<<<1, 1, 0, st>>>(h->d_dirty + 1, 1);   // (not a memcpy from a host stack variable: it must stay stream-ordered and asynchronous)
  fingerprint_kernel<<<dim3(h->n_fp, kFpSplit), 256, 0, st>>>((const FpSrc*)h->d_fp_src, h->d_fp_state);
  fingerprint_compare_kernel<<<1, 1, 0, st>>>(h->d_fp_state, h->d_dirty, h->d_fp16_stats);
  pack_jobs_kernel<<<h->job_blocks, 256, 0, st>>>((const PackJob*)h->d_jobs, h->n_jobs, h->d_dirty, prec_mask, h->d_fp16_stats);
  LAUNCH_CHECK();
  return SCLDM_OK;
}
static int run_pack(scldm_dit* h, bool force, hipStream_t st) { return scldm_run_pack(h, force, kPackAll, st); }

extern "C" int scldm_dit_load_weights(scldm_dit* h, const scldm_dit_weights* w, void* stream_) {
  if (!h || !w) return fail(SCLDM_ERR_SHAPE, "null argument");
  if (!h->fused)
    return fail(SCLDM_ERR_SHAPE, "fused DiT layer supports n_embed=256, n_head=8, seq_len=16, n_embed_input<=32 (got %d,%d,%d,%d); "
                "this shape is served by scldm_dit_train_forward / _backward only", h->cfg.n_embed, h->cfg.n_head, h->cfg.seq_len,
                h->cfg.n_embed_input);
  hipStream_t st = (hipStream_t)stream_;
  h->tables_built = false;   // an explicit load always rebuilds the tables (the caller may have re-allocated its parameters in place)
  int rc = scldm_build_pack_tables(h, w, st);
  if (rc) return rc;
  if ((rc = run_pack(h, true, st))) return rc;
  h->loaded = true;
  return SCLDM_OK;
}

int scldm_build_pack_tables(scldm_dit* h, const scldm_dit_weights* w, hipStream_t st) {
  const scldm_dit_config& c = h->cfg;
  const int L = c.n_layer, din = c.n_embed_input, H = c.hidden_dim, mw = h->mod_w;
  // the per-layer members are host arrays (re-created by the caller for every call): the key is the device pointers themselves
  std::vector<const void*> key = {w->pos_embed, w->t_w0, w->t_b0, w->t_w2, w->t_b2, w->in_w, w->in_b, w->fin_w, w->fin_b, w->fin_ada_w,
                                  w->fin_ada_b, h->bwd_stream};
  for (int ci = 0; ci < c.n_classes; ++ci) key.push_back(w->class_emb[ci]);
  for (int i = 0; i < L; ++i)
    for (const float* const* arr : {w->attn_w, w->attn_b, w->proj_w, w->proj_b, w->w1, w->w2, w->cproj, w->ada_w, w->ada_b}) key.push_back(arr[i]);
  if (h->tables_built && key == h->table_key) return SCLDM_OK;
  std::vector<PackJob> jobs, tjobs;   // tjobs: the subset the fused bf16 training step reads (its own dense block numbering)
  std::vector<FpSrc> fps;
  int blocks = 0, tblocks = 0;
  bool train = false;   // current job also goes into the training table
  auto add = [&](int kind, long long n, std::initializer_list<const float*> src, void* dst, std::initializer_list<int> par,
                 long long d_off = 0) {
    PackJob j{};
    j.kind = kind;
    j.first_block = blocks;
    j.n = n;
    int i = 0;
    for (const float* p : src) j.s[i++] = p;
    j.d = dst;
    i = 0;
    for (int v : par) j.p[i++] = v;
    j.d_off = d_off;
    const int nb = cdiv(pack_job_threads(kind, n, j.p), 256);
    blocks += nb;
    jobs.push_back(j);
    if (train) {
      j.first_block = tblocks;
      tblocks += nb;
      tjobs.push_back(j);
    }
  };
  auto src = [&](const float* p, long long n) { fps.push_back(FpSrc{(const uint32_t*)p, n}); return p; };
  for (int i = 0; i < L; ++i) {
    src(w->attn_w[i], 768 * 256); src(w->proj_w[i], 256 * 256); src(w->w1[i], (long long)H * 256); src(w->w2[i], (long long)H * 256);
    src(w->cproj[i], (long long)H * 256);
    for (int p = 0; p < kNPrec; ++p)
      for (int f = 0; f < 2; ++f) {
        if (!h->stream[p][f]) continue;
        const int nc = h->n_chunks[f], hf = h->half[f];
        const long long npk = (long long)4 * units_per_layer(nc, hf) * 1024;
        train = (p == SCLDM_PREC_BF16 || p == SCLDM_PREC_FP16) && f == 1;   // (the training launch masks the precision it runs in)
        const int m16 = h->fwd_m16 && f == 1 && (p == SCLDM_PREC_BF16 || p == SCLDM_PREC_FP16);   // = the kernels' M16
        add(kPackLayer, npk, {w->attn_w[i], w->proj_w[i], w->w1[i], w->w2[i], w->cproj[i]}, h->stream[p][f], {H, nc, hf, f + 1, p, m16}, npk * i);
        train = false;
      }
    if (h->bwd_stream) {
      const long long npk = (long long)8 * kBwdUnitsLayer * 512;
      train = true;
      add(kPackLayerBwd, npk, {w->attn_w[i], w->proj_w[i], w->w1[i], w->w2[i], w->cproj[i]}, h->bwd_stream, {H}, npk * i);
    }
    train = true;
    add(kPackCopy, 768, {src(w->attn_b[i], 768)}, h->b_qkv + (size_t)i * 768, {});
    add(kPackCopy, 256, {src(w->proj_b[i], 256)}, h->b_proj + (size_t)i * 256, {});
    // adaLN of block i -> columns [i*1536, (i+1)*1536) of the all-layer matrix
    add(kPackTranspose, 1536 * 256, {src(w->ada_w[i], 1536 * 256)}, h->ada_t, {1536, 256, mw, i * 1536});
    add(kPackCopy, 1536, {src(w->ada_b[i], 1536)}, h->ada_b + i * 1536, {});
    train = false;
    add(kPackAdaX3, 1536 * 256, {w->ada_w[i]}, h->ada_x3, {i * 1536});
  }
  train = true;
  add(kPackTranspose, 512 * 256, {src(w->fin_ada_w, 512 * 256)}, h->ada_t, {512, 256, mw, L * 1536});
  add(kPackCopy, 512, {src(w->fin_ada_b, 512)}, h->ada_b + L * 1536, {});
  train = false;
  add(kPackAdaX3, 512 * 256, {w->fin_ada_w}, h->ada_x3, {L * 1536});
  add(kPackTranspose, 256 * 256, {src(w->t_w0, 256 * 256)}, h->w0t, {256, 256, 256, 0});
  add(kPackTranspose, 256 * 256, {src(w->t_w2, 256 * 256)}, h->w2t, {256, 256, 256, 0});
  add(kPackCopy, 256, {src(w->t_b0, 256)}, h->b0, {});
  add(kPackCopy, 256, {src(w->t_b2, 256)}, h->b2, {});
  add(kPackTranspose, 256 * din, {src(w->in_w, 256 * din)}, h->in_wt, {256, din, 256, 0});
  train = true;
  add(kPackCopy, 256 * din, {w->in_w}, h->in_w, {});
  add(kPackCopy, 256, {src(w->in_b, 256)}, h->in_b, {});
  add(kPackCopy, 16 * 256, {src(w->pos_embed, 16 * 256)}, h->pos, {});
  train = false;
  src(w->fin_w, (long long)din * 256);
  for (int p = 0; p < kNPrec; ++p) {
    train = p == SCLDM_PREC_BF16 || p == SCLDM_PREC_FP16;
    add(kPackFinal, 16 * 512, {w->fin_w}, h->wfinal[p], {din, p});
  }
  train = true;
  add(kPackCopy, din, {src(w->fin_b, din)}, h->fin_b, {});
  train = false;
  for (int ci = 0; ci < c.n_classes; ++ci) {
    const int n = h->tab_rows[ci] * 256;
    add(kPackCopy, n, {src(w->class_emb[ci], n)}, h->emb + (size_t)h->emb_row0[ci] * 256, {});
  }
  // the tables may still be read by a previous refresh on this stream: drain it, then replace them (rare call)
  HIP_TRY(hipStreamSynchronize(st));
  if ((int)jobs.size() > h->jobs_cap) {
    if (h->d_jobs) (void)hipFree(h->d_jobs);
    h->d_jobs = nullptr;
    HIP_TRY(hipMalloc(&h->d_jobs, jobs.size() * sizeof(PackJob)));
    h->jobs_cap = (int)jobs.size();
  }
  if ((int)fps.size() > h->fp_cap) {
    if (h->d_fp_src) (void)hipFree(h->d_fp_src);
    h->d_fp_src = nullptr;
    HIP_TRY(hipMalloc(&h->d_fp_src, fps.size() * sizeof(FpSrc)));
    h->fp_cap = (int)fps.size();
  }
  HIP_TRY(hipMemcpy(h->d_jobs, jobs.data(), jobs.size() * sizeof(PackJob), hipMemcpyHostToDevice));
  if (h->d_tjobs) (void)hipFree(h->d_tjobs);
  h->d_tjobs = nullptr;
  HIP_TRY(hipMalloc(&h->d_tjobs, tjobs.size() * sizeof(PackJob)));
  HIP_TRY(hipMemcpy(h->d_tjobs, tjobs.data(), tjobs.size() * sizeof(PackJob), hipMemcpyHostToDevice));
  h->n_tjobs = (int)tjobs.size();
  h->tjob_blocks = tblocks;
  HIP_TRY(hipMemcpy(h->d_fp_src, fps.data(), fps.size() * sizeof(FpSrc), hipMemcpyHostToDevice));
  h->n_jobs = (int)jobs.size();
  h->job_blocks = blocks;
  h->n_fp = (int)fps.size();
  h->table_key = key;
  h->tables_built = true;
  return SCLDM_OK;
}

extern "C" int scldm_dit_refresh_weights(scldm_dit* h, void* stream_) {
  if (!h) return fail(SCLDM_ERR_SHAPE, "null handle");
  if (!h->loaded) return fail(SCLDM_ERR_STATE, "scldm_dit_load_weights has not been called");
  return run_pack(h, false, (hipStream_t)stream_);
}

extern "C" int scldm_dit_train_fp16_state(scldm_dit* h, float* scale, long long* nonfinite_last, int* headroom, long long* overflow_steps, void* stream_) {
  if (!h) return fail(SCLDM_ERR_SHAPE, "scldm_dit_train_fp16_state: null handle");
  hipStream_t st = (hipStream_t)stream_;
  unsigned v[16] = {0};
  HIP_TRY(hipMemcpyAsync(v, h->d_ls, sizeof(v), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  float S;
  memcpy(&S, &v[0], 4);
  if (scale) *scale = S;
  if (nonfinite_last) *nonfinite_last = (long long)(int)v[2];
  if (headroom) *headroom = (int)v[3];
  if (overflow_steps) *overflow_steps = (long long)(int)v[7];
  return SCLDM_OK;
}
extern "C" int scldm_dit_train_set_found_inf(scldm_dit* h, float* found_inf) {
  if (!h) return fail(SCLDM_ERR_SHAPE, "scldm_dit_train_set_found_inf: null handle");
  h->found_inf = found_inf;
  return SCLDM_OK;
}

extern "C" int scldm_dit_fp16_stats(scldm_dit* h, long long* overflow, long long* subnormal, long long* nonzero, void* stream_) {
  if (!h || !overflow || !subnormal || !nonzero) return fail(SCLDM_ERR_SHAPE, "null argument");
  *overflow = *subnormal = *nonzero = 0;
  if (!h->d_fp16_stats) return SCLDM_OK;
  hipStream_t st = (hipStream_t)stream_;
  int v[4] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(v, h->d_fp16_stats, 12, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  *overflow = v[0];
  *subnormal = v[1];
  *nonzero = v[2];
  return SCLDM_OK;
}

extern "C" int scldm_dit_label_errors(scldm_dit* h, int* count, void* stream_) {
  if (!h || !count) return fail(SCLDM_ERR_SHAPE, "null argument");
  *count = 0;
  if (!h->label_err) return SCLDM_OK;
  hipStream_t st = (hipStream_t)stream_;
  HIP_TRY(hipMemcpyAsync(count, h->label_err, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemsetAsync(h->label_err, 0, 4, st));
  HIP_TRY(hipStreamSynchronize(st));
  return SCLDM_OK;
}

// ------------------------------------------------------------------------------------------------
static const int kMaxTembEvals = 4096;  // solves with more evaluations embed t step by step
struct Ws {
  float* h;       // (pad8(n_fwd)*16, 256) residual between layer launches
  float* v;       // (n_fwd, 16*din)
  float* mod;     // (n_rows, mod_w)
  float* silu;    // (n_rows, 256)
  void* asplit;   // (pad32(n_rows), 256) split-bf16 A fragments of the conditioning rows (adaln_x3_block_kernel)
  float* temb;    // (256) timestep embedding shared by all rows of a scalar-t step
  int32_t* ridx;  // (n_fwd)
  float* dz;      // (n_state, e)
  float* k2;      // (n_state, e)
  float* ztmp;    // (n_state, e)
  size_t total;
};
static Ws carve(const scldm_dit* h, void* base, int n_fwd, int n_rows, int n_state) {
  Ws w;
  char* p = (char*)base;
  size_t off = 0;
  const size_t e = (size_t)16 * h->cfg.n_embed_input;
  auto take = [&](size_t bytes) { char* r = p + off; off += align256(bytes); return r; };
  w.h = (float*)take((size_t)pad8(n_fwd) * 16 * 256 * 4);
  w.v = (float*)take((size_t)n_fwd * e * 4);
  w.mod = (float*)take((size_t)n_rows * h->mod_w * 4);
  w.silu = (float*)take((size_t)(n_rows + 1) * 256 * 4);  // +1 spare row (device scalar t)
  w.asplit = take((size_t)((n_rows + 31) / 32 * 32) * 256 * 4);
  w.temb = (float*)take((size_t)kMaxTembEvals * 256 * 4);  // per-evaluation timestep embeddings of a whole solve
  w.ridx = (int32_t*)take((size_t)n_fwd * 4);
  w.dz = (float*)take((size_t)n_state * e * 4);
  w.k2 = (float*)take((size_t)n_state * e * 4);
  w.ztmp = (float*)take((size_t)n_state * e * 4);
  w.total = off;
  return w;
}
extern "C" size_t scldm_dit_workspace_bytes(const scldm_dit* h, int n_fwd, int n_rows, int n_state) {
  if (!h) return 0;
  return carve(h, nullptr, n_fwd, n_rows, n_state).total;
}

// conditioning rows -> silu_c rows [row0, row0+rows)
static int launch_cond(scldm_dit* h, const float* t, int t_stride, const int64_t* const* labels, uint32_t mask, int rows,
                       float* silu_c, hipStream_t st, const int* gate = nullptr, int gate_want = 0, const int32_t* row_map = nullptr) {
  if (rows <= 0) return SCLDM_OK;
  if (!h->cfg.has_null_row)
    for (int c = 0; c < h->cfg.n_classes; ++c)
      if (!(labels && labels[c] && ((mask >> c) & 1u)))
        return fail(SCLDM_ERR_SHAPE, "class %d needs its null token, but the class tables have no null row (cfg_dropout_prob == 0)", c);
  CondArgs a;
  a.t = t;
  a.t_stride = t_stride;
  a.w0t = h->w0t; a.b0 = h->b0; a.w2t = h->w2t; a.b2 = h->b2;
  a.emb = h->emb;
  a.n_classes = h->cfg.n_classes;
  for (int c = 0; c < SCLDM_MAX_CLASSES; ++c) {
    a.emb_row0[c] = c < a.n_classes ? h->emb_row0[c] : 0;
    a.null_tok[c] = c < a.n_classes ? h->cfg.class_vocab[c] : 0;
    a.tab_rows[c] = c < a.n_classes ? h->tab_rows[c] : 1;
    a.labels[c] = (c < a.n_classes && labels && labels[c] && ((mask >> c) & 1u)) ? labels[c] : nullptr;
  }
  a.silu_c = silu_c;
  a.rows = rows;
  a.label_err = h->label_err;
  a.gate = gate;
  a.gate_want = gate_want;
  a.row_map = row_map;
  cond_embed_kernel<<<rows, 256, 0, st>>>(a);
  LAUNCH_CHECK();
  return SCLDM_OK;
}
// prec: the precision policy of the forward that consumes the vectors.  fp32 (and callers without a policy): exact fp32 on the
// matrix pipe; the fast policies: split-bf16 operands (their own arithmetic class or finer).  Within a policy every output element
// is one fixed-order sum whatever the number of rows (a cell's vectors never depend on its batch).
static int launch_adaln(scldm_dit* h, const float* silu_c, float* mod, int rows, hipStream_t st, const int* rows_dev = nullptr,
                        int prec = SCLDM_PREC_FP32, void* asplit = nullptr) {
  if (prec != SCLDM_PREC_FP32 && !h->adaln_valu && !h->adaln_exact) {
    const bf16x8x2* wf = reinterpret_cast<const bf16x8x2*>(h->ada_x3);
    const int n_tiles = h->mod_w / 32;
    if (rows <= 128 || !asplit || h->adaln_rowtile) {   // few rows: one column tile per wave (every wave's latency chain as short as possible)
      if (rows <= 128) adaln_x3_kernel<1><<<dim3(cdiv(n_tiles, 4), cdiv(rows, 32)), 256, 0, st>>>(silu_c, wf, h->ada_b, mod, rows, h->mod_w, rows_dev);
      else adaln_x3_kernel<4><<<dim3(cdiv(n_tiles, 16), cdiv(rows, 32)), 256, 0, st>>>(silu_c, wf, h->ada_b, mod, rows, h->mod_w, rows_dev);
    } else {             // many rows: rows split once, 128 x 128 blocks (the weights are read once per 128 rows); same bits
      bf16x8x2* af = reinterpret_cast<bf16x8x2*>(asplit);
      adaln_split_rows_kernel<<<cdiv(rows, 32) * 4, 256, 0, st>>>(silu_c, af, rows, rows_dev);
      adaln_x3_block_kernel<<<dim3(cdiv(n_tiles, 4), cdiv(rows, 128)), 256, 0, st>>>(af, wf, h->ada_b, mod, rows, h->mod_w, rows_dev);
    }
    LAUNCH_CHECK();
    return SCLDM_OK;
  }
  if (h->adaln_valu) {   // SCLDM_ADALN_VALU=1 (read once at create): the round-1 VALU kernel, for A/B runs
    dim3 grid(cdiv(h->mod_w, 64), cdiv(rows, kAdaRU));
    adaln_all_kernel<<<grid, 256, 0, st>>>(silu_c, h->ada_t, h->ada_b, mod, rows, h->mod_w, rows_dev);
  } else {
    dim3 grid(cdiv(h->mod_w, 128), cdiv(rows, 32));
    adaln_mfma_kernel<<<grid, 256, 0, st>>>(silu_c, h->ada_t, h->ada_b, mod, rows, h->mod_w, rows_dev);
  }
  LAUNCH_CHECK();
  return SCLDM_OK;
}

template <typename OP, int NTT, int FT, bool M16 = false>
static int launch_fwd_t(const FwdArgs& a, hipStream_t st) {
  using L = FwdLayout<OP, NTT, FT>;
  static bool attr_set[64] = {};   // the attribute is per device
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64 || !attr_set[dev]) {
    HIP_TRY(hipFuncSetAttribute((const void*)dit_forward_kernel<OP, NTT, FT, false, M16>, hipFuncAttributeMaxDynamicSharedMemorySize, L::LDS_BYTES));
    if (dev >= 0 && dev < 64) attr_set[dev] = true;
  }
  const int tiles = cdiv((long long)a.n_fwd * 16, L::TM);
  const int grid = a.grid_tiles > 0 ? a.grid_tiles : tiles;
  dit_forward_kernel<OP, NTT, FT, false, M16><<<grid, L::NT, L::LDS_BYTES, st>>>(a);
  LAUNCH_CHECK();
  return SCLDM_OK;
}

// m16: the handle's fwd_m16 (the stream was packed for it); it selects the bf16 / fp16 FT=2 instantiations only
static int launch_fwd(int prec, int ntt, int ft, bool m16, const FwdArgs& a, hipStream_t st) {
  if (prec == SCLDM_PREC_FP32) return launch_fwd_t<OpF32, 2, 2>(a, st);
  if (prec == SCLDM_PREC_BF16X3)
    return ft == 1 ? launch_fwd_t<OpBF16x3, 2, 1>(a, st) : ntt == 1 ? launch_fwd_t<OpBF16x3, 1, 2>(a, st) : launch_fwd_t<OpBF16x3, 2, 2>(a, st);
  if (prec == SCLDM_PREC_FP16) {
    if (ft == 1) return launch_fwd_t<OpFP16, 2, 1>(a, st);
    if (m16) return ntt == 1 ? launch_fwd_t<OpFP16, 1, 2, true>(a, st) : launch_fwd_t<OpFP16, 2, 2, true>(a, st);
    return ntt == 1 ? launch_fwd_t<OpFP16, 1, 2>(a, st) : launch_fwd_t<OpFP16, 2, 2>(a, st);
  }
  if (ft == 1) return launch_fwd_t<OpBF16, 2, 1>(a, st);
  if (m16) return ntt == 1 ? launch_fwd_t<OpBF16, 1, 2, true>(a, st) : launch_fwd_t<OpBF16, 2, 2, true>(a, st);
  return ntt == 1 ? launch_fwd_t<OpBF16, 1, 2>(a, st) : launch_fwd_t<OpBF16, 2, 2>(a, st);
}

// The DiT trunk: one fused launch per layer (input projection rides in the first, the final layer in the last).
static int trunk(scldm_dit* h, const float* x, int n_direct, int rep, int n_fwd, const float* mod, const int32_t* ridx,
                 float* hbuf, float* out, int prec, hipStream_t st) {
  const scldm_dit_config& c = h->cfg;
  const size_t es = esize(prec);
  int ntt, ft;
  pick_shape(h, prec, &ntt, &ft);
  // Small batches (round 5): while 32-token tiles still get a CU each (<= 256 of them = 512 samples), the kernel's walk is what a
  // launch costs and it is a quarter shorter with half the MFMAs and LDS fragment reads per k-step (163-175 against 212-220 us for the
  // eight layers at 43-128 cells x 3 CFG branches); beyond that two workgroups share a CU and the doubled weight stream loses
  // (213 cells: 255 against 228 us).  Same weight stream, same arithmetic per token: bit-identical (SCLDM_SMALL_NTT=0 switches it off).
  if (h->small_ntt && (prec == SCLDM_PREC_BF16 || prec == SCLDM_PREC_FP16) && ntt == 2 && ft == 2 && (long long)n_fwd * 16 <= 256 * 32) ntt = 1;
  const size_t layer_elems = (size_t)4 * units_per_layer(h->n_chunks[ft - 1], h->half[ft - 1]) * 1024;
  FwdArgs a{};
  a.z = x;
  a.out = out;
  a.x = hbuf;
  a.mod = mod;
  a.row_index = ridx;
  a.w_final = h->wfinal[prec];
  a.in_wt = h->in_wt;
  a.in_w = h->in_w;
  a.in_b = h->in_b;
  a.pos = h->pos;
  a.fin_b = h->fin_b;
  a.n_fwd = n_fwd;
  a.n_direct = n_direct;
  a.rep = rep;
  a.din = c.n_embed_input;
  a.n_layer = c.n_layer;
  a.n_chunks = h->n_chunks[ft - 1];
  a.half_chunk = h->half[ft - 1];
  a.mod_stride = h->mod_w;
  a.eps = c.layernorm_eps;
  a.attn_scale_log2e = 1.4426950408889634f / sqrtf(32.0f);
  const int dbg_layer = h->dbg_layer >= 0 ? h->dbg_layer : c.n_layer / 2;   // debug builds: which layer's launch records the phase stamps
  // Tile groups: each layer is launched as G kernels over disjoint tile ranges, group g on its own stream, so that the
  // round boundaries (burst of residual loads at the start, store drain and idle slots at the end) of one group fall
  // inside the steady state of the others.
  int G = h->groups;
  const int tile_tok = 32 * ntt;
  const int tiles_all = cdiv((long long)n_fwd * 16, tile_tok);
  if (tiles_all < 512 * G) G = 1;
  int gt0[5];
  for (int g = 0; g <= G; ++g) gt0[g] = (int)((long long)tiles_all * g / G);
  if (G > 1) {
    for (int g = 1; g < G; ++g)
      if (!h->side[g - 1]) {
        HIP_TRY(hipStreamCreateWithFlags(&h->side[g - 1], hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&h->join_ev[g - 1], hipEventDisableTiming));
      }
    if (!h->fork_ev) HIP_TRY(hipEventCreateWithFlags(&h->fork_ev, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(h->fork_ev, st));
    for (int g = 1; g < G; ++g) HIP_TRY(hipStreamWaitEvent(h->side[g - 1], h->fork_ev, 0));
  }
  // Tail split (round 4): two 64-token workgroups share a CU, so a launch runs in rounds of 2 x CUs tiles and its last, partial round
  // leaves slots empty (768 tiles = 1 024 cells x 3 forwards: 1.5 rounds; 384 tiles = 512 cells: 0.75).  The tiles of the partial
  // round that would run with an empty neighbour slot are launched as 32-token tiles instead (the NTT = 1 instantiation, on a side
  // stream beside the 64-token launch): r <= CUs tiles become 2 r half tiles (one short round of pairs instead of a round of lone
  // workgroups); r > CUs: 2 CUs - r of them are halved so that every slot is taken.  A cell's result does not depend on the tile
  // shape that carried it (same k order, same per-token LayerNorm / softmax arithmetic: bit-identical, tested).
  // MEASURED SLOWER (profiles/r4o_ab_tail_split.txt: 1 024 cells x 3 forwards 0.415 -> 0.366 of peak, 512 cells 0.366 -> 0.357, 1 000
  // cells 0.412 -> 0.363, 300 cells 0.332 -> 0.293): a 32-token tile streams twice the weight bytes per token, and that stream is what
  // the kernel waits for (profiles/r4j_timing_proxies_random_vs_zero.txt); lone workgroups of the partial round already run ~1.5x faster.  Off by default.
  int tail_full = 0;
  if (h->tail_split && G == 1 && ntt == 2 && ft == 2 && (prec == SCLDM_PREC_BF16 || prec == SCLDM_PREC_FP16)) {
    const int slots = 2 * h->n_cu, r = tiles_all % slots;
    if (r > 0) tail_full = r <= slots / 2 ? r : slots - r;
  }
  const int n64 = tiles_all - tail_full;
  const int n32 = tail_full > 0 ? cdiv((long long)n_fwd * 16 - (long long)n64 * 64, 32) : 0;
  if (tail_full > 0 && n64 > 0) {
    if (!h->side[0]) {
      HIP_TRY(hipStreamCreateWithFlags(&h->side[0], hipStreamNonBlocking));
      HIP_TRY(hipEventCreateWithFlags(&h->join_ev[0], hipEventDisableTiming));
    }
    if (!h->fork_ev) HIP_TRY(hipEventCreateWithFlags(&h->fork_ev, hipEventDisableTiming));
  }
  a.tile0 = 0;
  a.grid_tiles = 0;
  // layers per launch: the residual stays in registers between the layers of a launch (fewer hand-off round trips and
  // launch boundaries); the weights of that many layers are then live in each XCD's L2
  const int lpl = h->lpl;
  a.w_layer_elems = (long)layer_elems;
  for (int i = 0; i < c.n_layer; i += lpl) {
    a.layer = i;
    a.n_here = (i + lpl <= c.n_layer) ? lpl : c.n_layer - i;
    a.dbg = (dbg_layer >= i && dbg_layer < i + a.n_here) ? h->dbg : nullptr;
    a.w_stream = (const char*)h->stream[prec][ft - 1] + (size_t)i * layer_elems * es;
    a.b_qkv = h->b_qkv + (size_t)i * 768;
    a.b_proj = h->b_proj + (size_t)i * 256;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (h->timing && h->ev_used + 2 <= 40000) {
      while (h->ev.size() < h->ev_used + 2) {
        hipEvent_t ev;
        HIP_TRY(hipEventCreate(&ev));
        h->ev.push_back(ev);
      }
      e0 = h->ev[h->ev_used];
      e1 = h->ev[h->ev_used + 1];
      h->ev_used += 2;
      HIP_TRY(hipEventRecord(e0, st));
    }
    int rc = SCLDM_OK;
    if (tail_full > 0) {
      hipStream_t s1 = st;
      if (n64 > 0) {
        HIP_TRY(hipEventRecord(h->fork_ev, st));
        HIP_TRY(hipStreamWaitEvent(h->side[0], h->fork_ev, 0));
        a.tile0 = 0;
        a.grid_tiles = n64;
        rc = launch_fwd(prec, 2, ft, h->fwd_m16, a, st);
        s1 = h->side[0];
      }
      a.tile0 = 2 * n64;
      a.grid_tiles = n32;
      if (rc == SCLDM_OK) rc = launch_fwd(prec, 1, ft, h->fwd_m16, a, s1);
      if (n64 > 0) {
        HIP_TRY(hipEventRecord(h->join_ev[0], h->side[0]));
        HIP_TRY(hipStreamWaitEvent(st, h->join_ev[0], 0));
      }
      a.tile0 = 0;
      a.grid_tiles = 0;
    } else
      for (int g = 0; g < G && rc == SCLDM_OK; ++g) {
        hipStream_t sg = g == 0 ? st : h->side[g - 1];
        if (G > 1) {
          a.tile0 = gt0[g];
          a.grid_tiles = gt0[g + 1] - gt0[g];
        }
        rc = launch_fwd(prec, ntt, ft, h->fwd_m16, a, sg);
      }
    if (rc != SCLDM_OK) return rc;
    if (e1) HIP_TRY(hipEventRecord(e1, st));
  }
  if (G > 1)
    for (int g = 1; g < G; ++g) {
      HIP_TRY(hipEventRecord(h->join_ev[g - 1], h->side[g - 1]));
      HIP_TRY(hipStreamWaitEvent(st, h->join_ev[g - 1], 0));
    }
  return SCLDM_OK;
}

static int check_ready(const scldm_dit* h, int prec) {
  if (!h) return fail(SCLDM_ERR_SHAPE, "null handle");
  if (!h->loaded) return fail(SCLDM_ERR_STATE, "scldm_dit_load_weights has not been called");
  if (prec != SCLDM_PREC_FP32 && prec != SCLDM_PREC_BF16 && prec != SCLDM_PREC_BF16X3 && prec != SCLDM_PREC_FP16) return fail(SCLDM_ERR_SHAPE, "unknown precision %d", prec);
  if (!h->fused) return fail(SCLDM_ERR_SHAPE, "this handle's shape is outside the fused family (scldm_dit_train_* and scldm_dit_infer_* serve it)");
  return SCLDM_OK;
}

extern "C" int scldm_dit_cond_rows(scldm_dit* h, const float* t, int t_stride, const int64_t* const* labels, int n_rows,
                                   float* mod_out, void* ws_, void* stream_) {
  int rc = check_ready(h, 0);
  if (rc) return rc;
  if (n_rows <= 0 || !t || !mod_out || !ws_) return fail(SCLDM_ERR_SHAPE, "bad argument");
  hipStream_t st = (hipStream_t)stream_;
  Ws w = carve(h, ws_, 0, n_rows, 0);
  if ((rc = launch_cond(h, t, t_stride, labels, 0xffffffffu, n_rows, w.silu, st))) return rc;
  return launch_adaln(h, w.silu, mod_out, n_rows, st);
}

extern "C" int scldm_dit_forward_rows(scldm_dit* h, const float* x, int n_direct, int rep, int n_fwd, const float* mod,
                                      const int32_t* row_index, float* out, int precision, void* ws_, void* stream_) {
  int rc = check_ready(h, precision);
  if (rc) return rc;
  if (n_fwd <= 0 || n_direct <= 0 || n_direct > n_fwd || (n_fwd > n_direct && (rep <= 0 || rep > n_direct)))
    return fail(SCLDM_ERR_SHAPE, "bad n_fwd/n_direct/rep (%d,%d,%d)", n_fwd, n_direct, rep);
  if (!x || !mod || !row_index || !out || !ws_) return fail(SCLDM_ERR_SHAPE, "null pointer argument");
  Ws w = carve(h, ws_, n_fwd, 0, 0);
  return trunk(h, x, n_direct, rep > 0 ? rep : 1, n_fwd, mod, row_index, w.h, out, precision, (hipStream_t)stream_);
}

extern "C" int scldm_dit_forward(scldm_dit* h, const float* x, const float* t, const int64_t* const* labels, float* out,
                                 int n, int precision, void* ws_, void* stream_) {
  int rc = check_ready(h, precision);
  if (rc) return rc;
  if (n <= 0 || !x || !t || !out || !ws_) return fail(SCLDM_ERR_SHAPE, "bad argument");
  hipStream_t st = (hipStream_t)stream_;
  Ws w = carve(h, ws_, n, n, 0);
  if ((rc = launch_cond(h, t, 1, labels, 0xffffffffu, n, w.silu, st))) return rc;
  if ((rc = launch_adaln(h, w.silu, w.mod, n, st, nullptr, precision, w.asplit))) return rc;
  iota_kernel<<<cdiv(n, 256), 256, 0, st>>>(w.ridx, n);
  LAUNCH_CHECK();
  return trunk(h, x, n, 1, n, w.mod, w.ridx, w.h, out, precision, st);
}

// One CFG evaluation (CfgPlan, make_plan: cfg_plan.hpp).
// plan (optional, device): plan[0] == 0 selects the dense plan (one row per sample-forward: uncond_rows = n_direct, U = B, no
// cell_row) over the uniform one given by the arguments
__global__ void fill_cfg_row_index_kernel(int32_t* __restrict__ ri, const int32_t* __restrict__ cell_row, int n_direct,
                                          int uncond_rows, int B, int U, int P, const int* __restrict__ plan = nullptr, int direct = 0) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (direct) {   // 2B sample-forwards: the first half unconditional (one shared row), the second half with its label rows
    if (s < 2 * B) ri[s] = s < B ? 0 : uncond_rows + (cell_row ? cell_row[s - B] : s - B);
    return;
  }
  if (s >= n_direct + P * B) return;
  if (plan && plan[0] == 0) {
    uncond_rows = n_direct;
    U = B;
    cell_row = nullptr;
  }
  if (s < n_direct) { ri[s] = (uncond_rows == 1) ? 0 : s; return; }
  const int p = (s - n_direct) / B, i = (s - n_direct) % B;
  ri[s] = uncond_rows + p * U + (cell_row ? cell_row[i] : i);
}
__global__ void set_scalar_kernel(float* p, float v) { *p = v; }

// The conditioning of one CFG evaluation (timestep rows, class embeddings, adaLN projection -> w.mod): depends on t and the labels
// only, never on the state.
static CondRowsArgs cond_rows_args(const scldm_dit* h, const CfgPlan& pl, const float* temb, float* silu_c, const int* gate) {
  CondRowsArgs ca;
  ca.temb = temb;
  ca.emb = h->emb;
  ca.n_classes = h->cfg.n_classes;
  ca.U = pl.U > 0 ? pl.U : 1;
  ca.rows = pl.n_rows;
  for (int c = 0; c < SCLDM_MAX_CLASSES; ++c) {
    ca.emb_row0[c] = c < ca.n_classes ? h->emb_row0[c] : 0;
    ca.null_tok[c] = c < ca.n_classes ? h->cfg.class_vocab[c] : 0;
    ca.tab_rows[c] = c < ca.n_classes ? h->tab_rows[c] : 1;
    ca.labels[c] = (c < ca.n_classes && pl.ulabels && pl.ulabels[c]) ? pl.ulabels[c] : nullptr;
    ca.mask[c] = c < pl.P ? pl.mask[c] : 0u;
  }
  ca.silu_c = silu_c;
  ca.label_err = h->label_err;
  ca.gate = gate;
  return ca;
}
static int cfg_cond(scldm_dit* h, const CfgPlan& pl, const float* t_dev, int t_stride, const Ws& w, int prec, hipStream_t st,
                    const float* temb_pre = nullptr) {
  int rc;
  const int* gate = t_stride == 2 ? h->d_plan : nullptr;   // dense t, uniformity decided on device: both plans are enqueued, one runs
  const int rows_u = 1 + pl.P * pl.U, rows_d = 2 * pl.B + pl.P * pl.B;
  if (t_stride == 0 || t_stride == 2) {
    // scalar t: one timestep-MLP evaluation per step, then all rows (unconditional + every pass) in one launch
    const float* temb = temb_pre;
    if (!temb) {
      t_embed_kernel<<<1, 256, 0, st>>>(t_dev, h->w0t, h->b0, h->w2t, h->b2, w.temb);
      temb = w.temb;
    }
    CondRowsArgs ca = cond_rows_args(h, pl, temb, w.silu, gate);
    cond_rows_kernel<<<t_stride == 2 ? rows_u : pl.n_rows, 256, 0, st>>>(ca);
    LAUNCH_CHECK();
  }
  if (t_stride == 1 || t_stride == 2) {
    // per-sample t: unconditional rows (every class null), then one launch per conditional pass (per-cell labels; under the
    // device-decided plan they are read through cell_row out of the de-duplicated rows)
    const int ur = t_stride == 2 ? 2 * pl.B : pl.uncond_rows, U = t_stride == 2 ? pl.B : pl.U;
    if ((rc = launch_cond(h, t_dev, 1, nullptr, 0u, ur, w.silu, st, gate, 0))) return rc;
    for (int p = 0; p < pl.P; ++p) {
      const float* tp = t_dev + pl.B;  // second half of t
      if ((rc = launch_cond(h, tp, 1, pl.ulabels, pl.mask[p], U, w.silu + (size_t)(ur + p * U) * 256, st, gate, 0,
                            t_stride == 2 ? pl.cell_row : nullptr)))
        return rc;
    }
  }
  return launch_adaln(h, w.silu, w.mod, t_stride == 2 ? rows_d : pl.n_rows, st, t_stride == 2 ? h->d_plan + 1 : nullptr, prec, w.asplit);
}

// The state-dependent part of a CFG evaluation in two halves, so that a solve can put its own conditioning route between them:
// the trunk over every sample-forward writes cfg_trunk_out(), cfg_finish() blends it into dz.
// direct: the guided rows are the conditional forward itself - the trunk runs 2B sample-forwards and writes dz, no blend.
static int cfg_trunk_rows(const CfgPlan& pl) { return pl.direct ? 2 * pl.B : pl.n_fwd; }
static float* cfg_trunk_out(const CfgPlan& pl, const Ws& w, float* dz) { return pl.direct ? dz : w.v; }
// euler_z / euler_h: the caller's Euler update z += h * dz is applied by the blend kernel itself (one launch less per evaluation)
static int cfg_finish(scldm_dit* h, const CfgPlan& pl, const Ws& w, float* dz, hipStream_t st, float* euler_z, float euler_h) {
  const int e = 16 * h->cfg.n_embed_input;
  if (!pl.direct) return scldm_cfg_blend(w.v, dz, pl.B, e, pl.P, pl.scale, euler_z, euler_h, st);
  return euler_z ? scldm_ode_axpy(euler_z, dz, euler_z, euler_h, (size_t)2 * pl.B * e, st) : SCLDM_OK;
}

// One CFG evaluation: dz (2B, e) = forward_with_cfg(z, t); t_dev/t_stride describe the device-side t.
static int cfg_eval(scldm_dit* h, const CfgPlan& pl, const float* z, const float* t_dev, int t_stride, const Ws& w,
                    float* dz, int prec, hipStream_t st) {
  int rc = cfg_cond(h, pl, t_dev, t_stride, w, prec, st);
  if (rc) return rc;
  if ((rc = trunk(h, z, 2 * pl.B, pl.B, cfg_trunk_rows(pl), w.mod, w.ridx, w.h, cfg_trunk_out(pl, w, dz), prec, st))) return rc;
  return cfg_finish(h, pl, w, dz, st, nullptr, 0.f);
}

// host launchers of the CFG / ODE kernels for the record-free inference path of wide shapes (train_api.hip; dit_handle.hpp)
int scldm_cfg_fill_row_index(int32_t* ri, const int32_t* cell_row, int n_direct, int uncond_rows, int B, int U, int P, hipStream_t st) {
  fill_cfg_row_index_kernel<<<cdiv(n_direct + P * B, 256), 256, 0, st>>>(ri, cell_row, n_direct, uncond_rows, B, U, P);
  LAUNCH_CHECK();
  return SCLDM_OK;
}
int scldm_cfg_blend(const float* v, float* dz, int B, int e, int P, const float* scale, float* euler_z, float euler_h, hipStream_t st) {
  CfgArgs ca;
  ca.v = v;
  ca.dz = dz;
  ca.B = B;
  ca.e = e;
  ca.P = P;
  fill_pass_scale(ca.scale, P, scale);
  ca.z = euler_z;
  ca.hstep = euler_h;
  cfg_blend_kernel<<<cdiv((size_t)2 * B * e, 256), 256, 0, st>>>(ca);
  LAUNCH_CHECK();
  return SCLDM_OK;
}
int scldm_ode_axpy(const float* z, const float* k, float* out, float hstep, size_t n, hipStream_t st) {
  axpy_kernel<<<cdiv(n, 256), 256, 0, st>>>(z, k, out, hstep, n);
  LAUNCH_CHECK();
  return SCLDM_OK;
}
int scldm_ode_heun(float* z, const float* k1, const float* k2, float half_h, size_t n, hipStream_t st) {
  heun_kernel<<<cdiv(n, 256), 256, 0, st>>>(z, k1, k2, half_h, n);
  LAUNCH_CHECK();
  return SCLDM_OK;
}

extern "C" int scldm_dit_forward_cfg(scldm_dit* h, const float* x, const float* t, int t_stride, const int64_t* const* ulabels,
                                     int n_urows, const int32_t* cell_row, int B, int n_pass, const uint32_t* pass_mask,
                                     const float* pass_scale, float* out, int precision, void* ws_, void* stream_) {
  int rc = check_ready(h, precision);
  if (rc) return rc;
  if (!x || !t || !out || !ws_) return fail(SCLDM_ERR_SHAPE, "null pointer argument");
  if (t_stride < 0 || t_stride > 2) return fail(SCLDM_ERR_SHAPE, "t_stride must be 0 (scalar), 1 (per sample) or 2 (dense, uniformity decided on device)");
  CfgPlan pl;
  if ((rc = make_plan(h, pl, ulabels, n_urows, cell_row, B, n_pass, pass_mask, pass_scale, t_stride))) return rc;
  hipStream_t st = (hipStream_t)stream_;
  Ws w = carve(h, ws_, pl.n_fwd, pl.n_rows, 0);
  if (t_stride == 2) {
    uniform_t_kernel<<<1, 256, 0, st>>>(t, 2 * B, 1 + pl.P * pl.U, 2 * B + pl.P * B, h->d_plan);
    LAUNCH_CHECK();
  }
  fill_cfg_row_index_kernel<<<cdiv(pl.n_fwd, 256), 256, 0, st>>>(w.ridx, cell_row, 2 * B, t_stride == 2 ? 1 : pl.uncond_rows, B, pl.U, pl.P,
                                                                   t_stride == 2 ? h->d_plan : nullptr, pl.direct);
  LAUNCH_CHECK();
  return cfg_eval(h, pl, x, t, t_stride, w, out, precision, st);
}

// The adaLN vectors of n_evals evaluations from their (n_evals, 256) timestep embeddings: ONE row launch over (rows, evaluations) and
// ONE projection over n_evals x n_rows rows -> mod, evaluation j in rows [j n_rows, (j + 1) n_rows).  silu, asplit: scratch for as
// many rows.  Same kernels and per-row arithmetic as the per-evaluation launches of cfg_cond: bit-identical (tested).
static int cond_batch(scldm_dit* h, const CfgPlan& pl, const float* temb, int n_evals, float* silu, float* mod, void* asplit, int prec,
                      hipStream_t st) {
  CondRowsArgs ca = cond_rows_args(h, pl, temb, silu, nullptr);
  cond_rows_kernel<<<dim3(pl.n_rows, n_evals), 256, 0, st>>>(ca);
  LAUNCH_CHECK();
  return launch_adaln(h, silu, mod, n_evals * pl.n_rows, st, nullptr, prec, asplit);
}

// Whole-solve conditioning (see FusedSolve): cond_batch over every evaluation of the solve, into the handle's buffer; *mod_all stays NULL
// when the per-evaluation launches are to be used (over budget, no room, or the buffer would have to grow inside a stream capture).
// temb: the (n_evals, 256) timestep embeddings of the solve.
static int cond_all_prepare(scldm_dit* h, const CfgPlan& pl, const float* temb, int n_evals, int prec, hipStream_t st, float** mod_all_out) {
  *mod_all_out = nullptr;
  const size_t rows_all = (size_t)n_evals * pl.n_rows;
  const size_t b_mod = align256(rows_all * h->mod_w * 4), b_silu = align256((rows_all + 1) * 256 * 4), b_split = align256((rows_all + 31) / 32 * 32 * 256 * 4);
  if (b_mod > ((size_t)1 << 30)) return SCLDM_OK;
  const size_t need = b_mod + b_silu + b_split;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing(st, &cap);
  if (h->cond_all_bytes < need && cap == hipStreamCaptureStatusNone) {   // (no allocation inside a stream capture: the per-evaluation launches)
    HIP_TRY(hipStreamSynchronize(st));     // (an earlier solve on this stream may still read the buffer that is replaced)
    if (h->cond_all) (void)hipFree(h->cond_all);
    h->cond_all = nullptr;
    h->cond_all_bytes = 0;
    if (hipMalloc(&h->cond_all, need) == hipSuccess) h->cond_all_bytes = need;
    else (void)hipGetLastError();          // no room: the per-evaluation launches
  }
  if (h->cond_all_bytes < need) return SCLDM_OK;
  char* base = reinterpret_cast<char*>(h->cond_all);
  *mod_all_out = reinterpret_cast<float*>(base);
  return cond_batch(h, pl, temb, n_evals, reinterpret_cast<float*>(base + b_mod), *mod_all_out, base + b_mod + b_silu, prec, st);
}

// One fixed-grid solve of the fused family (scldm_sample_ode, scldm_sample_sde, scldm_sample_ode_transport): set up once per call,
// then asked one thing per evaluation - eval(e, zin, out): the conditioning of evaluation e, then the trunk of zin into out.  Which
// conditioning route serves the solve is decided and kept in here:
//   whole solve    the adaLN vectors depend on t and the labels only, so every evaluation's rows go through ONE timestep-embedding
//                  launch, ONE row launch and ONE adaLN projection over n_evals x n_rows rows before the loop instead of two launches
//                  per evaluation on the critical path (4.7 + 8.2 us of a 174 us evaluation at 128 cells:
//                  profiles/r6_small_batch_trace.txt); an evaluation then reads its slice.  Budget 1 GB (15 rows x 100 evaluations =
//                  83 MB for the dentate vocabulary, 51 rows x 200 Heun evaluations = 564 MB for hlca; a batch of 1 024 distinct joint
//                  labels would need 5.7 GB and takes the next route).  SCLDM_COND_ALL=0 switches it off;
//   pre-embedded   every timestep embedding in one launch before the loop; the row launch and the projection per evaluation;
//   step by step   solves beyond kMaxTembEvals evaluations: a device scalar t, embedded per evaluation.
struct FusedSolve {
  scldm_dit* h;
  CfgPlan pl;
  Ws w;
  int prec;
  hipStream_t st;
  size_t n;   // elements of the (2B, e) state

  // the plan and the workspace: argument checks only, nothing is enqueued
  int plan(scldm_dit* h_, const int64_t* const* ulabels, int n_urows, const int32_t* cell_row, int B, int n_pass, const uint32_t* pass_mask,
           const float* pass_scale, int precision, void* ws, void* stream) {
    h = h_;
    prec = precision;
    st = (hipStream_t)stream;
    int rc = make_plan(h, pl, ulabels, n_urows, cell_row, B, n_pass, pass_mask, pass_scale, 0);
    if (rc) return rc;
    w = carve(h, ws, pl.n_fwd, pl.n_rows, 2 * B);
    n = (size_t)2 * B * 16 * h->cfg.n_embed_input;
    return SCLDM_OK;
  }
  // The row index, the timestep embeddings and (whole-solve route) the conditioning of every evaluation.  times: the time of each
  // evaluation (grid::eval_times).  grid_steps > 0: the solve runs over linspace(0, 1, grid_steps) and the embeddings come from the
  // device's own grid (t_embed_all_kernel, `grid_heun` its layout) - it forms 1 - step x as one fma, which the host list is not
  // guaranteed to reproduce, so scldm_sample_ode keeps it.
  int prepare(const std::vector<float>& times, int grid_steps = 0, bool grid_heun = false) {
    tl_ = times;
    const int n_evals = (int)tl_.size();
    fill_cfg_row_index_kernel<<<cdiv(pl.n_fwd, 256), 256, 0, st>>>(w.ridx, pl.cell_row, 2 * pl.B, 1, pl.B, pl.U, pl.P, nullptr, pl.direct);
    LAUNCH_CHECK();
    pre_ = n_evals <= kMaxTembEvals;
    if (!pre_) return SCLDM_OK;
    if (grid_steps > 0) {
      t_embed_all_kernel<<<n_evals, 256, 0, st>>>(grid_steps, grid_heun, h->w0t, h->b0, h->w2t, h->b2, w.temb);
    } else {
      // the list of times sits at the head of the trunk's residual buffer: the embedding launch below has read it before the first trunk
      // launch of this call overwrites it (stream order)
      float* tlist = w.h;
      for (int c0 = 0; c0 < n_evals; c0 += sde::kTChunk) {
        sde::TChunk ch{};
        const int m = std::min(sde::kTChunk, n_evals - c0);
        for (int j = 0; j < m; ++j) ch.t[j] = tl_[c0 + j];
        sde::set_tlist_kernel<<<1, sde::kTChunk, 0, st>>>(tlist + c0, ch, m);
      }
      sde::t_embed_list_kernel<<<n_evals, 256, 0, st>>>(tlist, h->w0t, h->b0, h->w2t, h->b2, w.temb);
    }
    LAUNCH_CHECK();
    if (h->cond_all_on && n_evals > 1) return cond_all_prepare(h, pl, w.temb, n_evals, prec, st, &mod_all_);
    return SCLDM_OK;
  }
  // the conditioning of evaluation e, then the trunk of zin -> out: (cfg_trunk_rows(pl), e) rows, for the entry's blend kernel
  int eval(int e, const float* zin, float* out) {
    const float* mod = w.mod;
    if (mod_all_) mod = mod_all_ + (size_t)e * pl.n_rows * h->mod_w;
    else {
      float* tscal = w.silu + (size_t)pl.n_rows * 256;   // device scalar t: the spare row carve() reserves after the silu rows
      if (!pre_) set_scalar_kernel<<<1, 1, 0, st>>>(tscal, tl_[e]);
      int rc = cfg_cond(h, pl, tscal, 0, w, prec, st, pre_ ? w.temb + (size_t)e * 256 : nullptr);
      if (rc) return rc;
    }
    return trunk(h, zin, 2 * pl.B, pl.B, cfg_trunk_rows(pl), mod, w.ridx, w.h, out, prec, st);
  }
  // grid::euler_heun over linspace(a, b, n_steps + 1) on the state z with the workspace's slope buffers; step_eval as its `eval`
  template <class Eval>
  int step_loop(int n_steps, float a, float b, bool heun, float* z, Eval&& step_eval) {
    return grid::euler_heun(
        n_steps, a, b, heun, grid::Buffers{z, w.dz, w.k2, w.ztmp}, step_eval,
        [&](const float* x, const float* k, float* out, float hs) { return scldm_ode_axpy(x, k, out, hs, n, st); },
        [&](float* x, const float* k1, const float* k2, float half_hs) { return scldm_ode_heun(x, k1, k2, half_hs, n, st); });
  }

 private:
  std::vector<float> tl_;
  bool pre_ = false;
  float* mod_all_ = nullptr;
};

extern "C" int scldm_sample_ode(scldm_dit* h, float* z, const int64_t* const* ulabels, int n_urows, const int32_t* cell_row,
                                int B, int n_pass, const uint32_t* pass_mask, const float* pass_scale, int n_steps, int method,
                                int precision, void* ws_, void* stream_) {
  int rc = check_ready(h, precision);
  if (rc) return rc;
  if (!z || !ws_) return fail(SCLDM_ERR_SHAPE, "null pointer argument");
  if (n_steps < 1) return fail(SCLDM_ERR_SHAPE, "n_steps must be >= 1");
  if (method != SCLDM_METHOD_EULER && method != SCLDM_METHOD_HEUN) return fail(SCLDM_ERR_SHAPE, "unknown method %d", method);
  FusedSolve s;
  if ((rc = s.plan(h, ulabels, n_urows, cell_row, B, n_pass, pass_mask, pass_scale, precision, ws_, stream_))) return rc;
  const bool heun = method == SCLDM_METHOD_HEUN;
  if ((rc = s.prepare(grid::eval_times(n_steps, 0.f, 1.f, heun ? grid::kNext : grid::kNone), n_steps + 1, heun))) return rc;
  // one evaluation: the trunk, then the CFG blend into dz (which also applies the Euler update when euler_z is given)
  auto eval = [&](int e, const float* zin, float* dz, float* euler_z, float hs) -> int {
    int rc2 = s.eval(e, zin, cfg_trunk_out(s.pl, s.w, dz));
    return rc2 ? rc2 : cfg_finish(h, s.pl, s.w, dz, s.st, euler_z, hs);
  };
  return s.step_loop(n_steps, 0.f, 1.f, heun, z, eval);
}

// ---- adaptive Dormand-Prince 5(4) sampling (dopri5_ctl.hpp, dopri5_fused.hpp) ----
// the handle-free controller entries: dopri5_ctl.hpp's decisions with a C face
extern "C" void scldm_dopri5_stage_plan(double t0, double h, scldm_dopri5_plan* out) {
  if (out) scldm::dopri5::stage_plan(t0, h, out);
}
extern "C" void scldm_dopri5_control(double t0, double h, double ratio, scldm_dopri5_control_out* out) {
  if (out) scldm::dopri5::control(t0, h, ratio, out);
}
extern "C" double scldm_dopri5_initial_h0(double d0, double d1) { return scldm::dopri5::initial_h0(d0, d1); }
extern "C" double scldm_dopri5_initial_step(double h0, double d1, double d2) { return scldm::dopri5::initial_step(h0, d1, d2); }

#include "dopri5_api.inc"

// ---- SDE sampling (sde.hpp) -----------------------------------------------------------------------------------------------------------
// D(t) of path.py:52-77 for the Linear path (sigma_t = 1 - t), in double from the fp32 t the model sees
static double sde_diffusion(int form, double norm, double t) {
  const double pi = 3.14159265358979323846;
  switch (form) {
    case SCLDM_SDE_FORM_SIGMA:
    case SCLDM_SDE_FORM_LINEAR: return norm * (1.0 - t);
    case SCLDM_SDE_FORM_CONSTANT: return norm;
    case SCLDM_SDE_FORM_DECREASING: { const double c = norm * cos(pi * t) + 1.0; return 0.25 * c * c; }
    default: { const double s = sin(pi * t); return norm * s * s; }   // SCLDM_SDE_FORM_INC_DEC
  }
}

extern "C" int scldm_sde_noise(float* out, long long n_rows_local, int e, unsigned long long seed, int step, int half, long long cell_offset,
                               long long cells_total, void* stream_) {
  if (!out || ((uintptr_t)out & 15)) return fail(SCLDM_ERR_SHAPE, "scldm_sde_noise: out must be a 16-byte aligned device pointer");
  if (n_rows_local < 1 || e < 4 || e % 4) return fail(SCLDM_ERR_SHAPE, "scldm_sde_noise: n_rows_local >= 1 and e a positive multiple of 4 (got %lld, %d)", n_rows_local, e);
  if (step < 0 || (half != 0 && half != 1)) return fail(SCLDM_ERR_SHAPE, "scldm_sde_noise: step >= 0 and half 0 | 1 (got %d, %d)", step, half);
  if (cell_offset < 0 || cells_total < cell_offset + n_rows_local)
    return fail(SCLDM_ERR_SHAPE, "scldm_sde_noise: cells_total (%lld) < cell_offset (%lld) + n_rows_local (%lld)", cells_total, cell_offset, n_rows_local);
  const long long n4 = n_rows_local * (e / 4);
  if (n4 > 0x7fffffffll) return fail(SCLDM_ERR_SHAPE, "scldm_sde_noise: at most 2^33 elements per call");
  const sde::NoiseGeom g{seed, cell_offset, cells_total, (uint32_t)step};
  sde::sde_noise_kernel<<<cdiv(n4, 256), 256, 0, (hipStream_t)stream_>>>(out, n_rows_local, e, half, g);
  LAUNCH_CHECK();
  return SCLDM_OK;
}

extern "C" int scldm_sample_sde(scldm_dit* h, float* z, const int64_t* const* ulabels, int n_urows, const int32_t* cell_row, int B, int n_pass,
                                const uint32_t* pass_mask, const float* pass_scale, int num_steps, int method, int diffusion_form,
                                float diffusion_norm, int last_step, float last_step_size, const float* noise, unsigned long long seed,
                                long long cell_offset, long long cells_total, float* traj, int precision, void* ws_, void* stream_) {
  int rc = check_ready(h, precision);
  if (rc) return rc;
  if (!z || !ws_) return fail(SCLDM_ERR_SHAPE, "null pointer argument");
  if (method != SCLDM_METHOD_EULER && method != SCLDM_METHOD_HEUN) return fail(SCLDM_ERR_SHAPE, "unknown method %d", method);
  if (diffusion_form == SCLDM_SDE_FORM_SBDM)
    return fail(SCLDM_ERR_SHAPE, "diffusion_form SBDM starts at t = 0 under the Linear path, where D = (1 - t) / t is infinite (the reference returns NaN); "
                "use sigma, linear, constant, decreasing or inccreasing-decreasing");
  if (diffusion_form < SCLDM_SDE_FORM_SIGMA || diffusion_form > SCLDM_SDE_FORM_INC_DEC) return fail(SCLDM_ERR_SHAPE, "unknown diffusion form %d", diffusion_form);
  if (last_step < SCLDM_SDE_LAST_NONE || last_step > SCLDM_SDE_LAST_EULER) return fail(SCLDM_ERR_SHAPE, "unknown last step %d", last_step);
  if (method == SCLDM_METHOD_HEUN && last_step == SCLDM_SDE_LAST_NONE)
    return fail(SCLDM_ERR_SHAPE, "Heun without a last step evaluates the score at t = 1 in its final K2 (the reference returns NaN / inf); "
                "use last_step Mean, Tweedie or Euler, or the Euler method");
  if (num_steps < 2) return fail(SCLDM_ERR_SHAPE, "num_steps must be >= 2 (grid points)");
  if (last_step == SCLDM_SDE_LAST_NONE) last_step_size = 0.f;   // transport.py:290-291
  if (!(last_step_size >= 0.f && last_step_size < 1.f)) return fail(SCLDM_ERR_SHAPE, "last_step_size must be in [0, 1) (got %g)", (double)last_step_size);
  if ((last_step == SCLDM_SDE_LAST_MEAN || last_step == SCLDM_SDE_LAST_TWEEDIE) && last_step_size == 0.f)
    return fail(SCLDM_ERR_SHAPE, "last_step Mean / Tweedie with last_step_size 0 evaluates the score at t = 1; give a positive last_step_size or use last_step Euler / None");
  if (cell_offset < 0 || cells_total < cell_offset + B) return fail(SCLDM_ERR_SHAPE, "cells_total (%lld) < cell_offset (%lld) + B (%d)", cells_total, cell_offset, B);
  if (((uintptr_t)z & 15) || ((uintptr_t)noise & 15) || ((uintptr_t)traj & 15)) return fail(SCLDM_ERR_SHAPE, "z, noise and traj must be 16-byte aligned");
  FusedSolve s;
  if ((rc = s.plan(h, ulabels, n_urows, cell_row, B, n_pass, pass_mask, pass_scale, precision, ws_, stream_))) return rc;
  const CfgPlan& pl = s.pl;
  const Ws& w = s.w;
  hipStream_t st = s.st;
  const int e_row = 16 * h->cfg.n_embed_input;
  const size_t n = s.n;
  if (n / 4 > 0x7fffffffull) return fail(SCLDM_ERR_SHAPE, "state too large (at most 2^33 elements)");
  const bool heun = method == SCLDM_METHOD_HEUN, has_last = last_step != SCLDM_SDE_LAST_NONE;
  const int n_steps = num_steps - 1;
  // the fp32 grid of integrators.py:23-24 and every evaluation's time
  const float t1 = (float)(1.0 - (double)last_step_size);
  const float dt = grid::linspace(1, num_steps, 0.f, t1) - grid::linspace(0, num_steps, 0.f, t1);
  const std::vector<float> tl = grid::eval_times(n_steps, 0.f, t1, heun ? grid::kPlusDt : grid::kNone, has_last ? &t1 : nullptr);
  for (int i = 0; i < (int)tl.size() - (has_last ? 1 : 0); ++i)
    if (!(tl[i] < 1.0f)) return fail(SCLDM_ERR_SHAPE, "evaluation %d of the solve sits at t = %g >= 1, where the score is singular", i, (double)tl[i]);
  if ((rc = s.prepare(tl))) return rc;
  sde::BlendArgs ba{};
  ba.v = w.v;
  ba.B = B;
  ba.e = e_row;
  ba.P = pl.P;
  ba.direct = pl.direct ? 1 : 0;
  fill_pass_scale(ba.scale, pl.P, pl.scale);
  ba.g = sde::NoiseGeom{seed, cell_offset, cells_total, 0u};
  int e_idx = 0;
  // one evaluation at zin, then out = a_x zin + a_v r (+ a_w w of step `step` when a_w != 0)
  auto eval = [&](const float* zin, float* out, float a_x, float a_v, float a_w, int step, float* traj_out) -> int {
    int rc2 = s.eval(e_idx++, zin, w.v);
    if (rc2) return rc2;
    ba.x = zin;
    ba.out = out;
    ba.traj = traj_out;
    ba.a_x = a_x;
    ba.a_v = a_v;
    ba.a_w = a_w;
    ba.noise_mode = a_w == 0.f ? sde::kNoiseNone : noise ? sde::kNoiseArray : sde::kNoisePhilox;
    ba.noise = noise ? noise + (size_t)step * n : nullptr;
    ba.g.step = (uint32_t)step;
    sde::cfg_blend_sde_kernel<<<cdiv(n / 4, 256), 256, 0, st>>>(ba);
    LAUNCH_CHECK();
    return SCLDM_OK;
  };
  // f = c_v v + c_x x at time t (double; rounded once where it enters a kernel argument)
  auto drift_coef = [&](float t, double* c_v, double* c_x) {
    const double D = sde_diffusion(diffusion_form, diffusion_norm, t), om = 1.0 - (double)t;
    *c_v = 1.0 + D * (double)t / om;
    *c_x = -D / om;
  };
  for (int i = 0; i < n_steps; ++i) {
    const float t = grid::linspace(i, num_steps, 0.f, t1);
    const float a_w = (float)sqrt(2.0 * sde_diffusion(diffusion_form, diffusion_norm, t) * (double)dt);
    float* tr = traj ? traj + (size_t)i * n : nullptr;
    double c_v, c_x;
    drift_coef(t, &c_v, &c_x);
    if (!heun) {   // x <- x + dt f(x, t) + sqrt(2 D dt) w
      if ((rc = eval(z, z, (float)(1.0 + (double)dt * c_x), (float)((double)dt * c_v), a_w, i, tr))) return rc;
    } else {
      if (a_w != 0.f) {   // xhat = x + sqrt(2 D(t) dt) w
        sde::PerturbArgs pa{z, noise ? noise + (size_t)i * n : nullptr, B, e_row, noise ? sde::kNoiseArray : sde::kNoisePhilox, a_w, ba.g};
        pa.g.step = (uint32_t)i;
        sde::sde_perturb_kernel<<<cdiv(n / 4, 256), 256, 0, st>>>(pa);
      }
      if ((rc = eval(z, w.dz, (float)c_x, (float)c_v, 0.f, i, nullptr))) return rc;          // K1 = f(xhat, t)
      axpy_kernel<<<cdiv(n, 256), 256, 0, st>>>(z, w.dz, w.ztmp, dt, n);                      // xp = xhat + dt K1
      drift_coef(t + dt, &c_v, &c_x);
      if ((rc = eval(w.ztmp, w.k2, (float)c_x, (float)c_v, 0.f, i, nullptr))) return rc;      // K2 = f(xp, t + dt)
      heun_kernel<<<cdiv(n, 256), 256, 0, st>>>(z, w.dz, w.k2, 0.5f * dt, n);                 // x = xhat + dt / 2 (K1 + K2)
      if (tr) HIP_TRY(hipMemcpyAsync(tr, z, n * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    LAUNCH_CHECK();
  }
  float* tr = traj ? traj + (size_t)n_steps * n : nullptr;
  if (has_last) {
    double c_v, c_x;
    drift_coef(t1, &c_v, &c_x);
    float a_x = 1.f, a_v = last_step_size;                                   // Euler: x + last_step_size v
    if (last_step == SCLDM_SDE_LAST_MEAN) {                                  // x + last_step_size f(x, t1)
      a_x = (float)(1.0 + (double)last_step_size * c_x);
      a_v = (float)((double)last_step_size * c_v);
    } else if (last_step == SCLDM_SDE_LAST_TWEEDIE) a_v = (float)(1.0 - (double)t1);   // x / t1 + (1 - t1)^2 / t1 score = x + (1 - t1) v
    if ((rc = eval(z, z, a_x, a_v, 0.f, n_steps, tr))) return rc;
  } else if (tr) HIP_TRY(hipMemcpyAsync(tr, z, n * sizeof(float), hipMemcpyDeviceToDevice, st));   // the reference appends the unchanged state
  return SCLDM_OK;
}

// ---- SDE sampling under any transport (sde_transport.hpp) -------------------------------------------------------------------------------
// The same launches as scldm_sample_sde - the trunk, then cfg_blend_sde_kernel with three scalars (sde_perturb_kernel, axpy and heun
// kernels for Heun) - with the scalars of sdet::eval_at over linspace(t0, t1, num_steps), (t0, t1) = sdet::sde_interval.  Every scalar
// of every update is formed before the first launch; one that is not finite refuses the solve.
extern "C" int scldm_sde_coef_at(const scldm_transport* tr, int diffusion_form, double diffusion_norm, double t, double dt, double* out) {
  if (!out || !tpath::transport_valid(tr) || !sdet::form_valid(diffusion_form))
    return fail(SCLDM_ERR_SHAPE, "scldm_sde_coef_at: bad argument (Linear | GVP, velocity | noise | score, 0 <= eps < 0.5, a known diffusion form)");
  const sdet::Eval ev = sdet::eval_at(tr, diffusion_form, diffusion_norm, t);
  out[0] = ev.D;
  out[1] = ev.c_x;
  out[2] = ev.c_m;
  out[3] = sdet::noise_scale(ev, dt);
  return SCLDM_OK;
}
extern "C" int scldm_sde_last_coef_at(const scldm_transport* tr, int diffusion_form, double diffusion_norm, int last_step, double last_step_size,
                                      double t1, double* out) {
  if (!out || !tpath::transport_valid(tr) || !sdet::form_valid(diffusion_form) || last_step < SCLDM_SDE_LAST_MEAN || last_step > SCLDM_SDE_LAST_EULER)
    return fail(SCLDM_ERR_SHAPE, "scldm_sde_last_coef_at: bad argument (Linear | GVP, velocity | noise | score, 0 <= eps < 0.5, a known diffusion "
                "form, last step Mean | Tweedie | Euler)");
  const sdet::Eval ev = sdet::eval_at(tr, diffusion_form, diffusion_norm, t1);
  sdet::last_coef(ev, last_step, last_step_size, &out[0], &out[1]);
  return SCLDM_OK;
}

extern "C" int scldm_sample_sde_transport(scldm_dit* h, float* z, const int64_t* const* ulabels, int n_urows, const int32_t* cell_row, int B,
                                          int n_pass, const uint32_t* pass_mask, const float* pass_scale, int num_steps, int method,
                                          int diffusion_form, float diffusion_norm, int last_step, float last_step_size, const float* noise,
                                          unsigned long long seed, long long cell_offset, long long cells_total, float* traj, int precision,
                                          void* ws_, void* stream_, const scldm_transport* tr) {
  if (!tpath::transport_valid(tr))
    return fail(SCLDM_ERR_SHAPE, "scldm_sample_sde_transport: bad transport (Linear | GVP, velocity | noise | score, 0 <= eps < 0.5)");
  if (tr->path == SCLDM_PATH_LINEAR && tr->model == SCLDM_MODEL_VELOCITY)   // the default transport: the existing solve, its refusals included
    return scldm_sample_sde(h, z, ulabels, n_urows, cell_row, B, n_pass, pass_mask, pass_scale, num_steps, method, diffusion_form, diffusion_norm,
                            last_step, last_step_size, noise, seed, cell_offset, cells_total, traj, precision, ws_, stream_);
  int rc = check_ready(h, precision);
  if (rc) return rc;
  if (!z || !ws_) return fail(SCLDM_ERR_SHAPE, "null pointer argument");
  if (method != SCLDM_METHOD_EULER && method != SCLDM_METHOD_HEUN) return fail(SCLDM_ERR_SHAPE, "unknown method %d", method);
  if (!sdet::form_valid(diffusion_form)) return fail(SCLDM_ERR_SHAPE, "unknown diffusion form %d", diffusion_form);
  if (last_step < SCLDM_SDE_LAST_NONE || last_step > SCLDM_SDE_LAST_EULER) return fail(SCLDM_ERR_SHAPE, "unknown last step %d", last_step);
  if (num_steps < 2) return fail(SCLDM_ERR_SHAPE, "num_steps must be >= 2 (grid points)");
  if (last_step == SCLDM_SDE_LAST_NONE) last_step_size = 0.f;   // transport.py:290-291
  if (!(last_step_size >= 0.f && last_step_size < 1.f)) return fail(SCLDM_ERR_SHAPE, "last_step_size must be in [0, 1) (got %g)", (double)last_step_size);
  if (cell_offset < 0 || cells_total < cell_offset + B) return fail(SCLDM_ERR_SHAPE, "cells_total (%lld) < cell_offset (%lld) + B (%d)", cells_total, cell_offset, B);
  if (((uintptr_t)z & 15) || ((uintptr_t)noise & 15) || ((uintptr_t)traj & 15)) return fail(SCLDM_ERR_SHAPE, "z, noise and traj must be 16-byte aligned");
  const bool heun = method == SCLDM_METHOD_HEUN, has_last = last_step != SCLDM_SDE_LAST_NONE;
  const int n_steps = num_steps - 1;
  // the fp32 grid of integrators.py:23-24, every evaluation's time and every update's scalars
  float t0, t1;
  sdet::sde_interval(tr, last_step_size, &t0, &t1);
  if (!(t0 < t1)) return fail(SCLDM_ERR_SHAPE, "the solve's interval [%g, %g] is empty (sample_eps against 1 - last_step_size)", (double)t0, (double)t1);
  const float dt = grid::linspace(1, num_steps, t0, t1) - grid::linspace(0, num_steps, t0, t1);
  const std::vector<float> tl = grid::eval_times(n_steps, t0, t1, heun ? grid::kPlusDt : grid::kNone, has_last ? &t1 : nullptr);
  struct Upd { float a_x, a_m, a_w; };
  std::vector<Upd> up;   // one per evaluation, in tl's order: a step's noise scale rides with its first evaluation
  up.reserve(tl.size());
  for (int i = 0; i < n_steps; ++i) {
    const float t = grid::linspace(i, num_steps, t0, t1);
    const sdet::Eval ev = sdet::eval_at(tr, diffusion_form, diffusion_norm, (double)t);
    const double a_w = sdet::noise_scale(ev, (double)dt);
    const double a_x = heun ? ev.c_x : 1.0 + (double)dt * ev.c_x, a_m = heun ? ev.c_m : (double)dt * ev.c_m;
    if (!sdet::all_finite({ev.D, a_x, a_m, a_w}))
      return fail(SCLDM_ERR_SHAPE, "scldm_sample_sde_transport: %s", sdet::refusal((int)up.size(), (double)t, "D, c_x, c_m or sqrt(2 D dt)").c_str());
    up.push_back(Upd{(float)a_x, (float)a_m, (float)a_w});
    if (heun) {
      const float t2 = t + dt;
      const sdet::Eval e2 = sdet::eval_at(tr, diffusion_form, diffusion_norm, (double)t2);
      if (!sdet::all_finite({e2.D, e2.c_x, e2.c_m}))
        return fail(SCLDM_ERR_SHAPE, "scldm_sample_sde_transport: %s", sdet::refusal((int)up.size(), (double)t2, "D, c_x or c_m of Heun's K2").c_str());
      up.push_back(Upd{(float)e2.c_x, (float)e2.c_m, 0.f});
    }
  }
  if (has_last) {
    const sdet::Eval ev = sdet::eval_at(tr, diffusion_form, diffusion_norm, (double)t1);
    double a_x, a_m;
    sdet::last_coef(ev, last_step, (double)last_step_size, &a_x, &a_m);
    if (!sdet::all_finite({a_x, a_m}))
      return fail(SCLDM_ERR_SHAPE, "scldm_sample_sde_transport: %s", sdet::refusal((int)up.size(), (double)t1, "a_x or a_m of the last step").c_str());
    up.push_back(Upd{(float)a_x, (float)a_m, 0.f});
  }
  FusedSolve s;
  if ((rc = s.plan(h, ulabels, n_urows, cell_row, B, n_pass, pass_mask, pass_scale, precision, ws_, stream_))) return rc;
  const CfgPlan& pl = s.pl;
  const Ws& w = s.w;
  hipStream_t st = s.st;
  const int e_row = 16 * h->cfg.n_embed_input;
  const size_t n = s.n;
  if (e_row % 4 || n / 4 > 0x7fffffffull) return fail(SCLDM_ERR_SHAPE, "state rows must be a multiple of 4 elements, at most 2^33 elements in all");
  if ((rc = s.prepare(tl))) return rc;
  sde::BlendArgs ba{};
  ba.v = w.v;
  ba.B = B;
  ba.e = e_row;
  ba.P = pl.P;
  ba.direct = pl.direct ? 1 : 0;
  fill_pass_scale(ba.scale, pl.P, pl.scale);
  ba.g = sde::NoiseGeom{seed, cell_offset, cells_total, 0u};
  int e_idx = 0;
  // evaluation e_idx at zin, then out = a_x zin + a_m m (+ a_w w of step `step` when with_noise)
  auto eval = [&](const float* zin, float* out, bool with_noise, int step, float* traj_out) -> int {
    const Upd& u = up[e_idx];
    int rc2 = s.eval(e_idx++, zin, w.v);
    if (rc2) return rc2;
    ba.x = zin;
    ba.out = out;
    ba.traj = traj_out;
    ba.a_x = u.a_x;
    ba.a_v = u.a_m;
    ba.a_w = with_noise ? u.a_w : 0.f;
    ba.noise_mode = (!with_noise || u.a_w == 0.f) ? sde::kNoiseNone : noise ? sde::kNoiseArray : sde::kNoisePhilox;
    ba.noise = noise ? noise + (size_t)step * n : nullptr;
    ba.g.step = (uint32_t)step;
    sde::cfg_blend_sde_kernel<<<cdiv(n / 4, 256), 256, 0, st>>>(ba);
    LAUNCH_CHECK();
    return SCLDM_OK;
  };
  for (int i = 0; i < n_steps; ++i) {
    float* trj = traj ? traj + (size_t)i * n : nullptr;
    if (!heun) {   // x <- x + dt f(x, t) + sqrt(2 D dt) w
      if ((rc = eval(z, z, true, i, trj))) return rc;
    } else {
      const float a_w = up[e_idx].a_w;
      if (a_w != 0.f) {   // xhat = x + sqrt(2 D(t) dt) w
        sde::PerturbArgs pa{z, noise ? noise + (size_t)i * n : nullptr, B, e_row, noise ? sde::kNoiseArray : sde::kNoisePhilox, a_w, ba.g};
        pa.g.step = (uint32_t)i;
        sde::sde_perturb_kernel<<<cdiv(n / 4, 256), 256, 0, st>>>(pa);
      }
      if ((rc = eval(z, w.dz, false, i, nullptr))) return rc;                                 // K1 = f(xhat, t)
      axpy_kernel<<<cdiv(n, 256), 256, 0, st>>>(z, w.dz, w.ztmp, dt, n);                      // xp = xhat + dt K1
      if ((rc = eval(w.ztmp, w.k2, false, i, nullptr))) return rc;                            // K2 = f(xp, t + dt)
      heun_kernel<<<cdiv(n, 256), 256, 0, st>>>(z, w.dz, w.k2, 0.5f * dt, n);                 // x = xhat + dt / 2 (K1 + K2)
      if (trj) HIP_TRY(hipMemcpyAsync(trj, z, n * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    LAUNCH_CHECK();
  }
  float* trj = traj ? traj + (size_t)n_steps * n : nullptr;
  if (has_last) {
    if ((rc = eval(z, z, false, n_steps, trj))) return rc;
  } else if (trj) HIP_TRY(hipMemcpyAsync(trj, z, n * sizeof(float), hipMemcpyDeviceToDevice, st));   // the reference appends the unchanged state
  return SCLDM_OK;
}

// ---- ODE sampling under a noise / score transport (transport_path.hpp) ------------------------------------------------------------------
// The probability-flow drift of such a model is f = a(t) x + b(t) m with m the CFG-blended model output (transport.py:152-183), over
// linspace(sample_eps, 1 - sample_eps, n_steps + 1).  The conditioning, the trunk and the Heun kernels are scldm_sample_ode's; the
// evaluation times go through the explicit list of the SDE entry; ONE elementwise kernel after the trunk blends, maps and (Euler) steps.
namespace {
struct DriftArgs {
  const float* v;       // trunk output: 2B unconditional rows, then P conditional passes of B rows (direct: 2B rows, the result itself)
  const float* x;       // (2B, e) the state the evaluation was made at
  float* f;             // (2B, e) receives f = a x + b m, or NULL
  float* z;             // Euler: the state, z += h f; or NULL
  int B, e, P, direct;
  float scale[kMaxClasses];
  float a, b, h;        // rounded to fp32 once on the host
};
// thread = 4 consecutive elements (16 bytes), no LDS
__global__ __launch_bounds__(256) void cfg_blend_drift_kernel(const DriftArgs a) {
#pragma clang fp contract(off)   // every product and sum rounded on its own (the blend keeps cfg_blend_kernel's contracted statement)
  const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t half = (size_t)a.B * a.e, half4 = half >> 2;
  if (q >= 2 * half4) return;
  const size_t i = q * 4;
  f32x4 r = reinterpret_cast<const f32x4*>(a.v)[q];
  if (!a.direct && q >= half4) {
    const float* vc = a.v + 2 * half + (i - half);   // pass 0 of these elements; pass p is p * half further
    const f32x4 u = r;
    for (int p = 0; p < a.P; ++p) r = sde::cfg_blend_pass(r, *reinterpret_cast<const f32x4*>(vc + (size_t)p * half), u, a.scale[p]);
  }
  const f32x4 x = reinterpret_cast<const f32x4*>(a.x)[q];
  const f32x4 f = x * a.a + r * a.b;
  if (a.f) reinterpret_cast<f32x4*>(a.f)[q] = f;
  if (a.z) {
    f32x4* zp = reinterpret_cast<f32x4*>(a.z);
    zp[q] = zp[q] + f * a.h;
  }
}
}  // namespace

extern "C" int scldm_sample_ode_transport(scldm_dit* h, float* z, const int64_t* const* ulabels, int n_urows, const int32_t* cell_row, int B,
                                          int n_pass, const uint32_t* pass_mask, const float* pass_scale, int n_steps, int method,
                                          const scldm_transport* tr, int precision, void* ws_, void* stream_) {
  if (!tpath::transport_valid(tr))
    return fail(SCLDM_ERR_SHAPE, "scldm_sample_ode_transport: bad transport (Linear | GVP, velocity | noise | score, 0 <= eps < 0.5)");
  if (tr->model == SCLDM_MODEL_VELOCITY)   // a velocity model's drift is the model output over [0, 1] on either path: the existing solve
    return scldm_sample_ode(h, z, ulabels, n_urows, cell_row, B, n_pass, pass_mask, pass_scale, n_steps, method, precision, ws_, stream_);
  int rc = check_ready(h, precision);
  if (rc) return rc;
  if (!z || !ws_) return fail(SCLDM_ERR_SHAPE, "null pointer argument");
  if ((uintptr_t)z & 15) return fail(SCLDM_ERR_SHAPE, "z must be 16-byte aligned");
  if (n_steps < 1) return fail(SCLDM_ERR_SHAPE, "n_steps must be >= 1");
  if (method != SCLDM_METHOD_EULER && method != SCLDM_METHOD_HEUN) return fail(SCLDM_ERR_SHAPE, "unknown method %d", method);
  if (!(tr->sample_eps > 0.f))
    return fail(SCLDM_ERR_SHAPE, "a noise / score model needs sample_eps > 0: its drift is singular at t = 0 (alpha'/alpha) and at t = 1 (noise: 1 / sigma)");
  FusedSolve s;
  if ((rc = s.plan(h, ulabels, n_urows, cell_row, B, n_pass, pass_mask, pass_scale, precision, ws_, stream_))) return rc;
  const int e_row = 16 * h->cfg.n_embed_input;
  if (e_row % 4 || s.n / 4 > 0x7fffffffull) return fail(SCLDM_ERR_SHAPE, "state rows must be a multiple of 4 elements, at most 2^33 elements in all");
  const bool heun = method == SCLDM_METHOD_HEUN;
  double td0, td1;
  tpath::transport_interval(tr, true, &td0, &td1);
  const float ta = (float)td0, tb = (float)td1;
  const std::vector<float> tl = grid::eval_times(n_steps, ta, tb, heun ? grid::kNext : grid::kNone);
  if ((rc = s.prepare(tl))) return rc;
  DriftArgs da{};
  da.v = s.w.v;
  da.B = B;
  da.e = e_row;
  da.P = s.pl.P;
  da.direct = s.pl.direct ? 1 : 0;
  fill_pass_scale(da.scale, s.pl.P, s.pl.scale);
  // one evaluation at zin: the Euler step z += hs f (euler_z given), or f_out = a zin + b m
  auto eval = [&](int e, const float* zin, float* f_out, float* euler_z, float hs) -> int {
    int rc2 = s.eval(e, zin, s.w.v);
    if (rc2) return rc2;
    scldm_transport_coef k;
    tpath::transport_coef(tr->path, tr->model, tr->weight, (double)tl[e], &k);
    da.x = zin;
    da.f = euler_z ? nullptr : f_out;
    da.z = euler_z;
    da.a = (float)k.a;
    da.b = (float)k.b;
    da.h = hs;
    cfg_blend_drift_kernel<<<cdiv(s.n / 4, 256), 256, 0, s.st>>>(da);
    LAUNCH_CHECK();
    return SCLDM_OK;
  };
  return s.step_loop(n_steps, ta, tb, heun, z, eval);
}

extern "C" void scldm_dit_block_timing_enable(scldm_dit* h, int enable) {
  if (!h) return;
  h->timing = enable != 0;
  h->ev_used = 0;
}
extern "C" int scldm_dit_block_timing(scldm_dit* h, int* n_launches, double* total_ms) {
  if (!h) return fail(SCLDM_ERR_SHAPE, "null handle");
  double tot = 0;
  int n = 0;
  for (size_t i = 0; i + 1 < h->ev_used; i += 2) {
    HIP_TRY(hipEventSynchronize(h->ev[i + 1]));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, h->ev[i], h->ev[i + 1]));
    tot += ms;
    ++n;
  }
  if (n_launches) *n_launches = n;
  if (total_ms) *total_ms = tot;
  h->ev_used = 0;
  return SCLDM_OK;
}

// ---- measurement aid: what the matrix pipe sustains on THIS device under its power budget -------------------------------------------
// A register-only v_mfma_f32_32x32x16_bf16 loop (two waves per SIMD, four independent accumulators, no memory traffic) on operand
// fragments of a given fill.  The instruction stream is the same for every fill; the rate differs because the part clocks to its
// power budget (MI355X_MICROARCH.md "DVFS give-back"): zero operands run near the nominal 2.5 PFLOP/s, N(0,1) operands at about half
// of it (profiles/r4c_mfma_power_ceiling.txt).  bench.py reports the figure beside roofline.frac, whose denominator stays nominal.
template <bool F16>
__global__ __launch_bounds__(256, 2) void mfma_ceiling_kernel(const bf16x8* __restrict__ frags_, float* __restrict__ out, int iters) {
  using Frag = typename std::conditional<F16, f16x8, bf16x8>::type;
  const Frag* __restrict__ frags = reinterpret_cast<const Frag*>(frags_);
  const int lane = threadIdx.x & 63;
  Frag a[4], b[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    a[i] = frags[(i * 2 + 0) * 64 + lane];
    b[i] = frags[(i * 2 + 1) * 64 + lane];
  }
  f32x16 acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if constexpr (F16) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[(i + u) & 3], b[(i + 2 * u + 1) & 3], acc[i], 0, 0, 0);
        else acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[(i + u) & 3], b[(i + 2 * u + 1) & 3], acc[i], 0, 0, 0);
      }
  }
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) s += acc[i][r];
  if (s == 12345.678f) out[blockIdx.x * 256 + threadIdx.x] = s;   // keeps the loop alive; never true in practice
}
// ---- Dormand-Prince 5(4) state arithmetic (ode_rk.hpp); pointer tables and coefficients are HOST arrays, passed by value ----
static int rk_args(scldm::rk::CombArgs* a, const float* const* k, const float* coef, int n_k, const char* who) {
  if (n_k < 0 || n_k > scldm::rk::kMaxK || (n_k && (!k || !coef))) return fail(SCLDM_ERR_SHAPE, "%s: 0..%d stage tensors", who, scldm::rk::kMaxK);
  a->n_k = n_k;
  for (int j = 0; j < n_k; ++j) {
    if (!k[j]) return fail(SCLDM_ERR_SHAPE, "%s: stage tensor %d is NULL", who, j);
    a->k[j] = k[j];
    a->c[j] = coef[j];
  }
  return SCLDM_OK;
}
extern "C" int scldm_rk_combine(float* out, const float* y0, const float* const* k, const float* coef, int n_k, long long n, void* stream_) {
  if (!out || n < 1 || n % 4) return fail(SCLDM_ERR_SHAPE, "scldm_rk_combine: n must be a positive multiple of 4");
  scldm::rk::CombArgs a{};
  int rc = rk_args(&a, k, coef, n_k, "scldm_rk_combine");
  if (rc) return rc;
  hipLaunchKernelGGL(scldm::rk::combine_kernel, dim3((unsigned)cdiv(n / 4, 256)), dim3(256), 0, (hipStream_t)stream_, out, y0, a, (long)(n / 4));
  LAUNCH_CHECK();
  return SCLDM_OK;
}
extern "C" int scldm_rk_error(const float* y0, const float* y1, const float* const* k, const float* coef, int n_k, long long n, float atol, float rtol,
                              void* ws, void* stream_) {
  if (!y0 || !y1 || !ws || n < 1) return fail(SCLDM_ERR_SHAPE, "scldm_rk_error: bad argument");
  scldm::rk::CombArgs a{};
  int rc = rk_args(&a, k, coef, n_k, "scldm_rk_error");
  if (rc) return rc;
  double* w = reinterpret_cast<double*>(ws);     // [0, 1022) block partials | [1022] mean of squared ratios | [1023] unused since round 6
  const unsigned blocks = (unsigned)std::min<long long>(cdiv(n, 256 * 8), 1022);
  hipLaunchKernelGGL(scldm::rk::error_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream_, y0, y1, a, (long)n, atol, rtol, w);
  hipLaunchKernelGGL(scldm::rk::error_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream_, w, blocks, (long)n, w + 1022);
  LAUNCH_CHECK();
  return SCLDM_OK;
}
extern "C" int scldm_rk_dense(const float* y0, const float* y1, const float* const* k, const float* mid_coef, int n_k, const float* fa, const float* fb,
                              float h, float two_h, long long n, float* c1, float* c2, float* c3, float* c4, void* stream_) {
  if (!y0 || !y1 || !fa || !fb || !c1 || !c2 || !c3 || !c4 || n < 1) return fail(SCLDM_ERR_SHAPE, "scldm_rk_dense: bad argument");
  scldm::rk::CombArgs a{};
  int rc = rk_args(&a, k, mid_coef, n_k, "scldm_rk_dense");
  if (rc) return rc;
  hipLaunchKernelGGL(scldm::rk::dense_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream_, y0, y1, a, fa, fb, h, two_h, (long)n, c1,
                     c2, c3, c4);
  LAUNCH_CHECK();
  return SCLDM_OK;
}
extern "C" int scldm_rk_poly(float* out, const float* c0, const float* c1, const float* c2, const float* c3, const float* c4, float s1, float s2, float s3,
                             float s4, long long n, void* stream_) {
  if (!out || !c0 || !c1 || !c2 || !c3 || !c4 || n < 1 || n % 4) return fail(SCLDM_ERR_SHAPE, "scldm_rk_poly: n must be a positive multiple of 4");
  hipLaunchKernelGGL(scldm::rk::poly_kernel, dim3((unsigned)cdiv(n / 4, 256)), dim3(256), 0, (hipStream_t)stream_, out, c0, c1, c2, c3, c4, s1, s2, s3, s4,
                     (long)(n / 4));
  LAUNCH_CHECK();
  return SCLDM_OK;
}

extern "C" int scldm_mfma_sustained_tflops(int fill, int iters, double* tflops) {
  const bool f16 = (fill & 4) != 0;   // fill | 4: the same loop on v_mfma_f32_32x32x16_f16 (fp16 fragments of the same values)
  fill &= ~4;
  if (!tflops || fill < 0 || fill > 2 || iters < 1) return fail(SCLDM_ERR_SHAPE, "scldm_mfma_sustained_tflops: bad argument");
  const int blocks = 512, launches = 5;   // 2 workgroups of 4 waves per CU
  std::vector<__bf16> hfr(8 * 64 * 8);
  unsigned long long st = 0x9E3779B97F4A7C15ull;   // splitmix64: the same fragments on every box
  auto u01 = [&]() {
    st += 0x9E3779B97F4A7C15ull;
    unsigned long long z = st;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return ((double)(z >> 11) + 0.5) / 9007199254740992.0;
  };
  for (auto& v : hfr) {
    float x = 0.f;
    if (fill == 1) x = (float)(2.0 * u01() - 1.0);
    if (fill == 2) x = (float)(sqrt(-2.0 * log(u01())) * cos(6.283185307179586 * u01()));
    if (f16) { const _Float16 hx = (_Float16)x; memcpy(&v, &hx, 2); }
    else v = (__bf16)x;
  }
  bf16x8* d_fr = nullptr;
  float* d_out = nullptr;
  HIP_TRY(hipMalloc((void**)&d_fr, hfr.size() * sizeof(__bf16)));
  hipError_t e = hipMalloc((void**)&d_out, (size_t)blocks * 256 * sizeof(float));
  if (e != hipSuccess) { (void)hipFree(d_fr); return fail(SCLDM_ERR_HIP, "hipMalloc: %s", hipGetErrorString(e)); }
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int rc = SCLDM_OK;
  auto run = [&]() -> int {
    HIP_TRY(hipMemcpy(d_fr, hfr.data(), hfr.size() * sizeof(__bf16), hipMemcpyHostToDevice));
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    auto kern = f16 ? mfma_ceiling_kernel<true> : mfma_ceiling_kernel<false>;
    kern<<<blocks, 256, 0, 0>>>(d_fr, d_out, iters / 8 + 1);   // warm-up
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipEventRecord(e0, 0));
    for (int k = 0; k < launches; ++k) kern<<<blocks, 256, 0, 0>>>(d_fr, d_out, iters);
    HIP_TRY(hipEventRecord(e1, 0));
    HIP_TRY(hipEventSynchronize(e1));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    *tflops = (double)launches * blocks * 4.0 * iters * 16.0 * 2.0 * 32 * 32 * 16 / ((double)ms * 1e9);
    return SCLDM_OK;
  };
  rc = run();
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  (void)hipFree(d_fr);
  (void)hipFree(d_out);
  return rc;
}

// Debug hook: device buffer receiving per-(block, wave) s_memtime phase stamps of the LAST fused-block launch
// (16 x u64 per wave).  Only -DSCLDM_PHASE_TIMING builds write it; production builds return SCLDM_ERR_STATE.
extern "C" int scldm_dit_set_debug_buffer(scldm_dit* h, void* dev_buf) {
  if (!h) return fail(SCLDM_ERR_SHAPE, "null handle");
#ifdef SCLDM_PHASE_TIMING
  h->dbg = (unsigned long long*)dev_buf;
  return SCLDM_OK;
#else
  (void)dev_buf;
  return fail(SCLDM_ERR_STATE, "phase timing is not compiled in (build with -DSCLDM_PHASE_TIMING)");
#endif
}

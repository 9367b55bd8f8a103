// C ABI of the fused evaluation metrics (include/scldm_hip.h): scldm_eval_count_metrics, scldm_log1p_normalize, scldm_gaussian_recon_loss.
#include <hip/hip_runtime.h>

#include "api_common.hpp"
#include "eval_metrics.hpp"

using namespace scldm;

namespace {
struct EvalLayout {   // byte offsets into the caller's workspace; a function of (n_pred, n_true, G) only
  int nrb_p, nrb_t, tiles;
  size_t plane;       // floats per partial plane
  size_t scale_p, scale_t, part, wg, gene, total;
};

EvalLayout eval_layout(int n_pred, int n_true, int G) {
  EvalLayout l;
  l.nrb_p = cdiv(n_pred, eval_row_block(n_pred));
  l.nrb_t = cdiv(n_true, eval_row_block(n_true));
  l.tiles = cdiv(G, kEvalTileG);
  l.plane = (size_t)(l.nrb_p > l.nrb_t ? l.nrb_p : l.nrb_t) * G;
  size_t o = 0;
  auto take = [&](size_t bytes) { size_t r = o; o += align256(bytes); return r; };
  l.scale_p = take((size_t)n_pred * 4);
  l.scale_t = take((size_t)n_true * 4);
  l.part = take(5 * l.plane * 4);
  l.wg = take((size_t)l.tiles * l.nrb_p * 2 * 8);
  l.gene = take((size_t)5 * G * 8);
  l.total = o;
  return l;
}
}  // namespace

extern "C" size_t scldm_eval_workspace_bytes(int n_pred, int n_true, int G) {
  if (n_pred < 1 || n_true < 1 || G < 1) return 0;
  return eval_layout(n_pred, n_true, G).total;
}

extern "C" int scldm_eval_count_metrics(const float* pred, int n_pred, const float* truth, int n_true, int G, const float* pred_div,
                                        const float* true_div, float target_sum, double* out, float* pcc_per_gene, float* gene_stats,
                                        void* ws, void* stream_) {
  if (!pred || !truth || !out || !ws) return fail(SCLDM_ERR_SHAPE, "null argument");
  if (n_pred < 1 || n_true < 1 || G < 1) return fail(SCLDM_ERR_SHAPE, "need n_pred, n_true, G >= 1 (got %d, %d, %d)", n_pred, n_true, G);
  hipStream_t st = (hipStream_t)stream_;
  const EvalLayout l = eval_layout(n_pred, n_true, G);
  char* base = (char*)ws;
  float *scale_p = (float*)(base + l.scale_p), *scale_t = (float*)(base + l.scale_t), *part = (float*)(base + l.part);
  double *wg = (double*)(base + l.wg), *gene = (double*)(base + l.gene);
  const bool raw = !(target_sum > 0.f), paired = n_pred == n_true;
  const float *sp = pred_div, *stv = true_div;
  if (!raw) {
    if (!pred_div) {
      hipLaunchKernelGGL(eval_row_scale_kernel, dim3(n_pred), dim3(256), 0, st, pred, G, target_sum, scale_p);
      sp = scale_p;
    }
    if (!true_div) {
      hipLaunchKernelGGL(eval_row_scale_kernel, dim3(n_true), dim3(256), 0, st, truth, G, target_sum, scale_t);
      stv = scale_t;
    }
  }
  const int dp = pred_div != nullptr, dt = true_div != nullptr;
  const int rb_p = eval_row_block(n_pred), rb_t = eval_row_block(n_true);
  if (paired) {
    const dim3 grid(l.tiles, l.nrb_p);
    if (raw) hipLaunchKernelGGL((eval_moments_kernel<true, true>), grid, dim3(256), 0, st, pred, truth, n_pred, G, rb_p, sp, dp, stv, dt, target_sum, part, l.plane, 0, wg);
    else hipLaunchKernelGGL((eval_moments_kernel<true, false>), grid, dim3(256), 0, st, pred, truth, n_pred, G, rb_p, sp, dp, stv, dt, target_sum, part, l.plane, 0, wg);
  } else {
    const dim3 gp(l.tiles, l.nrb_p), gt(l.tiles, l.nrb_t);
    const float* none = nullptr;
    if (raw) {
      hipLaunchKernelGGL((eval_moments_kernel<false, true>), gp, dim3(256), 0, st, pred, none, n_pred, G, rb_p, sp, dp, none, 0, target_sum, part, l.plane, 0, wg);
      hipLaunchKernelGGL((eval_moments_kernel<false, true>), gt, dim3(256), 0, st, truth, none, n_true, G, rb_t, stv, dt, none, 0, target_sum, part, l.plane, 2, wg);
    } else {
      hipLaunchKernelGGL((eval_moments_kernel<false, false>), gp, dim3(256), 0, st, pred, none, n_pred, G, rb_p, sp, dp, none, 0, target_sum, part, l.plane, 0, wg);
      hipLaunchKernelGGL((eval_moments_kernel<false, false>), gt, dim3(256), 0, st, truth, none, n_true, G, rb_t, stv, dt, none, 0, target_sum, part, l.plane, 2, wg);
    }
  }
  LAUNCH_CHECK();
  hipLaunchKernelGGL(eval_merge_kernel, dim3(cdiv(G, kEvalMergeThreads)), dim3(kEvalMergeThreads), 0, st, part, l.plane, G, n_pred, n_true, (int)paired, gene, pcc_per_gene,
                     gene_stats);
  hipLaunchKernelGGL(eval_finalize_kernel, dim3(1), dim3(kEvalFinalThreads), 0, st, gene, G, wg, l.tiles * l.nrb_p, (double)n_pred, (int)paired, out);
  LAUNCH_CHECK();
  return SCLDM_OK;
}

extern "C" int scldm_log1p_normalize(const float* x, int n, int G, const float* div, float target_sum, float* out, void* stream_) {
  if (!x || !out) return fail(SCLDM_ERR_SHAPE, "null argument");
  if (n < 1 || G < 1) return fail(SCLDM_ERR_SHAPE, "need n >= 1 and G >= 1 (got %d, %d)", n, G);
  hipLaunchKernelGGL(eval_log1p_normalize_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream_, x, G, div, target_sum, out);
  LAUNCH_CHECK();
  return SCLDM_OK;
}

extern "C" int scldm_gaussian_recon_loss(const float* counts, const float* mu, int B, int G, float target_sum, float* loss_rows, void* stream_) {
  if (!counts || !mu || !loss_rows) return fail(SCLDM_ERR_SHAPE, "null argument");
  if (B < 1 || G < 1) return fail(SCLDM_ERR_SHAPE, "need B >= 1 and G >= 1 (got %d, %d)", B, G);
  hipLaunchKernelGGL(gaussian_recon_loss_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream_, counts, mu, G, target_sum, loss_rows);
  LAUNCH_CHECK();
  return SCLDM_OK;
}

extern "C" int scldm_gaussian_recon_loss_bwd(const float* counts, const float* mu, const float* gout_rows, int B, int G, float target_sum,
                                             float* dmu, void* stream_) {
  if (!counts || !mu || !gout_rows || !dmu) return fail(SCLDM_ERR_SHAPE, "null argument");
  if (B < 1 || G < 1) return fail(SCLDM_ERR_SHAPE, "need B >= 1 and G >= 1 (got %d, %d)", B, G);
  hipLaunchKernelGGL(gaussian_recon_loss_bwd_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream_, counts, mu, gout_rows, G, target_sum, dmu);
  LAUNCH_CHECK();
  return SCLDM_OK;
}

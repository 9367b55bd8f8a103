// The plan of one classifier-free-guidance evaluation, shared by every entry that runs one: the fused family (api.hip), the record-free
// wide path (train_api.hip: infer_wide_api.inc) and the log-likelihood solve (logp_api.hip).  Host code only.
#pragma once
#include "api_common.hpp"
#include "dit_handle.hpp"

// One CFG evaluation: dz (2B, e) = forward_with_cfg(z, t) over 2B unconditional sample-forwards and P conditional passes of B.
struct CfgPlan {
  int B, P, U, uncond_rows, n_fwd, n_rows;
  bool direct;   // SCLDM_OPT_CFG1_DIRECT applies: rows [B, 2B) run the conditional forward only (guided = conditional at scale 1);
                 // honoured by the fused family alone - the wide path and the likelihood solve always blend
  const int64_t* const* ulabels;
  const int32_t* cell_row;
  uint32_t mask[SCLDM_MAX_CLASSES];
  float scale[SCLDM_MAX_CLASSES];
};

// t_stride: 0 (one scalar t), 1 (one t per sample) or 2 (dense t, uniformity decided on device)
static inline int make_plan(const scldm_dit* h, CfgPlan& pl, const int64_t* const* ulabels, int n_urows, const int32_t* cell_row, int B,
                            int n_pass, const uint32_t* pass_mask, const float* pass_scale, int t_stride) {
  if (B <= 0) return fail(SCLDM_ERR_SHAPE, "B must be positive");
  if (!h->cfg.has_null_row && h->cfg.n_classes > 0)
    return fail(SCLDM_ERR_SHAPE, "classifier-free guidance needs the null rows of the class tables (model built with cfg_dropout_prob == 0)");
  if (n_pass < 0 || n_pass > SCLDM_MAX_CLASSES) return fail(SCLDM_ERR_SHAPE, "n_pass out of range");
  if (n_pass > 0 && (!ulabels || !pass_mask || !pass_scale || n_urows <= 0)) return fail(SCLDM_ERR_SHAPE, "conditional passes need labels/masks/scales");
  if (n_pass > 0 && !cell_row && n_urows != B) return fail(SCLDM_ERR_SHAPE, "cell_row is NULL but n_urows (%d) != B (%d)", n_urows, B);
  if (t_stride == 1 && n_pass > 0 && (cell_row || n_urows != B))
    return fail(SCLDM_ERR_SHAPE, "per-sample t (t_stride=1) requires per-cell label rows (n_urows == B, cell_row NULL)");
  pl.B = B;
  pl.P = n_pass;
  pl.U = n_pass > 0 ? n_urows : 0;
  pl.uncond_rows = (t_stride == 0) ? 1 : 2 * B;
  pl.n_fwd = 2 * B + n_pass * B;
  pl.n_rows = (t_stride == 2) ? 2 * B + n_pass * B /* the larger, dense plan sizes the workspace */ : pl.uncond_rows + pl.P * pl.U;
  pl.ulabels = ulabels;
  pl.cell_row = cell_row;
  pl.direct = h->cfg1_direct && t_stride == 0 && n_pass == 1 && pass_scale[0] == 1.0f;
  for (int p = 0; p < n_pass; ++p) {
    pl.mask[p] = pass_mask[p];
    pl.scale[p] = pass_scale[p];
  }
  return SCLDM_OK;
}

// the guidance scales as a blend kernel's argument struct carries them: P entries, the rest zero
static inline void fill_pass_scale(float* dst, int P, const float* scale) {
  for (int p = 0; p < SCLDM_MAX_CLASSES; ++p) dst[p] = p < P ? scale[p] : 0.f;
}

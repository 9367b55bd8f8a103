// Launchers of the kernels of the record-free inference path of shapes outside the fused family (infer_wide.hip), called by
// infer_wide_api.inc in train_api.hip.  Their own translation unit: train_api.hip's device code stays what it was.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/scldm_hip.h"

// the class tables of cond_sum_rows_kernel (EmbedArgs of train.hpp): labels[c] == NULL selects the null token (row vocab[c]) for every row
struct InferEmbed {
  const float* table[SCLDM_MAX_CLASSES];
  const int64_t* labels[SCLDM_MAX_CLASSES];
  int vocab[SCLDM_MAX_CLASSES];
  int n_classes;
};

// h = LN(x') (1 + scale[r]) + shift[r] with r = ridx[sample] (ridx NULL: the sample itself); y != NULL: x' = x + gate[r] * y is formed first
// and written to x_out (ln_mod_fwd_kernel's fused residual).  y16 / h16: y / h are bf16 arrays.  D % 256 == 0, D <= 2048.
int scldm_infer_ln_rows(hipStream_t st, int D, const float* x, const void* y, bool y16, int g_off, float* x_out, const float* mod, long mw,
                        const int32_t* ridx, int sc_off, int sh_off, float eps, long T, void* h, bool h16);
// out = x + gate[ridx[sample]] * y
int scldm_infer_gate_res_rows(hipStream_t st, const float* x, const void* y, bool y16, const float* mod, long mw, const int32_t* ridx, int g_off,
                              long T, int D, float* out);
// c[i] = temb[i * temb_stride] + sum of the class embeddings of row i (temb_stride 0: one timestep embedding for all n rows)
int scldm_infer_cond_sum_rows(hipStream_t st, const float* temb, long temb_stride, const InferEmbed& e, int n, int D, float* c);
// x0 of sample-forward s >= n_direct = x0 of sample n_direct - rep + (s - n_direct) % rep; row = floats per sample
int scldm_infer_rep_rows(hipStream_t st, float* x0, int n_direct, int rep, int n_fwd, long row);
// t[i] = the time of evaluation e0 + i of a fixed-grid solve over linspace(0, 1, steps), i < m
int scldm_infer_grid_times(hipStream_t st, float* t, int steps, int heun, int e0, int m);

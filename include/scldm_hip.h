/*
 * scldm_hip.h - C ABI of libscldm_hip.so: the MI355X (gfx950) implementation of the scLDM
 * latent-diffusion hot path.  Plain pointers and sizes only; no torch types.
 *
 * The reference (czi-ai/scldm) has no FFI: its seam is Hydra `_target_` instantiation of
 * nn.Modules.  Each entry point below therefore cites the reference
 * Python method it replaces; the ctypes binding a maintainer would add is shown in INTEGRATION.md
 * and implemented in scldm_amd/_lib.py.
 *
 * Conventions
 *  - every pointer named `d_*` or documented "device" is a device (HBM) pointer; tensors are
 *    contiguous, row-major, fp32 unless stated; labels are int64 (torch.long);
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued asynchronously on it;
 *  - no hidden allocation in hot calls: the caller provides `ws` of at least
 *    scldm_dit_workspace_bytes(...) bytes (256-byte aligned);
 *  - return value: 0 on success, SCLDM_ERR_* (<0) otherwise; scldm_last_error() returns a
 *    thread-local message;
 *  - a handle belongs to one device and one host thread at a time.
 */
#ifndef SCLDM_HIP_H
#define SCLDM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCLDM_OK 0
#define SCLDM_ERR_SHAPE (-1)   /* unsupported / inconsistent shape or argument */
#define SCLDM_ERR_HIP (-2)     /* HIP runtime error (text in scldm_last_error) */
#define SCLDM_ERR_STATE (-3)   /* e.g. weights not loaded */

#define SCLDM_MAX_CLASSES 8

#define SCLDM_PREC_FP32 0  /* exact-fp32 MFMA (v_mfma_f32_32x32x2_f32): parity path, <=1e-4 vs reference */
#define SCLDM_PREC_BF16 1  /* bf16 operands, fp32 accumulate / LN / softmax / residual: throughput path */
#define SCLDM_PREC_BF16X3 2 /* split-bf16: every GEMM operand as hi + lo bf16, three v_mfma_f32_32x32x16_bf16 per k-step (hi*hi, hi*lo,
                             * lo*hi), fp32 accumulate - the arithmetic class of the reference's
                             * torch.set_float32_matmul_precision("high") (experiments/scripts/inference.py:26); ~1e-5 vs fp32,
                             * inside the 1e-4 parity gate at 5x the exact-fp32 MFMA rate.  Fused DiT inference kernels; the training /
                             * generic entry points serve it with the exact-fp32 GEMM route (same parity class). */

#define SCLDM_PREC_FP16 3  /* fp16 operands (v_mfma_f32_32x32x16_f16), fp32 accumulate / LN / softmax / residual: 10 mantissa bits = the
                            * TF32 arithmetic the reference runs under set_float32_matmul_precision("high") (inference.py:26,
                            * train_ldm.py:18) at the bf16 MFMA rate.  Fused DiT inference kernels; range |w| <= 65 504 checked at
                            * pack time (scldm_dit_fp16_stats).  Training / generic entry points: exact-fp32 route. */

#define SCLDM_METHOD_EULER 0
#define SCLDM_METHOD_HEUN 1

typedef struct scldm_dit scldm_dit;

/* Mirror of scldm.nnets.DiT.__init__ kwargs (reference src/scldm/nnets.py:219-234).
 * Classes are listed in SORTED NAME ORDER (the reference iterates sorted(class_vocab_sizes), :393,:404,:438). */
typedef struct {
  int n_embed;        /* 256 for the fused inference kernels; any multiple of 256 (<= 2048) on the generic scldm_dit_train_* path */
  int n_embed_input;  /* latent channels, <= 64 */
  int n_layer;
  int n_head;         /* 8 (head_dim 32) fused; head_dim 32 or 64 on the generic path */
  int seq_len;        /* 16 */
  int hidden_dim;     /* SwiGLU hidden (684 for n_embed 256, multiple_of 4), layers.py:165-167 */
  float layernorm_eps;
  int n_classes;
  int class_vocab[SCLDM_MAX_CLASSES]; /* vocab size per class; the null token index equals it */
  int has_null_row;   /* 1: class tables have vocab+1 rows (cfg_dropout_prob > 0, nnets.py:241-243); 0: vocab rows - every entry point
                       * that would need a null token (unconditional CFG pass, unselected class) then returns SCLDM_ERR_SHAPE, where
                       * the reference's nn.Embedding raises IndexError */
} scldm_dit_config;

/* Device pointers to the reference's parameters in their PyTorch layouts (Linear.weight is (out,in)).
 * state_dict keys: SURVEY.md section 8b.  Per-layer arrays are HOST arrays of n_layer device pointers. */
typedef struct {
  const float* pos_embed;                 /* pos_embed (1,S,D) */
  const float* t_w0; const float* t_b0;   /* t_embedder.mlp.0 (D,256),(D) */
  const float* t_w2; const float* t_b2;   /* t_embedder.mlp.2 (D,D),(D) */
  const float* in_w; const float* in_b;   /* input_proj (D,Din),(D) */
  const float* fin_w; const float* fin_b; /* final_layer.linear (Din,D),(Din) */
  const float* fin_ada_w; const float* fin_ada_b; /* final_layer.adaln_modulation.1 (2D,D),(2D) */
  const float* const* class_emb;          /* n_classes x class_embeddings.<name>.weight (vocab+1,D), sorted-name order */
  const float* const* attn_w; const float* const* attn_b;   /* blocks.i.attn.c_attn (3D,D),(3D) */
  const float* const* proj_w; const float* const* proj_b;   /* blocks.i.attn.c_proj (D,D),(D) */
  const float* const* w1; const float* const* w2;           /* blocks.i.mlp.w1/w2 (H,D) */
  const float* const* cproj;                                /* blocks.i.mlp.c_proj (D,H) */
  const float* const* ada_w; const float* const* ada_b;     /* blocks.i.adaln_modulation.1 (6D,D),(6D) */
} scldm_dit_weights;

const char* scldm_last_error(void);
int scldm_version(void);

/* A handle for a shape outside the fused family (n_embed 256, n_head 8, seq_len 16, n_embed_input <= 32) is valid for
 * scldm_dit_train_forward / _backward only; the fused entry points return SCLDM_ERR_SHAPE for it. */
int scldm_dit_create(const scldm_dit_config* cfg, scldm_dit** out);
void scldm_dit_destroy(scldm_dit* h);

/* Re-pack weights from the caller's parameter tensors into MFMA fragment streams (fp32, bf16 and split-bf16
 * copies) in one launch.  Sources stay owned by the caller and must stay allocated while the handle is used:
 * their addresses are remembered for scldm_dit_refresh_weights. */
int scldm_dit_load_weights(scldm_dit* h, const scldm_dit_weights* w, void* stream);

/* Cheap staleness guard for callers that cannot know whether the parameter tensors were modified in place
 * (e.g. ema_pytorch updates through `.data`, which does not bump torch's version counter; reference
 * src/scldm/models.py:446,690): fingerprints the tensors given to the last scldm_dit_load_weights ON DEVICE (every
 * element of every tensor: one read of the parameters, ~10 us for the base DiT) and re-packs, in the same stream and without a
 * host synchronisation, only if the fingerprint changed.  Three small launches when nothing changed. */
int scldm_dit_refresh_weights(scldm_dit* h, void* stream);

/* Range report of the fp16 weight stream packed by the last load / refresh (synchronises `stream`): values beyond +-65 504
 * (stored as inf: SCLDM_PREC_FP16 must not be used), non-zero values below the smallest fp16 normal 6.1e-5 (stored with fewer
 * than 10 mantissa bits) and the non-zero values packed. */
int scldm_dit_fp16_stats(scldm_dit* h, long long* overflow, long long* subnormal, long long* nonzero, void* stream);

/* AdamW step over every parameter tensor in ONE launch (csrc/optim.hip) - the optimizer of the reference's trainer is
 * torch.optim.AdamW (src/scldm/models.py configure_optimizers; experiments/configs/training/default.yaml); same arithmetic as torch's
 * fused AdamW.  `entries` is a HOST array (device pointers inside); `step` a device float holding the number of steps taken so far
 * (incremented here unless *found_inf != 0, in which case nothing is updated: torch.cuda.amp.GradScaler's protocol and the fp16
 * backward's overflow flag).  Python binding: scldm_amd.optim.AdamW. */
typedef struct {
  float* p;         /* parameter (updated in place) */
  const float* g;   /* gradient */
  float* m;         /* exp_avg */
  float* v;         /* exp_avg_sq */
  long long n;      /* elements */
} scldm_adamw_entry;
int scldm_adamw_step(const scldm_adamw_entry* entries, int count, float* step, const float* found_inf /* may be NULL */, float lr, float beta1,
                     float beta2, float eps, float weight_decay, int maximize, void* stream);

/* The same step driven by a launch table in DEVICE memory (any number of tensors is one launch), with the per-step hyper-parameters
 * read from device memory and the exponential moving average of the reference's trainer in the same pass:
 *   - LatentDiffusion wraps the diffusion model in ema_pytorch.EMA (src/scldm/models.py:446-453; ema-pytorch==0.7.7, pyproject.toml:30)
 *     and calls ema_model.update() after every optimizer step (models.py:83-87); update() copies the online parameters while
 *     step <= update_after_step and does `ema.lerp_(online, 1 - decay)` every update_every steps after (ldm_base.yaml:51-55);
 *   - configure_optimizers attaches a per-step LambdaLR (models.py:603-605).
 * `hyper` (device float[4], may be NULL): [0] learning rate, [1] weight decay, [2] EMA action of THIS step (0 none, 1 copy, 2 lerp),
 * [3] lerp weight.  The caller refreshes it before the call (scldm_amd.optim.AdamW: one 16-byte asynchronous copy); a captured HIP
 * graph therefore follows both schedules.  *found_inf != 0 skips the AdamW update (and the step count) but not the EMA action, as
 * the reference's hook runs after every batch.  The EMA is torch.lerp's arithmetic bit for bit (Tensor.lerp_ / torch._foreach_lerp_).
 * scldm_adamw_table_build fills a HOST buffer of scldm_adamw_table_bytes(...) bytes from the entries (+ one EMA tensor per entry, or
 * NULL); the caller copies it to the device once and passes that copy as `table`. */
size_t scldm_adamw_table_bytes(const scldm_adamw_entry* entries, int count);
int scldm_adamw_table_build(const scldm_adamw_entry* entries, float* const* ema /* count pointers or NULL */, int count, void* table_host,
                            size_t bytes, int* n_blocks);
/* The table is [count tensor records (addresses, size) | workgroup map (sizes only)]: when only addresses changed (autograd handed out
 * another gradient buffer), scldm_adamw_table_update fills just the records (scldm_adamw_table_records_bytes(count) bytes) for the caller
 * to copy over the head of the device table. */
size_t scldm_adamw_table_records_bytes(int count);
int scldm_adamw_table_update(const scldm_adamw_entry* entries, float* const* ema, int count, void* records_host, size_t bytes);
typedef struct {
  const void* table;       /* device copy of the table */
  int count, n_blocks;
  float* step;             /* device: steps taken so far */
  const float* found_inf;  /* device, may be NULL */
  const float* hyper;      /* device float[4], may be NULL (then lr / weight_decay below, no EMA) */
  float lr, beta1, beta2, eps, weight_decay;
  int maximize;
  /* Gradient-norm clipping of the reference's trainer (experiments/configs/training/default.yaml:15-16: gradient_clip_val 10,
   * gradient_clip_algorithm norm -> Lightning calls torch.nn.utils.clip_grad_norm_(parameters, 10.0) between backward and
   * optimizer.step): max_grad_norm > 0 runs two more launches over the same table ahead of the update - the sum of squares of every
   * 4 096-element chunk, then one workgroup summing those partials in a fixed order - and the update reads
   * g * min(1, max_grad_norm / (norm + 1e-6)), torch's clip_coef_clamped.  clip_ws: device memory of
   * scldm_adamw_clip_workspace_bytes(n_blocks) bytes; afterwards clip_ws[0] = the step's total gradient norm (before clipping),
   * clip_ws[1] = the coefficient applied.
   * max_grad_norm <= 0 or clip_ws == NULL: no clipping (the struct of version 4 zero-extended). */
  float max_grad_norm;
  float* clip_ws;
} scldm_adamw_launch;
size_t scldm_adamw_clip_workspace_bytes(int n_blocks);
int scldm_adamw_table_step(const scldm_adamw_launch* launch, void* stream);

/* State arithmetic of the adaptive Dormand-Prince 5(4) solver - the reference's DEFAULT sampler (src/scldm/models.py:793 ->
 * transport/transport.py:324-331 -> integrators.py:100-112 -> torchdiffeq.odeint(method="dopri5")) - as four kernels instead of ~40
 * elementwise launches per step; the step-size control stays on the host (scldm_amd/transport: Sampler._sample_dopri5).  All tensors
 * fp32, contiguous, `n` elements on the device; `k` / `coef` are HOST arrays of n_k <= 7 device pointers / h-scaled tableau weights.
 *   scldm_rk_combine: out = y0 + sum_j coef_j k_j (left to right; y0 may be NULL)                      - stage points
 *   scldm_rk_error:   ws[1022] (double) = mean((sum_j coef_j k_j / (atol + rtol max(|y0|, |y1|)))^2)    - error ratio^2; ws = 8 KB of
 *                     device memory (block partials, summed in block order by a second one-workgroup launch)
 *   scldm_rk_dense:   coefficients c1..c4 of the quartic interpolant of an accepted step (c0 = y0)
 *   scldm_rk_poly:    out = c0 + s1 c1 + s2 c2 + s3 c3 + s4 c4                                           - a save point */
int scldm_rk_combine(float* out, const float* y0, const float* const* k, const float* coef, int n_k, long long n, void* stream);
int scldm_rk_error(const float* y0, const float* y1, const float* const* k, const float* coef, int n_k, long long n, float atol, float rtol,
                   void* ws, void* stream);
int scldm_rk_dense(const float* y0, const float* y1, const float* const* k, const float* mid_coef, int n_k, const float* fa, const float* fb,
                   float h, float two_h, long long n, float* c1, float* c2, float* c3, float* c4, void* stream);
int scldm_rk_poly(float* out, const float* c0, const float* c1, const float* c2, const float* c3, const float* c4, float s1, float s2, float s3,
                  float s4, long long n, void* stream);

/* Overflow guard of the fp16 (loss-scaled) training backward - the counterpart of torch.cuda.amp.GradScaler's found_inf for the
 * reference's trainer (experiments/scripts/train_ldm.py: the reference trains in TF32 and needs none; fp16 operands have TF32's
 * mantissa but 5 exponent bits).  The last launch of scldm_dit_train_backward counts the non-finite values among ALL gradients it
 * produced; when there are any, the NEXT backward lowers its loss scale by one more power of two (the headroom recovers one step
 * per 2 000 clean backwards), and - if the caller registered one with scldm_dit_train_set_found_inf - a device float is set to 1.0
 * (reset to 0.0 at the start of every fp16 backward) so that an optimizer can skip the step without a host read (torch's fused
 * Adam/AdamW take it as `optimizer.found_inf`).  scldm_dit_train_fp16_state synchronises `stream` and reports the loss scale S of
 * the last backward, its non-finite count, the headroom (<= 0, powers of two below the nominal scale) and the number of
 * backwards that overflowed so far. */
int scldm_dit_train_fp16_state(scldm_dit* h, float* scale, long long* nonfinite_last, int* headroom, long long* overflow_steps, void* stream);
int scldm_dit_train_set_found_inf(scldm_dit* h, float* found_inf /* device, caller-owned, may be NULL */);

/* Labels outside [0, vocab] (or == vocab without a null row) are clamped by the conditioning kernels and counted in a
 * device-side sticky counter instead of reading another class's table (the reference's nn.Embedding raises).  This call
 * synchronises `stream`, returns the count since the last call in *count and resets it. */
int scldm_dit_label_errors(scldm_dit* h, int* count, void* stream);

/* Floats per conditioning row: n_layer*6*D + 2*D (all adaLN vectors of all layers + final layer). */
int scldm_dit_mod_width(const scldm_dit* h);

/* Workspace bytes for calls that process up to n_fwd sample-forwards, n_rows conditioning rows and
 * an ODE state of n_state samples (0 when not sampling). */
size_t scldm_dit_workspace_bytes(const scldm_dit* h, int n_fwd, int n_rows, int n_state);

/* Conditioning rows: c = TimestepEmbedder(t) + sum_classes Embedding(label or null), then
 * SiLU(c) W_adaLN^T + b for every block and the final layer in one pass.
 * Replaces layers.py:351-364, nnets.py:283-288,380-456 and the nine adaln_modulation Linears
 * (layers.py:206,214-216,395,398).  t: device (n_rows) with t_stride 1, or one device float with
 * t_stride 0.  labels[c]: device (n_rows) int64, or NULL => class c uses its null token.
 * mod_out: device (n_rows, mod_width). */
int scldm_dit_cond_rows(scldm_dit* h, const float* t, int t_stride, const int64_t* const* labels, int n_rows,
                        float* mod_out, void* ws, void* stream);

/* DiT trunk on prepared conditioning: input_proj + pos_embed, n_layer fused blocks, final layer
 * (nnets.py:290-296).  Sample-forward s < n_direct reads latent x[s]; s >= n_direct re-reads the last
 * `rep` latents (x[n_direct - rep + (s - n_direct) % rep]) - the conditional CFG passes.
 * row_index[s] selects the conditioning row of `mod`.  out: device (n_fwd, S, Din). */
int scldm_dit_forward_rows(scldm_dit* h, const float* x, int n_direct, int rep, int n_fwd, const float* mod,
                           const int32_t* row_index, float* out, int precision, void* ws, void* stream);

/* DiT.forward in eval mode (nnets.py:273-297): x (n,S,Din), t (n), labels[c] (n) or NULL. */
int scldm_dit_forward(scldm_dit* h, const float* x, const float* t, const int64_t* const* labels, float* out, int n,
                      int precision, void* ws, void* stream);

/* DiT.forward_with_cfg (nnets.py:336-378) in one call.  x, out: (2B,S,Din).  t: (2B) with t_stride 1 or a
 * single device float with t_stride 0 (the ODE solver broadcasts one scalar, integrators.py:103-104).
 * The unconditional pass covers all 2B rows; conditional pass p re-runs the second half with the classes
 * in pass_mask[p] (bit c = class c keeps its labels, others null) and is blended with pass_scale[p]:
 *   joint:              n_pass = 1, mask = all classes, scale = mean(cfg_scale)        (:364-369)
 *   mutually_exclusive: one pass per cfg_scale entry, mask = that class, scale = its value (:372-376)
 * Conditional labels are given for n_urows UNIQUE label rows (ulabels[c]: device (n_urows) int64) and
 * cell_row (device (B) int32, or NULL when n_urows == B) maps each cell of the second half to its row.
 * With t_stride 1 the rows must be per-cell (n_urows == B, cell_row NULL).
 * t_stride 2: t is a dense (2B) vector whose uniformity is decided ON DEVICE (what torchdiffeq's `ones(B) * t` looks like
 * to a callee, integrators.py:103-104): a one-workgroup kernel compares the entries, the conditioning kernels of both plans
 * are enqueued and the ones of the plan that does not apply exit at once - no host synchronisation; the workspace must be
 * sized for the dense plan (n_rows = 2B + n_pass * B); de-duplicated label rows + cell_row are accepted. */
int scldm_dit_forward_cfg(scldm_dit* h, const float* x, const float* t, int t_stride, const int64_t* const* ulabels,
                          int n_urows, const int32_t* cell_row, int B, int n_pass, const uint32_t* pass_mask,
                          const float* pass_scale, float* out, int precision, void* ws, void* stream);

/* Fixed-grid ODE sampling of dz/dt = forward_with_cfg(z, t) from t=0 to 1 (transport.py:324-369,
 * integrators.py:100-112 with sampling_method euler|heun): t_i = i/n_steps, h = 1/n_steps;
 * euler: one evaluation per step; heun: two (k1 at t_i, k2 at t_i+h).  z (2B,S,Din) is updated in place
 * (first B rows unconditional, last B guided - models.py:801-812).  `n_steps` = reference num_steps - 1. */
int scldm_sample_ode(scldm_dit* h, float* z, const int64_t* const* ulabels, int n_urows, const int32_t* cell_row, int B,
                     int n_pass, const uint32_t* pass_mask, const float* pass_scale, int n_steps, int method,
                     int precision, void* ws, void* stream);

/* Fixed-grid SDE sampling: the stochastic face of the reference's Sampler (transport.py:269-322, integrators.py:7-75) for the Linear
 * path with a velocity model, as one call.  With v = forward_with_cfg(x, t): score = (t v - x) / (1 - t), SDE drift
 * f = v + D(t) score, and D(t) by diffusion_form (norm = diffusion_norm; path.py:52-77):
 *   SIGMA, LINEAR: norm (1 - t)   CONSTANT: norm   DECREASING: 0.25 (norm cos(pi t) + 1)^2   INC_DEC: norm sin^2(pi t)
 * Grid: t = linspace(0, t1, num_steps) in fp32, t1 = 1 - last_step_size (last_step NONE forces last_step_size 0), dt = t[1] - t[0];
 * steps run at t[0] .. t[num_steps - 2], each with ONE normal draw w of the state's shape:
 *   euler: x <- x + dt f(x, t) + sqrt(2 D dt) w
 *   heun:  xhat = x + sqrt(2 D(t) dt) w; K1 = f(xhat, t); K2 = f(xhat + dt K1, t + dt); x <- xhat + dt / 2 (K1 + K2)
 * then one more evaluation at t1 without noise - MEAN: x + last_step_size f(x, t1); TWEEDIE: x + (1 - t1) v (the reference's
 * x / t1 + (1 - t1)^2 / t1 score, simplified); EULER: x + last_step_size v; NONE: x unchanged, no evaluation.
 * num_steps - 1 (+ 1) evaluations for euler, 2 (num_steps - 1) (+ 1) for heun; every update is x' = a_x x + a_v v + a_w w with
 * host-side scalars and rides in the kernel that blends the CFG passes.
 * z (2B,S,Din) is updated in place (first B rows unconditional, last B guided; labels / passes as scldm_sample_ode, same workspace:
 * scldm_dit_workspace_bytes(h, 2B + n_pass B, 1 + n_pass n_urows, 2B)).
 * noise: NULL, or device (num_steps - 1, 2B, S*Din) normals used INSTEAD of the generator (step-major).
 * Generator: Philox4x32-10 keyed by `seed`; the value of an element depends on (seed, step, global row, column) only, where the
 *   global state is (2, cells_total, S*Din) and this call holds cells [cell_offset, cell_offset + B) of it: shards of one solve draw
 *   the noise the whole solve would have drawn.  The seed is a launch argument: a captured graph replays the SAME noise.
 * traj: NULL, or device (num_steps, 2B, S*Din) receiving every state the reference's list holds (num_steps - 1 step results, then
 *   the last-step result, which is also left in z).
 * SCLDM_ERR_SHAPE (nothing is launched) for the corners where the reference returns NaN under this transport - form SBDM (D is
 * infinite at t = 0), heun with last_step NONE (score at t = 1), MEAN / TWEEDIE with last_step_size 0 (score at t = 1) - and for
 * num_steps < 2, last_step_size outside [0, 1), cells_total < cell_offset + B, unknown method / form / last step. */
#define SCLDM_SDE_FORM_SIGMA 0
#define SCLDM_SDE_FORM_LINEAR 1
#define SCLDM_SDE_FORM_CONSTANT 2
#define SCLDM_SDE_FORM_DECREASING 3
#define SCLDM_SDE_FORM_INC_DEC 4   /* the reference spells it "inccreasing-decreasing" */
#define SCLDM_SDE_FORM_SBDM 5      /* the reference's default; rejected here (see above), served by scldm_sample_sde_transport */
#define SCLDM_SDE_LAST_NONE 0
#define SCLDM_SDE_LAST_MEAN 1
#define SCLDM_SDE_LAST_TWEEDIE 2
#define SCLDM_SDE_LAST_EULER 3
int scldm_sample_sde(scldm_dit* h, float* z, const int64_t* const* ulabels, int n_urows, const int32_t* cell_row, int B, int n_pass,
                     const uint32_t* pass_mask, const float* pass_scale, int num_steps, int method, int diffusion_form,
                     float diffusion_norm, int last_step, float last_step_size, const float* noise, unsigned long long seed,
                     long long cell_offset, long long cells_total, float* traj, int precision, void* ws, void* stream);

/* The normals scldm_sample_sde draws at `step` for rows [cell_offset, cell_offset + n_rows_local) of CFG half `half` (0: the
 * unconditional rows, 1: the guided rows) of a (2, cells_total, e) state.  out: device (n_rows_local, e), 16-byte aligned; e % 4 == 0. */
int scldm_sde_noise(float* out, long long n_rows_local, int e, unsigned long long seed, int step, int half, long long cell_offset,
                    long long cells_total, void* stream);

/* Adaptive Dormand-Prince 5(4) sampling: the reference's DEFAULT sampler (`sample_ode()` with no arguments -> torchdiffeq dopri5 at
 * atol = rtol = 1e-5: transport.py:324-331, integrators.py:100-112) over forward_with_cfg, as one call.  Semantics are those of
 * scldm_amd.transport.Sampler._sample_dopri5, decision for decision and bit for bit: FSAL tableau, ONE step size for the whole
 * (2B, S, Din) state, mixed rms error ratio, accept iff ratio <= 1, h *= 10 for ratio == 0 and otherwise
 * h *= min(10, max(0.9 / ratio^0.2, ratio < 1 ? 1 : 0.2)), steps never clipped to the save times, the quartic interpolant of the last
 * accepted step evaluated at the fp32 linspace(0, 1, num_save) save times.  Times and step sizes are host float64; a stage time is
 * rounded to fp32 once; a tableau weight is (float)(h * w) formed in double (structural zeros skipped); state arithmetic is fp32 with
 * every product and sum rounded on its own.
 * z (2B,S,Din): in, and out = the state at t = 1 (first B rows unconditional, last B guided); labels / passes as scldm_sample_ode.
 * first_step > 0: the first attempted step; <= 0: the automatic initial step (Hairer / Norsett / Wanner), which costs one more
 *   evaluation, f(t0 + h0, y0 + h0 f0), beside the f(t0, y0) every solve starts with.
 * traj: NULL, or device (num_save, 2B, S*Din) receiving every save point, traj[0] being the initial z.
 * stats (host, may be NULL) and step_log (host (step_log_cap, 3) doubles: t0, dt, accepted (1.0 / 0.0) of each attempted step in
 *   order, at most step_log_cap of them; may be NULL) describe the solve.
 * ws: scldm_sample_ode_dopri5_workspace_bytes(h, B, n_pass, n_urows) bytes, 256-byte aligned; it holds the slopes k1..k7, two state
 *   buffers and the four interpolation coefficients (an accepted step swaps pointers, nothing is copied) and the adaLN vectors of one
 *   step's six new evaluations (prepared in one batched pass per attempted step).
 * The call reads the error ratio once per attempted step: it synchronises `stream` that often and CANNOT be captured into a graph.
 * SCLDM_ERR_SHAPE with nothing launched: a handle outside the fused family (checked before any HIP call), num_save < 2, atol <= 0 or
 *   rtol < 0, B < 1, NULL z / ws, an unknown precision, a capturing stream.  SCLDM_ERR_STATE: weights not loaded.
 * SCLDM_ERR_SOLVER: the step size underflowed (t + h == t) or more than 100 000 evaluations were made; z, traj and stats hold what the
 *   solve had reached (stats->status says which). */
#define SCLDM_ERR_SOLVER (-4)
#define SCLDM_DOPRI5_OK 0
#define SCLDM_DOPRI5_UNDERFLOW 1
#define SCLDM_DOPRI5_MAX_EVALS 2
typedef struct {
  long long evaluations;   /* model evaluations (one CFG evaluation = one) */
  long long accepted, rejected;   /* attempted steps by outcome */
  double first_step;       /* the first attempted step size */
  int status;              /* SCLDM_DOPRI5_* */
  int step_log_len;        /* rows written to step_log */
} scldm_dopri5_stats;
size_t scldm_sample_ode_dopri5_workspace_bytes(const scldm_dit* h, int B, int n_pass, int n_urows);
int scldm_sample_ode_dopri5(scldm_dit* h, float* z, const int64_t* const* ulabels, int n_urows, const int32_t* cell_row, int B, int n_pass,
                            const uint32_t* pass_mask, const float* pass_scale, int num_save, double atol, double rtol, double first_step,
                            float* traj, scldm_dopri5_stats* stats, double* step_log, int step_log_cap, int precision, void* ws,
                            void* stream);
/* The same solve with the save times given: save_times is a HOST array of num_save non-decreasing fp32 times, the first 0.
 * scldm_sample_ode_dopri5 forms them itself as start + step * i below the middle and end - step * (n - 1 - i) from it on, in fp32 - the
 * element-wise definition of torch.linspace, which torch's vectorised CPU kernel does not reproduce to the last bit at every index; a
 * caller that wants the interpolant at exactly the values ITS linspace holds (scldm_amd does: the host-composed solver and the
 * reference take them from torch on the host) passes them here.  The steps never depend on the save times. */
int scldm_sample_ode_dopri5_at(scldm_dit* h, float* z, const int64_t* const* ulabels, int n_urows, const int32_t* cell_row, int B, int n_pass,
                               const uint32_t* pass_mask, const float* pass_scale, int num_save, const float* save_times, double atol,
                               double rtol, double first_step, float* traj, scldm_dopri5_stats* stats, double* step_log, int step_log_cap,
                               int precision, void* ws, void* stream);

/* The solve's controller, handle-free and without a HIP call (csrc/dopri5_ctl.hpp): what the host decides between the kernels.
 * scldm_dopri5_stage_plan: for an attempted step from t0 with size h - the fp32 times of the six new evaluations, the fp32 weights
 *   (float)(h * w) of the six stage points (a[i][j]: slope j in stage point i), of the error estimate and of the mid-point, with a mask
 *   bit per weight that is NOT a structural zero of the tableau, and (float)h, (float)(2h) for the interpolant.
 * scldm_dopri5_control: after that step, given its error ratio - accepted or not, where the next step starts (t1), its size, and
 *   whether that next step underflows (t1 + h_next == t1).
 * scldm_dopri5_initial_h0 / _initial_step: the automatic first step from d0 = rms(y0 / scale), d1 = rms(f0 / scale) (the trial step
 *   h0), then from d2 = rms((f(t0 + h0, y0 + h0 f0) - f0) / scale) / h0; scale = atol + rtol |y0|. */
typedef struct {
  float t_stage[6];
  float a[6][7];
  float err[7], mid[7];
  unsigned a_mask[6], err_mask, mid_mask;
  float h, two_h;
} scldm_dopri5_plan;
typedef struct {
  int accepted, underflow;
  double t1, h_next;
} scldm_dopri5_control_out;
void scldm_dopri5_stage_plan(double t0, double h, scldm_dopri5_plan* out);
void scldm_dopri5_control(double t0, double h, double ratio, scldm_dopri5_control_out* out);
double scldm_dopri5_initial_h0(double d0, double d1);
double scldm_dopri5_initial_step(double h0, double d1, double d2);

/* Options of a handle (read by the calls that follow).
 * SCLDM_OPT_CFG1_DIRECT (default 0): with ONE conditional pass of guidance scale exactly 1.0 and a scalar t (scldm_sample_ode,
 *   scldm_dit_forward_cfg with t_stride 0), DiT.forward_with_cfg's guided half u2 + 1.0 * (c2 - u2) (nnets.py:368,376) is c2 up to
 *   one fp32 rounding of that expression: the unconditional forward over the second half is not run (2B sample-forwards per
 *   evaluation instead of 3B) and the conditional output is returned as the guided rows.  Off: the reference's arithmetic, term by
 *   term.  The reference's own configs use guidance 1.0 for dentate_gyrus / parse1m (datamodule/default.yaml:46-47). */
#define SCLDM_OPT_CFG1_DIRECT 1
/* SCLDM_OPT_TAIL_SPLIT (default 0; bf16 / fp16 policies): the tiles of a trunk launch's partial last round that would run beside an
 * empty workgroup slot are launched as 32-token tiles (two per 64-token tile) next to the 64-token launch.  Results are bit-identical
 * either way (tested); measured 2-12 % SLOWER (a 32-token tile streams twice the weight bytes per token), so it stays an A/B knob. */
#define SCLDM_OPT_TAIL_SPLIT 2
int scldm_dit_set_option(scldm_dit* h, int option, int value);

/* DiT layers one fused-kernel launch runs (8 by default, SCLDM_LPL=1..8: the residual stays in registers between them; 0 for a
 * handle outside the fused shape family).  bench.py uses it to state the algorithmic FLOPs of a launch. */
int scldm_dit_layers_per_launch(const scldm_dit* h);

/* Measurement aid (bench.py): TFLOP/s a register-only v_mfma_f32_32x32x16_bf16 loop sustains on the current device for about
 * `iters` x 5 x 16 MFMAs per wave (fill 0: zero operands, 1: uniform [-1, 1), 2: N(0, 1); fill | 4: the same loop and values on
 * v_mfma_f32_32x32x16_f16 - the ceiling of the fp16 policy); same instruction stream for every fill -
 * the part clocks to its power budget, so the figure for realistic operands is the ceiling an MFMA-bound kernel can reach on this
 * device, below the nominal 2.5 PFLOP/s.  Synchronises the device. */
int scldm_mfma_sustained_tflops(int fill, int iters, double* tflops);

/* Timing hook for bench.py: when enabled, every fused-block launch is bracketed by HIP events on its
 * own stream; scldm_dit_block_timing drains them (synchronises) and returns launches and total ms. */
void scldm_dit_block_timing_enable(scldm_dit* h, int enable);
int scldm_dit_block_timing(scldm_dit* h, int* n_launches, double* total_ms);

/* ------------------------------------------------------------------------------------------------
 * Training path: DiT.forward with saved activations and its backward,
 * GEMMs on MFMA with fp32 (exact, parity) or bf16 operands (SCLDM_PREC_*; fp32 accumulation, fp32 activations,
 * LayerNorm / softmax / SiLU / residual in fp32 either way, as bf16-mixed autocast would keep them; the reference's
 * trainer default is `precision: 32`, experiments/configs/training/default.yaml:6).  The reference differentiates DiT.forward (nnets.py:273-297) with torch autograd
 * inside Transport.training_losses (transport/transport.py:110-150); these two calls are the pair a
 * torch.autograd.Function binds (scldm_amd/nnets.py).  Weights are read LIVE from the caller's parameter
 * tensors (no packing, nothing to refresh after an optimiser step).  Labels are the ones the model sees:
 * training-mode label dropout (nnets.py:300-334) is applied by the caller by substituting null tokens.
 * ------------------------------------------------------------------------------------------------ */
/* Writable mirror of scldm_dit_weights: every pointer receives d loss / d parameter in the parameter's own
 * PyTorch layout (overwritten, not accumulated).  pos_embed may be NULL (frozen in the reference, nnets.py:248). */
typedef struct {
  float* pos_embed;
  float* t_w0; float* t_b0;
  float* t_w2; float* t_b2;
  float* in_w; float* in_b;
  float* fin_w; float* fin_b;
  float* fin_ada_w; float* fin_ada_b;
  float* const* class_emb;
  float* const* attn_w; float* const* attn_b;
  float* const* proj_w; float* const* proj_b;
  float* const* w1; float* const* w2;
  float* const* cproj;
  float* const* ada_w; float* const* ada_b;
} scldm_dit_grads;

/* Bytes of the activation record written by train_forward and read by train_backward for n samples. */
size_t scldm_dit_train_saved_bytes(const scldm_dit* h, int n);
/* Scratch bytes for either call (gradient temporaries, split-K partials). */
size_t scldm_dit_train_workspace_bytes(const scldm_dit* h, int n);
/* The same for a known precision: the fused bf16 route of the base shape keeps 32 KB per cell per layer (layer inputs + the two
 * gated branch outputs) instead of the generic route's 295 KB, and needs none of its per-token gradient temporaries; buffers
 * sized by the two functions above (precision unknown: the larger, generic layout) are accepted by every route. */
size_t scldm_dit_train_saved_bytes_for(const scldm_dit* h, int n, int precision);
size_t scldm_dit_train_workspace_bytes_for(const scldm_dit* h, int n, int precision);

/* One-time set-up for training on the parameter tensors `w` at batch size n and `precision`: everything the two calls below
 * would otherwise create on first use - the bf16 weight mirror of the bf16-source route (DiT-L: 0.9 GB) with its cast-job
 * table, or the fused route's pack-job tables, side streams and events.  May allocate and synchronise `stream`; after it,
 * train_forward / train_backward on the same parameter pointers issue kernel launches and event records only.  Optional: a
 * forward on parameters it was not prepared for prepares itself (scldm_amd.nnets calls this whenever the parameters' storage
 * moved).  SCLDM_PREC_BF16X3 is accepted on the training entry points and served by the exact-fp32 GEMM route. */
int scldm_dit_train_prepare(scldm_dit* h, const scldm_dit_weights* w, int n, int precision, void* stream);

/* Gradient-ready events for the NEXT scldm_dit_train_backward on this handle - what a data-parallel caller needs to start
 * all-reducing a bucket of gradients while the rest of the backward still runs (the reference gets this from DDP's autograd
 * hooks, experiments/scripts/train_ldm.py:101).  events[i] is a hipEvent_t the call records on its stream once the gradients it
 * stands for are complete:
 *   SCLDM_GRAD_LAYER, l : attn / proj / w1 / w2 / cproj gradients (weights and biases) of every layer >= l
 *   SCLDM_GRAD_ADA,   l : adaLN weight / bias gradients of every layer <= l (l == n_layer: the final layer's adaLN as well)
 *   SCLDM_GRAD_END      : every gradient
 * The backward walks the layers from last to first and computes the adaLN gradients afterwards, first layer first.  Routes that
 * produce everything at once (the fused base-shape route) record all events at the end.  The list is consumed by that call. */
#define SCLDM_GRAD_LAYER 0
#define SCLDM_GRAD_ADA 1
#define SCLDM_GRAD_END 2
int scldm_dit_train_set_grad_events(scldm_dit* h, void* const* events, const int* kinds, const int* layers, int n);

/* out (n,S,Din) = DiT.forward(x (n,S,Din), t (n), labels) keeping every intermediate the backward needs in `saved`. */
int scldm_dit_train_forward(scldm_dit* h, const scldm_dit_weights* w, const float* x, const float* t,
                            const int64_t* const* labels, int n, float* out, int precision, void* saved, void* ws,
                            void* stream);

/* Given dout = d loss / d out (n,S,Din): all parameter gradients into `grads`, and d loss / d x into dx (n,S,Din)
 * unless dx is NULL.  x, labels and `saved` must be those of the matching train_forward call. */
int scldm_dit_train_backward(scldm_dit* h, const scldm_dit_weights* w, const scldm_dit_grads* grads, const float* x,
                             const int64_t* const* labels, const float* dout, int n, float* dx, int precision, void* saved,
                             void* ws, void* stream);

/* The input-gradient-only backward: d loss / d x into dx (n,S,Din, required) against the record of the matching train_forward call,
 * and nothing else - the contract of scldm_dit_train_backward minus `grads`.  No weight-gradient GEMM, no bias / adaLN / embedding /
 * timestep-MLP gradient is formed (fused base-shape route: a second family of the backward layer kernel that writes d x only; generic
 * route: the parameter-gradient launches are skipped).  dx has the bits of scldm_dit_train_backward's dx on the same record.  What a
 * log-likelihood evaluation or an input VJP needs.  fp16: loss-scaled like the training backward (the handle's scale state advances).
 * Its workspace is smaller on the fused route (no operand-pair or partial buffers); a buffer of that size also serves the
 * train_forward call that writes the record. */
size_t scldm_dit_train_workspace_bytes_dx_for(const scldm_dit* h, int n, int precision);
int scldm_dit_train_backward_dx(scldm_dit* h, const scldm_dit_weights* w, const float* x, const int64_t* const* labels,
                                const float* dout, int n, float* dx, int precision, void* saved, void* ws, void* stream);

/* Record-free inference and sampling of the shapes outside the fused family (handles the fused entry points refuse: n_embed % 256 == 0,
 * seq_len 16, head_dim 32 or 64, e.g. a 1 024-wide DiT-L): conditioning rows -> trunk over a row index -> CFG blend + state update, the
 * three layers of scldm_dit_cond_rows / scldm_dit_forward_rows / scldm_dit_forward_cfg / scldm_sample_ode over the kernels of
 * scldm_dit_train_forward.  They read the live parameters `w` like the training entry points (nothing is loaded into the handle),
 * take the precisions scldm_dit_train_forward takes on such a handle (fp32, bf16; bf16x3 / fp16 are served by the fp32 route) and keep
 * no activation record: the workspace holds ONE layer's arrays, n_rows conditioning rows and the split-K partials, whatever n_layer is.
 * The bf16 policy's weight mirror (allocated inside the handle on first use) is refreshed from `w` once per call, not once per
 * evaluation; apart from that mirror no call allocates.  n_direct, rep, row_index, ulabels, n_urows, cell_row, pass_mask, pass_scale,
 * n_steps and method mean what their fused namesakes document above.  A fused-family handle, a rejected argument (n_steps < 1, an
 * unknown method or t_stride, a NULL pointer, a class without its null row): SCLDM_ERR_SHAPE with a message, nothing launched.
 *
 * Bits: with one conditioning row per sample-forward (row_index NULL = identity) and the same n, scldm_dit_infer_cond_rows(t_stride 1)
 * + scldm_dit_infer_forward_rows return what scldm_dit_train_forward returns (same kernels, operands and split-K choices).
 *
 * scldm_dit_infer_workspace_bytes(h, n_fwd, n_rows, n_state, precision): bytes for calls over up to n_fwd sample-forwards, n_rows
 *   conditioning rows and an ODE state of n_state samples.  n_fwd == 0 sizes scldm_dit_infer_cond_rows alone (it writes to mod_out).
 * scldm_dit_infer_cond_rows: t (n_rows) with t_stride 1, or one device float with t_stride 0 (its timestep embedding is formed once
 *   and shared by the rows); labels[c] (n_rows) int64 or NULL = the null token; mod_out (n_rows, mod_width).
 * scldm_dit_infer_forward_rows: x (n_direct, S, Din); sample-forwards beyond n_direct re-read the last `rep` latents;
 *   mod (rows, mod_width); row_index (n_fwd) int32 or NULL = sample-forward s reads row s; out (n_fwd, S, Din).
 * scldm_dit_infer_forward_cfg: scldm_dit_forward_cfg with t_stride 0 (one device float) or 1 (t (2B), per-cell label rows).
 * scldm_dit_infer_sample_ode: scldm_sample_ode; z (2B, S, Din) is updated in place. */
size_t scldm_dit_infer_workspace_bytes(const scldm_dit* h, int n_fwd, int n_rows, int n_state, int precision);
int scldm_dit_infer_cond_rows(scldm_dit* h, const scldm_dit_weights* w, const float* t, int t_stride, const int64_t* const* labels,
                              int n_rows, float* mod_out, int precision, void* ws, void* stream);
int scldm_dit_infer_forward_rows(scldm_dit* h, const scldm_dit_weights* w, const float* x, int n_direct, int rep, int n_fwd,
                                 const float* mod, const int32_t* row_index, float* out, int precision, void* ws, void* stream);
int scldm_dit_infer_forward_cfg(scldm_dit* h, const scldm_dit_weights* w, const float* x, const float* t, int t_stride,
                                const int64_t* const* ulabels, int n_urows, const int32_t* cell_row, int B, int n_pass,
                                const uint32_t* pass_mask, const float* pass_scale, float* out, int precision, void* ws, void* stream);
int scldm_dit_infer_sample_ode(scldm_dit* h, const scldm_dit_weights* w, float* z, const int64_t* const* ulabels, int n_urows,
                               const int32_t* cell_row, int B, int n_pass, const uint32_t* pass_mask, const float* pass_scale,
                               int n_steps, int method, int precision, void* ws, void* stream);

/* Exact log-likelihood of latents under the probability flow (Sampler.sample_ode_likelihood, src/scldm/transport/transport.py:371-430)
 * over forward_with_cfg, as launches only (no host read).  Capture: with SCLDM_PREC_FP32 / _BF16X3 everything runs on `stream` and
 * the call can be captured as it is; with bf16 / fp16 operands on the fused base shape every evaluation's scldm_dit_train_forward forks
 * its weight re-pack onto a side stream, so a captured graph has parallel branches.  fp16: each evaluation's backward runs under the
 * handle's training loss scale and advances that state; an overflow there is not retried - check logp for non-finite values.  Solver time s runs 0 -> 1 on the grid
 * s_i = i / n_steps (euler: one evaluation per step; heun: two, the second at s_{i+1}); the model is evaluated at t = 1 - s, the
 * state moves by -v and delta_logp accumulates logp_grad = eps . (dv/dx)^T eps with one fresh Rademacher probe eps per evaluation
 * (Hutchinson; the VJP is scldm_dit_train_backward_dx over the 2B + n_pass * B rows of the evaluation).
 *   z (2B,S,Din): in - the doubled state cat([x, x]) (first B rows: unconditional field, last B: guided field); out - the noise-end
 *       latents.  Labels / passes as scldm_sample_ode.  16-byte aligned.
 *   logp (2B): prior_logp(z_end) - delta_logp, prior_logp(z) = -S Din / 2 log 2 pi - sum z^2 / 2.
 *   probe: NULL (the generator: Philox keyed by (seed, evaluation, half, global cell, column), so a shard [cell_offset,
 *       cell_offset + B) of cells_total cells draws what the whole solve would), or (n_evaluations, 2B, S Din) values used instead.
 *   dlogp_traj: NULL, or (n_evaluations, 2B) receiving every logp_grad.
 *   saved: scldm_dit_train_saved_bytes_for(h, (2 + n_pass) B, precision) bytes; ws: scldm_logp_workspace_bytes bytes.
 * SCLDM_ERR_SHAPE with nothing launched for n_steps < 1, an unknown method, cells_total < cell_offset + B. */
size_t scldm_logp_workspace_bytes(const scldm_dit* h, int B, int n_pass, int precision);
int scldm_logp_ode(scldm_dit* h, const scldm_dit_weights* w, float* z, const int64_t* const* ulabels, int n_urows,
                   const int32_t* cell_row, int B, int n_pass, const uint32_t* pass_mask, const float* pass_scale, int n_steps, int method,
                   const float* probe, unsigned long long seed, long long cell_offset, long long cells_total, float* logp,
                   float* dlogp_traj, int precision, void* saved, void* ws, void* stream);
/* The probe scldm_logp_ode draws at `evaluation` for rows [cell_offset, cell_offset + n_rows_local) of CFG half `half` of a
 * (2, cells_total, e) state: values in {-1, +1}.  out: device (n_rows_local, e), 16-byte aligned; e % 4 == 0. */
int scldm_logp_probe(float* out, long long n_rows_local, int e, unsigned long long seed, int evaluation, int half, long long cell_offset,
                     long long cells_total, void* stream);
/* The same likelihood with the reference's default solver (Sampler.sample_ode_likelihood(sampling_method="dopri5", atol=1e-6,
 * rtol=1e-3)): adaptive Dormand-Prince 5(4) over the augmented state (x (2B, S Din), delta_logp (2B)) with the slopes (-v, logp_grad)
 * of scldm_logp_ode's evaluation, as one call on a handle of the fused shape family.  The controller is the one of
 * scldm_sample_ode_dopri5 (scldm_dopri5_stage_plan / _control / _initial_h0 / _initial_step): FSAL, one host read of the error ratio
 * per attempted step, steps never clipped to s = 1 (the solver steps past it: the model is then evaluated at slightly negative t), the
 * result is the quartic interpolant of the accepted step that contains s = 1, and logp = prior_logp(x_end) - delta_logp.
 * Error norm: ONE mixed rms norm over all 2B (S Din + 1) components with one atol / rtol (the packed state of
 * Sampler.sample_ode_likelihood): ratio = sqrt(mean((err / (atol + rtol max(|y0|, |y1|)))^2)); the automatic first step (first_step <= 0)
 * uses the same norm.  All cells of a call share the step size, so a shard of a solve does NOT reproduce the whole solve's rows.
 * Probes: evaluation index = the running count in execution order (f0 is 0, the initial-step probe evaluation 1 - absent when
 * first_step is given -, then six per attempted step, rejected steps included).  probe_per_solve != 0 holds ONE probe for the whole
 * solve (the usual FFJORD form): index 0 of the generator, or the given `probe` (2B, S Din); a given probe with probe_per_solve == 0 is
 * refused (the number of evaluations is not known ahead).
 *   z, labels / passes, seed / cell_offset / cells_total, logp, saved: as scldm_logp_ode.  dlogp_out: NULL or (2B) delta_logp at s = 1.
 *   stats: as scldm_sample_ode_dopri5.  step_log: NULL or step_log_cap x FOUR doubles per attempted step: t0, h, accepted (1.0 / 0.0),
 *       the error ratio the controller was given.
 *   ws: scldm_logp_ode_dopri5_workspace_bytes bytes (0 for a NULL handle, a handle outside the fused family or a bad argument), 256-byte
 *       aligned.
 * SCLDM_ERR_SHAPE with nothing launched (checked before any HIP call): a NULL pointer, atol <= 0 or rtol < 0, B < 1, cells_total <
 *   cell_offset + B, a probe without probe_per_solve, misaligned z / probe / ws, a handle outside the fused family; and a capturing
 *   stream.  SCLDM_ERR_STATE: a handle without its read-back slot.  SCLDM_ERR_SOLVER: step-size underflow or more than 100 000
 *   evaluations; z then holds the state reached and stats->status says which. */
size_t scldm_logp_ode_dopri5_workspace_bytes(const scldm_dit* h, int B, int n_pass, int precision);
int scldm_logp_ode_dopri5(scldm_dit* h, const scldm_dit_weights* w, float* z, const int64_t* const* ulabels, int n_urows,
                          const int32_t* cell_row, int B, int n_pass, const uint32_t* pass_mask, const float* pass_scale, double atol,
                          double rtol, double first_step, const float* probe, int probe_per_solve, unsigned long long seed,
                          long long cell_offset, long long cells_total, float* logp_out, float* dlogp_out, scldm_dopri5_stats* stats,
                          double* step_log, int step_log_cap, int precision, void* saved, void* ws, void* stream);

/* Flow-matching training step around the model call (Transport.training_losses, src/scldm/transport/transport.py:110-150 with
 * ICPlan.plan, path.py:148-151): the eager reference spends ~20 elementwise launches here per step.
 *   scldm_fm_mix:      xt = t*x1 + (1-t)*x0 (each product and the sum rounded separately, as eager torch does), ut = x1 - x0;
 *                      x1, x0, xt, ut are (n, e) fp32, t is (n).
 *   scldm_fm_loss:     loss[b] = mean_e (pred - ut)^2                              (mean_flat, utils.py:15-17)
 *   scldm_fm_loss_bwd: dpred[b][:] = gloss[b] * 2/e * (pred - ut)                  (its gradient w.r.t. pred) */
int scldm_fm_mix(const float* x1, const float* x0, const float* t, float* xt, float* ut, int n, int e, void* stream);

/* The same pieces with nothing left to the host (csrc/train_step.hip; round 6):
 *   scldm_fm_prepare   - Transport.sample + ICPlan.plan + the label dropout of DiT.forward in ONE kernel (transport.py:97-108,
 *                        path.py:148-151, nnets.py:395-402,440-452): t ~ U[0,1) and a drop decision per row, x0 ~ N(0, I), xt, ut,
 *                        and labels_out (n_classes, n) = what the model sees (null token where dropped; mutually_exclusive: ONE class
 *                        drawn per call among the non-NULL labels_in, every other class all-null - the reference draws it on the
 *                        host, nnets.py:395).  Draws come from Philox4x32-10 keyed by rng_state[0] (seed) at step rng_state[1]
 *                        (device memory, read only): reproducible, independent of the launch geometry.  x0 may be NULL.
 *   scldm_fm_loss_grad - loss_rows[b] = mean_e (pred - ut)^2, loss_mean = mean_b, dpred = d loss_mean / d pred, ONE kernel
 *                        (fixed-order sums); advances rng_state[1] when rng_state is given.  ticket: a zero-initialised device word.
 * Captured in a HIP graph both follow the device-side step counter: every replay draws a fresh batch. */
int scldm_fm_prepare(const float* x1, const int64_t* const* labels_in, const int* null_tokens, int n_classes, int strategy /* 0 mutually_exclusive, 1 joint */,
                     int drop, float p_drop, const unsigned long long* rng_state, int n, int e, float* t, float* x0, float* xt, float* ut,
                     int64_t* labels_out, void* stream);
int scldm_fm_loss_grad(const float* pred, const float* ut, int n, int e, float* loss_rows, float* loss_mean, float* dpred, unsigned int* ticket,
                       unsigned long long* rng_state, void* stream);

/* One optimisation step of LatentDiffusion.training_step on a batch of latents (src/scldm/models.py:628-663 + Lightning's backward
 * and optimizer.step(), + the EMA hook when `opt` carries one): scldm_fm_prepare -> scldm_dit_train_forward -> scldm_fm_loss_grad ->
 * scldm_dit_train_backward (every gradient into `grads`) -> scldm_adamw_table_step (skipped when opt is NULL: a data-parallel caller
 * reduces `grads` first).  Kernel launches and event records only; every per-step decision is read from device memory.  Buffers are
 * the caller's: */
typedef struct {
  int row_elems;            /* seq_len * n_embed_input */
  float* t;                 /* (n) */
  float* x0;                /* (n, row_elems) or NULL */
  float* xt; float* ut; float* pred; float* dpred;   /* (n, row_elems) */
  int64_t* labels;          /* (n_classes, n) */
  float* loss_rows;         /* (n) */
  float* loss_mean;         /* (1): the step's loss */
  unsigned int* ticket;     /* zero-initialised word */
  void* saved; void* ws;    /* scldm_dit_train_saved_bytes_for / _workspace_bytes_for */
} scldm_train_step_buffers;
int scldm_dit_train_step(scldm_dit* h, const scldm_dit_weights* w, const scldm_dit_grads* grads, const float* x1,
                         const int64_t* const* labels_in, const int* null_tokens, int n_classes, int strategy, float p_drop,
                         unsigned long long* rng_state, int n, int precision, const scldm_train_step_buffers* buffers,
                         const scldm_adamw_launch* opt /* may be NULL */, void* stream);
int scldm_fm_loss(const float* pred, const float* ut, float* loss, int n, int e, void* stream);
int scldm_fm_loss_bwd(const float* pred, const float* ut, const float* gloss, float* dpred, int n, int e, void* stream);

/* The rest of the reference's transport family (src/scldm/transport/path.py:24-151,190-208; transport.py:69-202): the GVP path, noise
 * and score prediction, the three loss weights.  With alpha, alpha', sigma, sigma' the path coefficients and their derivatives at t
 * (Linear: t, 1, 1 - t, -1; GVP: sin(pi t/2), pi/2 cos(pi t/2), cos(pi t/2), -pi/2 sin(pi t/2)) and
 * Dv = (alpha'/alpha) sigma^2 - sigma sigma':
 *   plan       xt = alpha x1 + sigma x0,  ut = alpha' x1 + sigma' x0
 *   loss row   w mean((c m - tgt)^2),  (c, tgt) = (1, ut) velocity | (1, x0) noise | (sigma, -x0) score,
 *              w = 1 | (Dv/sigma)^2 | Dv/sigma^2 for the weights none | velocity | likelihood (a velocity model ignores the weight)
 *   drift      f = a x + b m,  (a, b) = (0, 1) velocity | (alpha'/alpha, Dv) score | (alpha'/alpha, -Dv/sigma) noise
 *   interval   a velocity model trains and integrates over [0, 1]; noise / score models over [eps, 1 - eps] (train_eps, sample_eps).
 * The VP path is not provided.  Every entry below returns SCLDM_ERR_SHAPE for an unknown enum, VP, a negative eps or an eps >= 0.5. */
enum { SCLDM_PATH_LINEAR = 0, SCLDM_PATH_GVP = 1 };
enum { SCLDM_MODEL_VELOCITY = 0, SCLDM_MODEL_NOISE = 1, SCLDM_MODEL_SCORE = 2 };
enum { SCLDM_WEIGHT_NONE = 0, SCLDM_WEIGHT_VELOCITY = 1, SCLDM_WEIGHT_LIKELIHOOD = 2 };
typedef struct { int path, model, weight; float train_eps, sample_eps; } scldm_transport;
typedef struct { double alpha, d_alpha, sigma, d_sigma, ratio /* alpha'/alpha */, dv, a, b, c, w; } scldm_transport_coef;
/* The coefficients at one t, in double: no handle, no device.  A field the formula makes infinite at an end point (ratio at t = 0)
 * is returned as it comes; a velocity model gets (a, b, c, w) = (0, 1, 1, 1) without reading one. */
int scldm_transport_coef_at(const scldm_transport* tr, double t, scldm_transport_coef* out);
/* scldm_sample_ode for a noise / score model: fixed-grid Euler / Heun of the probability-flow drift f = a(t) x + b(t) m over the fp32
 * linspace(sample_eps, 1 - sample_eps, n_steps + 1), m the CFG-blended model output; arguments, workspace and precision as
 * scldm_sample_ode.  Per evaluation one elementwise kernel after the trunk blends, forms f and (Euler) steps the state; (a, b) are
 * evaluated in double at the fp32 grid time and rounded once.  A velocity model (either path) is handed to scldm_sample_ode.
 * SCLDM_ERR_SHAPE also for a noise / score transport with sample_eps == 0 (the drift is singular at the end points). */
int scldm_sample_ode_transport(scldm_dit* h, float* z, const int64_t* const* ulabels, int n_urows, const int32_t* cell_row, int B, int n_pass,
                               const uint32_t* pass_mask, const float* pass_scale, int n_steps, int method, const scldm_transport* tr,
                               int precision, void* ws, void* stream);
/* The SDE sampler and the likelihood under any transport above (scldm_sample_sde / scldm_logp_ode serve the default one: Linear path,
 * velocity model).  With m the CFG-blended model output at state x and model time t, rr = alpha / alpha' (0 at t = 0):
 *   drift      f_ode = a x + b m                                  (a, b) as scldm_transport_coef_at returns them
 *   score      s = s_x x + s_m m,  (s_x, s_m) = (-1/var, rr/var) velocity, var = sigma^2 - rr sigma' sigma | (0, 1) score | (0, -1/sigma) noise
 *   diffusion  D(t): SBDM norm Dv | SIGMA norm sigma (path-dependent) | LINEAR, CONSTANT, DECREASING, INC_DEC as scldm_sample_sde
 *   SDE drift  f = f_ode + D s = c_x x + c_m m
 * so every update of a solve is one affine map x' = a_x x + a_m m + a_w w: an Euler-Maruyama step (1 + dt c_x, dt c_m, sqrt(2 D dt)),
 * Heun's K1 / K2 (c_x, c_m, 0) and the last step at t1 - MEAN (1 + lss c_x, lss c_m), EULER (1 + lss a, lss b), TWEEDIE
 * (1/alpha + sigma^2/alpha s_x, sigma^2/alpha s_m).  All scalars are formed on the host in double from the fp32 time the model sees and
 * rounded to fp32 once, where they enter a kernel argument.
 * Grid: linspace(t0, t1, num_steps) in fp32, dt = t[1] - t[0], Heun's second evaluation at fp32 t + dt; a velocity model gets
 * (t0, t1) = (0, 1 - lss), a noise / score model (sample_eps, lss == 0 ? 1 - sample_eps : 1 - lss)  (lss = last_step_size).
 * Refusal rule: before the first launch every scalar of every update of the solve is formed; if one is not finite (as a double or once
 * rounded to fp32) the call returns SCLDM_ERR_SHAPE and the message names the evaluation index and its time.  This refuses SBDM for a
 * velocity model (Dv(0) is infinite on both paths), MEAN / TWEEDIE at t1 = 1 for a velocity model and a noise / score transport with
 * sample_eps == 0; it admits Heun with last_step NONE for a noise / score model with sample_eps > 0.
 *   scldm_sample_sde_transport: the arguments of scldm_sample_sde, then the transport.  The launches per evaluation are those of
 *       scldm_sample_sde.  The default transport is handed to scldm_sample_sde, with that entry's own refusals; GVP + velocity is not the
 *       default (its score conversion differs).
 *   scldm_logp_ode_transport / scldm_logp_transport_workspace_bytes: the arguments of scldm_logp_ode / scldm_logp_workspace_bytes, then
 *       the transport.  Solver time s runs over the fp32 linspace(t0, t1, n_steps + 1), (t0, t1) = (0, 1) for a velocity model and
 *       (sample_eps, 1 - sample_eps) otherwise; the model sees t = fp32(1 - s); the state moves by -(a x + b m) with (a, b) at t and
 *       logp_grad = a e + b (eps . (dm/dx)^T eps), formed as (float)(a e) + b * dot (e = S Din; eps . eps = e exactly for a Rademacher
 *       probe).  Probes, shards, Heun's form and the prior as scldm_logp_ode; the default transport is handed to scldm_logp_ode.
 *       Refused: a noise / score transport with sample_eps == 0 (as scldm_sample_ode_transport), and a solve with a non-finite (a, b, a e).
 *   scldm_sde_coef_at: out[4] = {D, c_x, c_m, sqrt(2 D dt)} at t;  scldm_sde_last_coef_at: out[2] = {a_x, a_m} of the last step at t1
 *       (last_step MEAN | TWEEDIE | EULER).  Host only, in double: no handle, no device; non-finite values are returned as they come.
 * SCLDM_ERR_SHAPE with nothing launched also for a bad transport, an unknown form / last step / method and a null pointer. */
int scldm_sde_coef_at(const scldm_transport* tr, int diffusion_form, double diffusion_norm, double t, double dt, double* out);
int scldm_sde_last_coef_at(const scldm_transport* tr, int diffusion_form, double diffusion_norm, int last_step, double last_step_size, double t1,
                           double* out);
int scldm_sample_sde_transport(scldm_dit* h, float* z, const int64_t* const* ulabels, int n_urows, const int32_t* cell_row, int B, int n_pass,
                               const uint32_t* pass_mask, const float* pass_scale, int num_steps, int method, int diffusion_form,
                               float diffusion_norm, int last_step, float last_step_size, const float* noise, unsigned long long seed,
                               long long cell_offset, long long cells_total, float* traj, int precision, void* ws, void* stream,
                               const scldm_transport* tr);
size_t scldm_logp_transport_workspace_bytes(const scldm_dit* h, int B, int n_pass, int precision, const scldm_transport* tr);
int scldm_logp_ode_transport(scldm_dit* h, const scldm_dit_weights* w, float* z, const int64_t* const* ulabels, int n_urows,
                             const int32_t* cell_row, int B, int n_pass, const uint32_t* pass_mask, const float* pass_scale, int n_steps,
                             int method, const float* probe, unsigned long long seed, long long cell_offset, long long cells_total,
                             float* logp, float* dlogp_traj, int precision, void* saved, void* ws, void* stream, const scldm_transport* tr);
/* Training around the model call, unfused (the generalisation of scldm_fm_mix / scldm_fm_loss / scldm_fm_loss_bwd):
 *   scldm_fm_plan:      one launch writes xt, the loss target tgt (ut | x0 | -x0) and rowc[b] = {c, w} (n, 2); each product is rounded
 *                       on its own, then the sum, like the eager form.  x1, x0, xt, tgt are (n, e) fp32, t is (n).
 *   scldm_fm_wloss:     loss[b] = w mean_e (c m - tgt)^2, summed in scldm_fm_loss's order
 *   scldm_fm_wloss_bwd: dm[b][:] = gloss[b] w (2/e) c (c m - tgt) */
int scldm_fm_plan(const scldm_transport* tr, const float* x1, const float* x0, const float* t, float* xt, float* tgt, float* rowc, int n,
                  int e, void* stream);
int scldm_fm_wloss(const float* m, const float* tgt, const float* rowc, float* loss, int n, int e, void* stream);
int scldm_fm_wloss_bwd(const float* m, const float* tgt, const float* rowc, const float* gloss, float* dm, int n, int e, void* stream);
/* The same with nothing left to the host (see scldm_fm_prepare / scldm_fm_loss_grad): the same Philox calls and counters, the row's
 * uniform u mapped to t = u (t1 - t0) + t0 (t1 = 1 - train_eps, t0 = train_eps, the span and t0 rounded to fp32 on the host, product
 * and sum rounded separately); tgt goes where scldm_fm_prepare writes ut, rowc is (n, 2). */
int scldm_fm_prepare_transport(const scldm_transport* tr, const float* x1, const int64_t* const* labels_in, const int* null_tokens,
                               int n_classes, int strategy, int drop, float p_drop, const unsigned long long* rng_state, int n, int e,
                               float* t, float* x0, float* xt, float* tgt, float* rowc, int64_t* labels_out, void* stream);
int scldm_fm_wloss_grad(const float* m, const float* tgt, const float* rowc, int n, int e, float* loss_rows, float* loss_mean, float* dm,
                        unsigned int* ticket, unsigned long long* rng_state, void* stream);
/* scldm_dit_train_step under a transport: the two entries above around the same forward / backward / AdamW calls; buffers->ut holds
 * tgt.  Launches and event records only, capturable like scldm_dit_train_step. */
int scldm_dit_train_step_transport(scldm_dit* h, const scldm_dit_weights* w, const scldm_dit_grads* grads, const float* x1,
                                   const int64_t* const* labels_in, const int* null_tokens, int n_classes, int strategy, float p_drop,
                                   unsigned long long* rng_state, int n, int precision, const scldm_train_step_buffers* buffers,
                                   const scldm_transport* tr, float* rowc, const scldm_adamw_launch* opt /* may be NULL */, void* stream);

/* ------------------------------------------------------------------------------------------------
 * TransformerVAE encode / decode (MCAB pooling / unpooling + negative-binomial head), fp32.
 * Shape family of the reference (experiments/configs/model/vae_base.yaml:8-19,64-73): n_embed 32, 16 inducing
 * points, trunk heads 8x4, cross heads 4x8, bias=False, shared gene embedding, shared theta, agg_func log1p.
 * ------------------------------------------------------------------------------------------------ */
typedef struct scldm_vae scldm_vae;

typedef struct {
  int n_genes;          /* vocabulary size; tables have n_genes+1 rows */
  int n_embed;          /* 32 */
  int n_inducing;       /* 16 */
  int n_embed_latent;   /* <= 32 (16) */
  int n_layer;          /* trunk Blocks per side */
  int n_head;           /* 8 */
  int n_head_cross;     /* 4 */
  int hidden_dim;       /* SwiGLU hidden: 88 */
  float layernorm_eps;
  int positional_encoding; /* Encoder.pos_embed present (nnets.py:103-106) */
  float nb_temperature; /* NegativeBinomialTransformerLayer.t (stochastic_layers.py:85) */
} scldm_vae_config;

/* One packed plain Block (state_dict prefix `encoder.encoder_layers.i.` / `decoder.decoder_layers.i.`). */
typedef struct {
  const float* ln1_w; const float* ln1_b; /* ln_1 (32) */
  const float* attn_w;                    /* attn.c_attn.weight (96,32) */
  const float* proj_w;                    /* attn.c_proj.weight (32,32) */
  const float* ln2_w; const float* ln2_b;
  const float* w1; const float* w2;       /* mlp.w1/w2.weight (H,32) */
  const float* cproj;                     /* mlp.c_proj.weight (32,H) */
} scldm_vae_block;

/* Cross-attention block parameters (`encoder.ca_layer.` / `decoder.decoder_cross_attention.`). */
typedef struct {
  const float* ln1_w; const float* ln1_b;   /* ln_1 (applied to x) */
  const float* ln1q_w; const float* ln1q_b; /* ln_1q (applied to the queries) */
  const float* attn_kv;                     /* attn.c_attn.weight (64,32): k | v */
  const float* attn_q;                      /* attn.c_attn_q.weight (32,32) */
  const float* attn_proj;                   /* attn.c_proj.weight (32,32) */
  const float* ln2_w; const float* ln2_b;
  const float* w1; const float* w2; const float* cproj; /* mlp */
} scldm_vae_cross;

typedef struct {
  const float* gene_embedding;     /* input_layer.gene_embedding.weight (n_genes+1, 32) */
  const float* inducing_points;    /* encoder.ca_layer.inducing_points (16,32) */
  const float* enc_pos_embed;      /* encoder.pos_embed (1,16,32) or NULL */
  const float* enc_latent_w;       /* encoder.encoder_latent_input.0.weight (n_lat,32) */
  const float* dec_latent_w;       /* decoder.decoder_latent_input.1.weight (32,n_lat) */
  const float* theta;              /* decoder_head.theta.weight (n_genes+1,1) */
  const float* head_w; const float* head_b; /* decoder_head.params (1,32),(1) */
  scldm_vae_cross enc_cross, dec_cross;
  const scldm_vae_block* enc_blocks; /* HOST array of n_layer entries */
  const scldm_vae_block* dec_blocks;
  /* Appended (every offset above is unchanged): decoder_head.ln.weight / .bias (32) of the Gaussian head
   * (GaussianTransformerLayer, stochastic_layers.py:13-35; `decoder_name: gaussian`).  Both NULL: a negative-binomial head,
   * as before.  Both given: a Gaussian head - theta must be NULL, head_w is (1,32), head_b is (1). */
  const float* head_ln_w; const float* head_ln_b;
} scldm_vae_weights;

int scldm_vae_create(const scldm_vae_config* cfg, scldm_vae** out);
void scldm_vae_destroy(scldm_vae* h);
int scldm_vae_load_weights(scldm_vae* h, const scldm_vae_weights* w, void* stream);
/* Same parameter tensors as the last scldm_vae_load_weights (the pointers are remembered), possibly updated in place: a 64-bit
 * fingerprint of every source tensor is compared ON DEVICE with that of the packed copies and the re-pack (one launch over a job
 * table + the two derived tables) runs only if it moved - five small launches, no host synchronisation.  What the Python face calls
 * before every encode / decode whose parameter storages and version counters are unchanged (`.data` updates are invisible to both). */
int scldm_vae_refresh_weights(scldm_vae* h, void* stream);
size_t scldm_vae_workspace_bytes(const scldm_vae* h, int B, int G);

/* TransformerVAE.encode (vae.py:58-69): counts (B,S) fp32, genes (B,S) int64 -> z (B,16,n_lat). */
int scldm_vae_encode(scldm_vae* h, const float* counts, const int64_t* genes, int B, int S, float* z, int precision, void* ws,
                     void* stream);

/* TransformerVAE.decode (vae.py:71-87) up to the distribution parameters: z (B,16,n_lat), genes (B,G) int64,
 * library_size (B) -> mu (B,G) = softmax_G(logit / t) * library_size, theta (B,G) = exp(theta_emb[genes]). */
/* precision (encode, decode, decode_sample): SCLDM_PREC_FP32 = exact-fp32 MFMA chain (parity path, <= 1e-4);
 * SCLDM_PREC_FP16 = fp16 operands for the per-gene MCAB / SwiGLU contractions (10 mantissa bits = TF32, the arithmetic class the
 * reference runs CrossAttention / MLP in under set_float32_matmul_precision("high"): experiments/scripts/inference.py:26,
 * src/scldm/layers.py:248-264,305-330), fp32 accumulate / softmax / LayerNorm / NB head, weights saturated at +-65 504;
 * SCLDM_PREC_BF16 = the same with bf16 operands (8 bits: narrower than the reference).  Both 16-bit policies run about 3x the fp32
 * decode rate; the Linears of the 16-token cell trunks take the policy's operand type too (the reference runs them in TF32 as well;
 * their 16 x 16 attention stays fp32 on the VALU).  Other values: SCLDM_ERR_SHAPE. */
int scldm_vae_decode(scldm_vae* h, const float* z, const int64_t* genes, const float* library_size, int B, int G, float* mu,
                     float* theta, int precision, void* ws, void* stream);

/* TransformerVAE.decode followed by the negative-binomial draw of LatentDiffusion.sample (src/scldm/models.py:819,
 * `nb.sample()` on the distribution vae.py:87 builds): counts (B,G) fp32 ~ Poisson(Gamma(concentration = theta,
 * rate = theta / mu)), the Gamma-Poisson mixture scvi-tools' NegativeBinomial samples.  The draw happens inside the pass that
 * normalises the logits, so mu / theta are never written to HBM.  Philox4x32-10 keyed by `seed`, one counter per output element:
 * reproducible for a given (seed, B, G), independent of the launch geometry.  RNG-dependent: outside the bit-parity claim. */
int scldm_vae_decode_sample(scldm_vae* h, const float* z, const int64_t* genes, const float* library_size, int B, int G,
                            float* counts, unsigned long long seed, int precision, void* ws, void* stream);

/* Measurement hook for bench.py (the MCAB counterpart of scldm_dit_block_timing): when enabled, every launch of an MCAB kernel by
 * scldm_vae_encode / _decode / _decode_sample is bracketed by HIP events on the stream it is launched on (up to 64 launches per
 * kernel kind, later ones are not recorded); scldm_vae_kernel_timing drains one kind (synchronises on its events) and returns the
 * number of recorded launches and their summed duration. */
enum {
  SCLDM_VAE_K_ENC_POOL = 0,   /* enc_pool_kernel: MCAB pooling over the S input genes of a cell */
  SCLDM_VAE_K_ENC_CELL = 1,   /* enc_cell_kernel: c_proj + MLP + 16-token trunk + latent head */
  SCLDM_VAE_K_DEC_CELL = 2,   /* dec_cell_kernel: latent input + 16-token trunk + K | V of the unpooling */
  SCLDM_VAE_K_DEC_GENE = 3,   /* dec_gene_kernel: MCAB unpooling + SwiGLU + NB-head logit per decoded gene */
  SCLDM_VAE_K_DEC_FINAL = 4   /* dec_finalize(_sample)_kernel: softmax over genes x library size (+ the NB draw) */
};
#define SCLDM_VAE_KERNEL_KINDS 5
void scldm_vae_kernel_timing_enable(scldm_vae* h, int enable);
int scldm_vae_kernel_timing(scldm_vae* h, int kind, int* n_launches, double* total_ms);

/* The same draw from explicit parameter tensors: out[i] ~ NB(mu[i], theta[i]), i < n  (NegativeBinomial(mu, theta).sample()). */
int scldm_nb_sample(const float* mu, const float* theta, float* out, size_t n, unsigned long long seed, void* stream);

/* TransformerVAE.decode with the Gaussian head (vae.py:82-85; the handle's weights carry head_ln_w / head_ln_b):
 * mu (B,G) = params(LayerNorm(h_x)), the mean of Normal(mu, 1); library_size plays no part.  The per-gene kernel stores mu itself:
 * no pass over (B,G) follows it.  The LayerNorm and the 32 -> 1 product of the head are fp32 in every `precision`.  Workspace:
 * scldm_vae_workspace_bytes.  A handle with a negative-binomial head returns SCLDM_ERR_SHAPE; so do scldm_vae_decode,
 * scldm_vae_decode_sample and the NB scldm_vae_train_* entry points on a handle with a Gaussian head (it trains through
 * scldm_vae_train_gaussian_forward / _gaussian_backward below). */
int scldm_vae_decode_gaussian(scldm_vae* h, const float* z, const int64_t* genes, int B, int G, float* mu, int precision, void* ws,
                              void* stream);
/* The same followed by Normal(mu, 1).sample() (models.py:819): out = mu + n with n the standard normal of Philox4x32-10 keyed by
 * `seed`, counter = element index cell * G + position, drawn in the per-gene kernel's epilogue (mu never reaches HBM).  Equal bit for
 * bit to scldm_vae_decode_gaussian followed by scldm_normal_sample with the same seed. */
int scldm_vae_decode_gaussian_sample(scldm_vae* h, const float* z, const int64_t* genes, int B, int G, float* out,
                                     unsigned long long seed, int precision, void* ws, void* stream);
/* out[i] = mu[i] + n_i, i < n: the draw of Normal(mu, 1) from an explicit mean tensor. */
int scldm_normal_sample(const float* mu, float* out, size_t n, unsigned long long seed, void* stream);

/* ------------------------------------------------------------------------------------------------
 * TransformerVAE TRAINING step (BASELINE configs[0]; the reference trains through torch autograd over
 * TransformerVAE.forward, src/scldm/vae.py:29-56, inside VAE.training_step, src/scldm/models.py:249-290, with the loss
 * -log_nb_positive(counts, mu, theta), models.py:243, src/scldm/distributions.py:6-42).  fp32 (fp16 operands: the _ex forms below).
 *   forward : (mu, theta, z) = TransformerVAE.forward(counts, genes, library_size, counts_subset, genes_subset) - the inference
 *             kernels - and leaves in `saved` what the backward cannot recompute cheaply (the pooling's attention output and
 *             log-sum-exp) or should not wait for (the decoder's per-cell K | V); `ws` need not survive the call; uses the packed weights of the last scldm_vae_load_weights (call it after every optimiser step).
 *   backward: given d loss / d mu, d theta (B, G; either may be NULL) and optionally d loss / d z (B, 16, n_lat), writes d loss / d
 *             parameter for EVERY tensor named in `g` (same struct and layouts as scldm_vae_weights, pointers writable; overwritten,
 *             not accumulated; enc_pos_embed is ignored: frozen in the reference, nnets.py:103-106).  Parameters are read LIVE from
 *             `w`.  The two embedding tables' gradients (gene_embedding, theta) are scatter-added with float atomics (like torch's
 *             embedding backward); every other gradient is a deterministic two-stage sum.  scldm_vae_train_backward_ordered below
 *             forms the two tables by a fixed-order sum instead: every gradient is then bit-equal run to run.
 * mu / theta / z passed to the backward are the forward's outputs.  Buffers: scldm_vae_train_saved_bytes / _workspace_bytes.
 * UNSHARED-THETA head (the handle's weights were loaded with theta == NULL: decoder_head.params is Linear(32, 2), theta = exp of its
 * second output, stochastic_layers.py:94-116): the same entries, plain, _ex and _ordered, in fp32 and fp16.  `theta` is then the
 * (B, G) per-element dispersion the forward wrote and `dtheta` its gradient; w->head_w is (2, 32); the backward requires g->head_w
 * (2, 32) and g->head_b (2) and writes both rows (d loss / d head_b[0] is analytically 0 and comes out as the sum it is); g->theta is
 * ignored, there is no theta table to fill or to order.  Under SCLDM_PREC_FP16 the cell's power of two comes from max(|d logit|,
 * |dtheta theta|) and scales both gradient streams.  Query the workspace size after scldm_vae_load_weights: it holds one more (B, G)
 * array for this head. */
size_t scldm_vae_train_saved_bytes(const scldm_vae* h, int B);
size_t scldm_vae_train_workspace_bytes(const scldm_vae* h, int B, int S, int G);
int scldm_vae_train_forward(scldm_vae* h, const float* counts_subset, const int64_t* genes_subset, int B, int S, const int64_t* genes,
                            const float* library_size, int G, float* mu, float* theta, float* z, void* saved, void* ws, void* stream);
int scldm_vae_train_backward(scldm_vae* h, const scldm_vae_weights* w, const scldm_vae_weights* g, const float* counts_subset,
                             const int64_t* genes_subset, int B, int S, const int64_t* genes, const float* library_size, int G,
                             const float* mu, const float* theta, const float* z, const float* dmu, const float* dtheta, const float* dz,
                             void* saved, void* ws, void* stream);

/* The same step with an operand policy (`precision`): SCLDM_PREC_FP32 = the two calls above; SCLDM_PREC_FP16 = the reference's TF32
 * class (set_float32_matmul_precision("high")): fp16 operands rounded to nearest even, fp32 accumulation, in the encoder pooling and
 * the per-gene decoder forward and in every contraction of the per-gene chain backward; the two 16-token trunks, the pooling backward,
 * LayerNorms, softmax, the SwiGLU gradient and the NB head stay fp32.  Forward and backward of one step take the same value; any
 * other value returns SCLDM_ERR_SHAPE.  The fp16 backward scales each cell's logit gradient by a power of
 * two (max |2^e dlogit| in [1024, 2048)) before rounding and its results back by 2^-e (exact), and - if the caller registered one with
 * scldm_vae_train_set_found_inf - sets a device float to 1.0 when the per-gene backward produced a non-finite gradient (reset to 0.0
 * at the start of every fp16 backward): an optimizer that takes GradScaler's `found_inf` skips the step on device. */
int scldm_vae_train_forward_ex(scldm_vae* h, const float* counts_subset, const int64_t* genes_subset, int B, int S, const int64_t* genes,
                               const float* library_size, int G, float* mu, float* theta, float* z, void* saved, void* ws, int precision,
                               void* stream);
int scldm_vae_train_backward_ex(scldm_vae* h, const scldm_vae_weights* w, const scldm_vae_weights* g, const float* counts_subset,
                                const int64_t* genes_subset, int B, int S, const int64_t* genes, const float* library_size, int G,
                                const float* mu, const float* theta, const float* z, const float* dmu, const float* dtheta,
                                const float* dz, void* saved, void* ws, int precision, void* stream);
int scldm_vae_train_set_found_inf(scldm_vae* h, float* found_inf /* device, caller-owned, may be NULL */);

/* How the backward divides its two gene-axis kernels at batch B, S encoder tokens and G decoded genes - host arithmetic, no handle
 * and no GPU: out = {tiles, chunks} of the per-gene decoder kernel (over G), then {tiles, chunks} of the pooling kernel (over S).
 * Every cell gets `chunks` workgroups, each walking `tiles` 64-token tiles in one go; the backward launches with exactly these
 * (about 512 workgroups per kernel, or this process's SCLDM_VAE_GENE_WGS / SCLDM_VAE_POOL_WGS).  For tests and tools that must know
 * which regime a shape runs in: 1 tile per workgroup up to a few cells, 266 and 97 tiles at G = 17 002, S = 6 147 from batch 257.
 * B, S or G below 1, or a NULL out: SCLDM_ERR_SHAPE. */
int scldm_vae_train_split(int B, int S, int G, int out[4]);

/* ORDERED table gradients: scldm_vae_train_backward_ex with the gradients of gene_embedding and theta formed without float atomics.
 * Replaces torch's embedding backward under the autograd of TransformerVAE.forward (src/scldm/vae.py:29-56; the gene-embedding lookups
 * of layers.py:111-118 and the theta lookup of stochastic_layers.py:108-110) when the trainer asks for `deterministic:`
 * (experiments/configs/training/default.yaml:14).  The kernels store every slot's contribution in `rows` (device,
 * scldm_vae_train_rows_bytes; written completely by each call, needs no initialisation) and a reduction adds, for each table row, the
 * entries the caller's index lists for it, in the listed order.
 *   entries: decoder slot (cell, slot) is entry cell * G + slot; encoder token (cell, tok) is entry B * G + cell * S + tok.
 *   order  : device, n_entries entry indices grouped by table row (the row of a decoder entry is genes[cell][slot], of an encoder entry
 *            genes_subset[cell][tok]).  The order inside a row IS the summation order; any fixed order is legal (scldm_amd.vae.table_order
 *            lists ascending entry indices).  Entries may be omitted - their contribution is then dropped: omit only encoder tokens with
 *            a zero count, whose contribution is exactly zero (the atomic path skips them too).
 *   seg    : device, n_genes + 2 offsets into `order`: table row r owns order[seg[r] .. seg[r + 1]); a row with an empty segment
 *            receives exact zeros.
 *   theta  : uses the same index - its reduction walks the same segments and takes the decoder entries (those below B * G) only; no
 *            second pair of arrays.
 * Guarantee: the same inputs give bit-equal gradients for EVERY tensor run to run, on one build and one GPU model.  No equality
 * across SCLDM_VAE_GENE_WGS / SCLDM_VAE_POOL_WGS settings (they change other partial sums too), and none with the atomic mode beyond
 * rounding (same addends, another order); every gradient but the two tables is bit-equal between the modes.  SCLDM_PREC_FP32 and
 * SCLDM_PREC_FP16, the found-inf flag and the two-stream overlap are those of scldm_vae_train_backward_ex; the reduction runs after
 * both producers of `rows`.  NULL order (with n_entries > 0) / seg / rows, or n_entries outside [0, B * G + B * S]: SCLDM_ERR_SHAPE.
 * Entries outside [0, B * G + B * S) are skipped by the reduction, never dereferenced. */
size_t scldm_vae_train_rows_bytes(const scldm_vae* h, int B, int S, int G);
int scldm_vae_train_backward_ordered(scldm_vae* h, const scldm_vae_weights* w, const scldm_vae_weights* g, const float* counts_subset,
                                     const int64_t* genes_subset, int B, int S, const int64_t* genes, const float* library_size, int G,
                                     const float* mu, const float* theta, const float* z, const float* dmu, const float* dtheta,
                                     const float* dz, void* saved, void* ws, int precision, const int32_t* order, const int32_t* seg,
                                     int n_entries, void* rows, void* stream);

/* The training step of a handle with the GAUSSIAN head (GaussianTransformerLayer; loss log_gaussian(log1p(counts / rowsum * 1e4),
 * mu).sum(1).mean(), models.py:239-245), fp32, beside the NB entries above as scldm_vae_decode_gaussian sits beside scldm_vae_decode.
 *   forward : (mu, z) on the inference kernels (the per-gene kernel writes mu itself); `saved` as scldm_vae_train_forward leaves it.
 *   backward: given d loss / d mu (B, G; may be NULL) and optionally d loss / d z, writes every gradient named in `g`, now including
 *             g->head_ln_w, g->head_ln_b, g->head_w (1,32) and g->head_b (1) - the bias gradient is real here; g->theta is ignored.
 *             order == NULL: gene_embedding by float atomics (seg, n_entries, rows are ignored); otherwise order / seg / n_entries /
 *             rows are those of scldm_vae_train_backward_ordered and every gradient is bit-equal run to run.
 * The LayerNorm in front of the head makes the gradient entering the per-gene MLP rank two, so the per-gene backward is a kernel of
 * its own (one workgroup per CU).  scldm_vae_train_saved_bytes / _workspace_bytes / _rows_bytes / _split serve both heads.  A handle
 * with a negative-binomial head returns SCLDM_ERR_SHAPE (the message names the head), as the NB entries do on a Gaussian handle. */
int scldm_vae_train_gaussian_forward(scldm_vae* h, const float* counts_subset, const int64_t* genes_subset, int B, int S,
                                     const int64_t* genes, int G, float* mu, float* z, void* saved, void* ws, void* stream);
int scldm_vae_train_gaussian_backward(scldm_vae* h, const scldm_vae_weights* w, const scldm_vae_weights* g, const float* counts_subset,
                                      const int64_t* genes_subset, int B, int S, const int64_t* genes, int G, const float* mu,
                                      const float* z, const float* dmu, const float* dz, void* saved, void* ws, const int32_t* order,
                                      const int32_t* seg, int n_entries, void* rows, void* stream);

/* log_nb_positive (src/scldm/distributions.py:6-42) elementwise over n values, and its gradient w.r.t. mu and theta given the
 * upstream gradient of the log-likelihood (either output may be NULL):
 *   res = theta (log(theta + eps) - L) + x (log(mu + eps) - L) + lgamma(x + theta) - lgamma(theta) - lgamma(x + 1),  L = log(theta + mu + eps) */
int scldm_nb_loglik(const float* x, const float* mu, const float* theta, float eps, float* out, size_t n, void* stream);
int scldm_nb_loglik_bwd(const float* x, const float* mu, const float* theta, const float* gout, float eps, float* dmu, float* dtheta,
                        size_t n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Encoder input path: tokenize_cells(sample_genes="expressed"),
 * reference src/scldm/datamodule.py:660-731.  counts: device (N,G) fp32; gene_idx: device int64 token ids,
 * one shared row (gene_row_stride 0) or per cell (gene_row_stride G) - the reference tiles one row N times (:691).
 * Outputs: genes_subset (N,S) int64 and counts_subset (N,S) fp32 - expressed genes (counts > 0) in gene order,
 * padded with mask_idx / 0 (:709-716); num_expressed (N) int32; library_size (N) fp32 = row sums (:692).
 * Rows with num_expressed > S keep their first S expressed genes; the caller raises like the reference (:706-707).
 * ------------------------------------------------------------------------------------------------ */
int scldm_tokenize_expressed(const float* counts, const int64_t* gene_idx, long gene_row_stride, int N, int G, int S,
                             int64_t mask_idx, int64_t* genes_subset, float* counts_subset, int32_t* num_expressed,
                             float* library_size, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Output assembly: dense generated counts (N,G) fp32 -> CSR on device, replacing the
 * per-batch scipy.sparse.csr_matrix(counts.cpu().numpy()) of src/scldm/_utils.py:192-197 (after models.py:742).
 * Entries != 0 are kept in column order.  scldm_csr_count writes nnz per row; the caller forms
 * indptr (N+1) int64 = exclusive scan of it; scldm_csr_fill writes indices (nnz) int32 and data (nnz) fp32.
 * ------------------------------------------------------------------------------------------------ */
int scldm_csr_count(const float* dense, int N, int G, int32_t* row_nnz, void* stream);
int scldm_csr_fill(const float* dense, int N, int G, const int64_t* indptr, int32_t* indices, float* data, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Generation-evaluation MMD: kernel matrices of src/scldm/evaluations.py:10-69 and the
 * sums MMDLoss needs (:72-82), without the (Bx,By,D) broadcast tensors of the reference.
 * x (nx,D), y (ny,D) device fp32.  sum_out: device double = sum_ij k(x_i, y_j).  kmat: device (nx,ny) fp32 or NULL.
 * ------------------------------------------------------------------------------------------------ */
#define SCLDM_MMD_RBF 0         /* exp(-scale * |x - y|^2), evaluations.py:10-21 */
#define SCLDM_MMD_BRAYCURTIS 1  /* 1 - sum|x - y| / (sum|x + y| + 1e-8), :24-37 */
#define SCLDM_MMD_TANIMOTO 2    /* sum xy / (sum(x + y - xy) + 1e-8), :40-53 */
#define SCLDM_MMD_RUZICKA 3     /* sum min / (sum max + 1e-8), :56-69 */
#define SCLDM_MMD_SQDIST 4      /* |x - y|^2: the cost matrix of wasserstein(power=2), :103-105 */
#define SCLDM_MMD_DIST 5        /* |x - y|  (torch.cdist): wasserstein(power=1) */
size_t scldm_mmd_workspace_bytes(int nx, int ny);
int scldm_mmd_kernel_sum(const float* x, int nx, const float* y, int ny, int D, int kind, float scale, double* sum_out,
                         float* kmat, void* ws, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Entropic optimal transport for the Wasserstein generation metrics: wasserstein(x0, x1, method="sinkhorn", reg, power) of
 * src/scldm/evaluations.py:85-108 (models.py:47-48 binds power 1 and 2) up to the final sqrt: uniform marginals,
 * M = cdist(x0, x1) ** power, Sinkhorn-Knopp scaling as third-party POT's ot.sinkhorn2 iterates it (error checked every
 * 10th iteration against stop_thr; POT default 1e-9; additionally ends when that error, already below 1e-6, has stopped
 * improving for three checks - the fp32 floor, which may sit above 1e-9), returns the HOST double *cost_out = <P, M>.  POT is not vendored:
 * parity unpinned, pinned to oracle/evaluations.py.  x0 (n,D), x1 (m,D) device fp32.  Synchronises the stream (the error
 * check is a host decision).  status: 0 converged, 1 iteration limit reached, 2 a scaling became zero / non-finite (as in
 * POT the previous scalings are kept and the loop ends - what reg = 0.05 on 17k-dimensional inputs usually does).
 * ------------------------------------------------------------------------------------------------ */
size_t scldm_sinkhorn_workspace_bytes(int n, int m);
int scldm_wasserstein_sinkhorn(const float* x0, int n, const float* x1, int m, int D, int power, float reg, long long num_iter_max,
                               float stop_thr, double* cost_out, long long* iters_out, int* status_out, void* ws, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Evaluation metrics of the validation step (src/scldm/models.py:315-331: zeros accuracy, mse, pcc) and of the generation
 * evaluation (:892-928: r2_mean, r2_var) in one fused streaming pass over pred (n_pred,G) and truth (n_true,G), device fp32.
 * U = log1p(pred / pred_div * target_sum), V = log1p(truth / true_div * target_sum); a NULL divisor vector means the
 * row's own sum; target_sum <= 0 means the inputs are already scaled (U = pred, V = truth; the divisors are ignored).
 *   MSE        mean (U - V)^2
 *   PCC        nanmean over genes of the Pearson correlation over cells (NaN where a variance is 0 or n < 2), clamped to [-1, 1]
 *   ZEROS      mean ((pred == 0) == (truth == 0)) on the untransformed inputs
 *   R2_MEAN    r2(U.mean(0), V.mean(0)), r2(preds, target) = 1 - sum (target - preds)^2 / sum (target - mean(target))^2
 *   R2_VAR     the same on the unbiased per-gene variances (NaN for n < 2)
 *   PCC_VALID  number of genes whose correlation is not NaN
 * n_pred != n_true: MSE, PCC and ZEROS are NaN (PCC_VALID 0); the r2 values need no paired rows.  A zero divisor gives the
 * NaN / inf of the expression above, and they propagate.  out: SCLDM_EVAL_N device doubles.  pcc_per_gene: device (G) fp32
 * or NULL.  gene_stats: device (4,G) fp32 = mean_p, var_p, mean_t, var_t, or NULL.  Every sum runs in a fixed order that
 * depends on (n_pred, n_true, G) alone: results are bit-reproducible.  No host synchronisation, no allocation.
 * scldm_log1p_normalize writes log1p(x / div * target_sum) (div NULL: the row's own sum; target_sum <= 0: a copy).
 * ------------------------------------------------------------------------------------------------ */
enum { SCLDM_EVAL_MSE = 0, SCLDM_EVAL_PCC = 1, SCLDM_EVAL_ZEROS = 2, SCLDM_EVAL_R2_MEAN = 3, SCLDM_EVAL_R2_VAR = 4,
       SCLDM_EVAL_PCC_VALID = 5, SCLDM_EVAL_N = 6 };
size_t scldm_eval_workspace_bytes(int n_pred, int n_true, int G);
int scldm_eval_count_metrics(const float* pred, int n_pred, const float* truth, int n_true, int G, const float* pred_div,
                             const float* true_div, float target_sum, double* out, float* pcc_per_gene, float* gene_stats,
                             void* ws, void* stream);
int scldm_log1p_normalize(const float* x, int n, int G, const float* div, float target_sum, float* out, void* stream);
/* Reconstruction loss of the Gaussian head per cell (models.py:239-245 before .mean()): loss_rows[b] = sum_g (log1p(counts[b,g] /
 * rowsum_b * target_sum) - mu[b,g])^2, one workgroup per row, fixed-order sums (bit-reproducible); the scaled counts are those of
 * scldm_log1p_normalize with div = NULL (target_sum <= 0: the counts as they are). */
int scldm_gaussian_recon_loss(const float* counts, const float* mu, int B, int G, float target_sum, float* loss_rows, void* stream);
/* ... and its gradient w.r.t. mu given d / d loss_rows (B): dmu[b,g] = -2 (y[b,g] - mu[b,g]) gout_rows[b], y recomputed as above. */
int scldm_gaussian_recon_loss_bwd(const float* counts, const float* mu, const float* gout_rows, int B, int G, float target_sum,
                                  float* dmu, void* stream);

/* ------------------------------------------------------------------------------------------------
 * ScviVAE: the scVI-style baseline of the reference (src/scldm/vae.py:90-128; EncoderScvi / DecoderScvi nnets.py:19-73,
 * GaussianLinearLayer / NegativeBinomialLinearLayer stochastic_layers.py:38-70,123-158).  Inference (eval mode), exact fp32:
 *   h = x = log1p(counts);  per layer  x = SiLU(BatchNorm1d_eval(Linear(x)))
 *   loc = Linear_loc(h),  scale = exp(hardtanh(Linear_scale(h), -7, 5)),  z = loc + eps scale
 *   g = decoder MLP(z);  mu = library_size softmax_G(Linear_mu(g));  theta = softplus(theta_param) (shared, (G)) or
 *   softplus(Linear_theta(g)) (per cell, (B, G); torch's threshold-20 softplus).
 * All weights are read where they live, in torch's Linear layout (out, in).  Only the BatchNorm affine and the Linear bias of every
 * MLP layer are packed, into y = s x + c per column (s = gamma / sqrt(running_var + eps), c = beta + (b - running_mean) s), by ONE
 * single-workgroup launch that first fingerprints those five vectors of every layer and re-packs only if they moved: scldm_scvi_pack
 * runs it unconditionally, every encode / decode / forward runs it first, so an in-place update of a parameter or a running statistic
 * is picked up in stream order without a host read.
 * Every product accumulates each output element in one fixed k order (a first layer with K > 1024 is split over K in chunks of 1024 -
 * a function of K alone - and a second launch sums the chunks in order); the softmax over genes merges per-tile (max, sum exp) pairs
 * in tile order.  No float atomics: results are bit-equal run to run, and a row's results do not depend on the other rows of the batch.
 * scldm_scvi_create allocates nothing on the device and needs none; the first scldm_scvi_pack of a handle allocates the packed
 * vectors.  After it, pack / encode / decode / forward make kernel launches only and can be captured into a graph.
 * SCLDM_ERR_SHAPE with a message and nothing launched: a NULL or misaligned pointer (floats 4 bytes, ws 256 bytes), a layer count
 * below 1 (or above 8), a non-positive dimension or B, n_library != B.  SCLDM_ERR_STATE: encode / decode / forward before pack.
 * ------------------------------------------------------------------------------------------------ */
typedef struct scldm_scvi scldm_scvi;
typedef struct {
  const float* w;        /* Linear weight (n_hidden, in) */
  const float* b;        /* Linear bias (n_hidden) */
  const float* bn_w;     /* BatchNorm1d weight, bias, running_mean, running_var (n_hidden each) */
  const float* bn_b;
  const float* bn_mean;
  const float* bn_var;
} scldm_scvi_layer;
typedef struct {
  const scldm_scvi_layer* enc;   /* n_enc_layers entries; layer 0 has in = n_genes */
  const scldm_scvi_layer* dec;   /* n_dec_layers entries; layer 0 has in = n_latent */
  const float* loc_w;   const float* loc_b;     /* (n_latent, n_hidden), (n_latent) */
  const float* scale_w; const float* scale_b;
  const float* mu_w;    const float* mu_b;      /* (n_genes, n_hidden), (n_genes) */
  const float* theta_w;                         /* shared theta: the parameter (n_genes); else Linear weight (n_genes, n_hidden) */
  const float* theta_b;                         /* shared theta: ignored (may be NULL); else (n_genes) */
} scldm_scvi_params;

int scldm_scvi_create(int n_enc_layers, int n_dec_layers, int n_genes, int n_hidden, int n_latent, int shared_theta, float bn_eps,
                      scldm_scvi** out);
void scldm_scvi_destroy(scldm_scvi* h);
int scldm_scvi_pack(scldm_scvi* h, const scldm_scvi_params* p, void* stream);
size_t scldm_scvi_workspace_bytes(const scldm_scvi* h, int B);
/* counts (B, n_genes) -> h (B, n_hidden), loc, scale (B, n_latent); with eps (B, n_latent) also z = loc + eps scale (z may be NULL
 * when eps is). */
int scldm_scvi_encode(scldm_scvi* h, const float* counts, int B, const float* eps, float* hout, float* loc, float* scale, float* z,
                      void* ws, void* stream);
/* z (B, n_latent), library_size (n_library = B) -> mu (B, n_genes), theta ((n_genes) shared | (B, n_genes)). */
int scldm_scvi_decode(scldm_scvi* h, const float* z, const float* library_size, int n_library, int B, float* mu, float* theta, void* ws,
                      void* stream);
/* encode (eps required) followed by decode of its z, one fingerprint / pack launch in front. */
int scldm_scvi_forward(scldm_scvi* h, const float* counts, const float* library_size, int n_library, int B, const float* eps, float* hout,
                       float* loc, float* scale, float* z, float* mu, float* theta, void* ws, void* stream);
/* The same three entries with the precision of the products as an argument (in front of ws).  Arguments, checks, workspace
 * (scldm_scvi_workspace_bytes serves both precisions: the activations between launches stay fp32), the fingerprint / pack launch in
 * front and the launch-only / graph-capture property are those of the entry without the suffix.
 *   SCLDM_PREC_FP32  exactly the launches of the plain entry; the results are bit-equal to it.
 *   SCLDM_PREC_FP16  every product on v_mfma_f32_32x32x16_f16 (the reference's TF32 class: 10 explicit mantissa bits, fp32
 *                    accumulate).  Both operands are read as fp32 where they live and rounded to fp16, round-to-nearest-even,
 *                    while they are staged (log1p of the counts is taken in fp32 first); a value beyond +-65 504 saturates to
 *                    +-65 504 as in the MCAB fp16 weight policy above; NaN operands are outside the contract.  There is no packed
 *                    fp16 copy of the weights.  The folded BatchNorm affine, SiLU, loc / scale / z, the logits, the softmax merge
 *                    and softplus stay fp32.  The determinism of the fp32 path holds word for word: one accumulator per output
 *                    element in ascending k order, K > 1024 split in chunks that depend on K alone and summed in split order, no
 *                    float atomics, bit-equal run to run, a row's bits independent of the other rows of the batch.
 *   any other value  SCLDM_ERR_SHAPE with a message, nothing launched (checked after the arguments, before the packed state). */
int scldm_scvi_encode_ex(scldm_scvi* h, const float* counts, int B, const float* eps, float* hout, float* loc, float* scale, float* z,
                         int precision, void* ws, void* stream);
int scldm_scvi_decode_ex(scldm_scvi* h, const float* z, const float* library_size, int n_library, int B, float* mu, float* theta,
                         int precision, void* ws, void* stream);
int scldm_scvi_forward_ex(scldm_scvi* h, const float* counts, const float* library_size, int n_library, int B, const float* eps,
                          float* hout, float* loc, float* scale, float* z, float* mu, float* theta, int precision, void* ws, void* stream);

/* Training of the same model (the reference: VAEScvi.training_step / loss, models.py:942-1113), exact fp32, forward and backward.
 *   forward   per MLP layer: a = x W^T + b; BatchNorm1d in TRAINING mode (batch mean and biased variance per column, the running
 *             statistics updated in place with `momentum`, running_var from the unbiased variance); SiLU; dropout keep / (1 - p).
 *             Then the posterior head (loc, scale, z = loc + eps scale) and the likelihood head as in scldm_scvi_forward.
 *   backward  from the upstream gradients of mu, theta, loc, scale and z (each may be NULL = zero) to every parameter's gradient.
 *             The gradient of a Linear bias in front of a training-mode BatchNorm is mathematically zero and written as exact zeros.
 * `masks`: n_enc_layers + n_dec_layers pointers (encoder first) to (B, n_hidden) keep bytes; an MLP whose rate is 0 ignores its
 * entries (masks may be NULL when both rates are 0).  masks_given = 0: the forward draws each keep byte from Philox4x32-10 keyed by
 * (seed; MLP, layer, row, column) and records it there; masks_given = 1: it reads them.  The backward reads them.
 * `record` (scldm_scvi_train_record_bytes, 256-byte aligned) carries the normalised activations from forward to backward; `ws`
 * (scldm_scvi_train_workspace_bytes) is scratch of one call.  Backward also takes the forward's eps, scale, z, mu and theta back.
 * Every reduction (BatchNorm column sums over the batch, bias gradients, the softmax backward's row sum, the split products) has one
 * fixed order and there are no float atomics: the same inputs, seed and build give the same bits.  A row's results depend on the
 * other rows of the batch (BatchNorm).  The forward ends with the fingerprint / pack launch of scldm_scvi_pack, so an eval call after
 * a step sees the new running statistics.  SCLDM_ERR_SHAPE with nothing launched: the checks of scldm_scvi_forward, B < 2 (torch's
 * BatchNorm refuses one row in training mode), a rate outside [0, 1), momentum outside [0, 1], a missing mask or gradient pointer. */
typedef struct { float* dw; float* db; float* dgamma; float* dbeta; } scldm_scvi_layer_grads;
typedef struct {
  const scldm_scvi_layer_grads* enc;   /* n_enc_layers entries */
  const scldm_scvi_layer_grads* dec;   /* n_dec_layers entries */
  float* loc_w;   float* loc_b;
  float* scale_w; float* scale_b;
  float* mu_w;    float* mu_b;
  float* theta_w;                      /* shared theta: (n_genes); else (n_genes, n_hidden) */
  float* theta_b;                      /* shared theta: ignored (may be NULL) */
} scldm_scvi_grads;
size_t scldm_scvi_train_record_bytes(const scldm_scvi* h, int B);
size_t scldm_scvi_train_workspace_bytes(const scldm_scvi* h, int B);
int scldm_scvi_train_forward(scldm_scvi* h, const float* counts, const float* library_size, int n_library, int B, const float* eps,
                             float p_enc, float p_dec, unsigned long long seed, unsigned char* const* masks, int masks_given,
                             float momentum, void* record, float* loc, float* scale, float* z, float* mu, float* theta, void* ws,
                             void* stream);
int scldm_scvi_train_backward(scldm_scvi* h, const float* counts, const float* library_size, int n_library, int B, const float* eps,
                              float p_enc, float p_dec, unsigned char* const* masks, const void* record, const float* scale,
                              const float* z, const float* mu, const float* theta, const float* dmu, const float* dtheta,
                              const float* dloc, const float* dscale, const float* dz, const scldm_scvi_grads* grads, void* ws,
                              void* stream);
/* The same step with the precision of its products as an argument (in front of ws); forward and backward of one step take the same
 * value.  Arguments, checks, record and workspace (the two size functions serve both precisions) are those of the plain entries.
 *   SCLDM_PREC_FP32  exactly the launches of the plain entries, which are calls of these; bit-equal results.
 *   SCLDM_PREC_FP16  the reference's TF32 class (it trains under torch.set_float32_matmul_precision("high")): every product of the
 *                    forward and of the backward on v_mfma_f32_32x32x16_f16 with the operand policy of scldm_scvi_forward_ex (fp32
 *                    where the operands live, rounded to fp16 while staged, log1p in fp32 first, saturation at +-65 504, fp32
 *                    accumulate).  BatchNorm forward and backward, SiLU and its derivative, dropout, the posterior head, the softmax
 *                    and its backward, the bias column sums and the split sums stay fp32.  Every gradient tensor that is an operand
 *                    (dlogit, the theta logits' gradient, each layer's da, dloc_t, dlog_scale) is staged as 2^e d with one e per
 *                    tensor, e = 10 - floor(log2(max |d|)) (max |2^e d| in [1024, 2048); 0 for a zero or non-finite tensor; |e| <=
 *                    126), and the product is multiplied by 2^-e, both exact: callers pass unscaled gradients, there is no loss
 *                    scale.  max |d| is an unsigned maximum of magnitude bits formed on the device by the kernel that writes the
 *                    tensor; the host never reads it.  The determinism statement above holds word for word.
 *   any other value  SCLDM_ERR_SHAPE with a message, nothing launched, nothing written (checked after the arguments, before the
 *                    packed state).
 * scldm_scvi_train_set_found_inf registers a caller-owned device float (NULL: none) with the contract of
 * scldm_vae_train_set_found_inf: every SCLDM_PREC_FP16 backward resets it to 0.0 at its start and sets it to 1.0 when an upstream
 * gradient or one of the gradient tensors above is non-finite, or when a parameter gradient it produced is; an optimizer that takes
 * GradScaler's `found_inf` (scldm_adamw_step) then skips the step on device.  The fp32 backward never touches it. */
int scldm_scvi_train_forward_ex(scldm_scvi* h, const float* counts, const float* library_size, int n_library, int B, const float* eps,
                                float p_enc, float p_dec, unsigned long long seed, unsigned char* const* masks, int masks_given,
                                float momentum, void* record, float* loc, float* scale, float* z, float* mu, float* theta,
                                int precision, void* ws, void* stream);
int scldm_scvi_train_backward_ex(scldm_scvi* h, const float* counts, const float* library_size, int n_library, int B, const float* eps,
                                 float p_enc, float p_dec, unsigned char* const* masks, const void* record, const float* scale,
                                 const float* z, const float* mu, const float* theta, const float* dmu, const float* dtheta,
                                 const float* dloc, const float* dscale, const float* dz, const scldm_scvi_grads* grads, int precision,
                                 void* ws, void* stream);
int scldm_scvi_train_set_found_inf(scldm_scvi* h, float* found_inf /* device, caller-owned, may be NULL */);

/* ------------------------------------------------------------------------------------------------
 * TransformerVAE inference beyond the 32-wide shape: a handle family of its own (scldm_vaew_*), config and weight structs shared with
 * scldm_vae_*.  The shape family, checked by scldm_vaew_create before any HIP call (SCLDM_ERR_SHAPE, the message names the violated
 * condition): n_embed % 32 == 0 and 64 <= n_embed <= 1024; n_embed % n_head == 0 and n_embed % n_head_cross == 0 with both head dims
 * multiples of 8 in [8, 256]; 1 <= n_inducing <= 64; 1 <= n_embed_latent <= n_embed; n_layer >= 0; any hidden_dim >= 1; positional
 * encoding on or off; bias=False, shared gene embedding, no adaLN; the negative-binomial head with a theta table or (theta = NULL)
 * with the two-logit params.  The Gaussian head (head_ln_w / head_ln_b given) is refused by scldm_vaew_load_weights.
 *
 * Inference only: encode and decode (the draw is scldm_nb_sample on decode's output).  `precision`: SCLDM_PREC_FP32 (every product on
 * v_mfma_f32_32x32x2_f32, <= 1e-4 against the reference) or SCLDM_PREC_FP16 (v_mfma_f32_32x32x16_f16, operands rounded while they are
 * staged: the reference's TF32 class; LayerNorm, attention, softmax and the head stay fp32); anything else: SCLDM_ERR_SHAPE.
 *
 * Nothing derived from the weights is kept: scldm_vaew_load_weights only remembers the pointers (no HIP call, `stream` unused), every
 * call reads the parameters where they live, so an in-place update is seen by the next call.  No allocation in encode / decode: the
 * caller passes scldm_vaew_workspace_bytes(h, B, S, G) bytes (S or G may be 0 when only the other call follows; 0 is returned when a
 * single cell does not fit the cap).  The cells of a call are processed in chunks whose workspace stays under a cap: 1024 MiB, or
 * SCLDM_VAEW_WS_MB (MiB, read at scldm_vaew_create).  Results are bit-equal run to run and do not depend on the chunking or on the
 * other cells of the batch.
 *
 * scldm_vaew_plan is host arithmetic: how B cells of `tokens` tokens (decode == 0: S encoder tokens, else G decoded genes) are cut
 * under `cap_bytes` (0 = the handle's cap): chunk i holds cells [i * cells_per_chunk, min(B, (i + 1) * cells_per_chunk)), ws_bytes is
 * the workspace of one chunk.  One cell above the cap: SCLDM_ERR_SHAPE.
 * ------------------------------------------------------------------------------------------------ */
typedef struct scldm_vaew scldm_vaew;
int scldm_vaew_create(const scldm_vae_config* cfg, scldm_vaew** out);
void scldm_vaew_destroy(scldm_vaew* h);
int scldm_vaew_load_weights(scldm_vaew* h, const scldm_vae_weights* w, void* stream);
int scldm_vaew_plan(const scldm_vaew* h, int decode, int B, int tokens, size_t cap_bytes, int* cells_per_chunk, int* n_chunks,
                    size_t* ws_bytes);
size_t scldm_vaew_workspace_bytes(const scldm_vaew* h, int B, int S, int G);
/* counts (B,S) fp32, genes (B,S) int64 -> z (B, n_inducing, n_embed_latent) */
int scldm_vaew_encode(scldm_vaew* h, const float* counts, const int64_t* genes, int B, int S, float* z, int precision, void* ws,
                      void* stream);
/* z (B, n_inducing, n_embed_latent), genes (B,G) int64, library_size (B) -> mu (B,G) = softmax_G(logit / t) * library_size,
 * theta (B,G) = exp(theta table row) or exp(second logit) */
int scldm_vaew_decode(scldm_vaew* h, const float* z, const int64_t* genes, const float* library_size, int B, int G, float* mu,
                      float* theta, int precision, void* ws, void* stream);

/* Training of the wide shapes: the backward of TransformerVAE.forward = scldm_vaew_encode on the subset + scldm_vaew_decode on all genes,
 * exact fp32 (both NB heads).  There is no recording forward: the caller keeps the inputs and (mu, theta, z) of the two inference calls,
 * and scldm_vaew_train_backward rebuilds what it needs.  For each chunk of cells, in ascending order: the decoder chain is re-run from the
 * saved z with the inference kernels, every stage into a buffer of its own (the two SwiGLU pre-activations by two plain products), and
 * walked back; dz = the upstream dz + the decoder's; the encoder chain is re-run from the inputs and walked back.  The chunk size comes
 * from scldm_vaew_train_plan under the handle's cap (SCLDM_VAEW_WS_MB, as for inference); one cell whose record exceeds the cap is
 * SCLDM_ERR_SHAPE, the message names the bytes needed.
 *
 * `g` is a scldm_vae_weights of gradient pointers (writable, zero-initialised by the caller; enc_pos_embed is frozen in the reference and
 * is not written; theta is NULL for the unshared head).  dmu, dtheta (B,G) and dz (B, n_inducing, n_embed_latent) may each be NULL.
 * (order, seg, n_order) is the index of scldm_amd.vae.table_order over n_genes + 1 table rows: entry cell * G + slot is a decoder slot,
 * entry B * G + cell * S + tok an encoder token; `rows` holds scldm_vaew_train_rows_bytes bytes (the per-entry rows of the gene table and
 * of the theta table, written completely by the call), `ws` scldm_vaew_train_workspace_bytes (0: one cell does not fit the cap).
 *
 * No float atomics: every product accumulates in ascending k with k-splits that depend on the row count alone and are added in split
 * order, LayerNorm / head column sums go through per-workgroup partials merged in workgroup order, attention splits in split order, the
 * tables in the index's order, and weight gradients accumulate over the chunks in chunk order.  Every gradient is bit-equal run to run
 * on one build, one GPU model and one cap; under another cap (another chunking) the weight gradients may differ in the last bits. */
int scldm_vaew_train_plan(const scldm_vaew* h, int B, int S, int G, size_t cap_bytes, int* cells_per_chunk, int* n_chunks, size_t* ws_bytes);
size_t scldm_vaew_train_workspace_bytes(const scldm_vaew* h, int B, int S, int G);
size_t scldm_vaew_train_rows_bytes(const scldm_vaew* h, int B, int S, int G);
int scldm_vaew_train_backward(scldm_vaew* h, const scldm_vae_weights* g, const float* counts_subset, const int64_t* genes_subset, int B, int S,
                              const int64_t* genes, const float* library_size, int G, const float* mu, const float* theta, const float* z,
                              const float* dmu, const float* dtheta, const float* dz, const int32_t* order, const int32_t* seg, int n_order,
                              void* rows, void* ws, void* stream);

/* Debug hook (tools/phase_timing.py): device buffer receiving 16 x u64 s_memtime phase stamps per
 * (workgroup, wave) of each fused-block launch.  Only builds with -DSCLDM_PHASE_TIMING record; the
 * production library returns SCLDM_ERR_STATE. */
int scldm_dit_set_debug_buffer(scldm_dit* h, void* dev_buf);

#ifdef __cplusplus
}
#endif
#endif /* SCLDM_HIP_H */

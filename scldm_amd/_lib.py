"""ctypes binding of libscldm_hip.so (C ABI in include/scldm_hip.h).

There is NO CPU fallback: importing the product without the built HIP library raises.
Build it with `./build.sh` (hipcc --offload-arch=gfx950) or `python -c "import __graft_entry__ as g; g.build()"`.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SCLDM_LIB", os.path.join(_HERE, "libscldm_hip.so"))  # SCLDM_LIB: debug-build override

MAX_CLASSES = 8
PREC_FP32, PREC_BF16, PREC_BF16X3, PREC_FP16 = 0, 1, 2, 3
METHOD_EULER, METHOD_HEUN = 0, 1
PRECISIONS = {"fp32": PREC_FP32, "bf16": PREC_BF16, "bf16x3": PREC_BF16X3, "fp16": PREC_FP16}
METHODS = {"euler": METHOD_EULER, "heun": METHOD_HEUN}
SDE_FORMS = {"sigma": 0, "linear": 1, "constant": 2, "decreasing": 3, "inccreasing-decreasing": 4, "SBDM": 5}   # SCLDM_SDE_FORM_*
SDE_LAST_STEPS = {None: 0, "Mean": 1, "Tweedie": 2, "Euler": 3}                                                  # SCLDM_SDE_LAST_*
OPT_CFG1_DIRECT = 1
OPT_TAIL_SPLIT = 2   # scldm_dit_set_option (include/scldm_hip.h)

c_float_p = C.POINTER(C.c_float)
c_void_pp = C.POINTER(C.c_void_p)


class DitConfig(C.Structure):
    _fields_ = [("n_embed", C.c_int), ("n_embed_input", C.c_int), ("n_layer", C.c_int), ("n_head", C.c_int),
                ("seq_len", C.c_int), ("hidden_dim", C.c_int), ("layernorm_eps", C.c_float), ("n_classes", C.c_int),
                ("class_vocab", C.c_int * MAX_CLASSES), ("has_null_row", C.c_int)]


class DitWeights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("pos_embed", "t_w0", "t_b0", "t_w2", "t_b2", "in_w", "in_b", "fin_w", "fin_b",
                                          "fin_ada_w", "fin_ada_b")] + \
               [(n, c_void_pp) for n in ("class_emb", "attn_w", "attn_b", "proj_w", "proj_b", "w1", "w2", "cproj", "ada_w", "ada_b")]


class AdamwEntry(C.Structure):
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("n", C.c_longlong)]


class VaeConfig(C.Structure):
    _fields_ = [("n_genes", C.c_int), ("n_embed", C.c_int), ("n_inducing", C.c_int), ("n_embed_latent", C.c_int),
                ("n_layer", C.c_int), ("n_head", C.c_int), ("n_head_cross", C.c_int), ("hidden_dim", C.c_int),
                ("layernorm_eps", C.c_float), ("positional_encoding", C.c_int), ("nb_temperature", C.c_float)]


class VaeBlock(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("ln1_w", "ln1_b", "attn_w", "proj_w", "ln2_w", "ln2_b", "w1", "w2", "cproj")]


class VaeCross(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("ln1_w", "ln1_b", "ln1q_w", "ln1q_b", "attn_kv", "attn_q", "attn_proj", "ln2_w", "ln2_b",
                                          "w1", "w2", "cproj")]


class VaeWeights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("gene_embedding", "inducing_points", "enc_pos_embed", "enc_latent_w", "dec_latent_w",
                                          "theta", "head_w", "head_b")] + \
               [("enc_cross", VaeCross), ("dec_cross", VaeCross), ("enc_blocks", C.POINTER(VaeBlock)), ("dec_blocks", C.POINTER(VaeBlock))] + \
               [("head_ln_w", C.c_void_p), ("head_ln_b", C.c_void_p)]       # appended: decoder_head.ln of the Gaussian head (NULL = NB head)


class AdamwLaunch(C.Structure):
    """scldm_adamw_launch (include/scldm_hip.h)."""
    _fields_ = [("table", C.c_void_p), ("count", C.c_int), ("n_blocks", C.c_int), ("step", C.c_void_p), ("found_inf", C.c_void_p),
                ("hyper", C.c_void_p), ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
                ("weight_decay", C.c_float), ("maximize", C.c_int), ("max_grad_norm", C.c_float), ("clip_ws", C.c_void_p)]


class TrainStepBuffers(C.Structure):
    """scldm_train_step_buffers (include/scldm_hip.h)."""
    _fields_ = [("row_elems", C.c_int)] + [(n, C.c_void_p) for n in ("t", "x0", "xt", "ut", "pred", "dpred", "labels", "loss_rows", "loss_mean",
                                                                      "ticket", "saved", "ws")]


class Dopri5Stats(C.Structure):
    """scldm_dopri5_stats (include/scldm_hip.h)."""
    _fields_ = [("evaluations", C.c_longlong), ("accepted", C.c_longlong), ("rejected", C.c_longlong), ("first_step", C.c_double),
                ("status", C.c_int), ("step_log_len", C.c_int)]


class Dopri5Plan(C.Structure):
    """scldm_dopri5_plan (include/scldm_hip.h)."""
    _fields_ = [("t_stage", C.c_float * 6), ("a", (C.c_float * 7) * 6), ("err", C.c_float * 7), ("mid", C.c_float * 7),
                ("a_mask", C.c_uint * 6), ("err_mask", C.c_uint), ("mid_mask", C.c_uint), ("h", C.c_float), ("two_h", C.c_float)]


class Dopri5Control(C.Structure):
    """scldm_dopri5_control_out (include/scldm_hip.h)."""
    _fields_ = [("accepted", C.c_int), ("underflow", C.c_int), ("t1", C.c_double), ("h_next", C.c_double)]


class TransportC(C.Structure):
    """scldm_transport (include/scldm_hip.h): path 0 Linear | 1 GVP, model 0 velocity | 1 noise | 2 score, weight 0 none | 1 velocity | 2 likelihood."""
    _fields_ = [("path", C.c_int), ("model", C.c_int), ("weight", C.c_int), ("train_eps", C.c_float), ("sample_eps", C.c_float)]


class TransportCoef(C.Structure):
    """scldm_transport_coef (include/scldm_hip.h)."""
    _fields_ = [(n, C.c_double) for n in ("alpha", "d_alpha", "sigma", "d_sigma", "ratio", "dv", "a", "b", "c", "w")]


class ScviLayer(C.Structure):
    """scldm_scvi_layer (include/scldm_hip.h)."""
    _fields_ = [(n, C.c_void_p) for n in ("w", "b", "bn_w", "bn_b", "bn_mean", "bn_var")]


class ScviLayerGrads(C.Structure):
    """scldm_scvi_layer_grads (include/scldm_hip.h)."""
    _fields_ = [(n, C.c_void_p) for n in ("dw", "db", "dgamma", "dbeta")]


class ScviGrads(C.Structure):
    """scldm_scvi_grads (include/scldm_hip.h)."""
    _fields_ = [("enc", C.POINTER(ScviLayerGrads)), ("dec", C.POINTER(ScviLayerGrads))] + \
               [(n, C.c_void_p) for n in ("loc_w", "loc_b", "scale_w", "scale_b", "mu_w", "mu_b", "theta_w", "theta_b")]


class ScviParams(C.Structure):
    """scldm_scvi_params (include/scldm_hip.h)."""
    _fields_ = [("enc", C.POINTER(ScviLayer)), ("dec", C.POINTER(ScviLayer))] + \
               [(n, C.c_void_p) for n in ("loc_w", "loc_b", "scale_w", "scale_b", "mu_w", "mu_b", "theta_w", "theta_b")]


ERR_SOLVER = -4   # SCLDM_ERR_SOLVER


class ScldmError(RuntimeError):
    pass


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build the HIP extension first (./build.sh). "
                          "scldm_amd has no CPU fallback by design.")
    L = C.CDLL(LIB_PATH)
    L.scldm_last_error.restype = C.c_char_p
    L.scldm_version.restype = C.c_int
    L.scldm_dit_create.argtypes = [C.POINTER(DitConfig), C.POINTER(C.c_void_p)]
    L.scldm_dit_destroy.argtypes = [C.c_void_p]
    L.scldm_dit_destroy.restype = None
    L.scldm_dit_load_weights.argtypes = [C.c_void_p, C.POINTER(DitWeights), C.c_void_p]
    L.scldm_dit_refresh_weights.argtypes = [C.c_void_p, C.c_void_p]
    L.scldm_adamw_step.argtypes = [C.POINTER(AdamwEntry), C.c_int, C.c_void_p, C.c_void_p] + [C.c_float] * 5 + [C.c_int, C.c_void_p]
    L.scldm_adamw_table_bytes.argtypes = [C.POINTER(AdamwEntry), C.c_int]
    L.scldm_adamw_table_bytes.restype = C.c_size_t
    L.scldm_adamw_table_build.argtypes = [C.POINTER(AdamwEntry), C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_int)]
    L.scldm_adamw_table_records_bytes.argtypes = [C.c_int]
    L.scldm_adamw_table_records_bytes.restype = C.c_size_t
    L.scldm_adamw_clip_workspace_bytes.argtypes = [C.c_int]
    L.scldm_adamw_clip_workspace_bytes.restype = C.c_size_t
    L.scldm_adamw_table_update.argtypes = [C.POINTER(AdamwEntry), C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_size_t]
    L.scldm_adamw_table_step.argtypes = [C.POINTER(AdamwLaunch), C.c_void_p]
    L.scldm_fm_prepare.argtypes = [C.c_void_p, c_void_pp, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_int, C.c_int,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.scldm_fm_loss_grad.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.scldm_dit_train_step.argtypes = [C.c_void_p, C.POINTER(DitWeights), C.POINTER(DitWeights), C.c_void_p, c_void_pp, C.POINTER(C.c_int), C.c_int,
                                       C.c_int, C.c_float, C.c_void_p, C.c_int, C.c_int, C.POINTER(TrainStepBuffers), C.POINTER(AdamwLaunch), C.c_void_p]
    fpp = C.POINTER(C.c_void_p)
    L.scldm_rk_combine.argtypes = [C.c_void_p, C.c_void_p, fpp, c_float_p, C.c_int, C.c_longlong, C.c_void_p]
    L.scldm_rk_error.argtypes = [C.c_void_p, C.c_void_p, fpp, c_float_p, C.c_int, C.c_longlong, C.c_float, C.c_float, C.c_void_p, C.c_void_p]
    L.scldm_rk_dense.argtypes = [C.c_void_p, C.c_void_p, fpp, c_float_p, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_longlong,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.scldm_rk_poly.argtypes = [C.c_void_p] * 6 + [C.c_float] * 4 + [C.c_longlong, C.c_void_p]
    L.scldm_dit_train_fp16_state.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_longlong), C.POINTER(C.c_int), C.POINTER(C.c_longlong), C.c_void_p]
    L.scldm_dit_train_set_found_inf.argtypes = [C.c_void_p, C.c_void_p]
    L.scldm_dit_fp16_stats.argtypes = [C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.c_void_p]
    L.scldm_dit_label_errors.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_void_p]
    L.scldm_dit_mod_width.argtypes = [C.c_void_p]
    L.scldm_dit_layers_per_launch.argtypes = [C.c_void_p]
    L.scldm_dit_set_option.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.scldm_dit_workspace_bytes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.scldm_dit_workspace_bytes.restype = C.c_size_t
    L.scldm_dit_cond_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int, c_void_pp, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.scldm_dit_forward_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_int, C.c_void_p, C.c_void_p]
    L.scldm_dit_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, c_void_pp, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                    C.c_void_p]
    L.scldm_dit_forward_cfg.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, c_void_pp, C.c_int, C.c_void_p, C.c_int,
                                        C.c_int, C.POINTER(C.c_uint32), c_float_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.scldm_sample_ode.argtypes = [C.c_void_p, C.c_void_p, c_void_pp, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                   C.POINTER(C.c_uint32), c_float_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.scldm_sample_sde.argtypes = [C.c_void_p, C.c_void_p, c_void_pp, C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_uint32), c_float_p,
                                   C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, C.c_void_p, C.c_uint64, C.c_longlong,
                                   C.c_longlong, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.scldm_sample_ode_dopri5_workspace_bytes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.scldm_sample_ode_dopri5_workspace_bytes.restype = C.c_size_t
    L.scldm_sample_ode_dopri5.argtypes = [C.c_void_p, C.c_void_p, c_void_pp, C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_uint32), c_float_p,
                                          C.c_int, C.c_double, C.c_double, C.c_double, C.c_void_p, C.POINTER(Dopri5Stats), C.c_void_p, C.c_int,
                                          C.c_int, C.c_void_p, C.c_void_p]
    a = L.scldm_sample_ode_dopri5.argtypes
    L.scldm_sample_ode_dopri5_at.argtypes = a[:10] + [c_float_p] + a[10:]     # the same call with the host array of save times after num_save
    L.scldm_dopri5_stage_plan.argtypes = [C.c_double, C.c_double, C.POINTER(Dopri5Plan)]
    L.scldm_dopri5_stage_plan.restype = None
    L.scldm_dopri5_control.argtypes = [C.c_double, C.c_double, C.c_double, C.POINTER(Dopri5Control)]
    L.scldm_dopri5_control.restype = None
    L.scldm_dopri5_initial_h0.argtypes = [C.c_double, C.c_double]
    L.scldm_dopri5_initial_h0.restype = C.c_double
    L.scldm_dopri5_initial_step.argtypes = [C.c_double, C.c_double, C.c_double]
    L.scldm_dopri5_initial_step.restype = C.c_double
    L.scldm_sde_noise.argtypes = [C.c_void_p, C.c_longlong, C.c_int, C.c_uint64, C.c_int, C.c_int, C.c_longlong, C.c_longlong, C.c_void_p]
    L.scldm_mfma_sustained_tflops.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_double)]
    L.scldm_dit_block_timing_enable.argtypes = [C.c_void_p, C.c_int]
    L.scldm_dit_block_timing_enable.restype = None
    L.scldm_dit_block_timing.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double)]
    L.scldm_dit_set_debug_buffer.argtypes = [C.c_void_p, C.c_void_p]
    L.scldm_dit_train_saved_bytes.argtypes = [C.c_void_p, C.c_int]
    L.scldm_dit_train_saved_bytes.restype = C.c_size_t
    L.scldm_dit_train_workspace_bytes.argtypes = [C.c_void_p, C.c_int]
    L.scldm_dit_train_workspace_bytes.restype = C.c_size_t
    L.scldm_dit_train_saved_bytes_for.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.scldm_dit_train_saved_bytes_for.restype = C.c_size_t
    L.scldm_dit_train_workspace_bytes_for.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.scldm_dit_train_workspace_bytes_for.restype = C.c_size_t
    L.scldm_dit_train_prepare.argtypes = [C.c_void_p, C.POINTER(DitWeights), C.c_int, C.c_int, C.c_void_p]
    L.scldm_dit_train_set_grad_events.argtypes = [C.c_void_p, c_void_pp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int]
    # scldm_dit_grads has the field order of scldm_dit_weights, so DitWeights serves for both
    L.scldm_dit_train_forward.argtypes = [C.c_void_p, C.POINTER(DitWeights), C.c_void_p, C.c_void_p, c_void_pp, C.c_int, C.c_void_p,
                                          C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.scldm_dit_train_backward.argtypes = [C.c_void_p, C.POINTER(DitWeights), C.POINTER(DitWeights), C.c_void_p, c_void_pp,
                                           C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.scldm_dit_train_workspace_bytes_dx_for.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.scldm_dit_train_workspace_bytes_dx_for.restype = C.c_size_t
    L.scldm_dit_train_backward_dx.argtypes = [C.c_void_p, C.POINTER(DitWeights), C.c_void_p, c_void_pp, C.c_void_p, C.c_int, C.c_void_p,
                                              C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.scldm_logp_workspace_bytes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.scldm_logp_workspace_bytes.restype = C.c_size_t
    L.scldm_logp_ode.argtypes = [C.c_void_p, C.POINTER(DitWeights), C.c_void_p, c_void_pp, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                 C.POINTER(C.c_uint32), c_float_p, C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_longlong, C.c_longlong,
                                 C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    # record-free inference of the shapes outside the fused family (the fused entries' arguments with the live weight struct in front)
    L.scldm_dit_infer_workspace_bytes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
    L.scldm_dit_infer_workspace_bytes.restype = C.c_size_t
    L.scldm_dit_infer_cond_rows.argtypes = [C.c_void_p, C.POINTER(DitWeights), C.c_void_p, C.c_int, c_void_pp, C.c_int, C.c_void_p, C.c_int,
                                            C.c_void_p, C.c_void_p]
    L.scldm_dit_infer_forward_rows.argtypes = [C.c_void_p, C.POINTER(DitWeights), C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.scldm_dit_infer_forward_cfg.argtypes = [C.c_void_p, C.POINTER(DitWeights), C.c_void_p, C.c_void_p, C.c_int, c_void_pp, C.c_int, C.c_void_p,
                                              C.c_int, C.c_int, C.POINTER(C.c_uint32), c_float_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.scldm_dit_infer_sample_ode.argtypes = [C.c_void_p, C.POINTER(DitWeights), C.c_void_p, c_void_pp, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                             C.POINTER(C.c_uint32), c_float_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.scldm_logp_probe.argtypes = [C.c_void_p, C.c_longlong, C.c_int, C.c_uint64, C.c_int, C.c_int, C.c_longlong, C.c_longlong, C.c_void_p]
    L.scldm_logp_ode_dopri5_workspace_bytes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.scldm_logp_ode_dopri5_workspace_bytes.restype = C.c_size_t
    L.scldm_logp_ode_dopri5.argtypes = [C.c_void_p, C.POINTER(DitWeights), C.c_void_p, c_void_pp, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                        C.POINTER(C.c_uint32), c_float_p, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_int, C.c_uint64,
                                        C.c_longlong, C.c_longlong, C.c_void_p, C.c_void_p, C.POINTER(Dopri5Stats), C.c_void_p, C.c_int, C.c_int,
                                        C.c_void_p, C.c_void_p, C.c_void_p]
    L.scldm_fm_mix.argtypes =[C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.scldm_fm_loss.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.scldm_fm_loss_bwd.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.scldm_transport_coef_at.argtypes = [C.POINTER(TransportC), C.c_double, C.POINTER(TransportCoef)]
    a = L.scldm_sample_ode.argtypes
    L.scldm_sample_ode_transport.argtypes = a[:11] + [C.POINTER(TransportC)] + a[11:]
    L.scldm_sample_sde_transport.argtypes = L.scldm_sample_sde.argtypes + [C.POINTER(TransportC)]
    L.scldm_logp_transport_workspace_bytes.argtypes = L.scldm_logp_workspace_bytes.argtypes + [C.POINTER(TransportC)]
    L.scldm_logp_transport_workspace_bytes.restype = C.c_size_t
    L.scldm_logp_ode_transport.argtypes = L.scldm_logp_ode.argtypes + [C.POINTER(TransportC)]
    L.scldm_sde_coef_at.argtypes = [C.POINTER(TransportC), C.c_int, C.c_double, C.c_double, C.c_double, C.POINTER(C.c_double)]
    L.scldm_sde_last_coef_at.argtypes = [C.POINTER(TransportC), C.c_int, C.c_double, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_double)]
    L.scldm_fm_plan.argtypes = [C.POINTER(TransportC)] + [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_void_p]
    L.scldm_fm_wloss.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.scldm_fm_wloss_bwd.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.scldm_fm_prepare_transport.argtypes = [C.POINTER(TransportC)] + L.scldm_fm_prepare.argtypes[:14] + [C.c_void_p] + L.scldm_fm_prepare.argtypes[14:]
    L.scldm_fm_wloss_grad.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p]
    a = L.scldm_dit_train_step.argtypes
    L.scldm_dit_train_step_transport.argtypes = a[:13] + [C.POINTER(TransportC), C.c_void_p] + a[13:]
    L.scldm_vae_create.argtypes = [C.POINTER(VaeConfig), C.POINTER(C.c_void_p)]
    L.scldm_vae_destroy.argtypes = [C.c_void_p]
    L.scldm_vae_destroy.restype = None
    L.scldm_vae_load_weights.argtypes = [C.c_void_p, C.POINTER(VaeWeights), C.c_void_p]
    L.scldm_vae_kernel_timing_enable.argtypes = [C.c_void_p, C.c_int]
    L.scldm_vae_kernel_timing_enable.restype = None
    L.scldm_vae_kernel_timing.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double)]
    L.scldm_vae_refresh_weights.argtypes = [C.c_void_p, C.c_void_p]
    L.scldm_vae_workspace_bytes.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.scldm_vae_workspace_bytes.restype = C.c_size_t
    L.scldm_vae_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.scldm_vae_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                   C.c_int, C.c_void_p, C.c_void_p]
    L.scldm_vae_decode_sample.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_uint64,
                                          C.c_int, C.c_void_p, C.c_void_p]
    L.scldm_vae_decode_gaussian.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.scldm_vae_decode_gaussian_sample.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_int,
                                                   C.c_void_p, C.c_void_p]
    L.scldm_normal_sample.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64, C.c_void_p]
    L.scldm_vae_train_saved_bytes.argtypes = [C.c_void_p, C.c_int]
    L.scldm_vae_train_saved_bytes.restype = C.c_size_t
    L.scldm_vae_train_workspace_bytes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.scldm_vae_train_workspace_bytes.restype = C.c_size_t
    L.scldm_vae_train_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.scldm_vae_train_backward.argtypes = [C.c_void_p, C.POINTER(VaeWeights), C.POINTER(VaeWeights), C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                           C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.scldm_vae_train_forward_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.scldm_vae_train_backward_ex.argtypes = [C.c_void_p, C.POINTER(VaeWeights), C.POINTER(VaeWeights), C.c_void_p, C.c_void_p, C.c_int,
                                              C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.scldm_vae_train_set_found_inf.argtypes = [C.c_void_p, C.c_void_p]
    L.scldm_vae_train_split.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.scldm_vae_train_rows_bytes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.scldm_vae_train_rows_bytes.restype = C.c_size_t
    L.scldm_vae_train_backward_ordered.argtypes = L.scldm_vae_train_backward_ex.argtypes[:-1] + [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                                                                                 C.c_void_p]
    L.scldm_nb_loglik.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_size_t, C.c_void_p]
    L.scldm_nb_loglik_bwd.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.scldm_nb_sample.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64, C.c_void_p]
    L.scldm_tokenize_expressed.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.scldm_csr_count.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.scldm_csr_fill.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.scldm_mmd_workspace_bytes.argtypes = [C.c_int, C.c_int]
    L.scldm_mmd_workspace_bytes.restype = C.c_size_t
    L.scldm_mmd_kernel_sum.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p]
    L.scldm_sinkhorn_workspace_bytes.argtypes = [C.c_int, C.c_int]
    L.scldm_sinkhorn_workspace_bytes.restype = C.c_size_t
    L.scldm_wasserstein_sinkhorn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_longlong, C.c_float,
                                             C.POINTER(C.c_double), C.POINTER(C.c_longlong), C.POINTER(C.c_int), C.c_void_p, C.c_void_p]
    L.scldm_eval_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
    L.scldm_eval_workspace_bytes.restype = C.c_size_t
    L.scldm_eval_count_metrics.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.scldm_log1p_normalize.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
    L.scldm_gaussian_recon_loss.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]
    L.scldm_gaussian_recon_loss_bwd.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]
    L.scldm_vae_train_gaussian_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.scldm_vae_train_gaussian_backward.argtypes = [C.c_void_p, C.POINTER(VaeWeights), C.POINTER(VaeWeights), C.c_void_p, C.c_void_p, C.c_int,
                                                    C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.scldm_scvi_create.argtypes = [C.c_int] * 6 + [C.c_float, C.POINTER(C.c_void_p)]
    L.scldm_scvi_destroy.argtypes = [C.c_void_p]
    L.scldm_scvi_destroy.restype = None
    L.scldm_scvi_pack.argtypes = [C.c_void_p, C.POINTER(ScviParams), C.c_void_p]
    L.scldm_scvi_workspace_bytes.argtypes = [C.c_void_p, C.c_int]
    L.scldm_scvi_workspace_bytes.restype = C.c_size_t
    L.scldm_scvi_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 7
    L.scldm_scvi_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4
    L.scldm_scvi_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 9
    L.scldm_scvi_encode_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.c_void_p, C.c_void_p]
    L.scldm_scvi_decode_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 2 + [C.c_int, C.c_void_p, C.c_void_p]
    L.scldm_scvi_forward_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 7 + [C.c_int, C.c_void_p, C.c_void_p]
    for f in (L.scldm_scvi_train_record_bytes, L.scldm_scvi_train_workspace_bytes):
        f.argtypes = [C.c_void_p, C.c_int]
        f.restype = C.c_size_t
    L.scldm_scvi_train_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_float,
                                           C.c_uint64, C.POINTER(C.c_void_p), C.c_int, C.c_float] + [C.c_void_p] * 8
    L.scldm_scvi_train_backward.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_float,
                                            C.POINTER(C.c_void_p)] + [C.c_void_p] * 10 + [C.POINTER(ScviGrads), C.c_void_p, C.c_void_p]
    L.scldm_scvi_train_forward_ex.argtypes = L.scldm_scvi_train_forward.argtypes[:-2] + [C.c_int, C.c_void_p, C.c_void_p]
    L.scldm_scvi_train_backward_ex.argtypes = L.scldm_scvi_train_backward.argtypes[:-2] + [C.c_int, C.c_void_p, C.c_void_p]
    L.scldm_scvi_train_set_found_inf.argtypes = [C.c_void_p, C.c_void_p]
    # TransformerVAE inference beyond the 32-wide shape (config and weight structs of scldm_vae_*)
    L.scldm_vaew_create.argtypes = [C.POINTER(VaeConfig), C.POINTER(C.c_void_p)]
    L.scldm_vaew_destroy.argtypes = [C.c_void_p]
    L.scldm_vaew_destroy.restype = None
    L.scldm_vaew_load_weights.argtypes = [C.c_void_p, C.POINTER(VaeWeights), C.c_void_p]
    L.scldm_vaew_plan.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_size_t)]
    L.scldm_vaew_workspace_bytes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.scldm_vaew_workspace_bytes.restype = C.c_size_t
    L.scldm_vaew_encode.argtypes = L.scldm_vae_encode.argtypes
    L.scldm_vaew_decode.argtypes = L.scldm_vae_decode.argtypes
    # ... and its training backward (h, gradient struct, counts_subset, genes_subset, B, S, genes, library_size, G, mu, theta, z, dmu,
    # dtheta, dz, order, seg, n_order, rows, ws, stream)
    L.scldm_vaew_train_plan.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                        C.POINTER(C.c_size_t)]
    for f in (L.scldm_vaew_train_workspace_bytes, L.scldm_vaew_train_rows_bytes):
        f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        f.restype = C.c_size_t
    L.scldm_vaew_train_backward.argtypes = ([C.c_void_p, C.POINTER(VaeWeights), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                             C.c_int] + [C.c_void_p] * 8 + [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p])
    _lib = L
    return L


EXPORTS = ["scldm_last_error", "scldm_version", "scldm_dit_create", "scldm_dit_destroy", "scldm_dit_load_weights",
           "scldm_dit_refresh_weights", "scldm_dit_fp16_stats", "scldm_dit_train_fp16_state", "scldm_dit_train_set_found_inf", "scldm_dit_label_errors", "scldm_dit_mod_width", "scldm_dit_layers_per_launch", "scldm_dit_set_option", "scldm_dit_workspace_bytes", "scldm_dit_cond_rows", "scldm_dit_forward_rows",
           "scldm_dit_forward", "scldm_dit_forward_cfg", "scldm_sample_ode", "scldm_adamw_step", "scldm_adamw_table_bytes", "scldm_adamw_table_build", "scldm_adamw_table_records_bytes", "scldm_adamw_clip_workspace_bytes", "scldm_adamw_table_update", "scldm_adamw_table_step", "scldm_fm_prepare", "scldm_fm_loss_grad", "scldm_dit_train_step", "scldm_rk_combine", "scldm_rk_error", "scldm_rk_dense", "scldm_rk_poly", "scldm_mfma_sustained_tflops", "scldm_dit_block_timing_enable",
           "scldm_dit_block_timing", "scldm_dit_set_debug_buffer", "scldm_dit_train_saved_bytes", "scldm_dit_train_workspace_bytes", "scldm_dit_train_saved_bytes_for", "scldm_dit_train_workspace_bytes_for",
           "scldm_dit_train_prepare", "scldm_dit_train_set_grad_events", "scldm_dit_train_forward", "scldm_dit_train_backward", "scldm_fm_mix", "scldm_fm_loss", "scldm_fm_loss_bwd", "scldm_vae_create", "scldm_vae_destroy", "scldm_vae_load_weights", "scldm_vae_refresh_weights", "scldm_vae_kernel_timing_enable", "scldm_vae_kernel_timing",
           "scldm_vae_workspace_bytes", "scldm_vae_encode", "scldm_vae_decode", "scldm_vae_decode_sample", "scldm_vae_train_saved_bytes", "scldm_vae_train_workspace_bytes", "scldm_vae_train_forward", "scldm_vae_train_backward", "scldm_vae_train_forward_ex", "scldm_vae_train_backward_ex", "scldm_vae_train_set_found_inf", "scldm_vae_train_rows_bytes", "scldm_vae_train_backward_ordered", "scldm_nb_loglik", "scldm_nb_loglik_bwd", "scldm_nb_sample", "scldm_tokenize_expressed", "scldm_csr_count", "scldm_csr_fill", "scldm_mmd_workspace_bytes",
           "scldm_mmd_kernel_sum", "scldm_sinkhorn_workspace_bytes", "scldm_wasserstein_sinkhorn", "scldm_eval_workspace_bytes",
           "scldm_eval_count_metrics", "scldm_log1p_normalize", "scldm_sample_sde", "scldm_sde_noise",
           "scldm_dit_train_workspace_bytes_dx_for", "scldm_dit_train_backward_dx", "scldm_logp_workspace_bytes", "scldm_logp_ode", "scldm_logp_probe",
           "scldm_vae_decode_gaussian", "scldm_vae_decode_gaussian_sample", "scldm_normal_sample", "scldm_gaussian_recon_loss",
           "scldm_vae_train_split",
           "scldm_vae_train_gaussian_forward", "scldm_vae_train_gaussian_backward", "scldm_gaussian_recon_loss_bwd",
           "scldm_dit_infer_workspace_bytes", "scldm_dit_infer_cond_rows", "scldm_dit_infer_forward_rows", "scldm_dit_infer_forward_cfg",
           "scldm_dit_infer_sample_ode",
           "scldm_sample_ode_dopri5_workspace_bytes", "scldm_sample_ode_dopri5", "scldm_sample_ode_dopri5_at", "scldm_dopri5_stage_plan", "scldm_dopri5_control",
           "scldm_dopri5_initial_h0", "scldm_dopri5_initial_step",
           "scldm_logp_ode_dopri5_workspace_bytes", "scldm_logp_ode_dopri5",
           "scldm_transport_coef_at", "scldm_sample_ode_transport", "scldm_fm_plan", "scldm_fm_wloss", "scldm_fm_wloss_bwd", "scldm_fm_prepare_transport", "scldm_fm_wloss_grad",
           "scldm_dit_train_step_transport",
           "scldm_sample_sde_transport", "scldm_logp_transport_workspace_bytes", "scldm_logp_ode_transport", "scldm_sde_coef_at", "scldm_sde_last_coef_at",
           "scldm_scvi_create", "scldm_scvi_destroy", "scldm_scvi_pack", "scldm_scvi_workspace_bytes", "scldm_scvi_encode", "scldm_scvi_decode",
           "scldm_scvi_forward",
           "scldm_scvi_train_record_bytes", "scldm_scvi_train_workspace_bytes", "scldm_scvi_train_forward", "scldm_scvi_train_backward",
           "scldm_scvi_encode_ex", "scldm_scvi_decode_ex", "scldm_scvi_forward_ex",
           "scldm_scvi_train_forward_ex", "scldm_scvi_train_backward_ex", "scldm_scvi_train_set_found_inf",
           "scldm_vaew_create", "scldm_vaew_destroy", "scldm_vaew_load_weights", "scldm_vaew_plan", "scldm_vaew_workspace_bytes",
           "scldm_vaew_encode", "scldm_vaew_decode",
           "scldm_vaew_train_plan", "scldm_vaew_train_workspace_bytes", "scldm_vaew_train_rows_bytes", "scldm_vaew_train_backward"]


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise ScldmError(f"{what} failed (code {rc}): {lib().scldm_last_error().decode()}")


def ptr_array(ptrs):
    """Host array of device pointers (None -> NULL)."""
    arr = (C.c_void_p * max(len(ptrs), 1))()
    for i, p in enumerate(ptrs):
        arr[i] = p
    return arr

"""CPU-side checks of the record-free inference path of shapes outside the fused family (scldm_dit_infer_*): the ABI surface, the
workspace contract and the argument checks, none of which needs a GPU (a wide handle allocates nothing at creation)."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT

ENTRIES = ["scldm_dit_infer_workspace_bytes", "scldm_dit_infer_cond_rows", "scldm_dit_infer_forward_rows", "scldm_dit_infer_forward_cfg",
           "scldm_dit_infer_sample_ode"]


def _wide_handle(n_layer, n_embed=1024, n_head=16, hidden=2732, vocab=(4, 2024)):
    from scldm_amd import _lib
    L = _lib.lib()
    cfg = _lib.DitConfig(n_embed=n_embed, n_embed_input=16, n_layer=n_layer, n_head=n_head, seq_len=16, hidden_dim=hidden, layernorm_eps=1e-8,
                         n_classes=len(vocab), has_null_row=1)
    for i, v in enumerate(vocab):
        cfg.class_vocab[i] = v
    h = C.c_void_p()
    assert L.scldm_dit_create(C.byref(cfg), C.byref(h)) == 0
    return L, h


def test_header_declares_and_library_exports_the_five_entries():
    from scldm_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "scldm_hip.h")).read()
    declared = set(re.findall(r"\b(scldm_[a-z_0-9]+)\s*\(", hdr))
    L = _lib.lib()
    for name in ENTRIES:
        assert name in declared, f"include/scldm_hip.h does not declare {name}"
        assert hasattr(L, name), f"libscldm_hip.so does not export {name}"
        assert name in _lib.EXPORTS
    assert L.scldm_version() == 5


def test_workspace_is_one_layer_whatever_the_depth():
    """The two workspace conditions of the inference path at width 1 024 (DiT-L's): between a 2-layer and a 24-layer handle the
    workspace differs by the conditioning rows' n_rows x mod_width x 4 bytes alone, and at n_fwd 768 / n_rows 16 / n_state 512 it is at
    most three layers' worth of the training record."""
    L2, h2 = _wide_handle(2)
    L, h24 = _wide_handle(24)
    try:
        for n_fwd, n_rows, n_state in [(768, 16, 512), (3, 3, 0), (288, 41, 192), (0, 16, 0)]:
            b2 = L.scldm_dit_infer_workspace_bytes(h2, n_fwd, n_rows, n_state, 1)
            b24 = L.scldm_dit_infer_workspace_bytes(h24, n_fwd, n_rows, n_state, 1)
            assert b2 > 0 and b24 > 0
            # (n_fwd == 0 sizes scldm_dit_infer_cond_rows alone, which writes its rows to the caller's array: no mod block at all)
            mod_bytes = lambda h: (n_rows * L.scldm_dit_mod_width(h) * 4 + 255) // 256 * 256 if n_fwd > 0 else 0
            assert b24 - b2 == mod_bytes(h24) - mod_bytes(h2), (n_fwd, n_rows, n_state, b2, b24)
            for prec in (0, 2, 3):      # every policy carves the same block
                assert L.scldm_dit_infer_workspace_bytes(h24, n_fwd, n_rows, n_state, prec) == b24
        ws = L.scldm_dit_infer_workspace_bytes(h24, 768, 16, 512, 1)
        saved = L.scldm_dit_train_saved_bytes(h24, 768)
        print(f"DiT-L inference workspace at n_fwd 768 / n_rows 16 / n_state 512: {ws / 2**20:.0f} MiB; training record {saved / 2**20:.0f} MiB "
              f"({saved / 24 / 2**20:.0f} MiB per layer)")
        assert ws <= 3 * saved // 24
        assert L.scldm_dit_infer_workspace_bytes(None, 4, 4, 0, 0) == 0
    finally:
        L.scldm_dit_destroy(h2)
        L.scldm_dit_destroy(h24)


def test_rejected_arguments_return_err_shape_without_a_gpu():
    """Every rejection happens before the first HIP call: a wide handle, an empty weight struct and a host buffer as the
    (never touched) workspace are enough to see them."""
    from scldm_amd import _lib
    L, h = _wide_handle(2, n_embed=512, n_head=8, hidden=1368)
    try:
        w = _lib.DitWeights()
        buf = (C.c_char * 256)()
        z = (C.c_float * 512)()
        ws, zp = C.addressof(buf), C.addressof(z)
        masks, scales = (C.c_uint32 * 1)(3), (C.c_float * 1)(1.5)
        ode = lambda z_, steps, method, ws_=ws: L.scldm_dit_infer_sample_ode(h, C.byref(w), z_, None, 0, None, 1, 0, masks, scales, steps, method, 0, ws_, None)
        assert ode(zp, 0, 0) == -1 and b"n_steps" in L.scldm_last_error()
        assert ode(zp, 3, 7) == -1 and b"method" in L.scldm_last_error()
        assert ode(None, 3, 0) == -1 and b"null" in L.scldm_last_error()
        assert ode(zp, 3, 0, None) == -1 and b"null" in L.scldm_last_error()
        assert all(v == 0.0 for v in z)
        assert L.scldm_dit_infer_sample_ode(h, C.byref(w), zp, None, 0, None, 1, 0, masks, scales, 3, 0, 9, ws, None) == -1 and b"precision" in L.scldm_last_error()
        assert L.scldm_dit_infer_forward_cfg(h, C.byref(w), zp, zp, 2, None, 0, None, 1, 0, masks, scales, zp, 0, ws, None) == -1 and b"t_stride" in L.scldm_last_error()
        assert L.scldm_dit_infer_forward_cfg(h, C.byref(w), zp, zp, 1, None, 0, None, 0, 0, masks, scales, zp, 0, ws, None) == -1 and b"B must" in L.scldm_last_error()
        assert L.scldm_dit_infer_forward_rows(h, C.byref(w), zp, 2, 3, 4, zp, None, zp, 0, ws, None) == -1 and b"n_direct" in L.scldm_last_error()
        assert L.scldm_dit_infer_cond_rows(h, C.byref(w), zp, 2, None, 1, zp, 0, ws, None) == -1 and b"t_stride" in L.scldm_last_error()
        # the fused entries keep refusing such a handle
        assert L.scldm_dit_load_weights(h, C.byref(w), None) == -1 and b"fused DiT layer" in L.scldm_last_error()
    finally:
        L.scldm_dit_destroy(h)


def test_python_routing_refuses_cpu_tensors():
    from scldm_amd.nnets import DiT
    m = DiT(n_embed=512, n_embed_input=16, n_layer=1, n_head=8, seq_len=16, dropout=0.0, bias=True, norm_layer="layernorm", multiple_of=4,
            layernorm_eps=1e-8, class_vocab_sizes={"a": 3}, cfg_dropout_prob=0.8).eval()
    assert not m.fused_shape
    lab = {"a": torch.zeros(2, dtype=torch.long)}
    with pytest.raises(RuntimeError, match="CUDA"):
        m(torch.zeros(2, 16, 16), torch.zeros(2), lab)
    with pytest.raises(RuntimeError, match="CUDA"):
        m.forward_with_cfg(torch.zeros(2, 16, 16), torch.zeros(2), lab, {"a": 2.0})
    with pytest.raises(RuntimeError, match="CUDA"):
        m.sample_ode_cfg(torch.zeros(2, 16, 16), lab, {"a": 2.0}, 3, "euler")

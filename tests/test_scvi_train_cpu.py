"""CPU-side checks of ScviVAE training: the train-mode restatement (tests/scvi_train_ref.py) reproduces the reference's fixtures under
autograd, the C entries are declared and refuse bad arguments before any HIP call, the Python switch is off by default and its
refusals are reached without a device.  The kernels themselves are tested in tests/test_gpu_scvi_train.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from scvi_ref import build_scvi, make_inputs, scvi_shapes
from scvi_train_ref import TRAIN_CASES, compare_to_fixture, make_masks, pre_bn_biases, scvi_train_step, train_case

RESTATEMENT_TOL = 1e-5      # the project's restatement gate (scale-relative)
NEW_EXPORTS = ("scldm_scvi_train_record_bytes", "scldm_scvi_train_workspace_bytes", "scldm_scvi_train_forward", "scldm_scvi_train_backward")


@pytest.mark.parametrize("name", sorted(TRAIN_CASES))
def test_restatement_reproduces_the_reference_training_step(name):
    g, sd, masks = train_case(name)
    n_genes, n_hidden, n_latent, n_layers, B, shared, p, seed = TRAIN_CASES[name]
    assert int(g["seed"]) == seed and float(g["dropout"]) == p
    assert list({k: tuple(v.shape) for k, v in sd.items()}.items()) == list(scvi_shapes(n_genes, n_hidden, n_latent, n_layers, shared).items())
    counts, lib, eps = make_inputs(n_genes, n_latent, B, seed)
    assert np.array_equal(counts, g["counts"]) and np.array_equal(lib, g["library_size"]) and np.array_equal(eps, g["eps"])
    want_masks = make_masks(n_layers, B, n_hidden, p, seed)
    assert len(masks) == len(want_masks) == (2 * n_layers if p > 0 else 0) and all(np.array_equal(a, b) for a, b in zip(masks, want_masks))
    out, stats, losses, grads = scvi_train_step(sd, counts, lib, eps, masks, p)
    stat_keys, grad_keys = compare_to_fixture(g, out, stats, losses, grads, RESTATEMENT_TOL, f"{name}: restatement vs reference")
    # nothing is left out: every running statistic, and every trainable parameter but the biases in front of a BatchNorm
    zero = pre_bn_biases(sd)
    assert len(zero) == 2 * n_layers and sorted(stat_keys) == sorted(k for k in sd if "running_" in k)
    assert sorted(grad_keys + zero) == sorted(k for k in sd if sd[k].dtype.is_floating_point and "running_" not in k and not k.startswith("prior."))
    # the fixture exercises both hardtanh clamps and the softplus threshold, and (with dropout) both mask values
    assert np.isclose(g["scale"].min(), np.exp(-7.0), rtol=1e-6) and np.isclose(g["scale"].max(), np.exp(5.0), rtol=1e-6)
    assert "theta_digest" in g or g["theta"].max() > 20
    for m in masks:
        assert m.dtype == np.uint8 and 0.6 < m.mean() < 0.9
    # in float64 the gradient of those biases is zero to roundoff
    _, _, _, g64 = scvi_train_step(sd, counts, lib, eps, masks, p, dtype=torch.float64)
    for k in zero:
        beta = k.rsplit(".", 2)[0] + f".{int(k.rsplit('.', 2)[1]) + 1}.bias"
        assert float(g64[k].abs().max()) < 1e-9 * float(g64[beta].abs().max()), k


def test_switch_is_off_by_default_and_training_refusals_need_no_device():
    import scldm_amd
    from scldm_amd.stochastic_layers import NegativeBinomial
    vae = build_scvi(203, 96, 10, 2, True)
    assert scldm_amd.ScviVAE.train_enabled is False and vae.train_enabled is False and vae.training
    counts, lib = torch.ones(3, 203), torch.full((3,), 203.0)
    with pytest.raises(NotImplementedError, match="no training path"):
        vae(counts, None, lib)
    vae.train_enabled = True
    with pytest.raises(NotImplementedError, match="no training path"):      # encode / decode alone keep refusing
        vae.encode(counts)
    with pytest.raises(NotImplementedError, match="no training path"):
        vae.decode(torch.zeros(3, 10), None, lib)
    with pytest.raises(RuntimeError, match="CUDA"):
        vae(counts, None, lib)
    with pytest.raises(NotImplementedError, match="requires grad"):
        vae(counts.clone().requires_grad_(), None, lib)
    with pytest.raises(ValueError, match="at least two cells"):
        vae(counts[:1], None, lib[:1])
    bn = vae.decoder.decoder_mlp[1]
    bn.momentum = None
    with pytest.raises(NotImplementedError, match="momentum=None"):
        vae(counts, None, lib)
    bn.momentum = 0.2
    with pytest.raises(NotImplementedError, match="one BatchNorm momentum"):
        vae(counts, None, lib)
    bn.momentum = 0.1
    bn.eps = 1e-3
    with pytest.raises(NotImplementedError, match="one eps"):
        vae(counts, None, lib)
    bn.eps = 1e-5
    vae._precision = "fp16"      # the setter refuses it; a module that got there another way is refused as well
    with pytest.raises(NotImplementedError, match="fp32 only"):
        vae(counts, None, lib)
    vae._precision = "fp32"
    vae.eval()                   # eval mode is untouched by the switch
    with pytest.raises(RuntimeError, match="CUDA"):
        vae(counts, None, lib)
    with pytest.raises(RuntimeError, match="CUDA"):
        NegativeBinomial(mu=torch.ones(3, 4), theta=torch.ones(4)).log_prob(torch.ones(3, 4))


def test_abi_declares_the_training_entries_and_refuses_bad_arguments_without_a_gpu():
    from scldm_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "scldm_hip.h")).read()
    declared = set(re.findall(r"\b(scldm_[a-z_0-9]+)\s*\(", hdr))
    L = _lib.lib()
    for name in NEW_EXPORTS:
        assert name in declared and name in _lib.EXPORTS and hasattr(L, name), name
    assert L.scldm_version() == 5 and C.sizeof(_lib.ScviLayer) == 6 * 8 and C.sizeof(_lib.ScviParams) == 10 * 8
    assert C.sizeof(_lib.ScviLayerGrads) == 4 * 8 and C.sizeof(_lib.ScviGrads) == 10 * 8
    err = lambda: L.scldm_last_error().decode()      # noqa: E731
    h = C.c_void_p()
    assert L.scldm_scvi_create(2, 1, 203, 96, 10, 0, 1e-5, C.byref(h)) == 0 and h.value
    try:
        rec, ws_b = L.scldm_scvi_train_record_bytes(h, 5), L.scldm_scvi_train_workspace_bytes(h, 5)
        assert rec > 0 and rec % 256 == 0 and ws_b > 0 and ws_b % 256 == 0
        assert L.scldm_scvi_train_record_bytes(h, 70) > rec and L.scldm_scvi_train_workspace_bytes(h, 70) > ws_b
        for f in (L.scldm_scvi_train_record_bytes, L.scldm_scvi_train_workspace_bytes):
            assert f(h, 1) == 0 and f(None, 5) == 0
        assert rec >= 3 * (2 * 5 * 96 * 4 + 96 * 4) + 5 * 10 * 4          # xhat, h, rstd per layer and the pre-clamp log-scale
        buf = (C.c_char * 4096)()
        base = (C.addressof(buf) + 255) & ~255        # host memory: never dereferenced, a rejected call launches nothing
        p, ws, r = base + 1024, base, base + 512
        masks = (C.c_void_p * 3)(p, p, p)
        no_masks = (C.c_void_p * 3)(p, None, p)

        def fwd(hh=h, counts=p, lib=p, n_lib=5, B=5, eps=p, p_enc=0.0, p_dec=0.0, m=masks, mom=0.1, record=r, loc=p, theta=p, w=ws):
            return L.scldm_scvi_train_forward(hh, counts, lib, n_lib, B, eps, p_enc, p_dec, 3, m, 0, mom, record, loc, p, p, p, theta, w, None)
        assert fwd(hh=None) == -1 and "handle" in err()
        assert fwd(B=1, n_lib=1) == -1 and "B >= 2" in err()
        assert fwd(n_lib=4) == -1 and "library_size has 4 entries for 5 cells" in err()
        assert fwd(counts=None) == -1 and "counts is NULL" in err()
        assert fwd(counts=p + 2) == -1 and "aligned" in err()
        assert fwd(eps=None) == -1 and "eps is NULL" in err()
        assert fwd(loc=None) == -1 and "loc is NULL" in err()
        assert fwd(theta=None) == -1 and "theta is NULL" in err()
        assert fwd(w=None) == -1 and "ws is NULL" in err()
        assert fwd(w=ws + 64) == -1 and "256-byte" in err()
        assert fwd(record=None) == -1 and "record is NULL" in err()
        assert fwd(record=r + 4) == -1 and "record is not 256-byte" in err()
        assert fwd(p_enc=1.0) == -1 and "[0, 1)" in err()
        assert fwd(p_dec=-0.5) == -1 and "[0, 1)" in err()
        assert fwd(mom=1.5) == -1 and "momentum" in err()
        assert fwd(p_enc=0.25, m=None) == -1 and "masks is NULL" in err()
        assert fwd(p_enc=0.25, m=no_masks) == -1 and "encoder layer 1" in err()
        assert fwd(p_dec=0.25, m=no_masks) == -3                           # the decoder's only mask is there: next stop, the pack check
        assert fwd() == -3 and "scldm_scvi_pack" in err()                  # a well-formed call before pack is a state error, not a launch

        lg = _lib.ScviLayerGrads(p, p, p, p)
        ea, da = (_lib.ScviLayerGrads * 2)(lg, lg), (_lib.ScviLayerGrads * 1)(lg)
        grads = _lib.ScviGrads(ea, da, p, p, p, p, p, p, p, p)

        def bwd(hh=h, B=5, n_lib=5, scale=p, z=p, mu=p, dmu=p, dz=None, g=grads, record=r, w=ws, p_enc=0.0, m=masks):
            return L.scldm_scvi_train_backward(hh, p, p, n_lib, B, p, p_enc, 0.0, m, record, scale, z, mu, p, dmu, None, None, None, dz,
                                               C.byref(g) if g is not None else None, w, None)
        assert bwd(hh=None) == -1 and "handle" in err()
        assert bwd(B=1, n_lib=1) == -1 and "B >= 2" in err()
        assert bwd(n_lib=6) == -1 and "library_size" in err()
        assert bwd(scale=None) == -1 and "scale is NULL" in err()
        assert bwd(z=None) == -1 and "z is NULL" in err()
        assert bwd(mu=p + 1) == -1 and "aligned" in err()
        assert bwd(dmu=p + 2) == -1 and "dmu is not 4-byte aligned" in err()
        assert bwd(dz=p + 2) == -1 and "dz is not 4-byte aligned" in err()
        assert bwd(record=None) == -1 and "record is NULL" in err()
        assert bwd(w=ws + 128) == -1 and "256-byte" in err()
        assert bwd(p_enc=0.5, m=None) == -1 and "masks is NULL" in err()
        assert bwd(g=None) == -1 and "grads is NULL" in err()
        bad = (_lib.ScviLayerGrads * 2)(lg, _lib.ScviLayerGrads(p, p, None, p))
        assert bwd(g=_lib.ScviGrads(bad, da, p, p, p, p, p, p, p, p)) == -1 and "encoder layer 1" in err()
        assert bwd(g=_lib.ScviGrads(ea, da, p, p, p, p, p, None, p, p)) == -1 and "mu_b is NULL" in err()
        assert bwd(g=_lib.ScviGrads(ea, da, p, p, p, p, p, p, p, None)) == -1 and "theta_b is NULL" in err()   # unshared theta
        assert bwd(dmu=None) == -3 and "scldm_scvi_pack" in err()          # every upstream gradient may be NULL
    finally:
        L.scldm_scvi_destroy(h)

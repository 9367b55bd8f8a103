"""CPU-side checks of the scVI-style baseline (ScviVAE): the restatement (tests/scvi_ref.py) reproduces the reference's golden
vectors, the Python mirror keeps the reference's state_dict, the C entries refuse bad arguments before any HIP call, and the Python
classes refuse CPU tensors and training mode.  The kernels themselves are tested in tests/test_gpu_scvi.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, golden_json, load_golden, max_abs_rel
from scvi_ref import CASES, OUTPUTS, build_scvi, make_inputs, make_scvi_state_dict, scvi_forward, scvi_shapes

RESTATEMENT_TOL = 1e-5      # the project's restatement gate (scale-relative)
NEW_EXPORTS = ("scldm_scvi_create", "scldm_scvi_destroy", "scldm_scvi_pack", "scldm_scvi_workspace_bytes", "scldm_scvi_encode",
               "scldm_scvi_decode", "scldm_scvi_forward")


def golden_case(name):
    g = load_golden(name)
    shapes = {k: tuple(v) for k, v in golden_json(g, "shapes_json").items()}
    return g, shapes, make_scvi_state_dict(shapes, int(g["seed"]))


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_reproduces_the_reference_golden(name):
    g, shapes, sd = golden_case(name)
    n_genes, n_hidden, n_latent, n_layers, B, shared, seed = CASES[name]
    assert int(g["seed"]) == seed and list(shapes.items()) == list(scvi_shapes(n_genes, n_hidden, n_latent, n_layers, shared).items())
    counts, lib, eps = make_inputs(n_genes, n_latent, B, seed)
    assert np.array_equal(counts, g["counts"]) and np.array_equal(lib, g["library_size"]) and np.array_equal(eps, g["eps"])
    assert g["counts"].shape == (B, n_genes) and np.array_equal(g["library_size"], g["counts"].sum(1))
    t = torch.from_numpy
    out = scvi_forward(sd, t(g["counts"]), t(g["library_size"]), t(g["eps"]))
    errs = {k: max_abs_rel(out[k], g[k]) for k in OUTPUTS}
    print(f"[parity] {name}: restatement vs reference  " + "  ".join(f"{k} {e:.3e}" for k, e in errs.items()) + f"  (gate {RESTATEMENT_TOL:g})")
    for k in OUTPUTS:
        assert out[k].shape == g[k].shape and errs[k] <= RESTATEMENT_TOL, (k, errs[k])
    assert g["theta"].shape == ((n_genes,) if shared else (B, n_genes))
    assert np.abs(g["mu"].sum(1) / g["library_size"] - 1).max() < 1e-5
    # the fixture exercises both hardtanh clamps and the softplus threshold, and depends on the BatchNorm statistics
    assert np.isclose(g["scale"].min(), np.exp(-7.0), rtol=1e-6) and np.isclose(g["scale"].max(), np.exp(5.0), rtol=1e-6)
    assert g["theta"].max() > 20
    plain = {k: (torch.zeros_like(v) if k.endswith("running_mean") else torch.ones_like(v) if k.endswith("running_var") else v)
             for k, v in sd.items()}
    assert max_abs_rel(scvi_forward(plain, t(g["counts"]), t(g["library_size"]), t(g["eps"]))["h"], g["h"]) > 1e-2


@pytest.mark.parametrize("name", ["scvi_small", "scvi_small_unshared"])
def test_classes_keep_the_reference_state_dict_and_load_it_strictly(name):
    g, shapes, sd = golden_case(name)
    n_genes, n_hidden, n_latent, n_layers, B, shared, seed = CASES[name]
    vae = build_scvi(n_genes, n_hidden, n_latent, n_layers, shared)
    ours = vae.state_dict()
    assert list(ours) == list(shapes) and {k: tuple(v.shape) for k, v in ours.items()} == shapes
    assert ours["encoder.encoder_mlp.1.num_batches_tracked"].dtype == torch.int64
    vae.load_state_dict(sd, strict=True)
    back = vae.state_dict()
    for k, v in sd.items():
        assert back[k].dtype == v.dtype and torch.equal(back[k], v), k
    assert not vae.prior.loc.requires_grad and vae.prior.loc.shape == (1, n_latent) and float(vae.prior.scale.min()) == 1.0
    assert vae.encoder.latent_embedding == 0 and vae.decoder.last_embedding is None
    assert isinstance(vae.decoder_head.theta, torch.nn.Parameter) == shared
    with pytest.raises(RuntimeError, match="Unexpected key"):
        vae.load_state_dict({**sd, "encoder.encoder_mlp.9.weight": torch.zeros(1)}, strict=True)


def test_standard_prior_holds_frozen_parameters_and_is_a_standard_normal():
    from scldm_amd.priors import StandardPrior
    for n_embed, shape in ((0, (1, 10)), (3, (1, 10, 3))):
        prior = StandardPrior(10, n_embed)
        assert list(prior.state_dict()) == ["loc", "scale"] and prior.loc.shape == shape and prior.scale.shape == shape
        assert not any(p.requires_grad for p in prior.parameters())
        assert float(prior.loc.abs().max()) == 0.0 and float((prior.scale - 1).abs().max()) == 0.0
        x = torch.linspace(-3, 3, 7 * 10 * max(n_embed, 1)).reshape((7,) + shape[1:])
        want = torch.distributions.Normal(torch.zeros(shape), torch.ones(shape)).log_prob(x)
        assert torch.allclose(prior.log_prob(x), want, rtol=0, atol=1e-6) and torch.equal(prior.loss(x), prior.log_prob(x))
        torch.manual_seed(0)
        s = prior.sample(4000)
        assert s.shape == (4000,) + shape[1:] and abs(float(s.mean())) < 0.05 and abs(float(s.std()) - 1) < 0.05
        d = prior()
        assert isinstance(d, torch.distributions.Normal) and d.loc.shape == shape
    with pytest.raises(ValueError, match="n_latent"):
        StandardPrior(0, 0)


def test_python_classes_refuse_cpu_tensors_training_mode_and_other_precisions():
    import scldm_amd
    vae = build_scvi(203, 96, 10, 2, True)
    assert scldm_amd.ScviVAE is type(vae)
    counts, lib = torch.ones(3, 203), torch.full((3,), 203.0)
    with pytest.raises(NotImplementedError, match="no training path"):          # a fresh module is in training mode
        vae(counts, None, lib)
    with pytest.raises(NotImplementedError, match="dropout=0.1"):
        vae.encode(counts)
    vae.eval()
    for call in (lambda: vae(counts, None, lib), lambda: vae.encode(counts), lambda: vae.decode(torch.zeros(3, 10), None, lib)):
        with pytest.raises(RuntimeError, match="CUDA"):
            call()
    with pytest.raises(NotImplementedError, match="requires grad"):
        vae(counts.clone().requires_grad_(), None, lib)
    with pytest.raises(NotImplementedError, match="requires grad"):
        vae.decode(torch.zeros(3, 10, requires_grad=True), None, lib)
    assert vae.precision == "fp32"
    with pytest.raises(NotImplementedError, match="fp32 only"):
        vae.precision = "fp16"
    vae.precision = "fp32"
    with pytest.raises(RuntimeError, match="fused"):
        vae.encoder(counts)
    from scldm_amd.nnets import EncoderScvi
    with pytest.raises(ValueError, match="n_layers"):
        EncoderScvi(10, 4, 0, 0.0)


def test_abi_declares_the_scvi_entries_and_refuses_bad_arguments_without_a_gpu():
    from scldm_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "scldm_hip.h")).read()
    declared = set(re.findall(r"\b(scldm_[a-z_0-9]+)\s*\(", hdr))
    L = _lib.lib()
    for name in NEW_EXPORTS:
        assert name in declared and name in _lib.EXPORTS and hasattr(L, name), name
    assert L.scldm_version() == 5 and C.sizeof(_lib.ScviLayer) == 6 * 8 and C.sizeof(_lib.ScviParams) == 10 * 8
    err = lambda: L.scldm_last_error().decode()      # noqa: E731
    h = C.c_void_p()
    # create: layer counts, dimensions, eps
    for args, word in (((0, 1, 8, 4, 2, 1, 1e-5), "n_layers"), ((1, 0, 8, 4, 2, 1, 1e-5), "n_layers"), ((9, 1, 8, 4, 2, 1, 1e-5), "at most"),
                       ((1, 1, 0, 4, 2, 1, 1e-5), "positive"), ((1, 1, 8, -1, 2, 1, 1e-5), "positive"), ((1, 1, 8, 4, 0, 1, 1e-5), "positive"),
                       ((1, 1, 8, 4, 2, 1, -1.0), "eps")):
        assert L.scldm_scvi_create(*args, C.byref(h)) == -1 and word in err() and not h.value, (args, err())
    assert L.scldm_scvi_create(1, 1, 8, 4, 2, 1, 1e-5, None) == -1
    assert L.scldm_scvi_create(2, 1, 203, 96, 10, 0, 1e-5, C.byref(h)) == 0 and h.value      # allocates nothing on the device
    try:
        ws_bytes = L.scldm_scvi_workspace_bytes(h, 5)
        assert ws_bytes > 0 and ws_bytes % 256 == 0 and L.scldm_scvi_workspace_bytes(h, 0) == 0 and L.scldm_scvi_workspace_bytes(None, 5) == 0
        assert L.scldm_scvi_workspace_bytes(h, 70) > ws_bytes
        buf = (C.c_char * 4096)()
        base = (C.addressof(buf) + 255) & ~255        # host memory: never dereferenced, a rejected call launches nothing
        p, ws = base + 1024, base
        # encode
        assert L.scldm_scvi_encode(None, p, 5, None, p, p, p, None, ws, None) == -1 and "handle" in err()
        assert L.scldm_scvi_encode(h, p, 0, None, p, p, p, None, ws, None) == -1 and "B >= 1" in err()
        assert L.scldm_scvi_encode(h, None, 5, None, p, p, p, None, ws, None) == -1 and "counts is NULL" in err()
        assert L.scldm_scvi_encode(h, p, 5, None, p, None, p, None, ws, None) == -1 and "loc is NULL" in err()
        assert L.scldm_scvi_encode(h, p + 2, 5, None, p, p, p, None, ws, None) == -1 and "aligned" in err()
        assert L.scldm_scvi_encode(h, p, 5, p, p, p, p, None, ws, None) == -1 and "z is NULL" in err()
        assert L.scldm_scvi_encode(h, p, 5, None, p, p, p, None, None, None) == -1 and "ws is NULL" in err()
        assert L.scldm_scvi_encode(h, p, 5, None, p, p, p, None, ws + 64, None) == -1 and "256-byte" in err()
        # decode: the library-size array has one entry per cell
        assert L.scldm_scvi_decode(h, p, p, 4, 5, p, p, ws, None) == -1 and "library_size has 4 entries for 5 cells" in err()
        assert L.scldm_scvi_decode(h, p, None, 5, 5, p, p, ws, None) == -1 and "library is NULL" in err()
        assert L.scldm_scvi_decode(h, p, p, 5, 5, p + 1, p, ws, None) == -1 and "aligned" in err()
        assert L.scldm_scvi_decode(h, p, p, 5, 5, p, None, ws, None) == -1 and "theta is NULL" in err()
        # forward: eps is always a given array
        assert L.scldm_scvi_forward(h, p, p, 5, 5, None, p, p, p, p, p, p, ws, None) == -1 and "eps is NULL" in err()
        assert L.scldm_scvi_forward(h, p, p, 6, 5, p, p, p, p, p, p, p, ws, None) == -1 and "library_size" in err()
        # pack: every pointer of the tables is checked before the first HIP call
        assert L.scldm_scvi_pack(h, None, None) == -1 and L.scldm_scvi_pack(None, None, None) == -1
        lay = _lib.ScviLayer(w=p, b=p, bn_w=p, bn_b=p, bn_mean=p, bn_var=None)
        ea, da = (_lib.ScviLayer * 2)(lay, lay), (_lib.ScviLayer * 1)(lay)
        prm = _lib.ScviParams(enc=ea, dec=da, loc_w=p, loc_b=p, scale_w=p, scale_b=p, mu_w=p, mu_b=p, theta_w=p, theta_b=p)
        assert L.scldm_scvi_pack(h, C.byref(prm), None) == -1 and "encoder layer 0" in err()
        ok = _lib.ScviLayer(w=p, b=p, bn_w=p, bn_b=p, bn_mean=p, bn_var=p)
        ea, da = (_lib.ScviLayer * 2)(ok, ok), (_lib.ScviLayer * 1)(ok)
        prm = _lib.ScviParams(enc=ea, dec=da, loc_w=p, loc_b=p, scale_w=p, scale_b=p, mu_w=p, mu_b=p, theta_w=p, theta_b=None)
        assert L.scldm_scvi_pack(h, C.byref(prm), None) == -1 and "theta_b is NULL" in err()      # unshared theta needs its bias
        # a well-formed call before pack is a state error, not a launch
        assert L.scldm_scvi_encode(h, p, 5, None, p, p, p, None, ws, None) == -3 and "scldm_scvi_pack" in err()
    finally:
        L.scldm_scvi_destroy(h)
    L.scldm_scvi_destroy(None)

"""CPU-side checks of the Gaussian decoder head: the restatement (tests/gauss_head_ref.py on top of oracle.vae.decoder) reproduces the
reference's golden vectors, the Python mirror keeps the reference's state_dict, and the C ABI declares and exports the new entry
points.  The kernels themselves are tested in tests/test_gpu_gauss_head.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, golden_json, load_golden, max_abs_rel
from gauss_head_ref import CASES, decode_gaussian, recon_loss_rows
from oracle.vae import VAEConfig, encode
from oracle.weights import make_state_dict

RESTATEMENT_TOL = 1e-5      # the project's restatement gate (scale-relative)
NEW_EXPORTS = ("scldm_vae_decode_gaussian", "scldm_vae_decode_gaussian_sample", "scldm_normal_sample", "scldm_gaussian_recon_loss")


def build_gauss_vae(n_genes):
    from scldm_amd.layers import InputTransformerVAE
    from scldm_amd.nnets import Decoder, Encoder
    from scldm_amd.stochastic_layers import GaussianTransformerLayer
    from scldm_amd.vae import TransformerVAE
    enc = Encoder(n_layer=8, n_inducing_points=16, n_embed=32, n_embed_latent=16, n_head=8, n_head_cross=4, dropout=0.0, bias=False,
                  multiple_of=4, layernorm_eps=1e-8, norm_layer="layernorm", positional_encoding=True)
    dec = Decoder(n_genes=n_genes, n_embed=32, n_embed_latent=16, n_head=8, n_head_cross=4, n_layer=8, n_inducing_points=16,
                  dropout=0.0, bias=False, multiple_of=4, layernorm_eps=1e-8, norm_layer="layernorm", shared_embedding=True,
                  use_adaln=False)
    head = GaussianTransformerLayer(n_embed=32, norm_layer="layernorm", layernorm_eps=1e-8)
    inp = InputTransformerVAE(n_genes=n_genes, n_embed=32, agg_func="log1p")
    return TransformerVAE(encoder=enc, decoder=dec, decoder_head=head, input_layer=inp)


def golden_case(name):
    g = load_golden(name)
    shapes = {k: tuple(v) for k, v in golden_json(g, "shapes_json").items()}
    return g, shapes, make_state_dict(shapes, int(g["seed"])), VAEConfig(n_genes=int(g["n_genes"]))


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_reproduces_the_reference_golden(name):
    g, shapes, sd, cfg = golden_case(name)
    n_genes, G, S, B, seed = CASES[name]
    assert (int(g["n_genes"]), g["genes"].shape, g["genes_subset"].shape, int(g["seed"])) == (n_genes, (B, G), (B, S), seed)
    t = torch.from_numpy
    z = encode(sd, cfg, t(g["counts_subset"]), t(g["genes_subset"]))
    assert max_abs_rel(z, g["z"]) < RESTATEMENT_TOL
    mu = decode_gaussian(sd, cfg, t(g["z"]), t(g["genes"]))
    mu_rand = decode_gaussian(sd, cfg, t(g["zrand"]), t(g["genes"]))
    e_mu, e_rand = max_abs_rel(mu, g["mu"]), max_abs_rel(mu_rand, g["mu_rand"])
    loss = recon_loss_rows(g["counts"], g["mu"])
    e_loss = max_abs_rel(loss, g["loss_rows"])
    print(f"[parity] {name}: restatement vs reference  mu {e_mu:.3e}  mu_rand {e_rand:.3e}  loss_rows {e_loss:.3e}  (gate {RESTATEMENT_TOL:g})")
    assert mu.shape == g["mu"].shape and e_mu <= RESTATEMENT_TOL and e_rand <= RESTATEMENT_TOL and e_loss <= RESTATEMENT_TOL
    assert float(np.std(g["mu"])) > 0 and float(np.abs(g["mu"] - g["mu_rand"]).max()) > 0      # the fixture depends on genes and latents


def test_class_keeps_the_reference_state_dict():
    from scldm_amd.stochastic_layers import GaussianTransformerLayer
    g, shapes, sd, cfg = golden_case("gauss_small")
    head = GaussianTransformerLayer(n_embed=32, norm_layer="layernorm", layernorm_eps=1e-8)
    ours = {f"decoder_head.{k}": tuple(v.shape) for k, v in head.state_dict().items()}
    assert ours == {k: v for k, v in shapes.items() if k.startswith("decoder_head.")}
    assert ours == {"decoder_head.ln.weight": (32,), "decoder_head.ln.bias": (32,), "decoder_head.params.weight": (1, 32),
                    "decoder_head.params.bias": (1,)}
    assert head.__class__.__name__ == "GaussianTransformerLayer" and head.ln.eps == 1e-8
    with pytest.raises(ValueError, match="n_embed"):
        GaussianTransformerLayer()


def test_vae_with_the_gaussian_head_loads_the_checkpoint_strictly():
    g, shapes, sd, cfg = golden_case("gauss_small")
    vae = build_gauss_vae(int(g["n_genes"]))
    assert {k: tuple(v.shape) for k, v in vae.state_dict().items()} == shapes
    vae.load_state_dict(sd, strict=True)
    assert vae.gaussian_head
    with pytest.raises(RuntimeError, match="CUDA"):         # no CPU path, and the head's missing .t / .theta are not what stops it
        vae.decode(torch.zeros(1, 16, 16), torch.zeros(1, 4, dtype=torch.long), torch.ones(1, 1))
    from test_abi_cpu import _build_vae
    assert not _build_vae(5).gaussian_head


def test_normal_holder_and_losses_have_no_cpu_kernel_path():
    from scldm_amd.distributions import gaussian_recon_loss, log_gaussian
    from scldm_amd.evaluations import reconstruction_metrics
    from scldm_amd.stochastic_layers import Normal
    mu = torch.full((4, 3), 0.5)
    d = Normal(mu, 1.0)
    assert isinstance(d, torch.distributions.Normal) and torch.equal(d.mu, mu) and torch.equal(d.scale, torch.ones(4, 3))
    assert torch.equal(d.mean, mu)
    with pytest.raises(RuntimeError, match="CUDA"):
        d.sample()
    x = torch.arange(12.0).reshape(4, 3)
    assert torch.equal(log_gaussian(x, mu), (x - mu) ** 2)                                   # distributions.py:58-59
    s = torch.full((4, 3), 2.0)
    assert torch.allclose(log_gaussian(x, mu, s), 0.5 * ((x - mu) / (s + 1e-8)) ** 2 + torch.log(s + 1e-8))
    with pytest.raises(RuntimeError, match="no CPU"):
        gaussian_recon_loss(x, mu)
    with pytest.raises(ValueError, match="head"):
        reconstruction_metrics(mu, x, head="poisson")


def test_abi_declares_the_gaussian_entry_points():
    from scldm_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "scldm_hip.h")).read()
    declared = set(re.findall(r"\b(scldm_[a-z_0-9]+)\s*\(", hdr))
    L = _lib.lib()
    for name in NEW_EXPORTS:
        assert name in declared and name in _lib.EXPORTS and hasattr(L, name), name
    # the two appended fields sit at the END of scldm_vae_weights: every earlier offset is where it was
    fields = [f[0] for f in _lib.VaeWeights._fields_]
    assert fields[-2:] == ["head_ln_w", "head_ln_b"] and fields[:8] == ["gene_embedding", "inducing_points", "enc_pos_embed", "enc_latent_w",
                                                                        "dec_latent_w", "theta", "head_w", "head_b"]
    assert _lib.VaeWeights.dec_blocks.offset == 8 * 8 + 2 * 12 * 8 + 8 and _lib.VaeWeights.head_ln_w.offset == _lib.VaeWeights.dec_blocks.offset + 8
    assert C.sizeof(_lib.VaeWeights) == _lib.VaeWeights.head_ln_b.offset + 8 and L.scldm_version() == 5
    # argument validation needs no GPU: nothing is launched for a rejected call
    assert L.scldm_normal_sample(None, None, 4, 0, None) == -1 and L.scldm_gaussian_recon_loss(None, None, 1, 1, 1e4, None, None) == -1
    assert L.scldm_vae_decode_gaussian(None, None, None, 1, 1, None, 0, None, None) == -1
    assert L.scldm_vae_decode_gaussian_sample(None, None, None, 1, 1, None, 0, 0, None, None) == -1

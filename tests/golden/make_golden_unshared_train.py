#!/usr/bin/env python3
"""Generate the unshared-theta NB head TRAINING fixtures by RUNNING THE REFERENCE (build container only; see make_golden.py for the
import stubs).

Run from the repo root:   python tests/golden/make_golden_unshared_train.py

tests/golden/vae_train_unshared_<case>.npz: the reference's own `TransformerVAE` with
`NegativeBinomialTransformerLayer(shared_theta=False)` (decoder_name negative_binomial_unshared_theta, vae_base.yaml:71-77) in train
mode, `VAE.loss = -log_nb_positive(counts, mu, theta).sum(1).mean()` (src/scldm/models.py:231-249) and the reference's own autograd
gradient of every parameter as digests (make_golden.grad_digest), in the layout of make_golden.gen_vae_train.  Inputs are drawn as
gen_vae_train draws them, with seeds of their own.  Only data is stored; the weights are rebuilt from
`oracle.weights.make_state_dict(shapes, seed)`."""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (installs the import stubs and puts the repo root on sys.path)
from scldm.distributions import log_nb_positive  # noqa: E402

# name: (n_genes, G, S, B, seed)
CASES = {"vae_train_unshared_small": (60, 50, 20, 3, 231), "vae_train_unshared_2000": (2000, 2000, 700, 2, 232)}


def gen_unshared_train(name, n_genes, G, S, B, seed):
    enc = mg.Encoder(n_layer=8, n_inducing_points=16, n_embed=32, n_embed_latent=16, n_head=8, n_head_cross=4, dropout=0.0,
                     bias=False, multiple_of=4, layernorm_eps=1e-8, norm_layer="layernorm", positional_encoding=True)
    dec = mg.Decoder(n_genes=n_genes, n_embed=32, n_embed_latent=16, n_head=8, n_head_cross=4, n_layer=8, n_inducing_points=16,
                     dropout=0.0, bias=False, multiple_of=4, layernorm_eps=1e-8, norm_layer="layernorm", shared_embedding=True,
                     use_adaln=False)
    head = mg.NegativeBinomialTransformerLayer(n_genes=n_genes, shared_theta=False, n_embed=32, norm_layer="layernorm",
                                               layernorm_eps=1e-8)
    inp = mg.InputTransformerVAE(n_genes=n_genes, n_embed=32, agg_func="log1p")
    vae = mg.TransformerVAE(encoder=enc, decoder=dec, decoder_head=head, input_layer=inp)
    shapes = mg.shapes_of(vae)
    assert "decoder_head.theta.weight" not in shapes and tuple(shapes["decoder_head.params.weight"]) == (2, 32)
    vae.load_state_dict(mg.make_state_dict(shapes, seed), strict=True)
    vae.train()
    rng = np.random.default_rng(seed + 1000)
    genes = np.stack([rng.permutation(n_genes)[:G] for _ in range(B)]).astype(np.int64)
    counts = rng.poisson(0.7, (B, G)).astype(np.float32)
    sub = np.stack([np.sort(rng.permutation(G)[:S]) for _ in range(B)])
    genes_subset = np.take_along_axis(genes, sub, 1)
    counts_subset = np.take_along_axis(counts, sub, 1)
    lib = counts.sum(1, keepdims=True).astype(np.float32) + 1.0
    t = torch.from_numpy
    params, z = vae(t(counts), t(genes), t(lib), t(counts_subset), t(genes_subset))
    assert set(params) == {"mu", "theta"} and params["theta"].shape == (B, G)
    recon = -log_nb_positive(t(counts), params["mu"], params["theta"])
    loss = recon.sum(dim=1).mean()
    loss.backward()
    out = {"shapes_json": np.array(json.dumps({k: list(v) for k, v in shapes.items()})), "seed": np.array(seed), "n_genes": np.array(n_genes),
           "genes": genes, "counts": counts, "genes_subset": genes_subset, "counts_subset": counts_subset, "library_size": lib,
           "loss": np.array(float(loss.detach())), "recon_row": recon.sum(dim=1).detach().numpy(), "z": z.detach().numpy(),
           "mu": params["mu"].detach().numpy(), "theta": params["theta"].detach().numpy()}
    frozen = []
    for k, p in vae.named_parameters():
        if p.grad is None:
            frozen.append(k)
            continue
        out[f"grad_{k}"] = mg.grad_digest(p.grad.numpy())
    out["frozen_json"] = np.array(json.dumps(frozen))
    np.savez_compressed(os.path.join(HERE, f"{name}.npz"), **out)
    print(name, "loss", float(loss.detach()), "frozen", frozen, "n grads", sum(k.startswith("grad_") for k in out),
          "d head bias", vae.decoder_head.params.bias.grad.tolist())


if __name__ == "__main__":
    for name, case in CASES.items():
        gen_unshared_train(name, *case)

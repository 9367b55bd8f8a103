#!/usr/bin/env python3
"""Generate the wide TransformerVAE fixtures by RUNNING THE REFERENCE (build container only; see make_golden.py for the import stubs).

Run from the repo root:   python tests/golden/make_golden_vae_wide.py

tests/golden/vae_wide_<n_embed>.npz (tests/vae_wide_cases.py: CASES): the reference's own `TransformerVAE` at four shapes outside
vae_base.yaml - `encode`, `decode` on the encoded and on random latents, and `forward`.  Inputs are drawn as make_golden.gen_vae draws
them.  Only data is stored; the weights are rebuilt from `oracle.weights.make_state_dict(shapes, seed)`.  Running the script twice gives
identical bytes."""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402  (installs the import stubs and puts the repo root on sys.path)

import vae_wide_cases  # noqa: E402


def gen_wide(name, c):
    ek, dk, hk, ik = vae_wide_cases.module_kwargs(c)
    vae = mg.TransformerVAE(encoder=mg.Encoder(**ek), decoder=mg.Decoder(**dk), decoder_head=mg.NegativeBinomialTransformerLayer(**hk),
                            input_layer=mg.InputTransformerVAE(**ik))
    shapes = mg.shapes_of(vae)
    seed, n_genes, G, S, B = c["seed"], c["n_genes"], c["G"], c["S"], c["B"]
    vae.load_state_dict(mg.make_state_dict(shapes, seed), strict=True)
    vae.eval()
    assert vae.encoder.ca_layer.mlp.w1.weight.shape[0] == vae_wide_cases.HIDDEN[name]
    rng = np.random.default_rng(seed + 1000)
    genes = np.stack([rng.permutation(n_genes)[:G] for _ in range(B)]).astype(np.int64)
    counts = rng.poisson(0.7, (B, G)).astype(np.float32)
    sub = np.stack([np.sort(rng.permutation(G)[:S]) for _ in range(B)])
    genes_subset = np.take_along_axis(genes, sub, 1)
    counts_subset = np.take_along_axis(counts, sub, 1)
    lib = counts.sum(1, keepdims=True).astype(np.float32) + 1.0
    t = torch.from_numpy
    with torch.no_grad():
        z = vae.encode(t(counts), t(genes), t(counts_subset), t(genes_subset))
        nb = vae.decode(z, t(genes), t(lib))
        zrand = t(rng.standard_normal((B, c["n_inducing"], c["n_embed_latent"])).astype(np.float32))
        nb2 = vae.decode(zrand, t(genes), t(lib))
        params, z_fwd = vae(t(counts), t(genes), t(lib), t(counts_subset), t(genes_subset))
        assert torch.equal(params["mu"], nb.mu) and torch.equal(params["theta"], nb.theta) and torch.equal(z_fwd, z)
    assert all(bool(torch.isfinite(x).all()) for x in (z, nb.mu, nb.theta, nb2.mu))
    np.savez_compressed(os.path.join(HERE, f"{name}.npz"),
                        shapes_json=np.array(json.dumps({k: list(v) for k, v in shapes.items()})), seed=np.array(seed),
                        n_genes=np.array(n_genes), genes=genes, counts=counts, genes_subset=genes_subset,
                        counts_subset=counts_subset, library_size=lib, z=z.numpy(), mu=nb.mu.numpy(), theta=nb.theta.numpy(),
                        zrand=zrand.numpy(), mu_rand=nb2.mu.numpy())
    print(name, "z absmax", float(z.abs().max()), "mu rowsum", nb.mu.sum(1).numpy(), "lib", lib[:, 0], "theta range",
          float(nb.theta.min()), float(nb.theta.max()))


if __name__ == "__main__":
    for name, case in vae_wide_cases.CASES.items():
        gen_wide(name, case)

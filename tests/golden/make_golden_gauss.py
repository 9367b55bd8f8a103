#!/usr/bin/env python3
"""Generate the Gaussian-head fixtures by RUNNING THE REFERENCE (build container only; see make_golden.py for the import stubs).

Run from the repo root:   python tests/golden/make_golden_gauss.py

tests/golden/gauss_<case>.npz: the reference's own `TransformerVAE` with `GaussianTransformerLayer` as decoder head
(`decoder_name: gaussian`, experiments/configs/model/vae_base.yaml:81-85) - `encode`, `decode(...).loc` on the encoded and on random
latents - and the reconstruction loss per cell as `VAE.loss` forms it (src/scldm/models.py:239-245):
`log_gaussian(log1p(counts / rowsum * 1e4), mu).sum(1)`.  Inputs are drawn as make_golden.gen_vae draws them.  Only data is stored;
the weights are rebuilt from `oracle.weights.make_state_dict(shapes, seed)`.  Running the script twice gives identical bytes."""
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
from scldm.distributions import log_gaussian  # noqa: E402
from scldm.stochastic_layers import GaussianTransformerLayer  # noqa: E402

import gauss_head_ref  # noqa: E402


def gen_gauss(name, n_genes, G, S, B, seed):
    enc = mg.Encoder(n_layer=8, n_inducing_points=16, n_embed=32, n_embed_latent=16, n_head=8, n_head_cross=4, dropout=0.0,
                     bias=False, multiple_of=4, layernorm_eps=1e-8, norm_layer="layernorm", positional_encoding=True)
    dec = mg.Decoder(n_genes=n_genes, n_embed=32, n_embed_latent=16, n_head=8, n_head_cross=4, n_layer=8, n_inducing_points=16,
                     dropout=0.0, bias=False, multiple_of=4, layernorm_eps=1e-8, norm_layer="layernorm", shared_embedding=True,
                     use_adaln=False)
    head = GaussianTransformerLayer(n_embed=32, norm_layer="layernorm", layernorm_eps=1e-8)
    inp = mg.InputTransformerVAE(n_genes=n_genes, n_embed=32, agg_func="log1p")
    vae = mg.TransformerVAE(encoder=enc, decoder=dec, decoder_head=head, input_layer=inp)
    shapes = mg.shapes_of(vae)
    vae.load_state_dict(mg.make_state_dict(shapes, seed), strict=True)
    vae.eval()
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
        d = vae.decode(z, t(genes), t(lib))
        assert type(d).__name__ == "Normal" and bool((d.scale == 1).all())
        zrand = t(rng.standard_normal((B, 16, 16)).astype(np.float32))
        d2 = vae.decode(zrand, t(genes), t(lib))
        params, z_fwd = vae(t(counts), t(genes), t(lib), t(counts_subset), t(genes_subset))
        assert set(params) == {"mu"} and torch.equal(params["mu"], d.loc) and torch.equal(z_fwd, z)
        y = torch.log1p((t(counts) / t(counts).sum(dim=1, keepdim=True)) * 10_000)        # models.py:240
        loss_rows = log_gaussian(y, d.loc).sum(dim=1)
    assert torch.isfinite(d.loc).all() and torch.isfinite(d2.loc).all() and torch.isfinite(loss_rows).all()
    np.savez_compressed(os.path.join(HERE, f"{name}.npz"),
                        shapes_json=np.array(json.dumps({k: list(v) for k, v in shapes.items()})), seed=np.array(seed),
                        n_genes=np.array(n_genes), genes=genes, counts=counts, genes_subset=genes_subset,
                        counts_subset=counts_subset, library_size=lib, z=z.numpy(), mu=d.loc.numpy(), zrand=zrand.numpy(),
                        mu_rand=d2.loc.numpy(), loss_rows=loss_rows.numpy())
    print(name, "z absmax", float(z.abs().max()), "mu absmax", float(d.loc.abs().max()), "mu std", float(d.loc.std()),
          "loss_rows", loss_rows.numpy())


if __name__ == "__main__":
    for name, case in gauss_head_ref.CASES.items():
        gen_gauss(name, *case)

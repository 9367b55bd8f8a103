#!/usr/bin/env python3
"""Generate the scVI-baseline fixtures by RUNNING THE REFERENCE (build container only; see make_golden.py for the import stubs).

Run from the repo root:   python tests/golden/make_golden_scvi.py

tests/golden/scvi_<case>.npz: the reference's own `ScviVAE` (src/scldm/vae.py:90-128) built from `EncoderScvi`, `GaussianLinearLayer`,
`DecoderScvi`, `NegativeBinomialLinearLayer` and `StandardPrior`, in eval mode, on the state dict of
`scvi_ref.make_scvi_state_dict(shapes, seed)` - once in fp32 and once in float64.  The reference draws the reparameterisation noise
inside forward (`torch.randn_like(loc)`); the script substitutes the stored `eps` for that one call so that both precisions see the
same noise.  Everything must be finite and the fp32 results within REF_AGREE (scale-relative) of the float64 ones.  Only data is
stored: seed, shapes, counts, library_size, eps and the fp32 h, loc, scale, z, mu, theta.  Running the script twice gives identical
bytes."""
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
from scldm.nnets import DecoderScvi, EncoderScvi  # noqa: E402
from scldm.priors import StandardPrior  # noqa: E402
from scldm.stochastic_layers import GaussianLinearLayer, NegativeBinomialLinearLayer  # noqa: E402
from scldm.vae import ScviVAE  # noqa: E402

import scvi_ref as R  # noqa: E402

REF_AGREE = 1e-5


def scale_rel(a, b) -> float:
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def run_reference(vae, counts, lib, eps):
    """{h, loc, scale, z, mu, theta} of the reference's forward in the module's dtype, with `eps` in place of its own draw."""
    dt = next(vae.parameters()).dtype
    counts, lib, eps = counts.to(dt), lib.to(dt), eps.to(dt)
    real = torch.randn_like
    calls = []

    def given(t, *a, **k):
        assert t.shape == eps.shape and t.dtype == dt
        calls.append(1)
        return eps
    torch.randn_like = given
    try:
        with torch.no_grad():
            lik, post, z = vae(counts, None, lib[:, None])
            h, _ = vae.encoder(counts)
    finally:
        torch.randn_like = real
    assert len(calls) == 1 and torch.equal(z, post.loc + eps * post.scale)
    return {"h": h, "loc": post.loc, "scale": post.scale, "z": z, "mu": lik.mu, "theta": lik.theta}


def gen_scvi(name, n_genes, n_hidden, n_latent, n_layers, B, shared_theta, seed):
    vae = ScviVAE(EncoderScvi(n_genes, n_hidden, n_layers, 0.1), GaussianLinearLayer(n_hidden, n_latent),
                  DecoderScvi(n_latent, n_hidden, n_layers, 0.1),
                  NegativeBinomialLinearLayer(n_genes=n_genes, n_hidden=n_hidden, shared_theta=shared_theta), StandardPrior(n_latent, 0))
    shapes = mg.shapes_of(vae)
    want = R.scvi_shapes(n_genes, n_hidden, n_latent, n_layers, shared_theta)
    assert list(shapes) == list(want) and {k: tuple(v) for k, v in shapes.items()} == want, "the restated key list drifted"
    sd = R.make_scvi_state_dict(shapes, seed)
    vae.load_state_dict(sd, strict=True)
    vae.eval()
    counts, lib, eps = R.make_inputs(n_genes, n_latent, B, seed)
    t = torch.from_numpy
    out32 = run_reference(vae, t(counts), t(lib), t(eps))
    out64 = run_reference(vae.double(), t(counts), t(lib), t(eps))
    errs = {}
    for k in R.OUTPUTS:
        a32, a64 = out32[k].numpy(), out64[k].numpy()
        assert a32.dtype == np.float32 and np.isfinite(a32).all() and np.isfinite(a64).all(), f"{name} {k}: not finite"
        errs[k] = scale_rel(a32, a64)
        assert errs[k] <= REF_AGREE, f"{name} {k}: the reference's fp32 result is {errs[k]:.2e} off its float64 one"
    mu = out32["mu"].numpy()
    assert np.abs(mu.sum(1) / lib - 1).max() < 1e-5
    assert out32["theta"].shape == ((n_genes,) if shared_theta else (B, n_genes))
    np.savez_compressed(os.path.join(HERE, f"{name}.npz"),
                        shapes_json=np.array(json.dumps({k: list(v) for k, v in shapes.items()})), seed=np.array(seed),
                        counts=counts, library_size=lib, eps=eps, **{k: out32[k].numpy() for k in R.OUTPUTS})
    print(name, "fp32 vs float64:", " ".join(f"{k} {e:.1e}" for k, e in errs.items()),
          "| scale range", float(out32["scale"].min()), float(out32["scale"].max()), "theta max", float(out32["theta"].max()))


if __name__ == "__main__":
    for name, case in R.CASES.items():
        gen_scvi(name, *case)

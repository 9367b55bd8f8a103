#!/usr/bin/env python3
"""Generate the scVI-baseline TRAINING fixtures by RUNNING THE REFERENCE (build container only; see make_golden.py for the import stubs).

Run from the repo root:   python tests/golden/make_golden_scvi_train.py

tests/golden/scvi_train_<case>.npz: the reference's own `ScviVAE` (src/scldm/vae.py:90-128) in TRAIN mode on the state dict of
`scvi_ref.make_scvi_state_dict(shapes, seed)` and the inputs of `scvi_ref.make_inputs`, once in fp32 and once in float64.  The
stored `eps` stands in for the reference's `torch.randn_like(loc)` and the stored keep masks for `torch.nn.functional.dropout`
(nn.Dropout looks F.dropout up at call time), so both precisions - and every implementation tested against the fixture - see the
same noise.  Loss: the reference's `log_nb_positive` (scldm.distributions, eps 1e-8) summed over genes and averaged over cells,
plus (post.log_prob(z) - prior.log_prob(z)).sum(1).mean(), as VAEScvi.loss forms them (models.py:1031-1053); backward of their sum.

Stored (data only): seed, shapes, dropout rate, counts, library_size, eps, the masks, the two loss terms, loc, scale, z, the updated
running statistics, mu and unshared theta (in full below scvi_train_ref.FULL_OUTPUT_GENES genes, as make_golden.grad_digest above)
and the grad_digest of every parameter gradient except the Linear biases in front of a BatchNorm, whose gradient is mathematically
zero.  Asserted here: every fp32 result within REF_AGREE (scale-relative) of the float64 run, and the float64 gradients of those
biases below 1e-9 of the same layer's dbeta maximum.  Running the script twice gives identical bytes."""
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
from scldm.distributions import log_nb_positive  # noqa: E402
from scldm.nnets import DecoderScvi, EncoderScvi  # noqa: E402
from scldm.priors import StandardPrior  # noqa: E402
from scldm.stochastic_layers import GaussianLinearLayer, NegativeBinomialLinearLayer  # noqa: E402
from scldm.vae import ScviVAE  # noqa: E402

import scvi_ref as R  # noqa: E402
import scvi_train_ref as T  # noqa: E402

REF_AGREE = 1e-5
assert mg.GRAD_SAMPLE == T.GRAD_SAMPLE


def scale_rel(a, b) -> float:
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def run_reference(vae, counts, lib, eps, masks, rate):
    """One train-mode step of the reference in the module's dtype: outputs, loss terms, gradients, updated running statistics."""
    dt = next(vae.parameters()).dtype
    counts, lib, eps = counts.to(dt), lib.to(dt), eps.to(dt)
    vae.train()
    vae.zero_grad(set_to_none=True)
    real_randn, real_dropout = torch.randn_like, torch.nn.functional.dropout
    noise_calls, queue = [], [m.to(dt) for m in masks]

    def given_noise(t, *a, **k):
        assert t.shape == eps.shape and t.dtype == dt
        noise_calls.append(1)
        return eps

    def given_dropout(x, p=0.5, training=True, inplace=False):
        assert training and p == rate
        if p == 0:
            return x
        return x * queue.pop(0) / (1 - p)
    torch.randn_like = given_noise
    torch.nn.functional.dropout = given_dropout
    try:
        lik, post, z = vae(counts, None, lib[:, None])
    finally:
        torch.randn_like = real_randn
        torch.nn.functional.dropout = real_dropout
    assert len(noise_calls) == 1 and not queue
    llh = (-log_nb_positive(counts, lik.mu, lik.theta)).sum(dim=1).mean()
    kl = (post.log_prob(z) - vae.prior.log_prob(z)).sum(dim=1).mean()
    (llh + kl).backward()
    out = {"loc": post.loc, "scale": post.scale, "z": z, "mu": lik.mu, "theta": lik.theta, "llh": llh, "kl": kl}
    out = {k: v.detach().numpy() for k, v in out.items()}
    grads = {k: v.grad.numpy() for k, v in vae.named_parameters() if v.requires_grad}
    stats = {k: v.detach().numpy().copy() for k, v in vae.state_dict().items() if "running_" in k}
    tracked = {int(v) for k, v in vae.state_dict().items() if k.endswith("num_batches_tracked")}
    assert tracked == {101}
    return out, grads, stats


def build(n_genes, n_hidden, n_latent, n_layers, shared_theta, p, sd, dtype):
    vae = ScviVAE(EncoderScvi(n_genes, n_hidden, n_layers, p), GaussianLinearLayer(n_hidden, n_latent),
                  DecoderScvi(n_latent, n_hidden, n_layers, p),
                  NegativeBinomialLinearLayer(n_genes=n_genes, n_hidden=n_hidden, shared_theta=shared_theta), StandardPrior(n_latent, 0))
    vae.load_state_dict(sd, strict=True)
    return vae.to(dtype)


def gen(name, n_genes, n_hidden, n_latent, n_layers, B, shared_theta, p, seed):
    shapes = R.scvi_shapes(n_genes, n_hidden, n_latent, n_layers, shared_theta)
    sd = R.make_scvi_state_dict(shapes, seed)
    counts, lib, eps = R.make_inputs(n_genes, n_latent, B, seed)
    masks = T.make_masks(n_layers, B, n_hidden, p, seed)
    t = torch.from_numpy
    args = (t(counts), t(lib), t(eps), [t(m) for m in masks], p)
    vae32 = build(n_genes, n_hidden, n_latent, n_layers, shared_theta, p, sd, torch.float32)
    assert {k: tuple(v.shape) for k, v in vae32.state_dict().items()} == shapes
    out32, g32, st32 = run_reference(vae32, *args)
    out64, g64, st64 = run_reference(build(n_genes, n_hidden, n_latent, n_layers, shared_theta, p, sd, torch.float64), *args)
    zero_bias = T.pre_bn_biases(sd)
    errs = {}
    for group, (a, b) in {"out": (out32, out64), "grad": (g32, g64), "stat": (st32, st64)}.items():
        for k in a:
            assert np.isfinite(a[k]).all() and np.isfinite(b[k]).all(), f"{name} {k}: not finite"
            if group == "grad" and k in zero_bias:
                beta = k.rsplit(".", 2)[0] + f".{int(k.rsplit('.', 2)[1]) + 1}.bias"
                assert np.abs(b[k]).max() < 1e-9 * np.abs(b[beta]).max(), f"{name} {k}: float64 pre-BatchNorm bias gradient is not zero"
                continue
            errs[f"{group}:{k}"] = scale_rel(a[k], b[k])
            assert a[k].dtype == np.float32 and errs[f"{group}:{k}"] <= REF_AGREE, f"{name} {k}: fp32 is {errs[f'{group}:{k}']:.2e} off float64"
    assert len(zero_bias) == 2 * n_layers
    for k in st32:      # the step moved the running statistics
        assert np.abs(st32[k] - sd[k].numpy()).max() > 1e-3, k
    full = n_genes < T.FULL_OUTPUT_GENES
    store = {"shapes_json": np.array(json.dumps({k: list(v) for k, v in shapes.items()})), "seed": np.array(seed), "dropout": np.array(p),
             "counts": counts, "library_size": lib, "eps": eps, "llh": out32["llh"], "kl": out32["kl"],
             "loc": out32["loc"], "scale": out32["scale"], "z": out32["z"]}
    for i, m in enumerate(masks):
        store[f"mask_{i}"] = m
    store["mu" if full else "mu_digest"] = out32["mu"] if full else mg.grad_digest(out32["mu"])
    if shared_theta or full:
        store["theta"] = out32["theta"]
    else:
        store["theta_digest"] = mg.grad_digest(out32["theta"])
    for k, v in st32.items():
        store["stat:" + k] = v
    for k, v in g32.items():
        if k not in zero_bias:
            store["grad:" + k] = mg.grad_digest(v)
    path = os.path.join(HERE, f"{name}.npz")
    np.savez_compressed(path, **store)
    worst = max(errs, key=errs.get)
    print(f"{name}: {os.path.getsize(path)} bytes; fp32 vs float64 worst {worst} {errs[worst]:.1e}; llh {float(out32['llh']):.4f} kl {float(out32['kl']):.4f}; "
          f"scale range {float(out32['scale'].min()):.2e} {float(out32['scale'].max()):.2e}; theta max {float(out32['theta'].max()):.1f}")


if __name__ == "__main__":
    for name, case in T.TRAIN_CASES.items():
        gen(name, *case)

#!/usr/bin/env python3
"""Generate the wide TransformerVAE TRAINING fixtures by RUNNING THE REFERENCE (build container only; see make_golden.py for the import
stubs).

Run from the repo root:   python tests/golden/make_golden_vae_wide_train.py

tests/golden/vae_wide_train_{64,128}.npz: the reference's own `TransformerVAE` under autograd, as make_golden.gen_vae_train runs the
32-wide shape, at `vae_wide_cases.CASES["vae_wide_64"]` (shared theta) and `["vae_wide_128"]` (unshared theta) with the inputs and
weights of tests/golden/vae_wide_{64,128}.npz.  Loss: -log_nb_positive(counts, mu, theta).sum(1).mean() + (z * z_weight).sum().
Stored: z_weight (the one input vae_wide_*.npz does not hold), loss, mu, z, make_golden.grad_digest of every parameter gradient and the
list of frozen parameters.  Only data.  Checked before anything is written: everything finite and the reference's fp32 gradients within
REF_AGREE (scale-relative) of its float64 ones; the one exception is decoder_head.params.bias under shared theta, whose gradient is
mathematically zero (softmax over genes is shift-invariant) and noise in both precisions - it must stay below 1e-3 of the norm of
decoder_head.params.weight's gradient, the gate the tests put on it.  Running the script twice gives identical bytes."""
from __future__ import annotations

import copy
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

REF_AGREE = 1e-5
BIAS = "decoder_head.params.bias"
NAMES = {"vae_wide_64": "vae_wide_train_64", "vae_wide_128": "vae_wide_train_128"}


def step(vae, g, zw, dtype):
    from scldm.distributions import log_nb_positive
    f = lambda k: torch.from_numpy(g[k]).to(dtype)      # noqa: E731
    for p in vae.parameters():
        p.grad = None
    params, z = vae(f("counts"), torch.from_numpy(g["genes"]), f("library_size"), f("counts_subset"), torch.from_numpy(g["genes_subset"]))
    loss = (-log_nb_positive(f("counts"), params["mu"], params["theta"])).sum(dim=1).mean() + (z * torch.from_numpy(zw).to(dtype)).sum()
    loss.backward()
    return loss.detach(), params["mu"].detach(), z.detach(), {k: p.grad for k, p in vae.named_parameters() if p.grad is not None}


def gen(case, out_name):
    c = vae_wide_cases.CASES[case]
    g = np.load(os.path.join(HERE, f"{case}.npz"))
    ek, dk, hk, ik = vae_wide_cases.module_kwargs(c)
    vae = mg.TransformerVAE(encoder=mg.Encoder(**ek), decoder=mg.Decoder(**dk), decoder_head=mg.NegativeBinomialTransformerLayer(**hk),
                            input_layer=mg.InputTransformerVAE(**ik))
    shapes = mg.shapes_of(vae)
    assert {k: list(v) for k, v in shapes.items()} == json.loads(str(g["shapes_json"]))
    vae.load_state_dict(mg.make_state_dict(shapes, int(g["seed"])), strict=True)
    vae.train()
    rng = np.random.default_rng(c["seed"] + 2000)
    zw = (0.3 * rng.standard_normal((c["B"], c["n_inducing"], c["n_embed_latent"]))).astype(np.float32)
    loss, mu, z, grads = step(vae, g, zw, torch.float32)
    loss64, mu64, z64, grads64 = step(copy.deepcopy(vae).double(), g, zw, torch.float64)
    frozen = [k for k, _ in vae.named_parameters() if k not in grads]
    assert set(grads) == set(grads64)
    rel = lambda a, b: float((a.double() - b).abs().max() / b.abs().max())      # noqa: E731
    assert abs(float(loss) - float(loss64)) <= REF_AGREE * abs(float(loss64)) and rel(mu, mu64) <= REF_AGREE and rel(z, z64) <= REF_AGREE
    worst = 0.0
    wn = float(grads64["decoder_head.params.weight"].norm())
    for k, v in grads.items():
        assert bool(torch.isfinite(v).all()), k
        if k == BIAS and c["shared_theta"]:
            assert float(v.abs().max()) <= 1e-3 * wn and float(grads64[k].abs().max()) <= 1e-3 * wn
            continue
        e = rel(v, grads64[k])
        assert e <= REF_AGREE, f"{k}: the reference's fp32 gradient is {e:.2e} off its float64 one"
        worst = max(worst, e)
    out = {"z_weight": zw, "loss": np.array(float(loss)), "mu": mu.numpy(), "z": z.numpy(), "frozen_json": np.array(json.dumps(frozen))}
    for k, v in grads.items():
        out[f"grad_{k}"] = mg.grad_digest(v.numpy())
    np.savez_compressed(os.path.join(HERE, f"{out_name}.npz"), **out)
    print(out_name, "loss", float(loss), "frozen", frozen, "n grads", len(grads), f"worst fp32 vs float64 {worst:.2e}")


if __name__ == "__main__":
    for case_, out_ in NAMES.items():
        gen(case_, out_)

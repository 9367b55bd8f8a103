"""The train-mode step of tests/scvi_train_ref.py with every product routed through `oracle.dit.linear`, so that under
`oracle.dit.matmul_operand_bits(10)` autograd rounds both operands of the forward product AND of the two backward products of every
Linear to 10 explicit mantissa bits (oracle.dit._RoundedMatmul): the reference's training arithmetic under
torch.set_float32_matmul_precision("high"), which ScviVAE's fp16 training path is gated against.  With bits None it is the plain
restatement.  BatchNorm, SiLU, dropout, hardtanh / exp, softmax, softplus and the loss stay plain torch.  The step takes optional
upstream gradients for its five outputs in place of the ELBO.  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle.dit import linear
from scvi_ref import BN_EPS
from scvi_train_ref import MOMENTUM, TRAIN_CASES, make_masks, pre_bn_biases, scvi_losses

OUTPUTS = ("loc", "scale", "z", "mu", "theta")

# the two cases without a fixture: name -> (n_genes, n_hidden, n_latent, n_layers, B, shared_theta, dropout, seed)
EXTRA_CASES = {
    "scvi_train_wide_hidden": (67, 1030, 4, 2, 3, False, 0.0, 721),      # K = 1 030: two k-splits in the hidden products, the head's and da W
    "scvi_train_long_batch": (67, 40, 4, 2, 1031, True, 0.25, 722),      # K = B = 1 031: every weight gradient split, with an odd tail
}
ALL_TRAIN_CASES = {**TRAIN_CASES, **EXTRA_CASES}


def _mlp(sd, prefix, x, masks, p, new_stats, momentum, bn_eps):
    i = 0
    while f"{prefix}.{4 * i}.weight" in sd:
        lin, bn = f"{prefix}.{4 * i}", f"{prefix}.{4 * i + 1}"
        a = linear(x, sd[lin + ".weight"], sd[lin + ".bias"])
        mean, var = a.mean(0), a.var(0, unbiased=False)
        n = a.shape[0]
        with torch.no_grad():
            new_stats[bn + ".running_mean"] = (1 - momentum) * sd[bn + ".running_mean"] + momentum * mean
            new_stats[bn + ".running_var"] = (1 - momentum) * sd[bn + ".running_var"] + momentum * var * (n / (n - 1))
        y = (a - mean) / torch.sqrt(var + bn_eps) * sd[bn + ".weight"] + sd[bn + ".bias"]
        x = F.silu(y)
        if p > 0:
            x = x * masks[i].to(x.dtype) / (1 - p)
        i += 1
    return x


def forward(sd, counts, library_size, eps, masks=(), p=0.0, momentum=MOMENTUM, bn_eps=BN_EPS):
    """scvi_train_ref.scvi_train_forward on oracle.dit.linear: ({loc, scale, z, mu, theta}, {running statistic key: updated value})."""
    n_layers = len(masks) // 2
    stats = {}
    h = _mlp(sd, "encoder.encoder_mlp", torch.log1p(counts), masks[:n_layers], p, stats, momentum, bn_eps)
    loc = linear(h, sd["encoder_head.loc.weight"], sd["encoder_head.loc.bias"])
    scale = torch.exp(F.hardtanh(linear(h, sd["encoder_head.scale.weight"], sd["encoder_head.scale.bias"]), min_val=-7.0, max_val=5.0))
    z = loc + eps * scale
    g = _mlp(sd, "decoder.decoder_mlp", z, masks[n_layers:], p, stats, momentum, bn_eps)
    mu = F.softmax(linear(g, sd["decoder_head.mu.weight"], sd["decoder_head.mu.bias"]), dim=1) * library_size.reshape(-1, 1)
    if "decoder_head.theta" in sd:
        theta = F.softplus(sd["decoder_head.theta"])
    else:
        theta = F.softplus(linear(g, sd["decoder_head.theta.weight"], sd["decoder_head.theta.bias"]))
    return {"loc": loc, "scale": scale, "z": z, "mu": mu, "theta": theta}, stats


def step(sd, counts, library_size, eps, masks=(), p=0.0, upstream=None, dtype=torch.float32):
    """One step under autograd, under whatever operand rounding is active: (outputs, stats, {parameter key: gradient}).
    upstream=None: the gradient of the ELBO (llh + kl); else a dict of upstream gradients for OUTPUTS (all five).  Operand rounding
    is defined on float32; dtype=torch.float64 is for comparing the helper itself (rounding off) free of summation-order noise."""
    leaf = {k: (v.detach().to(dtype).clone().requires_grad_(not k.startswith("prior.")) if v.dtype.is_floating_point and "running_" not in k
                else v.detach().to(dtype) if v.dtype.is_floating_point else v) for k, v in sd.items()}
    t = lambda a: torch.as_tensor(a).to(dtype)      # noqa: E731
    out, stats = forward(leaf, t(counts), t(library_size), t(eps), [t(m) for m in masks], p)
    keys = [k for k, v in leaf.items() if v.dtype.is_floating_point and v.requires_grad]
    if upstream is None:
        llh, kl = scvi_losses(out, t(counts))
        got = torch.autograd.grad(llh + kl, [leaf[k] for k in keys], allow_unused=True)
    else:
        got = torch.autograd.grad([out[k] for k in OUTPUTS], [leaf[k] for k in keys], grad_outputs=[t(upstream[k]) for k in OUTPUTS],
                                  allow_unused=True)
    grads = {k: (g if g is not None else torch.zeros_like(leaf[k])) for k, g in zip(keys, got)}
    return {k: v.detach() for k, v in out.items()}, stats, grads


def flat(out, stats, grads, sd):
    """One {name: tensor} for the per-tensor class gate: out:*, stat:* and grad:* without the Linear biases in front of a BatchNorm
    (their gradient is mathematically zero: roundoff in autograd, exact zeros in the kernels)."""
    zero = set(pre_bn_biases(sd))
    rec = {"out:" + k: v for k, v in out.items()}
    rec.update({"stat:" + k: v for k, v in stats.items()})
    rec.update({"grad:" + k: v for k, v in grads.items() if k not in zero})
    return rec


@functools.lru_cache(maxsize=None)
def case(name):
    """(state dict, counts, library_size, eps, masks, dropout) of a case of ALL_TRAIN_CASES as CPU tensors / numpy masks: the
    fixture's for TRAIN_CASES, the deterministic builders of scvi_ref for EXTRA_CASES.  Loaded once, never modified."""
    from scvi_ref import make_inputs, make_scvi_state_dict, scvi_shapes
    n_genes, n_hidden, n_latent, n_layers, B, shared, p, seed = ALL_TRAIN_CASES[name]
    if name in TRAIN_CASES:
        from scvi_train_ref import train_case
        g, sd, masks = train_case(name)
        counts, lib, eps = (torch.from_numpy(g[k]) for k in ("counts", "library_size", "eps"))
    else:
        sd = make_scvi_state_dict(scvi_shapes(n_genes, n_hidden, n_latent, n_layers, shared), seed)
        counts, lib, eps = (torch.from_numpy(v) for v in make_inputs(n_genes, n_latent, B, seed))
        masks = make_masks(n_layers, B, n_hidden, p, seed)
    return sd, counts, lib.reshape(-1), eps, list(masks), p


def upstream_grads(name, seed=0):
    """Random upstream gradients N(0, 1) for the five outputs of a case (theta: (n_genes,) when shared), from one numpy stream."""
    n_genes, n_hidden, n_latent, n_layers, B, shared, p, _ = ALL_TRAIN_CASES[name]
    rng = np.random.default_rng(seed + 4000)
    shape = {"loc": (B, n_latent), "scale": (B, n_latent), "z": (B, n_latent), "mu": (B, n_genes), "theta": (n_genes,) if shared else (B, n_genes)}
    return {k: torch.from_numpy(rng.standard_normal(shape[k]).astype(np.float32)) for k in OUTPUTS}

"""Gradients of the Gaussian-head VAE training loss through the CPU restatement.  TEST INFRASTRUCTURE ONLY (a helper module the
tests and tests/golden/make_golden_gauss_train.py import); it mirrors oracle.vae_train.vae_training_grads.

The reference differentiates `TransformerVAE.forward` (src/scldm/vae.py:29-56, `{"mu"}` for this head) and `VAE.loss`
(src/scldm/models.py:239-245: log_gaussian(log1p(counts / rowsum * 1e4), mu).sum(1).mean()) with torch autograd; oracle.vae.encode
and gauss_head_ref.decode_gaussian are plain differentiable torch, so autograd over them is the CPU restatement.  It is pinned
against digests of the reference's own gradients (tests/golden/gauss_train_*.npz)."""
from __future__ import annotations

import torch

from gauss_head_ref import TARGET_SUM, decode_gaussian
from oracle.vae import VAEConfig, encode
from oracle.vae_train import FROZEN  # noqa: F401  (encoder.pos_embed: the same frozen parameter for both heads)

# the fixtures of tests/golden/make_golden_gauss_train.py: name -> (n_genes, G, S, B, seed)
CASES = {"gauss_train_small": (60, 50, 20, 3, 231), "gauss_train_2000": (2000, 2000, 700, 2, 232)}


def normalized_log1p(counts: torch.Tensor, target_sum: float = TARGET_SUM) -> torch.Tensor:
    """models.py:240: the regression target of the Gaussian head."""
    return torch.log1p(counts / counts.sum(dim=1, keepdim=True) * target_sum)


def gauss_training_grads(sd: dict, cfg: VAEConfig, counts, genes, counts_subset, genes_subset, z_weight=None):
    """loss, (mu, z) and d loss / d parameter for every trainable state_dict entry.  z_weight (B, 16, n_lat): adds
    sum(z * z_weight) to the loss (exercises the gradient path through the returned latent)."""
    p = {k: v.clone().requires_grad_(k not in FROZEN) for k, v in sd.items()}
    z = encode(p, cfg, counts_subset, genes_subset)
    mu = decode_gaussian(p, cfg, z, genes)
    loss = ((normalized_log1p(counts) - mu) ** 2).sum(dim=1).mean()
    if z_weight is not None:
        loss = loss + (z * z_weight).sum()
    loss.backward()
    grads = {k: v.grad for k, v in p.items() if v.grad is not None}
    return loss.detach(), (mu.detach(), z.detach()), grads

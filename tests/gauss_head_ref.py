"""CPU restatement of the Gaussian decoder head on top of the oracle's decoder.  TEST INFRASTRUCTURE ONLY (a helper module the
tests and tests/golden/make_golden_gauss.py import).

Reference: `GaussianTransformerLayer` (src/scldm/stochastic_layers.py:13-35: mu = params(ln(h_x)).squeeze(-1)),
`TransformerVAE.decode` (src/scldm/vae.py:78-85: Normal(mu, 1)) and `VAE.loss` (src/scldm/models.py:239-245 with
src/scldm/distributions.py:58-59: (log1p(counts / rowsum * 1e4) - mu)^2, summed over the genes).  The 32 -> 1 product goes
through `oracle.dit.linear`, so `matmul_operand_bits(b)` rounds its operands like every other Linear of the chain; the kernels keep
the head in fp32 in every policy, which can only put them closer to the exact result than the operand-rounded oracle."""
from __future__ import annotations

import numpy as np
import torch

from oracle.dit import layer_norm, linear
from oracle.vae import VAEConfig, decoder

# the fixtures of tests/golden/make_golden_gauss.py: name -> (n_genes, G, S, B, seed)
CASES = {"gauss_small": (60, 50, 20, 2, 221), "gauss_2000": (2000, 2000, 2000, 2, 222)}
TARGET_SUM = 1e4    # models.py:240


def gaussian_head(sd: dict, cfg: VAEConfig, h: torch.Tensor) -> torch.Tensor:
    """GaussianTransformerLayer.forward: h (B, G, 32) -> mu (B, G)."""
    x = layer_norm(h, cfg.layernorm_eps, sd["decoder_head.ln.weight"], sd["decoder_head.ln.bias"])
    return linear(x, sd["decoder_head.params.weight"], sd["decoder_head.params.bias"]).squeeze(-1)


def decode_gaussian(sd: dict, cfg: VAEConfig, z: torch.Tensor, genes: torch.Tensor) -> torch.Tensor:
    """TransformerVAE.decode with the Gaussian head -> mu (B, G), the mean of Normal(mu, 1)."""
    emb = sd["input_layer.gene_embedding.weight"]
    return gaussian_head(sd, cfg, decoder(sd, cfg, z.to(emb.dtype), emb[genes.long()]))


def recon_loss_rows(counts, mu, target_sum: float = TARGET_SUM) -> np.ndarray:
    """(B,) float64: sum_g (log1p(counts / rowsum * target_sum) - mu)^2 with every step in float64."""
    c = np.asarray(counts, dtype=np.float64)
    m = np.asarray(mu, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        y = np.log1p(c / c.sum(1, keepdims=True) * target_sum)
    return ((y - m) ** 2).sum(1)

"""The latent prior of the scVI-style baseline.  It exists so that a reference `ScviVAE` state dict, which carries `prior.loc` and
`prior.scale`, loads strictly; inference never evaluates it.  Plain torch: nothing here is on a hot path."""
from __future__ import annotations

import math

import torch
from torch import nn


class StandardPrior(nn.Module):
    """N(0, 1) on the latent.  Holds two frozen parameters under the reference's names and shapes: `loc` (zeros) and `scale` (ones),
    (1, n_latent, n_embed), or (1, n_latent) when n_embed is 0 (what the baseline passes)."""

    def __init__(self, n_latent: int, n_embed: int = 1):
        super().__init__()
        if n_latent < 1 or n_embed < 0:
            raise ValueError(f"StandardPrior needs n_latent >= 1 and n_embed >= 0 (got {n_latent}, {n_embed})")
        self.n_latent = n_latent
        self.n_embed = n_embed
        dims = [1, n_latent] + ([n_embed] if n_embed else [])
        for name, fill in (("loc", 0.0), ("scale", 1.0)):
            self.register_parameter(name, nn.Parameter(torch.full(dims, fill), requires_grad=False))

    def extra_repr(self) -> str:
        return f"n_latent={self.n_latent}, n_embed={self.n_embed}"

    def forward(self, x: torch.Tensor | None = None) -> torch.distributions.Normal:
        """The prior as a distribution object (it does not depend on `x`)."""
        return torch.distributions.Normal(self.loc, self.scale)

    def sample(self, n_samples: int) -> torch.Tensor:
        """(n_samples, n_latent[, n_embed]) draws: loc + scale * standard normal noise."""
        noise = torch.randn((n_samples, *self.loc.shape[1:]), device=self.loc.device, dtype=self.loc.dtype)
        return self.loc + self.scale * noise

    def log_prob(self, x: torch.Tensor) -> torch.Tensor:
        """Elementwise log density of `x` (broadcast against the parameters)."""
        u = (x - self.loc) / self.scale
        return -0.5 * u * u - torch.log(self.scale) - 0.5 * math.log(2.0 * math.pi)

    def loss(self, x: torch.Tensor) -> torch.Tensor:
        """The prior's term of a training objective: the log density of the latent."""
        return self.log_prob(x)

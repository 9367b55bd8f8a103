"""Output heads of the VAE with the reference's API: the negative-binomial head (src/scldm/stochastic_layers.py:76-116), shared- and
unshared-theta variants, and the Gaussian head (stochastic_layers.py:13-35) of the `_gaussian` checkpoints."""
from __future__ import annotations

import torch
import torch.nn as nn


class GaussianTransformerLayer(nn.Module):
    """Parameter container of the reference's Gaussian head (stochastic_layers.py:13-35; vae_base.yaml `decoder_name: gaussian`): `ln`
    LayerNorm(n_embed) with affine and `params` Linear(n_embed, 1); mu = params(ln(h_x)), computed inside
    scldm_vae_decode_gaussian (the epilogue of dec_gene_kernel).  TransformerVAE.decode returns Normal(mu, 1) (vae.py:83-85).  The
    class name is what the reference dispatches on (vae.py:46-47, models.py:238).  Decodes only: there is no training backward for it."""

    def __init__(self, *, n_embed: int | None = None, norm_layer: str = "layernorm", layernorm_eps: float = 1e-8):
        super().__init__()
        if n_embed is None:
            raise ValueError("GaussianTransformerLayer requires n_embed (got None)")
        if norm_layer != "layernorm":
            raise NotImplementedError(f"the Gaussian head's kernel normalises with LayerNorm (norm_layer={norm_layer!r})")
        self.ln = nn.LayerNorm(n_embed, eps=layernorm_eps)
        self.params = nn.Linear(n_embed, 1, bias=True)
        self.layernorm_eps = layernorm_eps

    def forward(self, *a, **k):  # pragma: no cover - guard only
        raise RuntimeError("GaussianTransformerLayer is fused into scldm_amd.vae.TransformerVAE.decode")


class NegativeBinomialTransformerLayer(nn.Module):
    """Parameter container with the reference's two variants (stochastic_layers.py:89-96):
      shared_theta=True  (vae_base.yaml `negative_binomial_shared_theta`): `theta` Embedding(n_genes+1, 1) initialised to ones and
                         `params` Linear(n_embed, 1); theta = exp(theta[genes]);
      shared_theta=False (`negative_binomial_unshared_theta`): `theta` is None and `params` is Linear(n_embed, 2); theta = exp of the
                         head's second output, per cell and gene (stochastic_layers.py:109-111).
    mu = softmax_G(params(h)[..., 0] / t) * library_size.  Both are computed inside scldm_vae_decode (dec_gene_kernel); the training
    backward (TransformerVAE.forward under autograd) is built for the shared-theta head only."""

    def __init__(self, *, n_genes: int, shared_theta: bool = False, n_embed: int | None = None, norm_layer: str = "layernorm",
                 layernorm_eps: float = 1e-8, eps_: float = 1e-6, t: float = 1.0):
        super().__init__()
        self.shared_theta = shared_theta
        if shared_theta:
            self.theta = nn.Embedding(n_genes + 1, 1)
            nn.init.ones_(self.theta.weight)
            self.params = nn.Linear(n_embed, 1, bias=True)
        else:
            self.theta = None
            self.params = nn.Linear(n_embed, 2, bias=True)
        self.eps_ = eps_
        self.t = t

    def forward(self, *a, **k):  # pragma: no cover - guard only
        raise RuntimeError("NegativeBinomialTransformerLayer is fused into scldm_amd.vae.TransformerVAE.decode")


class GaussianLinearLayer(nn.Module):
    """Posterior head of the scVI-style baseline (stochastic_layers.py:38-70): `loc` and `scale` Linear(n_hidden, n_latent);
    Normal(loc(h), exp(hardtanh(scale(h), -7, 5))).  Both products, the clamp, the exp and z = loc + eps scale are one kernel inside
    scldm_amd.vae.ScviVAE (scldm_scvi_encode)."""

    def __init__(self, n_hidden: int, n_latent: int):
        super().__init__()
        self.n_hidden, self.n_latent = n_hidden, n_latent
        self.loc = nn.Linear(n_hidden, n_latent, bias=True)
        self.scale = nn.Linear(n_hidden, n_latent, bias=True)

    def forward(self, *a, **k):  # pragma: no cover - guard only
        raise RuntimeError("GaussianLinearLayer is fused into scldm_amd.vae.ScviVAE.encode")


class NegativeBinomialLinearLayer(nn.Module):
    """Likelihood head of the scVI-style baseline (stochastic_layers.py:123-158): `mu` Linear(n_hidden, n_genes); `theta` a
    Parameter (n_genes) initialised to ones (shared_theta=True) or a Linear(n_hidden, n_genes).  mu = library_size softmax_G(mu(g)),
    theta = softplus(theta) or softplus(theta(g)); computed inside scldm_amd.vae.ScviVAE.decode (scldm_scvi_decode)."""

    def __init__(self, *, n_genes: int, n_hidden: int, shared_theta: bool = False):
        super().__init__()
        self.shared_theta = shared_theta
        self.n_genes, self.n_hidden = n_genes, n_hidden
        self.mu = nn.Linear(n_hidden, n_genes, bias=True)
        if shared_theta:
            self.theta = nn.Parameter(torch.ones(n_genes), requires_grad=True)
        else:
            self.theta = nn.Linear(n_hidden, n_genes, bias=True)
        self.softplus = nn.Softplus()

    def forward(self, *a, **k):  # pragma: no cover - guard only
        raise RuntimeError("NegativeBinomialLinearLayer is fused into scldm_amd.vae.ScviVAE.decode")


class NegativeBinomial(torch.distributions.Distribution):
    """Minimal stand-in for scvi.distributions.NegativeBinomial(mu=, theta=) as used by the reference
    (vae.py:87; models.py:819 calls .sample()): holds mu / theta, samples with the Gamma-Poisson mixture."""

    arg_constraints = {}

    def __init__(self, mu: torch.Tensor, theta: torch.Tensor, validate_args=False):
        self.mu, self.theta = mu, theta
        super().__init__(batch_shape=mu.shape, validate_args=validate_args)

    @property
    def mean(self):
        return self.mu

    def log_prob(self, value: torch.Tensor) -> torch.Tensor:
        """Elementwise log-likelihood of `value` (B, G): scldm_amd.distributions.log_nb_positive(value, mu, theta) (the reference's
        own formula, eps 1e-8, one fused HIP kernel forward and one backward), a (G,) theta broadcast over the cells; differentiable
        with respect to mu and theta.  With it VAEScvi.loss runs as written (models.py:1041).  Device tensors only."""
        from .distributions import log_nb_positive
        if not (self.mu.is_cuda and value.is_cuda):
            raise RuntimeError("NegativeBinomial.log_prob runs on the MI355X (log_nb_positive); value, mu and theta must be CUDA (ROCm) tensors")
        return log_nb_positive(value, self.mu, self.theta)

    @torch.no_grad()
    def sample(self, sample_shape=torch.Size(), seed: int | None = None):
        """counts ~ Poisson(Gamma(concentration=theta, rate=theta/mu)) (the parameterisation scvi-tools uses), drawn by the HIP
        kernel behind scldm_nb_sample (Philox4x32-10 + Marsaglia-Tsang + PTRS).  `seed` defaults to a draw from torch's global
        generator, so torch.manual_seed makes it reproducible.  Device tensors only: there is no CPU path."""
        import ctypes as C

        from . import _lib
        shape = self._extended_shape(sample_shape)
        mu = self.mu.expand(shape).contiguous().float()
        theta = self.theta.expand(shape).contiguous().float()
        if not mu.is_cuda:
            raise RuntimeError("NegativeBinomial.sample draws on the MI355X (scldm_nb_sample); mu / theta must be CUDA (ROCm) tensors")
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (), dtype=torch.int64).item())
        out = torch.empty_like(mu)
        with torch.cuda.device(mu.device):
            _lib.check(_lib.lib().scldm_nb_sample(mu.data_ptr(), theta.data_ptr(), out.data_ptr(), mu.numel(), C.c_uint64(seed),
                                                  torch.cuda.current_stream().cuda_stream), "scldm_nb_sample")
        return out


class Normal(torch.distributions.Normal):
    """The distribution TransformerVAE.decode returns for the Gaussian head (vae.py:85: Normal(mu, ones_like(mu))): torch's Normal
    with `.mu` and a `sample` that draws on the device, mirroring NegativeBinomial.sample."""

    def __init__(self, mu: torch.Tensor, scale: torch.Tensor | float = 1.0, validate_args=False):
        self._unit_scale = isinstance(scale, (int, float)) and scale == 1      # (known without reading the device)
        if isinstance(scale, (int, float)):
            # a 0-d device tensor made by a fill launch: torch's own broadcast of a Python number is a host-to-device copy, which
            # makes every decode wait for the stream (measured: 0.2 ms per decode at 512 x 17 002)
            scale = torch.full((), float(scale), dtype=mu.dtype, device=mu.device)
        super().__init__(mu, scale, validate_args=validate_args)

    @property
    def mu(self):
        return self.loc

    @torch.no_grad()
    def sample(self, sample_shape=torch.Size(), seed: int | None = None):
        """mu + scale * n, n ~ N(0, 1) from the HIP kernel behind scldm_normal_sample (Philox4x32-10, Box-Muller; counter = element
        index, so the result depends on (seed, element) only).  `seed` defaults to a draw from torch's global generator.  With scale 1
        (what decode builds) this is bit for bit TransformerVAE.decode_sample with the same seed.  Device tensors only."""
        import ctypes as C

        from . import _lib
        shape = self._extended_shape(sample_shape)
        mu = self.loc.expand(shape).contiguous().float()
        if not mu.is_cuda:
            raise RuntimeError("Normal.sample draws on the MI355X (scldm_normal_sample); mu must be a CUDA (ROCm) tensor")
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (), dtype=torch.int64).item())
        unit = self._unit_scale
        out = torch.empty_like(mu)
        src = mu if unit else torch.zeros_like(mu)
        with torch.cuda.device(mu.device):
            _lib.check(_lib.lib().scldm_normal_sample(src.data_ptr(), out.data_ptr(), mu.numel(), C.c_uint64(seed),
                                                      torch.cuda.current_stream().cuda_stream), "scldm_normal_sample")
        return out if unit else mu + self.scale.expand(shape) * out

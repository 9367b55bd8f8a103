"""Losses with the reference's API (src/scldm/distributions.py): `log_nb_positive` as ONE HIP kernel forward and one backward;
`log_gaussian` and its fused per-cell form for the Gaussian head, `gaussian_recon_loss`."""
from __future__ import annotations

import torch

from . import _lib


class _LogNB(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mu, theta, eps):
        x, mu, theta = x.contiguous().float(), mu.contiguous().float(), theta.contiguous().float()
        out = torch.empty_like(mu)
        with torch.cuda.device(mu.device):
            _lib.check(_lib.lib().scldm_nb_loglik(x.data_ptr(), mu.data_ptr(), theta.data_ptr(), float(eps), out.data_ptr(), mu.numel(),
                                                  torch.cuda.current_stream().cuda_stream), "scldm_nb_loglik")
        ctx.save_for_backward(x, mu, theta)
        ctx.eps = float(eps)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        x, mu, theta = ctx.saved_tensors
        gout = gout.contiguous().float()
        dmu = torch.empty_like(mu) if ctx.needs_input_grad[1] else None
        dth = torch.empty_like(theta) if ctx.needs_input_grad[2] else None
        with torch.cuda.device(mu.device):
            _lib.check(_lib.lib().scldm_nb_loglik_bwd(x.data_ptr(), mu.data_ptr(), theta.data_ptr(), gout.data_ptr(), ctx.eps,
                                                      dmu.data_ptr() if dmu is not None else None, dth.data_ptr() if dth is not None else None,
                                                      mu.numel(), torch.cuda.current_stream().cuda_stream), "scldm_nb_loglik_bwd")
        return None, dmu, dth, None


def _eager_log_nb(x, mu, theta, eps, log_fn, lgamma_fn):
    """The formula of distributions.py:33-42 in torch ops (custom log / lgamma callables)."""
    log_theta_mu_eps = log_fn(theta + mu + eps)
    return (theta * (log_fn(theta + eps) - log_theta_mu_eps) + x * (log_fn(mu + eps) - log_theta_mu_eps)
            + lgamma_fn(x + theta) - lgamma_fn(theta) - lgamma_fn(x + 1))


def log_nb_positive(x: torch.Tensor, mu: torch.Tensor, theta: torch.Tensor, eps: float = 1e-8, log_fn=torch.log,
                    lgamma_fn=torch.lgamma) -> torch.Tensor:
    """Elementwise negative-binomial log-likelihood (distributions.py:6-42, same signature and defaults).
    x, mu, theta: CUDA (ROCm) fp32 tensors; differentiable w.r.t. mu and theta.  With the default `log_fn` / `lgamma_fn`
    (torch.log / torch.lgamma, or None) this is one fused HIP kernel forward and one backward; other callables are applied through
    the reference's formula in torch ops on the same device.  The HIP path has no CPU implementation: CPU tensors raise."""
    log_fn = torch.log if log_fn is None else log_fn
    lgamma_fn = torch.lgamma if lgamma_fn is None else lgamma_fn
    if not (mu.is_cuda and theta.is_cuda and x.is_cuda):
        raise RuntimeError("log_nb_positive runs on the MI355X HIP path; there is no CPU fallback")
    if log_fn is not torch.log or lgamma_fn is not torch.lgamma:
        return _eager_log_nb(x, mu, theta, eps, log_fn, lgamma_fn)
    if x.shape != mu.shape or theta.shape != mu.shape:
        x, mu, theta = torch.broadcast_tensors(x, mu, theta)
    return _LogNB.apply(x, mu, theta, eps)


def log_gaussian(x: torch.Tensor, mu: torch.Tensor, sigma: torch.Tensor | None = None, eps: float = 1e-8, log_fn=torch.log) -> torch.Tensor:
    """Elementwise Gaussian reconstruction term (distributions.py:45-62, same signature and defaults): (x - mu)^2 without `sigma` -
    what VAE.loss uses for the Gaussian head (models.py:241) - else 0.5 ((x - mu) / (sigma + eps))^2 + log(sigma + eps).  Plain
    tensor arithmetic on the inputs' device; the loss of a batch in one pass is `gaussian_recon_loss`."""
    if sigma is None:
        return (x - mu) ** 2
    sigma = sigma + eps
    return 0.5 * torch.pow((x - mu) / sigma, 2) + log_fn(sigma)


class _GaussRecon(torch.autograd.Function):
    @staticmethod
    def forward(ctx, counts, mu, target_sum):
        out = torch.empty(counts.shape[0], dtype=torch.float32, device=counts.device)
        with torch.cuda.device(counts.device):
            _lib.check(_lib.lib().scldm_gaussian_recon_loss(counts.data_ptr(), mu.data_ptr(), counts.shape[0], counts.shape[1], target_sum,
                                                            out.data_ptr(), torch.cuda.current_stream().cuda_stream), "scldm_gaussian_recon_loss")
        ctx.save_for_backward(counts, mu)
        ctx.target_sum = target_sum
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        counts, mu = ctx.saved_tensors
        gout = gout.contiguous().float()
        dmu = torch.empty_like(mu)
        with torch.cuda.device(mu.device):
            _lib.check(_lib.lib().scldm_gaussian_recon_loss_bwd(counts.data_ptr(), mu.data_ptr(), gout.data_ptr(), counts.shape[0],
                                                                counts.shape[1], ctx.target_sum, dmu.data_ptr(),
                                                                torch.cuda.current_stream().cuda_stream), "scldm_gaussian_recon_loss_bwd")
        return None, dmu, None


def gaussian_recon_loss(counts: torch.Tensor, mu: torch.Tensor, target_sum: float = 1e4) -> torch.Tensor:
    """(B,) fp32: sum_g (log1p(counts / rowsum * target_sum) - mu)^2, i.e. `log_gaussian(y, mu).sum(1)` of models.py:240-241,245 in
    one HIP pass (scldm_gaussian_recon_loss) that never writes y; `.mean()` of it is the reference's loss.  Fixed-order sums:
    bit-reproducible.  counts, mu: contiguous fp32 (B, G) CUDA (ROCm) tensors; no CPU path.  Differentiable with respect to `mu`
    when it requires grad (one fused backward pass, scldm_gaussian_recon_loss_bwd: -2 (y - mu) per element); never w.r.t. counts."""
    if not (isinstance(counts, torch.Tensor) and isinstance(mu, torch.Tensor) and counts.is_cuda and mu.device == counts.device):
        raise RuntimeError("gaussian_recon_loss runs on the MI355X HIP path; there is no CPU fallback")
    if counts.dim() != 2 or counts.shape != mu.shape or counts.shape[0] < 1 or counts.shape[1] < 1:
        raise ValueError(f"expected counts and mu (B, G), got {tuple(counts.shape)} and {tuple(mu.shape)}")
    counts = counts.detach().contiguous().float()
    if not (torch.is_grad_enabled() and mu.requires_grad):
        mu = mu.detach()
    return _GaussRecon.apply(counts, mu.contiguous().float(), float(target_sum))

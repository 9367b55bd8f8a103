"""Plain-torch restatement of the reference's scVI-style baseline in TRAIN mode (src/scldm/vae.py:90-128, nnets.py:19-73,
stochastic_layers.py:38-70,123-158) and of the loss the reference trains it with (models.py:1031-1053, distributions.py:6-42), as a
function of a state dict, the reparameterisation noise `eps` and the dropout keep masks.  The fixtures
(tests/golden/scvi_train_*.npz) are written by tests/golden/make_golden_scvi_train.py from the reference's own classes."""
from __future__ import annotations

import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from scvi_ref import BN_EPS

MOMENTUM = 0.1     # nn.BatchNorm1d's default, which the reference does not override
GRAD_SAMPLE = 64   # tests/golden/make_golden.py

# name: (n_genes, n_hidden, n_latent, n_layers, B, shared_theta, dropout, seed)
TRAIN_CASES = {
    "scvi_train_small": (203, 96, 10, 2, 5, True, 0.0, 711),
    "scvi_train_small_unshared": (203, 96, 10, 2, 5, False, 0.0, 712),
    "scvi_train_small_drop": (203, 96, 10, 2, 5, True, 0.25, 713),
    "scvi_train_rows": (203, 96, 10, 2, 70, True, 0.0, 714),
    "scvi_train_tiles": (2003, 128, 16, 1, 70, False, 0.25, 715),
}
FULL_OUTPUT_GENES = 1000      # mu / theta are stored in full below this many genes, as digests above


def make_masks(n_layers, B, n_hidden, p, seed):
    """2 n_layers keep masks (B, n_hidden) uint8, encoder layers first: keep with probability 1 - p.  Empty for p = 0."""
    if p == 0:
        return []
    rng = np.random.default_rng(seed + 2000)
    return [(rng.random((B, n_hidden)) >= p).astype(np.uint8) for _ in range(2 * n_layers)]


def grad_digest(g) -> np.ndarray:
    """[sum, l2, GRAD_SAMPLE strided entries] of a tensor (the digest of tests/golden/make_golden.py)."""
    f = np.asarray(g.detach().cpu().numpy() if hasattr(g, "detach") else g).reshape(-1).astype(np.float64)
    stride = max(1, f.size // GRAD_SAMPLE)
    smp = f[::stride][:GRAD_SAMPLE]
    smp = np.pad(smp, (0, GRAD_SAMPLE - smp.size))
    return np.concatenate([[f.sum(), np.sqrt((f * f).sum())], smp]).astype(np.float64)


def digest_error(ref, ours, numel) -> float:
    """Scale-relative distance of two digests: the sampled entries against the tensor's scale (its largest sampled entry, or its rms
    when the samples miss the large entries), and the L2 norms relative to each other."""
    scale = max(np.abs(ref[2:]).max(), ref[1] / math.sqrt(numel))
    return float(max(np.abs(ours[2:] - ref[2:]).max() / scale, abs(ours[1] - ref[1]) / (ref[1] + 1e-30)))


def pre_bn_biases(sd):
    """The Linear biases in front of a BatchNorm: their gradient is mathematically zero."""
    return [k for k in sd if k.endswith(".bias") and k.rsplit(".", 2)[0].endswith("_mlp") and int(k.rsplit(".", 2)[1]) % 4 == 0]


def _mlp(sd, prefix, x, masks, p, new_stats, momentum, bn_eps):
    i = 0
    while f"{prefix}.{4 * i}.weight" in sd:
        lin, bn = f"{prefix}.{4 * i}", f"{prefix}.{4 * i + 1}"
        a = F.linear(x, sd[lin + ".weight"], sd[lin + ".bias"])
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


def scvi_train_forward(sd, counts, library_size, eps, masks=(), p=0.0, momentum=MOMENTUM, bn_eps=BN_EPS):
    """({loc, scale, z, mu, theta}, {running statistic key: updated value}) of the train-mode forward; `masks` as make_masks gives
    them (torch tensors), encoder layers first."""
    n_layers = len(masks) // 2
    stats = {}
    h = _mlp(sd, "encoder.encoder_mlp", torch.log1p(counts), masks[:n_layers], p, stats, momentum, bn_eps)
    loc = F.linear(h, sd["encoder_head.loc.weight"], sd["encoder_head.loc.bias"])
    scale = torch.exp(F.hardtanh(F.linear(h, sd["encoder_head.scale.weight"], sd["encoder_head.scale.bias"]), min_val=-7.0, max_val=5.0))
    z = loc + eps * scale
    g = _mlp(sd, "decoder.decoder_mlp", z, masks[n_layers:], p, stats, momentum, bn_eps)
    mu = F.softmax(F.linear(g, sd["decoder_head.mu.weight"], sd["decoder_head.mu.bias"]), dim=1) * library_size.reshape(-1, 1)
    if "decoder_head.theta" in sd:
        theta = F.softplus(sd["decoder_head.theta"])
    else:
        theta = F.softplus(F.linear(g, sd["decoder_head.theta.weight"], sd["decoder_head.theta.bias"]))
    return {"loc": loc, "scale": scale, "z": z, "mu": mu, "theta": theta}, stats


def log_nb_positive(x, mu, theta, eps=1e-8):
    """distributions.py:6-42."""
    l = torch.log(theta + mu + eps)
    return theta * (torch.log(theta + eps) - l) + x * (torch.log(mu + eps) - l) + torch.lgamma(x + theta) - torch.lgamma(theta) - torch.lgamma(x + 1)


def scvi_losses(out, counts, kl_weight=1.0):
    """(llh, kl) of VAEScvi.loss with the standard-normal prior."""
    z, loc, scale = out["z"], out["loc"], out["scale"]
    llh = (-log_nb_positive(counts, out["mu"], out["theta"])).sum(1).mean()
    log_q = -0.5 * ((z - loc) / scale) ** 2 - torch.log(scale) - 0.5 * math.log(2 * math.pi)
    log_p = -0.5 * z ** 2 - 0.5 * math.log(2 * math.pi)
    return llh, (kl_weight * (log_q - log_p)).sum(1).mean()


def scvi_train_step(sd, counts, library_size, eps, masks=(), p=0.0, loss="elbo", dtype=torch.float32):
    """One step under autograd: (outputs, stats, (llh, kl), {parameter key: gradient}).  loss="elbo": llh + kl; "zsum": z.sum()."""
    leaf = {k: (v.detach().to(dtype).clone().requires_grad_(not k.startswith("prior.")) if v.dtype.is_floating_point and "running_" not in k
                else v.detach().to(dtype) if v.dtype.is_floating_point else v) for k, v in sd.items()}
    t = lambda a: torch.as_tensor(a).to(dtype)      # noqa: E731
    out, stats = scvi_train_forward(leaf, t(counts), t(library_size), t(eps), [t(m) for m in masks], p)
    llh, kl = scvi_losses(out, t(counts))
    (llh + kl if loss == "elbo" else out["z"].sum()).backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaf.items() if v.dtype.is_floating_point and v.requires_grad}
    return {k: v.detach() for k, v in out.items()}, stats, (llh.detach(), kl.detach()), grads


@functools.lru_cache(maxsize=None)
def train_case(name):
    """(fixture, state dict, masks): loaded once, never modified."""
    from conftest import golden_json, load_golden
    from scvi_ref import make_scvi_state_dict
    g = load_golden(name)
    shapes = {k: tuple(v) for k, v in golden_json(g, "shapes_json").items()}
    masks = [g[f"mask_{i}"] for i in range(sum(k.startswith("mask_") for k in g))]
    return g, make_scvi_state_dict(shapes, int(g["seed"])), masks


def compare_to_fixture(g, out, stats, losses, grads, tol, what):
    """Every output, loss term, running statistic and gradient digest of the fixture against `out` ... `grads` (CPU tensors)."""
    from conftest import max_abs_rel
    errs = {k: max_abs_rel(out[k], g[k]) for k in ("loc", "scale", "z")}
    for k in ("mu", "theta"):
        if k in g:
            errs[k] = max_abs_rel(out[k], g[k])
        else:
            errs[k] = digest_error(g[k + "_digest"], grad_digest(out[k]), out[k].numel())
    errs["llh"], errs["kl"] = max_abs_rel(losses[0], g["llh"]), max_abs_rel(losses[1], g["kl"])
    stat_keys = [k[5:] for k in g if k.startswith("stat:")]
    grad_keys = [k[5:] for k in g if k.startswith("grad:")]
    for k in stat_keys:
        errs["stat:" + k] = max_abs_rel(stats[k], g["stat:" + k])
    for k in grad_keys:
        assert grads[k] is not None, k
        errs["grad:" + k] = digest_error(g["grad:" + k], grad_digest(grads[k]), grads[k].numel())
    worst = max(errs, key=errs.get)
    print(f"[parity] {what}: worst {worst} {errs[worst]:.3e} (gate {tol:g}); llh {errs['llh']:.2e} kl {errs['kl']:.2e}")
    assert all(e <= tol for e in errs.values()), {k: e for k, e in errs.items() if not e <= tol}
    return stat_keys, grad_keys

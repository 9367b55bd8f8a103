"""Plain-torch restatement of the reference's scVI-style baseline in eval mode (src/scldm/vae.py:90-128, nnets.py:19-73,
stochastic_layers.py:38-70,123-158) as a function of a state dict, and the deterministic state-dict builder the fixtures
(tests/golden/scvi_*.npz, written by tests/golden/make_golden_scvi.py from the reference's own classes) are generated with."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

BN_EPS = 1e-5      # nn.BatchNorm1d's default, which the reference does not override

# name: (n_genes, n_hidden, n_latent, n_layers, B, shared_theta, seed)
CASES = {
    "scvi_small": (203, 96, 10, 2, 5, True, 701),
    "scvi_small_unshared": (203, 96, 10, 2, 5, False, 702),
    "scvi_tiles": (2003, 128, 16, 1, 70, True, 703),
}
OUTPUTS = ("h", "loc", "scale", "z", "mu", "theta")


def scvi_shapes(n_genes, n_hidden, n_latent, n_layers, shared_theta):
    """The reference's ScviVAE state_dict: key -> shape, in its order."""
    s = {}

    def mlp(prefix, n_in):
        for i in range(n_layers):
            s[f"{prefix}.{4 * i}.weight"] = (n_hidden, n_in if i == 0 else n_hidden)
            s[f"{prefix}.{4 * i}.bias"] = (n_hidden,)
            for k in ("weight", "bias", "running_mean", "running_var"):
                s[f"{prefix}.{4 * i + 1}.{k}"] = (n_hidden,)
            s[f"{prefix}.{4 * i + 1}.num_batches_tracked"] = ()

    mlp("encoder.encoder_mlp", n_genes)
    for k in ("loc", "scale"):
        s[f"encoder_head.{k}.weight"] = (n_latent, n_hidden)
        s[f"encoder_head.{k}.bias"] = (n_latent,)
    mlp("decoder.decoder_mlp", n_latent)
    if shared_theta:
        s["decoder_head.theta"] = (n_genes,)
    s["decoder_head.mu.weight"] = (n_genes, n_hidden)
    s["decoder_head.mu.bias"] = (n_genes,)
    if not shared_theta:
        s["decoder_head.theta.weight"] = (n_genes, n_hidden)
        s["decoder_head.theta.bias"] = (n_genes,)
    s["prior.loc"] = (1, n_latent)
    s["prior.scale"] = (1, n_latent)
    return s


def make_scvi_state_dict(shapes, seed):
    """Deterministic weights (numpy default_rng, keys in the given order) with NON-TRIVIAL BatchNorm statistics - running_mean ~
    U(-0.5, 0.5), running_var ~ U(0.5, 2), gamma ~ U(0.5, 1.5), beta ~ U(-0.3, 0.3): with freshly initialised ones a kernel that
    ignored them would pass.  The log-scale bias spans the hardtanh clamp on both sides and the theta (bias) the softplus threshold."""
    rng = np.random.default_rng(seed)
    sd = {}
    for k, shp in shapes.items():
        shp = tuple(shp)
        bn = k.rsplit(".", 1)[0] + ".running_mean" in shapes
        leaf = k.rsplit(".", 1)[1]
        if leaf == "num_batches_tracked":
            v = np.array(100, dtype=np.int64)
        elif bn:
            lo, hi = {"running_mean": (-0.5, 0.5), "running_var": (0.5, 2.0), "weight": (0.5, 1.5), "bias": (-0.3, 0.3)}[leaf]
            v = rng.uniform(lo, hi, shp)
        elif k == "prior.loc":
            v = np.zeros(shp)
        elif k == "prior.scale":
            v = np.ones(shp)
        elif k == "encoder_head.scale.bias":
            v = rng.permutation(np.linspace(-10.0, 8.0, shp[0]))       # both ends lie beyond the clamp whatever h is
        elif k in ("decoder_head.theta", "decoder_head.theta.bias"):
            v = rng.permutation(np.linspace(-3.0, 24.0, shp[0]))
        elif leaf == "weight":
            v = rng.standard_normal(shp) / np.sqrt(shp[1])
            if k == "decoder.decoder_mlp.0.weight":
                v = v / 32       # a latent at the upper clamp is ~ exp(5) eps: keep the decoder's pre-activations O(1), or mu is ill-conditioned
        else:
            v = rng.uniform(-0.1, 0.1, shp)
        sd[k] = torch.from_numpy(np.asarray(v, dtype=np.int64 if leaf == "num_batches_tracked" else np.float32))
    return sd


def build_scvi(n_genes, n_hidden, n_latent, n_layers, shared_theta, dropout=0.1):
    """This project's ScviVAE, composed as the reference composes its own (freshly initialised, in training mode, on the CPU)."""
    from scldm_amd.nnets import DecoderScvi, EncoderScvi
    from scldm_amd.priors import StandardPrior
    from scldm_amd.stochastic_layers import GaussianLinearLayer, NegativeBinomialLinearLayer
    from scldm_amd.vae import ScviVAE
    return ScviVAE(EncoderScvi(n_genes, n_hidden, n_layers, dropout), GaussianLinearLayer(n_hidden, n_latent),
                   DecoderScvi(n_latent, n_hidden, n_layers, dropout),
                   NegativeBinomialLinearLayer(n_genes=n_genes, n_hidden=n_hidden, shared_theta=shared_theta), StandardPrior(n_latent, 0))


def make_inputs(n_genes, n_latent, B, seed):
    """counts ~ Poisson(1.5), library_size = counts.sum(1), eps ~ N(0, 1)."""
    rng = np.random.default_rng(seed + 1000)
    counts = rng.poisson(1.5, (B, n_genes)).astype(np.float32)
    eps = rng.standard_normal((B, n_latent)).astype(np.float32)
    return counts, counts.sum(1).astype(np.float32), eps


def _mlp(sd, prefix, x, bn_eps):
    i = 0
    while f"{prefix}.{4 * i}.weight" in sd:
        lin, bn = f"{prefix}.{4 * i}", f"{prefix}.{4 * i + 1}"
        x = F.linear(x, sd[lin + ".weight"], sd[lin + ".bias"])
        x = F.batch_norm(x, sd[bn + ".running_mean"], sd[bn + ".running_var"], sd[bn + ".weight"], sd[bn + ".bias"], False, 0.0, bn_eps)
        x = F.silu(x)
        i += 1
    return x


def scvi_encode(sd, counts, eps=None, bn_eps=BN_EPS):
    h = _mlp(sd, "encoder.encoder_mlp", torch.log1p(counts), bn_eps)
    loc = F.linear(h, sd["encoder_head.loc.weight"], sd["encoder_head.loc.bias"])
    log_scale = F.linear(h, sd["encoder_head.scale.weight"], sd["encoder_head.scale.bias"])
    scale = torch.exp(F.hardtanh(log_scale, min_val=-7.0, max_val=5.0))
    return h, loc, scale, (loc + eps * scale if eps is not None else None)


def scvi_decode(sd, z, library_size, bn_eps=BN_EPS):
    g = _mlp(sd, "decoder.decoder_mlp", z, bn_eps)
    logits = F.linear(g, sd["decoder_head.mu.weight"], sd["decoder_head.mu.bias"])
    if "decoder_head.theta" in sd:
        theta = F.softplus(sd["decoder_head.theta"])
    else:
        theta = F.softplus(F.linear(g, sd["decoder_head.theta.weight"], sd["decoder_head.theta.bias"]))
    return F.softmax(logits, dim=1) * library_size.reshape(-1, 1), theta


def scvi_forward(sd, counts, library_size, eps, bn_eps=BN_EPS):
    """{h, loc, scale, z, mu, theta} of the eval-mode forward."""
    h, loc, scale, z = scvi_encode(sd, counts, eps, bn_eps)
    mu, theta = scvi_decode(sd, z, library_size, bn_eps)
    return {"h": h, "loc": loc, "scale": scale, "z": z, "mu": mu, "theta": theta}

"""CPU-side checks of Gaussian-head training: the restatement's autograd (tests/gauss_train_ref.py) against digests of the reference's
own gradients, and - in float64 - the two identities the per-gene backward kernel hard-codes: the rank-two form of the gradient that
enters the MLP through the head's LayerNorm, and the head's four gradients rebuilt from the running sums P and Q.  The kernels
themselves are tested in tests/test_gpu_gauss_train.py."""
import numpy as np
import pytest
import torch

from conftest import golden_json, load_golden, max_abs_rel
from gauss_train_ref import CASES, FROZEN, gauss_training_grads
from oracle.train import grad_digest
from oracle.vae import VAEConfig
from oracle.weights import make_state_dict

DIGEST_TOL = 1e-4       # the rule tests/test_oracle_vae.py applies to the NB digests


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_gradients_match_reference_digests(name):
    g = load_golden(name)
    n_genes, G, S, B, seed = CASES[name]
    assert (int(g["n_genes"]), g["genes"].shape, g["genes_subset"].shape, int(g["seed"])) == (n_genes, (B, G), (B, S), seed)
    shapes = {k: tuple(v) for k, v in golden_json(g, "shapes_json").items()}
    sd, cfg = make_state_dict(shapes, seed), VAEConfig(n_genes=n_genes)
    t = lambda k: torch.from_numpy(g[k])
    loss, (mu, z), grads = gauss_training_grads(sd, cfg, t("counts"), t("genes"), t("counts_subset"), t("genes_subset"))
    assert abs(float(loss) - float(g["loss"])) <= 2e-5 * abs(float(g["loss"]))
    assert max_abs_rel(mu, g["mu"]) < 5e-5 and max_abs_rel(z, g["z"]) < 5e-5
    assert golden_json(g, "frozen_json") == list(FROZEN)
    assert len(grads) == 176 and sorted(grads) == sorted(k[5:] for k in g if k.startswith("grad_"))
    worst = 0.0
    for k, v in grads.items():          # every one of the 176, the head bias included: nothing is shift-invariant here
        ref, ours = g[f"grad_{k}"], grad_digest(v)
        scale = max(np.abs(ref[2:]).max(), ref[1] / np.sqrt(v.numel()))
        e = max(np.abs(ours[2:] - ref[2:]).max() / scale, abs(ours[1] - ref[1]) / (ref[1] + 1e-30))
        worst = max(worst, e)
        assert e <= DIGEST_TOL, (k, e)
    print(f"[parity] {name}: restatement autograd vs reference digests, worst of 176: {worst:.2e}; "
          f"|d head bias| {abs(float(grads['decoder_head.params.bias'])):.1f}")
    assert abs(float(grads["decoder_head.params.bias"])) > 100


def _head(n, seed):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    return r(n, 32), r(32), r(32), r(32), r(1), r(n), 1e-8      # yo, ln_w, ln_b, head_w, head_b, g = d loss / d mu, eps


def test_rank_two_identity_of_the_gradient_through_the_head_layernorm():
    """d yo = alpha ub + beta xhat with ub = u - mean(u), u = head_w * ln_w, s = mean(u * xhat), alpha = g rstd, beta = -alpha s."""
    yo, ln_w, ln_b, hw, hb, g, eps = _head(64, 1)
    yo.requires_grad_(True)
    mu = torch.nn.functional.layer_norm(yo, (32,), ln_w, ln_b, eps) @ hw + hb
    (mu * g).sum().backward()
    with torch.no_grad():
        mean = yo.mean(1, keepdim=True)
        rstd = 1.0 / torch.sqrt(((yo - mean) ** 2).mean(1, keepdim=True) + eps)
        xhat = (yo - mean) * rstd
        u = hw * ln_w
        ub = u - u.mean()
        s = (u * xhat).mean(1, keepdim=True)
        assert torch.allclose(s, (ub * xhat).mean(1, keepdim=True), rtol=0, atol=1e-12)      # (the kernel uses ub for both)
        alpha = g[:, None] * rstd
        beta = -alpha * s
        dyo = alpha * ub + beta * xhat
    assert max_abs_rel(dyo, yo.grad) < 1e-12


def test_head_gradients_from_the_running_sums():
    """P_i = sum g xhat_i, Q = sum g:  d ln_w = head_w * P, d ln_b = head_w Q, d head_w = ln_w * P + ln_b Q, d head_b = Q."""
    yo, ln_w, ln_b, hw, hb, g, eps = _head(200, 2)
    for p in (ln_w, ln_b, hw, hb):
        p.requires_grad_(True)
    mu = torch.nn.functional.layer_norm(yo, (32,), ln_w, ln_b, eps) @ hw + hb
    (mu * g).sum().backward()
    with torch.no_grad():
        xhat = torch.nn.functional.layer_norm(yo, (32,), None, None, eps)
        P, Q = (g[:, None] * xhat).sum(0), g.sum()
        assert max_abs_rel(hw * P, ln_w.grad) < 1e-12
        assert max_abs_rel(hw * Q, ln_b.grad) < 1e-12
        assert max_abs_rel(ln_w * P + ln_b * Q, hw.grad) < 1e-12
        assert max_abs_rel(Q.reshape(1), hb.grad) < 1e-12


def test_abi_declares_the_gaussian_training_entries():
    import os
    import re
    from conftest import ROOT
    from scldm_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "scldm_hip.h")).read()
    declared = set(re.findall(r"\b(scldm_[a-z_0-9]+)\s*\(", hdr))
    L = _lib.lib()
    for name in ("scldm_vae_train_gaussian_forward", "scldm_vae_train_gaussian_backward", "scldm_gaussian_recon_loss_bwd"):
        assert name in declared and name in _lib.EXPORTS and hasattr(L, name), name
    # argument validation needs no GPU: nothing is launched for a rejected call
    assert L.scldm_gaussian_recon_loss_bwd(None, None, None, 1, 1, 1e4, None, None) == -1
    assert L.scldm_vae_train_gaussian_forward(None, None, None, 1, 1, None, 1, None, None, None, None, None) == -1
    from scldm_amd.vae import TransformerVAE
    assert TransformerVAE.train_gaussian_head is False

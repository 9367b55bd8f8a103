"""CPU-side checks of training the unshared-theta NB head (decoder_name negative_binomial_unshared_theta; params is Linear(32, 2),
theta = exp of its second output): oracle/vae_train.py runs unchanged on that state dict and is pinned here to digests of the
reference's own autograd gradients; in float64, the identities the per-gene backward kernel hard-codes (two launch-constant head
vectors: d hid = d0 c0 + d1 c1, d Wc = w0 (x) C0 + w1 (x) C1, d w_k = sum d_k y + Wc C_k).  The kernels themselves are tested in
tests/test_gpu_unshared_train.py."""
import numpy as np
import pytest
import torch

from conftest import golden_json, load_golden, max_abs_rel
from oracle.train import grad_digest
from oracle.vae import VAEConfig
from oracle.vae_train import FROZEN, vae_training_grads
from oracle.weights import make_state_dict

TOL = 1e-4       # of each tensor's scale: the rule tests/test_oracle_vae.py applies to the shared head's digests
# name: (n_genes, G, S, B, seed) - the cases of tests/golden/make_golden_unshared_train.py
CASES = {"vae_train_unshared_small": (60, 50, 20, 3, 231), "vae_train_unshared_2000": (2000, 2000, 700, 2, 232)}
BIAS, WEIGHT = "decoder_head.params.bias", "decoder_head.params.weight"


def digest_error(ref, ours, numel):
    scale = max(np.abs(ref[2:]).max(), ref[1] / np.sqrt(numel))
    return max(np.abs(ours[2:] - ref[2:]).max() / scale, abs(ours[1] - ref[1]) / (ref[1] + 1e-30))


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_gradients_match_reference_digests(name):
    g = load_golden(name)
    n_genes, G, S, B, seed = CASES[name]
    assert (int(g["n_genes"]), g["genes"].shape, g["genes_subset"].shape, int(g["seed"])) == (n_genes, (B, G), (B, S), seed)
    shapes = {k: tuple(v) for k, v in golden_json(g, "shapes_json").items()}
    assert "decoder_head.theta.weight" not in shapes and shapes[WEIGHT] == (2, 32) and shapes[BIAS] == (2,)
    sd, cfg = make_state_dict(shapes, seed), VAEConfig(n_genes=n_genes)
    t = lambda k: torch.from_numpy(g[k])
    loss, (mu, theta, z), grads = vae_training_grads(sd, cfg, t("counts"), t("genes"), t("library_size"), t("counts_subset"), t("genes_subset"))
    assert abs(float(loss) - float(g["loss"])) <= TOL * abs(float(g["loss"]))
    assert theta.shape == (B, G) and float(theta.std()) > 0
    assert max_abs_rel(mu, g["mu"]) < TOL and max_abs_rel(theta, g["theta"]) < TOL and max_abs_rel(z, g["z"]) < TOL
    assert golden_json(g, "frozen_json") == list(FROZEN)
    assert len(grads) == 174 and sorted(grads) == sorted(k[5:] for k in g if k.startswith("grad_"))
    assert "decoder_head.theta.weight" not in grads and grads[WEIGHT].shape == (2, 32) and grads[BIAS].shape == (2,)
    worst = (0.0, None)
    for k, v in grads.items():          # every one of the 174; the (2,) bias as one tensor (its second entry is large and real)
        assert torch.isfinite(v).all(), k
        e = digest_error(g[f"grad_{k}"], grad_digest(v), v.numel())
        worst = max(worst, (e, k))
        assert e <= TOL, (k, e)
    print(f"[parity] {name}: oracle autograd vs reference digests, worst of 174: {worst[0]:.2e} ({worst[1]}); "
          f"d head bias {grads[BIAS].tolist()}")
    assert abs(float(grads[BIAS][1])) > 1.0 and abs(float(grads[BIAS][0])) < 1e-3 * abs(float(grads[BIAS][1]))


def test_two_head_rows_identities_of_the_per_gene_backward():
    """yo = y + Wc hid, l_k = w_k . yo + b_k (k = 0, 1), loss gradients d_k per gene:  d hid = d0 c0 + d1 c1 with c_k = Wc^T w_k;
    d Wc = w0 (x) C0 + w1 (x) C1 with C_k = sum d_k hid;  d w_k = sum d_k y + Wc C_k;  d b_k = sum d_k;  d y = d0 w0 + d1 w1."""
    gen = torch.Generator().manual_seed(4)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    n, H = 70, 88
    y, hid, Wc, W, b, d = r(n, 32), r(n, H), r(32, H), r(2, 32), r(2), r(n, 2)
    for p in (y, hid, Wc, W, b):
        p.requires_grad_(True)
    l = (y + hid @ Wc.T) @ W.T + b
    (l * d).sum().backward()
    with torch.no_grad():
        c = W @ Wc                               # (2, H): c_k
        C_ = d.T @ hid                           # (2, H): C_k
        assert max_abs_rel(d @ c, hid.grad) < 1e-12
        assert max_abs_rel(W.T @ C_, Wc.grad) < 1e-12
        assert max_abs_rel(d.T @ y + C_ @ Wc.T, W.grad) < 1e-12
        assert max_abs_rel(d.sum(0), b.grad) < 1e-12
        assert max_abs_rel(d @ W, y.grad) < 1e-12


def test_switch_exists_and_is_off_by_default():
    from scldm_amd.vae import TransformerVAE
    assert TransformerVAE.train_unshared_theta is False
    from test_abi_cpu import _build_vae
    vae = _build_vae(20, shared_theta=False)
    assert vae.train_unshared_theta is False and vae.decoder_head.theta is None
    assert sum(p.numel() > 0 for n, p in vae.named_parameters() if n not in FROZEN) == 174

"""ScviVAE training on the MI355X where a product's K exceeds one split (1024 k-values), which no train-mode fixture reaches:

  * n_hidden = 1030: the posterior head's two forward products (K = n_hidden) arrive as two planes each, as do the hidden layers'
    forward products and the data gradients `da W` (K = n_hidden);
  * B = 1030: every weight gradient `dA^T X` (K = batch) is cut over the batch and merged in slot order, and the BatchNorm column sums
    walk 33 rows per thread.

The reference is the CPU restatement (tests/scvi_train_ref.py, pinned to the reference's fixtures by test_scvi_train_cpu.py) in
float64, so the gate is the project's standing fp32 one with nothing of the reference's own roundoff in it."""
import functools

import pytest
import torch

from conftest import max_abs_rel
from scvi_ref import build_scvi, make_inputs, make_scvi_state_dict, scvi_shapes
from scvi_train_ref import make_masks, pre_bn_biases, scvi_train_step

pytestmark = pytest.mark.gpu
TOL = 1e-4          # the project's standing fp32 gate: max abs error over max abs reference, per tensor

# name: (n_genes, n_hidden, n_latent, n_layers, B, shared_theta, dropout, seed)
SPLIT_CASES = {
    "wide_hidden": (203, 1030, 10, 2, 5, False, 0.0, 721),
    "long_batch": (203, 96, 10, 2, 1030, True, 0.25, 722),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(state dict, counts, library, eps, masks, the float64 restatement's step): computed once, shared, never modified."""
    n_genes, n_hidden, n_latent, n_layers, B, shared, p, seed = SPLIT_CASES[name]
    sd = make_scvi_state_dict(scvi_shapes(n_genes, n_hidden, n_latent, n_layers, shared), seed)
    counts, lib, eps = make_inputs(n_genes, n_latent, B, seed)
    masks = make_masks(n_layers, B, n_hidden, p, seed)
    return sd, counts, lib, eps, masks, scvi_train_step(sd, counts, lib, eps, masks, p, dtype=torch.float64)


@pytest.mark.parametrize("name", sorted(SPLIT_CASES))
def test_training_step_above_one_split(name):
    from scldm_amd.training import scvi_loss
    n_genes, n_hidden, n_latent, n_layers, B, shared, p, seed = SPLIT_CASES[name]
    sd, counts, lib, eps, masks, (r_out, r_stats, r_losses, r_grads) = case(name)
    vae = build_scvi(n_genes, n_hidden, n_latent, n_layers, shared, dropout=p)
    vae.load_state_dict(sd, strict=True)
    vae = vae.cuda().train()
    vae.train_enabled = True
    c, l, e = (torch.from_numpy(a).cuda() for a in (counts, lib, eps))
    lik, post, z = vae(c, None, l[:, None], eps=e, dropout_masks=[torch.from_numpy(m).cuda() for m in masks] if masks else None)
    terms = scvi_loss(vae, c, lik, post, z)
    sum(terms.values()).backward()
    out = {"loc": post.loc, "scale": post.scale, "z": z, "mu": lik.mu, "theta": lik.theta}
    errs = {"out:" + k: max_abs_rel(out[k].detach().cpu(), v.float()) for k, v in r_out.items()}
    errs["llh"] = max_abs_rel(terms["llh"].detach().cpu(), r_losses[0].float())
    errs["kl"] = max_abs_rel(terms["kl"].detach().cpu(), r_losses[1].float())
    now = vae.state_dict()
    errs.update({"stat:" + k: max_abs_rel(now[k].cpu(), v.float()) for k, v in r_stats.items()})
    grads = {k: q.grad for k, q in vae.named_parameters() if q.requires_grad}
    zero = pre_bn_biases(sd)
    for k, v in r_grads.items():
        assert grads[k] is not None and grads[k].shape == v.shape, k
        if k in zero:
            assert torch.count_nonzero(grads[k]) == 0, k
        else:
            errs["grad:" + k] = max_abs_rel(grads[k].cpu(), v.float())
    worst = max(errs, key=errs.get)
    print(f"[parity] {name}: HIP vs float64 restatement: worst {worst} {errs[worst]:.3e} (gate {TOL:g})")
    assert all(err <= TOL for err in errs.values()), {k: err for k, err in errs.items() if not err <= TOL}
    assert len(zero) == 2 * n_layers and len(r_stats) == 4 * n_layers
    assert len(errs) == 5 + 2 + len(r_stats) + len(r_grads) - len(zero)


def test_an_in_place_parameter_update_before_backward_is_refused():
    """The backward reads the weights where the forward read them, so autograd's version check has to see the parameters."""
    n_genes, n_hidden, n_latent, n_layers, B, shared, p, seed = 203, 96, 10, 2, 5, True, 0.0, 723
    vae = build_scvi(n_genes, n_hidden, n_latent, n_layers, shared, dropout=p)
    vae.load_state_dict(make_scvi_state_dict(scvi_shapes(n_genes, n_hidden, n_latent, n_layers, shared), seed), strict=True)
    vae = vae.cuda().train()
    vae.train_enabled = True
    counts, lib, eps = (torch.from_numpy(a).cuda() for a in make_inputs(n_genes, n_latent, B, seed))
    _, _, z = vae(counts, None, lib[:, None], eps=eps)
    with torch.no_grad():
        vae.encoder_head.loc.weight.mul_(0.5)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        z.sum().backward()

"""ScviVAE training on the MI355X (scldm_scvi_train_forward / _backward behind ScviVAE.forward with `train_enabled`) against the
reference's train-mode fixtures (tests/golden/scvi_train_*.npz, written by make_golden_scvi_train.py from the reference's own
classes) and the CPU restatement (tests/scvi_train_ref.py): outputs, loss terms, every gradient, the running statistics, bit-equal
repeats, the drawn dropout masks, partial upstream gradients, and the eval path after a step."""
import functools
import math

import numpy as np
import pytest
import torch

from conftest import max_abs_rel
from scvi_ref import build_scvi, scvi_forward
from scvi_train_ref import TRAIN_CASES, compare_to_fixture, pre_bn_biases, scvi_train_step, train_case

pytestmark = pytest.mark.gpu
TOL = 1e-4          # the project's standing fp32 gate: max abs error over max abs reference, per tensor


@functools.lru_cache(maxsize=None)
def device_inputs(name):
    g, sd, masks = train_case(name)
    x = {k: torch.from_numpy(g[k]).cuda() for k in ("counts", "library_size", "eps")}
    return x, ([torch.from_numpy(m).cuda() for m in masks] if masks else None)


@functools.lru_cache(maxsize=None)
def restatement(name, loss="elbo"):
    """The CPU restatement's step on the fixture's inputs: computed once, shared, never modified."""
    g, sd, masks = train_case(name)
    return scvi_train_step(sd, g["counts"], g["library_size"], g["eps"], masks, TRAIN_CASES[name][6], loss=loss)


def fresh_model(name, dropout=None, switch=True):
    n_genes, n_hidden, n_latent, n_layers, B, shared, p, seed = TRAIN_CASES[name]
    vae = build_scvi(n_genes, n_hidden, n_latent, n_layers, shared, dropout=p if dropout is None else dropout)
    vae.load_state_dict(train_case(name)[1], strict=True)
    vae = vae.cuda().train()
    vae.train_enabled = switch
    return vae


def step(vae, x, masks=None, seed=None, loss="elbo"):
    """One training step: (outputs, (llh, kl), {key: gradient}, {key: running statistic}), all on the device."""
    from scldm_amd.training import scvi_loss
    for p in vae.parameters():
        p.grad = None
    lik, post, z = vae(x["counts"], None, x["library_size"][:, None], eps=x["eps"], dropout_masks=masks, seed=seed)
    out = {"loc": post.loc, "scale": post.scale, "z": z, "mu": lik.mu, "theta": lik.theta}
    assert all(v.requires_grad for v in out.values())
    if loss == "elbo":
        terms = scvi_loss(vae, x["counts"], lik, post, z)
        assert list(terms) == ["llh", "kl"]
        sum(terms.values()).backward()
        losses = (terms["llh"].detach(), terms["kl"].detach())
    else:
        z.sum().backward()
        losses = None
    grads = {k: p.grad for k, p in vae.named_parameters() if p.requires_grad}
    stats = {k: v.clone() for k, v in vae.state_dict().items() if "running_" in k}
    return {k: v.detach() for k, v in out.items()}, losses, grads, stats


def cpu(d):
    return {k: (v.cpu() if v is not None else None) for k, v in d.items()}


@pytest.mark.parametrize("name", sorted(TRAIN_CASES))
def test_training_step_matches_the_reference(name):
    g, sd, _ = train_case(name)
    x, masks = device_inputs(name)
    vae = fresh_model(name)
    out, losses, grads, stats = step(vae, x, masks)
    n_genes, n_hidden, n_latent, n_layers, B, shared, p, seed = TRAIN_CASES[name]
    assert out["mu"].shape == (B, n_genes) and out["theta"].shape == ((n_genes,) if shared else (B, n_genes))
    compare_to_fixture(g, cpu(out), cpu(stats), tuple(t.cpu() for t in losses), cpu(grads), TOL, f"{name}: HIP training step vs reference")
    # elementwise against the restatement's full gradients (the fixture holds digests), outputs and statistics
    r_out, r_stats, r_losses, r_grads = restatement(name)
    zero = pre_bn_biases(sd)
    errs = {}
    for k, v in r_grads.items():
        assert grads[k] is not None and grads[k].shape == v.shape, k
        if k in zero:
            assert torch.count_nonzero(grads[k]) == 0, k      # exact zeros, not None and not roundoff
        else:
            errs[k] = max_abs_rel(grads[k].cpu(), v)
    errs.update({"out:" + k: max_abs_rel(out[k].cpu(), v) for k, v in r_out.items()})
    errs.update({"stat:" + k: max_abs_rel(stats[k].cpu(), v) for k, v in r_stats.items()})
    worst = max(errs, key=errs.get)
    print(f"[parity] {name}: HIP vs restatement, elementwise: worst {worst} {errs[worst]:.3e} (gate {TOL:g})")
    assert all(e <= TOL for e in errs.values()), {k: e for k, e in errs.items() if not e <= TOL}
    assert len(zero) == 2 * n_layers and len(errs) == len(r_grads) - len(zero) + len(r_out) + len(r_stats) and len(r_stats) == 4 * n_layers
    tracked = {int(v) for k, v in vae.state_dict().items() if k.endswith("num_batches_tracked")}
    assert tracked == {101}
    row = (out["mu"].double().sum(1) / x["library_size"].double() - 1).abs().max()
    assert float(row) < 1e-5


@pytest.mark.parametrize("name", ["scvi_train_small_drop", "scvi_train_tiles"])
def test_two_fresh_modules_give_the_same_bits(name):
    x, masks = device_inputs(name)
    a, b = step(fresh_model(name), x, masks), step(fresh_model(name), x, masks)
    for da, db in ((a[0], b[0]), (a[2], b[2]), (a[3], b[3])):
        for k in da:
            assert torch.equal(da[k], db[k]), k
    assert torch.equal(a[1][0], b[1][0]) and torch.equal(a[1][1], b[1][1])


def test_drawn_masks_depend_on_the_seed_alone_and_replay_bit_for_bit():
    name, p = "scvi_train_rows", 0.25
    x, _ = device_inputs(name)

    def run(seed=None, masks=None):
        vae = fresh_model(name, dropout=p)
        res = step(vae, x, masks=masks, seed=seed)
        return res, [m.clone() for m in vae.last_dropout_masks]
    (a, ma), (b, mb), (c, mc) = run(seed=3), run(seed=3), run(seed=4)
    assert len(ma) == 4 and all(m.dtype == torch.uint8 and m.shape == (70, 96) for m in ma)
    for i in range(4):
        assert torch.equal(ma[i], mb[i]) and not torch.equal(ma[i], mc[i])
        assert int(ma[i].max()) == 1 and int(ma[i].min()) == 0
        for j in range(i):
            assert not torch.equal(ma[i], ma[j])          # the layers draw from separate streams
    (d, md) = run(masks=ma)
    for res in (b, d):
        for da, db in ((a[0], res[0]), (a[2], res[2]), (a[3], res[3])):
            for k in da:
                assert torch.equal(da[k], db[k]), k
    assert not torch.equal(a[0]["mu"], c[0]["mu"])
    n = 4 * 70 * 96
    kept = sum(int(m.sum()) for m in ma) / n
    print(f"[dropout] kept fraction {kept:.4f} of {n} (expected {1 - p}, bound {4 * math.sqrt(p * (1 - p) / n):.4f})")
    assert abs(kept - (1 - p)) <= 4 * math.sqrt(p * (1 - p) / n)
    # the masks act as the restatement applies them
    g, sd, _ = train_case(name)
    r_out, r_stats, _, r_grads = scvi_train_step(sd, g["counts"], g["library_size"], g["eps"], [m.cpu().numpy() for m in ma], p)
    errs = {k: max_abs_rel(a[2][k].cpu(), v) for k, v in r_grads.items() if k not in pre_bn_biases(sd)}
    errs.update({"out:" + k: max_abs_rel(a[0][k].cpu(), v) for k, v in r_out.items()})
    assert all(e <= TOL for e in errs.values()), {k: e for k, e in errs.items() if not e <= TOL}


@pytest.mark.parametrize("name", ["scvi_train_small_unshared", "scvi_train_small_drop"])
def test_partial_upstream_gradients(name):
    """z.sum().backward() alone: no likelihood term, so the decoder and its head get zeros through the NULL-gradient path."""
    g, sd, _ = train_case(name)
    x, masks = device_inputs(name)
    out, _, grads, _ = step(fresh_model(name), x, masks, loss="zsum")
    _, _, _, r_grads = restatement(name, "zsum")
    zero = pre_bn_biases(sd)
    for k, v in r_grads.items():
        assert grads[k] is not None, k
        if k in zero or float(v.abs().max()) == 0.0:
            assert torch.count_nonzero(grads[k]) == 0, k
        else:
            e = max_abs_rel(grads[k].cpu(), v)
            assert e <= TOL, (k, e)
    assert any(k.startswith("decoder") and float(v.abs().max()) == 0.0 for k, v in r_grads.items())
    assert float(r_grads["encoder.encoder_mlp.0.weight"].abs().max()) > 0


def test_eval_after_a_step_uses_the_updated_running_statistics():
    name = "scvi_train_small_drop"
    g, sd, _ = train_case(name)
    x, masks = device_inputs(name)
    vae = fresh_model(name)
    vae.eval()
    before = vae(x["counts"], None, x["library_size"], eps=x["eps"])[0].mu.clone()
    vae.train()
    step(vae, x, masks)
    vae.eval()
    lik, post, z = vae(x["counts"], None, x["library_size"], eps=x["eps"])
    now = {k: v.detach().cpu() for k, v in vae.state_dict().items()}
    assert max_abs_rel(now["encoder.encoder_mlp.1.running_mean"], sd["encoder.encoder_mlp.1.running_mean"]) > 1e-2
    want = scvi_forward(now, torch.from_numpy(g["counts"]), torch.from_numpy(g["library_size"]), torch.from_numpy(g["eps"]))
    for k, v in (("loc", post.loc), ("scale", post.scale), ("z", z), ("mu", lik.mu), ("theta", lik.theta)):
        e = max_abs_rel(v.cpu(), want[k])
        assert e <= TOL, (k, e)
    assert max_abs_rel(before.cpu(), want["mu"]) > 1e-3          # the statistics matter to the result


def test_switch_off_keeps_refusing_training_mode_on_device_tensors():
    name = "scvi_train_small"
    x, _ = device_inputs(name)
    vae = fresh_model(name, switch=False)
    with pytest.raises(NotImplementedError, match="no training path"):
        vae(x["counts"], None, x["library_size"], eps=x["eps"])
    vae.train_enabled = True
    with pytest.raises(NotImplementedError, match="no training path"):
        vae.encode(x["counts"])
    with pytest.raises(ValueError, match="at least two cells"):
        vae(x["counts"][:1], None, x["library_size"][:1], eps=x["eps"][:1])
    with pytest.raises(NotImplementedError, match="requires grad"):
        vae(x["counts"], None, x["library_size"], eps=x["eps"].clone().requires_grad_())

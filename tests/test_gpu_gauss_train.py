"""GPU parity of TRAINING the Gaussian decoder head (`train_gaussian_head = True`): scldm_vae_train_gaussian_forward / _backward
through the autograd binding, against
  (a) digests of the REFERENCE's own autograd gradients of all 176 trainable parameters (tests/golden/gauss_train_*.npz), and
  (b) autograd over the CPU restatement (tests/gauss_train_ref.py) on ragged sizes, multi-tile walks, with a gradient through z.
fp32; tolerance: the rule of tests/test_gpu_vae_train.py - 1e-4 of each tensor's scale (max |entry|, or l2 / sqrt(numel) for the
digests).  No gradient is excused: the head bias gradient is large and real for this head."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from conftest import golden_json, load_golden, max_abs_rel
from gauss_train_ref import FROZEN, gauss_training_grads, normalized_log1p
from oracle.train import grad_digest
from oracle.vae import VAEConfig
from oracle.weights import make_state_dict
from test_gauss_head_cpu import build_gauss_vae

pytestmark = pytest.mark.gpu
TOL = 1e-4
TABLE = "input_layer.gene_embedding.weight"


def cu(a):
    return torch.from_numpy(np.asarray(a)).cuda()


def build(n_genes, seed):
    vae = build_gauss_vae(n_genes)
    sd = make_state_dict({k: tuple(v.shape) for k, v in vae.state_dict().items()}, seed)
    vae.load_state_dict(sd, strict=True)
    vae = vae.cuda().train()
    vae.train_gaussian_head = True
    return vae, sd, VAEConfig(n_genes=n_genes)


def hip_step(vae, counts, genes, counts_s, genes_s, z_weight=None, fused_loss=False):
    for p in vae.parameters():
        p.grad = None
    lib = torch.ones(counts.shape[0], 1, device="cuda")          # accepted and unused by this head, as in the reference
    params, z = vae(cu(counts), cu(genes), lib, cu(counts_s), cu(genes_s))
    assert set(params) == {"mu"} and params["mu"].requires_grad and z.requires_grad
    if fused_loss:
        from scldm_amd.distributions import gaussian_recon_loss
        rows = gaussian_recon_loss(cu(counts), params["mu"])
    else:   # the reference's own eager formula on top of the differentiable output (models.py:239-245)
        rows = ((normalized_log1p(cu(counts)) - params["mu"]) ** 2).sum(dim=1)
    loss = rows.mean()
    if z_weight is not None:
        loss = loss + (z * cu(z_weight)).sum()
    loss.backward()
    return loss.detach(), params["mu"].detach(), z.detach(), {k: p.grad.clone() for k, p in vae.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("name", ["gauss_train_small", "gauss_train_2000"])
@pytest.mark.parametrize("fused_loss", [False, True])
def test_gradients_match_reference_digests(name, fused_loss):
    g = load_golden(name)
    vae, sd, cfg = build(int(g["n_genes"]), int(g["seed"]))
    loss, mu, z, grads = hip_step(vae, g["counts"], g["genes"], g["counts_subset"], g["genes_subset"], fused_loss=fused_loss)
    print(f"[parity] {name} (fused loss {fused_loss}): loss {float(loss):.4f} (reference {float(g['loss']):.4f})")
    assert abs(float(loss) - float(g["loss"])) <= TOL * abs(float(g["loss"]))
    assert max_abs_rel(mu.cpu(), g["mu"]) < TOL and max_abs_rel(z.cpu(), g["z"]) < TOL
    assert golden_json(g, "frozen_json") == list(FROZEN)
    bad, worst, n = {}, (0.0, None), 0
    for name_, p in vae.named_parameters():
        if name_ in FROZEN:
            assert p.grad is None
            continue
        assert p.grad is not None and torch.isfinite(p.grad).all(), name_
        ref, ours = g[f"grad_{name_}"], grad_digest(p.grad)
        scale = max(np.abs(ref[2:]).max(), ref[1] / np.sqrt(p.numel()))
        e = max(np.abs(ours[2:] - ref[2:]).max() / scale, abs(ours[1] - ref[1]) / (ref[1] + 1e-30))
        worst, n = max(worst, (e, name_)), n + 1
        if not e <= TOL:
            bad[name_] = e
    print(f"[parity] Gaussian-head training {name} (fused loss {fused_loss}): {len(bad)} of {n} gradients outside {TOL:g}; "
          f"worst {worst[0]:.2e} ({worst[1]})")
    assert n == 176 and not bad, bad


@functools.lru_cache(maxsize=None)
def ragged_case(B, S, G, n_genes):
    """Module, inputs and the restatement's loss / outputs / gradients at one shape (computed once, never written to)."""
    vae, sd, cfg = build(n_genes, 300 + B)
    rng = np.random.default_rng(B * 100 + G)
    genes = rng.integers(0, n_genes + 1, (B, G)).astype(np.int64)          # repeats inside a cell: scatter-add into one row
    genes[:, -1] = genes[:, 0]
    counts = rng.poisson(0.9, (B, G)).astype(np.float32)
    counts[:, 0] += 1.0                                                    # no all-zero row (0 / 0 in the target)
    genes_s = rng.integers(0, n_genes + 1, (B, S)).astype(np.int64)
    counts_s = rng.poisson(0.9, (B, S)).astype(np.float32)
    counts_s[:, -max(1, S // 5):] = 0.0                                    # padding-style tokens (zero counts)
    zw = (0.3 * rng.standard_normal((B, 16, 16))).astype(np.float32)
    t = torch.from_numpy
    oracle = gauss_training_grads(sd, cfg, t(counts), t(genes), t(counts_s), t(genes_s), z_weight=t(zw))
    return vae, (counts, genes, counts_s, genes_s), zw, oracle


def oracle_gate(loss, mu, z, grads, oracle, what):
    loss_o, (mu_o, z_o), ref = oracle
    assert abs(float(loss) - float(loss_o)) <= TOL * abs(float(loss_o))
    assert max_abs_rel(z.cpu(), z_o) < TOL and max_abs_rel(mu.cpu(), mu_o) < TOL
    assert len(ref) == 176 and set(grads) == set(ref)
    bad, worst = {}, (0.0, None)
    for n, gr in grads.items():
        assert torch.isfinite(gr).all(), n
        e = max_abs_rel(gr.cpu(), ref[n]) if float(ref[n].abs().max()) > 0 else float(gr.abs().max())
        worst = max(worst, (e, n))
        if not e < TOL:
            bad[n] = e
    print(f"[parity] Gaussian-head training, {what}: worst of 176 gradient errors {worst[0]:.2e} ({worst[1]})")
    assert not bad, bad


@pytest.mark.parametrize("B,S,G,n_genes", [(5, 70, 130, 200), (9, 64, 65, 300), (1, 1, 1, 50), (3, 300, 1000, 2000)])
def test_gradients_match_oracle_on_ragged_sizes_with_a_gradient_through_z(B, S, G, n_genes):
    """Partial 16-gene steps, partial 64-token tiles, repeated genes in one cell, zero-count padding tokens, a loss term on z."""
    vae, inputs, zw, oracle = ragged_case(B, S, G, n_genes)
    loss, mu, z, grads = hip_step(vae, *inputs, z_weight=zw)
    oracle_gate(loss, mu, z, grads, oracle, f"B={B} S={S} G={G}")


@pytest.mark.parametrize("shape,split", [((200, 150, 300, 400), ((3, 2), (2, 2))), ((257, 200, 450, 600), ((8, 1), (4, 1)))],
                         ids=["B200-S150-G300", "B257-S200-G450"])
def test_multi_tile_walks_match_oracle(shape, split):
    """A workgroup walks several 64-gene tiles: the new accumulators (d Wc tiles, P, Q) are carried across tiles, the per-cell
    rotation of the walk wraps, the last chunk is shorter than the others."""
    from scldm_amd.vae import train_split
    B, S, G, n_genes = shape
    assert train_split(B, S, G) == split
    vae, inputs, zw, oracle = ragged_case(*shape)
    loss, mu, z, grads = hip_step(vae, *inputs, z_weight=zw)
    oracle_gate(loss, mu, z, grads, oracle, f"multi-tile B={B} S={S} G={G} (decoder {split[0]}, pooling {split[1]})")


def test_ordered_mode_is_bit_reproducible_and_equals_the_atomic_mode_outside_the_table():
    vae, inputs, zw, oracle = ragged_case(5, 70, 130, 200)
    try:
        vae.deterministic = True
        loss, mu, z, g1 = hip_step(vae, *inputs, z_weight=zw)
        assert vae.last_table_gradient_mode == "ordered"
        oracle_gate(loss, mu, z, g1, oracle, "ordered B=5 S=70 G=130")
        _, _, _, g2 = hip_step(vae, *inputs, z_weight=zw)
    finally:
        vae.deterministic = False
    assert len(g1) == 176
    diff = [n for n in g1 if not torch.equal(g1[n], g2[n])]
    assert not diff, diff
    _, _, _, ga = hip_step(vae, *inputs, z_weight=zw)
    assert vae.last_table_gradient_mode == "atomic"
    diff = [n for n in g1 if n != TABLE and not torch.equal(g1[n], ga[n])]
    assert not diff, diff
    assert max_abs_rel(ga[TABLE].cpu(), g1[TABLE].cpu()) < TOL


def test_recon_loss_backward_entry_and_autograd():
    from scldm_amd import _lib
    from scldm_amd.distributions import gaussian_recon_loss
    L = _lib.lib()
    rng = np.random.default_rng(11)
    for B, G in [(1, 1), (3, 33), (2, 1025), (5, 4099)]:
        counts = cu(rng.poisson(0.7, (B, G)).astype(np.float32))
        counts[:, 0] += 1.0
        mu = cu(rng.standard_normal((B, G)).astype(np.float32))
        gout = cu(rng.standard_normal(B).astype(np.float32))
        dmu = torch.empty_like(mu)
        assert L.scldm_gaussian_recon_loss_bwd(counts.data_ptr(), mu.data_ptr(), gout.data_ptr(), B, G, 1e4, dmu.data_ptr(),
                                               torch.cuda.current_stream().cuda_stream) == 0
        y = torch.log1p(counts.double() / counts.double().sum(1, keepdim=True) * 1e4)
        ref = -2.0 * (y - mu.double()) * gout.double()[:, None]
        assert max_abs_rel(dmu.cpu(), ref.cpu()) < 1e-5, (B, G)
        m = mu.clone().requires_grad_(True)
        loss = gaussian_recon_loss(counts, m)
        assert loss.requires_grad and torch.equal(loss.detach(), gaussian_recon_loss(counts, mu))      # unchanged values
        (loss * gout).sum().backward()
        assert torch.equal(m.grad, dmu)
        with torch.no_grad():
            assert not gaussian_recon_loss(counts, m).requires_grad
    assert L.scldm_gaussian_recon_loss_bwd(None, None, None, 1, 1, 1e4, None, None) == -1


def test_refusals():
    from scldm_amd import _lib
    from test_gpu_vae import build as build_nb
    L = _lib.lib()
    g = load_golden("gauss_train_small")
    args = (cu(g["counts"]), cu(g["genes"]), cu(g["library_size"]), cu(g["counts_subset"]), cu(g["genes_subset"]))
    vae, sd, cfg = build(int(g["n_genes"]), int(g["seed"]))
    vae.train_gaussian_head = False                                 # switch off: as before the head had a backward
    with pytest.raises(NotImplementedError, match="Gaussian"):
        vae(*args)
    vae.train_gaussian_head = True
    for prec in ("fp16", "bf16"):
        vae.precision = prec
        with pytest.raises(NotImplementedError, match="fp32"):
            vae(*args)
    vae.precision = "fp32"
    with torch.no_grad():
        p0, z0 = vae(*args)
    p1, z1 = vae(*args)
    assert not p0["mu"].requires_grad and p1["mu"].requires_grad and torch.equal(p1["mu"], p0["mu"]) and torch.equal(z1, z0)
    # the Gaussian training entries on a negative-binomial handle
    gn, nv, _, _ = build_nb("vae_small")
    nv.decode(cu(gn["z"]), cu(gn["genes"]), cu(gn["library_size"]))      # (builds and loads the handle)
    hn = nv._handle
    B, G = gn["genes"].shape
    S = gn["genes_subset"].shape[1]
    p = lambda t: t.data_ptr()
    cs, gs, genes = cu(gn["counts_subset"]), cu(gn["genes_subset"]), cu(gn["genes"])
    out, zb = torch.empty(B, G, device="cuda"), torch.empty(B, 16, 16, device="cuda")
    ws = torch.empty(1 << 24, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    assert L.scldm_vae_train_gaussian_forward(hn, p(cs), p(gs), B, S, p(genes), G, p(out), p(zb), p(ws), p(ws), st) == -1
    assert b"negative-binomial" in L.scldm_last_error()
    w, keep = nv._weights_struct(lambda t: t.data_ptr())
    assert L.scldm_vae_train_gaussian_backward(hn, C.byref(w), C.byref(w), p(cs), p(gs), B, S, p(genes), G, p(out), p(zb), p(out), p(zb),
                                               p(ws), p(ws), None, None, 0, None, st) == -1
    assert b"negative-binomial" in L.scldm_last_error()
    torch.cuda.synchronize()

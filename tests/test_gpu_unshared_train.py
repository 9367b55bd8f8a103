"""GPU parity of TRAINING the unshared-theta NB head (`train_unshared_theta = True`; decoder_name negative_binomial_unshared_theta:
params is Linear(32, 2), theta = exp of its second output, one dispersion per cell and gene): scldm_vae_train_forward_ex /
_backward_ex / _backward_ordered on such a handle (wide::dec_gene_bwd_nb2_kernel) through the autograd binding, against
  (a) digests of the REFERENCE's own autograd gradients of all 174 trainable parameters (tests/golden/vae_train_unshared_*.npz), and
  (b) autograd over the CPU oracle (oracle/vae_train.py, unchanged) on ragged sizes, multi-tile walks, with a gradient through z,
      and with each of the two gradient streams alone.
fp32 tolerance: the rule of tests/test_gpu_vae_train.py - 1e-4 of each tensor's scale (max |entry|, or l2 / sqrt(numel) for the
digests).  No tensor is excused; the (2,) head bias gradient is gated as one tensor (entry 0 is analytically zero, entry 1 is not).
fp16: the gate of tests/test_gpu_vae_train_fp16.py (its helpers, imported) - every gradient within 1.5 x the error of the oracle run
with matmul operands rounded to 10 bits, both against the exact oracle; the 50-gene fixture at that file's (3.0, 2.0) allowance."""
import functools
import types

import numpy as np
import pytest
import torch

from conftest import golden_json, load_golden, max_abs_rel
from oracle.train import grad_digest
from oracle.vae import VAEConfig
from oracle.vae_train import FROZEN, log_nb_positive as log_nb_oracle, vae_forward, vae_training_grads
from oracle.weights import make_state_dict
from test_abi_cpu import _build_vae
from test_gpu_vae_train import build as build_shared, cu, hip_step
from test_gpu_vae_train_fp16 import check_gate, errors, oracles, rel_l2

pytestmark = pytest.mark.gpu
TOL = 1e-4
TABLE = "input_layer.gene_embedding.weight"
BIAS, WEIGHT = "decoder_head.params.bias", "decoder_head.params.weight"
FIXTURES = ["vae_train_unshared_small", "vae_train_unshared_2000"]


def build(n_genes, seed, switch=True):
    vae = _build_vae(n_genes, shared_theta=False)
    sd = make_state_dict({k: tuple(v.shape) for k, v in vae.state_dict().items()}, seed)
    vae.load_state_dict(sd, strict=True)
    vae = vae.cuda().train()
    vae.train_unshared_theta = switch
    return vae, sd, VAEConfig(n_genes=n_genes)


def grads_of(vae):
    return {k: p.grad.clone() for k, p in vae.named_parameters() if p.grad is not None}


def golden_inputs(g):
    return g["counts"], g["genes"], g["library_size"], g["counts_subset"], g["genes_subset"]


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("fused_loss", [False, True])
def test_gradients_match_reference_digests(name, fused_loss):
    g = load_golden(name)
    vae, sd, cfg = build(int(g["n_genes"]), int(g["seed"]))
    loss, params, z = hip_step(vae, *golden_inputs(g), fused_loss=fused_loss)
    assert set(params) == {"mu", "theta"} and params["mu"].requires_grad and params["theta"].requires_grad
    print(f"[parity] {name} (fused loss {fused_loss}): loss {float(loss):.4f} (reference {float(g['loss']):.4f})")
    assert abs(float(loss) - float(g["loss"])) <= TOL * abs(float(g["loss"]))
    assert max_abs_rel(params["mu"].detach().cpu(), g["mu"]) < TOL and max_abs_rel(params["theta"].detach().cpu(), g["theta"]) < TOL
    assert max_abs_rel(z.cpu(), g["z"]) < TOL
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
    print(f"[parity] unshared-theta training {name} (fused loss {fused_loss}): {len(bad)} of {n} gradients outside {TOL:g}; "
          f"worst {worst[0]:.2e} ({worst[1]}); d head bias {vae.decoder_head.params.bias.grad.tolist()}")
    assert n == 174 and not bad, bad


def ragged_inputs(B, S, G, n_genes):
    rng = np.random.default_rng(B * 100 + G)
    genes = rng.integers(0, n_genes + 1, (B, G)).astype(np.int64)          # repeats inside a cell: scatter-add into one row
    genes[:, -1] = genes[:, 0]
    counts = rng.poisson(0.9, (B, G)).astype(np.float32)
    genes_s = rng.integers(0, n_genes + 1, (B, S)).astype(np.int64)
    counts_s = rng.poisson(0.9, (B, S)).astype(np.float32)
    counts_s[:, -max(1, S // 5):] = 0.0                                    # padding-style tokens (zero counts)
    lib = (counts.sum(1, keepdims=True) + 1.0).astype(np.float32)
    zw = (0.3 * rng.standard_normal((B, 16, 16))).astype(np.float32)
    return (counts, genes, lib, counts_s, genes_s), zw


@functools.lru_cache(maxsize=None)
def ragged_case(B, S, G, n_genes):
    """Module, inputs and the oracle's loss / outputs / gradients at one shape (computed once, never written to)."""
    vae, sd, cfg = build(n_genes, 300 + B)
    inputs, zw = ragged_inputs(B, S, G, n_genes)
    t = torch.from_numpy
    oracle = vae_training_grads(sd, cfg, *(t(a) for a in inputs), z_weight=t(zw))
    return vae, sd, cfg, inputs, zw, oracle


def oracle_gate(loss, params, z, grads, oracle, what):
    loss_o, (mu_o, theta_o, z_o), ref = oracle
    assert abs(float(loss) - float(loss_o)) <= TOL * abs(float(loss_o))
    assert max_abs_rel(z.cpu(), z_o) < TOL and max_abs_rel(params["mu"].detach().cpu(), mu_o) < TOL
    assert max_abs_rel(params["theta"].detach().cpu(), theta_o) < TOL
    assert len(ref) == 174 and set(grads) == set(ref)
    bad, worst = {}, (0.0, None)
    for n, gr in grads.items():
        assert torch.isfinite(gr).all(), n
        e = max_abs_rel(gr.cpu(), ref[n]) if float(ref[n].abs().max()) > 0 else float(gr.abs().max())
        worst = max(worst, (e, n))
        if not e < TOL:
            bad[n] = e
    print(f"[parity] unshared-theta training, {what}: worst of 174 gradient errors {worst[0]:.2e} ({worst[1]})")
    assert not bad, bad


@pytest.mark.parametrize("B,S,G,n_genes", [(1, 1, 1, 50), (5, 70, 130, 200), (9, 64, 65, 300), (3, 300, 1000, 2000)])
def test_gradients_match_oracle_on_ragged_sizes_with_a_gradient_through_z(B, S, G, n_genes):
    """Partial 16-gene steps, partial 64-token tiles, repeated genes in one cell, zero-count padding tokens, a loss term on z."""
    vae, sd, cfg, inputs, zw, oracle = ragged_case(B, S, G, n_genes)
    loss, params, z = hip_step(vae, *inputs, z_weight=zw)
    oracle_gate(loss, params, z, grads_of(vae), oracle, f"B={B} S={S} G={G}")


@pytest.mark.parametrize("shape,split", [((200, 150, 300, 400), ((3, 2), (2, 2))), ((257, 200, 450, 600), ((8, 1), (4, 1)))],
                         ids=["B200-S150-G300", "B257-S200-G450"])
def test_multi_tile_walks_match_oracle(shape, split):
    """A workgroup walks several 64-gene tiles: the new running sums (C1, head row 1, the second bias) are carried across tiles, the
    per-cell rotation of the walk wraps, the last chunk is shorter than the others."""
    from scldm_amd.vae import train_split
    B, S, G, n_genes = shape
    assert train_split(B, S, G) == split
    vae, sd, cfg, inputs, zw, oracle = ragged_case(*shape)
    loss, params, z = hip_step(vae, *inputs, z_weight=zw)
    oracle_gate(loss, params, z, grads_of(vae), oracle, f"multi-tile B={B} S={S} G={G} (decoder {split[0]}, pooling {split[1]})")


@pytest.mark.parametrize("stream", ["theta", "mu"])
def test_each_gradient_stream_alone(stream):
    """A loss through theta only (d mu absent: the softmax-logit stream d0 is zero) and one through mu only (d theta absent: d1 is
    zero), against the oracle with the same loss.  A kernel that drops or swaps the two head rows cannot pass both."""
    vae, sd, cfg, inputs, zw, _ = ragged_case(5, 70, 130, 200)
    counts = inputs[0]

    def loss_of(mu, theta, x):
        if stream == "theta":
            return (-log_nb_oracle(x, mu.detach(), theta)).sum(dim=1).mean()
        return (-log_nb_oracle(x, mu, theta.detach())).sum(dim=1).mean()

    t = torch.from_numpy
    p = {k: v.clone().requires_grad_(k not in FROZEN) for k, v in sd.items()}
    mu_o, theta_o, z_o = vae_forward(p, cfg, *(t(a) for a in inputs[1:]))
    loss_o = loss_of(mu_o, theta_o, t(counts))
    loss_o.backward()
    ref = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in p.items() if k not in FROZEN}
    for q in vae.parameters():
        q.grad = None
    params, z = vae(*(cu(a) for a in inputs))
    loss = loss_of(params["mu"], params["theta"], cu(counts))
    loss.backward()
    oracle_gate(loss.detach(), params, z.detach(), grads_of(vae), (loss_o.detach(), (mu_o.detach(), theta_o.detach(), z_o.detach()), ref),
                f"{stream} stream alone, B=5 S=70 G=130")
    w, b = vae.decoder_head.params.weight.grad, vae.decoder_head.params.bias.grad
    dead, live = (0, 1) if stream == "theta" else (1, 0)      # the absent stream's head row gets exactly nothing
    assert float(w[live].abs().max()) > 0
    assert float(w[dead].abs().max()) == 0.0 and float(b[dead]) == 0.0


def test_ordered_mode_is_bit_reproducible_and_equals_the_atomic_mode_outside_the_table():
    vae, sd, cfg, inputs, zw, oracle = ragged_case(5, 70, 130, 200)
    try:
        vae.deterministic = True
        loss, params, z = hip_step(vae, *inputs, z_weight=zw)
        g1 = grads_of(vae)
        assert vae.last_table_gradient_mode == "ordered"
        oracle_gate(loss, params, z, g1, oracle, "ordered B=5 S=70 G=130")
        hip_step(vae, *inputs, z_weight=zw)
        g2 = grads_of(vae)
    finally:
        vae.deterministic = False
    assert len(g1) == 174
    diff = [n for n in g1 if not torch.equal(g1[n], g2[n])]
    assert not diff, diff
    hip_step(vae, *inputs, z_weight=zw)
    ga = grads_of(vae)
    assert vae.last_table_gradient_mode == "atomic"
    diff = [n for n in g1 if n != TABLE and not torch.equal(g1[n], ga[n])]
    assert not diff, diff
    assert max_abs_rel(ga[TABLE].cpu(), g1[TABLE].cpu()) < TOL


# ---- fp16 ------------------------------------------------------------------------------------------------------------------------
def fp16_errors(vae, loss, params, z, exact, tf32):
    """errors() of test_gpu_vae_train_fp16.py (which leaves the head bias out: zero on the shared head) plus the second bias entry,
    which is large and real here; the first entry is the analytically zero one that check_gate bounds."""
    errs = errors(vae, loss, params["mu"], z, exact, tf32)
    errs["theta"] = (rel_l2(params["theta"], exact[1][1]), rel_l2(tf32[1][1], exact[1][1]))
    b, be, bt = vae.decoder_head.params.bias.grad, exact[2][BIAS], tf32[2][BIAS]
    errs[BIAS + "[1]"] = (rel_l2(b[1:], be[1:]), rel_l2(bt[1:], be[1:]))
    return errs


def gate(vae, errs, g_exact, what, factor, worst_factor):
    theta = errs.pop("theta")
    print(f"[parity] {what}: theta rel-L2 fp16 {theta[0]:.2e} / TF32-operand oracle {theta[1]:.2e}")
    assert theta[0] <= factor * theta[1] + 1e-5
    # (check_gate reads the head bias gradient as one number: hand it the entry that is mathematically zero)
    proxy = types.SimpleNamespace(decoder_head=types.SimpleNamespace(params=types.SimpleNamespace(
        bias=types.SimpleNamespace(grad=vae.decoder_head.params.bias.grad[0]))))
    return check_gate(proxy, errs, g_exact, what, factor, worst_factor)


_ORACLES = {}


def fp16_case(name):
    if name not in _ORACLES:
        if name in FIXTURES:
            g = load_golden(name)
            vae, sd, cfg = build(int(g["n_genes"]), int(g["seed"]))
            inputs, zw = golden_inputs(g), None
        else:
            vae, sd, cfg, inputs, zw, _ = ragged_case(5, 70, 130, 200)
        _ORACLES[name] = (vae, inputs, zw, oracles(sd, cfg, *inputs, zw))
    return _ORACLES[name]


@pytest.mark.parametrize("name", FIXTURES + ["B5-S70-G130"])
def test_fp16_training_is_in_the_references_tf32_class(name):
    vae, inputs, zw, (exact, tf32) = fp16_case(name)
    try:
        vae.precision = "fp16"
        flag = vae.found_inf_flag()
        loss, params, z = hip_step(vae, *inputs, z_weight=zw)
        errs = fp16_errors(vae, loss, params, z, exact, tf32)
        worst16 = gate(vae, errs, exact[2], f"unshared-theta fp16 training {name}", *((3.0, 2.0) if name == "vae_train_unshared_small" else (1.5, 1.5)))
        assert float(flag) == 0.0
    finally:
        vae.precision = "fp32"
    loss32, params32, z32 = hip_step(vae, *inputs, z_weight=zw)
    worst32 = max(v[0] for k, v in fp16_errors(vae, loss32, params32, z32, exact, tf32).items() if k not in ("loss", "mu", "z", "theta"))
    print(f"[parity] unshared-theta training {name}: worst gradient rel-L2 fp32 {worst32:.2e} vs fp16 {worst16:.2e}")
    assert 5 * worst32 <= worst16      # the fp16 operands are really used


def test_fp16_overflow_sets_the_flag():
    """The construction of test_overflow_sets_the_flag_and_adamw_skips_the_step (tests/test_gpu_vae_train_fp16.py) on this head: gene
    embeddings and the decoder's two c_proj weights times 1e-3, head row 0 scaled to |w| <= 1000 (row 1 stays: theta = exp(l1) must
    not overflow in the forward), so d y = d0 w0 + ... of the scaled backward leaves the fp16 range.  The flag reads 1 and the next
    clean step resets it.  (A numeric inf, not a GPU fault.)"""
    g = load_golden("vae_train_unshared_2000")
    vae, sd, cfg = build(int(g["n_genes"]), int(g["seed"]))
    inputs = golden_inputs(g)
    clean = {k: v.clone() for k, v in vae.state_dict().items()}
    with torch.no_grad():
        vae.input_layer.gene_embedding.weight.mul_(1e-3)
        vae.decoder.decoder_cross_attention.attn.c_proj.weight.mul_(1e-3)
        vae.decoder.decoder_cross_attention.mlp.c_proj.weight.mul_(1e-3)
        w = vae.decoder_head.params.weight
        w[0].mul_(1e3 / float(w[0].abs().max()))
        assert all(float(p.abs().max()) < 65504 for p in vae.parameters())
    vae.precision = "fp16"
    flag = vae.found_inf_flag()
    loss, params, z = hip_step(vae, *inputs)
    assert torch.isfinite(params["mu"]).all() and torch.isfinite(params["theta"]).all() and torch.isfinite(loss)
    assert float(flag) == 1.0
    with torch.no_grad():
        vae.load_state_dict(clean)
    hip_step(vae, *inputs)
    assert float(flag) == 0.0 and all(torch.isfinite(p.grad).all() for p in vae.parameters() if p.grad is not None)


# ---- the switch ------------------------------------------------------------------------------------------------------------------
def test_switch_and_refusals():
    g = load_golden("vae_train_unshared_small")
    args = tuple(cu(a) for a in golden_inputs(g))
    vae, sd, cfg = build(int(g["n_genes"]), int(g["seed"]), switch=False)
    for prec in ("fp32", "fp16", "bf16"):                          # switch off: as before the head had a backward
        vae.precision = prec
        with pytest.raises(NotImplementedError, match="shared-theta") as ei:
            vae(*args)
        assert "train_unshared_theta" in str(ei.value)
    vae.train_unshared_theta = True
    vae.precision = "bf16"
    with pytest.raises(NotImplementedError, match="fp32 or fp16"):
        vae(*args)
    vae.precision = "fp32"
    with torch.no_grad():
        p0, z0 = vae(*args)
    p1, z1 = vae(*args)
    assert not p0["mu"].requires_grad and not p0["theta"].requires_grad and not z0.requires_grad
    assert p1["mu"].requires_grad and p1["theta"].requires_grad and z1.requires_grad
    assert torch.equal(p1["mu"], p0["mu"]) and torch.equal(p1["theta"], p0["theta"]) and torch.equal(z1, z0)


def test_shared_theta_module_is_unaffected_by_the_switch():
    g = load_golden("vae_train_small")
    vae, sd, cfg = build_shared(int(g["n_genes"]), int(g["seed"]))
    inputs = golden_inputs(g)
    vae.deterministic = True
    out = []
    for switch in (False, True):
        vae.train_unshared_theta = switch
        loss, params, z = hip_step(vae, *inputs)
        assert vae.last_table_gradient_mode == "ordered"
        out.append((loss, params["mu"].detach(), params["theta"].detach(), z, grads_of(vae)))
    (l0, m0, t0, z0, g0), (l1, m1, t1, z1, g1) = out
    assert torch.equal(l0, l1) and torch.equal(m0, m1) and torch.equal(t0, t1) and torch.equal(z0, z1)
    assert len(g0) == 175 and set(g0) == set(g1) and all(torch.equal(g0[n], g1[n]) for n in g0)


def test_short_training_loop_reduces_the_loss():
    """B = 8 at G = 2 000, S = 700: 12 AdamW steps on a fixed batch in fp32."""
    from scldm_amd.datamodule import tokenize_cells_expressed
    from scldm_amd.distributions import log_nb_positive
    from scldm_amd.optim import AdamW
    G, S, B, n_genes = 2000, 700, 8, 2000
    vae, sd, cfg = build(n_genes, 402)
    with torch.no_grad():
        vae.input_layer.gene_embedding.weight.normal_(0, 1.0)
        vae.encoder.ca_layer.inducing_points.normal_(0, 1.0)
    rng = np.random.default_rng(6)
    rate = rng.gamma(0.3, 2.0, (1, G)).astype(np.float32)
    counts = rng.poisson(rate * rng.uniform(0.5, 1.5, (B, 1))).astype(np.float32)
    genes = np.tile(np.arange(G, dtype=np.int64), (B, 1))
    tok = tokenize_cells_expressed(cu(counts), cu(genes[0]), S, n_genes)
    lib = cu(counts).sum(1, keepdim=True)
    opt = AdamW(vae.parameters(), lr=2e-3)
    losses = []
    for _ in range(12):
        opt.zero_grad(set_to_none=True)
        params, z = vae(cu(counts), cu(genes), lib, tok["counts_subset"], tok["genes_subset"])
        loss = (-log_nb_positive(cu(counts), params["mu"], params["theta"])).sum(dim=1).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss))
    print(f"[parity] unshared-theta training loop (B=8, G=2000, S=700): loss {losses[0]:.1f} -> {losses[-1]:.1f}")
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]

"""GPU gates of the ORDERED table gradients of the TransformerVAE training backward (`TransformerVAE.deterministic`,
scldm_vae_train_backward_ordered): the gradients of gene_embedding and theta formed by a fixed-order segmented sum instead of float
atomics.
  1. routing: where every table row receives at most one contribution the two modes agree bit for bit, for every parameter;
  2. parity: the reference's autograd digests at the project's fp32 gate (1e-4), and fp16 ordered against fp16 atomic;
  3. run-to-run bit equality of all 175 gradients where the atomics collide, in fp32 and fp16, with the oracle check of the fp32 step;
  4. the switches; 5. the fp16 overflow flag.
The oracle comparison of (3) is made for the fp32 step only: 1e-4 is the project's gate for exact-fp32 arithmetic, which fp16 operands
(10 mantissa bits, errors near 1e-3) cannot meet in either mode; the fp16 ordered step is pinned to the fp16 atomic one in (2) - bit
equal outside the two tables - whose accuracy test_gpu_vae_train_fp16.py gates against the TF32-operand oracle.
All shapes here give every workgroup of the gene-axis kernels one 64-token tile; the row buffers of workgroups that walk several
tiles (the bench and production splits) are checked in test_gpu_vae_train_multitile.py."""
import numpy as np
import pytest
import torch

from conftest import golden_json, load_golden, max_abs_rel
from oracle.train import grad_digest
from oracle.vae_train import FROZEN, vae_training_grads
from test_gpu_vae_train import BIAS, TOL, build, hip_step

pytestmark = pytest.mark.gpu
TABLES = ("input_layer.gene_embedding.weight", "decoder_head.theta.weight")


def grads(vae, inputs, prec="fp32", deterministic=True, zw=None):
    vae.precision, vae.deterministic = prec, deterministic
    loss, params, z = hip_step(vae, *inputs, z_weight=zw)
    assert vae.last_table_gradient_mode == ("ordered" if deterministic else "atomic")
    g = {n: p.grad.clone() for n, p in vae.named_parameters() if p.grad is not None}
    assert set(g) == {n for n, _ in vae.named_parameters() if n not in FROZEN}
    return g, loss, params, z


def golden_inputs(name):
    g = load_golden(name)
    vae, sd, cfg = build(int(g["n_genes"]), int(g["seed"]))
    return g, vae, (g["counts"], g["genes"], g["library_size"], g["counts_subset"], g["genes_subset"])


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_disjoint_rows_route_bit_for_bit(prec):
    """Cell 0 decodes genes 0..99 and encodes 200..239, cell 1 decodes 100..199 and encodes 240..279: no table row is hit twice, so a
    sum of one addend must equal the atomic add of that addend - every entry reaches the row of its gene id, and only that row."""
    n_genes, B, G, S = 300, 2, 100, 40
    vae, sd, cfg = build(n_genes, 77)
    rng = np.random.default_rng(3)
    genes = np.arange(B * G, dtype=np.int64).reshape(B, G)
    genes_s = (200 + np.arange(B * S, dtype=np.int64)).reshape(B, S)
    counts = rng.poisson(0.9, (B, G)).astype(np.float32)
    counts_s = (1.0 + rng.poisson(0.9, (B, S))).astype(np.float32)
    lib = (counts.sum(1, keepdims=True) + 1.0).astype(np.float32)
    inputs = (counts, genes, lib, counts_s, genes_s)
    go, *_ = grads(vae, inputs, prec, True)
    ga, *_ = grads(vae, inputs, prec, False)
    for n in ga:
        assert torch.equal(go[n], ga[n]), n
    emb = go[TABLES[0]]
    assert float(emb[:280].abs().max()) > 0 and float(emb[280:].abs().max()) == 0.0      # rows 280 .. 300: used by nobody
    assert float(go[TABLES[1]][200:].abs().max()) == 0.0                                  # theta: decoded genes only


@pytest.mark.parametrize("name", ["vae_train_small", "vae_train_2000"])
def test_ordered_gradients_match_reference_digests(name):
    """The comparison of test_gpu_vae_train.test_gradients_match_reference_digests, in ordered mode."""
    g, vae, inputs = golden_inputs(name)
    _, loss, params, z = grads(vae, inputs, "fp32", True)
    assert abs(float(loss) - float(g["loss"])) <= TOL * abs(float(g["loss"]))
    assert max_abs_rel(params["mu"].detach().cpu(), g["mu"]) < TOL and max_abs_rel(z.cpu(), g["z"]) < TOL
    assert golden_json(g, "frozen_json") == list(FROZEN)
    wn = g["grad_decoder_head.params.weight"][1]
    bad = {}
    for name_, p in vae.named_parameters():
        if name_ in FROZEN:
            assert p.grad is None
            continue
        assert p.grad is not None and torch.isfinite(p.grad).all(), name_
        ref, ours = g[f"grad_{name_}"], grad_digest(p.grad)
        if name_ == BIAS:
            if not abs(ours[0]) <= 1e-3 * wn:
                bad[name_] = ours[0]
            continue
        scale = max(np.abs(ref[2:]).max(), ref[1] / np.sqrt(p.numel()))
        e = max(np.abs(ours[2:] - ref[2:]).max() / scale, abs(ours[1] - ref[1]) / (ref[1] + 1e-30))
        if not e <= TOL:
            bad[name_] = e
    print(f"[parity] VAE training {name}, ordered table gradients: {len(bad)} of 175 gradients outside {TOL:g}")
    assert not bad, bad


@pytest.mark.parametrize("name", ["vae_train_small", "vae_train_2000"])
def test_fp16_ordered_against_fp16_atomic(name):
    """The kernels are otherwise the same: every tensor but the two tables bit-equal; the tables hold the same addends in another
    order (fp32 sums of at most a few hundred terms: 1e-4 of the tensor's largest entry is orders above their rounding)."""
    g, vae, inputs = golden_inputs(name)
    go, *_ = grads(vae, inputs, "fp16", True)
    ga, *_ = grads(vae, inputs, "fp16", False)
    for n in ga:
        if n in TABLES:
            e = float((go[n] - ga[n]).abs().max()) / float(ga[n].abs().max())
            print(f"[parity] VAE fp16 training {name}: {n} ordered vs atomic {e:.2e} of the largest entry")
            assert e <= 1e-4, (n, e)
        else:
            assert torch.equal(go[n], ga[n]), n
    assert float(vae.found_inf_flag()) == 0.0


def collide_case(case):
    """(vae, sd, cfg, inputs, z_weight) of the four shapes where contributions to a table row collide"""
    B, G, S, n_genes = {"a": (37, 200, 70, 12), "b": (3, 1000, 300, 2000), "c": (1, 1, 1, 50), "d": (9, 65, 64, 300)}[case]
    vae, sd, cfg = build(n_genes, 500 + B)
    rng = np.random.default_rng(B * 100 + G)
    genes = rng.integers(0, n_genes + 1, (B, G)).astype(np.int64)
    counts = rng.poisson(0.9, (B, G)).astype(np.float32)
    genes_s = rng.integers(0, n_genes + 1, (B, S)).astype(np.int64)
    counts_s = rng.poisson(0.9, (B, S)).astype(np.float32)
    if case == "d":
        counts_s[:, -(S // 5):] = 0.0
    lib = (counts.sum(1, keepdims=True) + 1.0).astype(np.float32)
    zw = (0.3 * rng.standard_normal((B, 16, 16))).astype(np.float32)
    return vae, sd, cfg, (counts, genes, lib, counts_s, genes_s), zw


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("case", ["a", "b", "c", "d"])
def test_four_runs_are_bit_equal_where_the_atomics_collide(case, prec):
    """(a) 13 table rows hit hundreds of times each, genes repeated inside cells, 37 cells (no whole four-cell wave); (b) several
    chunks per cell, one 64-gene tile each (16 decoder and 5 pooling workgroups per cell), with a ragged last tile; (c) one cell, one
    gene, one token; (d) a fifth of the encoder tokens with zero counts (left out of the index).  Default two-stream overlap.  Every
    workgroup here walks ONE tile; workgroups that walk several are in test_gpu_vae_train_multitile.py."""
    vae, sd, cfg, inputs, zw = collide_case(case)
    first, loss, params, z = grads(vae, inputs, prec, True, zw)
    for run in range(3):
        again, *_ = grads(vae, inputs, prec, True, zw)
        diff = [n for n in first if not torch.equal(first[n], again[n])]
        assert not diff, (run, diff)
    if prec == "fp16":
        assert float(vae.found_inf_flag()) == 0.0
        return
    t = lambda a: torch.from_numpy(a)
    loss_o, (mu_o, th_o, z_o), ref = vae_training_grads(sd, cfg, *(t(a) for a in inputs), z_weight=t(zw))
    assert abs(float(loss) - float(loss_o)) <= TOL * abs(float(loss_o))
    assert max_abs_rel(z.cpu(), z_o) < TOL and max_abs_rel(params["mu"].detach().cpu(), mu_o) < TOL
    wn = float(ref["decoder_head.params.weight"].norm())
    bad, worst = {}, 0.0
    for n, gr in first.items():
        if n == BIAS:
            if not abs(float(gr)) <= 1e-3 * wn:
                bad[n] = float(gr)
            continue
        e = max_abs_rel(gr.cpu(), ref[n]) if float(ref[n].abs().max()) > 0 else float(gr.abs().max())
        worst = max(worst, e)
        if not e < TOL:
            bad[n] = e
    print(f"[parity] VAE training, ordered table gradients, case ({case}): worst gradient error {worst:.2e}")
    assert not bad, bad


def test_switches():
    g, vae, inputs = golden_inputs("vae_train_small")
    assert vae.deterministic is False and vae.last_table_gradient_mode is None
    ga, *_ = grads(vae, inputs, "fp32", False)
    assert vae.last_table_gradient_mode == "atomic"
    go, *_ = grads(vae, inputs, "fp32", True)
    for n in ga:
        if n not in TABLES:
            assert torch.equal(ga[n], go[n]), n
    vae.deterministic = False
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        hip_step(vae, *inputs)
        assert vae.last_table_gradient_mode == "ordered"
        gt = {n: p.grad.clone() for n, p in vae.named_parameters() if p.grad is not None}
    finally:
        torch.use_deterministic_algorithms(was)
    for n in go:
        assert torch.equal(gt[n], go[n]), n
    hip_step(vae, *inputs)
    assert vae.last_table_gradient_mode == "atomic"


def test_ordered_overflow_sets_the_flag_and_a_clean_step_resets_it():
    """The construction of test_gpu_vae_train_fp16.test_overflow_sets_the_flag_and_adamw_skips_the_step (every weight inside the fp16
    range, the scaled backward's d y outside it), in ordered mode.  (A numeric inf, not a GPU fault.)"""
    g, vae, inputs = golden_inputs("vae_train_2000")
    clean = {k: v.clone() for k, v in vae.state_dict().items()}
    with torch.no_grad():
        vae.input_layer.gene_embedding.weight.mul_(1e-3)
        vae.decoder.decoder_cross_attention.attn.c_proj.weight.mul_(1e-3)
        vae.decoder.decoder_cross_attention.mlp.c_proj.weight.mul_(1e-3)
        w = vae.decoder_head.params.weight
        w.mul_(1e3 / float(w.abs().max()))
        assert all(float(p.abs().max()) < 65504 for p in vae.parameters())
    vae.precision, vae.deterministic = "fp16", True
    flag = vae.found_inf_flag()
    loss, params, z = hip_step(vae, *inputs)
    assert vae.last_table_gradient_mode == "ordered"
    assert torch.isfinite(params["mu"]).all() and torch.isfinite(loss)
    assert float(flag) == 1.0
    with torch.no_grad():
        vae.load_state_dict(clean)
    hip_step(vae, *inputs)
    assert float(flag) == 0.0 and all(torch.isfinite(p.grad).all() for p in vae.parameters() if p.grad is not None)

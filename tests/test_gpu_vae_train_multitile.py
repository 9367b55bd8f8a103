"""GPU parity of the TransformerVAE training backward where a workgroup of the two gene-axis kernels (the per-gene decoder chain
`dec_gene_bwd_mfma2_kernel`, the pooling `enc_pool_bwd_kernel` / `enc_pool_bwd_rows_kernel`) walks SEVERAL 64-token tiles: the regime
of the bench and production steps (batch 32: 17 and 7 tiles; batch 512: 266 and 97), which the value-checked tests of
test_gpu_vae_train*.py never enter (their batches are small enough for one tile per workgroup).  What only a multi-tile walk runs:
the per-cell rotation of the walk with its two-step-ahead prefetch wrapping around, a partial sixteen-gene step in the middle of the
walk, the clamp of the prefetched slot, a last chunk shorter than the others, accumulators and the fp16 route's per-cell scale carried
over the whole walk, the ordered route's row buffers at that length.
  (a) three small shapes on both sides of the boundaries of the split (tests/test_vae_train_split_cpu.py lists them with their
      splits), random data as in the ragged tests, four routes each: fp32 / fp16 x atomic / ordered table gradients;
  (b) the production split itself, (266, 1) and (97, 1): 260 cells = four distinct cells x 65 copies in the order c0 c1 c2 c3 c0 ...
      (copies get different cell indices, so different rotations), each copy's z_weight divided by 65.  The loss and every gradient
      are then those of the four distinct cells alone (checked on the CPU in test_vae_train_split_cpu.py), which the oracle evaluates
      in a fraction of a second.
Every test first asks the library for the split (scldm_vae_train_split) and asserts the one it was designed for.  Gates: those of the
one-tile tests - fp32 1e-4 of each tensor's largest entry against autograd over the oracle; fp16 against the TF32-operand oracle."""
import numpy as np
import pytest
import torch

from conftest import max_abs_rel
from scldm_amd.vae import train_split
from test_gpu_vae_train import BIAS, TOL, build, cu, hip_step
from test_gpu_vae_train_fp16 import check_gate, errors, oracles
from test_gpu_vae_train_ordered import TABLES, grads
from test_vae_train_split_cpu import MULTITILE_SHAPES, PRODUCTION_SHAPE, PRODUCTION_SPLIT

pytestmark = pytest.mark.gpu
SHAPES = list(MULTITILE_SHAPES)
_CASES = {}


def case(shape):
    """(vae, inputs, z_weight, (exact oracle, TF32-operand oracle)) of one shape of (a): one module and one oracle evaluation per shape"""
    if shape not in _CASES:
        B, S, G, n_genes = shape
        vae, sd, cfg = build(n_genes, 300 + B)
        rng = np.random.default_rng(B * 100 + G)
        genes = rng.integers(0, n_genes + 1, (B, G)).astype(np.int64)          # repeats inside a cell: scatter-add into one row
        genes[:, -1] = genes[:, 0]
        counts = rng.poisson(0.9, (B, G)).astype(np.float32)
        genes_s = rng.integers(0, n_genes + 1, (B, S)).astype(np.int64)
        counts_s = rng.poisson(0.9, (B, S)).astype(np.float32)
        counts_s[:, -max(1, S // 5):] = 0.0                                    # padding-style tokens
        lib = (counts.sum(1, keepdims=True) + 1.0).astype(np.float32)
        zw = (0.3 * rng.standard_normal((B, 16, 16))).astype(np.float32)
        inputs = (counts, genes, lib, counts_s, genes_s)
        _CASES[shape] = (vae, inputs, zw, oracles(sd, cfg, *inputs, zw))
    return _CASES[shape]


def production_case():
    """The dentate shape's data (test_training_loop_at_the_dentate_shape_reduces_the_loss) for four cells, tiled to 260"""
    if "production" not in _CASES:
        from scldm_amd.datamodule import tokenize_cells_expressed
        B, S, G, n_genes = PRODUCTION_SHAPE
        k = 4
        vae, sd, cfg = build(n_genes, 401)       # gene embeddings and inducing points are drawn N(0, 1)
        with torch.no_grad():
            vae.decoder_head.theta.weight.fill_(1.0)       # the theta table at its reference init
        sd = {n: v.detach().cpu().clone() for n, v in vae.state_dict().items()}
        rng = np.random.default_rng(5)
        rate = rng.gamma(0.3, 2.0, (1, G)).astype(np.float32)
        counts = rng.poisson(rate * rng.uniform(0.5, 1.5, (k, 1))).astype(np.float32)
        genes = np.tile(np.arange(G, dtype=np.int64), (k, 1))
        tok = tokenize_cells_expressed(cu(counts), cu(genes[0]), S, n_genes)   # expressed genes in gene order, the tail at zero counts
        counts_s, genes_s = tok["counts_subset"].cpu().numpy(), tok["genes_subset"].cpu().numpy()
        assert (counts_s[:, -1] == 0).all() and int((counts_s > 0).sum(1).min()) > 64 * 8
        lib = counts.sum(1, keepdims=True).astype(np.float32)
        zw = (0.3 * rng.standard_normal((k, 16, 16))).astype(np.float32)
        four = (counts, genes, lib, counts_s, genes_s)
        rows = np.arange(B) % k                                                # c0 c1 c2 c3 c0 ...
        inputs = tuple(np.ascontiguousarray(a[rows]) for a in four)
        _CASES["production"] = (vae, inputs, np.ascontiguousarray(zw[rows] / (B // k)), oracles(sd, cfg, *four, zw), rows)
    return _CASES["production"]


def oracle_gate(g, loss, params, z, exact, what, rows=None):
    """The assertion block of test_gradients_match_oracle_on_ragged_sizes_with_a_gradient_through_z; `rows`: the oracle's cell of
    every row of the batch (the production case).  Returns (worst gradient error, its tensor)."""
    loss_o, (mu_o, _, z_o), ref = exact
    if rows is not None:
        mu_o, z_o = mu_o[rows], z_o[rows]
    assert abs(float(loss) - float(loss_o)) <= TOL * abs(float(loss_o))
    assert max_abs_rel(z.cpu(), z_o) < TOL and max_abs_rel(params["mu"].detach().cpu(), mu_o) < TOL
    wn = float(ref["decoder_head.params.weight"].norm())
    bad, worst = {}, (0.0, None)
    for n, gr in g.items():
        assert torch.isfinite(gr).all(), n
        if n == BIAS:
            if not abs(float(gr)) <= 1e-3 * wn:
                bad[n] = float(gr)
            continue
        e = max_abs_rel(gr.cpu(), ref[n]) if float(ref[n].abs().max()) > 0 else float(gr.abs().max())
        worst = max(worst, (e, n))
        if not e < TOL:
            bad[n] = e
    print(f"[parity] VAE training, multi-tile, {what}: worst gradient error {worst[0]:.2e} ({worst[1]})")
    assert not bad, bad
    return worst


def split_of(shape):
    B, S, G, _ = shape
    return train_split(B, S, G)


def what_of(shape, route):
    B, S, G, _ = shape
    dec, pool = split_of(shape)
    return f"B={B} S={S} G={G} (decoder {dec[0]} tiles x {dec[1]} chunks, pooling {pool[0]} x {pool[1]}), {route}"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B{}-S{}-G{}".format(*s))
def test_fp32_atomic_gradients_match_oracle(shape):
    assert split_of(shape) == MULTITILE_SHAPES[shape]
    vae, inputs, zw, (exact, _) = case(shape)
    g, loss, params, z = grads(vae, inputs, "fp32", False, zw)
    oracle_gate(g, loss, params, z, exact, what_of(shape, "fp32 atomic"))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B{}-S{}-G{}".format(*s))
def test_fp32_ordered_gradients_match_oracle_and_repeat_bit_for_bit(shape):
    assert split_of(shape) == MULTITILE_SHAPES[shape]
    vae, inputs, zw, (exact, _) = case(shape)
    g, loss, params, z = grads(vae, inputs, "fp32", True, zw)
    oracle_gate(g, loss, params, z, exact, what_of(shape, "fp32 ordered"))
    again, *_ = grads(vae, inputs, "fp32", True, zw)
    diff = [n for n in g if not torch.equal(g[n], again[n])]
    assert not diff, diff
    ga, *_ = grads(vae, inputs, "fp32", False, zw)
    diff = [n for n in g if n not in TABLES and not torch.equal(g[n], ga[n])]
    assert not diff, diff


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B{}-S{}-G{}".format(*s))
def test_fp16_gradients_are_in_the_tf32_class(shape):
    assert split_of(shape) == MULTITILE_SHAPES[shape]
    vae, inputs, zw, (exact, tf32) = case(shape)
    flag = vae.found_inf_flag()
    g, loss, params, z = grads(vae, inputs, "fp16", False, zw)
    check_gate(vae, errors(vae, loss, params["mu"], z, exact, tf32), exact[2], "multi-tile, " + what_of(shape, "fp16 atomic"), 3.0, 2.0)
    assert float(flag) == 0.0 and float(vae.found_inf_flag()) == 0.0


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B{}-S{}-G{}".format(*s))
def test_fp16_ordered_against_fp16_atomic(shape):
    """The rule of test_gpu_vae_train_ordered.test_fp16_ordered_against_fp16_atomic: bit-equal outside the two tables, the tables
    (the same addends in another order) within 1e-4 of the largest entry."""
    assert split_of(shape) == MULTITILE_SHAPES[shape]
    vae, inputs, zw, _ = case(shape)
    go, *_ = grads(vae, inputs, "fp16", True, zw)
    ga, *_ = grads(vae, inputs, "fp16", False, zw)
    for n in ga:
        if n in TABLES:
            e = float((go[n] - ga[n]).abs().max()) / float(ga[n].abs().max())
            print(f"[parity] VAE training, multi-tile, {what_of(shape, 'fp16')}: {n} ordered vs atomic {e:.2e} of the largest entry")
            assert e <= 1e-4, (n, e)
        else:
            assert torch.equal(go[n], ga[n]), n
    assert float(vae.found_inf_flag()) == 0.0


@pytest.mark.parametrize("deterministic", [False, True], ids=["atomic", "ordered"])
def test_fp32_gradients_match_oracle_at_the_production_split(deterministic):
    """266 decoder tiles = 1 063 sixteen-gene steps and 97 pooling tiles per workgroup, one workgroup per cell: what batch 512 runs."""
    assert split_of(PRODUCTION_SHAPE) == PRODUCTION_SPLIT
    vae, inputs, zw, (exact, _), rows = production_case()
    g, loss, params, z = grads(vae, inputs, "fp32", deterministic, zw)
    oracle_gate(g, loss, params, z, exact, what_of(PRODUCTION_SHAPE, "fp32 ordered" if deterministic else "fp32 atomic"), rows)
    if deterministic:
        again, *_ = grads(vae, inputs, "fp32", True, zw)
        diff = [n for n in g if not torch.equal(g[n], again[n])]
        assert not diff, diff


def test_fp16_gradients_are_in_the_tf32_class_at_the_production_split():
    """Gated at the factors of the small shapes (3 x per tensor, 2 x for the worst gradient), not at the 1.5 x of the 2 000-gene
    fixture: the batch holds FOUR distinct cells, so the cell-side gradients (the decoder trunk's LayerNorm vectors and attention
    weights) are sums over four cells of terms with large cancellation, and the ratio of two such errors spreads as on the small
    shapes whatever the split.  Measured on an MI355X (2026-10-19), fp32 inside 1e-4 throughout (1.5e-5): at this split the worst
    gradient is 1.20 x the TF32-operand oracle's and the largest per-tensor ratio 2.25 (decoder.decoder_layers.3.ln_1.weight; 5 of
    174 tensors above 1.5, all in the decoder trunk); the same four cells at ONE tile per workgroup give 1.74 / 1.64 / 1.04 / 0.70 x
    worst and 2.23 / 1.64 / 1.86 / 1.52 per tensor alone at batch 1, and 2.24 x worst and 2.50 per tensor together at batch 4 (the
    same figures with 1 and with 3 tiles per decoder workgroup).  The multi-tile walk adds nothing to the spread."""
    assert split_of(PRODUCTION_SHAPE) == PRODUCTION_SPLIT
    vae, inputs, zw, (exact, tf32), rows = production_case()
    flag = vae.found_inf_flag()
    g, loss, params, z = grads(vae, inputs, "fp16", False, zw)
    tile = lambda o: (o[0], (o[1][0][rows], o[1][1][rows], o[1][2][rows]), o[2])
    errs = errors(vae, loss, params["mu"], z, tile(exact), tile(tf32))
    worst = max((v[0], n) for n, v in errs.items() if n not in ("loss", "mu", "z"))
    print(f"[parity] VAE training, multi-tile, {what_of(PRODUCTION_SHAPE, 'fp16 atomic')}: worst gradient rel-L2 {worst[0]:.2e} ({worst[1]})")
    check_gate(vae, errs, exact[2], "multi-tile, " + what_of(PRODUCTION_SHAPE, "fp16 atomic"), 3.0, 2.0)
    assert float(flag) == 0.0

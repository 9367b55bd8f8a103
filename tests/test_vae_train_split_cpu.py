"""CPU-side checks of the split of the VAE training backward's two gene-axis kernels (scldm_vae_train_split: `chunks` workgroups per
cell, each walking `tiles` 64-token tiles), and of the identity the production-split GPU test rests on.
  1. the invariants of the split over batch sizes and axis lengths around every boundary;
  2. the shapes of tests/test_gpu_vae_train_multitile.py, each with the split it was designed for written next to it: if the default
     target of 512 workgroups moves, this fails here instead of the GPU tests going back to one tile per workgroup unnoticed;
  3. k distinct cells, each repeated R times with its z_weight divided by R, give the loss and every gradient of the k cells alone."""
import ctypes as C

import numpy as np
import torch

from conftest import load_golden
from oracle.vae import VAEConfig
from oracle.vae_train import vae_training_grads
from oracle.weights import make_state_dict
from test_abi_cpu import _build_vae
from test_gpu_vae_train import BIAS, TOL

# (B, S, G, n_genes): ((decoder tiles, chunks), (pooling tiles, chunks)) at the default target of 512 workgroups per kernel
MULTITILE_SHAPES = {
    (200, 150, 300, 400): ((3, 2), (2, 2)),      # last chunk shorter than the others (2 of 3 tiles, 1 of 2); last step: 12 valid tokens
    (257, 200, 450, 600): ((8, 1), (4, 1)),      # smallest B with one workgroup per cell; 29 steps, every rotation; 2 valid tokens
    (256, 130, 130, 200): ((2, 2), (2, 2)),      # the other side of 256 / 257; the last chunk is one tile of 2 tokens
}
PRODUCTION_SHAPE = (260, 6147, 17002, 17002)     # four distinct cells x 65 copies
PRODUCTION_SPLIT = ((266, 1), (97, 1))           # what batch 512 runs at G = 17 002, S = 6 147


def split(B, S, G):
    from scldm_amd.vae import train_split
    return train_split(B, S, G)


def test_split_invariants():
    for B in (1, 2, 31, 32, 255, 256, 257, 512, 65535):
        for n in (1, 63, 64, 65, 4096, 6147, 17002):
            dec, pool = split(B, n, n)
            assert dec == pool, (B, n, dec, pool)                      # the same rule and the same default target on both axes
            tiles, chunks = dec
            assert tiles >= 1 and chunks >= 1, (B, n, dec)
            assert chunks * tiles * 64 >= n, (B, n, dec)               # the workgroups cover the axis
            assert (chunks - 1) * tiles * 64 < n, (B, n, dec)          # no workgroup starts past its end
            assert chunks * B <= max(512, B), (B, n, dec)              # at most one full round, or one workgroup per cell


def test_the_two_axes_are_split_independently():
    assert split(200, 150, 300) == ((3, 2), (2, 2))
    assert split(200, 300, 150) == ((2, 2), (3, 2))


def test_split_rejects_empty_shapes_and_needs_no_handle():
    from scldm_amd import _lib
    L = _lib.lib()
    out = (C.c_int * 4)(-7, -7, -7, -7)
    for B, S, G in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-3, 5, 5)):
        assert L.scldm_vae_train_split(B, S, G, out) == -1, (B, S, G)      # SCLDM_ERR_SHAPE
        assert b">= 1" in L.scldm_last_error()
    assert list(out) == [-7] * 4                                           # untouched on error
    assert L.scldm_vae_train_split(1, 1, 1, None) == -1
    assert L.scldm_vae_train_split(1, 1, 1, out) == 0 and list(out) == [1, 1, 1, 1]


def test_multitile_test_shapes_keep_their_split():
    for (B, S, G, _), want in MULTITILE_SHAPES.items():
        assert split(B, S, G) == want, (B, S, G)
        assert all(tiles > 1 for tiles, _ in want)
    B, S, G, _ = PRODUCTION_SHAPE
    assert split(B, S, G) == PRODUCTION_SPLIT == split(512, S, G)
    # the value-checked shapes of the older training tests all walk one tile per workgroup; the dentate loss loops (batch 32) do not
    older = [(5, 70, 130), (3, 300, 1000), (9, 64, 65), (37, 70, 200), (6, 90, 150)]
    for name in ("vae_train_small", "vae_train_2000"):
        g = load_golden(name)
        older.append((*g["counts_subset"].shape, g["genes"].shape[1]))
    for B, S, G in older:
        dec, pool = split(B, S, G)
        assert dec[0] == 1 and pool[0] == 1, (B, S, G)
    assert split(32, 6147, 17002) == ((17, 16), (7, 14))


def test_duplicated_cells_give_the_gradients_of_the_distinct_cells():
    """.mean() over cells is unchanged by repeating every cell R times, and sum(z * z_weight / R) over R copies is the one cell's
    term.  In float64 (the oracle computes in the dtype of its weights) the two sides differ by rounding of the longer sums only:
    1e-12 of each tensor's largest entry is four orders above float64's unit roundoff times the few thousand addends and eight
    below the GPU gate.  Also in the oracle's fp32, the arithmetic the GPU test compares with: below half the GPU gate."""
    k, R, S, G, n_genes = 4, 5, 70, 130, 200
    shapes = {n: tuple(v.shape) for n, v in _build_vae(n_genes).state_dict().items()}
    cfg = VAEConfig(n_genes=n_genes)
    rng = np.random.default_rng(17)
    genes = rng.integers(0, n_genes + 1, (k, G)).astype(np.int64)
    counts = rng.poisson(0.9, (k, G)).astype(np.float64)
    genes_s = rng.integers(0, n_genes + 1, (k, S)).astype(np.int64)
    counts_s = rng.poisson(0.9, (k, S)).astype(np.float64)
    counts_s[:, -(S // 5):] = 0.0
    lib = counts.sum(1, keepdims=True) + 1.0
    zw = 0.3 * rng.standard_normal((k, 16, 16))
    rep = lambda a: np.tile(a, (R,) + (1,) * (a.ndim - 1))          # [c0, c1, c2, c3, c0, ...]
    for dtype, bound in ((torch.float64, 1e-12), (torch.float32, 0.5 * TOL)):
        sd = make_state_dict(shapes, 321, dtype=dtype)
        t = lambda a: torch.from_numpy(a) if a.dtype == np.int64 else torch.from_numpy(a).to(dtype)
        loss1, (mu1, _, z1), g1 = vae_training_grads(sd, cfg, t(counts), t(genes), t(lib), t(counts_s), t(genes_s), z_weight=t(zw))
        lossR, (muR, _, zR), gR = vae_training_grads(sd, cfg, t(rep(counts)), t(rep(genes)), t(rep(lib)), t(rep(counts_s)),
                                                     t(rep(genes_s)), z_weight=t(rep(zw) / R))
        assert loss1.dtype == dtype and all(g.dtype == dtype for g in g1.values())
        assert abs(float(lossR) - float(loss1)) <= bound * abs(float(loss1))
        assert float((muR - mu1.repeat(R, 1)).abs().max()) <= bound * float(mu1.abs().max())
        assert float((zR - z1.repeat(R, 1, 1)).abs().max()) <= bound * float(z1.abs().max())
        assert set(gR) == set(g1)
        worst = max((float((gR[n] - g1[n]).abs().max()) / float(g1[n].abs().max()), n) for n in g1 if n != BIAS)
        print(f"[parity] duplicated cells ({k} x {R}) against the distinct cells, {dtype}: worst gradient error {worst[0]:.2e} ({worst[1]})")
        assert worst[0] <= bound, worst

"""CPU-side checks of the ordered (deterministic) table gradients of the VAE training backward: the public switch, the two C-ABI
entry points, and the index `scldm_amd.vae.table_order` builds - against numpy's stable argsort on small inputs."""
import os
import re

import numpy as np
import torch

from conftest import ROOT


def test_the_switch_exists_and_is_off():
    from scldm_amd.vae import TransformerVAE
    assert hasattr(TransformerVAE, "deterministic") and TransformerVAE.deterministic is False
    assert TransformerVAE.last_table_gradient_mode is None


def test_entry_points_are_exported_and_prototyped():
    from scldm_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "scldm_hip.h")).read()
    L = _lib.lib()
    for name in ("scldm_vae_train_backward_ordered", "scldm_vae_train_rows_bytes"):
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert re.search(rf"\b{name}\s*\(", hdr), f"{name} has no prototype"
    # the ordered backward takes the arguments of _ex, then order, seg, n_entries, rows, and the stream last
    ex, od = L.scldm_vae_train_backward_ex.argtypes, L.scldm_vae_train_backward_ordered.argtypes
    assert list(od[:len(ex) - 1]) == list(ex[:-1]) and len(od) == len(ex) + 4
    assert L.scldm_vae_train_rows_bytes(None, 2, 3, 4) == 0          # no handle: 0, like the other size queries


def reference_index(genes, genes_s, counts_s, n_rows):
    B, G = genes.shape
    keys = np.concatenate([genes.reshape(-1), genes_s.reshape(-1)])
    entries = np.arange(keys.size)
    keep = np.concatenate([np.ones(B * G, bool), counts_s.reshape(-1) != 0])
    keys, entries = keys[keep], entries[keep]
    perm = np.argsort(keys, kind="stable")
    seg = np.concatenate([[0], np.cumsum(np.bincount(keys, minlength=n_rows))])
    return entries[perm], seg


def check(genes, genes_s, counts_s, n_rows):
    from scldm_amd.vae import table_order
    order, seg = table_order(torch.from_numpy(genes), torch.from_numpy(genes_s), torch.from_numpy(counts_s), n_rows)
    assert order.dtype == torch.int32 and seg.dtype == torch.int32
    order, seg = order.numpy(), seg.numpy()
    ref_order, ref_seg = reference_index(genes, genes_s, counts_s, n_rows)
    assert np.array_equal(order, ref_order) and np.array_equal(seg, ref_seg)
    assert seg.shape == (n_rows + 1,) and seg[0] == 0 and np.all(np.diff(seg) >= 0) and seg[-1] == len(order)
    keys = np.concatenate([genes.reshape(-1), genes_s.reshape(-1)])
    for r in range(n_rows):          # a row's segment: its entries, ascending
        mine = order[seg[r]:seg[r + 1]]
        assert np.all(keys[mine] == r) and np.all(np.diff(mine) > 0)
    return order, seg


def test_table_order_matches_a_stable_argsort():
    n_genes = 9                       # table rows 0 .. 9; rows 4, 6 and 8 are used by nobody
    genes = np.array([[3, 3, 0, 9, 3], [5, 0, 9, 2, 2], [0, 7, 7, 7, 1]], dtype=np.int64)        # repeats inside a cell; 0 in every cell; the last row
    genes_s = np.array([[9, 1, 1, 0], [2, 9, 0, 5], [0, 0, 3, 9]], dtype=np.int64)
    counts_s = np.array([[2.0, 1.0, 0.0, 3.0], [1.0, 0.0, 4.0, 0.0], [1.0, 2.0, 0.0, 0.0]], dtype=np.float32)
    order, seg = check(genes, genes_s, counts_s, n_genes + 1)
    B, G, S = 3, 5, 4
    # zero-count encoder tokens are dropped, every decoder slot and every other encoder token is listed once
    dropped = B * G + np.flatnonzero(counts_s.reshape(-1) == 0)
    assert not np.intersect1d(order, dropped).size
    assert len(order) == B * G + int((counts_s != 0).sum()) and len(set(order.tolist())) == len(order)
    for r in (4, 6, 8):
        assert seg[r] == seg[r + 1]
    # gene 0: decoder slots of all three cells, then the encoder tokens of cells 0 (3.0), 1 (4.0) and 2 (1.0, 2.0)
    assert order[seg[0]:seg[1]].tolist() == [2, 6, 10, B * G + 3, B * G + 6, B * G + 8, B * G + 9]
    # the last row (n_genes): decoder slots 3 and 7, encoder token (0, 0); tokens (1, 1) and (2, 3) have zero counts
    assert order[seg[9]:seg[10]].tolist() == [3, 7, B * G + 0]


def test_table_order_on_random_and_degenerate_inputs():
    rng = np.random.default_rng(11)
    for B, G, S, n_rows in [(1, 1, 1, 2), (4, 33, 17, 6), (7, 20, 50, 400)]:
        genes = rng.integers(0, n_rows, (B, G)).astype(np.int64)
        genes_s = rng.integers(0, n_rows, (B, S)).astype(np.int64)
        counts_s = rng.poisson(0.7, (B, S)).astype(np.float32)
        check(genes, genes_s, counts_s, n_rows)
    # every encoder count zero: decoder entries only
    genes = np.array([[1, 0]], dtype=np.int64)
    order, seg = check(genes, np.array([[1, 1, 1]], dtype=np.int64), np.zeros((1, 3), np.float32), 3)
    assert order.tolist() == [1, 0] and seg.tolist() == [0, 1, 2, 2]

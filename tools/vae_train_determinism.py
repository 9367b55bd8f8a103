#!/usr/bin/env python3
"""Run the TransformerVAE training backward several times on the same inputs and report which gradient tensors differ between runs,
how many entries and by how much relative to the first run: the VAE counterpart of tools/train_determinism.py (a race detector
for the per-gene backward, the pooling backward and the cell sides).  In `atomic` mode the two embedding tables (gene_embedding,
theta) are expected to differ - float atomics - and nothing else; in `ordered` mode (TransformerVAE.deterministic) nothing may.

usage: tools/vae_train_determinism.py [--cells 37] [--genes 200] [--tokens 70] [--n-genes 12] [--precision fp32|fp16]
                                      [--mode atomic|ordered] [--runs 4]
(the defaults: 13 table rows hit hundreds of times each, genes repeated inside cells; gene ids are uniform in [0, n_genes])"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_vae_train as T  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--cells", type=int, default=37)
ap.add_argument("--genes", type=int, default=200, help="decoded genes per cell (G)")
ap.add_argument("--tokens", type=int, default=70, help="encoder tokens per cell (S)")
ap.add_argument("--n-genes", type=int, default=12)
ap.add_argument("--precision", choices=["fp32", "fp16"], default="fp32")
ap.add_argument("--mode", choices=["atomic", "ordered"], default="atomic")
ap.add_argument("--runs", type=int, default=4)
a = ap.parse_args()
B, G, S = a.cells, a.genes, a.tokens
vae, sd, cfg = T.build(a.n_genes, 500 + B)
vae.precision, vae.deterministic = a.precision, a.mode == "ordered"
rng = np.random.default_rng(B * 100 + G)
genes = rng.integers(0, a.n_genes + 1, (B, G)).astype(np.int64)
counts = rng.poisson(0.9, (B, G)).astype(np.float32)
genes_s = rng.integers(0, a.n_genes + 1, (B, S)).astype(np.int64)
counts_s = rng.poisson(0.9, (B, S)).astype(np.float32)
lib = (counts.sum(1, keepdims=True) + 1.0).astype(np.float32)
zw = (0.3 * rng.standard_normal((B, 16, 16))).astype(np.float32)
runs = []
for _ in range(a.runs):
    T.hip_step(vae, counts, genes, lib, counts_s, genes_s, z_weight=zw)
    torch.cuda.synchronize()
    runs.append({k: p.grad.clone() for k, p in vae.named_parameters() if p.grad is not None})
assert vae.last_table_gradient_mode == a.mode
bad = {}
for i in range(1, a.runs):
    for k in runs[0]:
        d = runs[i][k] != runs[0][k]
        if bool(d.any()):
            bad.setdefault(k, []).append((int(d.sum()), float((runs[i][k] - runs[0][k]).norm() / runs[0][k].norm())))
print(f"{os.environ.get('SCLDM_LIB', 'tree')[-16:]} {B} cells G={G} S={S} n_genes={a.n_genes} {a.precision} {a.mode}: "
      f"{len(bad)} of {len(runs[0])} gradient tensors differ between {a.runs} runs")
for k, v in sorted(bad.items())[:40]:
    print("   ", k, "(entries differing, relative l2 difference) per run:", v)

#!/usr/bin/env python3
"""Generate long_euler_4097.npz: one cell through 4 097 Euler evaluations (4 098 grid points), one more than the fused solves embed
up front, so that the GPU test of the step-by-step route needs no 50-second CPU chain.

Run from the repo root:   python tests/golden/make_golden_long_euler.py

Uses oracle/ only (no reference import): dit_base's weights (oracle.weights.make_state_dict over the shapes and seed stored in
dit_base.npz), oracle.transport.sample_ode_fixed over oracle.dit.dit_forward_with_cfg, in float64 (stored) and in float32 (checked
against the float64 end state before anything is written, and its distance stored).  Running the script twice gives identical bytes."""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle.dit import DiTConfig, dit_forward_with_cfg  # noqa: E402
from oracle.transport import sample_ode_fixed  # noqa: E402
from oracle.weights import make_state_dict  # noqa: E402

GRID_POINTS = 4098
SCALE = 1.5
ORACLE_AGREE = 1e-5   # the float32 oracle chain against the float64 one (scale-relative max); the GPU gate is 1e-4


def main():
    with np.load(os.path.join(HERE, "dit_base.npz"), allow_pickle=False) as f:
        kw = json.loads(str(f["kwargs_json"]))
        shapes = {k: tuple(v) for k, v in json.loads(str(f["shapes_json"])).items()}
        seed = int(f["seed"])
    sd = make_state_dict(shapes, seed)
    sd64 = {k: v.double() for k, v in sd.items()}
    cfg = DiTConfig(n_embed=kw["n_embed"], n_embed_input=kw["n_embed_input"], n_layer=kw["n_layer"], n_head=kw["n_head"],
                    seq_len=kw["seq_len"], multiple_of=kw["multiple_of"], layernorm_eps=kw["layernorm_eps"],
                    class_vocab_sizes=kw["class_vocab_sizes"], condition_strategy=kw["condition_strategy"])
    (name, vocab), = cfg.class_vocab_sizes.items()
    rng = np.random.default_rng(11)
    z0 = rng.standard_normal((1, 16, 16)).astype(np.float32)
    label = rng.integers(0, vocab, 1).astype(np.int64)
    z2 = torch.from_numpy(np.concatenate([z0, z0]))
    cond2 = {name: torch.from_numpy(np.concatenate([label, label]))}
    scales = {name: SCALE}
    with torch.no_grad():
        end64 = sample_ode_fixed(z2.double(), lambda x, t: dit_forward_with_cfg(sd64, cfg, x, t, cond2, scales), GRID_POINTS, "euler").numpy()
        end32 = sample_ode_fixed(z2, lambda x, t: dit_forward_with_cfg(sd, cfg, x, t, cond2, scales), GRID_POINTS, "euler").numpy()
    assert end64.dtype == np.float64 and np.isfinite(end64).all() and np.isfinite(end32).all()
    err = float(np.abs(end32.astype(np.float64) - end64).max() / np.abs(end64).max())
    print(f"long_euler_4097: |end| max {np.abs(end64).max():.4f}, float32 oracle chain against float64 {err:.2e}")
    assert err <= ORACLE_AGREE, err
    np.savez_compressed(os.path.join(HERE, "long_euler_4097.npz"), z0=z0, label=label, label_name=np.array(name), scale=np.array(SCALE),
                        grid_points=np.array(GRID_POINTS), end64=end64, oracle_fp32_err=np.array(err))


if __name__ == "__main__":
    main()

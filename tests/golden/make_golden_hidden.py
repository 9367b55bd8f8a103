#!/usr/bin/env python3
"""Generate the DiT fixtures at SwiGLU hidden widths other than 684 by RUNNING THE REFERENCE (build container only; see
make_golden.py for the import stubs).

Run from the repo root:   python tests/golden/make_golden_hidden.py

tests/golden/dit_h<H>.npz: the reference's own 256-wide, 8-head, 16-token, 2-layer `DiT` built with a `multiple_of` that gives the
hidden width H (layers.py: multiple_of * ceil(int(2 * 4 * n_embed / 3) / multiple_of)) - every other fixture uses multiple_of=4,
H = 684.  Per case, batch 3: one plain forward with the `block0.mlp_out` tap and one `forward_with_cfg` at guidance 2.0.  A separate
script: make_golden.py's later cases depend on the order of its draws from torch's global RNG, so nothing may be inserted there, and
its fixtures keep regenerating bit-exactly.  Only data is stored; the weights are rebuilt from `oracle.weights.make_state_dict(shapes, seed)`.  Running the
script twice gives identical bytes."""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (installs the import stubs and puts the repo root on sys.path)

# name: (multiple_of, expected hidden width, seed)
#   768: six whole 128-unit chunks, no half chunk, no padding; the fused training route's upper edge (three exact 256-chunks)
#   704: five chunks + a half chunk with NO padded unit
#   700: five chunks + a half chunk, 4 padded units (the pad boundary inside a wave's 16-unit slice)
#   832: six chunks + a half chunk, beyond the fused training route (> 768)
#   682: the width multiple_of=2 gives: H % 4 == 2, refused by the training path
HIDDEN_CASES = {
    "dit_h768": (256, 768, 111),
    "dit_h704": (64, 704, 112),
    "dit_h700": (100, 700, 113),
    "dit_h832": (832, 832, 114),
    "dit_h682": (2, 682, 115),
}
KW = dict(n_embed=256, n_embed_input=16, n_layer=2, n_head=8, seq_len=16, class_vocab_sizes={"clusters": 14},
          condition_strategy="mutually_exclusive")
B = 3


def gen_hidden(name, multiple_of, hidden, seed):
    common = {**mg.COMMON, "multiple_of": multiple_of}
    m = mg.DiT(**KW, **common)
    assert tuple(m.blocks[0].mlp.w1.weight.shape) == (hidden, 256), (name, tuple(m.blocks[0].mlp.w1.weight.shape))
    shapes = mg.shapes_of(m)
    m.load_state_dict(mg.make_state_dict(shapes, seed), strict=True)
    m.eval()
    rng = np.random.default_rng(seed + 1000)
    S, C = KW["seq_len"], KW["n_embed_input"]
    out = {"shapes_json": np.array(json.dumps({k: list(v) for k, v in shapes.items()})),
           "kwargs_json": np.array(json.dumps({**KW, **common})), "seed": np.array(seed), "hidden": np.array(hidden)}
    x = rng.standard_normal((B, S, C)).astype(np.float32)
    t = rng.uniform(0, 1, (B,)).astype(np.float32)
    lab = rng.integers(0, 14, (B,)).astype(np.int64)
    out["fwd_x"], out["fwd_t"], out["fwd_label_clusters"] = x, t, lab
    out["fwd_classes"] = np.array(json.dumps(["clusters"]))
    taps = {}
    hook = m.blocks[0].mlp.register_forward_hook(lambda mod, i, o: taps.__setitem__("block0.mlp_out", o.detach().numpy().copy()))
    with torch.no_grad():
        y = m(torch.from_numpy(x), torch.from_numpy(t), {"clusters": torch.from_numpy(lab)}, force_drop_ids=False)
    hook.remove()
    out["fwd_out"] = y.numpy()
    out["tap_block0.mlp_out"] = taps["block0.mlp_out"]
    z = rng.standard_normal((B, S, C)).astype(np.float32)
    x2 = np.concatenate([z, z], 0)
    t2 = np.full((2 * B,), 0.37, np.float32)
    lab2 = np.concatenate([lab, lab])
    scales = {"clusters": 2.0}
    with torch.no_grad():
        y2 = m.forward_with_cfg(torch.from_numpy(x2), torch.from_numpy(t2), condition={"clusters": torch.from_numpy(lab2)},
                                cfg_scale=scales)
    out["cfg_x"], out["cfg_t"], out["cfg_label_clusters"] = x2, t2, lab2
    out["cfg_out_s2"] = y2.numpy()
    out["cfg_scales_s2"] = np.array(json.dumps(scales))
    assert np.isfinite(out["fwd_out"]).all() and np.isfinite(out["cfg_out_s2"]).all()
    np.savez_compressed(os.path.join(HERE, f"{name}.npz"), **out)
    print(name, "hidden", hidden, "fwd |y|max", float(np.abs(out["fwd_out"]).max()), "cfg |y|max", float(np.abs(out["cfg_out_s2"]).max()))


if __name__ == "__main__":
    torch.manual_seed(0)
    for name, (multiple_of, hidden, seed) in HIDDEN_CASES.items():
        gen_hidden(name, multiple_of, hidden, seed)

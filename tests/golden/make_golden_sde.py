#!/usr/bin/env python3
"""Generate the SDE sampler fixtures by RUNNING THE REFERENCE (build container only; see make_golden.py for the import stubs).

Run from the repo root:   python tests/golden/make_golden_sde.py

tests/golden/sde_<case>.npz: the reference's own `Sampler(create_transport()).sample_sde(...)` on the reference DiT through
`forward_with_cfg`, driven exactly as models.py:801-812 drives `sample_ode` (doubled state, doubled labels, cfg_scale closed over).
The normals `integrators.sde` draws with `th.randn` are recorded, and so is the t vector of every model evaluation (the reference
evaluates the model twice with identical arguments wherever it needs drift and score: such a pair counts once).  Stored: z0, labels,
scales, the noise, the t vectors and the returned list - data only; the weights are rebuilt from `oracle.weights.make_state_dict`.
tests/golden/sde_toy.npz: the same sampler on a plain callable (tests/sde_ref.py: toy_model) from `torch.manual_seed` alone - it
pins the ORDER in which the host generator is consumed.  Every returned state is checked to be finite before anything is written;
running the script twice gives identical bytes."""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402  (installs the import stubs and puts the repo root on sys.path)
from scldm.transport import Sampler, create_transport  # noqa: E402
from scldm.transport import integrators  # noqa: E402

import sde_ref  # noqa: E402


class _RecordingTorch:
    """Stands in for the `th` of the reference's integrators module: every attribute is torch's, `randn` also keeps its draws."""

    def __init__(self):
        self.draws = []

    def randn(self, *a, **k):
        w = torch.randn(*a, **k)
        self.draws.append(w.clone())
        return w

    def __getattr__(self, name):
        return getattr(torch, name)


def run_reference(model_fn, x0, method, form, norm, last_step, last_step_size, num_steps, **model_kwargs):
    rec = _RecordingTorch()
    seen = []

    def recording_model(x, t, **kw):
        if not (seen and torch.equal(seen[-1][0], x) and torch.equal(seen[-1][1], t)):
            seen.append((x.clone(), t.clone()))
        return model_fn(x, t, **kw)

    integrators.th = rec
    try:
        fn = Sampler(create_transport()).sample_sde(sampling_method=method, diffusion_form=form, diffusion_norm=norm, last_step=last_step,
                                                    last_step_size=last_step_size, num_steps=num_steps)
        with torch.no_grad():
            xs = fn(x0, recording_model, **model_kwargs)
    finally:
        integrators.th = torch
    xs = torch.stack(xs)
    assert xs.shape[0] == num_steps and torch.isfinite(xs).all(), "the reference returned a non-finite state"
    return xs.numpy(), torch.stack(rec.draws).numpy(), torch.stack([t for _, t in seen]).numpy()


def gen_case(name, dit_name, method, form, norm, last_step, last_step_size, num_steps):
    kwargs, _, seed = {**mg.DIT_CASES, **mg.LATE_DIT_CASES}[dit_name]
    m, _ = mg.build_dit(kwargs, seed)
    B = sde_ref.CASE_B
    rng = np.random.default_rng(seed + 7000 + num_steps)
    z0 = rng.standard_normal((B, kwargs["seq_len"], kwargs["n_embed_input"])).astype(np.float32)
    labels = {k: rng.integers(0, v, (B,)).astype(np.int64) for k, v in kwargs["class_vocab_sizes"].items()}
    scales = {k: 1.5 - 0.4 * i for i, k in enumerate(sorted(kwargs["class_vocab_sizes"]))}
    z2 = torch.from_numpy(np.concatenate([z0, z0]))
    cond2 = {k: torch.from_numpy(np.concatenate([v, v])) for k, v in labels.items()}
    model_fn = lambda x, t, **kw: m.forward_with_cfg(x, t, **kw, cfg_scale=scales)
    torch.manual_seed(seed + 7000)
    xs, noise, ts = run_reference(model_fn, z2, method, form, norm, last_step, last_step_size, num_steps, condition=cond2)
    out = {"z0": z0, "scales_json": np.array(json.dumps(scales)), "noise": noise, "t_seen": ts, "traj": xs,
           "settings_json": np.array(json.dumps([dit_name, method, form, norm, last_step, last_step_size, num_steps]))}
    for k, v in labels.items():
        out[f"label_{k}"] = v
    np.savez_compressed(os.path.join(HERE, f"{name}.npz"), **out)
    print(name, "evaluations", ts.shape[0], "|x|max per state", np.abs(xs).reshape(num_steps, -1).max(1))


def gen_toy():
    out = {"x0": np.random.default_rng(sde_ref.TOY_SEED).standard_normal(sde_ref.TOY_SHAPE).astype(np.float32)}
    torch.manual_seed(sde_ref.TOY_SEED)
    for i, (method, form, norm, last_step, lss, steps) in enumerate(sde_ref.TOY_RUNS):
        xs, noise, ts = run_reference(sde_ref.toy_model, torch.from_numpy(out["x0"]), method, form, norm, last_step, lss, steps)
        out[f"traj_{i}"], out[f"noise_{i}"], out[f"t_seen_{i}"] = xs, noise, ts
    np.savez_compressed(os.path.join(HERE, "sde_toy.npz"), **out)
    print("sde_toy", [float(np.abs(out[f"traj_{i}"]).max()) for i in range(len(sde_ref.TOY_RUNS))])


if __name__ == "__main__":
    for name, case in sde_ref.CASES.items():
        gen_case(name, *case)
    gen_toy()

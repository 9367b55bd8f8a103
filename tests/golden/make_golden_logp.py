#!/usr/bin/env python3
"""Generate the log-likelihood fixtures by RUNNING THE REFERENCE (build container only; see make_golden.py for the import stubs).

Run from the repo root:   python tests/golden/make_golden_logp.py

tests/golden/logp_<case>.npz: the reference's own `Sampler(create_transport()).sample_ode_likelihood(...)` on the reference DiT
through `forward_with_cfg` (doubled state, doubled labels, cfg_scale closed over, as models.py:801-812 drives `sample_ode`).
WHAT IS PINNED TO THE REFERENCE is the per-evaluation map (x, t, eps) -> (-v, logp_grad) of its `_likelihood_drift` (its own fp32
autograd), `prior_logp`, and the sign / time convention (model time 1 - s, state moves by -v, delta_logp accumulates +logp_grad,
logp = prior_logp(x_end) - delta_logp).  THE GRID STEPPING IS PINNED TO THIS PROJECT'S fixed-grid convention: the reference hands
stepping to `torchdiffeq.odeint`, which is not on the build machine, so `integrators.odeint` is replaced by a fixed-grid euler / heun
stand-in over the tuple state written here (h = float(t[i + 1] - t[i]); Heun's second evaluation at t[i + 1]).  The probes the
reference draws with `th.randint` are recorded, and so is the t vector of every model evaluation (the reference evaluates the model
twice with identical arguments per drift call: such a pair counts once).  Stored: x, labels, scales, the probes, the t vectors, every
logp_grad, logp and x_end - data only; the weights are rebuilt from `oracle.weights.make_state_dict`.
tests/golden/logp_toy.npz: the same sampler on a plain callable (tests/logp_ref.py: toy_model) from `torch.manual_seed` alone - it pins
the ORDER in which the host generator is consumed.  Every stored value is checked to be finite before anything is written; running
the script twice gives identical bytes."""
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
from scldm.transport import transport as transport_mod  # noqa: E402

import logp_ref  # noqa: E402


class _RecordingTorch:
    """Stands in for the `th` of the reference's transport module: every attribute is torch's, `randint` also keeps its draws."""

    def __init__(self):
        self.draws = []

    def randint(self, *a, **k):
        w = torch.randint(*a, **k)
        self.draws.append(w.clone())
        return w

    def __getattr__(self, name):
        return getattr(torch, name)


def fixed_grid_odeint(record):
    """Fixed-grid euler / heun over a tuple state, in place of torchdiffeq.odeint (same call signature, returns per-component stacks)."""

    def odeint(fn, y0, t, method=None, atol=None, rtol=None):
        method_l = str(method).lower()
        assert method_l in ("euler", "heun") and isinstance(y0, tuple)
        ys = [tuple(c.detach() for c in y0)]

        def f(tv, y):
            out = fn(tv, tuple(c.detach() for c in y))
            record.append(out[1].detach().clone())
            return tuple(c.detach() for c in out)

        for i in range(len(t) - 1):
            h = float(t[i + 1] - t[i])
            y = ys[-1]
            k1 = f(t[i], y)
            if method_l == "euler":
                y = tuple(c + h * k for c, k in zip(y, k1))
            else:
                k2 = f(t[i + 1], tuple(c + h * k for c, k in zip(y, k1)))
                y = tuple(c + (0.5 * h) * (a + b) for c, a, b in zip(y, k1, k2))
            ys.append(y)
        return tuple(torch.stack([y[j] for y in ys]) for j in range(len(y0)))

    return odeint


def run_reference(model_fn, x0, method, steps, **model_kwargs):
    rec = _RecordingTorch()
    seen, lgs = [], []

    def recording_model(x, t, **kw):
        if not (seen and torch.equal(seen[-1][0], x.detach()) and torch.equal(seen[-1][1], t)):
            seen.append((x.detach().clone(), t.clone()))
        return model_fn(x, t, **kw)

    transport_mod.th = rec
    integrators.odeint = fixed_grid_odeint(lgs)
    try:
        fn = Sampler(create_transport()).sample_ode_likelihood(sampling_method=method, num_steps=steps + 1)
        with torch.no_grad():
            logp, x_end = fn(x0.clone(), recording_model, **model_kwargs)
    finally:
        transport_mod.th = torch
        integrators.odeint = None
    n_ev = logp_ref.n_evaluations(method, steps)
    probes = torch.stack(rec.draws).float() * 2 - 1
    ts, lg = torch.stack([t for _, t in seen]), torch.stack(lgs)
    assert probes.shape[0] == n_ev and ts.shape[0] == n_ev and lg.shape[0] == n_ev, (probes.shape, ts.shape, lg.shape)
    for v in (logp, x_end, probes, ts, lg):
        assert torch.isfinite(v).all(), "the reference returned a non-finite value"
    return logp.detach().numpy(), x_end.detach().numpy(), probes.numpy(), ts.numpy(), lg.numpy()


def gen_case(name, dit_name, method, steps):
    kwargs, _, seed = {**mg.DIT_CASES, **mg.LATE_DIT_CASES}[dit_name]
    m, _ = mg.build_dit(kwargs, seed)
    B = logp_ref.CASE_B
    rng = np.random.default_rng(seed + 9000 + steps)
    x = rng.standard_normal((B, kwargs["seq_len"], kwargs["n_embed_input"])).astype(np.float32)
    labels = {k: rng.integers(0, v, (B,)).astype(np.int64) for k, v in kwargs["class_vocab_sizes"].items()}
    scales = {k: 1.5 - 0.4 * i for i, k in enumerate(sorted(kwargs["class_vocab_sizes"]))}
    z2 = torch.from_numpy(np.concatenate([x, x]))
    cond2 = {k: torch.from_numpy(np.concatenate([v, v])) for k, v in labels.items()}
    model_fn = lambda xx, t, **kw: m.forward_with_cfg(xx, t, **kw, cfg_scale=scales)
    torch.manual_seed(seed + 9000)
    logp, x_end, probes, ts, lg = run_reference(model_fn, z2, method, steps, condition=cond2)
    out = {"x": x, "scales_json": np.array(json.dumps(scales)), "probes": probes, "t_seen": ts, "logp_grad": lg, "logp": logp, "x_end": x_end,
           "settings_json": np.array(json.dumps([dit_name, method, steps]))}
    for k, v in labels.items():
        out[f"label_{k}"] = v
    np.savez_compressed(os.path.join(HERE, f"{name}.npz"), **out)
    print(name, "evaluations", ts.shape[0], "logp", logp, "|logp_grad|max", np.abs(lg).max())


def gen_toy():
    out = {"x0": np.random.default_rng(logp_ref.TOY_SEED).standard_normal(logp_ref.TOY_SHAPE).astype(np.float32)}
    torch.manual_seed(logp_ref.TOY_SEED)
    for i, (method, steps) in enumerate(logp_ref.TOY_RUNS):
        logp, x_end, probes, ts, lg = run_reference(logp_ref.toy_model, torch.from_numpy(out["x0"]), method, steps)
        out[f"logp_{i}"], out[f"x_end_{i}"], out[f"probes_{i}"], out[f"t_seen_{i}"], out[f"logp_grad_{i}"] = logp, x_end, probes, ts, lg
    np.savez_compressed(os.path.join(HERE, "logp_toy.npz"), **out)
    print("logp_toy", [out[f"logp_{i}"] for i in range(len(logp_ref.TOY_RUNS))])


if __name__ == "__main__":
    for name, case in logp_ref.CASES.items():
        gen_case(name, *case)
    gen_toy()

#!/usr/bin/env python3
"""Generate the fixtures of the SDE sampler and the likelihood under non-default transports by RUNNING THE REFERENCE (build container
only; see make_golden.py for the import stubs).

Run from the repo root:   python tests/golden/make_golden_sde_logp_transport.py

Data only, every value produced by the reference's own code (case tables: tests/transport_solvers_ref.py):
  sdet_<case>.npz    `Sampler(create_transport(path, prediction, None, None, sample_eps)).sample_sde(...)` on the reference DiT through
                     `forward_with_cfg`, driven as make_golden_sde.py drives the default transport: the `th.randn` draws of
                     `integrators.sde` are recorded, and so is the t vector of every model evaluation (identical repeated calls count once).
  logpt_<case>.npz   `.sample_ode_likelihood(...)` likewise, as make_golden_logp.py: the `th.randint` probes recorded, `integrators.odeint`
                     replaced by the fixed-grid euler / heun stand-in over the tuple state (h = float(t[i + 1] - t[i]); Heun's second
                     evaluation at t[i + 1]) - the per-evaluation map, prior_logp and the sign / time convention are the reference's, the
                     grid stepping this project's.
  sdet_toy.npz, logpt_toy.npz   the same samplers on a plain callable from `torch.manual_seed` alone: they pin the ORDER in which the
                     host generator is consumed.
  sde_logp_transport_coef.npz   for COEF_CASES, random float64 x and m: the reference's own sde_drift, diffusion_fn, score and the three
                     last-step results.
Asserted before anything is written: (a) everything finite; (b) the reference's fp32 run within 1e-5 (scale-relative) of the same run in
float64 (the reference DiT in float64 - double_dit of make_golden_transport_paths.py - on the same draws); (c) the model term is visible:
replacing the model output by zeros changes every SDE state, and the largest logp_grad, by at least 1e-2 (scale-relative).  Running the
script twice gives identical bytes."""
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
from make_golden_logp import fixed_grid_odeint  # noqa: E402
from make_golden_transport_paths import double_dit, scale_rel  # noqa: E402
from scldm.transport import Sampler, create_transport  # noqa: E402
from scldm.transport import integrators  # noqa: E402
from scldm.transport import transport as transport_mod  # noqa: E402

import transport_solvers_ref as R  # noqa: E402

REF_AGREE = 1e-5
MODEL_VISIBLE = 1e-2


def transport(path, prediction, eps):
    return create_transport(path, prediction, None, None, eps)      # (sample_eps given: the reference leaves it None otherwise)


class _Torch:
    """Stands in for the `th` of the reference's modules: every attribute is torch's; `randn` / `randint` record their draws, or replay a
    given list; `ones` makes float64 vectors when asked to (the float64 run keeps its times in double)."""

    def __init__(self, replay=None, double=False):
        self.draws, self.replay, self.double = [], (list(replay) if replay is not None else None), double

    def _draw(self, fn, a, k):
        w = self.replay.pop(0).clone() if self.replay is not None else fn(*a, **k)
        self.draws.append(w.clone())
        return w

    def randn(self, *a, **k):
        return self._draw(torch.randn, a, k)

    def randint(self, *a, **k):
        return self._draw(torch.randint, a, k)

    def ones(self, *a, **k):
        if self.double:
            k = {**k, "dtype": torch.float64}
        return torch.ones(*a, **k)

    def __getattr__(self, name):
        return getattr(torch, name)


def _recording(model_fn, seen, zero):
    def model(x, t, **kw):
        if not (seen and torch.equal(seen[-1][0], x.detach()) and torch.equal(seen[-1][1], t)):
            seen.append((x.detach().clone(), t.clone()))
        out = model_fn(x, t, **kw)
        return out * 0.0 if zero else out
    return model


def run_sde(tr_args, model_fn, x0, method, form, norm, last, lss, steps, replay=None, double=False, zero=False, **kw):
    rec, seen = _Torch(replay, double), []
    integrators.th = rec
    try:
        fn = Sampler(transport(*tr_args)).sample_sde(sampling_method=method, diffusion_form=form, diffusion_norm=norm, last_step=last,
                                                     last_step_size=lss, num_steps=steps)
        with torch.no_grad():
            xs = torch.stack(fn(x0.double() if double else x0, _recording(model_fn, seen, zero), **kw))
    finally:
        integrators.th = torch
    assert xs.shape[0] == steps and torch.isfinite(xs).all(), "the reference returned a non-finite state"
    return xs.numpy(), torch.stack(rec.draws), torch.stack([t for _, t in seen]).numpy()


def run_logp(tr_args, model_fn, x0, method, steps, replay=None, double=False, zero=False, **kw):
    rec, seen, lgs = _Torch(replay, double), [], []
    transport_mod.th = rec
    integrators.th = rec
    integrators.odeint = fixed_grid_odeint(lgs)
    try:
        fn = Sampler(transport(*tr_args)).sample_ode_likelihood(sampling_method=method, num_steps=steps + 1)
        with torch.no_grad():
            logp, x_end = fn((x0.double() if double else x0).clone(), _recording(model_fn, seen, zero), **kw)
    finally:
        transport_mod.th = torch
        integrators.th = torch
        integrators.odeint = None
    n_ev = R.n_evaluations(method, steps)
    draws, ts, lg = torch.stack(rec.draws), torch.stack([t for _, t in seen]), torch.stack(lgs)
    assert draws.shape[0] == n_ev and ts.shape[0] == n_ev and lg.shape[0] == n_ev, (draws.shape, ts.shape, lg.shape)
    for v in (logp, x_end, ts, lg):
        assert torch.isfinite(v).all(), "the reference returned a non-finite value"
    return logp.detach().numpy(), x_end.detach().numpy(), draws, ts.numpy(), lg.numpy()


def _dit_inputs(dit_name, seed_offset, key):
    kwargs, _, seed = {**mg.DIT_CASES, **mg.LATE_DIT_CASES}[dit_name]
    m, _ = mg.build_dit(kwargs, seed)
    rng = np.random.default_rng(seed + seed_offset)
    x = rng.standard_normal((R.CASE_B, kwargs["seq_len"], kwargs["n_embed_input"])).astype(np.float32)
    labels = {k: rng.integers(0, v, (R.CASE_B,)).astype(np.int64) for k, v in kwargs["class_vocab_sizes"].items()}
    scales = {k: 1.5 - 0.4 * i for i, k in enumerate(sorted(kwargs["class_vocab_sizes"]))}
    z2 = torch.from_numpy(np.concatenate([x, x]))
    cond2 = {k: torch.from_numpy(np.concatenate([v, v])) for k, v in labels.items()}
    fns = [lambda xx, t, mm=mm, **kw: mm.forward_with_cfg(xx, t, **kw, cfg_scale=scales) for mm in (m, double_dit(m))]
    out = {key: x, "scales_json": np.array(json.dumps(scales))}
    for k, v in labels.items():
        out[f"label_{k}"] = v
    return seed, z2, cond2, fns, out


def gen_sde_case(name, dit_name, path, pred, method, form, norm, last, lss, steps):
    seed, z2, cond2, (fn32, fn64), out = _dit_inputs(dit_name, 7100 + steps, "z0")
    tr_args = (path, pred, R.sde_eps(pred))
    torch.manual_seed(seed + 7100)
    xs, noise, ts = run_sde(tr_args, fn32, z2, method, form, norm, last, lss, steps, condition=cond2)
    xs64, _, _ = run_sde(tr_args, fn64, z2, method, form, norm, last, lss, steps, replay=noise, double=True, condition=cond2)
    xs0, _, _ = run_sde(tr_args, fn32, z2, method, form, norm, last, lss, steps, replay=noise, zero=True, condition=cond2)
    agree = max(scale_rel(xs[i], xs64[i]) for i in range(steps))
    visible = min(scale_rel(xs0[i], xs[i]) for i in range(steps))
    assert agree <= REF_AGREE, f"{name}: the reference's fp32 run is {agree:.2e} off its float64 one"
    assert visible >= MODEL_VISIBLE, f"{name}: the model term moves a state by {visible:.2e} only"
    out.update(noise=noise.numpy(), t_seen=ts, traj=xs,
               settings_json=np.array(json.dumps([dit_name, path, pred, method, form, norm, last, lss, steps])))
    np.savez_compressed(os.path.join(HERE, f"{name}.npz"), **out)
    print(name, "evaluations", ts.shape[0], "|x|max", float(np.abs(xs).max()), f"fp32 vs float64 {agree:.2e}  model term >= {visible:.2e}")


def gen_logp_case(name, dit_name, path, pred, method, steps, eps):
    seed, z2, cond2, (fn32, fn64), out = _dit_inputs(dit_name, 9100 + steps, "x")
    tr_args = (path, pred, eps)
    torch.manual_seed(seed + 9100)
    logp, x_end, draws, ts, lg = run_logp(tr_args, fn32, z2, method, steps, condition=cond2)
    logp64, x_end64, _, _, lg64 = run_logp(tr_args, fn64, z2, method, steps, replay=draws, double=True, condition=cond2)
    _, _, _, _, lg0 = run_logp(tr_args, fn32, z2, method, steps, replay=draws, zero=True, condition=cond2)
    agree = {"logp": scale_rel(logp, logp64), "x_end": scale_rel(x_end, x_end64), "logp_grad": scale_rel(lg, lg64)}
    visible = float(np.abs(lg - lg0).max() / np.abs(lg).max())
    assert max(agree.values()) <= REF_AGREE, f"{name}: the reference's fp32 run against its float64 one: {agree}"
    assert visible >= MODEL_VISIBLE, f"{name}: the model term moves the largest logp_grad by {visible:.2e} only"
    out.update(probes=(draws.float() * 2 - 1).numpy(), t_seen=ts, logp_grad=lg, logp=logp, x_end=x_end,
               settings_json=np.array(json.dumps([dit_name, path, pred, method, steps, eps])))
    np.savez_compressed(os.path.join(HERE, f"{name}.npz"), **out)
    print(name, "evaluations", ts.shape[0], "logp", logp, "|logp_grad|max", float(np.abs(lg).max()), "fp32 vs float64", agree, f"model term {visible:.2e}")


def gen_toys():
    x0 = np.random.default_rng(R.TOY_SEED).standard_normal(R.TOY_SHAPE).astype(np.float32)
    out = {"x0": x0}
    torch.manual_seed(R.TOY_SEED)
    for i, (path, pred, eps, method, form, norm, last, lss, steps) in enumerate(R.TOY_SDE_RUNS):
        xs, noise, ts = run_sde((path, pred, eps), R.toy_model, torch.from_numpy(x0), method, form, norm, last, lss, steps)
        out[f"traj_{i}"], out[f"noise_{i}"], out[f"t_seen_{i}"] = xs, noise.numpy(), ts
    np.savez_compressed(os.path.join(HERE, "sdet_toy.npz"), **out)
    print("sdet_toy", [float(np.abs(out[f"traj_{i}"]).max()) for i in range(len(R.TOY_SDE_RUNS))])
    out = {"x0": x0}
    torch.manual_seed(R.TOY_SEED + 1)
    for i, (path, pred, eps, method, steps) in enumerate(R.TOY_LOGP_RUNS):
        logp, x_end, draws, ts, lg = run_logp((path, pred, eps), R.toy_model, torch.from_numpy(x0), method, steps)
        out[f"logp_{i}"], out[f"x_end_{i}"], out[f"probes_{i}"], out[f"t_seen_{i}"], out[f"logp_grad_{i}"] = logp, x_end, (draws.float() * 2 - 1).numpy(), ts, lg
    np.savez_compressed(os.path.join(HERE, "logpt_toy.npz"), **out)
    print("logpt_toy", [out[f"logp_{i}"] for i in range(len(R.TOY_LOGP_RUNS))])


def gen_coef():
    """The reference's closures on float64 tensors: sde_drift, diffusion_fn, score, and the Mean / Tweedie / Euler last steps."""
    rng = np.random.default_rng(R.TOY_SEED + 2)
    out = {}
    for i, (path, pred, form, norm, t, lss) in enumerate(R.COEF_CASES):
        x = torch.from_numpy(rng.standard_normal(R.COEF_SHAPE))
        m = torch.from_numpy(rng.standard_normal(R.COEF_SHAPE))
        tv = torch.full((R.COEF_SHAPE[0],), t, dtype=torch.float64)
        s = Sampler(transport(path, pred, 0.05))
        sde_drift, diffusion_fn = s._Sampler__get_sde_diffusion_and_drift(diffusion_form=form, diffusion_norm=norm)
        model = lambda xx, tt: m
        D = diffusion_fn(x, tv)
        vals = {"x": x, "m": m, "drift": sde_drift(x, tv, model), "score": s.score(x, tv, model), "ode_drift": s.drift(x, tv, model),
                "D": torch.as_tensor(D, dtype=torch.float64) * torch.ones(R.COEF_SHAPE[0], 1, dtype=torch.float64)}
        for last in ("Mean", "Tweedie", "Euler"):
            vals[f"last_{last}"] = s._Sampler__get_last_step(sde_drift, last_step=last, last_step_size=lss)(x, tv, model)
        for k, v in vals.items():
            v = v.numpy()
            if k == "last_Tweedie" and t == 0.0:      # x / alpha(0): not a last step anyone takes; the t = 0 case is there for rr = 0
                continue
            assert v.dtype == np.float64 and np.isfinite(v).all(), (i, k)
            out[f"{i}_{k}"] = v
    np.savez_compressed(os.path.join(HERE, "sde_logp_transport_coef.npz"), **out)
    print("sde_logp_transport_coef", len(R.COEF_CASES), "cases")


if __name__ == "__main__":
    for name, case in R.SDE_CASES.items():
        gen_sde_case(name, *case)
    for name, case in R.LOGP_CASES.items():
        gen_logp_case(name, *case)
    gen_toys()
    gen_coef()

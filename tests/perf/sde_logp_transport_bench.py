#!/usr/bin/env python3
"""The SDE sampler and the likelihood under a non-default transport against the same solves under the default transport: time per
evaluation of `DiT.sample_sde_cfg` (Euler, GVP + score against Linear + velocity) and of `DiT.log_likelihood_cfg` (Euler, Linear + noise
against Linear + velocity) on the dentate_gyrus shape and vocabulary (8 layers, 14 clusters, guidance 1.5).  A plain script (not collected
by pytest).

Protocol: one module, one process; per workload one warm-up solve per side, then `--repeats` timed solves per side, ALTERNATED, a device
synchronise before and after every solve (host clock around work that ends in a synchronise).  min / median / max per solve and per
evaluation, and the verdict: a side is faster only when the medians differ by more than the run's repeat spread (the larger of the two
sides' max - min); otherwise the two are level.  The SDE launches the same kernels under both transports (only three scalars per update
differ); the likelihood's transport blend reads one more (2B, e) array per evaluation (the state the evaluation was made at).

usage: sde_logp_transport_bench.py [--cells 4096] [--precision bf16] [--repeats 7] [--sde-steps 26] [--logp-steps 11] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from oracle.weights import make_state_dict
from scldm_amd.nnets import DiT
from scldm_amd.transport import create_transport


def build(precision):
    with np.load(os.path.join(ROOT, "tests", "golden", "dit_base.npz"), allow_pickle=False) as f:
        kw, shapes, seed = json.loads(str(f["kwargs_json"])), json.loads(str(f["shapes_json"])), int(f["seed"])
    m = DiT(**kw)
    m.load_state_dict(make_state_dict({k: tuple(v) for k, v in shapes.items()}, seed), strict=True)
    m = m.cuda().eval()
    m.precision = precision
    return m


def solve_time(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert torch.isfinite(out).all()
    return dt


def compare(lines, title, run, n_evals, repeats):
    for fn in run.values():       # warm-up
        fn()
    times = {k: [] for k in run}
    for _ in range(repeats):
        for k, fn in run.items():
            times[k].append(solve_time(fn))
    lines.append(f"{title}: {n_evals} evaluations per solve")
    med = {}
    for k, t in times.items():
        med[k] = statistics.median(t)
        lines.append(f"    {k:22s} solve min {min(t) * 1e3:8.2f} ms  median {med[k] * 1e3:8.2f} ms  max {max(t) * 1e3:8.2f} ms   "
                     f"per evaluation {med[k] / n_evals * 1e6:8.1f} us")
    (ka, a), (kb, b) = med.items()
    spread = max(max(t) - min(t) for t in times.values())
    verdict = "level (within the repeat spread)" if abs(a - b) <= spread else f"{ka if a < b else kb} faster ({max(a, b) / min(a, b):.3f} x)"
    lines.append(f"    |difference of medians| {abs(a - b) * 1e3:.2f} ms, repeat spread {spread * 1e3:.2f} ms: {verdict}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=4096)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sde-steps", type=int, default=26)
    ap.add_argument("--logp-steps", type=int, default=11)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sde_logp_transport_bench.py needs the GPU: no timing is taken without one")
    m = build(a.precision)
    gen = torch.Generator(device="cuda").manual_seed(a.cells)
    z0 = torch.randn(a.cells, 16, 16, device="cuda", generator=gen)
    z2 = torch.cat([z0, z0])
    cond = {"clusters": torch.randint(0, 14, (a.cells,), device="cuda", generator=gen).repeat(2)}
    scales = {"clusters": 1.5}
    lines = [f"SDE sampler and likelihood under a non-default transport against the default transport, dentate_gyrus shape, guidance 1.5, "
             f"{a.cells} cells, {a.precision}, {a.repeats} alternated solves per side after one warm-up each ({torch.cuda.get_device_name(0)})"]
    score = create_transport("GVP", "score", None, None, 0.05, samplers_enabled=True)
    sde = lambda tr: m.sample_sde_cfg(z2, cond, scales, a.sde_steps, "euler", "sigma", 1.0, "Mean", 0.04, seed=11, transport=tr)
    compare(lines, f"SDE Euler solve, {a.sde_steps} grid points, form sigma, last step Mean",
            {"GVP + score": lambda: sde(score), "default transport": lambda: sde(None)}, a.sde_steps, a.repeats)
    noise = create_transport("Linear", "noise", None, None, 0.05, samplers_enabled=True)
    logp = lambda tr: m.log_likelihood_cfg(z2, cond, scales, a.logp_steps, "euler", seed=11, transport=tr)[0]
    compare(lines, f"likelihood Euler solve, {a.logp_steps} grid points",
            {"Linear + noise": lambda: logp(noise), "default transport": lambda: logp(None)}, a.logp_steps - 1, a.repeats)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

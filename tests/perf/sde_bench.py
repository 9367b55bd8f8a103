#!/usr/bin/env python3
"""What the fused SDE sampler costs beside the ODE sampler: dentate-shape sampling (8 layers, 14 clusters, guidance 1.5) of 4 096 cells
in bf16, `DiT.sample_sde_cfg` Euler-Maruyama over 101 grid points with the default "Mean" last step (101 evaluations, noise drawn
in registers from the seed) against `DiT.sample_ode_cfg` Euler over 102 grid points (101 evaluations).  A plain script (not collected
by pytest).

Protocol: both warmed up, then timed alternately in one process, `--repeats` solves each, a device synchronise around every solve;
min / median / max per solve and the median per evaluation are reported, and the ratio of the medians per evaluation.
The ODE code is the yardstick; the SDE evaluation runs the same conditioning and trunk launches and differs in its blend kernel
(cfg_blend_sde_kernel: the state update with the score terms and the normal draw, four elements per thread).

usage: sde_bench.py [--cells N] [--repeats R] [--out FILE]"""
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
    assert torch.isfinite(out).all()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sde_bench.py needs the GPU: no timing is taken without one")
    m = build(a.precision)
    gen = torch.Generator(device="cuda").manual_seed(0)
    z0 = torch.randn(a.cells, 16, 16, device="cuda", generator=gen)
    z2 = torch.cat([z0, z0])
    cond = {"clusters": torch.randint(0, 14, (a.cells,), device="cuda", generator=gen).repeat(2)}
    scales = {"clusters": 1.5}
    grid = 101
    runs = {"sde euler (101 grid points + Mean last step)": (grid, lambda: m.sample_sde_cfg(z2, cond, scales, grid, "euler", "sigma", 1.0, "Mean", 0.04, seed=1)),
            "ode euler (102 grid points)": (grid, lambda: m.sample_ode_cfg(z2, cond, scales, grid + 1, "euler"))}
    for _, fn in runs.values():
        solve_time(fn)
    times = {k: [] for k in runs}
    for _ in range(a.repeats):
        for k, (_, fn) in runs.items():
            times[k].append(solve_time(fn))
    lines = [f"{a.cells} cells, {a.precision}, {grid} evaluations per solve, {a.repeats} alternated solves each ({torch.cuda.get_device_name(0)})"]
    per_eval = {}
    for k, (evals, _) in runs.items():
        t = times[k]
        per_eval[k] = statistics.median(t) / evals
        lines.append(f"{k:48s} solve min {min(t) * 1e3:8.2f} ms  median {statistics.median(t) * 1e3:8.2f} ms  max {max(t) * 1e3:8.2f} ms   "
                     f"per evaluation {per_eval[k] * 1e6:8.1f} us")
    ks = list(runs)
    lines.append(f"per-evaluation ratio sde / ode: {per_eval[ks[0]] / per_eval[ks[1]]:.4f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

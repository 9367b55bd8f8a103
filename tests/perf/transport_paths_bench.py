#!/usr/bin/env python3
"""What a noise / score transport costs beside the default one.  A plain script (not collected by pytest).

Sampling: dentate-shape DiT (8 layers, 14 clusters, guidance 1.5) in bf16, 100 Euler evaluations (101 grid points), at 4 096 and at 128
cells: the Linear + noise one-call solve (`sample_ode_cfg(..., transport=)` -> scldm_sample_ode_transport) against the default velocity
solve (scldm_sample_ode) and against the host-driven route (`Sampler(transport).sample_ode` over `forward_with_cfg`).
Training: `FusedTrainStep` at 1 024 cells, GVP + noise + likelihood (scldm_dit_train_step_transport) against the default transport
(scldm_dit_train_step), both graphed.

Protocol: everything warmed up, then the variants of a group timed alternately in one process, `--repeats` times each, a device
synchronise around every timed call; min / median / max and the ratio of the medians are reported.

usage: transport_paths_bench.py [--repeats R] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

from sde_bench import build


def timed(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    return time.perf_counter() - t0


def alternate(runs, repeats):
    for fn in runs.values():
        timed(fn)
    times = {k: [] for k in runs}
    for _ in range(repeats):
        for k, fn in runs.items():
            times[k].append(timed(fn))
    return times


def report(title, times, per, unit, scale):
    lines = [title]
    med = {}
    for k, t in times.items():
        med[k] = statistics.median(t)
        lines.append(f"  {k:44s} min {min(t) * 1e3:8.3f} ms  median {med[k] * 1e3:8.3f} ms  max {max(t) * 1e3:8.3f} ms   {med[k] / per * scale:9.1f} {unit}")
    ks = list(times)
    for k in ks[1:]:
        lines.append(f"  ratio of the medians, {k} / {ks[0]}: {med[k] / med[ks[0]]:.4f}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("transport_paths_bench.py needs the GPU: no timing is taken without one")
    from scldm_amd.optim import AdamW
    from scldm_amd.training import FusedTrainStep
    from scldm_amd.transport import Sampler, create_transport
    lines = [f"{torch.cuda.get_device_name(0)}, bf16, {a.repeats} alternated repeats each"]
    m = build("bf16")
    noise = create_transport("Linear", "noise")
    grid = 101
    for cells in (4096, 128):
        gen = torch.Generator(device="cuda").manual_seed(0)
        z0 = torch.randn(cells, 16, 16, device="cuda", generator=gen)
        z2 = torch.cat([z0, z0])
        cond = {"clusters": torch.randint(0, 14, (cells,), device="cuda", generator=gen).repeat(2)}
        scales = {"clusters": 1.5}
        host = Sampler(noise).sample_ode(sampling_method="euler", num_steps=grid)
        runs = {"velocity, one call (scldm_sample_ode)": lambda: m.sample_ode_cfg(z2, cond, scales, grid, "euler"),
                "Linear + noise, one call": lambda: m.sample_ode_cfg(z2, cond, scales, grid, "euler", transport=noise),
                "Linear + noise, host driven": lambda: host(z2, m.forward_with_cfg, condition=cond, cfg_scale=scales)[-1]}
        lines += report(f"sampling, {cells} cells x {grid - 1} Euler evaluations (per evaluation in us)", alternate(runs, a.repeats), grid - 1, "us", 1e6)
    n = 1024
    steps = {}
    gen = torch.Generator(device="cuda").manual_seed(1)
    x1 = torch.randn(n, 16, 16, device="cuda", generator=gen)
    lab = {"clusters": torch.randint(0, 14, (n,), device="cuda", generator=gen)}
    for name, tr in (("default (scldm_dit_train_step)", create_transport()), ("GVP + noise + likelihood", create_transport("GVP", "noise", "likelihood"))):
        mt = build("bf16").train()
        opt = AdamW([p for p in mt.parameters() if p.requires_grad], lr=1e-4)
        fs = FusedTrainStep(mt, tr, opt, n, ["clusters"], seed=3, graph=True)
        steps[name] = lambda fs=fs: fs(x1, lab)
    lines += report(f"FusedTrainStep (graphed), {n} cells (per step in us)", alternate(steps, a.repeats * 3), 1, "us", 1e6)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

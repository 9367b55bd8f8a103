#!/usr/bin/env python3
"""What a log-likelihood evaluation costs: dentate-shape solve (8 layers, 14 clusters, guidance 1.5) of 4 096 cells in bf16, 50 Euler
evaluations (51 grid points).  A plain script (not collected by pytest).  Variants, per evaluation over the 3 x 4 096 rows of the CFG state:
  (a)  `DiT.log_likelihood_cfg`: the fused scldm_logp_ode (recording forward + input-gradient-only backward + the two logp kernels);
  (a') the same evaluation composed in Python from `DiT.input_vjp` (recording forward + scldm_dit_train_backward_dx) and torch
       elementwise work - the host-composed form of (a);
  (b)  (a') with the FULL training backward in place of the input-gradient-only one (autograd over `DiT.forward` with every parameter
       requiring a gradient: operand-pair stores, weight-gradient GEMMs, adaLN / embedding / timestep gradients, all discarded) - what
       could be written before scldm_dit_train_backward_dx existed;
  (c)  `DiT.sample_ode_cfg` Euler over the same grid: the forward-only floor.
Protocol: all warmed up, then timed alternately in one process, `--repeats` solves each, a device synchronise around every solve;
min / median / max per solve, the median per evaluation, and the ratios a / b, a' / b, a / c of the medians.

usage: logp_bench.py [--cells N] [--evals E] [--repeats R] [--out FILE]"""
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


def solve_time(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    return time.perf_counter() - t0


def composed(m, z2, lab, s_cfg, evals, seed, full_backward):
    """Euler likelihood solve, one evaluation = one 3B-row forward + backward, state arithmetic in torch."""
    B = z2.shape[0] // 2
    cond = {"clusters": torch.cat([torch.full((2 * B,), 14, device=z2.device), lab])}
    z, dl, h = z2.clone(), torch.zeros(2 * B, device=z2.device), 1.0 / evals
    for ev in range(evals):
        ep = m.logp_probe(seed, ev, B)
        xin = torch.cat([z, z[B:]])
        dout = torch.cat([ep[:B], ep[B:] * (1.0 - s_cfg), ep[B:] * s_cfg])
        tv = torch.full((3 * B,), 1.0 - ev * h, device=z2.device)
        if full_backward:
            xr = xin.requires_grad_(True)
            out = m(xr, tv, cond)
            (dx,) = torch.autograd.grad(out, xr, dout)
            out = out.detach()
        else:
            out, dx = m.input_vjp(xin, tv, cond, dout)
        u = out[B:2 * B]
        v = torch.cat([out[:B], u + s_cfg * (out[2 * B:] - u)])
        d = torch.cat([dx[:B], dx[B:2 * B] + dx[2 * B:]])
        dl = dl + h * (ep * d).sum(dim=(1, 2))
        z = z - h * v
    return -0.5 * 256 * 1.8378770664093453 - 0.5 * z.pow(2).sum(dim=(1, 2)) - dl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=4096)
    ap.add_argument("--evals", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("logp_bench.py needs the GPU: no timing is taken without one")
    m = build(a.precision)
    gen = torch.Generator(device="cuda").manual_seed(0)
    z0 = torch.randn(a.cells, 16, 16, device="cuda", generator=gen)
    z2 = torch.cat([z0, z0])
    lab = torch.randint(0, 14, (a.cells,), device="cuda", generator=gen)
    cond, scales, E = {"clusters": lab.repeat(2)}, {"clusters": 1.5}, a.evals
    runs = {"a  fused scldm_logp_ode": lambda: m.log_likelihood_cfg(z2, cond, scales, E + 1, "euler", seed=1)[0],
            "a' composed, input-gradient-only backward": lambda: composed(m, z2, lab, 1.5, E, 1, False),
            "b  composed, full training backward": lambda: composed(m, z2, lab, 1.5, E, 1, True),
            "c  sample_ode_cfg (forward only)": lambda: m.sample_ode_cfg(z2, cond, scales, E + 1, "euler")}
    for fn in runs.values():
        solve_time(fn)
    times = {k: [] for k in runs}
    for _ in range(a.repeats):
        for k, fn in runs.items():
            times[k].append(solve_time(fn))
    lines = [f"{a.cells} cells, {a.precision}, {E} Euler evaluations per solve, {a.repeats} alternated solves each ({torch.cuda.get_device_name(0)})"]
    per = {}
    for k in runs:
        t = times[k]
        per[k] = statistics.median(t) / E
        lines.append(f"{k:44s} solve min {min(t) * 1e3:9.2f} ms  median {statistics.median(t) * 1e3:9.2f} ms  max {max(t) * 1e3:9.2f} ms   "
                     f"per evaluation {per[k] * 1e3:8.3f} ms")
    ka, ka2, kb, kc = list(runs)
    lines.append(f"per-evaluation ratios: a / b {per[ka] / per[kb]:.4f}   a' / b {per[ka2] / per[kb]:.4f}   a / c {per[ka] / per[kc]:.4f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

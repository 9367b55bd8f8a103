#!/usr/bin/env python3
"""The reference's default sampler at the reference's operating point, fused against host-composed: `DiT.sample_ode_cfg(..., "dopri5")`
with the reference's defaults (atol = rtol = 1e-5, 2 save points - models.py:812 takes [-1]) on the dentate_gyrus shape and vocabulary
(8 layers, 14 clusters, guidance 1.5), 128 / 256 / 1 024 / 4 096 cells, bf16 and fp16.  A plain script (not collected by pytest).

Protocol: two modules with the same weights in ONE process - one created under SCLDM_DOPRI5_FUSED=1 (scldm_sample_ode_dopri5: one C call per
solve), one under SCLDM_DOPRI5_FUSED=0 (Sampler._sample_dopri5 over forward_with_cfg: one ctypes call per evaluation and per state kernel) -
one warm-up solve each, then `--repeats` timed solves each, ALTERNATED, a device synchronise before and after every solve (host clock
around work that ends in a synchronise).  min / median / max per solve, the evaluation and step counts of both routes (they must
agree: same solver, same decisions) and the verdict per batch size: the fused route is faster when its median is below the composed
route's by more than the run's repeat spread (the larger of the two routes' max - min).

usage: dopri5_fused_bench.py [--cells 128,256,1024,4096] [--precisions bf16,fp16] [--repeats 5] [--out FILE]"""
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


def build(precision, fused):
    with np.load(os.path.join(ROOT, "tests", "golden", "dit_base.npz"), allow_pickle=False) as f:
        kw, shapes, seed = json.loads(str(f["kwargs_json"])), json.loads(str(f["shapes_json"])), int(f["seed"])
    m = DiT(**kw)
    m.load_state_dict(make_state_dict({k: tuple(v) for k, v in shapes.items()}, seed), strict=True)
    m = m.cuda().eval()
    m.precision = precision
    os.environ["SCLDM_DOPRI5_FUSED"] = "1" if fused else "0"     # read when the native handle is created: now
    m._native_handle()
    return m


def solve_time(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert torch.isfinite(out).all()
    return dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="128,256,1024,4096")
    ap.add_argument("--precisions", default="bf16,fp16")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dopri5_fused_bench.py needs the GPU: no timing is taken without one")
    keep_env = os.environ.get("SCLDM_DOPRI5_FUSED")
    lines = [f"default sampler (dopri5, atol = rtol = 1e-5, 2 save points), dentate_gyrus shape, guidance 1.5, {a.repeats} alternated solves per route "
             f"after one warm-up each ({torch.cuda.get_device_name(0)})"]
    scales = {"clusters": 1.5}
    for precision in a.precisions.split(","):
        routes = {"fused": build(precision, True), "composed": build(precision, False)}
        for cells in (int(c) for c in a.cells.split(",")):
            gen = torch.Generator(device="cuda").manual_seed(cells)
            z0 = torch.randn(cells, 16, 16, device="cuda", generator=gen)
            z2 = torch.cat([z0, z0])
            cond = {"clusters": torch.randint(0, 14, (cells,), device="cuda", generator=gen).repeat(2)}
            run = {k: (lambda m=m: m.sample_ode_cfg(z2, cond, scales, 2, "dopri5")) for k, m in routes.items()}
            outs, stats = {}, {}
            for k, fn in run.items():       # warm-up (and the results the two routes are compared on)
                outs[k] = fn()
                stats[k] = dict(routes[k].last_solver_stats)
            times = {k: [] for k in run}
            for _ in range(a.repeats):
                for k, fn in run.items():
                    times[k].append(solve_time(fn))
            diff = float((outs["fused"] - outs["composed"]).abs().max() / outs["composed"].abs().max())
            counts = {k: (s["evaluations"], len(s["accepted_steps"]), len(s["rejected_steps"])) for k, s in stats.items()}
            lines.append(f"{precision} {cells:5d} cells: evaluations / accepted / rejected steps  fused {counts['fused']}  composed {counts['composed']}  "
                         f"{'(agree)' if counts['fused'] == counts['composed'] else '(DIFFER)'}   max |fused - composed| / max |composed| = {diff:.2e}")
            med = {}
            for k, t in times.items():
                med[k] = statistics.median(t)
                lines.append(f"    {k:9s} solve min {min(t) * 1e3:8.2f} ms  median {med[k] * 1e3:8.2f} ms  max {max(t) * 1e3:8.2f} ms   "
                             f"per evaluation {med[k] / counts[k][0] * 1e6:7.1f} us")
            spread = max(max(t) - min(t) for t in times.values())
            gain = med["composed"] - med["fused"]
            verdict = "fused faster" if gain > spread else ("fused slower" if -gain > spread else "within the repeat spread")
            lines.append(f"    composed - fused = {gain * 1e3:+.2f} ms ({med['composed'] / med['fused']:.3f} x), repeat spread {spread * 1e3:.2f} ms: {verdict}")
        del routes
    if keep_env is None:
        os.environ.pop("SCLDM_DOPRI5_FUSED", None)
    else:
        os.environ["SCLDM_DOPRI5_FUSED"] = keep_env
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

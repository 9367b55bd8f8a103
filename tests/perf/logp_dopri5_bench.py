#!/usr/bin/env python3
"""The reference's default likelihood solve (dopri5, atol 1e-6, rtol 1e-3) on the dentate_gyrus shape and vocabulary (8 layers, 14 clusters,
guidance 1.5), bf16, 128 / 1 024 / 4 096 cells: the fused `DiT.log_likelihood_cfg(..., "dopri5")` (scldm_logp_ode_dopri5, one C call)
against the only route there was before it - the generic `Sampler.sample_ode_likelihood("dopri5")` over differentiable
`_composed_forward_with_cfg` calls (autograd through the full training backward, ~40 elementwise launches per step).  A plain script (not
collected by pytest).

Two configurations per batch size: the reference's form (a fresh probe at every evaluation, `probe_per="evaluation"`) and one probe held
for the whole solve (`probe_per="solve"`).  Both routes get the same probes (the generator keyed by one seed, by evaluation index) and the
same first step (the fused route's automatic one, from its warm-up solve).  Protocol: one warm-up solve each, then `--repeats` timed solves
each, ALTERNATED in one process, a device synchronise before and after every solve.  Reported: min / median / max per solve, evaluations,
accepted / rejected steps, the time per evaluation, the generic / fused ratio of the medians with the run's repeat spread (the larger of
the two routes' max - min), and the fused route's per-evaluation overhead over the floor: the per-evaluation time of
`log_likelihood_cfg(..., "euler")` (50 evaluations of scldm_logp_ode, no host read) in the same run.  Last, the evaluation counts with a
fresh probe per evaluation against one probe per solve.  No threshold: this is a measurement.

usage: logp_dopri5_bench.py [--cells 128,1024,4096] [--precision bf16] [--repeats 3] [--out FILE]"""
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

ATOL, RTOL = 1e-6, 1e-3     # the reference's defaults (transport.py:371-378)


def solve_time(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert torch.isfinite(out).all()
    return dt


def generic(m, z2, cond, scales, seed, per_solve, first_step):
    """Today's other route: the generic sampler over differentiable forward calls, the probes the fused solve draws."""
    from scldm_amd.transport import Sampler, create_transport
    B = z2.shape[0] // 2
    count = iter(range(1 << 62))
    held = m.logp_probe(seed, 0, B) if per_solve else None
    draw = (lambda x: held) if per_solve else (lambda x: m.logp_probe(seed, next(count), B))
    fn = Sampler(create_transport()).sample_ode_likelihood(sampling_method="dopri5", num_steps=50, atol=ATOL, rtol=RTOL, first_step=first_step)
    logp, _ = fn(z2, lambda x, t: m._composed_forward_with_cfg(x, t.contiguous(), cond, scales), _probe=draw)
    st = fn.last_stats
    return logp, (st["evaluations"], len(st["accepted_steps"]), len(st["rejected_steps"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="128,1024,4096")
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("logp_dopri5_bench.py needs the GPU: no timing is taken without one")
    m = build(a.precision)
    scales, seed = {"clusters": 1.5}, 1
    lines = []

    def emit(line):         # (shown as it is measured: the larger batches take a while)
        lines.append(line)
        print(line, flush=True)

    emit(f"default likelihood solve (dopri5, atol {ATOL:g}, rtol {RTOL:g}), dentate_gyrus shape, guidance 1.5, {a.precision}, {a.repeats} alternated "
         f"solves per route after one warm-up each ({torch.cuda.get_device_name(0)})")
    counts_by = {}
    for cells in (int(c) for c in a.cells.split(",")):
        gen = torch.Generator(device="cuda").manual_seed(cells)
        z0 = torch.randn(cells, 16, 16, device="cuda", generator=gen)
        z2 = torch.cat([z0, z0])
        cond = {"clusters": torch.randint(0, 14, (cells,), device="cuda", generator=gen).repeat(2)}
        euler = lambda: m.log_likelihood_cfg(z2, cond, scales, 51, "euler", seed=seed)[0]
        euler()
        floor = statistics.median(solve_time(euler) for _ in range(a.repeats)) / 50
        emit(f"{cells:5d} cells: floor = log_likelihood_cfg(..., 'euler') {floor * 1e6:8.1f} us per evaluation (50 evaluations, no host read)")
        for per in ("evaluation", "solve"):
            fused = lambda fs=None: m.log_likelihood_cfg(z2, cond, scales, 50, "dopri5", atol=ATOL, rtol=RTOL, first_step=fs, probe_per=per, seed=seed)[0]
            out_f = fused()                                         # warm-up, automatic first step
            st = dict(m.last_solver_stats)
            first = st["first_step"]
            out_f = fused(first)
            st = dict(m.last_solver_stats)
            cnt_f = (st["evaluations"], st["accepted"], st["rejected"])
            out_g, cnt_g = generic(m, z2, cond, scales, seed, per == "solve", first)
            times = {"fused": [], "generic": []}
            for _ in range(a.repeats):
                times["fused"].append(solve_time(lambda: fused(first)))
                times["generic"].append(solve_time(lambda: generic(m, z2, cond, scales, seed, per == "solve", first)[0]))
            diff = float((out_f - out_g).abs().max() / out_g.abs().max())
            counts_by[(cells, per)] = cnt_f
            emit(f"  probe per {per}: first step {first:.6g}; evaluations / accepted / rejected steps  fused {cnt_f}  generic {cnt_g};  "
                 f"max |logp fused - generic| / max |logp| = {diff:.2e}")
            med = {}
            for k, t in times.items():
                med[k] = statistics.median(t)
                n_ev = (cnt_f if k == "fused" else cnt_g)[0]
                emit(f"    {k:8s} solve min {min(t) * 1e3:9.2f} ms  median {med[k] * 1e3:9.2f} ms  max {max(t) * 1e3:9.2f} ms   "
                     f"per evaluation {med[k] / n_ev * 1e6:8.1f} us")
            spread = max(max(t) - min(t) for t in times.values())
            per_f, per_g = med["fused"] / cnt_f[0], med["generic"] / cnt_g[0]
            emit(f"    generic / fused: per solve {med['generic'] / med['fused']:.3f} x, per evaluation {per_g / per_f:.3f} x  (repeat spread "
                 f"{spread * 1e3:.2f} ms);  fused over the Euler floor: {(per_f - floor) * 1e6:+.1f} us per evaluation ({per_f / floor:.3f} x)")
    emit("evaluations with a fresh probe per evaluation | one probe per solve (fused route, the reference's tolerances):")
    for cells in sorted({c for c, _ in counts_by}):
        ev, so = counts_by[(cells, "evaluation")], counts_by[(cells, "solve")]
        emit(f"  {cells:5d} cells: {ev[0]} ({ev[1]} accepted, {ev[2]} rejected) | {so[0]} ({so[1]} accepted, {so[2]} rejected)")
    text = "\n".join(lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

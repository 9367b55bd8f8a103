#!/usr/bin/env python3
"""Time the fused evaluation metrics (scldm_amd.evaluations.count_metrics) against the reference's formulation written in torch
on the same device - the expressions of models.py:321-331 and :899-900 with Pearson, mse and r2 taken from their definitions:
what a caller without the fused pass runs.  A plain script (not collected by pytest).

Protocol: warm-up, device events over windows of >= 0.5 s, the variants alternated in one process, three repeats (min / median /
max reported).  For the fused path: algorithmic bytes / time as GB/s and as a share of the 6.3 TB/s achievable HBM rate.
Algorithmic bytes: each matrix read twice with own-row-sum scaling (row sums, then moments), once with supplied divisors, plus
the row-block partials written once and read once.

usage: eval_metrics_bench.py [--out FILE] [--window SECONDS]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

from scldm_amd.evaluations import count_metrics

HBM_ACHIEVABLE = 6.3e12
SHAPES = [(128, 17002), (2048, 17002), (2048, 36130)]


def torch_composition(pred, true, div=None):
    dp = pred.sum(dim=1, keepdim=True) if div is None else div
    dt = true.sum(dim=1, keepdim=True) if div is None else div
    u = torch.log1p((pred / dp) * 10_000)
    v = torch.log1p((true / dt) * 10_000)
    zeros = ((pred == 0).float() == (true == 0).float()).float().mean()
    mse = ((u - v) ** 2).mean()
    mu, mv = u.mean(0), v.mean(0)
    du, dv = u - mu, v - mv
    pcc = torch.nanmean(((du * dv).sum(0) / ((du * du).sum(0).sqrt() * (dv * dv).sum(0).sqrt())).clamp(-1, 1))
    vu, vv = u.var(0), v.var(0)
    r2m = 1 - ((mv - mu) ** 2).sum() / ((mv - mv.mean()) ** 2).sum()
    r2v = 1 - ((vv - vu) ** 2).sum() / ((vv - vv.mean()) ** 2).sum()
    return mse, pcc, zeros, r2m, r2v


def algorithmic_bytes(n, G, own_sums: bool) -> int:
    rb = 64 if n >= 1024 else (32 if n >= 256 else 16)
    nrb = -(-n // rb)
    matrices = 2 * n * G * 4 * (2 if own_sums else 1)
    partials = 2 * 5 * nrb * G * 4          # written by the moments pass, read by the merge
    per_gene = 2 * 5 * G * 8                # merge -> finalize, in double
    return matrices + partials + per_gene


def timed(fn, window: float) -> float:
    """seconds per call, device events around a window of at least `window` seconds"""
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 4
    while True:
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        dt = e0.elapsed_time(e1) * 1e-3
        if dt >= window:
            return dt / reps
        reps = max(reps * 2, int(reps * window / max(dt, 1e-6) * 1.2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--window", type=float, default=0.5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "eval_metrics_bench.py needs the MI355X"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# fused count_metrics vs the torch composition; windows >= {a.window} s, 3 alternating repeats; {torch.cuda.get_device_name(0)}")
    gen = torch.Generator(device="cuda").manual_seed(0)
    for n, G in SHAPES:
        lam = torch.exp(torch.randn(G, device="cuda", generator=gen) * 1.2 - 1.0) * torch.exp(torch.randn((n, 1), device="cuda", generator=gen) * 0.5)
        true = torch.poisson(lam, generator=gen).float()
        pred = torch.poisson(0.7 * true + 0.3 * lam, generator=gen).float()
        true[:, -1] += 1
        pred[:, -1] += 1
        lib = true.sum(1, keepdim=True)
        variants = {
            "fused own-sum": lambda: count_metrics(pred, true),
            "torch own-sum": lambda: torch_composition(pred, true),
            "fused divisor": lambda: count_metrics(pred, true, pred_size=lib, true_size=lib),
            "torch divisor": lambda: torch_composition(pred, true, lib),
        }
        f, t = count_metrics(pred, true), torch_composition(pred, true)
        agree = max(abs(float(f[k]) - float(x)) for k, x in zip(("mse", "pcc", "zeros_accuracy", "r2_mean", "r2_var"), t))
        for fn in variants.values():   # warm-up of every variant at this shape
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(3):
            for k, fn in variants.items():
                times[k].append(timed(fn, a.window))
        say(f"shape {n} x {G}  (fused vs torch fp32, largest metric difference {agree:.2e})")
        for k, ts in times.items():
            lo, med, hi = min(ts), statistics.median(ts), max(ts)
            s = f"  {k:14s} {med * 1e6:10.1f} us  (min {lo * 1e6:.1f}, max {hi * 1e6:.1f})"
            if k.startswith("fused"):
                b = algorithmic_bytes(n, G, k.endswith("own-sum"))
                s += f"   {b / 1e6:8.1f} MB algorithmic -> {b / med / 1e9:7.1f} GB/s = {100 * b / med / HBM_ACHIEVABLE:5.1f} % of 6.3 TB/s"
            say(s)
        for mode in ("own-sum", "divisor"):
            say(f"  speed-up {mode}: {statistics.median(times['torch ' + mode]) / statistics.median(times['fused ' + mode]):.2f} x")
        del variants, pred, true, lam, lib
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

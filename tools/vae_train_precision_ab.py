#!/usr/bin/env python3
"""A/B timing of the TransformerVAE training step in precision "fp32" against "fp16", interleaved in one process on one GPU.

One step is what bench.py's vae_training_record times: TransformerVAE.forward -> -log_nb_positive(...).sum(1).mean() -> HIP backward ->
fused AdamW (global-norm clip 10), at the dentate_gyrus shape (G = 17 002 decoded genes, S = 6 147 encoder tokens).  Each repetition
times every (batch, precision) pair once, in alternating order, so that clock and thermal drift fall on both sides alike.
bench.py itself is not changed.

usage: tools/vae_train_precision_ab.py [--batches 128 512] [--reps 5] [--steps 10] [--warmup 3] [--only fp16 --reps 1] [--out FILE]
(--only runs one precision: the form to put under `rocprofv3 --kernel-trace --stats -- python tools/vae_train_precision_ab.py ...`)"""
import argparse
import gc
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from bench import make_optimizer, make_vae  # noqa: E402
from scldm_amd.distributions import log_nb_positive  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[128, 512])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["fp32", "fp16"], default=None)
    ap.add_argument("--n-genes", type=int, default=17002)
    ap.add_argument("--tokens", type=int, default=6147)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    precs = [a.only] if a.only else ["fp32", "fp16"]
    setups = {}
    for B in a.batches:
        vae = make_vae(a.n_genes, dev).train()
        g = torch.Generator().manual_seed(5)
        counts = torch.poisson(torch.full((B, a.n_genes), 0.5), generator=g).to(dev)
        genes = torch.arange(a.n_genes, device=dev).repeat(B, 1)
        gs = torch.stack([torch.sort(torch.randperm(a.n_genes, generator=g)[:a.tokens]).values for _ in range(B)]).to(dev)
        cs = counts.gather(1, gs)
        lib = counts.sum(1, keepdim=True)
        opt = make_optimizer(vae.parameters(), 1e-3, max_grad_norm=10.0)
        setups[B] = (vae, opt, counts, genes, gs, cs, lib)

    def step(B, prec):
        vae, opt, counts, genes, gs, cs, lib = setups[B]
        vae.precision = prec
        if prec == "fp16":
            opt.found_inf = vae.found_inf_flag()
        elif hasattr(opt, "found_inf"):
            del opt.found_inf
        opt.zero_grad(set_to_none=True)
        params, _ = vae(counts, genes, lib, cs, gs)
        loss = (-log_nb_positive(counts, params["mu"], params["theta"])).sum(1).mean()
        loss.backward()
        opt.step()
        return loss

    times = {(B, p): [] for B in a.batches for p in precs}
    flags = {}
    for B in a.batches:
        for p in precs:
            for _ in range(a.warmup):
                step(B, p)
    torch.cuda.synchronize()
    for rep in range(a.reps):
        order = precs if rep % 2 == 0 else precs[::-1]
        for B in a.batches:
            for p in order:
                gc.collect()
                gc.disable()
                try:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(a.steps):
                        loss = step(B, p)
                    torch.cuda.synchronize()
                    dt = (time.perf_counter() - t0) / a.steps
                finally:
                    gc.enable()
                times[(B, p)].append(1e3 * dt)
                if p == "fp16":
                    flags[B] = max(flags.get(B, 0.0), float(setups[B][0].found_inf_flag()))
                print(json.dumps({"rep": rep, "batch": B, "precision": p, "ms_per_step": round(1e3 * dt, 3),
                                  "loss": round(float(loss), 3)}), flush=True)
    summary = {"gpu": torch.cuda.get_device_name(), "n_genes": a.n_genes, "tokens_per_cell": a.tokens, "steps_per_rep": a.steps,
               "reps": a.reps, "results": {}}
    for B in a.batches:
        r = {}
        for p in precs:
            t = times[(B, p)]
            r[p] = {"median_ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3),
                    "all_ms": [round(x, 3) for x in t]}
        if len(precs) == 2:
            r["fp32_over_fp16"] = round(r["fp32"]["median_ms"] / r["fp16"]["median_ms"], 3)
        if B in flags:
            r["fp16_found_inf_max"] = flags[B]
        summary["results"][f"b{B}"] = r
    print(json.dumps(summary, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(summary, f, indent=1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""A/B timing of the TransformerVAE training step with atomic against ordered table gradients (TransformerVAE.deterministic),
interleaved in one process on one GPU; modelled on tools/vae_train_precision_ab.py.

One step is what bench.py's vae_training_record times: TransformerVAE.forward -> -log_nb_positive(...).sum(1).mean() -> HIP backward ->
fused AdamW (global-norm clip 10), at the dentate_gyrus shape (G = 17 002 decoded genes, S = 6 147 encoder tokens).  Each repetition
times every (batch, precision, mode) once, in alternating order, so that clock and thermal drift fall on both sides alike.  The
index build of the ordered mode (scldm_amd.vae.table_order: a stable sort through torch) is inside the ordered step's time and has
its own line in the record: it is also timed alone on the same inputs.  The record carries the reductions' algorithmic traffic
(`reduce_read_bytes`: one read of the row buffers plus the index); their time comes from a kernel trace,
`rocprofv3 --kernel-trace --stats -- python tools/vae_train_ordered_ab.py --only ordered --reps 1`.
There is no pass / fail threshold: the mode is opt-in whatever it costs.

usage: tools/vae_train_ordered_ab.py [--batches 128 512] [--precisions fp32 fp16] [--reps 5] [--steps 10] [--warmup 3]
                                     [--only atomic|ordered] [--out profiles/vae_train_ordered_ab.json]"""
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
from scldm_amd.vae import table_order  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[128, 512])
    ap.add_argument("--precisions", nargs="+", choices=["fp32", "fp16"], default=["fp32", "fp16"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["atomic", "ordered"], default=None)
    ap.add_argument("--n-genes", type=int, default=17002)
    ap.add_argument("--tokens", type=int, default=6147)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    modes = [a.only] if a.only else ["atomic", "ordered"]
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

    def step(B, prec, mode):
        vae, opt, counts, genes, gs, cs, lib = setups[B]
        vae.precision, vae.deterministic = prec, mode == "ordered"
        if prec == "fp16":
            opt.found_inf = vae.found_inf_flag()
        elif hasattr(opt, "found_inf"):
            del opt.found_inf
        opt.zero_grad(set_to_none=True)
        params, _ = vae(counts, genes, lib, cs, gs)
        loss = (-log_nb_positive(counts, params["mu"], params["theta"])).sum(1).mean()
        loss.backward()
        opt.step()
        assert vae.last_table_gradient_mode == mode
        return loss

    def timed(fn, n):
        gc.collect()
        gc.disable()
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                out = fn()
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0) / n, out
        finally:
            gc.enable()

    keys = [(B, p, m) for B in a.batches for p in a.precisions for m in modes]
    times = {k: [] for k in keys}
    index_ms = {B: [] for B in a.batches}
    for k in keys:
        for _ in range(a.warmup):
            step(*k)
    torch.cuda.synchronize()
    for rep in range(a.reps):
        order = modes if rep % 2 == 0 else modes[::-1]
        for B in a.batches:
            for p in a.precisions:
                for m in order:
                    dt, loss = timed(lambda: step(B, p, m), a.steps)
                    times[(B, p, m)].append(dt)
                    print(json.dumps({"rep": rep, "batch": B, "precision": p, "mode": m, "ms_per_step": round(dt, 3),
                                      "loss": round(float(loss), 3)}), flush=True)
            if "ordered" in modes:      # the index build alone (the stable sort and its plumbing), same inputs as the step's
                vae, _, _, genes, gs, cs, _ = setups[B]
                dt, (order_idx, _) = timed(lambda: table_order(genes, gs, cs, a.n_genes + 1), a.steps)
                index_ms[B].append(dt)
                print(json.dumps({"rep": rep, "batch": B, "index_build_ms": round(dt, 3), "entries": int(order_idx.numel())}), flush=True)
    stat = lambda t: {"median_ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3),
                      "all_ms": [round(x, 3) for x in t]}
    summary = {"gpu": torch.cuda.get_device_name(), "n_genes": a.n_genes, "tokens_per_cell": a.tokens, "steps_per_rep": a.steps,
               "reps": a.reps, "results": {}}
    for B in a.batches:
        r = {}
        for p in a.precisions:
            r[p] = {m: stat(times[(B, p, m)]) for m in modes}
            if len(modes) == 2:
                r[p]["ordered_over_atomic"] = round(r[p]["ordered"]["median_ms"] / r[p]["atomic"]["median_ms"], 3)
        if index_ms[B]:
            r["index_build"] = stat(index_ms[B])
            # row buffers written once and read once by the reductions, plus the index: the reductions' algorithmic traffic
            n_dec, n_enc = B * a.n_genes, B * a.tokens
            r["reduce_read_bytes"] = 4 * ((n_dec + n_enc) * 32 + n_dec) + 4 * 2 * (n_dec + n_enc) + 2 * 4 * (a.n_genes + 2)
        summary["results"][f"b{B}"] = r
    print(json.dumps(summary, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(summary, f, indent=1)


if __name__ == "__main__":
    main()

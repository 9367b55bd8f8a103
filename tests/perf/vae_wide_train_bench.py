#!/usr/bin/env python3
"""One training step of a wide TransformerVAE (`train_wide`: forward on the scldm_vaew_* inference route, the reference's loss in torch
ops, scldm_vaew_train_backward) against the same step by torch autograd over oracle.vae on device tensors, on the same GPU in one process.

    python tests/perf/vae_wide_train_bench.py [--rounds 5] [--B 4 16] [--G 36130] [--S 8000] [--out profiles/vae_wide_train_bench.txt]
    python tests/perf/vae_wide_train_bench.py --profile --B 4     one warm-up step and one step of the HIP side, nothing timed: the
                                                                   rocprofv3 target (tools/rocprof_stats.sh NAME tests/perf/vae_wide_train_bench.py --profile --B 4)

Shape: that of tests/perf/vae_wide_bench.py (256 wide, 8 + 8 layers, heads 8 / 4, 16 inducing points, latent 16, hidden 684; 36 130
genes decoded, 8 000 encoded).  One step is forward + -log_nb_positive(counts, mu, theta).sum(1).mean() + backward; the other side runs
under float32 matmul precision "highest" (exact fp32, what the HIP step computes).  Both sides are warmed up, then timed in alternating
rounds of one step between two device events.  The report gives each side's median round, its min-max range with the width in percent
of the median, the ratio of the medians, the peak of torch's allocator over each side's steps (`max_memory_allocated`, the parameters
and inputs included on both sides) and the largest gradient difference between the sides.  Needs a GPU."""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import vae as O  # noqa: E402
from oracle.vae_train import FROZEN, log_nb_positive  # noqa: E402
from oracle.weights import make_state_dict  # noqa: E402
from vae_wide_cases import build_module, oracle_config  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--B", type=int, nargs="+", default=[4, 16])
    ap.add_argument("--G", type=int, default=36130)
    ap.add_argument("--S", type=int, default=8000)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "vae_wide_train_bench needs the MI355X"
    torch.set_float32_matmul_precision("highest")
    G, S = args.G, args.S
    c = dict(n_embed=256, n_head=8, n_head_cross=4, n_inducing=16, n_embed_latent=16, n_layer=8, n_genes=G, multiple_of=4, shared_theta=True)
    vae = build_module(c)
    sd = make_state_dict({k: tuple(v.shape) for k, v in vae.state_dict().items()}, 7)
    vae.load_state_dict(sd, strict=True)
    vae = vae.cuda().train()
    vae.train_wide = True
    cfg = oracle_config(c)
    sd_dev = {k: v.cuda().requires_grad_(k not in FROZEN) for k, v in sd.items()}
    lines = [f"TransformerVAE wide route, one training step (forward + NB loss + backward, exact fp32): n_embed 256, 8 + 8 layers, heads 8 / 4, "
             f"16 inducing points, latent 16, hidden 684; G={G} S={S}; {torch.cuda.get_device_name(0)}",
             f"median of {args.rounds} alternating rounds of one step (device events); the other side: torch autograd over oracle.vae, matmul precision \"highest\""]
    for B in args.B:
        rng = np.random.default_rng(11)
        genes = torch.from_numpy(np.tile(np.arange(G, dtype=np.int64), (B, 1))).cuda()
        counts_np = rng.poisson(0.7, (B, G)).astype(np.float32)
        sub = np.stack([np.sort(rng.permutation(G)[:S]) for _ in range(B)])
        counts = torch.from_numpy(counts_np).cuda()
        lib = counts.sum(1, keepdim=True) + 1
        cs = torch.from_numpy(np.take_along_axis(counts_np, sub, 1)).cuda()
        gs = torch.from_numpy(sub.astype(np.int64)).cuda()

        def hip():
            for p in vae.parameters():
                p.grad = None
            params, _ = vae(counts, genes, lib, cs, gs)
            (-log_nb_positive(counts, params["mu"], params["theta"])).sum(dim=1).mean().backward()

        def eager():
            for p in sd_dev.values():
                p.grad = None
            z = O.encode(sd_dev, cfg, cs, gs)
            mu, theta = O.decode(sd_dev, cfg, z, genes, lib)
            (-log_nb_positive(counts, mu, theta)).sum(dim=1).mean().backward()

        if args.profile:
            hip()
            hip()
            torch.cuda.synchronize()
            return
        sides = {"hip": hip, "eager autograd": eager}
        peak = {}
        for name, fn in sides.items():
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            for _ in range(2):
                fn()
            torch.cuda.synchronize()
            peak[name] = torch.cuda.max_memory_allocated()
        worst = 0.0
        for k, p in vae.named_parameters():
            if k in FROZEN or k == "decoder_head.params.bias":
                continue
            ref = sd_dev[k].grad
            worst = max(worst, float((p.grad - ref).abs().max() / ref.abs().max()))
        times = {name: [] for name in sides}
        for _ in range(args.rounds):
            for name, fn in sides.items():
                times[name].append(timed(fn))
        med = {name: statistics.median(t) for name, t in times.items()}
        for name, t in times.items():
            lines.append(f"B={B:3d} {name:14s} {med[name]:9.2f} ms [{min(t):.2f}, {max(t):.2f}] ({100 * (max(t) - min(t)) / med[name]:.1f} %)   "
                         f"max_memory_allocated {peak[name] / 2**20:8.0f} MiB")
        lines.append(f"B={B:3d} eager autograd / hip = {med['eager autograd'] / med['hip']:.2f}x   largest gradient difference between the sides "
                     f"(scale-relative, every tensor but the frozen one and the shift-invariant head bias) {worst:.2e}")
        vae.__dict__["_wtrain_ws"] = None
        for p in list(vae.parameters()) + list(sd_dev.values()):
            p.grad = None
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

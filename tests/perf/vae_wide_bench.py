#!/usr/bin/env python3
"""Wide TransformerVAE inference (the scldm_vaew_* route) against the same module composed from eager torch ops, on the same GPU in one
process.

    python tests/perf/vae_wide_bench.py [--rounds 5] [--B 16] [--G 36130] [--S 8000] [--out profiles/vae_wide_bench.txt]
    python tests/perf/vae_wide_bench.py --profile        one encode + decode per precision, nothing timed: the rocprofv3 target
                                                          (tools/rocprof_stats.sh vae_wide tests/perf/vae_wide_bench.py --profile)

Shape: the census walkthrough's, as far as it is known - 256 wide, 8 + 8 layers, heads 8 / 4, 16 inducing points, latent 16 (the
dimensions are inferred from the 20M checkpoint's parameter count, not read from its config), 36 130 genes decoded, 8 000 encoded,
batch 16.  Sides: `encode` and `decode` of the module in "fp32" and "fp16", and oracle.vae's encode / decode on device tensors (torch
matmul / softmax / elementwise kernels) under float32 matmul precision "highest" (exact fp32, what "fp32" computes) and "high" (the
reference's setting, what "fp16" stands in for).  All sides are warmed up, then timed in alternating rounds between two device events;
a round is as many calls as fill about half a second.  The report gives each side's median round, its min-max range with the width in
percent of the median, and the ratios of the medians.  Needs a GPU."""
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
from oracle.weights import make_state_dict  # noqa: E402
from vae_wide_cases import build_module, oracle_config  # noqa: E402


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--G", type=int, default=36130)
    ap.add_argument("--S", type=int, default=8000)
    ap.add_argument("--round-ms", type=float, default=500.0)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "vae_wide_bench needs the MI355X"
    B, G, S = args.B, args.G, args.S
    c = dict(n_embed=256, n_head=8, n_head_cross=4, n_inducing=16, n_embed_latent=16, n_layer=8, n_genes=G, multiple_of=4, shared_theta=True)
    vae = build_module(c)
    sd = make_state_dict({k: tuple(v.shape) for k, v in vae.state_dict().items()}, 7)
    vae.load_state_dict(sd, strict=True)
    vae = vae.cuda().eval()
    cfg = oracle_config(c)
    sd_dev = {k: v.cuda() for k, v in sd.items()}
    rng = np.random.default_rng(11)
    genes = torch.from_numpy(np.tile(np.arange(G, dtype=np.int64), (B, 1))).cuda()
    counts = rng.poisson(0.7, (B, G)).astype(np.float32)
    sub = np.stack([np.sort(rng.permutation(G)[:S]) for _ in range(B)])
    lib = torch.from_numpy(counts.sum(1, keepdims=True) + 1).cuda()
    cs = torch.from_numpy(np.take_along_axis(counts, sub, 1)).cuda()
    gs = torch.from_numpy(sub.astype(np.int64)).cuda()
    z = torch.from_numpy(rng.standard_normal((B, 16, 16)).astype(np.float32)).cuda()

    def hip(prec, what):
        def run():
            vae.precision = prec
            return vae.encode(cs, gs) if what == "encode" else vae.decode(z, genes, lib).mu
        return run

    def eager(mode, what):
        def run():
            torch.set_float32_matmul_precision(mode)
            with torch.no_grad():
                return O.encode(sd_dev, cfg, cs, gs) if what == "encode" else O.decode(sd_dev, cfg, z, genes, lib)[0]
        return run

    if args.profile:
        for prec in ("fp32", "fp16"):
            hip(prec, "encode")()
            hip(prec, "decode")()
        torch.cuda.synchronize()
        return
    lines = [f"TransformerVAE wide route: n_embed 256, 8 + 8 layers, heads 8 / 4, 16 inducing points, latent 16, hidden 684; B={B} G={G} S={S}; "
             f"{torch.cuda.get_device_name(0)}",
             f"median of {args.rounds} alternating rounds (device events; calls per round chosen to fill ~{args.round_ms:.0f} ms)"]
    for what in ("encode", "decode"):
        sides = {"hip fp32": hip("fp32", what), "hip fp16": hip("fp16", what), "eager highest": eager("highest", what),
                 "eager high": eager("high", what)}
        outs, calls = {}, {}
        for name, fn in sides.items():
            for _ in range(2):
                outs[name] = fn()
            torch.cuda.synchronize()
            calls[name] = max(1, int(args.round_ms / max(timed(fn, 1), 1e-3)))
        times = {name: [] for name in sides}
        for _ in range(args.rounds):
            for name, fn in sides.items():
                times[name].append(timed(fn, calls[name]))
        torch.set_float32_matmul_precision("highest")
        med = {name: statistics.median(t) for name, t in times.items()}
        ref = outs["eager highest"].double()
        for name, t in times.items():
            diff = float((outs[name].double() - ref).abs().max() / ref.abs().max())
            lines.append(f"{what:6s} {name:14s} {med[name]:9.3f} ms [{min(t):.3f}, {max(t):.3f}] ({100 * (max(t) - min(t)) / med[name]:.1f} %)   "
                         f"{calls[name]:3d} calls / round   max|x - eager highest| / max = {diff:.2e}")
        lines.append(f"{what:6s} eager highest / hip fp32 = {med['eager highest'] / med['hip fp32']:.2f}x   eager high / hip fp16 = "
                     f"{med['eager high'] / med['hip fp16']:.2f}x   hip fp32 / hip fp16 = {med['hip fp32'] / med['hip fp16']:.2f}x")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""ScviVAE.forward on fp16 operands against the exact-fp32 HIP path and against eager torch at both fp32 matmul precisions, on the
same GPU in one process (the protocol of tests/perf/scvi_bench.py).

    python tests/perf/scvi_fp16_bench.py [--batches 128 512] [--rounds 7] [--calls 300] [--out profiles/scvi_fp16_bench.txt]
    python tests/perf/scvi_fp16_bench.py --profile 512 [--calls 20]      # only fp16 forwards of one batch size, for a kernel trace

Shape: G = 17 002, hidden 512, latent 32, 2 layers, shared theta.  Four sides: the HIP path with precision "fp32" and "fp16" (two
modules over the same state dict), and tests/scvi_ref.scvi_forward on device tensors with torch.set_float32_matmul_precision at
"highest" (exact fp32) and at "high" (what the reference's entry scripts select).  Per batch size all sides are warmed up with 50
calls, then timed in alternating rounds of `calls` calls between two device events; the report gives each side's median round, its
[min, max] over the rounds with the width in percent of the median, and the fp32 / fp16 ratio of the HIP medians with a note whether
the gap exceeds both round spreads.  Needs a GPU."""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import scvi_ref as R  # noqa: E402

G, H, NL, LAYERS = 17002, 512, 32, 2


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def build(sd, precision):
    vae = R.build_scvi(G, H, NL, LAYERS, True)
    vae.load_state_dict(sd, strict=True)
    vae = vae.cuda().eval()
    vae.fp16_enabled = True
    vae.precision = precision
    return vae


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[128, 512])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", type=int, default=None, metavar="B")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "scvi_fp16_bench needs the MI355X"
    sd = R.make_scvi_state_dict(R.scvi_shapes(G, H, NL, LAYERS, True), 7)
    if args.profile is not None:
        vae = build(sd, "fp16")
        counts, lib, eps = (torch.from_numpy(a).cuda() for a in R.make_inputs(G, NL, args.profile, 11))
        for _ in range(args.calls):
            vae(counts, None, lib, eps=eps)
        torch.cuda.synchronize()
        return
    v32, v16 = build(sd, "fp32"), build(sd, "fp16")
    sd_dev = {k: v.cuda() for k, v in sd.items()}
    lines = [f"ScviVAE.forward, G={G} hidden={H} latent={NL} layers={LAYERS} shared theta; {torch.cuda.get_device_name(0)}",
             f"median of {args.rounds} alternating rounds x {args.calls} calls (device events) after 50 warm-up calls per side"]
    for B in args.batches:
        counts, lib, eps = (torch.from_numpy(a).cuda() for a in R.make_inputs(G, NL, B, 11))

        def eager(mode):
            def f():
                return R.scvi_forward(sd_dev, counts, lib, eps)
            return mode, f
        sides = {"hip fp32": (None, lambda: v32(counts, None, lib, eps=eps)), "hip fp16": (None, lambda: v16(counts, None, lib, eps=eps)),
                 "eager highest": eager("highest"), "eager high": eager("high")}
        times = {k: [] for k in sides}
        out = {}
        with torch.no_grad():
            for k, (mode, fn) in sides.items():
                torch.set_float32_matmul_precision(mode or "highest")
                for _ in range(50):
                    out[k] = fn()
            torch.cuda.synchronize()
            for _ in range(args.rounds):
                for k, (mode, fn) in sides.items():
                    torch.set_float32_matmul_precision(mode or "highest")
                    times[k].append(timed(fn, args.calls))
        torch.set_float32_matmul_precision("highest")
        ref_mu = out["eager highest"]["mu"].double()
        rel = lambda m: float((m.double() - ref_mu).norm() / ref_mu.norm())            # noqa: E731
        diff = {"hip fp32": rel(out["hip fp32"][0].mu), "hip fp16": rel(out["hip fp16"][0].mu), "eager high": rel(out["eager high"]["mu"])}
        med = {k: statistics.median(t) for k, t in times.items()}
        pct = {k: 100 * (max(t) - min(t)) / med[k] for k, t in times.items()}
        for k, t in times.items():
            note = f"   mu rel-L2 vs eager highest {diff[k]:.2e}" if k in diff else ""
            lines.append(f"B={B:4d}  {k:14s} {med[k]:8.3f} ms [{min(t):.3f}, {max(t):.3f}] ({pct[k]:.1f} %){note}")
        gap = 100 * abs(med["hip fp32"] - med["hip fp16"]) / med["hip fp32"]
        clear = gap > max(pct["hip fp32"], pct["hip fp16"])
        lines.append(f"B={B:4d}  hip fp32 / hip fp16 = {med['hip fp32'] / med['hip fp16']:.2f}x   (gap {gap:.1f} % of the fp32 median; "
                     f"{'exceeds' if clear else 'does NOT exceed'} both round spreads)   eager highest / hip fp16 = "
                     f"{med['eager highest'] / med['hip fp16']:.2f}x   eager high / hip fp16 = {med['eager high'] / med['hip fp16']:.2f}x")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""ScviVAE.forward on the HIP path against the same module composed from eager torch ops, on the same GPU in one process.

    python tests/perf/scvi_bench.py [--batches 128 512] [--rounds 7] [--calls 300] [--out profiles/scvi_bench.txt]

Shape: G = 17 002, hidden 512, latent 32, 2 layers, shared theta (the bench shapes of the transformer VAE).  The eager baseline is
tests/scvi_ref.scvi_forward on device tensors (F.linear / F.batch_norm / F.silu / softmax: rocBLAS / hipBLASLt and elementwise kernels),
with torch's default fp32 matmul precision ("highest": exact fp32, what the HIP path computes).  Per batch size both sides are warmed
up, then timed in alternating rounds of `calls` calls between two device events; the report gives each side's median round, its
min-max range over the rounds with its width in percent of the median, and the ratio of the medians, plus the scale-relative difference
of the two results.  A round is a few hundred calls (about 0.1 s or more), so that it measures the work and not the clock.  The HIP
side is `ScviVAE.forward` as a caller sees it: the launches plus the wrapper's per-call host work (the pointer key over the ~30
parameter tensors, seven torch.empty calls, the argument checks), which the device-event window contains whenever the host is the
slower side.  A third column replays the same call from a captured graph in the same alternation: the launches without that host work,
so that what the wrapper costs and what the kernels cost can be told apart.  Needs a GPU."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[128, 512])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "scvi_bench needs the MI355X"
    sd = R.make_scvi_state_dict(R.scvi_shapes(G, H, NL, LAYERS, True), 7)
    vae = R.build_scvi(G, H, NL, LAYERS, True)
    vae.load_state_dict(sd, strict=True)
    vae = vae.cuda().eval()
    sd_dev = {k: v.cuda() for k, v in sd.items()}
    lines = [f"ScviVAE.forward, G={G} hidden={H} latent={NL} layers={LAYERS} shared theta, fp32; {torch.cuda.get_device_name(0)}",
             f"median of {args.rounds} alternating rounds x {args.calls} calls (device events); float32 matmul precision "
             f"{torch.get_float32_matmul_precision()!r}"]
    for B in args.batches:
        counts, lib, eps = (torch.from_numpy(a).cuda() for a in R.make_inputs(G, NL, B, 11))
        hip = lambda: vae(counts, None, lib, eps=eps)                                  # noqa: E731
        with torch.no_grad():
            eager = lambda: R.scvi_forward(sd_dev, counts, lib, eps)                   # noqa: E731
            for _ in range(50):
                out_h, out_e = hip(), eager()
            torch.cuda.synchronize()
            diff = float((out_h[0].mu.double() - out_e["mu"].double()).abs().max() / out_e["mu"].double().abs().max())
            # the HIP launches alone: the same call captured once and replayed, which takes the wrapper's host work out of the window
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                hip()
            for _ in range(50):
                graph.replay()
            torch.cuda.synchronize()
            t_h, t_e, t_g = [], [], []
            for _ in range(args.rounds):
                t_h.append(timed(hip, args.calls))
                t_e.append(timed(eager, args.calls))
                t_g.append(timed(graph.replay, args.calls))
        mh, me, mg = statistics.median(t_h), statistics.median(t_e), statistics.median(t_g)
        pct = lambda t, m: 100 * (max(t) - min(t)) / m                                 # noqa: E731
        lines.append(f"B={B:4d}  hip {mh:8.3f} ms [{min(t_h):.3f}, {max(t_h):.3f}] ({pct(t_h, mh):.1f} %)   eager torch {me:8.3f} ms "
                     f"[{min(t_e):.3f}, {max(t_e):.3f}] ({pct(t_e, me):.1f} %)   eager / hip = {me / mh:5.2f}x   "
                     f"hip launches alone (graph replay) {mg:8.3f} ms [{min(t_g):.3f}, {max(t_g):.3f}] ({pct(t_g, mg):.1f} %)   "
                     f"mu: max|hip - eager| / max|eager| = {diff:.2e}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

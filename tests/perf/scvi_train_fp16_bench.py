#!/usr/bin/env python3
"""One ScviVAE training step (forward, loss, backward; no optimizer) three ways on the same GPU in one process: the HIP step on fp16
operands (`train_fp16_enabled`, precision "fp16"), the HIP step in exact fp32 (the baseline) and the same model composed from eager
torch ops under autograd.

    python tests/perf/scvi_train_fp16_bench.py [--batches 128 512] [--rounds 7] [--calls 40] [--out profiles/scvi_train_fp16_bench.txt]
    python tests/perf/scvi_train_fp16_bench.py --trace-steps 12 --trace-batch 512 [--trace-precision fp16]     (under a kernel tracer)

Shape and protocol of tests/perf/scvi_train_bench.py (G = 17 002, hidden 512, latent 32, 2 + 2 layers, shared theta, dropout 0.1;
`ScviVAE.forward` in training mode, `scldm_amd.training.scvi_loss` and `backward()` as a caller runs them; the eager side with matmul
precision "highest" and the two NaN checks of `scvi_loss`).  The three sides are warmed up, then timed in alternating rounds of
`calls` steps between two device events; the report gives each side's median round, its min-max range with its width in percent of
the median, the ratios of the medians, and whether the fp16 / fp32 ratio lies outside both sides' round spread.  It also gives the
rel-L2 distance of the fp16 first-layer weight gradient to the fp32 one at dropout 0.  `--trace-steps N` runs N steps of one HIP
side and nothing else.  Needs a GPU."""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import scvi_ref as R  # noqa: E402
from scvi_train_bench import DROPOUT, G, H, LAYERS, NL, eager_step, timed  # noqa: E402


def build(sd, precision):
    vae = R.build_scvi(G, H, NL, LAYERS, True, dropout=DROPOUT)
    vae.load_state_dict(sd, strict=True)
    vae = vae.cuda().train()
    vae.train_enabled = True
    if precision == "fp16":
        vae.fp16_enabled = vae.train_fp16_enabled = True
        vae.precision = "fp16"
    return vae


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[128, 512])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-steps", type=int, default=0)
    ap.add_argument("--trace-batch", type=int, default=512)
    ap.add_argument("--trace-precision", default="fp16", choices=("fp16", "fp32"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "scvi_train_fp16_bench needs the MI355X"
    from scldm_amd.training import scvi_loss
    torch.set_float32_matmul_precision("highest")
    sd = R.make_scvi_state_dict(R.scvi_shapes(G, H, NL, LAYERS, True), 7)

    def stepper(vae, counts, lib, eps):
        def run(seed=5):
            for p in vae.parameters():
                p.grad = None
            lik, post, z = vae(counts, None, lib, eps=eps, seed=seed)
            sum(scvi_loss(vae, counts, lik, post, z).values()).backward()
        return run

    if args.trace_steps:
        counts, lib, eps = (torch.from_numpy(a).cuda() for a in R.make_inputs(G, NL, args.trace_batch, 11))
        run = stepper(build(sd, args.trace_precision), counts, lib, eps)
        for _ in range(args.trace_steps):
            run()
        torch.cuda.synchronize()
        print(f"traced {args.trace_steps} {args.trace_precision} steps at {args.trace_batch} cells")
        return

    v16, v32 = build(sd, "fp16"), build(sd, "fp32")
    sd_dev = {k: (v.cuda().requires_grad_(True) if v.dtype.is_floating_point and "running_" not in k and not k.startswith("prior.")
                  else v.cuda()) for k, v in sd.items()}
    params = [v for v in sd_dev.values() if v.requires_grad]
    lines = [f"ScviVAE training step (forward, loss, backward), G={G} hidden={H} latent={NL} layers={LAYERS}+{LAYERS} shared theta, "
             f"dropout {DROPOUT}; {torch.cuda.get_device_name(0)}",
             f"three sides in one process: HIP fp16 operands, HIP exact fp32 (baseline), eager torch (float32 matmul precision "
             f"{torch.get_float32_matmul_precision()!r}); median of {args.rounds} alternating rounds x {args.calls} steps (device events)"]
    for B in args.batches:
        counts, lib, eps = (torch.from_numpy(a).cuda() for a in R.make_inputs(G, NL, B, 11))
        s16, s32 = stepper(v16, counts, lib, eps), stepper(v32, counts, lib, eps)
        eager = lambda: eager_step(sd_dev, params, counts, lib, eps, DROPOUT)      # noqa: E731
        # distance of the two HIP sides at dropout 0, from the same running statistics
        for v in (v16, v32):
            v.load_state_dict(sd, strict=True)
            v.encoder.dropout = v.decoder.dropout = 0.0
        s16()
        s32()
        g16, g32 = v16.encoder.encoder_mlp[0].weight.grad.double(), v32.encoder.encoder_mlp[0].weight.grad.double()
        diff = float((g16 - g32).norm() / g32.norm())
        for v in (v16, v32):
            v.encoder.dropout = v.decoder.dropout = DROPOUT
        for _ in range(10):
            s16()
            s32()
            eager()
        torch.cuda.synchronize()
        t = {"fp16": [], "fp32": [], "eager": []}
        for _ in range(args.rounds):
            t["fp16"].append(timed(s16, args.calls))
            t["fp32"].append(timed(s32, args.calls))
            t["eager"].append(timed(eager, args.calls))
        med = {k: statistics.median(v) for k, v in t.items()}
        side = lambda k: (f"{med[k]:8.3f} ms [{min(t[k]):.3f}, {max(t[k]):.3f}] "       # noqa: E731
                          f"({100 * (max(t[k]) - min(t[k])) / med[k]:.1f} %)")
        apart = max(t["fp16"]) < min(t["fp32"]) or max(t["fp32"]) < min(t["fp16"])
        lines.append(f"B={B:4d}  hip fp16 {side('fp16')}   hip fp32 {side('fp32')}   eager torch {side('eager')}   "
                     f"fp32 / fp16 = {med['fp32'] / med['fp16']:5.2f}x ({'outside' if apart else 'INSIDE'} both sides' round spread)   "
                     f"eager / fp16 = {med['eager'] / med['fp16']:5.2f}x   eager / fp32 = {med['eager'] / med['fp32']:5.2f}x   "
                     f"dW_0 at dropout 0: rel-L2(fp16, fp32) = {diff:.2e}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

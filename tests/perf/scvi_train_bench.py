#!/usr/bin/env python3
"""One ScviVAE training step (forward, loss, backward; no optimizer) on the HIP path against the same model composed from eager
torch ops under autograd, on the same GPU in one process.

    python tests/perf/scvi_train_bench.py [--batches 128 512] [--rounds 7] [--calls 40] [--out profiles/scvi_train_bench.txt]

Shape: G = 17 002, hidden 512, latent 32, 2 + 2 layers, shared theta, dropout 0.1.  The HIP side is `ScviVAE.forward` in training mode
with `train_enabled`, `scldm_amd.training.scvi_loss` and `backward()` as a caller runs them (masks drawn on the device from a fixed
seed).  The eager side is F.linear / F.batch_norm(training=True) / F.silu / F.dropout / softmax / softplus and the reference's
log_nb_positive formula in torch ops, with matmul precision "highest" (exact fp32, what the HIP path computes), and the two NaN
checks of `scvi_loss` (the reference's; each one waits for the device), so that both sides do the same host work.  Both sides are warmed
up, then timed in alternating rounds of `calls` steps between two device events; the report gives each side's median round, its
min-max range over the rounds with its width in percent of the median, and the ratio of the medians, plus the scale-relative
difference of the two first-layer weight gradients at dropout 0 (the two sides draw different masks).  Needs a GPU."""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import scvi_ref as R  # noqa: E402
import scvi_train_ref as T  # noqa: E402

G, H, NL, LAYERS, DROPOUT = 17002, 512, 32, 2, 0.1
W0 = "encoder.encoder_mlp.0.weight"


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def eager_mlp(sd, prefix, x, p):
    i = 0
    while f"{prefix}.{4 * i}.weight" in sd:
        lin, bn = f"{prefix}.{4 * i}", f"{prefix}.{4 * i + 1}"
        x = F.linear(x, sd[lin + ".weight"], sd[lin + ".bias"])
        x = F.batch_norm(x, sd[bn + ".running_mean"], sd[bn + ".running_var"], sd[bn + ".weight"], sd[bn + ".bias"], True, 0.1, R.BN_EPS)
        x = F.dropout(F.silu(x), p, True)
        i += 1
    return x


def eager_step(sd, params, counts, lib, eps, p):
    for v in params:
        v.grad = None
    h = eager_mlp(sd, "encoder.encoder_mlp", torch.log1p(counts), p)
    loc = F.linear(h, sd["encoder_head.loc.weight"], sd["encoder_head.loc.bias"])
    scale = torch.exp(F.hardtanh(F.linear(h, sd["encoder_head.scale.weight"], sd["encoder_head.scale.bias"]), min_val=-7.0, max_val=5.0))
    z = loc + eps * scale
    g = eager_mlp(sd, "decoder.decoder_mlp", z, p)
    mu = F.softmax(F.linear(g, sd["decoder_head.mu.weight"], sd["decoder_head.mu.bias"]), dim=1) * lib.reshape(-1, 1)
    out = {"loc": loc, "scale": scale, "z": z, "mu": mu, "theta": F.softplus(sd["decoder_head.theta"])}
    llh, kl = T.scvi_losses(out, counts)
    for v in (llh, kl):      # scvi_loss's two NaN checks (the reference's): two host synchronisations per step on either side
        if torch.isnan(v).any():
            raise ValueError("NaN values detected")
    (llh + kl).backward()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[128, 512])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "scvi_train_bench needs the MI355X"
    from scldm_amd.training import scvi_loss
    torch.set_float32_matmul_precision("highest")
    sd = R.make_scvi_state_dict(R.scvi_shapes(G, H, NL, LAYERS, True), 7)
    vae = R.build_scvi(G, H, NL, LAYERS, True, dropout=DROPOUT)
    vae.load_state_dict(sd, strict=True)
    vae = vae.cuda().train()
    vae.train_enabled = True
    sd_dev = {k: (v.cuda().requires_grad_(True) if v.dtype.is_floating_point and "running_" not in k and not k.startswith("prior.")
                  else v.cuda()) for k, v in sd.items()}
    params = [v for v in sd_dev.values() if v.requires_grad]
    lines = [f"ScviVAE training step (forward, loss, backward), G={G} hidden={H} latent={NL} layers={LAYERS}+{LAYERS} shared theta, "
             f"dropout {DROPOUT}, fp32; {torch.cuda.get_device_name(0)}",
             f"median of {args.rounds} alternating rounds x {args.calls} steps (device events); float32 matmul precision "
             f"{torch.get_float32_matmul_precision()!r}"]
    for B in args.batches:
        counts, lib, eps = (torch.from_numpy(a).cuda() for a in R.make_inputs(G, NL, B, 11))

        def hip(seed=5):
            for p in vae.parameters():
                p.grad = None
            lik, post, z = vae(counts, None, lib, eps=eps, seed=seed)
            sum(scvi_loss(vae, counts, lik, post, z).values()).backward()
        eager = lambda: eager_step(sd_dev, params, counts, lib, eps, DROPOUT)      # noqa: E731
        # agreement at dropout 0 (same arithmetic on both sides)
        vae.encoder.dropout = vae.decoder.dropout = 0.0
        hip()
        eager_step(sd_dev, params, counts, lib, eps, 0.0)
        gh, ge = vae.encoder.encoder_mlp[0].weight.grad.double(), sd_dev[W0].grad.double()
        diff = float((gh - ge).abs().max() / ge.abs().max())
        vae.encoder.dropout = vae.decoder.dropout = DROPOUT
        for _ in range(10):
            hip()
            eager()
        torch.cuda.synchronize()
        t_h, t_e = [], []
        for _ in range(args.rounds):
            t_h.append(timed(hip, args.calls))
            t_e.append(timed(eager, args.calls))
        mh, me = statistics.median(t_h), statistics.median(t_e)
        pct = lambda t, m: 100 * (max(t) - min(t)) / m                                 # noqa: E731
        lines.append(f"B={B:4d}  hip {mh:8.3f} ms [{min(t_h):.3f}, {max(t_h):.3f}] ({pct(t_h, mh):.1f} %)   eager torch {me:8.3f} ms "
                     f"[{min(t_e):.3f}, {max(t_e):.3f}] ({pct(t_e, me):.1f} %)   eager / hip = {me / mh:5.2f}x   "
                     f"dW_0 at dropout 0: max|hip - eager| / max|eager| = {diff:.2e}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time TransformerVAE.decode / decode_sample with the Gaussian head against the negative-binomial head at the same shape and
operand policy.  The Gaussian decode launches a subset of the NB decode: the same cell-pair kernel, the per-gene kernel with the
LayerNorm + 32 -> 1 epilogue instead of the logit and the (max, sum exp) partials, and no finalize pass over (B, G).  A plain script
(not collected by pytest).

Protocol: both modules share every weight but the head's; warm-up, then device events over windows of >= `--window` seconds, the
eight variants (2 heads x decode / decode_sample x fp32 / fp16) alternated in one process, 5 repeats (min / median / max reported).
The yardstick of a Gaussian variant is the NB variant of the same run; the margin is that run's own repeat spread.

usage: gauss_decode_bench.py [--out FILE] [--window SECONDS] [--cells B] [--genes G]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

from oracle.weights import make_state_dict
from scldm_amd.layers import InputTransformerVAE
from scldm_amd.nnets import Decoder, Encoder
from scldm_amd.stochastic_layers import GaussianTransformerLayer, NegativeBinomialTransformerLayer
from scldm_amd.vae import TransformerVAE

REPEATS = 5


def build(n_genes, gaussian):
    enc = Encoder(n_layer=8, n_inducing_points=16, n_embed=32, n_embed_latent=16, n_head=8, n_head_cross=4, dropout=0.0, bias=False,
                  multiple_of=4, layernorm_eps=1e-8, norm_layer="layernorm", positional_encoding=True)
    dec = Decoder(n_genes=n_genes, n_embed=32, n_embed_latent=16, n_head=8, n_head_cross=4, n_layer=8, n_inducing_points=16,
                  dropout=0.0, bias=False, multiple_of=4, layernorm_eps=1e-8, norm_layer="layernorm", shared_embedding=True,
                  use_adaln=False)
    head = (GaussianTransformerLayer(n_embed=32, norm_layer="layernorm", layernorm_eps=1e-8) if gaussian else
            NegativeBinomialTransformerLayer(n_genes=n_genes, shared_theta=True, n_embed=32, norm_layer="layernorm", layernorm_eps=1e-8))
    return TransformerVAE(encoder=enc, decoder=dec, decoder_head=head, input_layer=InputTransformerVAE(n_genes=n_genes, n_embed=32, agg_func="log1p"))


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
    ap.add_argument("--cells", type=int, default=512)
    ap.add_argument("--genes", type=int, default=17002)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "gauss_decode_bench.py needs the MI355X"
    B, G = a.cells, a.genes
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    nb = build(G, False)
    nb.load_state_dict(make_state_dict({k: tuple(v.shape) for k, v in nb.state_dict().items()}, 77), strict=True)
    ga = build(G, True)
    sd = make_state_dict({k: tuple(v.shape) for k, v in ga.state_dict().items()}, 78)
    sd.update({k: v for k, v in nb.state_dict().items() if k in sd and not k.startswith("decoder_head.")})
    ga.load_state_dict(sd, strict=True)
    nb, ga = nb.cuda().eval(), ga.cuda().eval()
    gen = torch.Generator(device="cuda").manual_seed(0)
    z = torch.randn(B, 16, 16, device="cuda", generator=gen)
    genes = torch.arange(G, device="cuda").repeat(B, 1)
    lib = torch.full((B, 1), 5000.0, device="cuda")
    say(f"# TransformerVAE decode / decode_sample, Gaussian head vs negative-binomial head; {B} cells x {G} genes; windows >= {a.window} s, "
        f"{REPEATS} alternating repeats; {torch.cuda.get_device_name(0)}")
    variants = {}
    for prec in ("fp32", "fp16"):
        for head, m in (("nb", nb), ("gaussian", ga)):
            def dec(m=m, prec=prec):
                m.precision = prec
                return m.decode(z, genes, lib)

            def smp(m=m, prec=prec):
                m.precision = prec
                return m.decode_sample(z, genes, lib, seed=11)
            variants[f"{prec} decode        {head}"] = dec
            variants[f"{prec} decode_sample {head}"] = smp
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(REPEATS):
        for k, fn in variants.items():
            times[k].append(timed(fn, a.window))
    for k, ts in times.items():
        say(f"  {k:32s} {statistics.median(ts) * 1e3:8.3f} ms  (min {min(ts) * 1e3:.3f}, max {max(ts) * 1e3:.3f}; spread {100 * (max(ts) - min(ts)) / statistics.median(ts):.1f} %)")
    for prec in ("fp32", "fp16"):
        for op in ("decode       ", "decode_sample"):
            n, g = times[f"{prec} {op} nb"], times[f"{prec} {op} gaussian"]
            spread = (max(n) - min(n)) / statistics.median(n)
            ratio = statistics.median(g) / statistics.median(n)
            verdict = "faster" if ratio < 1 - spread else ("slower" if ratio > 1 + spread else "within the spread")
            say(f"  {prec} {op.strip():13s}: gaussian / nb = {ratio:.3f}  (nb repeat spread {100 * spread:.1f} %): {verdict}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

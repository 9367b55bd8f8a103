#!/usr/bin/env python3
"""A/B timing of the TransformerVAE training step with the unshared-theta NB head against the shared-theta NB head, fp32 and fp16,
interleaved in one process on one GPU.  A plain script (not collected by pytest).

One step is what bench.py's vae_training_record times: TransformerVAE.forward -> -log_nb_positive(...).sum(1).mean() (fused) -> HIP
backward -> fused AdamW (global-norm clip 10), at the dentate_gyrus shape (G = 17 002 decoded genes, S = 6 147 encoder tokens).  The
two modules share every weight but the head's.  Each repetition times every (batch, precision, head) triple once, in alternating
order, so that clock and thermal drift fall on both sides alike; the yardstick of the unshared step is the shared step of the same
run and precision, the margin that run's repeat spread.

usage: unshared_train_bench.py [--batches 128 512] [--precisions fp32 fp16] [--reps 5] [--steps 10] [--warmup 3]
                               [--only unshared --reps 1] [--out FILE] [--kernel-stats CSV ...]
--only runs one head: the form to put under `rocprofv3 --kernel-trace --stats` (tools/rocprof_stats.sh); --kernel-stats takes the
`*_kernel_stats.csv` files of such runs and copies the per-gene backward kernels' rows into the report."""
import argparse
import csv
import gc
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from bench import make_optimizer, make_vae  # noqa: E402
from scldm_amd.distributions import log_nb_positive  # noqa: E402
from scldm_amd.layers import InputTransformerVAE  # noqa: E402
from scldm_amd.nnets import Decoder, Encoder  # noqa: E402
from scldm_amd.stochastic_layers import NegativeBinomialTransformerLayer  # noqa: E402
from scldm_amd.vae import TransformerVAE, train_split  # noqa: E402


def make_unshared_vae(nb, n_genes, dev):
    """The unshared-theta module on the shared-theta module's weights (head: seeded like bench.make_vae's other tensors)."""
    kw = dict(n_embed=32, n_embed_latent=16, n_head=8, n_head_cross=4, n_layer=8, dropout=0.0, bias=False, multiple_of=4,
              layernorm_eps=1e-8, norm_layer="layernorm")
    vae = TransformerVAE(Encoder(n_inducing_points=16, positional_encoding=True, **kw),
                         Decoder(n_genes=n_genes, n_inducing_points=16, shared_embedding=True, use_adaln=False, **kw),
                         NegativeBinomialTransformerLayer(n_genes=n_genes, shared_theta=False, n_embed=32),
                         InputTransformerVAE(n_genes=n_genes, n_embed=32, agg_func="log1p"))
    g = torch.Generator().manual_seed(6)
    sd = {k: v.detach().cpu() for k, v in nb.state_dict().items() if not k.startswith("decoder_head.")}
    for k, v in vae.state_dict().items():
        if k.startswith("decoder_head."):
            sd[k] = torch.randn(v.shape, generator=g) * 0.05
    vae.load_state_dict(sd, strict=True)
    vae = vae.to(dev).train()
    vae.train_unshared_theta = True
    return vae


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[128, 512])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--precisions", nargs="+", choices=["fp32", "fp16"], default=["fp32", "fp16"])
    ap.add_argument("--only", choices=["shared", "unshared"], default=None)
    ap.add_argument("--n-genes", type=int, default=17002)
    ap.add_argument("--tokens", type=int, default=6147)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-stats", nargs="*", default=[])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "unshared_train_bench.py needs the MI355X"
    dev = torch.device("cuda")
    heads = [a.only] if a.only else ["shared", "unshared"]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    setups = {}
    for B in a.batches:
        nb = make_vae(a.n_genes, dev).train()
        un = make_unshared_vae(nb, a.n_genes, dev)
        g = torch.Generator().manual_seed(5)
        counts = torch.poisson(torch.full((B, a.n_genes), 0.5), generator=g).to(dev)
        genes = torch.arange(a.n_genes, device=dev).repeat(B, 1)
        gs = torch.stack([torch.sort(torch.randperm(a.n_genes, generator=g)[:a.tokens]).values for _ in range(B)]).to(dev)
        cs = counts.gather(1, gs)
        lib = counts.sum(1, keepdim=True)
        mods = {"shared": nb, "unshared": un}
        opts = {k: make_optimizer(m.parameters(), 1e-3, max_grad_norm=10.0) for k, m in mods.items() if k in heads}
        setups[B] = (mods, opts, counts, genes, gs, cs, lib)

    def step(B, prec, head):
        mods, opts, counts, genes, gs, cs, lib = setups[B]
        vae, opt = mods[head], opts[head]
        vae.precision = prec
        opt.zero_grad(set_to_none=True)
        params, _ = vae(counts, genes, lib, cs, gs)
        loss = (-log_nb_positive(counts, params["mu"], params["theta"])).sum(1).mean()
        loss.backward()
        opt.step()
        return loss

    say(f"# TransformerVAE training step, unshared-theta NB head vs shared-theta NB head; G = {a.n_genes}, S = {a.tokens}; {a.reps} alternating "
        f"repetitions of {a.steps} steps after {a.warmup} warm-up steps; {torch.cuda.get_device_name(0)}")
    cases = [(B, p) for B in a.batches for p in a.precisions]
    times = {(B, p, h): [] for B, p in cases for h in heads}
    for B, p in cases:
        for h in heads:
            for _ in range(a.warmup):
                step(B, p, h)
    torch.cuda.synchronize()
    for rep in range(a.reps):
        order = heads if rep % 2 == 0 else heads[::-1]
        for B, p in cases:
            for h in order:
                gc.collect()
                gc.disable()
                try:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(a.steps):
                        loss = step(B, p, h)
                    torch.cuda.synchronize()
                    dt = (time.perf_counter() - t0) / a.steps
                finally:
                    gc.enable()
                times[(B, p, h)].append(1e3 * dt)
                print(f"rep {rep} batch {B} {p} {h}: {1e3 * dt:.3f} ms / step, loss {float(loss):.3f}", flush=True)
    for B, p in cases:
        dec, pool = train_split(B, a.tokens, a.n_genes)
        say(f"batch {B} {p} (per-gene backward: {dec[0]} tiles x {dec[1]} chunks per cell; pooling {pool[0]} x {pool[1]})")
        for h in heads:
            t = times[(B, p, h)]
            say(f"  {h:9s} {statistics.median(t):9.3f} ms / step  (min {min(t):.3f}, max {max(t):.3f}; spread "
                f"{100 * (max(t) - min(t)) / statistics.median(t):.1f} %)")
        if len(heads) == 2:
            n, g = times[(B, p, "shared")], times[(B, p, "unshared")]
            per_rep = [y / x for x, y in zip(n, g)]
            say(f"  unshared / shared = {statistics.median(g) / statistics.median(n):.3f}  (per repetition {min(per_rep):.3f} .. {max(per_rep):.3f})")
    for path in a.kernel_stats:
        say(f"# rocprofv3 --kernel-trace --stats, {os.path.basename(path)}: the per-gene backward kernels and the five largest (times in us)")
        with open(path) as fh:
            rows = list(csv.DictReader(fh))
        name = lambda r: r.get("Name") or r.get("KernelName") or ""
        tot = lambda r: float(r.get("TotalDurationNs") or 0.0) / 1e3
        rows.sort(key=tot, reverse=True)
        keep = [r for i, r in enumerate(rows) if i < 5 or "dec_gene_bwd" in name(r)]
        for r in keep:
            calls = int(float(r.get("Calls") or 0))
            say(f"  {name(r)[:96]:96s} calls {calls:4d}  total {tot(r):11.1f}  avg {tot(r) / max(calls, 1):9.1f}  {float(r.get('Percentage') or 0):6.2f} %")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

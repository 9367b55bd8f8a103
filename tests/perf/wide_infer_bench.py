#!/usr/bin/env python3
"""What the record-free inference route buys a shape outside the fused family: a guided Euler solve (20 evaluations, joint replogle
vocabulary cell_line 4 x gene 2024, guidance 2.0) of the DiT-L shape bench.py trains (1 024 wide, 24 layers, 16 heads) in bf16, at 128
and 1 024 cells - `DiT.sample_ode_cfg` through scldm_dit_infer_sample_ode against the route composed from scldm_dit_train_forward
calls (SCLDM_WIDE_INFER=0).  A plain script (not collected by pytest).

Protocol: both routes are built in one process (the knob is read when a module's native handle is created), warmed up, then timed
alternately, `--repeats` solves each with a device synchronise around every solve; min / median / max per solve, torch.cuda.max_memory_allocated
of one further solve per route from an empty allocator cache (the weights and both modules' mirrors are in both figures) and the number of
conditioning rows are reported.  The labels are drawn uniformly from the whole vocabulary: at 1 024 cells nearly every cell has its own
row, the least favourable case for the de-duplicated conditioning.

The default rule this measurement serves: the new route is the default only if, at both sizes, its median is not above the composed
route's by more than that run's own repeat spread (max - min of the composed route's solves).

usage: wide_infer_bench.py [--cells 128,1024] [--repeats R] [--evals E] [--layers L] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch

from oracle.weights import make_state_dict
from scldm_amd.nnets import DiT

VOCAB = {"cell_line": 4, "gene": 2024}


def build(n_layer, precision, wide_infer):
    os.environ["SCLDM_WIDE_INFER"] = "1" if wide_infer else "0"
    m = DiT(n_embed=1024, n_embed_input=16, n_layer=n_layer, n_head=16, seq_len=16, dropout=0.0, bias=True, norm_layer="layernorm",
            multiple_of=4, layernorm_eps=1e-8, class_vocab_sizes=VOCAB, condition_strategy="joint", cfg_dropout_prob=0.8)
    m.load_state_dict(make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, 0), strict=True)
    m = m.cuda().eval()
    m.precision = precision
    m._native_handle()          # the knob is read here
    os.environ.pop("SCLDM_WIDE_INFER")
    return m


def solve_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert torch.isfinite(out).all()
    return dt, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="128,1024")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--evals", type=int, default=20)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("wide_infer_bench.py needs the GPU: no timing is taken without one")
    routes = {"infer": build(a.layers, a.precision, True), "composed": build(a.layers, a.precision, False)}
    scales = {"cell_line": 2.0, "gene": 2.0}
    lines = [f"wide_infer_bench: DiT-L 1024 x {a.layers} layers x 16 heads, {a.precision}, joint {VOCAB}, {a.evals} Euler evaluations with guidance, "
             f"{a.repeats} repeats per route (alternating, device synchronise around each solve), {torch.cuda.get_device_name(0)}"]
    verdict = []
    for cells in [int(c) for c in a.cells.split(",")]:
        gen = torch.Generator(device="cuda").manual_seed(cells)
        z0 = torch.randn(cells, 16, 16, device="cuda", generator=gen)
        z2 = torch.cat([z0, z0])
        lab = {k: torch.randint(0, v, (cells,), device="cuda", generator=gen) for k, v in VOCAB.items()}
        cond = {k: torch.cat([v, v]) for k, v in lab.items()}
        rows = 1 + int(torch.unique(torch.stack([lab[k] for k in VOCAB], dim=1), dim=0).shape[0])
        run = {k: (lambda m=m: m.sample_ode_cfg(z2, cond, scales, a.evals + 1, "euler")) for k, m in routes.items()}
        times, peak, outs = {k: [] for k in run}, {k: 0 for k in run}, {}
        for k in run:                                   # warm-up (allocations, the mirrors' first cast-job tables)
            _, outs[k] = solve_time(run[k])
        for _ in range(a.repeats):                      # timing: steady state (the caching allocator keeps both routes' blocks)
            for k in run:
                times[k].append(solve_time(run[k])[0])
        for k in run:                                   # memory: one solve per route from an empty cache
            routes["infer"].__dict__.pop("_ws_wide", None)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            solve_time(run[k])
            peak[k] = torch.cuda.max_memory_allocated()
        rel = float((outs["infer"] - outs["composed"]).norm() / outs["composed"].norm())
        for k in run:
            t = times[k]
            lines.append(f"  {cells:5d} cells  {k:9s} min {min(t) * 1e3:9.2f} ms  median {statistics.median(t) * 1e3:9.2f} ms  max {max(t) * 1e3:9.2f} ms   "
                         f"max_memory_allocated {peak[k] / 2**30:7.2f} GiB")
        med = {k: statistics.median(times[k]) for k in run}
        spread = max(times["composed"]) - min(times["composed"])
        ok = med["infer"] <= med["composed"] + spread
        verdict.append(ok)
        lines.append(f"  {cells:5d} cells  conditioning rows {rows} (composed: {3 * cells}); median ratio composed / infer {med['composed'] / med['infer']:.2f}; "
                     f"rel-L2 between the routes' results {rel:.2e}; within the default rule: {ok}")
    lines.append(f"default rule (new route's median not above the composed route's by more than its repeat spread, at every size): {'met' if all(verdict) else 'NOT met'}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

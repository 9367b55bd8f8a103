#!/usr/bin/env python3
"""Generate the transport-path fixtures by RUNNING THE REFERENCE (build container only; see make_golden.py for the import stubs).

Run from the repo root:   python tests/golden/make_golden_transport_paths.py

Data only, every value produced by the reference's own code (case tables: tests/transport_paths_ref.py):
  transport_paths_coef.npz     ICPlan / GVPCPlan evaluated on float64 tensors at COEF_T (both interval ends included).
  transport_paths_kernel.npz   per n in KERNEL_N: x1, x0, t and an upstream gradient; per path the reference's `path_sampler.plan` and
                               the plain callable's output there; per case the reference's `Transport.training_losses` loss and its
                               autograd gradient w.r.t. the model output; per (path, prediction) its `get_drift()` output.  t and x0
                               enter by replacing `tr.sample` (the idiom of tests/test_gpu_train.py).
  transport_paths_train.npz    the same through the reference DiT (train_base2 of make_golden.py, B = 5): loss per case, pred per
                               path, and for GRAD_CASES the digest of every parameter gradient of loss.mean().
  transport_paths_solver.npz   the reference's ODE stepping is torchdiffeq (a stub here), so per SOLVER_CASES a plain Euler / Heun loop
                               over the reference's `get_drift()` and the reference DiT's `forward_with_cfg` on the fp32
                               linspace(sample_eps, 1 - sample_eps, num_steps), run in float32 and in float64 (the float64 DiT's
                               t_embedder.mlp is fed the double cast of `timestep_embedding`, which builds fp32 frequencies); both end
                               states are stored.
Checked before anything is written: everything finite, the training draws inside T_RANGE (the seed is searched for), and the reference's
fp32 results within 1e-5 (scale-relative) of its float64 ones.  Running the script twice gives identical bytes."""
from __future__ import annotations

import copy
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402  (installs the import stubs and puts the repo root on sys.path)
from scldm.layers import TimestepEmbedder  # noqa: E402
from scldm.transport import create_transport, path as ref_path  # noqa: E402

import transport_paths_ref as R  # noqa: E402

REF_AGREE = 1e-5


def scale_rel(a, b) -> float:
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def agree(a32, a64, what):
    assert np.isfinite(np.asarray(a32)).all() and np.isfinite(np.asarray(a64)).all(), f"{what}: not finite"
    err = scale_rel(a32, a64)
    assert err <= REF_AGREE, f"{what}: the reference's fp32 result is {err:.2e} off its float64 one"
    return err


def transport(path_type, prediction, loss_weight=None):
    return create_transport(path_type, prediction, loss_weight, None, 1e-3)    # (sample_eps given: the reference leaves it None otherwise)


def draws(n, seed0):
    """x1, x0, t (n rows) with every t inside T_RANGE: the first seed >= seed0 whose draws are."""
    for seed in range(seed0, seed0 + 1000):
        rng = np.random.default_rng(seed)
        x1 = rng.standard_normal((n, *R.ROW_SHAPE)).astype(np.float32)
        x0 = rng.standard_normal((n, *R.ROW_SHAPE)).astype(np.float32)
        t = rng.uniform(0, 1, (n,)).astype(np.float32)
        if t.min() >= R.T_RANGE[0] and t.max() <= R.T_RANGE[1]:
            return x1, x0, t, rng
    raise AssertionError("no seed puts the draws inside T_RANGE")


def double_dit(m):
    """The reference DiT in float64; the sinusoidal features stay the fp32 ones `timestep_embedding` builds, cast to double."""
    m64 = copy.deepcopy(m).double()
    te = m64.t_embedder
    te.forward = lambda t: te.mlp(TimestepEmbedder.timestep_embedding(t, te.frequency_embedding_size).double())
    return m64


def gen_coef():
    out = {"t": np.array(R.COEF_T, np.float64)}
    t = torch.tensor(R.COEF_T, dtype=torch.float64)
    x = torch.ones(len(R.COEF_T), 1, dtype=torch.float64)
    for name, plan in (("Linear", ref_path.ICPlan()), ("GVP", ref_path.GVPCPlan())):
        al, dal = plan.compute_alpha_t(t)
        sg, dsg = plan.compute_sigma_t(t)
        vals = {"alpha": al, "d_alpha": dal, "sigma": sg, "d_sigma": dsg, "ratio": plan.compute_d_alpha_alpha_ratio_t(t),
                "dv": plan.compute_drift(x, t)[1][:, 0]}
        for k, v in vals.items():
            v = (torch.as_tensor(v, dtype=torch.float64) * torch.ones_like(t)).numpy()
            assert np.isfinite(v).all()
            out[f"{name}_{k}"] = v
    np.savez_compressed(os.path.join(HERE, "transport_paths_coef.npz"), **out)


def run_losses(tr, model, x1, x0, t, gloss, dtype):
    """The reference's training_losses with (t, x0) injected: loss, pred and d (loss . gloss) / d pred."""
    tt, x0t, x1t = (torch.from_numpy(v).to(dtype) for v in (t, x0, x1))
    tr.sample = lambda x1_: (tt, x0t, x1_)
    keep = []

    def leaf_model(xt, tv, **kw):
        out = model(xt, tv, **kw).detach().requires_grad_(True)
        keep.append(out)
        return out

    terms = tr.training_losses(leaf_model, x1t)
    (terms["loss"] * torch.from_numpy(gloss).to(dtype)).sum().backward()
    return terms["loss"].detach().numpy(), keep[0].detach().numpy(), keep[0].grad.numpy()


def gen_kernel():
    out, worst = {}, 0.0
    for n in R.KERNEL_N:
        x1, x0, t, rng = draws(n, 9100 + n)
        gloss = rng.uniform(0.05, 1.0, (n,)).astype(np.float32)
        out.update({f"n{n}_x1": x1, f"n{n}_x0": x0, f"n{n}_t": t, f"n{n}_gloss": gloss})
        for path_type in ("Linear", "GVP"):
            plan = transport(path_type, "noise").path_sampler
            res = {}
            for dtype in (torch.float32, torch.float64):
                _, xt, ut = plan.plan(*(torch.from_numpy(v).to(dtype) for v in (t, x0, x1)))
                res[dtype] = (xt.numpy(), ut.numpy(), R.toy_model(xt, torch.from_numpy(t).to(dtype)).numpy())
            for i, key in enumerate(("xt", "ut", "pred")):
                worst = max(worst, agree(res[torch.float32][i], res[torch.float64][i], f"n{n} {path_type} {key}"))
                out[f"n{n}_{path_type}_{key}"] = res[torch.float32][i]
        for case in R.CASES:
            l32, _, d32 = run_losses(transport(*case), R.toy_model, x1, x0, t, gloss, torch.float32)
            l64, _, d64 = run_losses(transport(*case), R.toy_model, x1, x0, t, gloss, torch.float64)
            worst = max(worst, agree(l32, l64, f"n{n} {case} loss"), agree(d32, d64, f"n{n} {case} dpred"))
            out[f"n{n}_{R.case_key(*case)}_loss"], out[f"n{n}_{R.case_key(*case)}_dpred"] = l32, d32
        if n == R.KERNEL_N[0]:
            for path_type, prediction in R.DRIFT_CASES:
                res = {}
                for dtype in (torch.float32, torch.float64):
                    xt = torch.from_numpy(out[f"n{n}_{path_type}_xt"]).to(dtype)
                    with torch.no_grad():
                        res[dtype] = transport(path_type, prediction).get_drift()(xt, torch.from_numpy(t).to(dtype), R.toy_model).numpy()
                worst = max(worst, agree(res[torch.float32], res[torch.float64], f"drift {path_type} {prediction}"))
                out[f"drift_{path_type}_{prediction}"] = res[torch.float32]
    # the interval ends: plan / loss / drift of the reference in fp32 against its float64 (checked, not stored)
    for case in R.CASES:
        for t_end in (1e-3, 1 - 1e-3):
            x1, x0, _, rng = draws(3, 9300)
            t = np.full((3,), t_end, np.float32)
            gloss = np.ones(3, np.float32)
            l32, _, d32 = run_losses(transport(*case), R.toy_model, x1, x0, t, gloss, torch.float32)
            l64, _, d64 = run_losses(transport(*case), R.toy_model, x1, x0, t, gloss, torch.float64)
            worst = max(worst, agree(l32, l64, f"end {t_end} {case} loss"), agree(d32, d64, f"end {t_end} {case} dpred"))
            res = {}
            for dtype in (torch.float32, torch.float64):
                with torch.no_grad():
                    res[dtype] = transport(*case).get_drift()(torch.from_numpy(x1).to(dtype), torch.from_numpy(t).to(dtype), R.toy_model).numpy()
            worst = max(worst, agree(res[torch.float32], res[torch.float64], f"end {t_end} {case} drift"))
    np.savez_compressed(os.path.join(HERE, "transport_paths_kernel.npz"), **out)
    print("transport_paths_kernel: fp32 against float64, worst", worst)


def gen_train():
    kwargs, B, seed = mg.TRAIN_CASES["train_base2"]
    m, shapes = mg.build_dit(kwargs, seed)
    m64 = double_dit(m)
    x1, x0, t, rng = draws(B, 9500)
    labels = {k: rng.integers(0, v, (B,)).astype(np.int64) for k, v in kwargs["class_vocab_sizes"].items()}
    k0 = sorted(labels)[0]
    labels[k0][B // 2] = kwargs["class_vocab_sizes"][k0]          # one label replaced by its null token, as label dropout would
    cond = {k: torch.from_numpy(v) for k, v in labels.items()}
    out = {"kwargs_json": np.array(json.dumps({**kwargs, **mg.COMMON})), "seed": np.array(seed), "x1": x1, "x0": x0, "t": t,
           "shapes_json": np.array(json.dumps({k: list(v) for k, v in shapes.items()}))}
    for k, v in labels.items():
        out[f"label_{k}"] = v
    worst = 0.0
    for case in R.CASES:
        res = {}
        for dtype, model in ((torch.float32, m), (torch.float64, m64)):
            model.zero_grad(set_to_none=True)
            tr = transport(*case)
            tt, x0t = torch.from_numpy(t).to(dtype), torch.from_numpy(x0).to(dtype)
            tr.sample = lambda x1_, tt=tt, x0t=x0t: (tt, x0t, x1_)
            terms = tr.training_losses(lambda xt, tv, **kw: model(xt, tv, kw["condition"], force_drop_ids=False),
                                       torch.from_numpy(x1).to(dtype), {"condition": cond})
            res[dtype] = (terms["loss"].detach().numpy(), terms["pred"].detach().numpy())
            if dtype == torch.float32 and case in R.GRAD_CASES:
                terms["loss"].mean().backward()
                frozen = []
                for name, p in model.named_parameters():
                    if p.grad is None:
                        frozen.append(name)
                        continue
                    out[f"grad_{R.case_key(*case)}_{name}"] = mg.grad_digest(p.grad.numpy())
                out["frozen_json"] = np.array(json.dumps(frozen))
        worst = max(worst, agree(res[torch.float32][0], res[torch.float64][0], f"train {case} loss"),
                    agree(res[torch.float32][1], res[torch.float64][1], f"train {case} pred"))
        out[f"loss_{R.case_key(*case)}"] = res[torch.float32][0]
        out[f"pred_{case[0]}"] = res[torch.float32][1]
    np.savez_compressed(os.path.join(HERE, "transport_paths_train.npz"), **out)
    print("transport_paths_train: fp32 against float64, worst", worst)


def solve(drift, model_fn, z, ts, method, dtype, **kw):
    """Plain fixed-grid Euler / Heun over the reference's drift: state arithmetic in `dtype`, the grid the fp32 linspace."""
    x = z.to(dtype)
    ones = torch.ones(x.shape[0], dtype=dtype)
    with torch.no_grad():
        for i in range(len(ts) - 1):
            h = (ts[i + 1] - ts[i]).to(dtype)
            k1 = drift(x, ones * ts[i].to(dtype), model_fn, **kw)
            if method == "euler":
                x = x + h * k1
            else:
                k2 = drift(x + h * k1, ones * ts[i + 1].to(dtype), model_fn, **kw)
                x = x + (0.5 * h) * (k1 + k2)
    return x.numpy()


def gen_solver():
    out, worst = {}, 0.0
    for name, (dit_name, B, scale, path_type, prediction, method, num_steps) in R.SOLVER_CASES.items():
        kwargs, _, seed = {**mg.DIT_CASES, **mg.LATE_DIT_CASES}[dit_name]
        m, _ = mg.build_dit(kwargs, seed)
        m64 = double_dit(m)
        rng = np.random.default_rng(seed + 9700 + num_steps)
        z0 = rng.standard_normal((B, kwargs["seq_len"], kwargs["n_embed_input"])).astype(np.float32)
        names = sorted(kwargs["class_vocab_sizes"])
        labels = {k: rng.integers(0, kwargs["class_vocab_sizes"][k], (B,)).astype(np.int64) for k in names}
        scales = {k: (1.5 - 0.4 * i if scale is None else float(scale)) for i, k in enumerate(names)}
        tr = transport(path_type, prediction)
        t0, t1 = tr.check_interval(tr.train_eps, tr.sample_eps, sde=False, eval=True, reverse=False)
        ts = torch.linspace(t0, t1, num_steps)
        z2 = torch.from_numpy(np.concatenate([z0, z0]))
        cond2 = {k: torch.from_numpy(np.concatenate([v, v])) for k, v in labels.items()}
        ends = {}
        for dtype, model in ((torch.float32, m), (torch.float64, m64)):
            fn = lambda x, t, model=model, **kw: model.forward_with_cfg(x, t, **kw, cfg_scale=scales)
            ends[dtype] = solve(tr.get_drift(), fn, z2, ts, method, dtype, condition=cond2)
        worst = max(worst, agree(ends[torch.float32], ends[torch.float64], name))
        out.update({f"{name}_z0": z0, f"{name}_scales_json": np.array(json.dumps(scales)), f"{name}_end32": ends[torch.float32],
                    f"{name}_end64": ends[torch.float64], f"{name}_ts": ts.numpy()})
        for k, v in labels.items():
            out[f"{name}_label_{k}"] = v
        print(name, "|end| max", float(np.abs(ends[torch.float64]).max()), "fp32 against float64", scale_rel(ends[torch.float32], ends[torch.float64]))
    np.savez_compressed(os.path.join(HERE, "transport_paths_solver.npz"), **out)
    print("transport_paths_solver: worst", worst)


if __name__ == "__main__":
    gen_coef()
    gen_kernel()
    gen_train()
    gen_solver()

"""CPU restatement of the reference's likelihood sampler for the Linear path with a velocity model.  TEST INFRASTRUCTURE ONLY (a helper
module the log-likelihood tests import).

`Sampler.sample_ode_likelihood` of the reference (src/scldm/transport/transport.py:371-430, prior_logp :59-67) written as what it
computes.  With solver time s from 0 to 1, the model evaluated at t = fp32(1 - s), a probe eps in {-1, +1} per evaluation and
v = model(x, t):

    drift     d x / d s = -v,     d delta_logp / d s = logp_grad = sum eps * grad_x(sum v * eps)      (_likelihood_drift)
    grid      s = linspace(0, 1, num_steps) in fp32, h = float(s[i + 1] - s[i])                       (this project's fixed grid)
    Euler     x <- x + h (-v),  delta_logp <- delta_logp + h logp_grad
    Heun      k1 at (x, s_i);  k2 at (x + h k1x, s_{i+1});  x <- x + h / 2 (k1x + k2x), delta_logp likewise
    end       logp = prior_logp(x_end) - delta_logp,   prior_logp(z) = -N / 2 log 2 pi - sum z^2 / 2

The per-evaluation map (x, t, eps) -> (-v, logp_grad), prior_logp and the sign / time convention are the reference's (checked against
its own recorded runs, tests/golden/logp_*.npz, in tests/test_logp_cpu.py); the grid stepping is this project's fixed-grid convention
(the reference hands stepping to torchdiffeq, which is not vendored).  The model is any differentiable callable (x, t (n,)) -> v;
the probes are GIVEN ((n_evaluations, *x.shape), one slice per evaluation)."""
from __future__ import annotations

import math

import numpy as np
import torch

# the fixtures generated from the reference (tests/golden/make_golden_logp.py): name -> (DiT fixture, method, integration steps)
CASES = {
    "logp_base_euler": ("dit_base", "euler", 4),
    "logp_base_heun": ("dit_base", "heun", 3),
    "logp_me2_euler": ("dit_me2_256", "euler", 3),
    "logp_joint_euler": ("dit_joint", "euler", 3),
}
CASE_B = 3


def toy_model(x: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    """A plain differentiable callable with a state- and time-dependent, non-diagonal Jacobian (the toy fixture's model)."""
    te = t.view(-1, *([1] * (x.dim() - 1)))
    return -0.7 * x + torch.sin(3.0 * te) + 0.25 * torch.tanh(x.flip(-1)) * te


TOY_SEED = 20241
TOY_SHAPE = (4, 6)
TOY_RUNS = [("euler", 5), ("heun", 4), ("euler", 2)]   # (method, integration steps): one run each in logp_toy.npz, all from torch.manual_seed(TOY_SEED)


def n_evaluations(method: str, steps: int) -> int:
    return steps * (2 if method.lower() == "heun" else 1)


def prior_logp(z: torch.Tensor) -> torch.Tensor:
    n = z[0].numel()
    return z.new_tensor(-n / 2.0) * math.log(2 * math.pi) - z.pow(2).flatten(1).sum(1) / 2.0


def eval_times(method: str, steps: int) -> list[float]:
    """The model time t = fp32(1 - s) of every evaluation of a solve, in order (floats holding fp32 values)."""
    s = torch.linspace(0.0, 1.0, steps + 1)
    out = []
    for i in range(steps):
        out.append(float(1 - s[i]))
        if method.lower() == "heun":
            out.append(float(1 - s[i + 1]))
    return out


def likelihood_drift(x: torch.Tensor, model_fn, t: float, eps: torch.Tensor):
    """(-v, logp_grad, sum |grad| per row) of one evaluation."""
    tv = torch.full((x.shape[0],), t, dtype=torch.float32)
    with torch.enable_grad():
        xr = x.detach().requires_grad_(True)
        v = model_fn(xr, tv)
        grad = torch.autograd.grad(torch.sum(v * eps), xr)[0]
    dims = tuple(range(1, x.dim()))
    return -v.detach(), torch.sum(grad * eps, dim=dims), grad.abs().sum(dim=dims), tv


def logp_ref(x: torch.Tensor, model_fn, method: str, steps: int, probes: torch.Tensor):
    """Returns (logp, x_end, list of logp_grad, list of the (n,) t vectors the model saw, list of per-row sum |grad| (the scale of
    a logp_grad))."""
    method = method.lower()
    assert method in ("euler", "heun") and probes.shape[0] == n_evaluations(method, steps)
    s = torch.linspace(0.0, 1.0, steps + 1)
    dl = torch.zeros(x.shape[0], dtype=x.dtype)
    lgs, seen, scales = [], [], []
    e = 0

    def ev(xc, sv):
        nonlocal e
        k, lg, sc, tv = likelihood_drift(xc, model_fn, float(1 - sv), probes[e])
        e += 1
        lgs.append(lg)
        seen.append(tv)
        scales.append(sc)
        return k, lg

    x = x.detach()
    for i in range(steps):
        h = float(s[i + 1] - s[i])
        k1x, k1l = ev(x, s[i])
        if method == "euler":
            x, dl = x + h * k1x, dl + h * k1l
        else:
            k2x, k2l = ev(x + h * k1x, s[i + 1])
            x, dl = x + (0.5 * h) * (k1x + k2x), dl + (0.5 * h) * (k1l + k2l)
    return prior_logp(x) - dl, x, lgs, seen, scales


def load_case(name: str):
    """A DiT fixture of CASES on the oracle side: (fixture arrays, state dict, oracle config, z (2B,S,C), doubled labels, scales,
    (method, steps))."""
    import json

    from conftest import golden_json, load_golden
    from oracle.dit import DiTConfig
    from oracle.weights import make_state_dict
    dit_name, method, steps = CASES[name]
    f = load_golden(name)
    assert json.loads(str(f["settings_json"])) == [dit_name, method, steps], "tests/logp_ref.py: CASES and the stored fixture disagree"
    g = load_golden(dit_name)
    kw = golden_json(g, "kwargs_json")
    sd = make_state_dict({k: tuple(v) for k, v in golden_json(g, "shapes_json").items()}, int(g["seed"]))
    cfg = DiTConfig(n_embed=kw["n_embed"], n_embed_input=kw["n_embed_input"], n_layer=kw["n_layer"], n_head=kw["n_head"],
                    seq_len=kw["seq_len"], multiple_of=kw["multiple_of"], layernorm_eps=kw["layernorm_eps"],
                    class_vocab_sizes=kw["class_vocab_sizes"], condition_strategy=kw["condition_strategy"])
    z2 = torch.from_numpy(np.concatenate([f["x"], f["x"]]))
    cond2 = {k: torch.from_numpy(np.concatenate([f[f"label_{k}"]] * 2)) for k in cfg.class_vocab_sizes}
    return f, sd, cfg, z2, cond2, golden_json(f, "scales_json"), (method, steps)

"""CPU restatement of the reference's SDE sampler for the Linear path with a velocity model.  TEST INFRASTRUCTURE ONLY (a helper
module the SDE tests import).

`Sampler.sample_sde` of the reference (src/scldm/transport/transport.py:269-322, integrators.py:7-75, path.py:52-95) written as what
it computes: with v = model(x, t), score = (t v - x) / (1 - t), drift f = v + D(t) score = c_v v + c_x x,

    grid    t = linspace(0, t1, num_steps) in fp32, t1 = 1 - last_step_size (0 when last_step is None), dt = fp32(t[1] - t[0])
    Euler   x <- x + dt f(x, t) + sqrt(2 D dt) w
    Heun    xhat = x + sqrt(2 D(t) dt) w;  K1 = f(xhat, t);  K2 = f(xhat + dt K1, fp32(t + dt));  x <- xhat + dt / 2 (K1 + K2)
    last    Mean: x + last_step_size f(x, t1);  Tweedie: x + (1 - t1) v;  Euler: x + last_step_size v;  None: x

i.e. every update is x' = a_x x + a_v v + a_w w with three scalars formed in float64 from the fp32 times and rounded once - the
arithmetic of the fused sampler, checked against the reference's own recorded trajectories (tests/golden/sde_*.npz) in
tests/test_sde_cpu.py.  The model is any callable (x, t (n,)) -> v; the noise is GIVEN ((num_steps - 1, *x.shape), one slice per step).
"""
from __future__ import annotations

import math

import numpy as np
import torch

FORMS = ("sigma", "linear", "constant", "decreasing", "inccreasing-decreasing")
LAST_STEPS = (None, "Mean", "Tweedie", "Euler")
# the fixtures generated from the reference (tests/golden/make_golden_sde.py): name -> (DiT fixture, method, form, norm, last step,
# last step size, grid points)
CASES = {
    "sde_base_euler": ("dit_base", "Euler", "sigma", 1.0, "Mean", 0.04, 5),
    "sde_base_heun": ("dit_base", "Heun", "decreasing", 1.0, "Tweedie", 0.04, 4),
    "sde_joint_euler": ("dit_joint", "Euler", "inccreasing-decreasing", 0.5, "Euler", 0.04, 4),
    "sde_me2_heun": ("dit_me2_256", "Heun", "linear", 1.0, "Mean", 0.04, 3),
    "sde_base_nolast": ("dit_base", "Euler", "sigma", 1.0, None, 0.04, 4),
}
CASE_B = 3


def toy_model(x: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    """A plain callable with a state- and time-dependent velocity (the toy fixture's model)."""
    te = t.view(-1, *([1] * (x.dim() - 1)))
    return -0.7 * x + torch.sin(3.0 * te) + 0.25 * x.flip(-1) * te


TOY_SEED = 20240
TOY_SHAPE = (4, 6)
# (method, form, norm, last step, last step size, grid points) - one run each in sde_toy.npz, all from torch.manual_seed(TOY_SEED)
TOY_RUNS = [("Euler", "sigma", 1.0, "Mean", 0.04, 6), ("Heun", "decreasing", 0.5, "Tweedie", 0.1, 5),
            ("Euler", "inccreasing-decreasing", 1.0, "Euler", 0.04, 4), ("Heun", "linear", 1.0, "Euler", 0.04, 4),
            ("Euler", "linear", 0.5, None, 0.04, 5)]


def diffusion(form: str, norm: float, t: float) -> float:
    if form in ("sigma", "linear"):
        return norm * (1.0 - t)
    if form == "constant":
        return float(norm)
    if form == "decreasing":
        return 0.25 * (norm * math.cos(math.pi * t) + 1.0) ** 2
    if form == "inccreasing-decreasing":
        return norm * math.sin(math.pi * t) ** 2
    raise NotImplementedError(form)


def drift_coef(form: str, norm: float, t: float) -> tuple[float, float]:
    """(c_v, c_x) of f = c_v v + c_x x at time t."""
    D = diffusion(form, norm, t)
    return 1.0 + D * t / (1.0 - t), -D / (1.0 - t)


def grid(num_steps: int, last_step, last_step_size: float):
    """(t (num_steps,) fp32, dt as float of the fp32 difference, t1 as float of its fp32 value)."""
    if last_step is None:
        last_step_size = 0.0
    ts = torch.linspace(0, 1 - last_step_size, num_steps)
    return ts, float(ts[1] - ts[0]), float(torch.tensor(1 - last_step_size, dtype=torch.float32))


def eval_times(num_steps: int, method: str, last_step, last_step_size: float) -> list[float]:
    """The time of every model evaluation of a solve, in order (floats holding fp32 values)."""
    ts, dt, t1 = grid(num_steps, last_step, last_step_size)
    out = []
    for i in range(num_steps - 1):
        out.append(float(ts[i]))
        if method.lower() == "heun":
            out.append(float(ts[i] + torch.tensor(dt, dtype=torch.float32)))
    if last_step is not None:
        out.append(t1)
    return out


def f32(v: float) -> float:
    return float(np.float32(v))


@torch.no_grad()
def sample_sde_ref(x: torch.Tensor, model_fn, num_steps: int, method: str, form: str, norm: float, last_step, last_step_size: float,
                   noise: torch.Tensor):
    """Returns (list of num_steps states, list of the (n,) t vectors the model saw)."""
    method = method.lower()
    assert method in ("euler", "heun") and form in FORMS and last_step in LAST_STEPS
    ts, dt, t1 = grid(num_steps, last_step, last_step_size)
    if last_step is None:
        last_step_size = 0.0
    seen = []

    def model(xc, t):
        tv = torch.full((xc.shape[0],), t, dtype=torch.float32)
        seen.append(tv)
        return model_fn(xc, tv)

    xs = []
    for i in range(num_steps - 1):
        t = float(ts[i])
        a_w = f32(math.sqrt(2.0 * diffusion(form, norm, t) * dt))
        c_v, c_x = drift_coef(form, norm, t)
        w = noise[i]
        if method == "euler":
            x = (f32(1.0 + dt * c_x) * x + f32(dt * c_v) * model(x, t)) + a_w * w
        else:
            xhat = x + a_w * w
            k1 = f32(c_v) * model(xhat, t) + f32(c_x) * xhat
            xp = xhat + f32(dt) * k1
            t2 = float(ts[i] + torch.tensor(dt, dtype=torch.float32))
            c_v2, c_x2 = drift_coef(form, norm, t2)
            k2 = f32(c_v2) * model(xp, t2) + f32(c_x2) * xp
            x = xhat + f32(0.5 * dt) * (k1 + k2)
        xs.append(x)
    if last_step is not None:
        v = model(x, t1)
        if last_step == "Mean":
            c_v, c_x = drift_coef(form, norm, t1)
            x = f32(1.0 + last_step_size * c_x) * x + f32(last_step_size * c_v) * v
        elif last_step == "Tweedie":
            x = x + f32(1.0 - t1) * v
        else:
            x = x + f32(last_step_size) * v
    xs.append(x)
    return xs, seen


def load_case(name: str):
    """A DiT fixture of CASES on the oracle side: (fixture arrays, state dict, oracle config, z (2B,S,C), doubled labels, scales,
    (method, form, norm, last step, last step size, grid points))."""
    import json

    from conftest import golden_json, load_golden
    from oracle.dit import DiTConfig
    from oracle.weights import make_state_dict
    dit_name, *settings = CASES[name]
    f = load_golden(name)
    assert json.loads(str(f["settings_json"])) == [dit_name, *settings], "tests/sde_ref.py: CASES and the stored fixture disagree"
    g = load_golden(dit_name)
    kw = golden_json(g, "kwargs_json")
    sd = make_state_dict({k: tuple(v) for k, v in golden_json(g, "shapes_json").items()}, int(g["seed"]))
    cfg = DiTConfig(n_embed=kw["n_embed"], n_embed_input=kw["n_embed_input"], n_layer=kw["n_layer"], n_head=kw["n_head"],
                    seq_len=kw["seq_len"], multiple_of=kw["multiple_of"], layernorm_eps=kw["layernorm_eps"],
                    class_vocab_sizes=kw["class_vocab_sizes"], condition_strategy=kw["condition_strategy"])
    z2 = torch.from_numpy(np.concatenate([f["z0"], f["z0"]]))
    cond2 = {k: torch.from_numpy(np.concatenate([f[f"label_{k}"]] * 2)) for k in cfg.class_vocab_sizes}
    return f, sd, cfg, z2, cond2, golden_json(f, "scales_json"), tuple(settings)


def oracle_solve(name: str):
    """The restatement over the oracle DiT on a fixture's inputs and recorded noise: a zero-argument callable returning the
    (num_steps, 2B, S, C) stack (what tests/precision_class.py runs under its operand-rounding modes)."""
    from oracle.dit import dit_forward_with_cfg
    f, sd, cfg, z2, cond2, scales, (method, form, norm, last, lss, steps) = load_case(name)
    model = lambda x, t: dit_forward_with_cfg(sd, cfg, x, t, cond2, scales)
    return lambda: torch.stack(sample_sde_ref(z2, model, steps, method, form, norm, last, lss, torch.from_numpy(f["noise"]))[0])

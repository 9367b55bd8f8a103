"""CPU restatement of the reference's SDE sampler and likelihood sampler under every transport of the project (Linear | GVP x velocity |
noise | score), and the case tables of their fixtures.  TEST INFRASTRUCTURE ONLY (a helper module the tests import).

`Sampler.sample_sde` / `.sample_ode_likelihood` of the reference (src/scldm/transport/transport.py:152-430, integrators.py:7-75,
path.py:24-208) written as what they compute.  With m = model(x, t), rr = alpha / alpha' and Dv = (alpha'/alpha) sigma^2 - sigma sigma':

    drift      f_ode = a x + b m     (a, b) = (0, 1) velocity | (alpha'/alpha, Dv) score | (alpha'/alpha, -Dv/sigma) noise
    score      s = s_x x + s_m m     (-1/var, rr/var), var = sigma^2 - rr sigma' sigma  velocity | (0, 1) score | (0, -1/sigma) noise
    D(t)       SBDM norm Dv | sigma norm sigma | linear norm (1 - t) | constant norm | decreasing 0.25 (norm cos(pi t) + 1)^2
               | inccreasing-decreasing norm sin^2(pi t)
    SDE drift  f = f_ode + D s = c_x x + c_m m
    grid       t = linspace(t0, t1, num_steps) fp32; velocity (0, 1 - lss), noise / score (eps, 1 - eps if lss == 0 else 1 - lss)
    Euler      x <- x + dt f + sqrt(2 D dt) w
    Heun       xhat = x + sqrt(2 D dt) w;  K1 = f(xhat, t);  K2 = f(xhat + dt K1, fp32(t + dt));  x <- xhat + dt / 2 (K1 + K2)
    last       Mean x + lss f;  Euler x + lss f_ode;  Tweedie x / alpha + sigma^2 / alpha s;  None x
    likelihood solver time s over linspace(t0, t1, steps + 1), (t0, t1) = (0, 1) velocity | (eps, 1 - eps); model time t = fp32(1 - s);
               d x / d s = -(a x + b m);  logp_grad = a e + b (eps . (dm/dx)^T eps), formed as lg = ae + b * dot with ae = fp32(a e)

Every update is x' = a_x x + a_m m + a_w w with scalars formed in float64 from the fp32 times and rounded to fp32 once: the arithmetic of
the fused solves, checked against the reference's own recorded runs (tests/golden/sdet_*.npz, logpt_*.npz) in
tests/test_sde_logp_transport_cpu.py.  The model is any callable (x, t (n,)) -> m; noise and probes are GIVEN."""
from __future__ import annotations

import math

import numpy as np
import torch

FORMS = ("SBDM", "sigma", "linear", "constant", "decreasing", "inccreasing-decreasing")
SDE_EPS = 0.05     # sample_eps of the noise / score SDE fixtures (a solve started at 1e-3 with so few steps is all x / t)
# name -> (DiT fixture, path, prediction, method, form, norm, last step, last step size, grid points)
SDE_CASES = {
    "sdet_gvp_velocity_euler": ("dit_base", "GVP", "velocity", "Euler", "sigma", 1.0, "Mean", 0.04, 6),
    "sdet_gvp_velocity_heun": ("dit_base", "GVP", "velocity", "Heun", "inccreasing-decreasing", 1.0, "Tweedie", 0.1, 5),
    "sdet_linear_noise_euler": ("dit_me2_256", "Linear", "noise", "Euler", "SBDM", 1.0, "Mean", 0.04, 6),
    "sdet_gvp_score_heun": ("dit_me2_256", "GVP", "score", "Heun", "decreasing", 0.5, "Tweedie", 0.1, 5),
    "sdet_linear_score_heun_nolast": ("dit_base", "Linear", "score", "Heun", "linear", 1.0, None, 0.04, 5),
    "sdet_gvp_noise_euler": ("dit_base", "GVP", "noise", "Euler", "sigma", 1.0, "Euler", 0.04, 6),
}
# name -> (DiT fixture, path, prediction, method, integration steps, sample_eps)
LOGP_CASES = {
    "logpt_gvp_velocity_euler": ("dit_base", "GVP", "velocity", "euler", 4, 0.0),
    "logpt_linear_noise_euler": ("dit_me2_256", "Linear", "noise", "euler", 4, 0.05),
    "logpt_gvp_score_heun": ("dit_me2_256", "GVP", "score", "heun", 3, 0.05),
    "logpt_linear_score_heun": ("dit_base", "Linear", "score", "heun", 3, 0.05),
    "logpt_gvp_noise_euler": ("dit_base", "GVP", "noise", "euler", 4, 1e-3),
}
CASE_B = 3

TOY_SEED = 20250
TOY_SHAPE = (4, 6)
# (path, prediction, sample_eps, method, form, norm, last step, last step size, grid points): one run each in sdet_toy.npz, all from
# torch.manual_seed(TOY_SEED)
TOY_SDE_RUNS = [("GVP", "velocity", 0.0, "Euler", "sigma", 1.0, "Mean", 0.04, 6), ("Linear", "noise", 0.05, "Heun", "SBDM", 0.5, "Tweedie", 0.1, 5),
                ("GVP", "score", 0.05, "Euler", "decreasing", 1.0, "Euler", 0.04, 4), ("Linear", "score", 0.05, "Heun", "linear", 1.0, None, 0.04, 4),
                ("GVP", "noise", 0.1, "Euler", "inccreasing-decreasing", 0.5, None, 0.04, 5)]
# (path, prediction, sample_eps, method, integration steps): one run each in logpt_toy.npz
TOY_LOGP_RUNS = [("GVP", "velocity", 0.0, "euler", 5), ("Linear", "noise", 0.05, "heun", 4), ("GVP", "score", 0.05, "euler", 2),
                 ("Linear", "score", 1e-3, "heun", 3)]
# the coefficient fixture: (path, prediction, form, norm, t, last step size) - the reference's own functions on float64 tensors
COEF_CASES = [("GVP", "velocity", "sigma", 1.0, 0.0, 0.04), ("GVP", "velocity", "inccreasing-decreasing", 0.7, 0.37, 0.1),
              ("GVP", "velocity", "decreasing", 1.0, 0.9, 0.1), ("Linear", "noise", "SBDM", 1.0, 0.05, 0.04),
              ("Linear", "noise", "linear", 0.5, 0.96, 0.04), ("GVP", "score", "SBDM", 0.5, 0.3, 0.1), ("GVP", "score", "sigma", 1.0, 0.9, 0.1),
              ("Linear", "score", "constant", 0.3, 0.5, 0.04), ("GVP", "noise", "decreasing", 1.0, 0.62, 0.04)]
COEF_SHAPE = (3, 5)


def toy_model(x: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    """A plain differentiable callable with a state- and time-dependent, non-diagonal Jacobian (the toy fixtures' model)."""
    te = t.view(-1, *([1] * (x.dim() - 1)))
    return -0.7 * x + torch.sin(3.0 * te) + 0.25 * torch.tanh(x.flip(-1)) * te


def f32(v: float) -> float:
    return float(np.float32(v))


# ---------------------------------------------------------------------------------------------------------------- the scalar algebra
def path_coef(path: str, model: str, t: float) -> dict:
    """alpha, alpha', sigma, sigma', alpha'/alpha, Dv and the probability-flow (a, b) at t, in float64; infinities come as they are."""
    t = np.float64(t)
    with np.errstate(all="ignore"):
        if path == "GVP":
            h = np.float64(math.pi / 2)
            al, dal, sg, dsg = np.sin(t * h), h * np.cos(t * h), np.cos(t * h), -h * np.sin(t * h)
            ratio = h / np.tan(t * h)
            if t >= 1.0:      # the exact end point: cos(pi / 2) in float64 is the rounding residue of pi
                dal, sg, ratio = np.float64(0.0), np.float64(0.0), np.float64(0.0)
        else:
            al, dal, sg, dsg = t, np.float64(1.0), 1.0 - t, np.float64(-1.0)
            ratio = np.float64(1.0) / t
        dv = ratio * (sg * sg) - sg * dsg
        if model == "velocity":
            a, b = np.float64(0.0), np.float64(1.0)
        else:
            a, b = ratio, (dv if model == "score" else -dv / sg)
    return dict(alpha=al, d_alpha=dal, sigma=sg, d_sigma=dsg, ratio=ratio, dv=dv, a=a, b=b)


def sde_coef(path: str, model: str, form: str, norm: float, t: float) -> dict:
    """path_coef plus D, (s_x, s_m) and (c_x, c_m) at t."""
    k = path_coef(path, model, t)
    t = np.float64(t)
    with np.errstate(all="ignore"):
        D = {"SBDM": norm * k["dv"], "sigma": norm * k["sigma"], "linear": norm * (1.0 - t), "constant": np.float64(norm),
             "decreasing": 0.25 * (norm * np.cos(np.pi * t) + 1.0) ** 2, "inccreasing-decreasing": norm * np.sin(np.pi * t) ** 2}[form]
        if model == "velocity":
            rr = k["alpha"] / k["d_alpha"]
            var = k["sigma"] ** 2 - rr * k["d_sigma"] * k["sigma"]
            s_x, s_m = -1.0 / var, rr / var
        elif model == "score":
            s_x, s_m = np.float64(0.0), np.float64(1.0)
        else:
            s_x, s_m = np.float64(0.0), -1.0 / k["sigma"]
        k.update(D=D, s_x=s_x, s_m=s_m, c_x=k["a"] + D * s_x, c_m=k["b"] + D * s_m)
    return k


def last_coef(k: dict, last_step: str, lss: float) -> tuple[float, float]:
    with np.errstate(all="ignore"):
        if last_step == "Mean":
            return 1.0 + lss * k["c_x"], lss * k["c_m"]
        if last_step == "Euler":
            return 1.0 + lss * k["a"], lss * k["b"]
        q = k["sigma"] ** 2 / k["alpha"]
        return 1.0 / k["alpha"] + q * k["s_x"], q * k["s_m"]


def sde_interval(model: str, eps: float, lss: float) -> tuple[float, float]:
    if model == "velocity":
        return 0, 1 - lss
    return eps, (1 - eps if lss == 0 else 1 - lss)


def sde_grid(model: str, eps: float, num_steps: int, last_step, lss: float):
    """(t (num_steps,) fp32, dt as the fp32 tensor difference, t1 as float of its fp32 value)."""
    if last_step is None:
        lss = 0.0
    t0, t1 = sde_interval(model, eps, lss)
    ts = torch.linspace(t0, t1, num_steps)
    return ts, ts[1] - ts[0], float(torch.tensor(t1, dtype=torch.float32))


def sde_eval_times(model: str, eps: float, num_steps: int, method: str, last_step, lss: float) -> list[float]:
    ts, dt, t1 = sde_grid(model, eps, num_steps, last_step, lss)
    out = []
    for i in range(num_steps - 1):
        out.append(float(ts[i]))
        if method.lower() == "heun":
            out.append(float(ts[i] + dt))
    if last_step is not None:
        out.append(t1)
    return out


# ---------------------------------------------------------------------------------------------------------------- the SDE solve
@torch.no_grad()
def sample_sde_ref(x, model_fn, path, model, eps, num_steps, method, form, norm, last_step, lss, noise, zero_model=False):
    """Returns (list of num_steps states, list of the (n,) t vectors the model saw).  zero_model: the model output replaced by zeros
    (how much of a state the model term carries)."""
    method = method.lower()
    assert method in ("euler", "heun") and form in FORMS
    ts, dt_t, t1 = sde_grid(model, eps, num_steps, last_step, lss)
    dt = float(dt_t)
    if last_step is None:
        lss = 0.0
    seen = []

    def m_at(xc, t):
        tv = torch.full((xc.shape[0],), t, dtype=torch.float32)
        seen.append(tv)
        out = model_fn(xc, tv)
        return torch.zeros_like(out) if zero_model else out

    xs = []
    for i in range(num_steps - 1):
        t = float(ts[i])
        k = sde_coef(path, model, form, norm, t)
        a_w = f32(math.sqrt(2.0 * k["D"] * dt))
        w = noise[i]
        if method == "euler":
            x = (f32(1.0 + dt * k["c_x"]) * x + f32(dt * k["c_m"]) * m_at(x, t)) + a_w * w
        else:
            xhat = x + a_w * w
            k1 = f32(k["c_x"]) * xhat + f32(k["c_m"]) * m_at(xhat, t)
            xp = xhat + f32(dt) * k1
            t2 = float(ts[i] + dt_t)
            k2c = sde_coef(path, model, form, norm, t2)
            k2 = f32(k2c["c_x"]) * xp + f32(k2c["c_m"]) * m_at(xp, t2)
            x = xhat + f32(0.5 * dt) * (k1 + k2)
        xs.append(x)
    if last_step is not None:
        a_x, a_m = last_coef(sde_coef(path, model, form, norm, t1), last_step, lss)
        x = f32(a_x) * x + f32(a_m) * m_at(x, t1)
    xs.append(x)
    return xs, seen


# ---------------------------------------------------------------------------------------------------------------- the likelihood solve
def logp_interval(model: str, eps: float) -> tuple[float, float]:
    return (0.0, 1.0) if model == "velocity" else (eps, 1 - eps)


def n_evaluations(method: str, steps: int) -> int:
    return steps * (2 if method.lower() == "heun" else 1)


def prior_logp(z: torch.Tensor) -> torch.Tensor:
    n = z[0].numel()
    return z.new_tensor(-n / 2.0) * math.log(2 * math.pi) - z.pow(2).flatten(1).sum(1) / 2.0


def logp_eval_times(model: str, eps: float, method: str, steps: int) -> list[float]:
    s = torch.linspace(*logp_interval(model, eps), steps + 1)
    out = []
    for i in range(steps):
        out.append(float(1 - s[i]))
        if method.lower() == "heun":
            out.append(float(1 - s[i + 1]))
    return out


def logp_ref(x, model_fn, path, model, eps, method, steps, probes, zero_model=False):
    """Returns (logp, x_end, list of logp_grad, list of the (n,) t vectors the model saw, list of per-row sum |dm/dx^T eps| (the scale of
    a divergence term), list of the float64 a(t) e of every evaluation)."""
    method = method.lower()
    assert method in ("euler", "heun") and probes.shape[0] == n_evaluations(method, steps)
    s = torch.linspace(*logp_interval(model, eps), steps + 1)
    dl = torch.zeros(x.shape[0], dtype=x.dtype)
    e = x[0].numel()
    dims = tuple(range(1, x.dim()))
    lgs, seen, scales, aes = [], [], [], []

    def ev(xc, sv):
        t = float(1 - sv)
        tv = torch.full((xc.shape[0],), t, dtype=torch.float32)
        k = path_coef(path, model, t)
        a32, b32, ae = f32(k["a"]), f32(k["b"]), f32(k["a"] * e)
        with torch.enable_grad():
            xr = xc.detach().requires_grad_(True)
            m = model_fn(xr, tv)
            if zero_model:
                m = m * 0.0
            grad = torch.autograd.grad(torch.sum(m * probes[len(lgs)]), xr)[0]
        dot = torch.sum(grad * probes[len(lgs)], dim=dims)
        scales.append(grad.abs().sum(dim=dims))
        lg = ae + b32 * dot
        lgs.append(lg)
        seen.append(tv)
        aes.append(float(k["a"]) * e)
        return -(a32 * xc + b32 * m.detach()), lg

    x = x.detach()
    for i in range(steps):
        h = float(s[i + 1] - s[i])
        k1x, k1l = ev(x, s[i])
        if method == "euler":
            x, dl = x + h * k1x, dl + h * k1l
        else:
            k2x, k2l = ev(x + h * k1x, s[i + 1])
            x, dl = x + (0.5 * h) * (k1x + k2x), dl + (0.5 * h) * (k1l + k2l)
    return prior_logp(x) - dl, x, lgs, seen, scales, aes


# ---------------------------------------------------------------------------------------------------------------- fixtures
def make_transport(path: str, prediction: str, eps: float, enabled: bool = True):
    from scldm_amd.transport import create_transport
    return create_transport(path, prediction, None, None, eps if prediction != "velocity" else None, samplers_enabled=enabled)


def _load(name: str, table: dict, first: str):
    import json

    from conftest import golden_json, load_golden
    from oracle.dit import DiTConfig
    from oracle.weights import make_state_dict
    dit_name, *settings = table[name]
    f = load_golden(name)
    assert json.loads(str(f["settings_json"])) == [dit_name, *settings], "tests/transport_solvers_ref.py: the case table and the stored fixture disagree"
    g = load_golden(dit_name)
    kw = golden_json(g, "kwargs_json")
    sd = make_state_dict({k: tuple(v) for k, v in golden_json(g, "shapes_json").items()}, int(g["seed"]))
    cfg = DiTConfig(n_embed=kw["n_embed"], n_embed_input=kw["n_embed_input"], n_layer=kw["n_layer"], n_head=kw["n_head"],
                    seq_len=kw["seq_len"], multiple_of=kw["multiple_of"], layernorm_eps=kw["layernorm_eps"],
                    class_vocab_sizes=kw["class_vocab_sizes"], condition_strategy=kw["condition_strategy"])
    z2 = torch.from_numpy(np.concatenate([f[first], f[first]]))
    cond2 = {k: torch.from_numpy(np.concatenate([f[f"label_{k}"]] * 2)) for k in cfg.class_vocab_sizes}
    return f, sd, cfg, z2, cond2, golden_json(f, "scales_json"), tuple(settings)


def load_sde_case(name: str):
    """(fixture arrays, state dict, oracle config, z (2B,S,C), doubled labels, scales, (path, prediction, method, form, norm, last step,
    last step size, grid points))."""
    return _load(name, SDE_CASES, "z0")


def load_logp_case(name: str):
    """... (path, prediction, method, steps, sample_eps))."""
    return _load(name, LOGP_CASES, "x")


def sde_eps(prediction: str) -> float:
    return 0.0 if prediction == "velocity" else SDE_EPS


def oracle_sde_solve(name: str):
    """The SDE restatement over the oracle DiT on a fixture's inputs and recorded noise: a zero-argument callable returning the
    (num_steps, 2B, S, C) stack (what tests/precision_class.py runs under its operand-rounding modes)."""
    from oracle.dit import dit_forward_with_cfg
    f, sd, cfg, z2, cond2, scales, (path, pred, method, form, norm, last, lss, steps) = load_sde_case(name)
    model = lambda x, t: dit_forward_with_cfg(sd, cfg, x, t, cond2, scales)
    return lambda: torch.stack(sample_sde_ref(z2, model, path, pred, sde_eps(pred), steps, method, form, norm, last, lss, torch.from_numpy(f["noise"]))[0])

"""What the transport-path tests and their fixture generator share: the case tables, the plain callable that stands in for a model, and
float64 restatements of the path arithmetic (src/scldm/transport/path.py:24-151,190-208; transport.py:110-183 of the reference).

    alpha, alpha', sigma, sigma', alpha'/alpha:   Linear  t, 1, 1 - t, -1, 1 / t
                                                  GVP     sin(pi t/2), pi/2 cos(pi t/2), cos(pi t/2), -pi/2 sin(pi t/2), pi / (2 tan(pi t/2))
    Dv = (alpha'/alpha) sigma^2 - sigma sigma'
    loss row   w mean((c m - tgt)^2), (c, tgt) = (1, ut) | (1, x0) | (sigma, -x0);  w = 1 | (Dv/sigma)^2 | Dv/sigma^2
    drift      a x + b m, (a, b) = (0, 1) | (alpha'/alpha, Dv) score | (alpha'/alpha, -Dv/sigma) noise
"""
from __future__ import annotations

import numpy as np
import torch

# (path_type, prediction, loss_weight): Linear x {noise, score} x 3 weights, GVP velocity, GVP x {noise, score} x 3 weights
CASES = ([("Linear", p, w) for p in ("noise", "score") for w in (None, "velocity", "likelihood")] + [("GVP", "velocity", None)]
         + [("GVP", p, w) for p in ("noise", "score") for w in (None, "velocity", "likelihood")])
assert len(CASES) == 13
# one weight per (path, prediction): the cases whose parameter gradients are stored
GRAD_CASES = [("Linear", "noise", "velocity"), ("Linear", "score", "likelihood"), ("GVP", "velocity", None), ("GVP", "noise", "likelihood"),
              ("GVP", "score", "velocity")]
DRIFT_CASES = [("Linear", "noise"), ("Linear", "score"), ("GVP", "velocity"), ("GVP", "noise"), ("GVP", "score")]
COEF_T = [1e-3, 0.05, 0.25, 0.5, 0.75, 0.95, 0.999]      # both ends of the default interval [1e-3, 1 - 1e-3]
KERNEL_N = (5, 9)                                         # rows of the kernel fixtures: a partial and a second group of the 8-row loss kernel
ROW_SHAPE = (16, 16)
T_RANGE = (0.05, 0.95)                                    # the training draws of every fixture lie here
# solver fixtures: name -> (dit case of make_golden, B, cfg scales (None: 1.5 - 0.4 i per class; a float: that value for every class),
#                           path_type, prediction, method, num_steps)
SOLVER_CASES = {
    "me2_euler9_linear_noise": ("dit_me2_256", 3, None, "Linear", "noise", "euler", 9),
    "me2_heun5_gvp_score": ("dit_me2_256", 3, None, "GVP", "score", "heun", 5),
    "base_direct_euler9_gvp_noise": ("dit_base", 2, 1.0, "GVP", "noise", "euler", 9),
    "base_direct_heun5_linear_score": ("dit_base", 2, 1.0, "Linear", "score", "heun", 5),
}


def case_key(path_type, prediction, loss_weight=None) -> str:
    return f"{path_type}_{prediction}_{loss_weight or 'none'}"


def toy_model(xt: torch.Tensor, t: torch.Tensor, **_) -> torch.Tensor:
    """A plain callable standing in for the model: smooth in both arguments, the size of a unit normal."""
    te = t.view(-1, *([1] * (xt.dim() - 1)))
    return 0.6 * xt - 0.25 * torch.tanh(xt) * te + 0.1 * te


def coef(path_type: str, prediction: str, loss_weight, t) -> dict:
    """The coefficient table above in float64 numpy at t (array or scalar)."""
    t = np.asarray(t, dtype=np.float64)
    if path_type == "GVP":
        al, dal, sg, dsg = np.sin(t * np.pi / 2), np.pi / 2 * np.cos(t * np.pi / 2), np.cos(t * np.pi / 2), -np.pi / 2 * np.sin(t * np.pi / 2)
        with np.errstate(divide="ignore"):
            ratio = np.pi / (2 * np.tan(t * np.pi / 2))
    else:
        al, dal, sg, dsg = t, np.ones_like(t), 1 - t, -np.ones_like(t)
        with np.errstate(divide="ignore"):
            ratio = 1 / t
    dv = ratio * sg ** 2 - sg * dsg
    one, zero = np.ones_like(t), np.zeros_like(t)
    if prediction == "velocity":
        a, b, c, w = zero, one, one, one
    else:
        a = ratio
        b = dv if prediction == "score" else -dv / sg
        c = sg if prediction == "score" else one
        w = {"velocity": (dv / sg) ** 2, "likelihood": dv / sg ** 2}.get(loss_weight, one)
    return dict(alpha=al, d_alpha=dal, sigma=sg, d_sigma=dsg, ratio=ratio, dv=dv, a=a, b=b, c=c, w=w)


def plan_loss_ref(path_type, prediction, loss_weight, x1, x0, t, m, gloss):
    """float64: xt, tgt, rowc (n, 2), loss (n), d m for the upstream gradient gloss (n); x1, x0, m (n, e), t (n)."""
    x1, x0, m, t, gloss = (np.asarray(v, dtype=np.float64) for v in (x1, x0, m, t, gloss))
    k = {key: v[:, None] for key, v in coef(path_type, prediction, loss_weight, t).items()}
    xt = k["alpha"] * x1 + k["sigma"] * x0
    tgt = k["d_alpha"] * x1 + k["d_sigma"] * x0 if prediction == "velocity" else (x0 if prediction == "noise" else -x0)
    d = k["c"] * m - tgt
    loss = k["w"][:, 0] * (d ** 2).mean(1)
    dm = gloss[:, None] * k["w"] * (2.0 / m.shape[1]) * k["c"] * d
    return xt, tgt, np.concatenate([k["c"], k["w"]], 1), loss, dm


def grad_digest(g, sample: int = 64) -> np.ndarray:
    """[sum, l2, `sample` strided entries] of a gradient tensor (the digest of tests/golden/make_golden.py)."""
    f = np.asarray(g.detach().cpu().numpy() if hasattr(g, "detach") else g).reshape(-1).astype(np.float64)
    stride = max(1, f.size // sample)
    smp = f[::stride][:sample]
    smp = np.pad(smp, (0, sample - smp.size))
    return np.concatenate([[f.sum(), np.sqrt((f * f).sum())], smp]).astype(np.float64)

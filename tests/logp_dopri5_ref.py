"""Float64 restatement of the reference's default likelihood solve, `Sampler.sample_ode_likelihood(sampling_method="dopri5")`.  TEST
INFRASTRUCTURE ONLY (a helper module the dopri5 log-likelihood tests import).

The reference hands torchdiffeq the tuple state (x, delta_logp), which it flattens: one adaptive Dormand-Prince solve over the packed
state (n, e + 1) with ONE mixed rms error norm and one atol / rtol.  Here that solve is the float64 oracle's
(oracle/transport.py: sample_ode_dopri5) and the drift is tests/logp_ref.py's `likelihood_drift` - (-v, logp_grad) at model time
t = fp32(1 - s) - over any differentiable callable (x, t (n,)) -> v.  The probes are GIVEN: one tensor held for the whole solve, or a
callable evaluation index -> probe (the index is the running count in execution order: f0 is 0, the initial-step evaluation 1, then
six per attempted step, rejected steps included)."""
from __future__ import annotations

import numpy as np
import torch

import logp_ref


def logp_dopri5_ref(x: torch.Tensor, model_fn, probes, atol: float = 1e-6, rtol: float = 1e-3, num_steps: int = 2):
    """Returns (logp (n,), x_end, stats) in float64; stats = {"accepted": [(s0, h), ...], "rejected": [...], "evaluations": count}.
    `num_steps` is the save-point count (only the last point is used; the steps do not depend on it)."""
    from oracle.transport import sample_ode_dopri5
    x = x.detach().double()
    n, shape = x.shape[0], tuple(x.shape)
    e = x[0].numel()
    count = 0

    def packed(y, sv):
        nonlocal count
        eps = probes(count) if callable(probes) else probes
        count += 1
        t = float(np.float32(1) - np.float32(float(sv[0])))        # the model's time, formed in fp32 as the sampler forms it
        k, lg, _, _ = logp_ref.likelihood_drift(y[:, :e].reshape(shape), model_fn, t, eps.to(y.dtype))
        return torch.cat([k.reshape(n, e), lg.reshape(n, 1).to(k.dtype)], dim=1)

    y0 = torch.cat([x.reshape(n, e), torch.zeros(n, 1, dtype=torch.float64)], dim=1)
    traj, stats = sample_ode_dopri5(y0, packed, num_steps, atol, rtol, return_stats=True)
    y = traj[-1]
    x_end, dl = y[:, :e].reshape(shape), y[:, e]
    return logp_ref.prior_logp(x_end) - dl, x_end, stats

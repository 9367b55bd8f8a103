"""CPU tests of the log-likelihood solve: the restatement of tests/logp_ref.py against the reference's own recorded runs
(tests/golden/logp_*.npz, written by tests/golden/make_golden_logp.py), `Transport.prior_logp` and the generic
`Sampler.sample_ode_likelihood` of scldm_amd.transport against closed forms, the fixtures and a float64 restatement of the adaptive
driver, and the C ABI's new declarations.  The fused on-device solve is held to the same fixtures in tests/test_gpu_logp.py."""
import math
import os
import re

import numpy as np
import pytest
import torch

import logp_ref
from conftest import ROOT, load_golden, max_abs_rel
from scldm_amd.transport import Sampler, create_transport

TOL = 1e-5       # restatement vs the reference's own fp32 autograd, scale-relative
_SOLVES = {}


def _solve(name):
    """The restatement over the oracle DiT on a fixture's inputs and recorded probes, once per session."""
    if name not in _SOLVES:
        from oracle.dit import dit_forward_with_cfg
        f, sd, cfg, z2, cond2, scales, (method, steps) = logp_ref.load_case(name)
        model = lambda x, t: dit_forward_with_cfg(sd, cfg, x, t, cond2, scales)
        n_thr = torch.get_num_threads()
        torch.set_num_threads(min(16, n_thr))
        try:
            _SOLVES[name] = (*logp_ref.logp_ref(z2, model, method, steps, torch.from_numpy(f["probes"])), f)
        finally:
            torch.set_num_threads(n_thr)
    return _SOLVES[name]


def _sampler():
    return Sampler(create_transport("Linear", "velocity", "velocity", 1e-5, 1e-5))


@pytest.mark.parametrize("name", list(logp_ref.CASES))
def test_restatement_sees_the_references_times_exactly(name):
    logp, x_end, lgs, seen, scales, f = _solve(name)
    assert np.array_equal(torch.stack(seen).numpy(), f["t_seen"])
    method, steps = logp_ref.CASES[name][1:]
    assert [float(t[0]) for t in seen] == logp_ref.eval_times(method, steps)
    assert set(np.unique(f["probes"])) == {-1.0, 1.0}


@pytest.mark.parametrize("name", list(logp_ref.CASES))
def test_restatement_reproduces_the_references_solve(name):
    logp, x_end, lgs, seen, scales, f = _solve(name)
    assert len(lgs) == f["logp_grad"].shape[0] and np.isfinite(f["logp"]).all()
    for e, (lg, sc) in enumerate(zip(lgs, scales)):     # a logp_grad is a signed sum: its scale is sum |grad| of the row
        err = float(((lg.double() - torch.from_numpy(f["logp_grad"][e]).double()).abs() / sc.double()).max())
        print(f"[parity] {name} evaluation {e}: logp_grad restatement vs reference {err:.3e} of sum|dx| (tol {TOL:g})")
        assert err < TOL, (name, e, err)
    e_l, e_x = max_abs_rel(logp, f["logp"]), max_abs_rel(x_end, f["x_end"])
    print(f"[parity] {name}: logp {e_l:.3e}, x_end {e_x:.3e} (tol {TOL:g})")
    assert e_l < TOL and e_x < TOL, (name, e_l, e_x)


def test_toy_fixture_restatement_and_generic_sampler_from_the_seed_alone():
    """`Sampler.sample_ode_likelihood` on a plain callable, CPU tensors: with the fixture's `torch.manual_seed` and no other input it
    reproduces the reference's runs - it consumes the host generator in the reference's order (one `randint` of the state's shape per
    evaluation).  The runs share one generator stream, in TOY_RUNS order, as they did when the fixture was written."""
    f = load_golden("logp_toy")
    x0 = torch.from_numpy(f["x0"])
    torch.manual_seed(logp_ref.TOY_SEED)
    for i, (method, steps) in enumerate(logp_ref.TOY_RUNS):
        fn = _sampler().sample_ode_likelihood(sampling_method=method, num_steps=steps + 1)
        logp, x_end = fn(x0, logp_ref.toy_model)
        assert np.array_equal(torch.stack(fn.last_trace["t"]).numpy(), f[f"t_seen_{i}"])
        r_logp, r_x, r_lg, r_seen, _ = logp_ref.logp_ref(x0, logp_ref.toy_model, method, steps, torch.from_numpy(f[f"probes_{i}"]))
        assert np.array_equal(torch.stack(r_seen).numpy(), f[f"t_seen_{i}"])
        for got_l, got_x, got_g in ((logp, x_end, fn.last_trace["logp_grad"]), (r_logp, r_x, r_lg)):
            assert max_abs_rel(got_l, f[f"logp_{i}"]) < TOL and max_abs_rel(got_x, f[f"x_end_{i}"]) < TOL, i
            assert max_abs_rel(torch.stack(got_g), f[f"logp_grad_{i}"]) < TOL, i


def test_injected_probe_replaces_the_host_generator():
    f = load_golden("logp_toy")
    x0 = torch.from_numpy(f["x0"])
    probes = iter(torch.from_numpy(f["probes_1"]))
    state = torch.random.get_rng_state()
    fn = _sampler().sample_ode_likelihood(sampling_method=logp_ref.TOY_RUNS[1][0], num_steps=logp_ref.TOY_RUNS[1][1] + 1)
    logp, x_end = fn(x0, logp_ref.toy_model, _probe=lambda x: next(probes))
    assert torch.equal(torch.random.get_rng_state(), state)      # nothing drawn
    assert max_abs_rel(logp, f["logp_1"]) < TOL and max_abs_rel(x_end, f["x_end_1"]) < TOL


@pytest.mark.parametrize("method", ["euler", "heun"])
def test_closed_form_linear_field(method):
    """v = a x: the Jacobian is a I and eps_i^2 = 1, so the Hutchinson term is exactly a N for EVERY probe.  Euler over n steps of
    size h: x_end = x (1 - a h)^n, delta_logp = n h a N; Heun's step factor is 1 - a h + (a h)^2 / 2.  float64."""
    a, n, shape = 0.3, 7, (3, 2, 5)
    N, h = shape[1] * shape[2], 1.0 / n
    x = torch.from_numpy(np.random.default_rng(5).standard_normal(shape))
    tr = create_transport()
    fn = Sampler(tr).sample_ode_likelihood(sampling_method=method, num_steps=n + 1)
    logp, x_end = fn(x, lambda xx, t: a * xx)
    factor = (1 - a * h) if method == "euler" else (1 - a * h + (a * h) ** 2 / 2)
    want_x = x * factor ** n
    want_prior = -N / 2 * math.log(2 * math.pi) - (want_x ** 2).sum(dim=(1, 2)) / 2
    assert logp.dtype == torch.float64 and x_end.dtype == torch.float64
    assert float((x_end - want_x).abs().max()) < 1e-6
    assert float((tr.prior_logp(want_x) - want_prior).abs().max()) < 1e-6
    assert float((logp - (want_prior - n * h * a * N)).abs().max()) < 1e-6
    for lg in fn.last_trace["logp_grad"]:
        assert float((lg - a * N).abs().max()) < 1e-6


def test_prior_logp_is_the_standard_normal_log_density():
    z = torch.from_numpy(np.random.default_rng(6).standard_normal((4, 3, 5)))
    want = torch.distributions.Normal(0.0, 1.0).log_prob(z).sum(dim=(1, 2))
    tr = create_transport()
    assert float((tr.prior_logp(z) - want).abs().max()) < 1e-10
    assert max_abs_rel(tr.prior_logp(z.float()), want) < 1e-6 and tr.prior_logp(z.float()).dtype == torch.float32
    assert max_abs_rel(logp_ref.prior_logp(z), want) < 1e-12


def test_dopri5_on_the_packed_state_against_a_float64_restatement():
    """`sample_ode_likelihood("dopri5")` = the Dormand-Prince driver of sample_ode on the packed state (n, numel + 1) with one mixed rms
    norm: against oracle.transport.sample_ode_dopri5 (the float64 restatement of that driver) run on the same packed field with the
    same probe per evaluation index."""
    from oracle.transport import sample_ode_dopri5
    x0 = torch.from_numpy(np.random.default_rng(7).standard_normal(logp_ref.TOY_SHAPE))
    n, e = x0.shape
    g = torch.Generator().manual_seed(11)
    probes = [(torch.randint(2, x0.shape, generator=g) * 2 - 1).double() for _ in range(400)]
    used = iter(probes)
    fn = _sampler().sample_ode_likelihood(num_steps=5)       # the reference's defaults: dopri5, atol 1e-6, rtol 1e-3
    logp, x_end = fn(x0, logp_ref.toy_model, _probe=lambda x: next(used))
    n_used = len(fn.last_trace["t"])
    k = 0

    def packed(y, tv):
        nonlocal k
        dxv, lg, _, _ = logp_ref.likelihood_drift(y[:, :-1], logp_ref.toy_model, float(1 - tv[0]), probes[k])
        k += 1
        return torch.cat([dxv, lg.reshape(n, 1)], dim=1)

    y = sample_ode_dopri5(torch.cat([x0, torch.zeros(n, 1, dtype=torch.float64)], dim=1), packed, num_steps=5, atol=1e-6, rtol=1e-3)[-1]
    assert k == n_used and 7 <= k < 400
    assert float((x_end - y[:, :-1]).abs().max()) < 1e-9
    assert float((logp - (logp_ref.prior_logp(y[:, :-1]) - y[:, -1])).abs().max()) < 1e-9


def test_rejected_arguments():
    s = _sampler()
    with pytest.raises(NotImplementedError):
        s.sample_ode_likelihood(sampling_method="rk4")
    with pytest.raises(ValueError):
        s.sample_ode_likelihood(sampling_method="euler", num_steps=1)
    with pytest.raises(NotImplementedError):
        s.sample_ode(reverse=True)      # unchanged: the likelihood solve returns the inversion


def test_abi_declares_the_likelihood_entry_points():
    from scldm_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "scldm_hip.h")).read()
    declared = set(re.findall(r"\b(scldm_[a-z_0-9]+)\s*\(", hdr))
    L = _lib.lib()
    for name in ("scldm_dit_train_backward_dx", "scldm_dit_train_workspace_bytes_dx_for", "scldm_logp_ode", "scldm_logp_probe",
                 "scldm_logp_workspace_bytes"):
        assert name in declared and name in _lib.EXPORTS and hasattr(L, name), name
    # argument validation needs no GPU: nothing is launched for a rejected call
    assert L.scldm_logp_probe(None, 1, 16, 0, 0, 0, 0, 1, None) == -1 and b"aligned" in L.scldm_last_error()
    assert L.scldm_logp_workspace_bytes(None, 3, 1, 0) == 0 and L.scldm_dit_train_workspace_bytes_dx_for(None, 3, 0) == 0

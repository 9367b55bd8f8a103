"""CPU tests of the SDE sampler: the restatement of tests/sde_ref.py against the reference's own recorded runs
(tests/golden/sde_*.npz, written by tests/golden/make_golden_sde.py), and the generic `Sampler.sample_sde` of scldm_amd.transport
against both.  The fused on-device solve is held to the same fixtures in tests/test_gpu_sde.py."""
import numpy as np
import pytest
import torch

import sde_ref
from conftest import load_golden, max_abs_rel
from scldm_amd.transport import Sampler, create_transport

TOL = 2e-5       # oracle-vs-reference, as test_transport_face_and_training_losses_cpu
_SOLVES = {}


def _solve(name):
    """The restatement over the oracle DiT on a fixture's inputs, once per session: (states, t vectors, fixture)."""
    if name not in _SOLVES:
        from oracle.dit import dit_forward_with_cfg
        f, sd, cfg, z2, cond2, scales, (method, form, norm, last, lss, steps) = sde_ref.load_case(name)
        model = lambda x, t: dit_forward_with_cfg(sd, cfg, x, t, cond2, scales)
        n_thr = torch.get_num_threads()
        torch.set_num_threads(min(16, n_thr))
        try:
            xs, seen = sde_ref.sample_sde_ref(z2, model, steps, method, form, norm, last, lss, torch.from_numpy(f["noise"]))
        finally:
            torch.set_num_threads(n_thr)
        _SOLVES[name] = (torch.stack(xs), torch.stack(seen), f)
    return _SOLVES[name]


def _sampler():
    return Sampler(create_transport("Linear", "velocity", "velocity", 1e-5, 1e-5))


@pytest.mark.parametrize("name", list(sde_ref.CASES))
def test_restatement_sees_the_references_times_exactly(name):
    xs, seen, f = _solve(name)
    assert seen.shape == f["t_seen"].shape
    assert np.array_equal(seen.numpy(), f["t_seen"])


@pytest.mark.parametrize("name", list(sde_ref.CASES))
def test_restatement_reproduces_the_references_trajectory(name):
    xs, seen, f = _solve(name)
    steps = sde_ref.CASES[name][-1]
    assert xs.shape == f["traj"].shape and xs.shape[0] == steps and np.isfinite(f["traj"]).all()
    for i in range(steps):      # every returned state, each against its own scale
        e = max_abs_rel(xs[i], f["traj"][i])
        print(f"[parity] {name} state {i}: restatement vs reference {e:.3e} (tol {TOL:g})")
        assert e < TOL, (name, i, e)


def test_toy_fixture_restatement_and_generic_sampler_from_the_seed_alone():
    """`Sampler.sample_sde` on a plain callable, CPU tensors: with the fixture's `torch.manual_seed` and no other input it reproduces the
    reference's lists - it consumes the host generator in the reference's order (one `randn` of the state's shape per step).  The runs
    share one generator stream, in TOY_RUNS order, as they did when the fixture was written."""
    f = load_golden("sde_toy")
    x0 = torch.from_numpy(f["x0"])
    torch.manual_seed(sde_ref.TOY_SEED)
    for i, (method, form, norm, last, lss, steps) in enumerate(sde_ref.TOY_RUNS):
        fn = _sampler().sample_sde(sampling_method=method, diffusion_form=form, diffusion_norm=norm, last_step=last, last_step_size=lss,
                                   num_steps=steps)
        xs = fn(x0, sde_ref.toy_model)
        assert isinstance(xs, list) and len(xs) == steps
        ref, seen = sde_ref.sample_sde_ref(x0, sde_ref.toy_model, steps, method, form, norm, last, lss, torch.from_numpy(f[f"noise_{i}"]))
        assert np.array_equal(torch.stack(seen).numpy(), f[f"t_seen_{i}"])
        for k in range(steps):
            assert max_abs_rel(xs[k], f[f"traj_{i}"][k]) < TOL, (i, k)
            assert max_abs_rel(ref[k], f[f"traj_{i}"][k]) < TOL, (i, k)


def test_model_sees_a_stride0_t_and_kwargs():
    seen = []

    def model(x, t, scale=None):
        seen.append((t, scale))
        return -x

    fn = _sampler().sample_sde(sampling_method="Heun", diffusion_form="sigma", last_step="Euler", num_steps=3)
    fn(torch.ones(5, 2), model, scale=2.0)
    assert len(seen) == 5 and all(t.shape == (5,) and t.stride(0) == 0 and t.dtype == torch.float32 and s == 2.0 for t, s in seen)


@pytest.mark.parametrize("method", ["Euler", "Heun"])
def test_zero_noise_known_answer(method):
    """diffusion_norm = 0 removes score and noise: v = -x leaves the deterministic steps x <- (1 - dt) x (Euler) or
    x <- (1 - dt + dt^2 / 2) x (Heun) and the Euler last step x <- (1 - last_step_size) x."""
    x0 = torch.tensor([[1.0, -2.0, 0.5]])
    steps, lss = 5, 0.04
    fn = _sampler().sample_sde(sampling_method=method, diffusion_form="sigma", diffusion_norm=0.0, last_step="Euler", last_step_size=lss,
                               num_steps=steps)
    torch.manual_seed(0)
    xs = fn(x0, lambda x, t: -x)
    dt = 0.96 / 4
    g = 1 - dt if method == "Euler" else 1 - dt + dt * dt / 2
    want = [x0.double() * g ** (k + 1) for k in range(steps - 1)]
    want.append(want[-1] * (1 - lss))
    assert len(xs) == steps
    for a, b in zip(xs, want):
        assert torch.allclose(a.double(), b, rtol=2e-6, atol=0)
    ref, _ = sde_ref.sample_sde_ref(x0, lambda x, t: -x, steps, method, "sigma", 0.0, "Euler", lss, torch.zeros(steps - 1, 1, 3))
    for a, b in zip(ref, want):
        assert torch.allclose(a.double(), b, rtol=2e-6, atol=0)


def test_time_sequence_and_list_length():
    seen = []
    fn = _sampler().sample_sde(sampling_method="Euler", diffusion_form="sigma", last_step="Mean", last_step_size=0.04, num_steps=5)
    xs = fn(torch.zeros(2, 3), lambda x, t: (seen.append(float(t[0])), x)[1])
    assert len(xs) == 5
    assert np.allclose(seen, [0.0, 0.24, 0.48, 0.72, 0.96], rtol=0, atol=1e-7)
    assert seen == sde_ref.eval_times(5, "Euler", "Mean", 0.04)
    seen.clear()
    xs = _sampler().sample_sde(sampling_method="Euler", diffusion_form="sigma", last_step=None, num_steps=4)(torch.zeros(2, 3), lambda x, t: (seen.append(float(t[0])), x)[1])
    assert len(xs) == 4 and len(seen) == 3 and xs[-1] is xs[-2]       # no last evaluation; the reference appends the unchanged state
    assert seen == sde_ref.eval_times(4, "Euler", None, 0.04)


def test_error_paths():
    s = _sampler()
    with pytest.raises(ValueError, match="sigma"):       # the reference's default form; the message names the working choices
        s.sample_sde()
    with pytest.raises(ValueError, match="Mean"):
        s.sample_sde(sampling_method="Heun", diffusion_form="sigma", last_step=None)
    with pytest.raises(NotImplementedError):
        s.sample_sde(diffusion_form="quadratic")
    with pytest.raises(NotImplementedError):
        s.sample_sde(sampling_method="dopri5", diffusion_form="sigma")
    with pytest.raises(NotImplementedError):
        s.sample_sde(diffusion_form="sigma", last_step="Median")
    with pytest.raises(ValueError):
        s.sample_sde(diffusion_form="sigma", num_steps=1)
    with pytest.raises(ValueError):
        s.sample_sde(diffusion_form="sigma", last_step_size=1.0)
    assert s.transport.check_interval(0, 0, sde=True, last_step_size=0.04) == (0, 1)     # unchanged for its existing callers


@pytest.mark.parametrize("method,last", [("Euler", "Mean"), ("Heun", "Tweedie"), ("Euler", None)])
def test_constant_form_matches_the_restatement(method, last):
    """diffusion_form="constant" has NO reference fixture: the reference raises TypeError for it (`th.sqrt` of a Python float).  It is
    implemented as the mathematics (D = norm) and held to the CPU restatement only."""
    torch.manual_seed(3)
    x0 = torch.randn(4, 6)
    steps = 5
    noise = torch.randn(steps - 1, 4, 6)
    draws = iter(noise)
    fn = _sampler().sample_sde(sampling_method=method, diffusion_form="constant", diffusion_norm=0.3, last_step=last, num_steps=steps)
    xs = fn(x0, sde_ref.toy_model, _draw=lambda x: next(draws))
    ref, _ = sde_ref.sample_sde_ref(x0, sde_ref.toy_model, steps, method, "constant", 0.3, last, 0.04, noise)
    assert len(xs) == steps and all(torch.isfinite(x).all() for x in xs)
    for a, b in zip(xs, ref):
        assert max_abs_rel(a, b) < TOL


def test_transport_exposes_score_and_diffusion():
    tr = create_transport()
    x, t = torch.randn(3, 4), torch.tensor([0.1, 0.5, 0.9])
    v = torch.randn(3, 4)
    s = tr.get_score()(x, t, lambda x_, t_: v)
    assert torch.allclose(s, (t[:, None] * v - x) / (1 - t[:, None]), rtol=1e-5, atol=1e-6)
    D = tr.path_sampler.compute_diffusion(x, t, form="decreasing", norm=0.5)
    assert torch.allclose(D, 0.25 * (0.5 * torch.cos(torch.pi * t[:, None]) + 1) ** 2)
    with pytest.raises(NotImplementedError):
        tr.path_sampler.compute_diffusion(x, t, form="SBDM")

"""CPU tests of the SDE sampler and the likelihood under the non-default transports (Linear | GVP x velocity | noise | score, opt-in with
`create_transport(..., samplers_enabled=True)`): the restatement of tests/transport_solvers_ref.py and the generic `Sampler` against the
reference's own recorded runs (tests/golden/sdet_*.npz, logpt_*.npz, written by tests/golden/make_golden_sde_logp_transport.py), the
host-only scalar entries (scldm_sde_coef_at / scldm_sde_last_coef_at) against the reference's closures on float64 tensors, the refusal
rule, and what the switch leaves alone.  The fused on-device solves are held to the same fixtures in tests/test_gpu_sde_logp_transport.py."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import transport_solvers_ref as R
from conftest import load_golden, max_abs_rel
from scldm_amd import _lib
from scldm_amd.transport import Sampler, create_transport

TOL = 2e-5       # oracle-vs-reference, as tests/test_sde_cpu.py and tests/test_logp_cpu.py
_PATH = {"Linear": 0, "GVP": 1}
_MODEL = {"velocity": 0, "noise": 1, "score": 2}


def _tr(path, pred, eps=0.05):
    return _lib.TransportC(path=_PATH[path], model=_MODEL[pred], weight=0, train_eps=0.0, sample_eps=0.0 if pred == "velocity" else eps)


# ---------------------------------------------------------------------------------------------------------------- toy fixtures
def test_generic_sde_sampler_reproduces_the_toy_fixture_from_the_seed_alone():
    """`Sampler.sample_sde` under an enabled non-default transport, plain callable, CPU tensors: with the fixture's `torch.manual_seed` and
    no other input it reproduces the reference's lists - the host generator is consumed in the reference's order.  The runs share one
    generator stream, in TOY_SDE_RUNS order, as they did when the fixture was written; the restatement gets the recorded draws."""
    f = load_golden("sdet_toy")
    x0 = torch.from_numpy(f["x0"])
    torch.manual_seed(R.TOY_SEED)
    for i, (path, pred, eps, method, form, norm, last, lss, steps) in enumerate(R.TOY_SDE_RUNS):
        fn = Sampler(R.make_transport(path, pred, eps)).sample_sde(sampling_method=method, diffusion_form=form, diffusion_norm=norm,
                                                                   last_step=last, last_step_size=lss, num_steps=steps)
        seen = []
        xs = fn(x0, lambda x, t: (seen.append(t.clone()), R.toy_model(x, t))[1])
        assert isinstance(xs, list) and len(xs) == steps
        assert np.array_equal(torch.stack(seen).numpy(), f[f"t_seen_{i}"])
        ref, rseen = R.sample_sde_ref(x0, R.toy_model, path, pred, eps, steps, method, form, norm, last, lss, torch.from_numpy(f[f"noise_{i}"]))
        assert np.array_equal(torch.stack(rseen).numpy(), f[f"t_seen_{i}"])
        for k in range(steps):
            assert max_abs_rel(xs[k], f[f"traj_{i}"][k]) < TOL, (i, k)
            assert max_abs_rel(ref[k], f[f"traj_{i}"][k]) < TOL, (i, k)


def test_generic_likelihood_sampler_reproduces_the_toy_fixture_from_the_seed_alone():
    f = load_golden("logpt_toy")
    x0 = torch.from_numpy(f["x0"])
    torch.manual_seed(R.TOY_SEED + 1)
    for i, (path, pred, eps, method, steps) in enumerate(R.TOY_LOGP_RUNS):
        fn = Sampler(R.make_transport(path, pred, eps)).sample_ode_likelihood(sampling_method=method, num_steps=steps + 1)
        logp, x_end = fn(x0, R.toy_model)
        assert np.array_equal(torch.stack(fn.last_trace["t"]).numpy(), f[f"t_seen_{i}"])
        got_lg = torch.stack(fn.last_trace["logp_grad"])
        rl, rx, rlg, rseen, _, _ = R.logp_ref(x0, R.toy_model, path, pred, eps, method, steps, torch.from_numpy(f[f"probes_{i}"]))
        assert np.array_equal(torch.stack(rseen).numpy(), f[f"t_seen_{i}"])
        for what, a, b in (("logp", logp, rl), ("x_end", x_end, rx), ("logp_grad", got_lg, torch.stack(rlg))):
            assert max_abs_rel(a, f[f"{what}_{i}"]) < TOL, (i, what, "generic")
            assert max_abs_rel(b, f[f"{what}_{i}"]) < TOL, (i, what, "restatement")


def test_dopri5_likelihood_runs_on_the_packed_state_over_the_transports_interval():
    tr = R.make_transport("Linear", "score", 0.05)
    fn = Sampler(tr).sample_ode_likelihood(sampling_method="dopri5", num_steps=3)
    torch.manual_seed(5)
    logp, x_end = fn(torch.randn(4, 6), R.toy_model)
    assert torch.isfinite(logp).all() and torch.isfinite(x_end).all()
    ts = [float(t[0]) for t in fn.last_trace["t"]]
    assert ts[0] == pytest.approx(0.95, abs=1e-6)      # model time starts at 1 - eps (the driver's steps are not clipped to the interval's end)
    assert fn.last_stats["evaluations"] == len(ts)


# ---------------------------------------------------------------------------------------------------------------- DiT fixtures
_SDE, _LOGP = {}, {}


def _capped(fn):
    n_thr = torch.get_num_threads()
    torch.set_num_threads(min(16, n_thr))
    try:
        return fn()
    finally:
        torch.set_num_threads(n_thr)


def _sde_solve(name):
    if name not in _SDE:
        from oracle.dit import dit_forward_with_cfg
        f, sd, cfg, z2, cond2, scales, (path, pred, method, form, norm, last, lss, steps) = R.load_sde_case(name)
        model = lambda x, t: dit_forward_with_cfg(sd, cfg, x, t, cond2, scales)
        xs, seen = _capped(lambda: R.sample_sde_ref(z2, model, path, pred, R.sde_eps(pred), steps, method, form, norm, last, lss,
                                                    torch.from_numpy(f["noise"])))
        _SDE[name] = (torch.stack(xs), torch.stack(seen), f)
    return _SDE[name]


def _logp_solve(name):
    if name not in _LOGP:
        from oracle.dit import dit_forward_with_cfg
        f, sd, cfg, z2, cond2, scales, (path, pred, method, steps, eps) = R.load_logp_case(name)
        model = lambda x, t: dit_forward_with_cfg(sd, cfg, x, t, cond2, scales)
        _LOGP[name] = (_capped(lambda: R.logp_ref(z2, model, path, pred, eps, method, steps, torch.from_numpy(f["probes"]))), f)
    return _LOGP[name]


@pytest.mark.parametrize("name", list(R.SDE_CASES))
def test_sde_restatement_sees_the_references_times_exactly_and_reproduces_its_states(name):
    xs, seen, f = _sde_solve(name)
    assert seen.shape == f["t_seen"].shape and np.array_equal(seen.numpy(), f["t_seen"])
    path, pred, method, form, norm, last, lss, steps = R.SDE_CASES[name][1:]
    assert [float(t[0]) for t in seen] == R.sde_eval_times(pred, R.sde_eps(pred), steps, method, last, lss)
    assert xs.shape == f["traj"].shape and np.isfinite(f["traj"]).all()
    for i in range(steps):
        e = max_abs_rel(xs[i], f["traj"][i])
        print(f"[parity] {name} state {i}: restatement vs reference {e:.3e} (tol {TOL:g})")
        assert e < TOL, (name, i, e)


@pytest.mark.parametrize("name", list(R.LOGP_CASES))
def test_likelihood_restatement_sees_the_references_times_exactly_and_reproduces_its_run(name):
    (logp, x_end, lgs, seen, scales, aes), f = _logp_solve(name)
    assert np.array_equal(torch.stack(seen).numpy(), f["t_seen"])
    path, pred, method, steps, eps = R.LOGP_CASES[name][1:]
    assert [float(t[0]) for t in seen] == R.logp_eval_times(pred, eps, method, steps)
    lg = torch.stack(lgs)
    div_ref = f["logp_grad"].astype(np.float64) - np.array(aes)[:, None]
    div = lg.double().numpy() - np.array(aes)[:, None]
    d = {"logp": max_abs_rel(logp, f["logp"]), "x_end": max_abs_rel(x_end, f["x_end"]), "logp_grad": max_abs_rel(lg, f["logp_grad"]),
         "divergence term": float(np.abs(div - div_ref).max() / np.abs(div_ref).max())}
    print(f"[parity] {name}: restatement vs reference {d} (tol {TOL:g}; divergence term 1e-4)")
    assert d["logp"] < TOL and d["x_end"] < TOL and d["logp_grad"] < TOL and d["divergence term"] < 1e-4


# ---------------------------------------------------------------------------------------------------------------- the scalar entries
def test_scalar_entries_reproduce_the_references_closures_in_float64():
    """c_x x + c_m m is the reference's sde_drift, D its diffusion_fn, a_x x + a_m m its three last steps; the restatement's (s_x, s_m) and
    (a, b) are its score and probability-flow drift, and agree with the library's scalars: 1e-12 relative, everything evaluated on
    float64 tensors by the reference."""
    f = load_golden("sde_logp_transport_coef")
    L = _lib.lib()
    out4, out2 = (C.c_double * 4)(), (C.c_double * 2)()
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    for i, (path, pred, form, norm, t, lss) in enumerate(R.COEF_CASES):
        x, m = f[f"{i}_x"], f[f"{i}_m"]
        tr = _tr(path, pred)
        assert L.scldm_sde_coef_at(C.byref(tr), _lib.SDE_FORMS[form], norm, t, 0.125, out4) == 0
        D, c_x, c_m, a_w = out4
        assert rel(np.full_like(f[f"{i}_D"], D), f[f"{i}_D"]) < 1e-12, (i, "D")
        assert rel(c_x * x + c_m * m, f[f"{i}_drift"]) < 1e-12, (i, "drift")
        assert a_w == pytest.approx(math.sqrt(2 * D * 0.125), rel=1e-15)
        k = R.sde_coef(path, pred, form, norm, t)
        assert rel(k["s_x"] * x + k["s_m"] * m, f[f"{i}_score"]) < 1e-12 and rel(k["a"] * x + k["b"] * m, f[f"{i}_ode_drift"]) < 1e-12
        assert (D, c_x, c_m) == pytest.approx((float(k["D"]), float(k["c_x"]), float(k["c_m"])), rel=1e-13)
        for last in ("Mean", "Tweedie", "Euler"):
            if f"{i}_last_{last}" not in f:
                continue
            assert L.scldm_sde_last_coef_at(C.byref(tr), _lib.SDE_FORMS[form], norm, _lib.SDE_LAST_STEPS[last], lss, t, out2) == 0
            assert rel(out2[0] * x + out2[1] * m, f[f"{i}_last_{last}"]) < 1e-12, (i, last)


def test_reverse_ratio_is_zero_at_t0_and_the_gvp_end_point_is_exact():
    L = _lib.lib()
    out4, out2 = (C.c_double * 4)(), (C.c_double * 2)()
    tr = _tr("GVP", "velocity")
    assert L.scldm_sde_coef_at(C.byref(tr), _lib.SDE_FORMS["sigma"], 1.0, 0.0, 0.1, out4) == 0
    assert tuple(out4)[:3] == (1.0, -1.0, 1.0)                      # D = sigma = 1; score = -x (rr = 0, var = 1): f = m - x
    assert L.scldm_sde_coef_at(C.byref(tr), _lib.SDE_FORMS["SBDM"], 1.0, 0.0, 0.1, out4) == 0
    assert not math.isfinite(out4[0])                               # Dv(0) is infinite
    assert L.scldm_sde_last_coef_at(C.byref(tr), 0, 1.0, _lib.SDE_LAST_STEPS["Tweedie"], 0.0, 1.0, out2) == 0
    assert not all(map(math.isfinite, out2))                        # the score at t = 1 is singular


def test_bad_arguments_to_the_new_entries_return_err_shape():
    L = _lib.lib()
    out4, out2 = (C.c_double * 4)(), (C.c_double * 2)()
    good = _tr("GVP", "score")
    vp = _lib.TransportC(path=2, model=0, weight=0, train_eps=0.0, sample_eps=0.0)
    wide = _lib.TransportC(path=1, model=2, weight=0, train_eps=0.0, sample_eps=0.5)
    for tr in (None, C.byref(vp), C.byref(wide)):
        assert L.scldm_sde_coef_at(tr, 0, 1.0, 0.5, 0.1, out4) == -1 and L.scldm_last_error()
        assert L.scldm_sde_last_coef_at(tr, 0, 1.0, 1, 0.04, 0.96, out2) == -1
        assert L.scldm_logp_transport_workspace_bytes(None, 3, 1, 0, tr) == 0
        # (the transport is checked before the handle is touched: nothing is launched, nothing dereferenced)
        assert L.scldm_sample_sde_transport(None, None, None, 0, None, 3, 0, None, None, 4, 0, 0, 1.0, 1, 0.04, None, 1, 0, 3, None, 0, None, None, tr) == -1
        assert L.scldm_logp_ode_transport(None, None, None, None, 0, None, 3, 0, None, None, 3, 0, None, 1, 0, 3, None, None, 0, None, None, None, tr) == -1
    assert L.scldm_sde_coef_at(C.byref(good), 9, 1.0, 0.5, 0.1, out4) == -1          # unknown form
    assert L.scldm_sde_coef_at(C.byref(good), 0, 1.0, 0.5, 0.1, None) == -1          # null out
    assert L.scldm_sde_last_coef_at(C.byref(good), 0, 1.0, 0, 0.04, 0.96, out2) == -1     # last step NONE has no coefficients
    assert L.scldm_sde_last_coef_at(C.byref(good), 0, 1.0, 7, 0.04, 0.96, out2) == -1
    assert L.scldm_sde_last_coef_at(C.byref(good), 0, 1.0, 1, 0.04, 0.96, None) == -1
    # a good transport with null pointers: refused by the entries' own null checks
    assert L.scldm_logp_ode_transport(None, None, None, None, 0, None, 3, 0, None, None, 3, 0, None, 1, 0, 3, None, None, 0, None, None, None, C.byref(good)) == -1
    assert L.scldm_logp_transport_workspace_bytes(None, 3, 1, 0, C.byref(good)) == 0


# ---------------------------------------------------------------------------------------------------------------- the refusal rule
def test_refusal_rule_names_the_evaluation_and_its_time():
    x0 = torch.zeros(2, 3)
    calls = []
    model = lambda x, t: (calls.append(1), x)[1]
    with pytest.raises(ValueError, match=r"evaluation 0 .* t = 0\b"):          # SBDM for a velocity model: Dv(0) is infinite
        Sampler(R.make_transport("GVP", "velocity", 0.0)).sample_sde(diffusion_form="SBDM", num_steps=5)
    with pytest.raises(ValueError, match=r"evaluation 4 .* t = 1\b"):          # Tweedie at t1 = 1 for a velocity model
        Sampler(R.make_transport("GVP", "velocity", 0.0)).sample_sde(diffusion_form="sigma", last_step="Tweedie", last_step_size=0.0, num_steps=5)
    with pytest.raises(ValueError, match=r"evaluation 0 .* t = 0\b"):          # a noise / score transport with sample_eps = 0
        Sampler(R.make_transport("Linear", "score", 0.0)).sample_sde(diffusion_form="sigma", num_steps=5)
    with pytest.raises(ValueError, match="sample_eps > 0"):                   # the likelihood: refused as the one-call ODE sampler refuses it
        Sampler(R.make_transport("GVP", "noise", 0.0)).sample_ode_likelihood(sampling_method="euler", num_steps=4)
    assert not calls
    # Heun without a last step for a score model with eps > 0: the reference computes a finite result there, so it runs
    fn = Sampler(R.make_transport("Linear", "score", 0.05)).sample_sde(sampling_method="Heun", diffusion_form="linear", last_step=None, num_steps=5)
    torch.manual_seed(1)
    xs = fn(torch.randn(4, 6), R.toy_model)
    assert len(xs) == 5 and all(torch.isfinite(x).all() for x in xs)
    # the arguments of the default transport's sampler are checked the same way
    s = Sampler(R.make_transport("GVP", "score", 0.05))
    for kw in (dict(diffusion_form="quadratic"), dict(sampling_method="dopri5", diffusion_form="sigma"), dict(diffusion_form="sigma", last_step="Median")):
        with pytest.raises(NotImplementedError):
            s.sample_sde(**kw)
    for kw in (dict(diffusion_form="sigma", num_steps=1), dict(diffusion_form="sigma", last_step_size=1.0)):
        with pytest.raises(ValueError):
            s.sample_sde(**kw)


# ---------------------------------------------------------------------------------------------------------------- what the switch leaves alone
def test_switch_off_raises_as_before_and_default_transport_is_untouched_by_it():
    assert create_transport("GVP", "score").samplers_enabled is False
    for path, pred in (("GVP", "velocity"), ("Linear", "noise"), ("GVP", "score")):
        s = Sampler(create_transport(path, pred))
        with pytest.raises(NotImplementedError):
            s.sample_sde(diffusion_form="sigma")
        with pytest.raises(NotImplementedError):
            s.sample_ode_likelihood(sampling_method="euler")
    with pytest.raises(NotImplementedError):
        create_transport("VP", "velocity", samplers_enabled=True)
    on, off = create_transport(samplers_enabled=True), create_transport()
    assert on.is_default and on.samplers_enabled
    x0 = torch.randn(4, 6, generator=torch.Generator().manual_seed(2))
    runs = []
    for tr in (on, off):
        torch.manual_seed(11)
        xs = Sampler(tr).sample_sde(sampling_method="Heun", diffusion_form="decreasing", last_step="Tweedie", num_steps=4)(x0, R.toy_model)
        fn = Sampler(tr).sample_ode_likelihood(sampling_method="heun", num_steps=4)
        runs.append((torch.stack(xs), *fn(x0, R.toy_model)))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match="sigma"):
        Sampler(on).sample_sde()                                   # SBDM, the reference's default form, stays refused by name
    with pytest.raises(ValueError, match="Mean"):
        Sampler(on).sample_sde(sampling_method="Heun", diffusion_form="sigma", last_step=None)
    with pytest.raises(NotImplementedError):
        on.path_sampler.compute_diffusion(x0, torch.full((4,), 0.5), form="SBDM")
    with pytest.raises(NotImplementedError):
        R.make_transport("GVP", "score", 0.05).path_sampler.compute_diffusion(x0, torch.full((4,), 0.5), form="SBDM")

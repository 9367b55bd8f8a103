"""CPU checks of the wider transport family (GVP path, noise / score prediction, loss weights): the handle-free coefficient entry
against the reference's path classes in float64, the Python `Transport` on CPU tensors against the reference's fp32 results
(tests/golden/transport_paths_*.npz, written by tests/golden/make_golden_transport_paths.py), the eps / interval rules, the generic
ODE loop, and the argument checks of the new C entries (none of which reaches a device)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import transport_paths_ref as R
from conftest import load_golden, max_abs_rel

PATHS = {"Linear": 0, "GVP": 1}
MODELS = {"velocity": 0, "noise": 1, "score": 2}
WEIGHTS = {None: 0, "velocity": 1, "likelihood": 2}


def _tr(path_type="Linear", prediction="noise", loss_weight=None, train_eps=1e-3, sample_eps=1e-3):
    from scldm_amd import _lib
    return _lib.TransportC(PATHS[path_type], MODELS[prediction], WEIGHTS[loss_weight], train_eps, sample_eps)


def test_coef_entry_matches_reference_path_classes_in_float64():
    """scldm_transport_coef_at evaluates the same formulas in double: 1e-10 relative (the worst conditioning is tan at t = 0.999,
    about 1e3 ulp).  The derived fields follow from the table by their definitions."""
    from scldm_amd import _lib
    L = _lib.lib()
    g = load_golden("transport_paths_coef")
    assert list(g["t"]) == R.COEF_T
    k = _lib.TransportCoef()
    for path_type in PATHS:
        for prediction in MODELS:
            for weight in WEIGHTS:
                tr = _tr(path_type, prediction, weight)
                for i, t in enumerate(R.COEF_T):
                    assert L.scldm_transport_coef_at(C.byref(tr), t, C.byref(k)) == 0
                    for name in ("alpha", "d_alpha", "sigma", "d_sigma", "ratio", "dv"):
                        ref = float(g[f"{path_type}_{name}"][i])
                        assert abs(getattr(k, name) - ref) <= 1e-10 * abs(ref), (path_type, name, t)
                    ours = R.coef(path_type, prediction, weight, t)
                    for name in ("a", "b", "c", "w"):
                        assert abs(getattr(k, name) - float(ours[name])) <= 1e-10 * abs(float(ours[name])), (path_type, prediction, weight, name, t)
    # end points come as the formula gives them; a velocity model reads none of them
    assert L.scldm_transport_coef_at(C.byref(_tr("Linear", "noise")), 0.0, C.byref(k)) == 0 and math.isinf(k.ratio) and math.isinf(k.a)
    assert L.scldm_transport_coef_at(C.byref(_tr("Linear", "velocity")), 0.0, C.byref(k)) == 0
    assert (k.a, k.b, k.c, k.w) == (0.0, 1.0, 1.0, 1.0)


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: R.case_key(*c))
def test_python_transport_matches_reference_fp32(case):
    """Transport.training_losses / path_sampler.plan / get_drift on CPU tensors with a plain callable model, against what the
    reference returned for the same (t, x0): test_abi_cpu's 2e-5."""
    from scldm_amd.transport import create_transport
    g = load_golden("transport_paths_kernel")
    n = R.KERNEL_N[0]
    x1, x0, t = (torch.from_numpy(g[f"n{n}_{k}"]) for k in ("x1", "x0", "t"))
    tr = create_transport(*case)
    _, xt, ut = tr.path_sampler.plan(t, x0, x1)
    assert max_abs_rel(xt, g[f"n{n}_{case[0]}_xt"]) < 2e-5 and max_abs_rel(ut, g[f"n{n}_{case[0]}_ut"]) < 2e-5
    tr.sample = lambda x1_: (t, x0, x1_)
    out = tr.training_losses(R.toy_model, x1)
    assert max_abs_rel(out["loss"], g[f"n{n}_{R.case_key(*case)}_loss"]) < 2e-5
    assert max_abs_rel(out["pred"], g[f"n{n}_{case[0]}_pred"]) < 2e-5
    drift = tr.get_drift()(torch.from_numpy(g[f"n{n}_{case[0]}_xt"]), t, R.toy_model)
    assert max_abs_rel(drift, g[f"drift_{case[0]}_{case[1]}"]) < 2e-5
    # the float64 restatement the GPU tests lean on agrees with the reference too
    gl = g[f"n{n}_gloss"]
    _, _, _, loss, dm = R.plan_loss_ref(*case, x1.reshape(n, -1), x0.reshape(n, -1), t, g[f"n{n}_{case[0]}_pred"].reshape(n, -1), gl)
    assert max_abs_rel(loss, g[f"n{n}_{R.case_key(*case)}_loss"]) < 2e-5
    assert max_abs_rel(dm, g[f"n{n}_{R.case_key(*case)}_dpred"].reshape(n, -1)) < 2e-5


def test_eps_and_interval_rules():
    from scldm_amd.transport import ModelType, PathType, WeightType, create_transport
    for path_type in ("Linear", "GVP"):
        tr = create_transport(path_type, "velocity", "likelihood", 1e-2, 1e-2)         # velocity: both forced to 0, [0, 1]
        assert (tr.train_eps, tr.sample_eps) == (0, 0) and tr.check_interval(tr.train_eps, tr.sample_eps) == (0, 1)
        assert tr.check_interval(tr.train_eps, tr.sample_eps, eval=True) == (0, 1)
        for prediction in ("noise", "score"):
            tr = create_transport(path_type, prediction)
            assert (tr.train_eps, tr.sample_eps) == (1e-3, 1e-3)                        # sample_eps=None -> 1e-3 (the documented rule)
            assert tr.check_interval(tr.train_eps, tr.sample_eps) == (1e-3, 1 - 1e-3)
            tr = create_transport(path_type, prediction, None, 1e-2, 5e-3)
            assert tr.check_interval(tr.train_eps, tr.sample_eps) == (1e-2, 1 - 1e-2)
            assert tr.check_interval(tr.train_eps, tr.sample_eps, eval=True) == (5e-3, 1 - 5e-3)
            assert tr.check_interval(tr.train_eps, tr.sample_eps, eval=True, reverse=True) == (1 - 5e-3, 1 - (1 - 5e-3))
            tr = create_transport(path_type, prediction, None, 1e-2)                    # train_eps given, sample_eps None -> 1e-3
            assert (tr.train_eps, tr.sample_eps) == (1e-2, 1e-3)
    tr = create_transport("GVP", "score", "likelihood")
    assert (tr.path_type, tr.model_type, tr.loss_type) == (PathType.GVP, ModelType.SCORE, WeightType.LIKELIHOOD) and not tr.is_default
    assert create_transport().is_default and not create_transport("GVP").is_default
    # training draws are scaled into the interval
    torch.manual_seed(3)
    t, x0, x1 = create_transport("Linear", "noise", None, 0.25, 0.25).sample(torch.zeros(4000, 2))
    assert 0.25 <= float(t.min()) and float(t.max()) <= 0.75 and float(t.max()) - float(t.min()) > 0.49
    torch.manual_seed(3)
    torch.randn(4000, 2)                                   # (x0 is drawn first)
    assert torch.equal(t, torch.rand(4000) * (0.75 - 0.25) + 0.25)
    with pytest.raises(ValueError):
        create_transport("Linear", "noise", None, 0.5, 1e-3)
    with pytest.raises(ValueError):
        create_transport("Linear", "noise", None, 1e-3, -1e-3)


def test_vp_and_out_of_scope_samplers_raise():
    from scldm_amd.transport import Sampler, create_transport
    for prediction in ("velocity", "noise", "score"):
        with pytest.raises(NotImplementedError):
            create_transport("VP", prediction)
    for tr in (create_transport("GVP"), create_transport("Linear", "noise"), create_transport("GVP", "score")):
        with pytest.raises(NotImplementedError):
            Sampler(tr).sample_sde(diffusion_form="sigma")
        with pytest.raises(NotImplementedError):
            Sampler(tr).sample_ode_likelihood()


@pytest.mark.parametrize("path_type", ["Linear", "GVP"])
def test_generic_sample_ode_closed_form(path_type):
    """With m = 0 a noise model's drift is (alpha'/alpha) x: the grid is linspace(t0, t1) and the Euler states equal a hand loop exactly."""
    from scldm_amd.transport import Sampler, create_transport
    tr = create_transport(path_type, "noise", None, 1e-3, 1e-2)
    seen = []
    fn = Sampler(tr).sample_ode(sampling_method="euler", num_steps=6)
    x = torch.tensor([[1.0, -2.0, 0.5], [0.25, 3.0, -1.0]])
    traj = fn(x, lambda xx, t: (seen.append(float(t[0])), torch.zeros_like(xx))[1])
    ts = torch.linspace(1e-2, 1 - 1e-2, 6)
    assert seen == [float(v) for v in ts[:-1]] and traj.shape == (6, 2, 3)
    ratio = tr.path_sampler.compute_d_alpha_alpha_ratio_t
    state = x
    for i in range(5):
        tv = torch.full((), float(ts[i]), dtype=torch.float32).expand(2).view(2, 1)
        state = state + float(ts[i + 1] - ts[i]) * (ratio(tv) * state)      # (the m = 0 term adds a signed zero)
        assert torch.equal(traj[i + 1], state)
    # the growth is the closed form's: prod (1 + h alpha'/alpha) per component
    grow = np.prod([1 + float(ts[i + 1] - ts[i]) * float(R.coef(path_type, "noise", None, float(ts[i]))["ratio"]) for i in range(5)])
    assert max_abs_rel(traj[-1], x.double() * grow) < 1e-5
    # dopri5 integrates over the same interval
    fn = Sampler(tr)._sample_dopri5(3, 1e-5, 1e-5)
    traj = fn(x, lambda xx, t: torch.zeros_like(xx))
    al = lambda t: float(R.coef(path_type, "noise", None, t)["alpha"])
    assert max_abs_rel(traj[-1], x.double() * (al(1 - 1e-2) / al(1e-2))) < 1e-3      # x' = (alpha'/alpha) x  =>  x(t) = x(t0) alpha(t) / alpha(t0)


def test_new_entries_reject_bad_arguments():
    """SCLDM_ERR_SHAPE (-1) for an unknown enum, VP, a negative eps, an eps >= 0.5 and null pointers - all decided before any launch."""
    from scldm_amd import _lib
    L = _lib.lib()
    k = _lib.TransportCoef()
    bad = [_lib.TransportC(2, 0, 0, 0, 0), _lib.TransportC(-1, 0, 0, 0, 0), _lib.TransportC(0, 3, 0, 0, 0), _lib.TransportC(0, 0, 3, 0, 0),
           _lib.TransportC(0, 1, 0, -1e-3, 1e-3), _lib.TransportC(0, 1, 0, 1e-3, 0.5), _lib.TransportC(1, 2, 1, float("nan"), 1e-3)]
    for tr in bad:
        assert L.scldm_transport_coef_at(C.byref(tr), 0.5, C.byref(k)) == -1
        assert L.scldm_fm_plan(C.byref(tr), 8, 8, 8, 8, 8, 8, 1, 4, None) == -1
        assert L.scldm_fm_prepare_transport(C.byref(tr), 8, None, None, 1, 0, 1, 0.1, 8, 1, 4, 8, None, 8, 8, 8, 8, None) == -1
        assert L.scldm_sample_ode_transport(None, 8, None, 0, None, 1, 0, None, None, 1, 0, C.byref(tr), 0, 8, None) == -1
        assert L.scldm_dit_train_step_transport(8, None, None, None, None, None, 1, 0, 0.1, None, 1, 1, None, C.byref(tr), None, None, None) == -1
    good = _tr()
    assert L.scldm_transport_coef_at(None, 0.5, C.byref(k)) == -1 and L.scldm_transport_coef_at(C.byref(good), 0.5, None) == -1
    assert L.scldm_fm_plan(None, 8, 8, 8, 8, 8, 8, 1, 4, None) == -1
    assert L.scldm_fm_plan(C.byref(good), None, 8, 8, 8, 8, 8, 1, 4, None) == -1
    assert L.scldm_fm_plan(C.byref(good), 8, 8, 8, 8, 8, None, 1, 4, None) == -1
    assert L.scldm_fm_plan(C.byref(good), 8, 8, 8, 8, 8, 8, 0, 4, None) == -1
    assert L.scldm_fm_wloss(8, 8, None, 8, 1, 4, None) == -1 and L.scldm_fm_wloss(8, 8, 8, 8, 1, 0, None) == -1
    assert L.scldm_fm_wloss_bwd(8, 8, 8, None, 8, 1, 4, None) == -1
    assert L.scldm_fm_wloss_grad(8, 8, None, 1, 4, 8, 8, 8, 8, None, None) == -1
    assert L.scldm_fm_prepare_transport(C.byref(good), 8, None, None, 1, 0, 1, 0.1, 8, 1, 4, 8, None, 8, 8, 8, 8, None) == -1
    assert b"bad" in L.scldm_last_error()
    # Python refuses the same
    from scldm_amd.transport import ModelType, PathType, Transport, WeightType
    with pytest.raises(NotImplementedError):
        Transport(model_type=ModelType.NOISE, path_type=PathType.VP, loss_type=WeightType.NONE, train_eps=1e-5, sample_eps=1e-3)

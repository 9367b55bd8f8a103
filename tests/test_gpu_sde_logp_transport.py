"""GPU tests of the SDE sampler and the likelihood under the non-default transports (scldm_sample_sde_transport /
scldm_logp_ode_transport, DiT.sample_sde_cfg(..., transport=) / DiT.log_likelihood_cfg(..., transport=)): against the reference's recorded
runs (tests/golden/sdet_*.npz, logpt_*.npz; noise and probes are the fixtures', so everything downstream of the draws is compared), the
CPU restatement of tests/transport_solvers_ref.py, the generic Python samplers, the default transport's entries, and themselves across
seeds and shards.  B = 3 from the fixtures (1 536 state elements: one and a half workgroups of the elementwise kernels, one padded wave
block of the row kernels), plus B = 1 (a partial workgroup) and B = 6 (three workgroups; two blocks of four waves).

Tolerances: fp32 / bf16x3 1e-4 on max|a-b| / max|b| of every returned state, logp, x_end, logp_grad and of the divergence term
logp_grad - a(t) e alone (a e formed in float64: the x term is ~90 % of a logp_grad and would hide the kernel's b * dot path).  bf16 / fp16:
the SDE through the arithmetic-class gate of tests/precision_class.py against the restatement with reduced operand bits; the likelihood at
most 1.5 x the generic sampler's own distance at the same precision - both as tests/test_gpu_sde.py and tests/test_gpu_logp.py gate the
default transport."""
import ctypes as C

import numpy as np
import pytest
import torch

import transport_solvers_ref as R
from conftest import check_err, max_abs_rel
from precision_class import exact_result, gate_tensor
from scldm_amd import _lib
from test_gpu_dit import BITS, FLOOR_TOL, PARITY, SIXTEEN, build

pytestmark = pytest.mark.gpu


def _st():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------------------------- SDE
def _sde_inputs(name):
    f, sd, cfg, z2, cond2, scales, (path, pred, *settings) = R.load_sde_case(name)
    return f, z2.cuda(), {k: v.cuda() for k, v in cond2.items()}, scales, R.make_transport(path, pred, R.SDE_EPS), tuple(settings)


def _check_states(got, want, tol, what):
    got = torch.as_tensor(got).cpu()
    assert got.shape == tuple(want.shape) and torch.isfinite(got).all()
    for i in range(got.shape[0]):
        e = max_abs_rel(got[i], want[i])
        print(f"[parity] {what} state {i}: max|a-b|/max|b| = {e:.3e}   tol {tol:g}")
        assert e < tol, (what, i, e)


def _sde_gate(traj, name, precision, tol, what):
    f = R.load_sde_case(name)[0]
    if precision not in BITS:
        _check_states(traj, f["traj"], tol, f"{what} {name} [{precision}] vs the reference's recorded run")
        return
    fn = R.oracle_sde_solve(name)
    ref = exact_result(fn, f"sdet/{name}")
    check_err(traj.cpu(), ref, tol, f"{what} {name} [{precision}] vs restatement", FLOOR_TOL[precision])
    gate_tensor(traj.cpu(), ref, fn, BITS[precision], f"{what} {name} vs restatement", tag=f"sdet/{name}")


def _fused_sde(m, name):
    f, z2, cond, scales, tr, (method, form, norm, last, lss, steps) = _sde_inputs(name)
    return m.sample_sde_cfg(z2, cond, scales, steps, method, form, norm, last, lss, noise=torch.from_numpy(f["noise"]).cuda(),
                            return_trajectory=True, transport=tr)


@pytest.mark.parametrize("name", list(R.SDE_CASES))
@pytest.mark.parametrize("precision,tol", PARITY + SIXTEEN)
def test_fused_sde_solve_on_recorded_noise(name, precision, tol):
    g, m, cfg, sd = build(R.SDE_CASES[name][0], precision)
    traj = _fused_sde(m, name)
    assert traj.shape[0] == R.SDE_CASES[name][-1]
    _sde_gate(traj, name, precision, tol, "fused SDE solve")


@pytest.mark.parametrize("name", ["sdet_linear_noise_euler", "sdet_gvp_velocity_heun"])
@pytest.mark.parametrize("precision,tol", PARITY + SIXTEEN)
def test_generic_sde_sampler_over_forward_with_cfg(name, precision, tol):
    """Sampler(tr).sample_sde -> lambda -> forward_with_cfg with the fixture's draws: the fused call's gates, and within 1e-4 of the fused
    call where operands are not rounded to 16 bits."""
    from scldm_amd.transport import Sampler
    g, m, cfg, sd = build(R.SDE_CASES[name][0], precision)
    f, z2, cond, scales, tr, (method, form, norm, last, lss, steps) = _sde_inputs(name)
    draws = iter(torch.from_numpy(f["noise"]).cuda())
    fn = Sampler(tr).sample_sde(sampling_method=method, diffusion_form=form, diffusion_norm=norm, last_step=last, last_step_size=lss, num_steps=steps)
    xs = fn(z2, lambda x, t, **kw: m.forward_with_cfg(x, t, **kw, cfg_scale=scales), _draw=lambda x: next(draws), condition=cond)
    traj = torch.stack(xs)
    _sde_gate(traj, name, precision, tol, "generic SDE sampler")
    if precision not in BITS:
        assert max_abs_rel(traj.cpu(), _fused_sde(m, name).cpu()) < tol


def test_sde_noise_source_seed_shards_and_one_cell():
    from scldm_amd.sampling import sample_latents
    g, m, cfg, sd = build("dit_base", "bf16")
    tr = R.make_transport("GVP", "score", R.SDE_EPS)
    gen = torch.Generator().manual_seed(23)
    z0 = torch.randn(6, 16, 16, generator=gen).cuda()
    lab = {"clusters": torch.randint(0, 14, (6,), generator=gen).cuda()}
    scales = {"clusters": 1.5}
    z2, cond2 = torch.cat([z0[:3], z0[:3]]), {"clusters": lab["clusters"][:3].repeat(2)}
    for method, last in (("euler", "Mean"), ("heun", None)):
        a = m.sample_sde_cfg(z2, cond2, scales, 4, method, "SBDM", 1.0, last, seed=1234, transport=tr)
        noise = torch.stack([m.sde_noise(1234, s, 3) for s in range(3)])
        b = m.sample_sde_cfg(z2, cond2, scales, 4, method, "SBDM", 1.0, last, noise=noise, transport=tr)
        assert torch.isfinite(a).all() and torch.equal(a, b)
        assert not torch.equal(a, m.sample_sde_cfg(z2, cond2, scales, 4, method, "SBDM", 1.0, last, seed=1235, transport=tr))
        # B = 6 whole = two shards of 3, through sample_latents as a sharded caller passes it
        opts = dict(diffusion_form="SBDM", diffusion_norm=0.5, last_step=last, seed=99)
        whole = sample_latents(m, z0, lab, scales, 4, method, sde=dict(opts), transport=tr)
        assert whole.shape == (12, 16, 16) and torch.isfinite(whole).all()
        for lo in (0, 3):
            part = sample_latents(m, z0[lo:lo + 3], {"clusters": lab["clusters"][lo:lo + 3]}, scales, 4, method,
                                  sde=dict(opts, cell_offset=lo, cells_total=6), transport=tr)
            assert torch.equal(part[:3], whole[lo:lo + 3]) and torch.equal(part[3:], whole[6 + lo:6 + lo + 3])
        # B = 1: cell 0 of the 6-cell solve
        one = m.sample_sde_cfg(torch.cat([z0[:1], z0[:1]]), {"clusters": lab["clusters"][:1].repeat(2)}, scales, 4, method, "SBDM", 0.5, last,
                               seed=99, cells_total=6, transport=tr)
        assert torch.isfinite(one).all() and torch.equal(one[0], whole[0]) and torch.equal(one[1], whole[6])


# ---------------------------------------------------------------------------------------------------------------- likelihood
_REF = {}


def _restatement(name):
    if name not in _REF:
        from oracle.dit import dit_forward_with_cfg
        f, sd, cfg, z2, cond2, scales, (path, pred, method, steps, eps) = R.load_logp_case(name)
        n_thr = torch.get_num_threads()
        torch.set_num_threads(min(16, n_thr))
        try:
            _REF[name] = R.logp_ref(z2, lambda x, t: dit_forward_with_cfg(sd, cfg, x, t, cond2, scales), path, pred, eps, method, steps,
                                    torch.from_numpy(f["probes"]))
        finally:
            torch.set_num_threads(n_thr)
    return _REF[name]


def _logp_inputs(name):
    f, sd, cfg, z2, cond2, scales, (path, pred, method, steps, eps) = R.load_logp_case(name)
    return f, z2.cuda(), {k: v.cuda() for k, v in cond2.items()}, scales, R.make_transport(path, pred, eps), method, steps


def _distances(got, name):
    """Scale-relative distances to the fixture: (logp_grad, its divergence term logp_grad - a(t) e, logp, x_end)."""
    logp, z_end, trace = got
    f = R.load_logp_case(name)[0]
    ae = np.array(_restatement(name)[5])[:, None]
    assert trace.shape == f["logp_grad"].shape and torch.isfinite(trace).all() and torch.isfinite(logp).all() and torch.isfinite(z_end).all()
    div, div_ref = trace.cpu().double().numpy() - ae, f["logp_grad"].astype(np.float64) - ae
    return (max_abs_rel(trace.cpu(), f["logp_grad"]), float(np.abs(div - div_ref).max() / np.abs(div_ref).max()),
            max_abs_rel(logp.cpu(), f["logp"]), max_abs_rel(z_end.cpu(), f["x_end"]))


def _fused_logp(m, name):
    f, z2, cond, scales, tr, method, steps = _logp_inputs(name)
    return m.log_likelihood_cfg(z2, cond, scales, steps + 1, method, probe=torch.from_numpy(f["probes"]).cuda(), return_trace=True, transport=tr)


def _generic_logp(m, name):
    from scldm_amd.transport import Sampler
    f, z2, cond, scales, tr, method, steps = _logp_inputs(name)
    probes = iter(torch.from_numpy(f["probes"]).cuda())
    fn = Sampler(tr).sample_ode_likelihood(sampling_method=method, num_steps=steps + 1)
    logp, z_end = fn(z2, lambda x, t: m._composed_forward_with_cfg(x, t.contiguous(), cond, scales), _probe=lambda x: next(probes))
    return logp, z_end, torch.stack(fn.last_trace["logp_grad"])


_WHAT = ("logp_grad", "divergence term", "logp", "x_end")


@pytest.mark.parametrize("name", list(R.LOGP_CASES))
@pytest.mark.parametrize("precision,tol", PARITY)
def test_fused_likelihood_on_recorded_probes(name, precision, tol):
    g, m, cfg, sd = build(R.LOGP_CASES[name][0], precision)
    d = _distances(_fused_logp(m, name), name)
    print(f"[parity] fused likelihood {name} [{precision}]: " + ", ".join(f"{w} {v:.3e}" for w, v in zip(_WHAT, d)) + f"   tol {tol:g}")
    assert all(v <= tol for v in d), dict(zip(_WHAT, d))


@pytest.mark.parametrize("name", ["logpt_gvp_score_heun", "logpt_linear_noise_euler"])
def test_generic_likelihood_sampler_on_recorded_probes_fp32(name):
    g, m, cfg, sd = build(R.LOGP_CASES[name][0], "fp32")
    d = _distances(_generic_logp(m, name), name)
    print(f"[parity] generic likelihood sampler {name} [fp32]: " + ", ".join(f"{w} {v:.3e}" for w, v in zip(_WHAT, d)))
    assert all(v <= 1e-4 for v in d), dict(zip(_WHAT, d))


@pytest.mark.parametrize("name", list(R.LOGP_CASES))
@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_fused_likelihood_within_the_generic_paths_distance_16_bit(name, precision):
    """bf16 / fp16 operands: the fused solve and the generic sampler at the same precision run the same forward and backward kernels on the
    same probes and differ only in fp32 state arithmetic and summation order, so the fused solve's distance to the fp32 fixture may be at
    most 1.5 x the generic path's own (the factor of the project's operand-class gates), as tests/test_gpu_logp.py gates the default
    transport."""
    g, m, cfg, sd = build(R.LOGP_CASES[name][0], precision)
    d_f, d_g = _distances(_fused_logp(m, name), name), _distances(_generic_logp(m, name), name)
    for what, a, b in zip(_WHAT, d_f, d_g):
        print(f"[class] {name} [{precision}] {what}: fused {a:.4e}  generic {b:.4e}  ratio {a / b:.3f}")
    for what, a, b in zip(_WHAT, d_f, d_g):
        assert a <= 1.5 * b, (name, precision, what, a, b)


def test_likelihood_shards_equal_the_whole_solve_and_one_cell_runs():
    g, m, cfg, sd = build("dit_base", "bf16")
    gen = torch.Generator().manual_seed(29)
    x = torch.randn(6, 16, 16, generator=gen).cuda()
    lab = torch.randint(0, 14, (6,), generator=gen).cuda()
    scales = {"clusters": 1.5}
    for tr, method in ((R.make_transport("Linear", "noise", 0.05), "heun"), (R.make_transport("GVP", "velocity", 0.0), "euler")):
        whole = m.log_likelihood_cfg(torch.cat([x, x]), {"clusters": lab.repeat(2)}, scales, 3, method, seed=7, return_trace=True, transport=tr)
        assert all(torch.isfinite(v).all() for v in whole)
        for lo in (0, 3):
            part = m.log_likelihood_cfg(torch.cat([x[lo:lo + 3]] * 2), {"clusters": lab[lo:lo + 3].repeat(2)}, scales, 3, method, seed=7,
                                        cell_offset=lo, cells_total=6, return_trace=True, transport=tr)
            rows = list(range(lo, lo + 3)) + list(range(6 + lo, 6 + lo + 3))
            assert torch.equal(part[0], whole[0][rows]) and torch.equal(part[1], whole[1][rows]) and torch.equal(part[2], whole[2][:, rows])
        one = m.log_likelihood_cfg(torch.cat([x[:1]] * 2), {"clusters": lab[:1].repeat(2)}, scales, 3, method, seed=7, cells_total=6, transport=tr)
        assert torch.isfinite(one[0]).all() and torch.equal(one[0], whole[0][[0, 6]]) and torch.equal(one[1], whole[1][[0, 6]])


# ---------------------------------------------------------------------------------------------------------------- the entries themselves
def test_default_transport_through_the_new_entries_is_the_existing_solve_bit_for_bit():
    from scldm_amd.transport import create_transport
    g, m, cfg, sd = build("dit_base", "bf16")
    f, z2, cond, scales, _, _ = _sde_inputs("sdet_gvp_velocity_euler")
    B = z2.shape[0] // 2
    cs = create_transport().c_struct()
    ul, n_u, cell_row, n_pass, masks, sc, keep = m._cfg_plan(cond, scales, B, dedup=True)
    L, h = m._native()
    ws = m._workspace(L, 2 * B + n_pass * B, 1 + n_pass * n_u, 2 * B)
    z = z2.clone()
    _lib.check(L.scldm_sample_sde_transport(h, z.data_ptr(), C.cast(ul, _lib.c_void_pp), n_u, cell_row, B, n_pass, masks, sc, 4, 1, 3, 0.5, 2, 0.1,
                                            None, 77, 0, B, None, m._prec(), ws, _st(), C.byref(cs)), "scldm_sample_sde_transport")
    assert torch.equal(z, m.sample_sde_cfg(z2, cond, scales, 4, "heun", "decreasing", 0.5, "Tweedie", 0.1, seed=77))
    assert torch.equal(z, m.sample_sde_cfg(z2, cond, scales, 4, "heun", "decreasing", 0.5, "Tweedie", 0.1, seed=77, transport=create_transport(samplers_enabled=True)))
    # SBDM under the default transport stays that entry's refusal
    assert L.scldm_sample_sde_transport(h, z.data_ptr(), C.cast(ul, _lib.c_void_pp), n_u, cell_row, B, n_pass, masks, sc, 4, 0, 5, 1.0, 1, 0.04,
                                        None, 77, 0, B, None, m._prec(), ws, _st(), C.byref(cs)) == -1
    # the likelihood
    want = m.log_likelihood_cfg(z2, cond, scales, 3, "heun", seed=5, return_trace=True)
    got = m.log_likelihood_cfg(z2, cond, scales, 3, "heun", seed=5, return_trace=True, transport=create_transport(samplers_enabled=True))
    assert all(torch.equal(a, b) for a, b in zip(want, got))
    prec = m._prec()
    params = tuple(m.parameters())
    w, _ = m._weights_struct(params)
    N = (2 + n_pass) * B
    saved = torch.empty(L.scldm_dit_train_saved_bytes_for(h, N, prec), dtype=torch.uint8, device="cuda")
    nb = L.scldm_logp_transport_workspace_bytes(h, B, n_pass, prec, C.byref(cs))
    assert nb == L.scldm_logp_workspace_bytes(h, B, n_pass, prec) and nb > 0
    lws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    z, logp, trace = z2.clone(), torch.empty(2 * B, device="cuda"), torch.empty(4, 2 * B, device="cuda")
    _lib.check(L.scldm_logp_ode_transport(h, C.byref(w), z.data_ptr(), C.cast(ul, _lib.c_void_pp), n_u, cell_row, B, n_pass, masks, sc, 2, 1, None, 5,
                                          0, B, logp.data_ptr(), trace.data_ptr(), prec, saved.data_ptr(), lws.data_ptr(), _st(), C.byref(cs)),
               "scldm_logp_ode_transport")
    assert torch.equal(logp, want[0]) and torch.equal(z, want[1]) and torch.equal(trace, want[2])
    del keep


def test_refusals_leave_the_state_untouched_and_the_stream_usable():
    g, m, cfg, sd = build("dit_base", "fp32")
    f, z2, cond, scales, _, _ = _sde_inputs("sdet_gvp_velocity_euler")
    gv, sc0 = R.make_transport("GVP", "velocity", 0.0), R.make_transport("Linear", "score", 0.0)
    with pytest.raises(ValueError, match=r"evaluation 0 .* t = 0\b"):
        m.sample_sde_cfg(z2, cond, scales, 4, "euler", "SBDM", transport=gv)
    with pytest.raises(ValueError, match=r"evaluation 3 .* t = 1\b"):
        m.sample_sde_cfg(z2, cond, scales, 4, "euler", "sigma", 1.0, "Tweedie", 0.0, transport=gv)
    with pytest.raises(ValueError, match=r"evaluation 0 .* t = 0\b"):
        m.sample_sde_cfg(z2, cond, scales, 4, "euler", "sigma", transport=sc0)
    with pytest.raises(ValueError, match="sample_eps > 0"):
        m.log_likelihood_cfg(z2, cond, scales, 3, "euler", seed=1, transport=sc0)
    with pytest.raises(NotImplementedError):
        m.sample_sde_cfg(z2, cond, scales, 4, "euler", "sigma", transport=R.make_transport("GVP", "score", 0.05, enabled=False))
    with pytest.raises(NotImplementedError):
        m.log_likelihood_cfg(z2, cond, scales, 3, "euler", transport=R.make_transport("GVP", "score", 0.05, enabled=False))
    # the C ABI itself: SCLDM_ERR_SHAPE with a message, the state untouched
    L, h = m._native()
    before = z2.clone()
    ws = m._workspace(L, 6, 1, 6)
    cs = gv.c_struct()

    def call(form=0, last=1, lss=0.04, num_steps=4, method=0, tr=cs):
        return L.scldm_sample_sde_transport(h, before.data_ptr(), None, 0, None, 3, 0, None, None, num_steps, method, form, 1.0, last, lss, None, 1, 0, 3,
                                            None, 0, ws, _st(), C.byref(tr))

    for what, rc in (("SBDM for a velocity model", call(form=_lib.SDE_FORMS["SBDM"])), ("Tweedie at t1 = 1", call(last=2, lss=0.0)),
                     ("Mean at t1 = 1", call(last=1, lss=0.0)), ("score model with eps 0", call(tr=sc0.c_struct())), ("unknown form", call(form=9)),
                     ("one grid point", call(num_steps=1)), ("unknown method", call(method=2)), ("last_step_size 1", call(lss=1.0))):
        assert rc == -1 and L.scldm_last_error(), what
    torch.cuda.synchronize()
    assert torch.equal(before, z2)
    assert call() == 0      # the same call with valid arguments runs on the same stream
    torch.cuda.synchronize()
    assert torch.isfinite(before).all() and not torch.equal(before, z2)


def test_training_mode_and_a_wide_dit_take_the_generic_route():
    """Training mode (dropout-free module, so the same numbers) and a 512-wide DiT outside the fused family go through the same public calls
    and the generic samplers: the fp32 gate against the fixture / against the restatement over the module's own forward."""
    name = "sdet_gvp_score_heun"
    g, m, cfg, sd = build(R.SDE_CASES[name][0], "fp32")
    m.train()
    try:
        traj = _fused_sde(m, name)
        d = _distances(_fused_logp(m, "logpt_gvp_score_heun"), "logpt_gvp_score_heun")
    finally:
        m.eval()
    _sde_gate(traj, name, "fp32", 1e-4, "training-mode SDE solve")
    assert all(v <= 1e-4 for v in d), dict(zip(_WHAT, d))
    from test_gpu_train import build as build_wide
    wide, _, _ = build_wide({"a": 5, "b": 7}, "joint", 2, 77, n_embed=512, n_head=8)
    wide = wide.cuda().eval()
    wide.precision = "fp32"
    assert not wide.fused_shape
    gen = torch.Generator().manual_seed(31)
    z0 = torch.randn(3, wide.seq_len, wide.n_embed_input, generator=gen).cuda()
    cond2 = {"a": torch.randint(0, 5, (3,), generator=gen).cuda().repeat(2), "b": torch.randint(0, 7, (3,), generator=gen).cuda().repeat(2)}
    scales, z2 = {"a": 1.5, "b": 1.1}, torch.cat([z0, z0])
    tr = R.make_transport("Linear", "noise", 0.05)
    noise = torch.randn(3, *z2.shape, generator=gen).cuda()
    got = wide.sample_sde_cfg(z2, cond2, scales, 4, "euler", "SBDM", 1.0, "Mean", 0.04, noise=noise, return_trajectory=True, transport=tr)
    fwd = lambda x, t: wide._generic_forward_with_cfg(x, t.contiguous(), cond2, scales)
    want = torch.stack(R.sample_sde_ref(z2, lambda x, t: fwd(x, t.cuda()), "Linear", "noise", 0.05, 4, "euler", "SBDM", 1.0, "Mean", 0.04, noise)[0])
    _check_states(got, want.cpu(), 1e-4, "wide DiT SDE solve vs restatement")
    logp, z_end = wide.log_likelihood_cfg(z2, cond2, scales, 3, "euler", seed=3, transport=tr)
    assert logp.shape == (6,) and torch.isfinite(logp).all() and torch.isfinite(z_end).all()

"""GPU tests of the fused SDE sampler (scldm_sample_sde / DiT.sample_sde_cfg) and its noise source (scldm_sde_noise): against the
reference's recorded runs (tests/golden/sde_*.npz; the noise is the fixture's, so everything downstream of the draws is compared), the
CPU restatement of tests/sde_ref.py, the ODE sampler, and itself across seeds, shards and plans.  B in {1, 3, 6} cells = 512, 1 536,
3 072 state elements: with four elements per thread a partial workgroup, one and a half, and three.

Tolerances: fp32 / bf16x3 1e-4 on max|a-b| / max|b| of EVERY returned state (the project's gate); bf16 / fp16 through the arithmetic-class
gate of tests/precision_class.py against the restatement with reduced operand bits, as test_fused_sampler_vs_oracle gates the ODE."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import sde_ref
from conftest import check_err, max_abs_rel
from precision_class import exact_result, gate_tensor
from test_gpu_dit import BITS, FLOOR_TOL, PARITY, SIXTEEN, build

pytestmark = pytest.mark.gpu


def _inputs(name):
    f, sd, cfg, z2, cond2, scales, settings = sde_ref.load_case(name)
    return f, z2.cuda(), {k: v.cuda() for k, v in cond2.items()}, scales, settings


def _check_states(got, want, tol, what):
    got = torch.as_tensor(got).cpu()
    assert got.shape == tuple(want.shape) and torch.isfinite(got).all()
    for i in range(got.shape[0]):
        e = max_abs_rel(got[i], want[i])
        print(f"[parity] {what} state {i}: max|a-b|/max|b| = {e:.3e}   tol {tol:g}")
        assert e < tol, (what, i, e)


def _gate(traj, name, precision, tol, what):
    """One trajectory against the gates of its precision: the reference's recorded states (fp32 / bf16x3), or the exact restatement under
    the flat bound plus the class gate (bf16 / fp16)."""
    f = sde_ref.load_case(name)[0]
    if precision not in BITS:
        _check_states(traj, f["traj"], tol, f"{what} {name} [{precision}] vs the reference's recorded run")
        return
    fn = sde_ref.oracle_solve(name)
    ref = exact_result(fn, f"sde/{name}")
    check_err(traj.cpu(), ref, tol, f"{what} {name} [{precision}] vs restatement", FLOOR_TOL[precision])
    gate_tensor(traj.cpu(), ref, fn, BITS[precision], f"{what} {name} vs restatement", tag=f"sde/{name}")


@pytest.mark.parametrize("name", list(sde_ref.CASES))
@pytest.mark.parametrize("precision,tol", PARITY + SIXTEEN)
def test_fused_solve_on_recorded_noise(name, precision, tol):
    g, m, cfg, sd = build(sde_ref.CASES[name][0], precision)
    f, z2, cond, scales, (method, form, norm, last, lss, steps) = _inputs(name)
    traj = m.sample_sde_cfg(z2, cond, scales, steps, method, form, norm, last, lss, noise=torch.from_numpy(f["noise"]).cuda(), return_trajectory=True)
    assert traj.shape == (steps, *z2.shape)
    _gate(traj, name, precision, tol, "fused SDE solve")


@pytest.mark.parametrize("name", ["sde_base_euler", "sde_me2_heun"])
@pytest.mark.parametrize("precision,tol", PARITY + SIXTEEN)
def test_generic_sampler_over_forward_with_cfg(name, precision, tol, monkeypatch):
    """The reference-shaped call chain (Sampler.sample_sde -> lambda -> forward_with_cfg) with the host generator's draws replaced by the
    fixture's: same gates as the fused call, and within the same 1e-4 of it where operands are not rounded to 16 bits."""
    from scldm_amd.transport import Sampler, create_transport
    g, m, cfg, sd = build(sde_ref.CASES[name][0], precision)
    f, z2, cond, scales, (method, form, norm, last, lss, steps) = _inputs(name)
    draws = iter(torch.from_numpy(f["noise"]))
    real_randn = torch.randn
    monkeypatch.setattr(torch, "randn", lambda *a, **k: next(draws) if (a and tuple(a[0]) == tuple(z2.shape)) else real_randn(*a, **k))
    fn = Sampler(create_transport()).sample_sde(sampling_method=method, diffusion_form=form, diffusion_norm=norm, last_step=last,
                                                last_step_size=lss, num_steps=steps)
    xs = fn(z2, lambda x, t, **kw: m.forward_with_cfg(x, t, **kw, cfg_scale=scales), condition=cond)
    monkeypatch.undo()
    assert len(xs) == steps
    traj = torch.stack(xs)
    _gate(traj, name, precision, tol, "generic SDE sampler")
    if precision not in BITS:
        fused = m.sample_sde_cfg(z2, cond, scales, steps, method, form, norm, last, lss, noise=torch.from_numpy(f["noise"]).cuda(), return_trajectory=True)
        assert max_abs_rel(traj.cpu(), fused.cpu()) < tol


@pytest.mark.parametrize("method,last", [("euler", "Mean"), ("heun", "Tweedie")])
def test_seed_is_the_noise_of_scldm_sde_noise(method, last):
    g, m, cfg, sd = build("dit_base", "bf16")
    f, z2, cond, scales, _ = _inputs("sde_base_euler")
    steps, B = 4, z2.shape[0] // 2
    a = m.sample_sde_cfg(z2, cond, scales, steps, method, "sigma", 1.0, last, seed=1234)
    noise = torch.stack([m.sde_noise(1234, s, B) for s in range(steps - 1)])
    b = m.sample_sde_cfg(z2, cond, scales, steps, method, "sigma", 1.0, last, noise=noise)
    assert torch.isfinite(a).all() and torch.equal(a, b)
    assert torch.equal(a, m.sample_sde_cfg(z2, cond, scales, steps, method, "sigma", 1.0, last, seed=1234))
    c = m.sample_sde_cfg(z2, cond, scales, steps, method, "sigma", 1.0, last, seed=1235)
    assert not torch.equal(a, c) and max_abs_rel(a.cpu(), c.cpu()) > 1e-2
    d = m.sample_sde_cfg(z2, cond, scales, steps, method, "sigma", 1.0, last)        # seed=None: drawn from torch's host generator
    assert torch.isfinite(d).all() and not torch.equal(a, d)


def _noise(n_rows, e, seed, step, half=0, cell_offset=0, cells_total=None):
    from scldm_amd import _lib
    out = torch.empty(n_rows, e, device="cuda")
    _lib.check(_lib.lib().scldm_sde_noise(out.data_ptr(), n_rows, e, seed, step, half, cell_offset, n_rows + cell_offset if cells_total is None else cells_total,
                                          torch.cuda.current_stream().cuda_stream), "scldm_sde_noise")
    return out


def test_noise_moments_and_row_addressing():
    """n = 2^20 draws: five-sigma bounds of the sample mean, variance, excess kurtosis (standard errors 1 / sqrt n, sqrt(2 / n),
    sqrt(24 / n) for a normal sample) and of the lag-1, cross-step and cross-half correlations (1 / sqrt n); a value depends on its
    global row alone - a row range generated with `cell_offset` is the same rows of the full array."""
    rows, e, seed = 4096, 256, 0x5DE0C0FFEE
    n = rows * e
    assert n == 2 ** 20
    a = _noise(rows, e, seed, 0)
    assert torch.isfinite(a).all()
    x = a.double().flatten()
    mean, var = float(x.mean()), float(x.var(unbiased=False))
    kurt = float(((x - mean) ** 4).mean() / var ** 2 - 3.0)
    z = (x - mean) / math.sqrt(var)
    b = ((_noise(rows, e, seed, 1).double().flatten()) - 0.0)
    h1 = _noise(rows, e, seed, 0, half=1, cells_total=rows).double().flatten()
    lag1 = float((z[:-1] * z[1:]).mean())
    cross_step = float((z * (b - b.mean()) / b.std()).mean())
    cross_half = float((z * (h1 - h1.mean()) / h1.std()).mean())
    print(f"[noise] n = {n}: mean {mean:.3e} var-1 {var - 1:.3e} excess kurtosis {kurt:.3e} lag-1 {lag1:.3e} cross-step {cross_step:.3e} "
          f"cross-half {cross_half:.3e}   (5 sigma: {5 / math.sqrt(n):.3e}, {5 * math.sqrt(2 / n):.3e}, {5 * math.sqrt(24 / n):.3e})")
    assert abs(mean) < 5 / math.sqrt(n)
    assert abs(var - 1) < 5 * math.sqrt(2 / n)
    assert abs(kurt) < 5 * math.sqrt(24 / n)
    assert abs(lag1) < 5 / math.sqrt(n) and abs(cross_step) < 5 / math.sqrt(n) and abs(cross_half) < 5 / math.sqrt(n)
    assert not torch.equal(a, _noise(rows, e, seed + 1, 0))
    part = _noise(100, e, seed, 0, cell_offset=1000, cells_total=rows)
    assert torch.equal(part, a[1000:1100])
    odd = _noise(7, 12, seed, 3, half=1, cell_offset=5, cells_total=40)       # a narrow row (e = 12), second half, partial workgroup
    assert torch.equal(odd, _noise(40, 12, seed, 3, half=1, cells_total=40)[5:12])


@pytest.mark.parametrize("method,last", [("euler", "Mean"), ("heun", "Euler")])
def test_shards_of_a_solve_draw_the_whole_solves_noise(method, last):
    """B = 6 solved whole is bit-equal to two shards of 3 with cell_offset 0 / 3 and cells_total 6 (cells are independent, and the
    noise of a cell does not depend on the batch it is solved in) - through sampling.sample_latents, as a sharded caller passes it."""
    from scldm_amd.sampling import sample_latents
    g, m, cfg, sd = build("dit_base", "bf16")
    gen = torch.Generator().manual_seed(17)
    z0 = torch.randn(6, 16, 16, generator=gen).cuda()
    lab = {"clusters": torch.randint(0, 14, (6,), generator=gen).cuda()}
    scales = {"clusters": 1.5}
    opts = dict(diffusion_form="decreasing", diffusion_norm=0.5, last_step=last, seed=99)
    whole = sample_latents(m, z0, lab, scales, 4, method, sde=dict(opts))
    parts = [sample_latents(m, z0[lo:lo + 3], {"clusters": lab["clusters"][lo:lo + 3]}, scales, 4, method,
                            sde=dict(opts, cell_offset=lo, cells_total=6)) for lo in (0, 3)]
    assert whole.shape == (12, 16, 16) and torch.isfinite(whole).all()
    for i, lo in enumerate((0, 3)):
        assert torch.equal(parts[i][:3], whole[lo:lo + 3]) and torch.equal(parts[i][3:], whole[6 + lo:6 + lo + 3])
    alone = sample_latents(m, z0[3:], {"clusters": lab["clusters"][3:]}, scales, 4, method, sde=dict(opts))   # same cells, offset 0: other noise
    assert not torch.equal(alone, parts[1])
    assert torch.equal(sample_latents(m, z0, lab, scales, 4, method), m.sample_ode_cfg(torch.cat([z0, z0]), {"clusters": lab["clusters"].repeat(2)}, scales, 4, method))


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16", "fp16"])
def test_zero_diffusion_is_the_ode_sampler(precision):
    """diffusion_norm = 0 (no score, no noise), no last step, 5 grid points: the Euler solve of sample_ode_cfg.  Both sides share the trunk
    bits, so only the update's rounding differs."""
    g, m, cfg, sd = build("dit_base", precision)
    f, z2, cond, scales, _ = _inputs("sde_base_euler")
    a = m.sample_sde_cfg(z2, cond, scales, 5, "euler", "sigma", 0.0, None, seed=5)
    b = m.sample_ode_cfg(z2, cond, scales, 5, "euler")
    e = max_abs_rel(a.cpu(), b.cpu())
    print(f"[parity] zero-diffusion SDE vs ODE [{precision}]: {e:.3e}")
    assert torch.isfinite(a).all() and e < 1e-4


def test_plans(monkeypatch):
    """One cell; no condition (n_pass = 0); guidance exactly 1.0 with the direct option on vs off; whole-solve vs per-evaluation
    conditioning (bit-identical); the trajectory's last entry is the in-place result."""
    g, m, cfg, sd = build("dit_base", "fp32")
    f, z2, cond, scales, _ = _inputs("sde_base_euler")
    kw = dict(num_steps=4, sampling_method="heun", diffusion_form="linear", diffusion_norm=0.7, last_step="Mean", last_step_size=0.04, seed=7)
    # B = 1: rows 0 and 3 of the doubled state, as cell 0 of a 3-cell solve
    one = torch.cat([z2[:1], z2[3:4]])
    cond1 = {k: torch.cat([v[:1], v[3:4]]) for k, v in cond.items()}
    full = m.sample_sde_cfg(z2, cond, scales, **kw)
    a1 = m.sample_sde_cfg(one, cond1, scales, cells_total=3, **kw)
    assert torch.isfinite(a1).all() and torch.equal(a1[0], full[0]) and torch.equal(a1[1], full[3])
    # no condition: both halves run unconditionally on the same state - but on different noise rows
    u = m.sample_sde_cfg(z2, None, None, **kw)
    assert torch.isfinite(u).all() and torch.equal(u[:3], full[:3]) and not torch.equal(u[3:], u[:3])
    un = m.sample_sde_cfg(z2, None, None, **{**kw, "diffusion_norm": 0.0})
    assert torch.equal(un[3:], un[:3])
    # the trajectory's last entry is the returned state, its earlier entries the intermediate ones
    tr = m.sample_sde_cfg(z2, cond, scales, return_trajectory=True, **kw)
    assert tr.shape == (4, *z2.shape) and torch.equal(tr[-1], full) and not torch.equal(tr[-2], full)
    # guidance 1.0: the direct plan (no blend: the conditional output IS the guided row) against the blended one
    ones = {k: 1.0 for k in scales}
    base = m.sample_sde_cfg(z2, cond, ones, **kw)
    m.guidance1_direct = True
    fast = m.sample_sde_cfg(z2, cond, ones, **kw)
    m.guidance1_direct = False
    assert torch.equal(fast[:3], base[:3]) and max_abs_rel(fast.cpu(), base.cpu()) < 1e-4
    # per-evaluation conditioning (SCLDM_COND_ALL=0, read when the native handle is created) against the whole-solve pass
    monkeypatch.setenv("SCLDM_COND_ALL", "0")
    _, m0, _, _ = build("dit_base", "fp32")
    m0._native_handle()
    monkeypatch.delenv("SCLDM_COND_ALL")
    for k2 in (kw, {**kw, "sampling_method": "euler", "last_step": None}):
        assert torch.equal(m0.sample_sde_cfg(z2, cond, scales, **k2), m.sample_sde_cfg(z2, cond, scales, **k2))


def test_rejected_arguments_launch_nothing():
    from scldm_amd import _lib
    g, m, cfg, sd = build("dit_base", "fp32")
    f, z2, cond, scales, _ = _inputs("sde_base_euler")
    with pytest.raises(ValueError, match="sigma"):
        m.sample_sde_cfg(z2, cond, scales, 4, "euler", "SBDM")
    with pytest.raises(ValueError, match="Mean"):
        m.sample_sde_cfg(z2, cond, scales, 4, "heun", "sigma", 1.0, None)
    with pytest.raises(NotImplementedError):
        m.sample_sde_cfg(z2, cond, scales, 4, "rk4", "sigma")
    with pytest.raises(NotImplementedError):
        m.sample_sde_cfg(z2, cond, scales, 4, "euler", "quadratic")
    with pytest.raises(NotImplementedError):
        m.sample_sde_cfg(z2, cond, scales, 4, "euler", "sigma", 1.0, "Median")
    with pytest.raises(ValueError):
        m.sample_sde_cfg(z2, cond, scales, 4, "euler", "sigma", cell_offset=2, cells_total=4)
    # the C ABI itself: every rejected call returns SCLDM_ERR_SHAPE with a message and leaves the state untouched
    L, h = m._native()
    before = z2.clone()
    ws = m._workspace(L, 6, 1, 6)
    st = torch.cuda.current_stream().cuda_stream

    def call(z=None, num_steps=4, method=0, form=0, last=1, lss=0.04, cell_offset=0, cells_total=3):
        return L.scldm_sample_sde(h, before.data_ptr() if z is None else z, None, 0, None, 3, 0, None, None, num_steps, method, form, 1.0, last, lss,
                                  None, 1, cell_offset, cells_total, None, 0, ws, st)

    for what, rc in (("null z", call(z=0)), ("SBDM", call(form=_lib.SDE_FORMS["SBDM"])), ("heun without last step", call(method=1, last=0)),
                     ("one grid point", call(num_steps=1)), ("last_step_size 1", call(lss=1.0)), ("negative last_step_size", call(lss=-0.1)),
                     ("cells_total too small", call(cell_offset=1, cells_total=3)), ("unknown form", call(form=9)), ("unknown method", call(method=2)),
                     ("Mean at t = 1", call(lss=0.0))):
        assert rc == -1 and L.scldm_last_error(), what
    torch.cuda.synchronize()
    assert torch.equal(before, z2)
    assert call() == 0      # the same call with valid arguments runs
    torch.cuda.synchronize()
    assert torch.isfinite(before).all() and not torch.equal(before, z2)

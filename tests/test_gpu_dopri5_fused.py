"""GPU tests of the fused adaptive sampler (DiT.sample_ode_cfg(..., "dopri5") -> scldm_sample_ode_dopri5) against the host-composed route
(Sampler._sample_dopri5 over DiT.forward_with_cfg), which tests/test_gpu_dit.py pins to the float64 oracle.  Started from the same first
step the two routes perform the same fp32 operations in the same order and take their decisions from the same doubles, so everything
is compared bit for bit: the 50-point trajectory, the final state, the accepted / rejected (t0, dt) lists and the evaluation count.
Only the automatic first step is tolerance-close: it comes from three sums of non-negative doubles whose ORDER differs between the routes."""
import pytest
import torch

from conftest import check_err, golden_json
from test_gpu_dit import TOL_FP32, build

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _fused_route_on(monkeypatch):
    monkeypatch.setenv("SCLDM_DOPRI5_FUSED", "1")     # read when a module's native handle is created


def _composed(m, z2, cond, scales, num_steps, tol, first_step=None):
    """(trajectory, stats) of the host-composed route on the same module."""
    from scldm_amd.transport import Sampler, create_transport
    fn = Sampler(create_transport())._sample_dopri5(num_steps, tol, tol, first_step)
    traj = fn(z2, m.forward_with_cfg, condition=cond, cfg_scale=scales)
    return traj, fn.last_stats


def _first_dt(st):
    return sorted(st["accepted_steps"] + st["rejected_steps"])[0][1]


def _inputs(m, g, B, case, seed):
    gen = torch.Generator().manual_seed(seed)
    z0 = torch.randn(B, m.seq_len, m.n_embed_input, generator=gen)
    z2 = torch.cat([z0, z0]).cuda()
    if case == "none":
        return z2, None, None
    if case == "few_labels":       # 3 distinct labels among B cells: de-duplicated rows (n_urows < B) behind a cell_row map
        lab = torch.randint(0, 3, (B,), generator=gen)
        return z2, {"clusters": lab.repeat(2).cuda()}, {"clusters": 2.0}
    cond = {k: torch.randint(0, v, (B,), generator=gen).repeat(2).cuda() for k, v in m.class_vocab_sizes.items()}
    scales = {"clusters": 2.0} if case == "scale2" else golden_json(g, "cfg_scales_s2")
    return z2, cond, scales


def _three_way(m, z2, cond, scales, tol):
    """Composed route (automatic first step) -> its first attempted dt -> fused and composed route from that dt."""
    _, st0 = _composed(m, z2, cond, scales, 50, tol)
    dt0 = _first_dt(st0)
    new = m.sample_ode_cfg(z2, cond, scales, 50, "dopri5", tol, tol, first_step=dt0, return_trajectory=True)
    st_new = dict(m.last_solver_stats)
    ref, st_ref = _composed(m, z2, cond, scales, 50, tol, first_step=dt0)
    return dt0, new, st_new, ref, st_ref


def _assert_identical(new, st_new, ref, st_ref, what):
    print(f"[dopri5 fused] {what}: {len(st_ref['accepted_steps'])} accepted / {len(st_ref['rejected_steps'])} rejected, "
          f"{st_ref['evaluations']} evaluations; fused {len(st_new['accepted_steps'])} / {len(st_new['rejected_steps'])}, {st_new['evaluations']}; "
          f"max |fused - composed| = {float((new - ref).abs().max()):.3e}")
    assert new.shape == ref.shape and torch.isfinite(new).all()
    assert st_new["accepted_steps"] == st_ref["accepted_steps"], what
    assert st_new["rejected_steps"] == st_ref["rejected_steps"], what
    assert st_new["evaluations"] == st_ref["evaluations"] and st_new["rejected"] == st_ref["rejected"], what
    assert torch.equal(new[-1], ref[-1]), f"{what}: final state differs"
    assert torch.equal(new, ref), f"{what}: trajectory differs"


CASES = [  # fixture, cells, conditioning, precision, tolerance
    ("dit_base", 4, "scale2", "fp32", 1e-5), ("dit_base", 4, "scale2", "fp32", 1e-7),
    ("dit_base", 4, "scale2", "bf16", 1e-5), ("dit_base", 4, "scale2", "bf16", 1e-7),
    ("dit_joint", 4, "golden", "fp32", 1e-5),          # one joint pass over two classes
    ("dit_me2_256", 4, "golden", "fp32", 1e-5),        # two mutually-exclusive passes
    ("dit_base", 4, "none", "fp32", 1e-5),             # no conditional pass at all
    ("dit_base", 37, "few_labels", "bf16", 1e-5),      # n_urows < B, cell_row map, partial last tile
]


@pytest.mark.parametrize("name,B,case,precision,tol", CASES, ids=[f"{c[0]}-B{c[1]}-{c[2]}-{c[3]}-{c[4]:g}" for c in CASES])
def test_fused_solve_is_bit_identical_to_the_composed_route(name, B, case, precision, tol):
    g, m, cfg, sd = build(name, precision)
    z2, cond, scales = _inputs(m, g, B, case, 40 + B)
    dt0, new, st_new, ref, st_ref = _three_way(m, z2, cond, scales, tol)
    assert st_new["first_step"] == dt0 and torch.equal(new[0], z2)
    _assert_identical(new, st_new, ref, st_ref, f"{name} B={B} {case} [{precision}] tol {tol:g}")


@pytest.fixture(scope="module")
def base():
    """dit_base, 4 cells, scale 2, fp32, the default tolerances: solved once for the harness / rejection tests below."""
    mp = pytest.MonkeyPatch()        # (a module-scoped fixture is set up before the function-scoped one above)
    mp.setenv("SCLDM_DOPRI5_FUSED", "1")
    try:
        g, m, cfg, sd = build("dit_base", "fp32")
        z2, cond, scales = _inputs(m, g, 4, "scale2", 44)
        dt0, new, st_new, ref, st_ref = _three_way(m, z2, cond, scales, 1e-5)
    finally:
        mp.undo()
    assert torch.equal(new, ref)
    return dict(m=m, z2=z2, cond=cond, scales=scales, dt0=dt0, traj=new.clone(), stats=st_new)


def test_automatic_first_step_and_trajectory_at_1e6(base):
    """first_step=None: the fused route forms the Hairer / Norsett / Wanner step from the same fp32 arrays through the same float64
    formula; the three rms norms are sums of 4 096 non-negative doubles added in another order (relative difference <= ~4096 x 2^-53 =
    5e-13 per norm), so the step agrees to 1e-9 and - at atol = rtol = 1e-6, where the solver's own error is below the parity gate -
    the trajectories to the gate of the oracle test."""
    m, z2, cond, scales = base["m"], base["z2"], base["cond"], base["scales"]
    ref, st_ref = _composed(m, z2, cond, scales, 50, 1e-6)
    new = m.sample_ode_cfg(z2, cond, scales, 50, "dopri5", 1e-6, 1e-6, return_trajectory=True)
    st = m.last_solver_stats
    h_ref = _first_dt(st_ref)
    print(f"[dopri5 fused] automatic first step: fused {st['first_step']!r}, composed {h_ref!r} (relative difference {abs(st['first_step'] - h_ref) / h_ref:.3e}); "
          f"evaluations {st['evaluations']} / {st_ref['evaluations']}")
    assert abs(st["first_step"] - h_ref) <= 1e-9 * h_ref
    assert _first_dt(st) == st["first_step"]
    check_err(new.cpu(), ref.cpu(), TOL_FP32, "dopri5 fused vs composed trajectory, automatic first step, atol = rtol = 1e-6", 5e-3)


def test_save_points_do_not_move_the_steps_and_the_harness_reaches_the_fused_route(base):
    from scldm_amd.sampling import sample_latents
    m, z2, cond, scales, dt0 = base["m"], base["z2"], base["cond"], base["scales"], base["dt0"]
    end = m.sample_ode_cfg(z2, cond, scales, 2, "dopri5", first_step=dt0)
    assert end.shape == z2.shape and torch.equal(end, base["traj"][-1])          # same steps; only the save times differ
    assert m.last_solver_stats["accepted_steps"] == base["stats"]["accepted_steps"]
    tr = m.sample_ode_cfg(z2, cond, scales, 3, "dopri5", first_step=dt0, return_trajectory=True)
    assert tr.shape == (3, *z2.shape) and torch.equal(tr[0], z2) and torch.equal(tr[-1], end)
    m.last_solver_stats = None
    B = z2.shape[0] // 2
    out = sample_latents(m, z2[:B], {k: v[:B] for k, v in cond.items()}, scales, 2, sampling_method="dopri5", atol=1e-4, rtol=1e-4)
    st = m.last_solver_stats
    assert out.shape == z2.shape and st is not None and st["evaluations"] >= 7 and st["first_step"] > 0
    assert st["evaluations"] < base["stats"]["evaluations"] + 2                   # the looser tolerance arrived
    assert torch.isfinite(out).all()


def test_rejected_arguments_raise_and_leave_the_next_solve_intact(base):
    m, z2, cond, scales, dt0 = base["m"], base["z2"], base["cond"], base["scales"], base["dt0"]
    with pytest.raises(ValueError, match="num_save"):
        m.sample_ode_cfg(z2, cond, scales, 1, "dopri5", first_step=dt0)
    with pytest.raises(ValueError, match="atol"):
        m.sample_ode_cfg(z2, cond, scales, 2, "dopri5", atol=0.0, first_step=dt0)
    with pytest.raises(ValueError, match="expected z"):
        m.sample_ode_cfg(z2[:, :, :8].contiguous(), cond, scales, 2, "dopri5", first_step=dt0)
    with pytest.raises(ValueError, match="expected z"):
        m.sample_ode_cfg(z2[:7], {k: v[:7] for k, v in cond.items()}, scales, 2, "dopri5", first_step=dt0)
    assert torch.equal(m.sample_ode_cfg(z2, cond, scales, 2, "dopri5", first_step=dt0), base["traj"][-1])


def test_weights_are_read_live():
    """An in-place `.data` change (what an EMA swap does: no version counter moves) between two solves is seen by the second one."""
    g, m, cfg, sd = build("dit_base", "fp32")
    z2, cond, scales = _inputs(m, g, 4, "scale2", 51)
    h = 0.03125
    a = m.sample_ode_cfg(z2, cond, scales, 2, "dopri5", first_step=h)
    with torch.no_grad():
        p = [q for q in m.parameters() if q.dim() == 2 and q.shape[0] >= 256][2]
        p.data.mul_(1.25)
    b = m.sample_ode_cfg(z2, cond, scales, 2, "dopri5", first_step=h)
    st_b = dict(m.last_solver_stats)
    ref, st_ref = _composed(m, z2, cond, scales, 2, 1e-5, first_step=h)
    assert not torch.equal(a, b)
    assert torch.equal(b, ref[-1]) and st_b["accepted_steps"] == st_ref["accepted_steps"] and st_b["evaluations"] == st_ref["evaluations"]


def test_knob_restores_the_composed_route(monkeypatch):
    """SCLDM_DOPRI5_FUSED=0 (read when the native handle is created): the same call, the host-driven solve - and the same bits."""
    g, m, cfg, sd = build("dit_base", "fp32")
    z2, cond, scales = _inputs(m, g, 4, "scale2", 44)
    h = 0.03125
    fused = m.sample_ode_cfg(z2, cond, scales, 2, "dopri5", first_step=h)
    st_f = dict(m.last_solver_stats)
    monkeypatch.setenv("SCLDM_DOPRI5_FUSED", "0")
    g, m0, cfg, sd = build("dit_base", "fp32")
    calls = []
    orig = m0.forward_with_cfg
    m0.forward_with_cfg = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    comp = m0.sample_ode_cfg(z2, cond, scales, 2, "dopri5", first_step=h)
    st_c = m0.last_solver_stats
    assert len(calls) == st_c["evaluations"] > 0                  # the host-driven route ran
    assert torch.equal(fused, comp) and st_f["accepted_steps"] == st_c["accepted_steps"] and st_f["first_step"] == st_c["first_step"] == h

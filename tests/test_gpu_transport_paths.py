"""GPU tests of the wider transport family (GVP path, noise / score prediction, loss weights): the plan / weighted-loss kernels alone,
`Transport.training_losses` through the DiT, the fused training step under a transport, and the ODE samplers of noise / score models -
against the reference's own results (tests/golden/transport_paths_*.npz, tests/golden/make_golden_transport_paths.py) and the float64
restatement of tests/transport_paths_ref.py.  Gate: 1e-4 on max|a-b| / max|b| at fp32 (the project's); bit equality where two routes
of this project must agree."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import transport_paths_ref as R
from conftest import golden_json, load_golden, max_abs_rel
from scldm_amd import _lib

pytestmark = pytest.mark.gpu
TOL = 1e-4
F32 = dict(dtype=torch.float32, device="cuda")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _err(got, want, what):
    e = max_abs_rel(torch.as_tensor(got).detach().cpu(), want)
    print(f"[parity] {what}: max|a-b|/max|b| = {e:.3e}   tol {TOL:g}")
    return e


def _plan_loss(tr, x1, x0, t, pred, gloss):
    """scldm_fm_plan, scldm_fm_wloss, scldm_fm_wloss_bwd on (n, e) device tensors."""
    L = _lib.lib()
    n, e = x1.shape
    xt, tgt, dm = (torch.empty(n, e, **F32) for _ in range(3))
    rowc, loss = torch.empty(n, 2, **F32), torch.empty(n, **F32)
    cs = tr.c_struct()
    _lib.check(L.scldm_fm_plan(C.byref(cs), x1.data_ptr(), x0.data_ptr(), t.data_ptr(), xt.data_ptr(), tgt.data_ptr(), rowc.data_ptr(), n, e, _st()),
               "scldm_fm_plan")
    _lib.check(L.scldm_fm_wloss(pred.data_ptr(), tgt.data_ptr(), rowc.data_ptr(), loss.data_ptr(), n, e, _st()), "scldm_fm_wloss")
    _lib.check(L.scldm_fm_wloss_bwd(pred.data_ptr(), tgt.data_ptr(), rowc.data_ptr(), gloss.data_ptr(), dm.data_ptr(), n, e, _st()), "scldm_fm_wloss_bwd")
    return xt, tgt, rowc, loss, dm


@pytest.mark.parametrize("n", R.KERNEL_N)
@pytest.mark.parametrize("case", R.CASES, ids=lambda c: R.case_key(*c))
def test_plan_and_weighted_loss_kernels_against_the_reference(case, n):
    from scldm_amd.transport import create_transport
    g = load_golden("transport_paths_kernel")
    x1, x0, pred = (torch.from_numpy(g[k]).cuda().reshape(n, -1) for k in (f"n{n}_x1", f"n{n}_x0", f"n{n}_{case[0]}_pred"))
    t, gloss = torch.from_numpy(g[f"n{n}_t"]).cuda(), torch.from_numpy(g[f"n{n}_gloss"]).cuda()
    xt, tgt, rowc, loss, dm = _plan_loss(create_transport(*case), x1, x0, t, pred, gloss)
    key = R.case_key(*case)
    assert _err(xt, g[f"n{n}_{case[0]}_xt"].reshape(n, -1), f"{key} n={n} xt") < TOL
    want_tgt = {"velocity": g[f"n{n}_{case[0]}_ut"], "noise": g[f"n{n}_x0"], "score": -g[f"n{n}_x0"]}[case[1]].reshape(n, -1)
    assert _err(tgt, want_tgt, f"{key} n={n} tgt") < TOL
    assert _err(loss, g[f"n{n}_{key}_loss"], f"{key} n={n} loss") < TOL
    assert _err(dm, g[f"n{n}_{key}_dpred"].reshape(n, -1), f"{key} n={n} d pred") < TOL
    want_c = R.coef(*case, g[f"n{n}_t"])
    assert _err(rowc[:, 0], want_c["c"], f"{key} n={n} c") < TOL and _err(rowc[:, 1], want_c["w"], f"{key} n={n} w") < TOL


@pytest.mark.parametrize("case", [("GVP", "score", "velocity"), ("Linear", "noise", "likelihood"), ("GVP", "velocity", None)], ids=lambda c: R.case_key(*c))
@pytest.mark.parametrize("n,e", [(3, 12), (2, 1030)])
def test_plan_and_weighted_loss_kernels_at_other_row_lengths(case, n, e):
    """e = 12: less than a wave; e = 1030: a second, partial 1 024-element chunk of the plan kernel and a fifth pass of the loss kernel."""
    from scldm_amd.transport import create_transport
    rng = np.random.default_rng(7 + e)
    x1, x0, m = (rng.standard_normal((n, e)).astype(np.float32) for _ in range(3))
    t = rng.uniform(*R.T_RANGE, (n,)).astype(np.float32)
    gl = rng.uniform(0.1, 1.0, (n,)).astype(np.float32)
    got = _plan_loss(create_transport(*case), *(torch.from_numpy(v).cuda() for v in (x1, x0, t, m, gl)))
    want = R.plan_loss_ref(*case, x1, x0, t, m, gl)
    for name, a, b in zip(("xt", "tgt", "rowc", "loss", "d pred"), got, want):
        assert _err(a, b, f"{R.case_key(*case)} e={e} {name}") < TOL


# ---------------------------------------------------------------------------------------------------------------- through the DiT
_MODEL = {}


def _train_model():
    from test_gpu_train import build
    if "m" not in _MODEL:
        g = load_golden("transport_paths_train")
        kw = golden_json(g, "kwargs_json")
        m, _, _ = build(kw["class_vocab_sizes"], kw["condition_strategy"], kw["n_layer"], int(g["seed"]))
        m.precision = "fp32"
        _MODEL["m"], _MODEL["g"], _MODEL["kw"] = m, g, kw
    return _MODEL["m"], _MODEL["g"], _MODEL["kw"]


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: R.case_key(*c))
def test_training_losses_through_the_dit(case):
    """loss and pred of every case, and for one weight per (path, prediction) every parameter gradient, against the reference's autograd."""
    from scldm_amd.transport import create_transport
    from test_gpu_train import FROZEN, grad_digest
    m, g, kw = _train_model()
    tr = create_transport(*case)
    t, x0 = torch.from_numpy(g["t"]).cuda(), torch.from_numpy(g["x0"]).cuda()
    tr.sample = lambda x1_: (t, x0, x1_)
    for p in m.parameters():
        p.grad = None
    cond = {k: torch.from_numpy(g[f"label_{k}"]).cuda() for k in kw["class_vocab_sizes"]}
    terms = tr.training_losses(lambda xt, tt, **k: m(xt, tt, k["condition"], force_drop_ids=False), torch.from_numpy(g["x1"]).cuda(), {"condition": cond})
    key = R.case_key(*case)
    assert terms["loss"].grad_fn is not None and type(terms["loss"].grad_fn).__name__.startswith("_WeightedFlowMatchLoss")   # the HIP route
    assert _err(terms["pred"], g[f"pred_{case[0]}"], f"{key} pred") < TOL
    assert _err(terms["loss"], g[f"loss_{key}"], f"{key} loss") < TOL
    if case not in R.GRAD_CASES:
        return
    terms["loss"].mean().backward()
    assert golden_json(g, "frozen_json") == list(FROZEN)
    worst = 0.0
    for name, p in m.named_parameters():
        if name in FROZEN:
            assert p.grad is None
            continue
        ref = g[f"grad_{key}_{name}"]
        ours = grad_digest(p.grad)
        scale = max(np.abs(ref[2:]).max(), ref[1] / np.sqrt(p.numel()))
        worst = max(worst, np.abs(ours[2:] - ref[2:]).max() / scale, abs(ours[1] - ref[1]) / ref[1])
        assert np.abs(ours[2:] - ref[2:]).max() <= TOL * scale, name
        assert abs(ours[1] - ref[1]) <= TOL * ref[1] + 1e-12, name
    print(f"[parity] {key} parameter gradients: worst {worst:.3e}   tol {TOL:g}")


# ---------------------------------------------------------------------------------------------------------------- fused step
def _prepare(entry_tr, x1, labels, nulls, strategy, p_drop, rng):
    """scldm_fm_prepare (entry_tr None) or scldm_fm_prepare_transport on the same arguments: t, x0, xt, ut | tgt, rowc, labels."""
    L = _lib.lib()
    n, e = x1.shape[0], x1[0].numel()
    t, x0, xt, ut = torch.empty(n, **F32), torch.empty(n, e, **F32), torch.empty(n, e, **F32), torch.empty(n, e, **F32)
    rowc = torch.empty(n, 2, **F32)
    out = torch.empty(len(labels), n, dtype=torch.long, device="cuda")
    ptrs = _lib.ptr_array([l.data_ptr() for l in labels])
    nl = (C.c_int * len(labels))(*nulls)
    head = (x1.data_ptr(), C.cast(ptrs, _lib.c_void_pp), nl, len(labels), strategy, 1, p_drop, rng.data_ptr(), n, e, t.data_ptr(), x0.data_ptr(), xt.data_ptr(),
            ut.data_ptr())
    if entry_tr is None:
        _lib.check(L.scldm_fm_prepare(*head, out.data_ptr(), _st()), "scldm_fm_prepare")
    else:
        cs = entry_tr.c_struct()
        _lib.check(L.scldm_fm_prepare_transport(C.byref(cs), *head, rowc.data_ptr(), out.data_ptr(), _st()), "scldm_fm_prepare_transport")
    return t, x0, xt, ut, rowc, out


@pytest.mark.parametrize("n", [8, 33])
@pytest.mark.parametrize("case", [("GVP", "noise", "likelihood"), ("Linear", "score", "velocity")], ids=lambda c: R.case_key(*c))
def test_fused_step_under_a_transport_equals_the_unfused_route(case, n):
    """scldm_dit_train_step_transport (bf16): its t is the uniform scldm_fm_prepare draws for the same seed / counter mapped by
    u (t1 - t0) + t0, bit for bit and inside the interval; its plan is scldm_fm_plan's on the (t, x0) it drew; its row losses and its flat
    gradient buffer are those of scldm_fm_plan -> train forward -> scldm_fm_wloss / _bwd -> train backward, bit for bit.  (The mean over
    rows is formed in a fixed order by the fused kernel and by torch.mean on the other route: 2e-6, as test_gpu_train_step.)"""
    from scldm_amd.optim import AdamW
    from scldm_amd.training import FusedTrainStep
    from scldm_amd.transport import _WeightedFlowMatchLoss, create_transport
    from test_gpu_train import build
    vocab = {"cell_line": 4, "gene": 2024}
    m1, _, _ = build(vocab, "joint", 2, 31)
    m1.precision = "bf16"
    m1.cfg_dropout_prob = 0.6
    m2 = copy.deepcopy(m1)
    tr = create_transport(*case)
    gen = torch.Generator(device="cuda").manual_seed(4 + n)
    x1 = torch.randn(n, 16, 16, device="cuda", generator=gen)
    cond = {k: torch.randint(0, v, (n,), device="cuda", generator=gen) for k, v in vocab.items()}
    opt = AdamW([p for p in m1.parameters() if p.requires_grad], lr=1e-3, weight_decay=0.01)
    f1 = FusedTrainStep(m1, tr, opt, n, list(vocab), seed=99, graph=False)
    assert f1.rowc is not None
    loss1 = f1(x1, cond).clone()
    assert int(f1.rng[1]) == 1
    # the draws: the same Philox calls as the default entry, at the counter the step started from
    rng0 = torch.tensor([99, 0], dtype=torch.int64, device="cuda")
    labs = [cond[c] for c in m1._class_names]
    nulls = [vocab[c] for c in m1._class_names]
    u, x0_d, _, _, _, lab_d = _prepare(None, x1, labs, nulls, 1, 0.6, rng0)
    t, x0, xt, tgt, rowc, lab = _prepare(tr, x1, labs, nulls, 1, 0.6, rng0)
    eps = float(np.float32(tr.train_eps))
    t0, t1 = eps, 1.0 - eps
    assert torch.equal(t, u * (t1 - t0) + t0) and torch.equal(f1.t, t)
    assert float(t.min()) >= t0 and float(t.max()) <= t1
    assert torch.equal(x0, x0_d) and torch.equal(lab, lab_d) and torch.equal(f1.labels, lab)
    assert torch.equal(f1.xt, xt) and torch.equal(f1.ut, tgt) and torch.equal(f1.rowc, rowc)
    # the plan kernel on the reported (t, x0)
    xt_p, tgt_p, rowc_p, _, _ = _plan_loss(tr, x1.view(n, -1), x0, t, xt, torch.ones(n, **F32))
    for name, a, b in (("xt", xt_p, xt), ("tgt", tgt_p, tgt), ("rowc", rowc_p, rowc)):
        print(f"[bits] plan kernel vs fused preparation, {name}: {int((a != b).sum())} of {a.numel()} differ, max |a-b| {float((a - b).abs().max()):.3e}")
    assert torch.equal(xt_p, xt) and torch.equal(tgt_p, tgt) and torch.equal(rowc_p, rowc)
    # the unfused route on the same plan (labels already dropped: no second mask)
    m2.cfg_dropout_prob = 0.0
    pred = m2(xt.view(n, 16, 16), t, {c: lab[i] for i, c in enumerate(m2._class_names)}, force_drop_ids=False)
    rows = _WeightedFlowMatchLoss.apply(pred.view(n, -1), tgt, rowc)
    rows.mean().backward()
    assert torch.equal(f1.loss_rows, rows.detach())
    assert abs(float(loss1) - float(rows.mean())) <= 2e-6 * abs(float(rows.mean()))
    offs = m1._grad_offsets
    checked = 0
    for (k, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        if p2.grad is None:
            continue
        assert torch.equal(f1.flat[offs[id(p1)]:offs[id(p1)] + p1.numel()].view(p1.shape), p2.grad), k
        checked += 1
    assert checked > 10


def test_fused_step_under_a_transport_replays_as_a_graph():
    from scldm_amd.optim import AdamW
    from scldm_amd.training import FusedTrainStep
    from scldm_amd.transport import create_transport
    from test_gpu_train import build
    vocab, n = {"cell_line": 4, "gene": 2024}, 24
    m, _, _ = build(vocab, "joint", 2, 33)
    m.precision = "bf16"
    m.cfg_dropout_prob = 0.5
    m_eager = copy.deepcopy(m)
    tr = create_transport("GVP", "noise", "likelihood")
    gen = torch.Generator(device="cuda").manual_seed(6)
    batches = [(torch.randn(n, 16, 16, device="cuda", generator=gen), {k: torch.randint(0, v, (n,), device="cuda", generator=gen) for k, v in vocab.items()})
               for _ in range(2)]
    out = {}
    for name, mod, graph in (("graph", m, True), ("eager", m_eager, False)):
        opt = AdamW([p for p in mod.parameters() if p.requires_grad], lr=1e-3, weight_decay=0.01)
        fs = FusedTrainStep(mod, tr, opt, n, list(vocab), seed=7, graph=graph)
        assert (fs.graph is not None) == graph
        losses = [float(fs(*b)) for b in batches]
        assert int(fs.rng[1]) == 2 and float(opt.param_groups[0]["_step_t"]) == 2.0
        assert all(np.isfinite(losses)) and losses[0] != losses[1]
        out[name] = (losses, [p.detach().clone() for p in mod.parameters()])
        with pytest.raises(NotImplementedError):
            fs.profile_stages()
    assert out["graph"][0] == out["eager"][0]
    for a, b in zip(out["graph"][1], out["eager"][1]):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------- samplers
def _solver_inputs(name):
    from scldm_amd.transport import create_transport
    from test_gpu_dit import build
    dit_name, B, _, path_type, prediction, method, steps = R.SOLVER_CASES[name]
    g = load_golden("transport_paths_solver")
    _, m, _, _ = build(dit_name, "fp32")
    names = sorted(golden_json(load_golden(dit_name), "kwargs_json")["class_vocab_sizes"])
    z0 = torch.from_numpy(g[f"{name}_z0"]).cuda()
    cond2 = {k: torch.from_numpy(np.concatenate([g[f"{name}_label_{k}"]] * 2)).cuda() for k in names}
    scales = golden_json(g, f"{name}_scales_json")
    return g, m, torch.cat([z0, z0]), cond2, scales, create_transport(path_type, prediction), method, steps


@pytest.mark.parametrize("name", list(R.SOLVER_CASES))
def test_one_call_and_host_driven_solves_against_the_float64_end_state(name):
    """sample_ode_cfg(..., transport=) at fp32 (scldm_sample_ode_transport) and the host-driven Sampler(tr).sample_ode over forward_with_cfg,
    both against the float64 end state of the reference's drift over the reference DiT."""
    from scldm_amd.transport import Sampler
    g, m, z2, cond2, scales, tr, method, steps = _solver_inputs(name)
    direct = name.startswith("base_direct")
    m.guidance1_direct = direct
    seen = []
    want = g[f"{name}_end64"]
    got = m.sample_ode_cfg(z2, cond2, scales, steps, method, transport=tr)
    assert got.shape == z2.shape and torch.isfinite(got).all()
    assert _err(got, want, f"{name} one call") < TOL
    fn = Sampler(tr).sample_ode(sampling_method=method, num_steps=steps)

    def fwd(x, t, **kw):
        seen.append(float(t[0]))
        return m.forward_with_cfg(x, t, **kw)

    host = fn(z2, fwd, condition=cond2, cfg_scale=scales)[-1]
    assert _err(host, want, f"{name} host driven") < TOL
    assert _err(got, host.cpu(), f"{name} one call vs host driven") < TOL
    ts = [float(v) for v in g[f"{name}_ts"]]
    assert seen == (ts[:-1] if method == "euler" else [v for i in range(steps - 1) for v in (ts[i], ts[i + 1])])
    # training mode takes the host-driven route through the same public call
    if not direct:
        m.train()
        try:
            again = m.sample_ode_cfg(z2, cond2, scales, steps, method, transport=tr)
        finally:
            m.eval()
        assert _err(again, want, f"{name} training mode") < TOL


def test_velocity_transports_are_the_plain_solve_bit_for_bit():
    from scldm_amd.sampling import sample_latents
    from scldm_amd.transport import create_transport
    g, m, z2, cond2, scales, _, _, _ = _solver_inputs("me2_euler9_linear_noise")
    for method in ("euler", "heun"):
        plain = m.sample_ode_cfg(z2, cond2, scales, 5, method)
        for tr in (create_transport(), create_transport("GVP"), create_transport("GVP", "velocity", "likelihood")):
            assert torch.equal(m.sample_ode_cfg(z2, cond2, scales, 5, method, transport=tr), plain)
    B = z2.shape[0] // 2
    cond = {k: v[:B] for k, v in cond2.items()}
    assert torch.equal(sample_latents(m, z2[:B], cond, scales, 5, "euler", transport=create_transport("GVP")), m.sample_ode_cfg(z2, cond2, scales, 5, "euler"))
    tr = create_transport("Linear", "noise")
    assert torch.equal(sample_latents(m, z2[:B], cond, scales, 5, "euler", transport=tr), m.sample_ode_cfg(z2, cond2, scales, 5, "euler", transport=tr))
    # the C entry hands a velocity model to the plain solve itself
    z = z2.clone()
    ul, n_u, cell_row, n_pass, masks, sc, keep = m._cfg_plan(cond2, scales, B, dedup=True)
    L, h = m._native()
    ws = m._workspace(L, 2 * B + n_pass * B, 1 + n_pass * n_u, 2 * B)
    cs = create_transport("GVP").c_struct()
    _lib.check(L.scldm_sample_ode_transport(h, z.data_ptr(), C.cast(ul, _lib.c_void_pp), n_u, cell_row, B, n_pass, masks, sc, 4, 0, C.byref(cs),
                                            m._prec(), ws, _st()), "scldm_sample_ode_transport")
    assert torch.equal(z, m.sample_ode_cfg(z2, cond2, scales, 5, "euler"))


def test_dopri5_under_a_noise_transport_is_the_host_driven_solve():
    """No one-call dopri5 exists for noise / score models: the public call runs Sampler(tr)._sample_dopri5 over forward_with_cfg - the same
    operations in the same order, so the same bits - over [sample_eps, 1 - sample_eps]."""
    from scldm_amd.transport import Sampler
    g, m, z2, cond2, scales, tr, _, _ = _solver_inputs("me2_euler9_linear_noise")
    a = m.sample_ode_cfg(z2, cond2, scales, 2, "dopri5", atol=1e-3, rtol=1e-3, transport=tr)
    fn = Sampler(tr)._sample_dopri5(2, 1e-3, 1e-3)
    b = fn(z2, m.forward_with_cfg, condition=cond2, cfg_scale=scales)[-1]
    assert torch.isfinite(a).all() and torch.equal(a, b)
    steps = fn.last_stats["accepted_steps"]
    assert abs(steps[0][0] - 1e-3) < 1e-9 and steps[-1][0] + steps[-1][1] >= 1 - 1e-3 - 1e-6


def test_refused_combinations_raise():
    from scldm_amd.sampling import sample_latents
    from scldm_amd.transport import Sampler, create_transport
    g, m, z2, cond2, scales, tr, _, _ = _solver_inputs("me2_euler9_linear_noise")
    B = z2.shape[0] // 2
    for bad in (tr, create_transport("GVP"), create_transport("GVP", "score", "likelihood")):
        with pytest.raises(NotImplementedError):
            m.sample_sde_cfg(z2, cond2, scales, 4, "euler", transport=bad)
        with pytest.raises(NotImplementedError):
            Sampler(bad).sample_ode_likelihood(sampling_method="euler", num_steps=4)
        with pytest.raises(NotImplementedError):
            sample_latents(m, z2[:B], {k: v[:B] for k, v in cond2.items()}, scales, 4, "euler", sde={}, transport=bad)
    with pytest.raises(NotImplementedError):
        create_transport("VP", "noise")
    with pytest.raises(ValueError):
        m.sample_ode_cfg(z2, cond2, scales, 5, "euler", transport=tr, return_trajectory=True)
    # a noise / score model with sample_eps = 0 has a singular drift at both ends: refused by the entry, nothing launched
    zero = create_transport("Linear", "noise", None, 1e-3, 0.0)
    with pytest.raises(_lib.ScldmError, match="sample_eps"):
        m.sample_ode_cfg(z2, cond2, scales, 5, "euler", transport=zero)

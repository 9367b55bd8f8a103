"""GPU tests of the adaptive log-likelihood solve (DiT.log_likelihood_cfg(..., "dopri5") -> scldm_logp_ode_dopri5): replayed bit for bit
from its own step log through DiT.input_vjp / DiT.logp_probe and torch arithmetic in the kernels' operation order, against the float64
restatement (tests/logp_dopri5_ref.py over the float64 oracle), against the generic `Sampler.sample_ode_likelihood("dopri5")` in the
16-bit classes, and itself across seeds, refusals and a weight change."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import logp_dopri5_ref
import logp_ref
from conftest import golden_json, max_abs_rel
from test_gpu_dit import PARITY, build
from test_gpu_logp import _fma, _row_sum_fixed

pytestmark = pytest.mark.gpu
f32 = np.float32


def _two_layer(n_embed_input, precision):
    """A two-layer model of the fused family at an input width the golden fixtures do not have."""
    from scldm_amd.nnets import DiT
    m = DiT(n_embed=256, n_embed_input=n_embed_input, n_layer=2, n_head=8, seq_len=16, dropout=0.0, bias=True, norm_layer="layernorm",
            multiple_of=4, layernorm_eps=1e-8, class_vocab_sizes={"clusters": 14}, cfg_dropout_prob=0.8)
    gen = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn(p.shape, generator=gen) * 0.05)
    m = m.cuda().eval()
    m.precision = precision
    return m


def _inputs(m, g, B, case, seed):
    gen = torch.Generator().manual_seed(seed)
    z0 = torch.randn(B, m.seq_len, m.n_embed_input, generator=gen)
    z2 = torch.cat([z0, z0]).cuda()
    probe = (torch.randint(2, z2.shape, generator=gen) * 2 - 1).float().cuda()
    if case == "none":
        return z2, None, None, probe
    if case == "few_labels":       # 3 distinct labels among B cells: de-duplicated rows (n_urows < B) behind a cell_row map
        return z2, {"clusters": torch.randint(0, 3, (B,), generator=gen).repeat(2).cuda()}, {"clusters": 2.0}, probe
    cond = {k: torch.randint(0, v, (B,), generator=gen).repeat(2).cuda() for k, v in m.class_vocab_sizes.items()}
    scales = {"clusters": 1.5} if case == "scale1.5" else golden_json(g, "cfg_scales_s2")
    return z2, cond, scales, probe


# ---------------------------------------------------------------------------------------------------------------- replay
def _plan(t0, h):
    from scldm_amd import _lib
    p = _lib.Dopri5Plan()
    _lib.lib().scldm_dopri5_stage_plan(float(t0), float(h), C.byref(p))
    return p


def _weights(w, mask):
    return [(j, float(w[j])) for j in range(7) if (mask >> j) & 1]


class _Replay:
    """The solve's evaluation and state arithmetic in torch, in the kernels' operation order (every product and sum rounded on its own in
    fp32; the CFG blend's fma formed in float64)."""

    def __init__(self, m, z2, cond, scales, probe_of, atol, rtol):
        self.m, self.B, self.e = m, z2.shape[0] // 2, m.seq_len * m.n_embed_input
        self.shape = z2.shape
        names = sorted(m.class_vocab_sizes)
        B = self.B
        if cond is None:
            passes = []
        elif m.condition_strategy == "joint":
            passes = [(f32(sum(scales.values()) / len(scales)), {c: cond[c][B:] for c in names})]
        else:
            passes = [(f32(scales[c]), {c: cond[c][B:]}) for c in scales]
        self.scales = [s for s, _ in passes]
        coef_u = f32(1)
        for s in self.scales:
            coef_u = f32(coef_u - s)
        self.coefs = [1.0, float(coef_u)] + [float(s) for s in self.scales]
        # per-row labels of the (2 + P) B forward rows: the null token (= the vocabulary size) wherever a class is not conditioned on
        self.labels = {}
        for c in names:
            null = torch.full((B,), m.class_vocab_sizes[c], device="cuda", dtype=torch.long)
            self.labels[c] = torch.cat([null, null] + [lab[c].long() if c in lab else null for _, lab in passes])
        self.probe_of, self.n_eval = probe_of, 0
        self.atol, self.rtol = float(f32(atol)), float(f32(rtol))

    def evaluate(self, x, s):
        """(-v (2B,S,C), logp_grad (2B)) at the fp32 solver time s; advances the evaluation index."""
        m, B = self.m, self.B
        ep = self.probe_of(self.n_eval)
        self.n_eval += 1
        P = len(self.scales)
        xin = torch.cat([x] + [x[B:]] * P)
        dout = torch.cat([ep[:B] * self.coefs[0], ep[B:] * self.coefs[1]] + [ep[B:] * self.coefs[2 + p] for p in range(P)])
        tv = torch.full((xin.shape[0],), float(f32(1) - f32(s)), device="cuda")
        strategy = m.condition_strategy
        m.condition_strategy = "joint"      # every class as given (the null tokens are explicit): no class is drawn
        try:
            out, dx = m.input_vjp(xin, tv, self.labels, dout)
        finally:
            m.condition_strategy = strategy
        u = out[B:2 * B]
        v2, d2 = u, dx[B:2 * B]
        for p, sc in enumerate(self.scales):
            v2 = _fma(sc, out[(2 + p) * B:(3 + p) * B] - u, v2)
            d2 = d2 + dx[(2 + p) * B:(3 + p) * B]
        v, d = torch.cat([out[:B], v2]), torch.cat([dx[:B], d2])
        return -v, _row_sum_fixed((ep * d).reshape(2 * B, self.e))

    @staticmethod
    def combine(y0, ks, weights):
        acc = y0
        for j, c in weights:
            acc = acc + ks[j] * c
        return acc

    @staticmethod
    def err_sum(ks, weights):
        acc = None
        for j, c in weights:
            t = ks[j] * c
            acc = t if acc is None else acc + t
        return acc

    def sq_sum(self, num, y0, y1=None):
        """sum((num / (atol + rtol max(|y0|, |y1|)))^2) in float64 of fp32 quotients (the fp32 division through float64: a correctly
        rounded quotient, as the kernels')."""
        ref = y0.abs() if y1 is None else torch.maximum(y0.abs(), y1.abs())
        den = self.atol + self.rtol * ref
        q = (num.double() / den.double()).float().double()
        return float((q * q).sum())

    def attempt(self, t0, h, y0, l0, kx0, kl0):
        """One attempted step from (t0, y0, l0) with first slopes (kx0, kl0): (y1, l1, the seven slope pairs, the error ratio, the plan)."""
        p = _plan(t0, h)
        kx, kl = [kx0], [kl0]
        for i in range(6):
            w = _weights(p.a[i], p.a_mask[i])
            yx, yl = self.combine(y0, kx, w), self.combine(l0, kl, w)
            a, b = self.evaluate(yx, p.t_stage[i])
            kx.append(a)
            kl.append(b)
        w = _weights(p.err, p.err_mask)
        total = self.sq_sum(self.err_sum(kx, w), y0, yx) + self.sq_sum(self.err_sum(kl, w), l0, yl)
        return yx, yl, kx, kl, (total / (2 * self.B * (self.e + 1))) ** 0.5, p

    def interpolate(self, p, s, y0, y1, ks):
        ym = self.combine(y0, ks, _weights(p.mid, p.mid_mask))
        fa, fb, h, two_h = ks[0], ks[6], float(p.h), float(p.two_h)
        c1 = h * fa
        c2 = ((h * (fb - 4.0 * fa) - 11.0 * y0) - 5.0 * y1) + 16.0 * ym
        c3 = ((h * (5.0 * fa - 3.0 * fb) + 18.0 * y0) + 14.0 * y1) - 32.0 * ym
        c4 = (two_h * (fb - fa) - 8.0 * (y1 + y0)) + 16.0 * ym
        s1, s2, s3, s4 = float(f32(s)), float(f32(s * s)), float(f32(s * s * s)), float(f32(s * s * s * s))
        t = y0 + c1 * s1
        t = t + c2 * s2
        t = t + c3 * s3
        return t + c4 * s4


def _control(t0, h, ratio):
    from scldm_amd import _lib
    c = _lib.Dopri5Control()
    _lib.lib().scldm_dopri5_control(float(t0), float(h), float(ratio), C.byref(c))
    return c


def _solve(m, z2, cond, scales, **kw):
    """(logp, z_end, delta_logp, stats, step log rows) of the C entry itself (DiT.log_likelihood_cfg does not return delta_logp)."""
    from scldm_amd import _lib
    L, h = m._native_handle()
    w, _ = m._weights_struct(tuple(m.parameters()))
    B = z2.shape[0] // 2
    prec = m._prec()
    ul, n_u, cell_row, n_pass, masks, sc, keep = m._cfg_plan(cond, scales, B, dedup=True)
    z = z2.clone()
    saved = torch.empty(L.scldm_dit_train_saved_bytes_for(h, (2 + n_pass) * B, prec), dtype=torch.uint8, device="cuda")
    ws = torch.empty(L.scldm_logp_ode_dopri5_workspace_bytes(h, B, n_pass, prec), dtype=torch.uint8, device="cuda")
    logp, dl = torch.empty(2 * B, device="cuda"), torch.empty(2 * B, device="cuda")
    stats, cap = _lib.Dopri5Stats(), 64
    log = (C.c_double * (4 * cap))()
    probe = kw.get("probe")
    rc = L.scldm_logp_ode_dopri5(h, C.byref(w), z.data_ptr(), C.cast(ul, _lib.c_void_pp) if ul is not None else None, n_u, cell_row, B, n_pass,
                                 masks, sc, kw["atol"], kw["rtol"], kw.get("first_step") or 0.0, probe.data_ptr() if probe is not None else None,
                                 int(probe is not None or kw.get("per_solve", False)), kw.get("seed", 0), 0, B, logp.data_ptr(), dl.data_ptr(),
                                 C.byref(stats), log, cap, prec, saved.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "scldm_logp_ode_dopri5")
    torch.cuda.synchronize()
    del keep
    assert stats.step_log_len < cap
    return logp, z, dl, stats, [tuple(log[4 * i:4 * i + 4]) for i in range(stats.step_log_len)]


REPLAY = [  # fixture (or input width of the two-layer model), cells, conditioning, precision, probe, first step, at least one rejection
    ("dit_base", 3, "scale1.5", "bf16", "seed", 1.0, True),       # 6 rows: a workgroup with two idle waves, 2B % 4 != 0
    ("dit_base", 4, "none", "fp32", "given", None, False),        # P = 0; the automatic first step
    ("dit_me2_256", 3, "golden", "fp32", "given", 0.25, False),   # two passes
    ("dit_joint", 3, "golden", "fp32", "seed", 0.25, False),      # one joint pass
    ("dit_base", 37, "few_labels", "bf16", "given", 0.25, False), # n_urows < B, cell_row map
    (12, 5, "scale1.5", "bf16", "seed", 0.25, False),             # e = 192: idle lanes
    (32, 5, "scale1.5", "bf16", "given", 0.25, False),            # e = 512: two groups per lane
]


@pytest.mark.parametrize("name,B,case,precision,probes,first_step,want_rejection", REPLAY,
                         ids=[f"{c[0]}-B{c[1]}-{c[2]}-{c[3]}-{c[4]}-h{c[5]}" for c in REPLAY])
def test_fused_solve_replays_bit_for_bit_from_its_step_log(name, B, case, precision, probes, first_step, want_rejection):
    """Every logged attempt (s0, h, accepted, ratio) is recomputed: the six evaluations through DiT.input_vjp and DiT.logp_probe, the stage
    points and the error ratio in torch (|mine - logged| <= 1e-9 logged: only the order of at most ~2e4 non-negative double additions
    differs, ~2e-12), the controller's decision from the LOGGED ratio (exactly the accept flag and the next logged (s0, h)); then the
    interpolant at s = 1: z_end, delta_logp and logp bit for bit.  atol = rtol = 1e-3: a handful of attempts."""
    if isinstance(name, int):
        g, m = None, _two_layer(name, precision)
    else:
        g, m, _, _ = build(name, precision)
    z2, cond, scales, probe = _inputs(m, g, B, case, 70 + B)
    tol, seed = 1e-3, 0xD0931
    given = probe if probes == "given" else None
    logp, z_end, dl, stats, log = _solve(m, z2, cond, scales, atol=tol, rtol=tol, first_step=first_step, probe=given, seed=seed)
    n_rej = sum(1 for r in log if r[2] == 0.0)
    print(f"[logp dopri5 replay] {name} B={B} {case} [{precision}] {probes}: {len(log)} attempts, {n_rej} rejected, {stats.evaluations} evaluations, "
          f"first step {stats.first_step!r}; ratios {[f'{r[3]:.3g}' for r in log]}")
    assert torch.isfinite(logp).all() and torch.isfinite(z_end).all() and stats.status == 0
    assert stats.accepted + stats.rejected == len(log) and stats.rejected == n_rej and len(log) >= 1
    if want_rejection:
        assert n_rej >= 1
    rp = _Replay(m, z2, cond, scales, (lambda ev: given) if given is not None else (lambda ev: m.logp_probe(seed, ev, B)), tol, tol)
    y0, l0 = z2.clone(), torch.zeros(2 * B, device="cuda")
    kx0, kl0 = rp.evaluate(y0, 0.0)
    if first_step is None:      # Hairer / Norsett / Wanner on the test's own norms: the order of the double sums differs, nothing else
        from scldm_amd import _lib
        L = _lib.lib()
        cnt = 2 * B * (rp.e + 1)
        d0 = ((rp.sq_sum(y0, y0) + rp.sq_sum(l0, l0)) / cnt) ** 0.5
        d1 = ((rp.sq_sum(kx0, y0) + rp.sq_sum(kl0, l0)) / cnt) ** 0.5
        h0 = L.scldm_dopri5_initial_h0(d0, d1)
        h0f = float(f32(h0))
        kx1, kl1 = rp.evaluate(y0 + kx0 * h0f, f32(0.0 + h0))
        d2 = ((rp.sq_sum(kx1 - kx0, y0) + rp.sq_sum(kl1 - kl0, l0)) / cnt) ** 0.5 / h0
        want = L.scldm_dopri5_initial_step(h0, d1, d2)
        assert abs(stats.first_step - want) <= 1e-9 * want, (stats.first_step, want)
    else:
        assert stats.first_step == first_step
    assert log[0][0] == 0.0 and log[0][1] == stats.first_step
    fit = None
    for i, (t0, h, accepted, ratio) in enumerate(log):
        y1, l1, kx, kl, mine, plan = rp.attempt(t0, h, y0, l0, kx0, kl0)
        assert abs(mine - ratio) <= 1e-9 * ratio, (i, mine, ratio)
        c = _control(t0, h, ratio)
        assert c.accepted == int(accepted != 0.0) and not c.underflow
        if i + 1 < len(log):
            assert (c.t1, c.h_next) == (log[i + 1][0], log[i + 1][1]) and c.t1 < 1.0
        else:
            assert c.accepted and c.t1 >= 1.0
        if c.accepted:
            fit = (plan, t0, c.t1, y0, l0, y1, l1, kx, kl)
            y0, l0, kx0, kl0 = y1, l1, kx[6], kl[6]
    assert rp.n_eval == stats.evaluations
    plan, t0, t1, ya, la, yb, lb, kx, kl = fit
    s = (1.0 - t0) / (t1 - t0)
    z_want, l_want = rp.interpolate(plan, s, ya, yb, kx), rp.interpolate(plan, s, la, lb, kl)
    c0 = float(f32(-0.5 * rp.e * math.log(2.0 * math.pi)))
    assert torch.equal(z_end, z_want)
    assert torch.equal(dl, l_want)
    assert torch.equal(logp, (c0 - _row_sum_fixed((z_want * z_want).reshape(2 * B, rp.e)) * 0.5) - l_want)
    # the Python entry returns the same bits and reports the log
    kw = dict(probe_per="solve", probe=given) if given is not None else dict(seed=seed)
    lp2, z2_end = m.log_likelihood_cfg(z2, cond, scales, 50, "dopri5", atol=tol, rtol=tol, first_step=first_step, **kw)
    st = m.last_solver_stats
    assert torch.equal(lp2, logp) and torch.equal(z2_end, z_end)
    assert st["evaluations"] == stats.evaluations and st["accepted"] == stats.accepted and st["rejected"] == n_rej and st["status"] == 0
    assert st["accepted_steps"] == [(r[0], r[1]) for r in log if r[2]] and st["rejected_steps"] == [(r[0], r[1]) for r in log if not r[2]]
    assert st["error_ratios"] == [r[3] for r in log] and st["first_step"] == stats.first_step


# ---------------------------------------------------------------------------------------------------------------- float64 parity, class gate
_F64 = {}
FIRST = 0.0625     # the given first step of the class gate (both routes start from it)


def _parity_case():
    """dit_base, 3 cells (the fixture's latents and labels), scale 1.5, one fixed probe, atol = rtol = 1e-6: the float64 restatement over
    the float64 oracle, once per session."""
    f, sd, cfg, z2, cond2, scales, _ = logp_ref.load_case("logp_base_euler")
    assert scales == {"clusters": 1.5} and z2.shape[0] == 6
    gen = torch.Generator().manual_seed(77)
    probe = (torch.randint(2, z2.shape, generator=gen) * 2 - 1).float()
    if "ref" not in _F64:
        from oracle.dit import dit_forward_with_cfg
        sd64 = {k: v.double() for k, v in sd.items()}
        n_thr = torch.get_num_threads()
        torch.set_num_threads(min(16, n_thr))
        try:
            _F64["ref"] = logp_dopri5_ref.logp_dopri5_ref(z2, lambda x, t: dit_forward_with_cfg(sd64, cfg, x, t, cond2, scales), probe.double(), 1e-6, 1e-6)
        finally:
            torch.set_num_threads(n_thr)
    return z2.cuda(), {k: v.cuda() for k, v in cond2.items()}, scales, probe.cuda(), _F64["ref"]


@pytest.mark.parametrize("precision,tol", PARITY)
def test_fused_solve_against_the_float64_restatement(precision, tol):
    """fp32 / bf16x3 at atol = rtol = 1e-6 (the solver's own error is below the gate there): logp and z_end within the project's 1e-4."""
    g, m, cfg, sd = build("dit_base", precision)
    z2, cond, scales, probe, (logp64, z64, st64) = _parity_case()
    logp, z_end = m.log_likelihood_cfg(z2, cond, scales, 50, "dopri5", atol=1e-6, rtol=1e-6, probe_per="solve", probe=probe)
    st = m.last_solver_stats
    d_l, d_x = max_abs_rel(logp.cpu(), logp64), max_abs_rel(z_end.cpu(), z64)
    print(f"[parity] fused logp dopri5 [{precision}]: logp {d_l:.3e}, z_end {d_x:.3e}   tol {tol:g};  evaluations fused {st['evaluations']} "
          f"({st['accepted']} accepted, {st['rejected']} rejected), float64 {st64['evaluations']} ({len(st64['accepted'])}, {len(st64['rejected'])})")
    assert torch.isfinite(logp).all() and d_l <= tol and d_x <= tol


def _generic(m, z2, cond, scales, probe, atol, rtol, first_step):
    from scldm_amd.transport import Sampler, create_transport
    fn = Sampler(create_transport()).sample_ode_likelihood(sampling_method="dopri5", num_steps=2, atol=atol, rtol=rtol, first_step=first_step)
    logp, z_end = fn(z2, lambda x, t: m._composed_forward_with_cfg(x, t.contiguous(), cond, scales), _probe=lambda x: probe)
    return logp, z_end, fn.last_stats


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_fused_solve_within_the_generic_paths_distance_16_bit(precision):
    """bf16 / fp16 operands, the parity case's inputs and probe, both routes from the same given first step: the fused solve's distance
    to the float64 result may be at most 1.5 x the distance of the generic `Sampler.sample_ode_likelihood("dopri5")` on the same module
    (the factor and form of test_gpu_logp.py's 16-bit gate), for logp and for z_end.
    The two routes share the forward and backward kernels but not the steps: their error ratios differ in the last bits (the generic
    route sums the packed state in torch), and at atol = rtol = 1e-6 the operand rounding is what the controller reacts to, so the
    evaluation counts drift apart (bf16: fused 1327, generic 1345; fp16: 265 | 241).
    Measured on MI355X, distance fused | generic (ratio):
      bf16  logp 3.176e-4 | 2.797e-4 (1.135);  z_end 2.924e-3 | 2.847e-3 (1.027)
      fp16  logp 5.298e-5 | 3.851e-5 (1.376);  z_end 4.411e-4 | 4.382e-4 (1.007)"""
    g, m, cfg, sd = build("dit_base", precision)
    z2, cond, scales, probe, (logp64, z64, st64) = _parity_case()
    logp, z_end = m.log_likelihood_cfg(z2, cond, scales, 50, "dopri5", atol=1e-6, rtol=1e-6, first_step=FIRST, probe_per="solve", probe=probe)
    st = dict(m.last_solver_stats)
    lg, zg, stg = _generic(m, z2, cond, scales, probe, 1e-6, 1e-6, FIRST)
    d_f = (max_abs_rel(logp.cpu(), logp64), max_abs_rel(z_end.cpu(), z64))
    d_g = (max_abs_rel(lg.cpu(), logp64), max_abs_rel(zg.cpu(), z64))
    for what, a, b in zip(("logp", "z_end"), d_f, d_g):
        print(f"[class] logp dopri5 [{precision}] {what}: fused {a:.4e}  generic {b:.4e}  ratio {a / b:.3f};  evaluations fused {st['evaluations']} "
              f"generic {stg['evaluations']}")
    assert torch.isfinite(logp).all() and torch.isfinite(z_end).all()
    for what, a, b in zip(("logp", "z_end"), d_f, d_g):
        assert a <= 1.5 * b, (precision, what, a, b)


# ---------------------------------------------------------------------------------------------------------------- seeds, routing, refusals
@pytest.fixture(scope="module")
def base():
    g, m, cfg, sd = build("dit_base", "bf16")
    z2, cond, scales, probe = _inputs(m, g, 3, "scale1.5", 91)
    kw = dict(atol=1e-3, rtol=1e-3, first_step=0.25)
    ref = m.log_likelihood_cfg(z2, cond, scales, 50, "dopri5", seed=11, **kw)
    return dict(m=m, z2=z2, cond=cond, scales=scales, probe=probe, kw=kw, ref=ref)


def test_seed_reproduces_and_one_probe_per_solve_is_evaluation_zero(base):
    m, z2, cond, scales, kw = base["m"], base["z2"], base["cond"], base["scales"], base["kw"]
    again = m.log_likelihood_cfg(z2, cond, scales, 50, "dopri5", seed=11, **kw)
    other = m.log_likelihood_cfg(z2, cond, scales, 50, "dopri5", seed=12, **kw)
    assert torch.equal(again[0], base["ref"][0]) and torch.equal(again[1], base["ref"][1])
    assert not torch.equal(other[0], base["ref"][0])
    held = m.log_likelihood_cfg(z2, cond, scales, 50, "dopri5", seed=11, probe_per="solve", **kw)
    p0 = m.logp_probe(11, 0, 3)
    for given in (p0, p0[None]):
        same = m.log_likelihood_cfg(z2, cond, scales, 50, "dopri5", probe_per="solve", probe=given, **kw)
        assert torch.equal(held[0], same[0]) and torch.equal(held[1], same[1])
    assert torch.isfinite(held[0]).all() and not torch.equal(held[0], base["ref"][0])
    few = m.log_likelihood_cfg(z2, cond, scales, 2, "dopri5", seed=11, **kw)             # the save-point count does not move the steps
    assert torch.equal(few[0], base["ref"][0]) and torch.equal(few[1], base["ref"][1])


def test_refusals_leave_the_next_solve_intact(base):
    m, z2, cond, scales, kw, probe = base["m"], base["z2"], base["cond"], base["scales"], base["kw"], base["probe"]
    with pytest.raises(NotImplementedError):
        m.log_likelihood_cfg(z2, cond, scales, 4, "rk4")
    for bad in (dict(return_trace=True), dict(probe=probe), dict(atol=0.0), dict(rtol=-1e-3), dict(probe_per="step"), dict(first_step=-0.5),
                dict(probe_per="solve", probe=probe[:4]), dict(cell_offset=2, cells_total=4)):
        with pytest.raises(ValueError):
            m.log_likelihood_cfg(z2, cond, scales, 50, "dopri5", **{**kw, **bad})
    with pytest.raises(ValueError):
        m.log_likelihood_cfg(z2, cond, scales, 4, "euler", probe_per="solve")
    with pytest.raises(ValueError):
        m.log_likelihood_cfg(z2, cond, scales, 4, "heun", probe_per="solve")
    # under graph capture the entry refuses before it launches anything: the capture ends cleanly and the stream stays usable
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(ValueError, match="capturing"):
        with torch.cuda.graph(graph):
            m.log_likelihood_cfg(z2, cond, scales, 50, "dopri5", seed=11, **kw)
    torch.cuda.synchronize()
    again = m.log_likelihood_cfg(z2, cond, scales, 50, "dopri5", seed=11, **kw)
    assert torch.equal(again[0], base["ref"][0]) and torch.equal(again[1], base["ref"][1])


def _count_composed(m):
    calls = []
    orig = m._composed_forward_with_cfg
    m._composed_forward_with_cfg = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    return calls


def test_training_mode_and_wide_shapes_take_the_generic_route(base):
    z2, cond, scales, kw = base["z2"], base["cond"], base["scales"], base["kw"]
    g, m, cfg, sd = build("dit_base", "bf16")
    m.train()
    calls = _count_composed(m)
    logp, z_end = m.log_likelihood_cfg(z2, cond, scales, 50, "dopri5", seed=11, probe_per="solve", **kw)
    st = m.last_solver_stats
    assert len(calls) == st["evaluations"] > 0 and (st["evaluations"] - 1) % 6 == 0 and st["first_step"] == 0.25
    assert torch.isfinite(logp).all() and torch.isfinite(z_end).all() and logp.shape == (6,)
    from test_gpu_train import build as build_wide
    mw, _, _ = build_wide({"a": 5, "b": 7}, "joint", 2, 77, n_embed=512, n_head=8)
    mw = mw.cuda().eval()
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(3, mw.seq_len, mw.n_embed_input, generator=gen).cuda()
    cw = {"a": torch.randint(0, 5, (3,), generator=gen).repeat(2).cuda(), "b": torch.randint(0, 7, (3,), generator=gen).repeat(2).cuda()}
    calls = _count_composed(mw)
    logp, z_end = mw.log_likelihood_cfg(torch.cat([x, x]), cw, {"a": 1.5, "b": 1.5}, 50, "dopri5", seed=3, **kw)
    st = mw.last_solver_stats
    assert len(calls) == st["evaluations"] > 0 and st["status"] == 0
    assert torch.isfinite(logp).all() and torch.isfinite(z_end).all()


def test_weights_are_read_live(base):
    """An in-place `.data` change (what an EMA swap does: no version counter moves) between two solves is seen by the second one."""
    z2, cond, scales, kw = base["z2"], base["cond"], base["scales"], base["kw"]
    g, m, cfg, sd = build("dit_base", "bf16")
    a = m.log_likelihood_cfg(z2, cond, scales, 50, "dopri5", seed=11, **kw)
    assert torch.equal(a[0], base["ref"][0])
    with torch.no_grad():
        p = [q for q in m.parameters() if q.dim() == 2 and q.shape[0] >= 256][2]
        p.data.mul_(1.25)
    b = m.log_likelihood_cfg(z2, cond, scales, 50, "dopri5", seed=11, **kw)
    assert torch.isfinite(b[0]).all() and not torch.equal(a[0], b[0]) and not torch.equal(a[1], b[1])

"""CPU-side checks of the fused adaptive sampler (scldm_sample_ode_dopri5): the ABI surface, the refusal of a handle outside the fused
family (before any HIP call) and the solve's host side, plain C++ (csrc/dopri5_ctl.hpp) - the handle-free scldm_dopri5_* entries and the
step loop both fused solves run, compiled into a test shim - against the float64 oracle (oracle/transport.py: sample_ode_dopri5) and
against the weights the host-composed solver hands to its kernels."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

ENTRIES = ["scldm_sample_ode_dopri5_workspace_bytes", "scldm_sample_ode_dopri5", "scldm_sample_ode_dopri5_at", "scldm_dopri5_stage_plan", "scldm_dopri5_control",
           "scldm_dopri5_initial_h0", "scldm_dopri5_initial_step"]


def test_header_declares_and_library_exports_the_entries():
    from scldm_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "scldm_hip.h")).read()
    declared = set(re.findall(r"\b(scldm_[a-z_0-9]+)\s*\(", hdr))
    L = _lib.lib()
    for name in ENTRIES:
        assert name in declared, f"include/scldm_hip.h does not declare {name}"
        assert hasattr(L, name), f"libscldm_hip.so does not export {name}"
        assert name in _lib.EXPORTS
    assert len(_lib.EXPORTS) == len(set(_lib.EXPORTS))
    assert L.scldm_version() == 5
    for struct in ("scldm_dopri5_stats", "scldm_dopri5_plan", "scldm_dopri5_control_out"):
        assert re.search(r"\}\s*" + struct + r"\s*;", hdr), struct
    # the ctypes mirrors have the layout the header's structs compile to (4-byte floats / ints, 8-byte doubles, natural alignment)
    assert C.sizeof(_lib.Dopri5Plan) == 4 * (6 + 42 + 14 + 8 + 2) and C.sizeof(_lib.Dopri5Control) == 24 and C.sizeof(_lib.Dopri5Stats) == 40


def test_wide_handle_is_refused_before_any_hip_call():
    """A handle outside the fused family holds no device memory; the entry names the shape family and touches nothing - host buffers stand
    in for z and the workspace and stay as they are."""
    from scldm_amd import _lib
    L = _lib.lib()
    cfg = _lib.DitConfig(n_embed=512, n_embed_input=16, n_layer=2, n_head=8, seq_len=16, hidden_dim=1368, layernorm_eps=1e-8, n_classes=1,
                         has_null_row=1)
    cfg.class_vocab[0] = 4
    h = C.c_void_p()
    assert L.scldm_dit_create(C.byref(cfg), C.byref(h)) == 0
    try:
        z = (C.c_float * 512)(*([1.5] * 512))
        buf = (C.c_char * 4096)()
        ws = (C.addressof(buf) + 255) & ~255
        stats = _lib.Dopri5Stats(evaluations=7)
        masks, scales = (C.c_uint32 * 1)(1), (C.c_float * 1)(2.0)
        rc = L.scldm_sample_ode_dopri5(h, C.addressof(z), None, 0, None, 1, 0, masks, scales, 2, 1e-5, 1e-5, 0.0, None, C.byref(stats), None, 0, 0,
                                       ws, None)
        assert rc == -1, rc                                   # SCLDM_ERR_SHAPE
        msg = L.scldm_last_error().decode()
        assert "fused family" in msg and "512" in msg, msg
        assert all(v == 1.5 for v in z) and stats.evaluations == 0
        assert L.scldm_sample_ode_dopri5_workspace_bytes(h, 4, 1, 4) == 0
        assert L.scldm_sample_ode_dopri5(None, C.addressof(z), None, 0, None, 1, 0, masks, scales, 2, 1e-5, 1e-5, 0.0, None, None, None, 0, 0, ws,
                                         None) == -1 and b"null" in L.scldm_last_error()
    finally:
        L.scldm_dit_destroy(h)


def _plan(L, t0, h):
    from scldm_amd import _lib
    p = _lib.Dopri5Plan()
    L.scldm_dopri5_stage_plan(float(t0), float(h), C.byref(p))
    return p


def _control(L, t0, h, ratio):
    from scldm_amd import _lib
    c = _lib.Dopri5Control()
    L.scldm_dopri5_control(float(t0), float(h), float(ratio), C.byref(c))
    return c


def _bits(v):
    return np.asarray(v, dtype=np.float32).view(np.uint32).tolist()


@pytest.mark.parametrize("t0,h", [(0.0, 0.04512345678), (0.3141592653589793, 0.2718281828459045), (0.9, 0.37), (0.123456789, 1e-7),
                                  (0.5, 3.3e-41), (0.0, 1.0)])
def test_stage_plan_is_bitwise_what_the_composed_solver_hands_to_its_kernels(t0, h):
    """Times as `float(tval)` -> `torch.full(float32)`, weights as `_tab` / `f32` of Sampler._sample_dopri5: (float)(h * w) formed in
    double, structural zeros skipped (mask bit clear) - compared as fp32 bit patterns."""
    from scldm_amd import _lib
    from scldm_amd.transport import _DP_A, _DP_C, _DP_E, _DP_MID
    L = _lib.lib()
    p = _plan(L, t0, h)
    f32 = lambda v: float(np.float32(v))
    times = [float(torch.full((), float(t0 + h if c == 1.0 else t0 + c * h), dtype=torch.float32)) for c in _DP_C]
    assert _bits(list(p.t_stage)) == _bits(times)

    def tab(w):                       # (indices kept, their fp32 weights): `_tab` without the tensors
        keep = [j for j, wi in enumerate(w) if wi != 0.0]
        return keep, [f32(h * w[j]) for j in keep]

    for i, row in enumerate(_DP_A):
        keep, cs = tab(row)
        assert p.a_mask[i] == sum(1 << j for j in keep)
        assert _bits([p.a[i][j] for j in keep]) == _bits(cs)
    for name, w, mask, got in (("error", _DP_E, p.err_mask, p.err), ("mid-point", _DP_MID, p.mid_mask, p.mid)):
        keep, cs = tab(w)
        assert mask == sum(1 << j for j in keep), name
        assert _bits([got[j] for j in keep]) == _bits(cs), name
    assert _bits([p.h, p.two_h]) == _bits([f32(h), f32(2 * h)])


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """The shipped step loop (scldm::dopri5::solve, csrc/dopri5_ctl.hpp) behind tests/dopri5_driver_shim.cpp, compiled with the first host
    compiler there is.  No compiler is a failure, not a skip: the loop would go untested."""
    import shutil
    import subprocess
    from scldm_amd import _lib
    cxx = next((c for c in ("c++", "g++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler (c++, g++, ROCm's clang++): the dopri5 step loop cannot be tested"
    so = str(tmp_path_factory.mktemp("dopri5_driver") / "dopri5_driver_shim.so")
    cmd = [cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(ROOT, "tests", "dopri5_driver_shim.cpp"), "-o", so]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stderr

    class Step(C.Structure):          # scldm::dopri5::Step
        _fields_ = [("t0", C.c_double), ("h", C.c_double), ("n_eval", C.c_longlong), ("plan", _lib.Dopri5Plan)]

    pd = C.POINTER(C.c_double)
    members = [("first_slope", C.CFUNCTYPE(C.c_int)), ("start_norms", C.CFUNCTYPE(C.c_int, pd)), ("probe", C.CFUNCTYPE(C.c_int, C.c_double, pd)),
               ("save_time", C.CFUNCTYPE(C.c_double, C.c_int)), ("attempt", C.CFUNCTYPE(C.c_int, C.POINTER(Step), pd)),
               ("accept", C.CFUNCTYPE(C.c_int, C.POINTER(Step), C.c_int)), ("emit", C.CFUNCTYPE(C.c_int, C.c_int, C.c_double)),
               ("reached", C.CFUNCTYPE(C.c_int))]

    class Callbacks(C.Structure):     # shim_callbacks of the shim, in its order
        _fields_ = members

    D = C.CDLL(so)
    D.Callbacks = Callbacks
    D.dopri5_shim_solve.argtypes = [C.POINTER(Callbacks), C.c_double, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_int, C.c_int,
                                    C.POINTER(_lib.Dopri5Stats)]
    D.dopri5_shim_solve.restype = C.c_int
    D.dopri5_shim_message.restype = C.c_char_p
    return D


def _drive(D, problem, save_times, first_step=0.0, first_save=1, cap=4096, stride=3):
    """One solve of the shipped loop over `problem` (an object with the members the loop calls, save_time apart): return code, stats, the
    step log's written rows (the rest of the buffer must be untouched) and how often emit / reached were called."""
    from scldm_amd import _lib
    calls = {"emit": [], "reached": 0}
    raised = []

    def guard(fn):                # an exception must not pass through the C frames: it ends the solve with a code and is raised after it
        def run(*a):
            try:
                return fn(*a) or 0
            except BaseException as e:     # noqa: BLE001
                raised.append(e)
                return -99
        return run

    def emit(si, s):
        calls["emit"].append((si, s))
        return problem.emit(si, s)

    def reached():
        calls["reached"] += 1
        return problem.reached()

    members = dict(first_slope=guard(problem.first_slope), start_norms=guard(problem.start_norms), probe=guard(problem.probe),
                   save_time=lambda si: float(save_times[si]), attempt=guard(problem.attempt), accept=guard(problem.accept), emit=guard(emit),
                   reached=guard(reached))
    cb = D.Callbacks(**{name: typ(members[name]) for name, typ in D.Callbacks._fields_})
    slack = 4                     # rows past the cap, which must stay as they are
    log = (C.c_double * (stride * (cap + slack)))(*([-7.0] * (stride * (cap + slack))))
    stats = _lib.Dopri5Stats()
    rc = D.dopri5_shim_solve(C.byref(cb), float(first_step), first_save, len(save_times), log, cap, stride, C.byref(stats))
    if raised:
        raise raised[0]
    rows = [tuple(log[stride * i:stride * (i + 1)]) for i in range(stats.step_log_len)]
    assert all(v == -7.0 for v in log[stride * stats.step_log_len:]), "the step log was written past step_log_len rows"
    return rc, stats, rows, calls


class _OracleArithmetic:
    """Dormand-Prince's state arithmetic in float64 numpy exactly as oracle/transport.py writes it (its `@` products and torch.sin fix the
    bits); WHEN each piece runs, with which step, is the shipped loop's business."""

    def __init__(self, x, model_fn, atol, rtol):
        self.shape, self.nb, self.model_fn, self.atol, self.rtol = tuple(x.shape), x.shape[0], model_fn, atol, rtol
        self.y0 = x.detach().to(torch.float64).numpy().reshape(-1).copy()
        self.n_eval = 0

    def f(self, t32, y):
        self.n_eval += 1
        tv = torch.full((self.nb,), float(t32), dtype=torch.float32)
        return self.model_fn(torch.from_numpy(y.reshape(self.shape).copy()), tv).detach().to(torch.float64).numpy().reshape(-1)

    @staticmethod
    def _ms(a):                   # _rms64 before its square root
        return float(np.mean(np.square(np.abs(a))))

    def first_slope(self):
        self.f0 = self.f(np.float32(0.0), self.y0)

    def start_norms(self, ms):
        self.scale = self.atol + np.abs(self.y0) * self.rtol
        ms[0], ms[1] = self._ms(self.y0 / self.scale), self._ms(self.f0 / self.scale)

    def probe(self, h0, ms):
        ms[0] = self._ms((self.f(np.float32(0.0 + h0), self.y0 + h0 * self.f0) - self.f0) / self.scale)

    def attempt(self, step, ms):
        from oracle.transport import _DP_BETA, _DP_C_ERROR
        st, y0 = step.contents, self.y0
        assert st.n_eval == self.n_eval
        dt, p = st.h, st.plan
        k = np.empty((7, y0.size))
        k[0] = self.f0
        for i, beta in enumerate(_DP_BETA):
            assert p.a_mask[i] == sum(1 << j for j, b in enumerate(beta) if b != 0.0)
            yi = y0 + (beta * dt) @ k[:i + 1]
            k[i + 1] = self.f(p.t_stage[i], yi)
        ms[0] = self._ms(((dt * _DP_C_ERROR) @ k) / (self.atol + self.rtol * np.maximum(np.abs(y0), np.abs(yi))))
        self.y1, self.f1 = yi, k[6]

    def accept(self, step, fit_dense):
        self.y0, self.f0 = self.y1, self.f1

    def emit(self, si, s):
        assert 0.0 <= s <= 1.0, s

    def reached(self):
        pass


def _c_stepper(D, x, model_fn, num_steps, atol, rtol, **kw):
    """The shipped loop over the oracle's arithmetic: (accepted, rejected) (t0, dt) lists from the loop's own step log, the number of
    model evaluations made, and what _drive returns."""
    problem = _OracleArithmetic(x, model_fn, atol, rtol)
    ts = torch.linspace(0.0, 1.0, num_steps).to(torch.float64).numpy()
    rc, stats, rows, calls = _drive(D, problem, ts, **kw)
    accepted, rejected = [r[:2] for r in rows if r[2] == 1.0], [r[:2] for r in rows if r[2] == 0.0]
    assert len(accepted) + len(rejected) == len(rows)
    return accepted, rejected, problem.n_eval, (rc, stats, rows, calls)


def _forced(x, t):            # y' = -y + sin(8 t), every unknown with its own start value
    return -x + torch.sin(8.0 * t.double()).view(-1, 1)


def _rotation(x, t):          # (u, v)' = w (-v, u), a different angular velocity per pair
    u, v = x[:, :8], x[:, 8:]
    w = torch.linspace(1.0, 9.0, 8, dtype=torch.float64)
    return torch.cat([-w * v, w * u], dim=1)


@pytest.mark.parametrize("system", [_forced, _rotation], ids=["forced_decay", "rotation"])
@pytest.mark.parametrize("tol", [1e-5, 1e-7])
def test_controller_reproduces_the_oracle_step_sequence(driver, system, tol):
    """64 unknowns, 50 save points: exactly the oracle's accepted and rejected (t0, dt) lists and its evaluation count - the lists as the
    shipped step loop logs them - and the loop's statistics agree with its log."""
    from oracle.transport import sample_ode_dopri5
    x0 = torch.randn(4, 16, generator=torch.Generator().manual_seed(11), dtype=torch.float64)
    _, st = sample_ode_dopri5(x0, system, 50, tol, tol, return_stats=True)
    acc, rej, n_eval, (rc, stats, rows, calls) = _c_stepper(driver, x0, system, 50, tol, tol)
    print(f"[dopri5 controller] {system.__name__} tol {tol:g}: {len(acc)} accepted, {len(rej)} rejected, {n_eval} evaluations")
    assert len(st["accepted"]) >= 3
    assert acc == [(float(a), float(b)) for a, b in st["accepted"]]
    assert rej == [(float(a), float(b)) for a, b in st["rejected"]]
    assert n_eval == st["evaluations"]
    assert rc == 0 and stats.status == 0 and stats.evaluations == n_eval
    assert (stats.accepted, stats.rejected, stats.step_log_len) == (len(acc), len(rej), len(rows))
    assert stats.first_step == rows[0][1] and rows[0][0] == 0.0
    assert [si for si, _ in calls["emit"]] == list(range(1, 50)) and calls["reached"] == 0


class _Scripted:
    """A problem without a state: attempt k reports the k-th scripted mean squared error ratio (the last one from then on)."""

    def __init__(self, mean_squares):
        self.script, self.attempts = list(mean_squares), 0
        self.first_slope = self.start_norms = self.probe = self.accept = self.emit = self.reached = lambda *a: 0

    def attempt(self, step, ms):
        ms[0] = self.script[min(self.attempts, len(self.script) - 1)]
        self.attempts += 1


def test_loop_flags_a_step_that_cannot_advance_the_time(driver):
    """The underflow exit of the shipped loop.  Time starts at 0, where every positive step advances it, so no given first step underflows
    before the first attempt; the shortest way there is one accepted step to t = 0.5 and then rejections, each shrinking the step to a fifth,
    until 0.5 + h == 0.5.  The loop must stop exactly there: SCLDM_ERR_SOLVER, status SCLDM_DOPRI5_UNDERFLOW, reached() once, no save point."""
    h, attempts = 0.5 * 0.9, 1                # ratio 1 is accepted and the next step is 0.9 of it
    while 0.5 + h > 0.5:
        h, attempts = h * 0.2, attempts + 1   # ratio 1e150: min(10, max(0.9 / ratio^0.2, 0.2)) == 0.2
    problem = _Scripted([1.0, 1e300])
    rc, stats, rows, calls = _drive(driver, problem, [0.0, 1.0], first_step=0.5)
    assert rc == -4 and stats.status == 1, (rc, stats.status)
    assert b"dopri5: step size underflow / too many evaluations" in driver.dopri5_shim_message()
    assert problem.attempts == attempts and stats.evaluations == 1 + 6 * attempts
    assert (stats.accepted, stats.rejected, stats.first_step, stats.step_log_len) == (1, attempts - 1, 0.5, attempts)
    assert rows[0] == (0.0, 0.5, 1.0) and all(r[0] == 0.5 and r[2] == 0.0 for r in rows[1:]) and 0.5 + rows[-1][1] * 0.2 == 0.5
    assert calls["reached"] == 1 and calls["emit"] == []


def test_step_log_cap_bounds_the_log_not_the_solve(driver):
    """A step log of 2 rows on a solve with more attempts: exactly 2 rows are written (_drive checks the buffer behind them), with the
    ratio in the fourth column of the 4-wide layout, and the solve still finishes."""
    x0 = torch.randn(4, 16, generator=torch.Generator().manual_seed(11), dtype=torch.float64)
    acc, rej, n_eval, (rc, stats, rows, calls) = _c_stepper(driver, x0, _forced, 3, 1e-5, 1e-5, cap=2, stride=4)
    assert rc == 0 and stats.status == 0 and stats.step_log_len == 2 and len(rows) == 2
    assert stats.accepted + stats.rejected > 2 and stats.evaluations == n_eval == 2 + 6 * (stats.accepted + stats.rejected)
    assert all(r[3] > 0.0 and (r[3] <= 1.0) == (r[2] == 1.0) for r in rows)
    assert [si for si, _ in calls["emit"]] == [1, 2]


def test_control_rule_and_underflow_flag():
    from scldm_amd import _lib
    L = _lib.lib()
    c = _control(L, 0.25, 0.1, 0.5)
    assert c.accepted == 1 and c.t1 == 0.25 + 0.1 and c.h_next == 0.1 * min(10.0, max(0.9 / 0.5 ** 0.2, 1.0)) and c.underflow == 0
    c = _control(L, 0.25, 0.1, 1.0)                      # ratio == 1 is accepted; the step may not shrink after an accepted step... below 1
    assert c.accepted == 1 and c.h_next == 0.1 * min(10.0, max(0.9 / 1.0 ** 0.2, 0.2))
    c = _control(L, 0.25, 0.1, 7.0)
    assert c.accepted == 0 and c.t1 == 0.25 and c.h_next == 0.1 * min(10.0, max(0.9 / 7.0 ** 0.2, 0.2))
    c = _control(L, 0.25, 0.1, 1e9)
    assert c.accepted == 0 and c.h_next == 0.1 * 0.2
    c = _control(L, 0.25, 0.1, 0.0)
    assert c.accepted == 1 and c.h_next == 0.1 * 10.0
    c = _control(L, 0.25, 0.1, 1e-12)
    assert c.h_next == 0.1 * 10.0
    # t + h == t: a step that cannot advance the time is flagged, whether it follows an accepted or a rejected one
    c = _control(L, 1.0, 1e-20, 0.5)
    assert c.accepted == 1 and c.t1 == 1.0 and c.t1 + c.h_next == c.t1 and c.underflow == 1
    c = _control(L, 0.5, 1e-16, 50.0)
    assert c.accepted == 0 and c.t1 + c.h_next == c.t1 and c.underflow == 1
    assert _control(L, 0.5, 1e-15, 50.0).underflow == 0
    # the initial step's corner cases (Hairer / Norsett / Wanner)
    assert L.scldm_dopri5_initial_h0(1e-6, 3.0) == 1e-6 and L.scldm_dopri5_initial_h0(2.0, 4.0) == 0.01 * 2.0 / 4.0
    assert L.scldm_dopri5_initial_step(1e-6, 0.0, 0.0) == max(1e-6, 1e-6 * 1e-3)
    assert L.scldm_dopri5_initial_step(0.005, 2.0, 3.0) == min(100.0 * 0.005, (0.01 / 3.0) ** (1.0 / 5.0))


def test_python_surface():
    """Signatures the issue fixes, and the routing of a CPU module: there is no CPU path."""
    import inspect
    from scldm_amd import sampling
    from scldm_amd.nnets import DiT
    from scldm_amd.transport import Sampler
    sig = inspect.signature(DiT.sample_ode_cfg).parameters
    assert sig["first_step"].default is None and sig["first_step"].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig["return_trajectory"].default is False and sig["atol"].default == 1e-5 and sig["rtol"].default == 1e-5
    assert inspect.signature(Sampler._sample_dopri5).parameters["first_step"].default is None
    for fn in (sampling.sample_latents, sampling.sample_cells, sampling.generate_cells_stream):
        p = inspect.signature(fn).parameters
        assert p["atol"].default == 1e-5 and p["rtol"].default == 1e-5, fn.__name__
    assert "share" in sampling.generate_cells_stream.__doc__ and "step size" in sampling.generate_cells_stream.__doc__
    m = DiT(n_embed=256, n_embed_input=16, n_layer=1, n_head=8, seq_len=16, dropout=0.0, bias=True, norm_layer="layernorm", multiple_of=4,
            layernorm_eps=1e-8, class_vocab_sizes={"a": 3}, cfg_dropout_prob=0.8).eval()
    assert m.last_solver_stats is None
    with pytest.raises(RuntimeError, match="CUDA"):
        m.sample_ode_cfg(torch.zeros(2, 16, 16), {"a": torch.zeros(2, dtype=torch.long)}, {"a": 2.0}, 2, "dopri5")
    # first_step on the generic host solver: the given step is the first attempted one and the probe evaluation is saved
    calls = []
    f = lambda x, t: (calls.append(float(t[0])), -x)[1]
    from scldm_amd.transport import create_transport
    s = Sampler(create_transport())
    fn = s._sample_dopri5(3, 1e-6, 1e-6, first_step=0.0625)
    fn(torch.ones(2, 4, dtype=torch.float64), f)
    st = fn.last_stats
    assert sorted(st["accepted_steps"] + st["rejected_steps"])[0] == (0.0, 0.0625) and (st["evaluations"] - 1) % 6 == 0

"""CPU-side checks of the host side of the fixed-grid solves, plain C++ (csrc/fixed_grid.hpp) compiled into a test shim
(tests/fixed_grid_shim.cpp): the one fp32 linspace against numpy-fp32 restatements of the three formulas it replaced, the evaluation-time
lists of the four layouts in use, and the Euler / Heun step loop's call sequence."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT

f32 = np.float32
# the grids in use, end points formed as the entries form them: [0, 1] (scldm_sample_ode, scldm_logp_ode, the wide path),
# [0, fp32(1 - last_step_size)] (scldm_sample_sde) and [fp32(eps), fp32(1 - eps)] (scldm_sample_ode_transport)
GRIDS = [(f32(0), f32(1)), (f32(0), f32(1.0 - float(f32(0.04)))), (f32(1e-3), f32(1.0 - 1e-3)), (f32(1e-5), f32(1.0 - 1e-5))]
POINTS = [2, 3, 5, 6, 10, 51, 101, 201, 4097, 4098]


@pytest.fixture(scope="module")
def grid(tmp_path_factory):
    """csrc/fixed_grid.hpp behind tests/fixed_grid_shim.cpp, compiled with the first host compiler there is.  No compiler is a failure,
    not a skip: the grid and the loop would go untested."""
    import shutil
    import subprocess
    cxx = next((c for c in ("c++", "g++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler (c++, g++, ROCm's clang++): the fixed-grid host code cannot be tested"
    so = str(tmp_path_factory.mktemp("fixed_grid") / "fixed_grid_shim.so")
    cmd = [cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(ROOT, "tests", "fixed_grid_shim.cpp"), "-o", so]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stderr
    G = C.CDLL(so)
    pf = C.POINTER(C.c_float)
    G.fixed_grid_linspace.argtypes = [C.c_int, C.c_int, C.c_float, C.c_float]
    G.fixed_grid_linspace.restype = C.c_float
    G.fixed_grid_eval_times.argtypes = [C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, C.c_float, pf]
    G.fixed_grid_eval_times.restype = C.c_int
    G.eval_t = C.CFUNCTYPE(C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float)
    G.axpy_t = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float)
    G.heun_t = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float)

    class Ops(C.Structure):   # shim_ops of the shim, in its order
        _fields_ = [("eval", G.eval_t), ("axpy", G.axpy_t), ("heun", G.heun_t)]

    G.Ops = Ops
    G.fixed_grid_euler_heun.argtypes = [C.c_int, C.c_float, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Ops)]
    G.fixed_grid_euler_heun.restype = C.c_int
    return G


def shipped(G, steps, a, b):
    return np.array([G.fixed_grid_linspace(i, steps, float(a), float(b)) for i in range(steps)], dtype=f32)


def _bits(x):
    return np.asarray(x, dtype=f32).view(np.uint32)


# The three formulas the unified linspace replaced, restated in numpy: every array is float32, so every product and sum rounds to
# fp32 on its own, in the order the C++ wrote them.
def _fill(steps, lower, upper):
    idx = np.arange(steps)
    return np.where(idx < steps // 2, lower(idx.astype(f32)), upper((steps - idx - 1).astype(f32))).astype(f32)


def parent_linspace01(steps):            # step = 1 / (steps - 1);  step i  |  1 - step (steps - i - 1)
    step = f32(1) / f32(steps - 1)
    return _fill(steps, lambda i: step * i, lambda j: f32(1) - step * j)


def parent_linspace0(steps, t1):         # step = t1 / (steps - 1);  step i  |  t1 - step (steps - i - 1)
    step = f32(t1) / f32(steps - 1)
    return _fill(steps, lambda i: step * i, lambda j: f32(t1) - step * j)


def parent_linspace_ab(steps, t0, t1):   # step = (t1 - t0) / (steps - 1);  t0 + step i  |  t1 - step (steps - i - 1)
    step = (f32(t1) - f32(t0)) / f32(steps - 1)
    return _fill(steps, lambda i: f32(t0) + step * i, lambda j: f32(t1) - step * j)


@pytest.mark.parametrize("steps", POINTS)
@pytest.mark.parametrize("a,b", GRIDS)
def test_linspace_has_the_bits_of_every_formula_it_replaced(grid, a, b, steps):
    got = shipped(grid, steps, a, b)
    assert got.dtype == f32 and got[0] == a and got[-1] == b and np.all(np.diff(got.astype(np.float64)) > 0)
    assert np.array_equal(_bits(got), _bits(parent_linspace_ab(steps, a, b)))
    if a == 0:
        assert np.array_equal(_bits(got), _bits(parent_linspace0(steps, b)))
    if a == 0 and b == 1:
        assert np.array_equal(_bits(got), _bits(parent_linspace01(steps)))


def eval_times(G, n_steps, a, b, second, last=None):
    out = (C.c_float * (2 * n_steps + 1))()
    n = G.fixed_grid_eval_times(n_steps, float(a), float(b), second, last is not None, float(last or 0), out)
    return np.array(out[:n], dtype=f32)


def test_evaluation_time_lists_of_the_four_layouts(grid):
    n_steps = 3
    for a, b in GRIDS:
        t = shipped(grid, n_steps + 1, a, b)
        dt = f32(t[1] - t[0])
        last = f32(b)
        want = {0: [t[0], t[1], t[2]],                                                    # Euler
                1: [t[0], t[1], t[1], t[2], t[2], t[3]],                                  # Heun
                2: [t[0], f32(t[0] + dt), t[1], f32(t[1] + dt), t[2], f32(t[2] + dt)]}    # the SDE's Heun
        for second, w in want.items():
            assert np.array_equal(_bits(eval_times(grid, n_steps, a, b, second)), _bits(w)), (a, b, second)
            assert np.array_equal(_bits(eval_times(grid, n_steps, a, b, second, last)), _bits(w + [last])), (a, b, second, "last")


@pytest.mark.parametrize("a,b", GRIDS)
@pytest.mark.parametrize("heun", [False, True])
def test_step_loop_call_sequence(grid, heun, a, b):
    n_steps = 5
    bufs = {name: np.zeros(4, dtype=f32) for name in ("z", "k1", "k2", "ztmp")}
    who = {v.ctypes.data: k for k, v in bufs.items()}
    who[None] = None
    calls = []
    ops = grid.Ops(grid.eval_t(lambda e, zin, out, ez, hs: calls.append(("eval", e, who[zin], who[out], who[ez], f32(hs))) or 0),
                   grid.axpy_t(lambda z, k, out, hs: calls.append(("axpy", who[z], who[k], who[out], f32(hs))) or 0),
                   grid.heun_t(lambda z, k1, k2, hh: calls.append(("heun", who[z], who[k1], who[k2], f32(hh))) or 0))
    rc = grid.fixed_grid_euler_heun(n_steps, float(a), float(b), int(heun), *(bufs[k].ctypes.data for k in ("z", "k1", "k2", "ztmp")), C.byref(ops))
    assert rc == 0
    t = shipped(grid, n_steps + 1, a, b)
    want = []
    for i in range(n_steps):
        hs = f32(t[i + 1] - t[i])      # the fp32 difference of neighbouring grid values, exactly
        if not heun:
            want.append(("eval", i, "z", "k1", "z", hs))
        else:
            want += [("eval", 2 * i, "z", "k1", None, f32(0)), ("axpy", "z", "k1", "ztmp", hs),
                     ("eval", 2 * i + 1, "ztmp", "k2", None, f32(0)), ("heun", "z", "k1", "k2", f32(f32(0.5) * hs))]
    assert len(calls) == len(want)
    for got, w in zip(calls, want):
        assert got[:-1] == w[:-1] and _bits(got[-1]) == _bits(w[-1]), (got, w)


def test_step_loop_stops_at_the_first_error(grid):
    calls = []
    ops = grid.Ops(grid.eval_t(lambda e, zin, out, ez, hs: calls.append(e) or (7 if e == 2 else 0)),
                   grid.axpy_t(lambda *a: calls.append("axpy") or 0), grid.heun_t(lambda *a: calls.append("heun") or 0))
    assert grid.fixed_grid_euler_heun(4, 0.0, 1.0, 1, None, None, None, None, C.byref(ops)) == 7
    assert calls == [0, "axpy", 1, "heun", 2]

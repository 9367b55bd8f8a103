"""GPU tests of the log-likelihood solve (scldm_logp_ode / DiT.log_likelihood_cfg), its probe source (scldm_logp_probe) and the
input-gradient-only backward under it (scldm_dit_train_backward_dx / DiT.input_vjp): against the training backward (bit for bit), the
reference's recorded runs (tests/golden/logp_*.npz; the probes are the fixture's, so everything downstream of the draws is compared),
the generic Python sampler, its own pieces, and itself across seeds, shards and a graph replay.  Shapes follow the tile rules: 3 cells
(one padded 64-token tile), 6, 15 (no multiple of 4), 324 (past the 320-cell switch from 32- to 64-token tiles)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import logp_ref
from conftest import max_abs_rel
from test_gpu_dit import PARITY, build

pytestmark = pytest.mark.gpu
_REF = {}


def _restatement(name):
    """The CPU restatement on a fixture's inputs and probes, once per session (for the per-row scale sum |dx| of a logp_grad)."""
    if name not in _REF:
        from oracle.dit import dit_forward_with_cfg
        f, sd, cfg, z2, cond2, scales, (method, steps) = logp_ref.load_case(name)
        n_thr = torch.get_num_threads()
        torch.set_num_threads(min(16, n_thr))
        try:
            _REF[name] = logp_ref.logp_ref(z2, lambda x, t: dit_forward_with_cfg(sd, cfg, x, t, cond2, scales), method, steps, torch.from_numpy(f["probes"]))
        finally:
            torch.set_num_threads(n_thr)
    return _REF[name]


def _inputs(name):
    f, sd, cfg, z2, cond2, scales, settings = logp_ref.load_case(name)
    return f, z2.cuda(), {k: v.cuda() for k, v in cond2.items()}, scales, settings


def _distances(got, name):
    """(worst logp_grad error in units of the row's sum |dx|, scale-relative logp error, scale-relative x_end error) against the fixture."""
    logp, z_end, trace = got
    f = logp_ref.load_case(name)[0]
    sc = torch.stack(_restatement(name)[4]).double()
    assert trace.shape == f["logp_grad"].shape and torch.isfinite(trace).all() and torch.isfinite(logp).all() and torch.isfinite(z_end).all()
    d_g = float(((trace.cpu().double() - torch.from_numpy(f["logp_grad"]).double()).abs() / sc).max())
    return d_g, max_abs_rel(logp.cpu(), f["logp"]), max_abs_rel(z_end.cpu(), f["x_end"])


def _fused(m, name):
    f, z2, cond, scales, (method, steps) = _inputs(name)
    return m.log_likelihood_cfg(z2, cond, scales, steps + 1, method, probe=torch.from_numpy(f["probes"]).cuda(), return_trace=True)


def _generic(m, name):
    """The reference-shaped chain: Sampler.sample_ode_likelihood over differentiable forward calls, with the fixture's probes."""
    from scldm_amd.transport import Sampler, create_transport
    f, z2, cond, scales, (method, steps) = _inputs(name)
    probes = iter(torch.from_numpy(f["probes"]).cuda())
    fn = Sampler(create_transport()).sample_ode_likelihood(sampling_method=method, num_steps=steps + 1)
    logp, z_end = fn(z2, lambda x, t: m._composed_forward_with_cfg(x, t.contiguous(), cond, scales), _probe=lambda x: next(probes))
    return logp, z_end, torch.stack(fn.last_trace["logp_grad"])


# ---------------------------------------------------------------------------------------------------------------- input VJP
def vjp_pair(name, precision, n, model=None):
    """(out, dx) of the training backward (autograd with every parameter requiring a gradient) and of DiT.input_vjp, same inputs.
    Without a given model each side gets a fresh one, so that the fp16 loss-scale state one backward leaves on its handle (a power of two
    chosen from max |dout|, lowered after an overflow) cannot reach the other: both choose their scale from the same dout."""
    m = build(name, precision)[1] if model is None else model
    m_dx = build(name, precision)[1] if model is None else model
    gen = torch.Generator().manual_seed(300 + n)
    x = torch.randn(n, m.seq_len, m.n_embed_input, generator=gen).cuda()
    t = torch.rand(n, generator=gen).cuda()
    cond = {k: torch.randint(0, v + 1, (n,), generator=gen).cuda() for k, v in m.class_vocab_sizes.items()}   # (v = the null token)
    if m.condition_strategy != "joint":
        cond = {k: cond[k] for k in sorted(cond)[:1]}
    dout = torch.randn(n, m.seq_len, m.n_embed_input, generator=gen).cuda()
    xr = x.clone().requires_grad_(True)
    y = m(xr, t, cond)
    (dx_full,) = torch.autograd.grad(y, xr, dout)
    assert any(p.grad is None for p in m.parameters())        # (autograd.grad: nothing accumulated, but the full backward ran)
    y2, dx = m_dx.input_vjp(x, t, cond, dout)
    return y.detach(), dx_full, y2, dx


@pytest.mark.parametrize("n", [3, 6, 15, 324])
@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_input_vjp_is_the_training_backwards_dx_bit_for_bit(precision, n):
    """Fused base shape: the d x family of the backward layer kernel, the final layer's d x kernel and the input projection's data
    gradient against scldm_dit_train_backward on an identical record.  No tolerance: the same operands in the same k order."""
    y, dx_full, y2, dx = vjp_pair("dit_base", precision, n)
    assert torch.isfinite(dx).all() and float(dx.abs().max()) > 0
    assert torch.equal(y, y2)
    assert torch.equal(dx, dx_full), float((dx - dx_full).abs().max() / dx_full.abs().max())


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_input_vjp_on_64_token_tiles_at_324_cells_with_small_tiles_off(precision, tmp_path):
    """SCLDM_TRAIN_SMALL_NTT=0 (read once per process): both backwards on 64-token tiles."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_logp_vjp_child.py")
    out = str(tmp_path / "r.pt")
    e = {k: v for k, v in os.environ.items() if not k.startswith("SCLDM_TRAIN_")}
    e["SCLDM_TRAIN_SMALL_NTT"] = "0"
    r = subprocess.run([sys.executable, child, out, precision, "324"], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert torch.load(out) == {"equal_dx": True, "equal_out": True, "finite": True, "nonzero": True}


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_input_vjp_on_the_generic_route(precision):
    """A 512-wide model (head_dim 64: the GEMM-based route): the d x mode only skips the weight-gradient, column-sum and conditioning
    launches and keeps the split-K scratch partition, so bit equality holds here too."""
    from test_gpu_train import build as build_wide
    m, sd, cfg = build_wide({"a": 5, "b": 7}, "joint", 2, 77, n_embed=512, n_head=8)
    m = m.cuda().eval()
    m.precision = precision
    for n in (5, 70):
        y, dx_full, y2, dx = vjp_pair(None, precision, n, model=m)
        assert torch.isfinite(dx).all() and float(dx.abs().max()) > 0
        assert torch.equal(y, y2) and torch.equal(dx, dx_full), (n, float((dx - dx_full).abs().max() / dx_full.abs().max()))


def test_autograd_takes_the_input_gradient_only_call_when_no_parameter_needs_a_gradient(monkeypatch):
    """With every parameter frozen autograd through DiT.forward must not enter scldm_dit_train_backward at all (that entry point is
    replaced by one that raises), and returns the bits it returned through it before."""
    from scldm_amd import _lib
    g, m, cfg, sd = build("dit_base", "bf16")
    y, dx_full, _, _ = vjp_pair("dit_base", "bf16", 6, model=m)
    for p in m.parameters():
        p.requires_grad_(False)
    calls = []
    real_dx = _lib.lib().scldm_dit_train_backward_dx

    def full_backward(*a):
        raise AssertionError("the full training backward ran although no parameter needs a gradient")

    monkeypatch.setattr(_lib.lib(), "scldm_dit_train_backward", full_backward)
    monkeypatch.setattr(_lib.lib(), "scldm_dit_train_backward_dx", lambda *a: (calls.append(1), real_dx(*a))[1])
    y, dx_full2, _, dx = vjp_pair("dit_base", "bf16", 6, model=m)
    assert len(calls) == 2          # autograd's backward and input_vjp's
    assert torch.equal(dx_full, dx_full2) and torch.equal(dx, dx_full2)


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_input_vjp_at_an_input_width_without_edge_kernels(precision):
    """n_embed_input 12 (the single-kernel ends of the fused backward exist for 8 / 16 / 32): the d x walk takes the training backward's
    GEMM-based final layer in front of the same layer kernels - bit for bit the training backward's d x, at 5 and 70 cells; and the
    likelihood solve runs on it."""
    from scldm_amd.nnets import DiT
    torch.manual_seed(12)

    def make():
        m = DiT(n_embed=256, n_embed_input=12, n_layer=2, n_head=8, seq_len=16, dropout=0.0, bias=True, norm_layer="layernorm", multiple_of=4,
                layernorm_eps=1e-8, class_vocab_sizes={"clusters": 14}, cfg_dropout_prob=0.8)
        gen = torch.Generator().manual_seed(3)
        with torch.no_grad():
            for p in m.parameters():
                p.copy_(torch.randn(p.shape, generator=gen) * 0.05)
        m = m.cuda().eval()
        m.precision = precision
        return m

    for n in (5, 70):
        gen = torch.Generator().manual_seed(500 + n)
        x, t = torch.randn(n, 16, 12, generator=gen).cuda(), torch.rand(n, generator=gen).cuda()
        cond = {"clusters": torch.randint(0, 15, (n,), generator=gen).cuda()}
        dout = torch.randn(n, 16, 12, generator=gen).cuda()
        xr = x.clone().requires_grad_(True)
        y = make()(xr, t, cond)
        (dx_full,) = torch.autograd.grad(y, xr, dout)
        m = make()
        y2, dx = m.input_vjp(x, t, cond, dout)
        assert torch.isfinite(dx).all() and float(dx.abs().max()) > 0
        assert torch.equal(y.detach(), y2) and torch.equal(dx, dx_full), (n, float((dx - dx_full).abs().max() / dx_full.abs().max()))
    z = torch.cat([x[:3], x[:3]])
    logp, z_end = m.log_likelihood_cfg(z, {"clusters": cond["clusters"][:3].repeat(2)}, {"clusters": 1.5}, 3, "heun", seed=4)
    assert logp.shape == (6,) and torch.isfinite(logp).all() and torch.isfinite(z_end).all() and not torch.equal(z_end, z)


# ---------------------------------------------------------------------------------------------------------------- fixtures
@pytest.mark.parametrize("name", list(logp_ref.CASES))
@pytest.mark.parametrize("precision,tol", PARITY)
def test_fused_solve_on_recorded_probes(name, precision, tol):
    """fp32 / bf16x3: every logp_grad (scale: sum |dx| of the row), logp and x_end within the project's 1e-4 of the reference's run."""
    g, m, cfg, sd = build(logp_ref.CASES[name][0], precision)
    d_g, d_l, d_x = _distances(_fused(m, name), name)
    print(f"[parity] fused logp solve {name} [{precision}]: logp_grad {d_g:.3e} of sum|dx|, logp {d_l:.3e}, x_end {d_x:.3e}   tol {tol:g}")
    assert d_g <= tol and d_l <= tol and d_x <= tol


@pytest.mark.parametrize("name", ["logp_base_heun", "logp_me2_euler"])
def test_generic_sampler_on_recorded_probes_fp32(name):
    g, m, cfg, sd = build(logp_ref.CASES[name][0], "fp32")
    d_g, d_l, d_x = _distances(_generic(m, name), name)
    print(f"[parity] generic logp sampler {name} [fp32]: logp_grad {d_g:.3e} of sum|dx|, logp {d_l:.3e}, x_end {d_x:.3e}")
    assert d_g <= 1e-4 and d_l <= 1e-4 and d_x <= 1e-4


@pytest.mark.parametrize("name", list(logp_ref.CASES))
@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_fused_solve_within_the_generic_paths_distance_16_bit(name, precision):
    """bf16 / fp16 operands: the fused solve and the generic Python sampler at the same precision run the same forward and backward
    kernels on the same probes and may differ only in how the per-row dot and the blend are summed (fp32 summation error), so the
    fused solve's distance to the fp32 fixture may be at most 1.5 x the generic path's own (the factor of the project's operand-class
    gates) - for every logp_grad, logp and x_end.
    Measured on MI355X, worst distance fused | generic (profiles/logp_bench.txt has every line):
      bf16  logp_grad 9.5e-4 .. 1.49e-3 | the same to four digits;  logp 2.7e-4 .. 3.7e-4 | the same (me2: 3.192e-4 | 3.195e-4);
            x_end 3.0e-3 .. 4.7e-3 | the same
      fp16  logp_grad 1.70e-4 .. 3.28e-4 | 1.79e-4 .. 3.10e-4 (ratios 0.86 .. 1.15);  logp 3.2e-5 .. 6.9e-5 | 3.0e-5 .. 6.8e-5
            (ratios 0.71 .. 1.06);  x_end 4.7e-4 .. 6.9e-4 | the same"""
    g, m, cfg, sd = build(logp_ref.CASES[name][0], precision)
    d_f, d_g = _distances(_fused(m, name), name), _distances(_generic(m, name), name)
    for what, a, b in zip(("logp_grad", "logp", "x_end"), d_f, d_g):
        print(f"[class] {name} [{precision}] {what}: fused {a:.4e}  generic {b:.4e}  ratio {a / b:.3f}")
    for what, a, b in zip(("logp_grad", "logp", "x_end"), d_f, d_g):
        assert a <= 1.5 * b, (name, precision, what, a, b)


# ---------------------------------------------------------------------------------------------------------------- the solve = its pieces
def _f32(v):
    return np.float32(v)


def _lin01(i, steps):
    step = _f32(1) / _f32(steps - 1)
    return step * _f32(i) if i < steps // 2 else _f32(1) - step * _f32(steps - i - 1)


def _fma(a, b, c):
    """fp32 fma(a, b, c) of a python float a and fp32 tensors: the product of two fp32 values is exact in float64."""
    return (b.double() * float(a) + c.double()).float()


def _row_sum_fixed(p):
    """The kernels' per-row sum of a (R, e) fp32 array: lane l adds the four elements of its groups l, l + 64, ... in order, then a
    butterfly over the 64 lanes."""
    R, e = p.shape
    acc = torch.zeros(R, 64, device=p.device)
    g = p.view(R, e // 4, 4)
    for c4 in range(0, e // 4, 64):
        blk = g[:, c4:c4 + 64]
        for i in range(4):
            acc[:, :blk.shape[1]] = acc[:, :blk.shape[1]] + blk[:, :, i]
    lanes = torch.arange(64, device=p.device)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ o]
    return acc[:, 0]


@pytest.mark.parametrize("method", ["euler", "heun"])
def test_fused_solve_equals_its_pieces(method):
    """scldm_logp_ode with a given probe against a Python loop of the evaluation's rows through DiT.input_vjp (the recording forward +
    scldm_dit_train_backward_dx) and torch state arithmetic in the kernels' operation order.  Every product and sum of the kernels is
    rounded on its own, except the CFG blend u + s (c - u), which is cfg_blend_kernel's contracted statement (one fma): the loop forms
    that fma in float64 (exact product, one rounding to fp32 barring a double-rounding tie).  Bit for bit."""
    g, m, cfg, sd = build("dit_base", "bf16")
    B, steps, s_cfg = 3, 2, 1.5
    gen = torch.Generator().manual_seed(41)
    z0 = torch.randn(B, 16, 16, generator=gen)
    lab = torch.randint(0, 14, (B,), generator=gen).cuda()
    n_ev = steps * (2 if method == "heun" else 1)
    probe = (torch.randint(2, (n_ev, 2 * B, 16, 16), generator=gen) * 2 - 1).float().cuda()
    z2 = torch.cat([z0, z0]).cuda()
    logp, z_end, trace = m.log_likelihood_cfg(z2, {"clusters": torch.cat([lab, lab])}, {"clusters": s_cfg}, steps + 1, method, probe=probe,
                                              return_trace=True)
    # ---- the pieces
    cond = {"clusters": torch.cat([torch.full((2 * B,), 14, device="cuda"), lab])}       # null token on the unconditional rows
    coef_u = _f32(1) - _f32(s_cfg)
    e = 256

    def evaluate(x, s, ev):
        ep = probe[ev]
        xin = torch.cat([x, x[B:]])
        dout = torch.cat([ep[:B] * 1.0, ep[B:] * float(coef_u), ep[B:] * float(_f32(s_cfg))])
        tv = torch.full((3 * B,), float(_f32(1) - s), device="cuda")
        out, dx = m.input_vjp(xin, tv, cond, dout)
        u = out[B:2 * B]
        v = torch.cat([out[:B], _fma(_f32(s_cfg), out[2 * B:] - u, u)])
        d = torch.cat([dx[:B], dx[B:2 * B] + dx[2 * B:]])
        return -v, _row_sum_fixed((ep * d).reshape(2 * B, e))

    z, dl, lgs, ev = z2.clone(), torch.zeros(2 * B, device="cuda"), [], 0
    for i in range(steps):
        s0, s1 = _lin01(i, steps + 1), _lin01(i + 1, steps + 1)
        hs = float(s1 - s0)
        k1v, k1l = evaluate(z, s0, ev)
        ev += 1
        lgs.append(k1l)
        if method == "euler":
            z, dl = z + k1v * hs, dl + k1l * hs
        else:
            k2v, k2l = evaluate(z + k1v * hs, s1, ev)
            ev += 1
            lgs.append(k2l)
            hh = float(_f32(0.5) * _f32(hs))
            z, dl = z + (k1v + k2v) * hh, dl + (k1l + k2l) * hh
    c0 = float(_f32(-0.5 * e * math.log(2.0 * math.pi)))
    want = (c0 - _row_sum_fixed((z * z).reshape(2 * B, e)) * 0.5) - dl
    assert torch.isfinite(logp).all()
    assert torch.equal(trace, torch.stack(lgs))
    assert torch.equal(z_end, z)
    assert torch.equal(logp, want)


# ---------------------------------------------------------------------------------------------------------------- generator, shards, graph
def test_probe_values_and_row_addressing():
    from scldm_amd import _lib

    def probe(n_rows, e, seed, ev, half=0, cell_offset=0, cells_total=None):
        out = torch.empty(n_rows, e, device="cuda")
        _lib.check(_lib.lib().scldm_logp_probe(out.data_ptr(), n_rows, e, seed, ev, half, cell_offset, n_rows + cell_offset if cells_total is None else cells_total,
                                               torch.cuda.current_stream().cuda_stream), "scldm_logp_probe")
        return out

    rows, e, seed = 1024, 256, 0x10CA11
    a = probe(rows, e, seed, 0)
    assert set(a.unique().tolist()) == {-1.0, 1.0}
    n = rows * e
    assert abs(float(a.double().mean())) < 5 / math.sqrt(n)                                    # five sigma of a fair +-1 sample
    x = a.double().flatten()
    b, h1 = probe(rows, e, seed, 1).double().flatten(), probe(rows, e, seed, 0, half=1, cells_total=rows).double().flatten()
    for other in (x[1:] * x[:-1], x * b, x * h1):                                                # lag-1, cross-evaluation, cross-half
        assert abs(float(other.mean())) < 5 / math.sqrt(n)
    assert not torch.equal(a, probe(rows, e, seed + 1, 0))
    assert torch.equal(probe(100, e, seed, 0, cell_offset=500, cells_total=rows), a[500:600])    # a shard = the slice of the whole
    odd = probe(7, 12, seed, 3, half=1, cell_offset=5, cells_total=40)                           # narrow rows, second half, partial workgroup
    assert torch.equal(odd, probe(40, 12, seed, 3, half=1, cells_total=40)[5:12])


@pytest.mark.parametrize("method", ["euler", "heun"])
def test_seed_reproduces_and_is_the_probe_of_scldm_logp_probe(method):
    g, m, cfg, sd = build("dit_base", "bf16")
    f, z2, cond, scales, _ = _inputs("logp_base_euler")
    steps, B = 3, z2.shape[0] // 2
    a = m.log_likelihood_cfg(z2, cond, scales, steps, method, seed=1234, return_trace=True)
    b = m.log_likelihood_cfg(z2, cond, scales, steps, method, seed=1234, return_trace=True)
    n_ev = (steps - 1) * (2 if method == "heun" else 1)
    probe = torch.stack([m.logp_probe(1234, ev, B) for ev in range(n_ev)])
    c = m.log_likelihood_cfg(z2, cond, scales, steps, method, probe=probe, return_trace=True)
    d = m.log_likelihood_cfg(z2, cond, scales, steps, method, seed=1235, return_trace=True)
    assert all(torch.isfinite(v).all() for v in a)
    for k in range(3):
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k])
    assert not torch.equal(a[2], d[2]) and not torch.equal(a[0], d[0])


def test_shards_of_a_solve_draw_the_whole_solves_probes():
    """5 cells solved whole are bit-equal to the shards [0, 3) + [3, 5) with cell_offset / cells_total (cells are independent, and a
    cell's probe does not depend on the batch it is solved in)."""
    g, m, cfg, sd = build("dit_base", "bf16")
    gen = torch.Generator().manual_seed(19)
    x = torch.randn(5, 16, 16, generator=gen).cuda()
    lab = torch.randint(0, 14, (5,), generator=gen).cuda()
    scales = {"clusters": 1.5}
    kw = dict(num_steps=3, sampling_method="heun", seed=77, return_trace=True)
    whole = m.log_likelihood_cfg(torch.cat([x, x]), {"clusters": torch.cat([lab, lab])}, scales, **kw)
    assert all(torch.isfinite(v).all() for v in whole)
    for lo, hi in ((0, 3), (3, 5)):
        part = m.log_likelihood_cfg(torch.cat([x[lo:hi], x[lo:hi]]), {"clusters": torch.cat([lab[lo:hi], lab[lo:hi]])}, scales, cell_offset=lo,
                                    cells_total=5, **kw)
        rows = torch.cat([torch.arange(lo, hi), 5 + torch.arange(lo, hi)]).cuda()
        assert torch.equal(part[0], whole[0][rows]) and torch.equal(part[1], whole[1][rows]) and torch.equal(part[2], whole[2][:, rows])
    alone = m.log_likelihood_cfg(torch.cat([x[3:], x[3:]]), {"clusters": torch.cat([lab[3:], lab[3:]])}, scales, **kw)   # offset 0: other probes
    assert not torch.equal(alone[0], whole[0][torch.tensor([3, 4, 8, 9]).cuda()])


def test_graph_replay_equals_the_eager_solve():
    """The solve is launches only: captured once (fp32 on the fused shape = the single-stream GEMM route, so the captured graph has no
    parallel branches) after an eager warm-up, one replay writes what the eager call returned."""
    g, m, cfg, sd = build("dit_me2_256", "fp32")
    f, z2, cond, scales, (method, steps) = _inputs("logp_me2_euler")
    kw = dict(num_steps=steps + 1, sampling_method=method, seed=5, return_trace=True)
    eager = m.log_likelihood_cfg(z2, cond, scales, **kw)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = m.log_likelihood_cfg(z2, cond, scales, **kw)
    for v in out:
        v.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, out):
        assert torch.isfinite(b).all() and torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------- error paths
def test_rejected_arguments_launch_nothing():
    import ctypes as C
    from scldm_amd import _lib
    g, m, cfg, sd = build("dit_base", "fp32")
    f, z2, cond, scales, _ = _inputs("logp_base_euler")
    with pytest.raises(ValueError):
        m.log_likelihood_cfg(z2, cond, scales, 1, "euler")
    with pytest.raises(NotImplementedError):
        m.log_likelihood_cfg(z2, cond, scales, 4, "rk4")
    with pytest.raises(ValueError):
        m.log_likelihood_cfg(z2, cond, scales, 4, "euler", cell_offset=2, cells_total=4)
    with pytest.raises(ValueError):
        m.log_likelihood_cfg(z2[:5], cond, scales, 4, "euler")
    with pytest.raises(ValueError):
        m.log_likelihood_cfg(z2, cond, scales, 4, "euler", probe=torch.ones(2, *z2.shape, device="cuda"))
    with pytest.raises(ValueError):
        m.logp_probe(1, 0, 3, cell_offset=2, cells_total=4)
    # the C ABI itself: SCLDM_ERR_SHAPE with a message, the state untouched
    L, h = m._native_handle()
    w, _ = m._weights_struct(tuple(m.parameters()))
    before = z2.clone()
    saved = torch.empty(L.scldm_dit_train_saved_bytes_for(h, 6, 0), dtype=torch.uint8, device="cuda")
    ws = torch.empty(L.scldm_logp_workspace_bytes(h, 3, 0, 0), dtype=torch.uint8, device="cuda")
    logp = torch.zeros(6, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call(n_steps=3, method=0, cell_offset=0, cells_total=3, z=None):
        return L.scldm_logp_ode(h, C.byref(w), before.data_ptr() if z is None else z, None, 0, None, 3, 0, None, None, n_steps, method, None, 1,
                                cell_offset, cells_total, logp.data_ptr(), None, 0, saved.data_ptr(), ws.data_ptr(), st)

    for what, rc in (("no steps", call(n_steps=0)), ("unknown method", call(method=2)), ("cells_total too small", call(cell_offset=1)),
                     ("null z", call(z=0))):
        assert rc == -1 and L.scldm_last_error(), what
    torch.cuda.synchronize()
    assert torch.equal(before, z2) and float(logp.abs().max()) == 0.0
    assert call() == 0      # the same call with valid arguments runs (no condition: both halves unconditional, on their own probes)
    torch.cuda.synchronize()
    assert torch.isfinite(logp).all() and not torch.equal(before, z2) and not torch.equal(logp[:3], logp[3:])

"""GPU tests of the DiT kernels at SwiGLU hidden widths other than the 684 that multiple_of=4 gives at n_embed 256 (every other DiT test
on the GPU).  The hidden width H steers the chunk layout of the fused forward (api.hip: whole 128-unit chunks + an optional trailing
64-unit chunk, zero-padded units), the weight packers (dit_aux.hpp), the 16x16 MFMA passes of the up- and down-projection, the operand
arrays of the fused training route (padded to 768; H <= 768 and H % 4 == 0) and the padded rows of the generic bf16-source route:

    H     multiple_of  fused forward layout                                  training route
    768   256          6 chunks, no half chunk, no padding                   fused (three exact 256-unit backward chunks)
    704   64           5 chunks + half chunk, no padding                     fused
    700   100          5 chunks + half chunk, 4 padded units                 fused (weight-gradient M = 700: ragged 128-row tile)
    832   832          6 chunks + half chunk, no padding                     generic GEMM route (H > 768): the hand-over
    682   2            5 chunks + half chunk, 22 padded units                refused (H % 4 != 0)
    685   5            as 682, odd width (forward only, against the oracle)  refused
    1024  1024         8 chunks, no half chunk (forward only)                -
    720   720          6 chunks, 48 padded units in a WHOLE chunk, across    (forward only)
                       three waves' 16-unit slices of the two-tile kernels
    1366 / 1380 at n_embed 512 (multiple_of 2 / 20): the generic path, refused / H % 8 == 4 (rows padded to a multiple of 8)

Fixtures from the reference: tests/golden/dit_h<H>.npz (make_golden_hidden.py, two layers, three cells).  No tolerance is new: every
comparison uses a gate of tests/test_gpu_dit.py, test_gpu_train.py, test_gpu_logp.py or test_gpu_wide_infer.py, against the oracle or
the reference fixture; comparisons of one kernel route with another are bitwise.  Which one-line corruption of the hidden-width handling
each test catches: profiles/hidden_widths_mutations.txt; the figures of a run: profiles/hidden_widths_gpu_tests.txt."""
import numpy as np
import pytest
import torch

import logp_ref
from conftest import check_err, golden_json, max_abs_rel
from oracle.dit import DiTConfig, dit_forward, dit_forward_with_cfg
from oracle.train import FROZEN
from oracle.transport import sample_ode_fixed
from oracle.weights import make_state_dict
from precision_class import class_error, class_gate, distances, exact_result, gate_tensor, oracle_grads, train_case
from test_gpu_dit import BITS, FLOOR_TOL, PARITY, SIXTEEN, TOL_BF16, TOL_FP32, build, cu
from test_gpu_train import hip_training_step

pytestmark = pytest.mark.gpu

GOLDEN = {768: "dit_h768", 704: "dit_h704", 700: "dit_h700", 832: "dit_h832", 682: "dit_h682"}
VOCAB = {"clusters": 14}
COMMON = dict(dropout=0.0, bias=True, norm_layer="layernorm", layernorm_eps=1e-8, cfg_dropout_prob=0.8)


def make(multiple_of, precision="fp32", n_layer=2, n_embed=256, n_head=8, seed=None, vocab=VOCAB, strategy="mutually_exclusive"):
    """A model without a reference fixture (the oracle is its reference): (module in eval mode, oracle config, state dict)."""
    from scldm_amd.layers import swiglu_hidden
    from scldm_amd.nnets import DiT
    m = DiT(n_embed=n_embed, n_embed_input=16, n_layer=n_layer, n_head=n_head, seq_len=16, multiple_of=multiple_of,
            class_vocab_sizes=vocab, condition_strategy=strategy, **COMMON)
    sd = make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, 500 + multiple_of + n_layer if seed is None else seed)
    m.load_state_dict(sd, strict=True)
    assert tuple(sd["blocks.0.mlp.w1.weight"].shape) == (swiglu_hidden(n_embed, multiple_of), n_embed)
    m = m.cuda().eval()
    m.precision = precision
    cfg = DiTConfig(n_embed=n_embed, n_head=n_head, n_layer=n_layer, multiple_of=multiple_of, class_vocab_sizes=vocab,
                    condition_strategy=strategy)
    return m, cfg, sd


def trainable(m):
    m.train()
    m.cfg_dropout_prob = 0.0     # deterministic labels (the null rows of the tables stay: built with 0.8)
    return m


def with_env(monkeypatch, builder, **env):
    """builder() with run-time knobs set, which the lazily created native handle reads once."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = builder()
    m._native_handle()
    for k in env:
        monkeypatch.delenv(k)
    return m


def cells(n, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(n, 16, 16, device="cuda", generator=gen)
    t = torch.rand(n, device="cuda", generator=gen)
    return x, t, {"clusters": torch.randint(0, 14, (n,), device="cuda", generator=gen)}


def fused_training_route(m, n, precision):
    """True when the library serves a training step of n cells on the fused route (its record is the small one)."""
    from scldm_amd import _lib
    L, h = m._native_handle()
    return L.scldm_dit_train_saved_bytes_for(h, n, _lib.PRECISIONS[precision]) < L.scldm_dit_train_saved_bytes(h, n) / 4


# ---- a. forward and CFG forward against the reference fixtures ----------------------------------------------------------------------------
@pytest.mark.parametrize("H", sorted(GOLDEN))
@pytest.mark.parametrize("precision,tol", PARITY + SIXTEEN)
def test_forward_and_cfg_forward_match_reference_golden(H, precision, tol):
    g, m, cfg, sd = build(GOLDEN[H], precision)
    assert int(g["hidden"]) == H and tuple(m.blocks[0].mlp.w1.weight.shape) == (H, 256)
    x, t, lab = torch.from_numpy(g["fwd_x"]), torch.from_numpy(g["fwd_t"]), {"clusters": torch.from_numpy(g["fwd_label_clusters"])}
    y = m(x.cuda(), t.cuda(), {"clusters": lab["clusters"].cuda()})
    assert y.shape == g["fwd_out"].shape and torch.isfinite(y).all()
    check_err(y.cpu(), g["fwd_out"], tol, f"forward H={H} [{precision}] vs reference golden", FLOOR_TOL[precision])
    xc, tc = torch.from_numpy(g["cfg_x"]), torch.from_numpy(g["cfg_t"])
    cc = {"clusters": torch.from_numpy(g["cfg_label_clusters"])}
    scales = golden_json(g, "cfg_scales_s2")
    m.detect_uniform_t = False
    y2 = m.forward_with_cfg(xc.cuda(), tc.cuda(), {"clusters": cc["clusters"].cuda()}, scales)          # per-sample rows
    check_err(y2.cpu(), g["cfg_out_s2"], tol, f"forward_with_cfg H={H} [{precision}] per-sample t", FLOOR_TOL[precision])
    m.detect_uniform_t = True
    y3 = m.forward_with_cfg(xc.cuda(), tc.cuda(), {"clusters": cc["clusters"].cuda()}, scales)          # shared rows
    check_err(y3.cpu(), g["cfg_out_s2"], tol, f"forward_with_cfg H={H} [{precision}] dense uniform t", FLOOR_TOL[precision])
    if precision in BITS:
        gate_tensor(y.cpu(), g["fwd_out"], lambda: dit_forward(sd, cfg, x, t, lab), BITS[precision], f"forward H={H} vs reference golden",
                    tag=f"hidden_fwd/{H}")
        fn = lambda: dit_forward_with_cfg(sd, cfg, xc, tc, cc, scales)
        for path, out in (("per-sample t", y2), ("dense uniform t", y3)):
            gate_tensor(out.cpu(), g["cfg_out_s2"], fn, BITS[precision], f"forward_with_cfg H={H} {path}", tag=f"hidden_cfg/{H}")


# ---- b. ragged batches against the oracle -------------------------------------------------------------------------------------------------
def _ragged(m, cfg, sd, what, n, precision, tol):
    rng = np.random.default_rng(1000 + n)
    x = rng.standard_normal((n, 16, 16)).astype(np.float32)
    t = rng.uniform(0, 1, n).astype(np.float32)
    lab = rng.integers(0, 14, n).astype(np.int64)
    fn = lambda: dit_forward(sd, cfg, torch.from_numpy(x), torch.from_numpy(t), {"clusters": torch.from_numpy(lab)})
    ref = exact_result(fn, f"hidden_ragged/{what}/{n}")
    y = m(cu(x), cu(t), {"clusters": cu(lab)})
    assert torch.isfinite(y).all()
    check_err(y.cpu(), ref, tol, f"ragged {what} n={n} [{precision}] vs oracle", FLOOR_TOL[precision])
    if precision in BITS:
        gate_tensor(y.cpu(), ref, fn, BITS[precision], f"ragged {what} n={n} vs oracle", tag=f"hidden_ragged/{what}/{n}")


@pytest.mark.parametrize("H", sorted(GOLDEN))
@pytest.mark.parametrize("precision,tol", PARITY + SIXTEEN)
def test_ragged_batches_vs_oracle(H, precision, tol):
    """1 cell (a padded 32-token tile), 5 and 9 cells (ragged tiles; 9 fills more than one 64-token tile)."""
    g, m, cfg, sd = build(GOLDEN[H], precision)
    for n in (1, 5, 9):
        _ragged(m, cfg, sd, f"H={H}", n, precision, tol)


@pytest.mark.parametrize("multiple_of,H", [(1024, 1024), (5, 685), (720, 720)])
@pytest.mark.parametrize("precision,tol", PARITY + SIXTEEN)
def test_ragged_batches_vs_oracle_eight_chunks_and_an_odd_width(multiple_of, H, precision, tol):
    """Forward only: 8 whole chunks without a half chunk (more than the 5 of every other test), an odd hidden width, and padded units
    inside a whole chunk of the two-tile stream (at 684 / 700 / 685 they sit in the trailing half chunk, at 768 / 704 / 832 there are none)."""
    m, cfg, sd = make(multiple_of, precision)
    assert tuple(m.blocks[0].mlp.w1.weight.shape) == (H, 256) and m.fused_shape
    for n in (1, 5, 9):
        _ragged(m, cfg, sd, f"H={H}", n, precision, tol)


# ---- c. kernel-route identities (bitwise) -------------------------------------------------------------------------------------------------
ROUTE_H = [768, 704, 832]


@pytest.mark.parametrize("H", ROUTE_H)
@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_mfma16_forward_matches_the_all_32x32_form(H, precision, monkeypatch):
    """SCLDM_FWD_MFMA=32 against the default 16x16 passes: 1 / 9 cells (32-token tiles) and 513 (64-token tiles, ragged)."""
    mk = lambda: build(GOLDEN[H], precision)[1]
    m16, m32 = with_env(monkeypatch, mk), with_env(monkeypatch, mk, SCLDM_FWD_MFMA="32")
    for n in (1, 9, 513):
        x, t, lab = cells(n, 91 + n)
        with torch.no_grad():
            y16, y32 = m16(x, t, lab), m32(x, t, lab)
        assert torch.isfinite(y16).all() and float(y16.abs().max()) > 0
        assert torch.equal(y16, y32), (n, float((y16 - y32).abs().max() / y32.abs().max()))


@pytest.mark.parametrize("H", [768, 704])      # (832 trains on the generic route: no recording forward of the fused kernel)
@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_mfma16_recording_forward_gives_the_same_training_step(H, precision, monkeypatch):
    n = 8
    x1, x0, t, cond = train_case(n, 23, VOCAB)
    monkeypatch.setenv("SCLDM_TRAIN_FUSED", "1")
    res = {}
    for knob in (None, "32"):
        m = trainable(with_env(monkeypatch, lambda: build(GOLDEN[H], precision)[1], **({"SCLDM_FWD_MFMA": knob} if knob else {})))
        assert fused_training_route(m, n, precision)
        terms = hip_training_step(m, x1, x0, t, cond)
        res[knob] = (terms["loss"].detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None})
    (loss16, g16), (loss32, g32) = res[None], res["32"]
    assert torch.isfinite(loss16).all() and len(g16) == len(g32) > 0 and torch.equal(loss16, loss32)
    for k in g16:
        assert torch.equal(g16[k], g32[k]), k


@pytest.mark.parametrize("H", ROUTE_H)
@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_32_and_64_token_tiles_give_the_same_bits(H, precision, monkeypatch):
    mk = lambda: build(GOLDEN[H], precision)[1]
    m, m64 = with_env(monkeypatch, mk), with_env(monkeypatch, mk, SCLDM_SMALL_NTT="0")
    x, t, lab = cells(9, 31)
    with torch.no_grad():
        y = m(x, t, lab)
        assert torch.isfinite(y).all() and torch.equal(y, m64(x, t, lab))


@pytest.mark.parametrize("H,multiple_of", [(768, 256), (704, 64), (832, 832)])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_launch_groupings_of_a_three_layer_model_give_the_same_bits(H, multiple_of, precision, monkeypatch):
    """Three layers in one launch (the default) against one and two layers per launch: the next layer's weights start at a per-wave
    offset and a per-layer stride that come from the chunk count; and two tile groups against one.  The default against the oracle."""
    mk = lambda: make(multiple_of, precision, n_layer=3)[0]
    m, cfg, sd = make(multiple_of, precision, n_layer=3)
    assert tuple(m.blocks[2].mlp.w1.weight.shape) == (H, 256)
    x, t, lab = cells(9, 12)
    with torch.no_grad():
        ref = m(x, t, lab)
        fn = lambda: dit_forward(sd, cfg, x.cpu(), t.cpu(), {"clusters": lab["clusters"].cpu()})
        exact = exact_result(fn, f"hidden_lpl/{H}")
        check_err(ref.cpu(), exact, TOL_FP32 if precision == "fp32" else TOL_BF16, f"3-layer model H={H} [{precision}] vs oracle", FLOOR_TOL[precision])
        if precision == "bf16":
            gate_tensor(ref.cpu(), exact, fn, 7, f"3-layer model H={H} vs oracle", tag=f"hidden_lpl/{H}")
        for knob, val in (("SCLDM_LPL", "1"), ("SCLDM_LPL", "2"), ("SCLDM_GROUPS", "2")):
            y = with_env(monkeypatch, mk, **{knob: val})(x, t, lab)
            assert torch.equal(y, ref), (knob, val, float((y - ref).abs().max()))
        big = cells(300, 13)                          # enough tiles for two groups (9 cells are one group's)
        y1, y2 = m(*big), with_env(monkeypatch, mk, SCLDM_GROUPS="2")(*big)
        assert torch.isfinite(y1).all() and torch.equal(y1, y2)


# ---- d. fused sampler ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [768, 832])
@pytest.mark.parametrize("precision,tol", PARITY + SIXTEEN)
def test_fused_sampler_vs_oracle(H, precision, tol):
    g, m, cfg, sd = build(GOLDEN[H], precision)
    rng = np.random.default_rng(11)
    B, steps, scales = 3, 4, {"clusters": 2.0}
    z0 = rng.standard_normal((B, 16, 16)).astype(np.float32)
    lab = rng.integers(0, 14, B).astype(np.int64)
    z2 = torch.from_numpy(np.concatenate([z0, z0]))
    cond2 = {"clusters": torch.from_numpy(np.concatenate([lab, lab]))}
    fn = lambda: sample_ode_fixed(z2, lambda x, t: dit_forward_with_cfg(sd, cfg, x, t, cond2, scales), steps, "euler")
    ref = exact_result(fn, f"hidden_sampler/{H}")
    out = m.sample_ode_cfg(z2.cuda(), {"clusters": cond2["clusters"].cuda()}, scales, steps, "euler")
    check_err(out.cpu(), ref, tol, f"fused sampler H={H} euler x{steps} [{precision}] vs oracle", FLOOR_TOL[precision])
    if precision in BITS:
        gate_tensor(out.cpu(), ref, fn, BITS[precision], f"fused sampler H={H} euler x{steps} vs oracle", tag=f"hidden_sampler/{H}")


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_fused_dopri5_solve_is_bit_identical_to_the_composed_route(precision, monkeypatch):
    from test_gpu_dopri5_fused import _assert_identical, _inputs, _three_way
    monkeypatch.setenv("SCLDM_DOPRI5_FUSED", "1")
    g, m, cfg, sd = build(GOLDEN[768], precision)
    z2, cond, scales = _inputs(m, g, 3, "scale2", 43)
    dt0, new, st_new, ref, st_ref = _three_way(m, z2, cond, scales, 1e-5)
    assert st_new["first_step"] == dt0 and torch.equal(new[0], z2)
    _assert_identical(new, st_new, ref, st_ref, f"H=768 B=3 [{precision}]")


# ---- e. fused training at H <= 768 --------------------------------------------------------------------------------------------------------
def _train_inputs(n):
    return train_case(n, 9, VOCAB)


def _exact_grads(H, n, sd, cfg):
    x1, x0, t, cond = _train_inputs(n)
    return exact_result(lambda: oracle_grads(sd, cfg, x1, x0, t, cond), f"hidden_train/{H}/{n}")


def _training_step_vs_oracle(H, n, precision, expect_fused):
    """One training step against autograd over the fp32 oracle: bf16 under the flat 3e-2 and the class gate of
    test_bf16_training_gradients_close_to_fp32_oracle, fp16 under the per-tensor bound of
    test_fp16_training_is_in_the_references_tf32_class (1.5 x the TF32-operand oracle + 1e-5)."""
    g, m, cfg, sd = build(GOLDEN[H], precision)
    trainable(m)
    assert fused_training_route(m, n, precision) == expect_fused
    x1, x0, t, cond = _train_inputs(n)
    terms = hip_training_step(m, x1, x0, t, cond)
    exact = _exact_grads(H, n, sd, cfg)
    ours = {"pred": terms["pred"].detach().cpu()}
    for name, p in m.named_parameters():
        if name not in FROZEN:
            assert p.grad is not None and torch.isfinite(p.grad).all(), name
            ours[name] = p.grad.cpu()
    got = distances(ours, exact)
    assert set(got) == set(exact)
    bits = BITS[precision]
    cls = class_error(lambda: oracle_grads(sd, cfg, x1, x0, t, cond), bits, exact, per="tensor", tag=f"hidden_train/{H}/{n}")
    what = f"{precision} training step H={H}, {n} cells x 2 layers, {'fused' if expect_fused else 'generic'} route vs oracle autograd"
    if precision == "bf16":
        flat = dict(got, pred=max_abs_rel(ours["pred"], exact["pred"]))
        bad = {k: v for k, v in flat.items() if not v < 3e-2}
        assert not bad, bad
        class_gate(got, cls, what)
    else:
        print(f"[parity] {what}: worst gradient rel-L2 {max(got.values()):.2e}, TF32-operand oracle {max(cls.values()):.2e}")
        bad = {k: (v, cls[k]) for k, v in got.items() if not v <= 1.5 * cls[k] + 1e-5}
        assert not bad, bad
    return m, ours


@pytest.mark.parametrize("H", [768, 704, 700])
@pytest.mark.parametrize("n", [5, 8])
@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_fused_training_gradients_vs_oracle(H, n, precision, monkeypatch):
    monkeypatch.setenv("SCLDM_TRAIN_FUSED", "1")
    _training_step_vs_oracle(H, n, precision, expect_fused=True)


@pytest.mark.parametrize("H", [768, 704, 700])
def test_fused_training_path_is_taken_and_agrees_with_the_generic_bf16_path(H, monkeypatch):
    n = 8
    x1, x0, t, cond = _train_inputs(n)
    grads = {}
    for fused in (True, False):
        m = trainable(with_env(monkeypatch, lambda: build(GOLDEN[H], "bf16")[1], SCLDM_TRAIN_FUSED="1" if fused else "0"))
        assert fused_training_route(m, n, "bf16") == fused
        hip_training_step(m, x1, x0, t, cond)
        grads[fused] = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    worst = {k: float((grads[True][k].double() - grads[False][k].double()).norm() / grads[False][k].double().norm()) for k in grads[True]}
    bad = {k: v for k, v in worst.items() if not v < 2e-2}
    assert not bad, bad
    assert max(worst.values()) > 0.0      # two different code paths


def _fp32_step_vs_oracle(H, n):
    g, m, cfg, sd = build(GOLDEN[H], "fp32")
    trainable(m)
    x1, x0, t, cond = _train_inputs(n)
    terms = hip_training_step(m, x1, x0, t, cond)
    exact = _exact_grads(H, n, sd, cfg)
    assert max_abs_rel(terms["pred"].detach().cpu(), exact["pred"]) < TOL_FP32
    bad = {}
    for name, p in m.named_parameters():
        if name in FROZEN:
            assert p.grad is None
            continue
        e = max_abs_rel(p.grad.cpu(), exact[name])
        if not e < TOL_FP32:
            bad[name] = e
    assert not bad, bad


def test_fp32_training_gradients_vs_oracle_at_768():
    _fp32_step_vs_oracle(768, 5)


def _input_vjp_vs_training_backward_and_oracle(H, precision, n):
    """dx of DiT.input_vjp: bit for bit the training backward's (tests/test_gpu_logp.py: vjp_pair), and with the end-layer gradients
    against the oracle as test_fused_training_input_gradient_matches_oracle gates them."""
    from test_gpu_logp import vjp_pair
    y, dx_full, y2, dx = vjp_pair(GOLDEN[H], precision, n)
    assert torch.isfinite(dx).all() and float(dx.abs().max()) > 0
    assert torch.equal(y, y2)
    assert torch.equal(dx, dx_full), float((dx - dx_full).abs().max() / dx_full.abs().max())
    g, m, cfg, sd = build(GOLDEN[H], precision)
    trainable(m)
    m.pos_embed.requires_grad_(True)
    gen = torch.Generator().manual_seed(6)
    x, t = torch.randn(n, 16, 16, generator=gen), torch.rand(n, generator=gen)
    lab = torch.randint(0, 14, (n,), generator=gen)
    wgt = torch.randn(n, 16, 16, generator=gen)
    xg = x.cuda().requires_grad_(True)
    (m(xg, t.cuda(), {"clusters": lab.cuda()}, force_drop_ids=False) * wgt.cuda()).sum().backward()
    names = ("pos_embed", "input_proj.weight", "input_proj.bias", "final_layer.linear.weight", "final_layer.linear.bias")

    def oracle():
        p = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
        xo = x.clone().requires_grad_(True)
        (dit_forward(p, cfg, xo, t, {"clusters": lab}) * wgt).sum().backward()
        return {"x": xo.grad, **{k: p[k].grad for k in names}}
    exact = oracle()
    got = distances({"x": xg.grad.cpu(), **{k: dict(m.named_parameters())[k].grad.cpu() for k in names}}, exact)
    assert set(got) == set(exact)
    if precision == "fp32":
        bad = {k: e for k, e in got.items() if not e < TOL_FP32}
        assert not bad, bad
        return
    for name, e in got.items():
        assert e < 3e-2, (name, e)
    class_gate(got, class_error(oracle, 7, exact, per="tensor"), f"input / pos_embed / end-layer gradients H={H}, {n} cells")


@pytest.mark.parametrize("n", [8, 7])
def test_input_vjp_at_768(n, monkeypatch):
    monkeypatch.setenv("SCLDM_TRAIN_FUSED", "1")
    _input_vjp_vs_training_backward_and_oracle(768, "bf16", n)


# ---- f. the route hand-over at H = 832 (a fused inference shape whose training runs on the generic route) ----------------------------------
@pytest.mark.parametrize("n", [5, 8])
@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_training_beyond_768_runs_on_the_generic_route_in_its_class(n, precision):
    """bf16: the generic bf16 GEMM route under the bf16 gates.  fp16: the library serves it with the exact-fp32 route (train_api.hip:
    train_precision) - more precise than the class it is held to here, never less."""
    m, ours = _training_step_vs_oracle(832, n, precision, expect_fused=False)
    assert m.fused_shape and not m.fused_train_shape


def test_fp32_training_gradients_vs_oracle_at_832():
    _fp32_step_vs_oracle(832, 5)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_input_vjp_at_832(precision):
    _input_vjp_vs_training_backward_and_oracle(832, precision, 7)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_log_likelihood_at_832_matches_the_generic_sampler(precision):
    """scldm_logp_ode (one C call; its evaluations run the generic training forward and the input-gradient-only backward here) against the
    Python Sampler.sample_ode_likelihood over differentiable forwards on the same probes, both against the CPU restatement over the
    oracle: fp32 inside the project's 1e-4 (tests/test_gpu_logp.py: test_fused_solve_on_recorded_probes), bf16 at most 1.5 x the generic
    path's own distance (test_fused_solve_within_the_generic_paths_distance_16_bit)."""
    from scldm_amd.transport import Sampler, create_transport
    g, m, cfg, sd = build(GOLDEN[832], precision)
    B, steps, method, scales = 2, 3, "euler", {"clusters": 1.5}
    gen = torch.Generator().manual_seed(21)
    z0 = torch.randn(B, 16, 16, generator=gen)
    z2 = torch.cat([z0, z0])
    cond2 = {"clusters": torch.randint(0, 14, (B,), generator=gen).repeat(2)}
    condg = {"clusters": cond2["clusters"].cuda()}
    n_ev = steps - 1
    probes = torch.stack([m.logp_probe(0, ev, B) for ev in range(n_ev)])
    assert probes.shape == (n_ev, 2 * B, 16, 16) and bool((probes.abs() == 1).all())
    logp, z_end, trace = m.log_likelihood_cfg(z2.cuda(), condg, scales, steps, method, seed=0, return_trace=True)
    assert logp.shape == (2 * B,) and torch.isfinite(logp).all() and torch.isfinite(z_end).all() and torch.isfinite(trace).all()
    it = iter(probes)
    fn = Sampler(create_transport()).sample_ode_likelihood(sampling_method=method, num_steps=steps)
    logp_g, z_end_g = fn(z2.cuda(), lambda x, t: m._composed_forward_with_cfg(x, t.contiguous(), condg, scales), _probe=lambda x: next(it))
    trace_g = torch.stack(fn.last_trace["logp_grad"])
    r_logp, r_x, r_lgs, _, r_sc = exact_result(
        lambda: logp_ref.logp_ref(z2, lambda x, t: dit_forward_with_cfg(sd, cfg, x, t, cond2, scales), method, n_ev, probes.cpu()), "hidden_logp/832")
    sc = torch.stack(r_sc).double()

    def dist(lp, ze, tr):
        return (float(((tr.cpu().double() - torch.stack(r_lgs).double()).abs() / sc).max()), max_abs_rel(lp.cpu(), r_logp), max_abs_rel(ze.cpu(), r_x))
    d_f, d_g = dist(logp, z_end, trace), dist(logp_g, z_end_g, trace_g)
    for what, a, b in zip(("logp_grad", "logp", "x_end"), d_f, d_g):
        print(f"[parity] logp solve H=832 [{precision}] {what}: one-call solve {a:.3e}, generic sampler {b:.3e}")
        if precision == "fp32":
            assert a <= TOL_FP32 and b <= TOL_FP32, (what, a, b)
        else:
            assert a <= 1.5 * b, (what, a, b)


def test_fused_train_step_refuses_a_width_without_the_fused_training_route():
    """FusedTrainStep is documented to require the fused training route: beyond 768 hidden units it refuses with the package's message
    (naming the width) instead of running another route unannounced; at 768 it is constructed."""
    from scldm_amd.optim import AdamW
    from scldm_amd.training import FusedTrainStep
    from scldm_amd.transport import create_transport
    for H, ok in ((832, False), (682, False), (768, True)):
        g, m, cfg, sd = build(GOLDEN[H], "bf16")
        trainable(m)
        m.cfg_dropout_prob = 0.8
        assert m.fused_shape and m.fused_train_shape == ok
        opt = AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-3)
        if not ok:
            with pytest.raises(NotImplementedError, match=f"hidden width {H}"):
                FusedTrainStep(m, create_transport(), opt, 8, ["clusters"], graph=False)
            continue
        step = FusedTrainStep(m, create_transport(), opt, 8, ["clusters"], seed=3, graph=False)
        x1, _, _, cond = _train_inputs(8)
        loss = float(step(x1.cuda(), {"clusters": cond["clusters"].clamp(max=13).cuda()}))
        assert np.isfinite(loss) and loss > 0


# ---- g. widths the training path rejects --------------------------------------------------------------------------------------------------
def _training_is_refused_and_the_handle_stays_usable(m, check):
    from scldm_amd._lib import ScldmError
    x, t, lab = cells(3, 5)
    before = check()
    trainable(m)
    for prec in ("fp32", "bf16"):
        m.precision = prec
        with pytest.raises(ScldmError, match="hidden_dim"):
            m(x, t, lab, force_drop_ids=False)
        with pytest.raises(ScldmError, match="hidden_dim"):
            m.input_vjp(x, t, lab, torch.ones_like(x))
    m.eval()
    m.precision = "fp32"
    assert torch.equal(check(), before)


def test_training_refuses_682_and_the_handle_stays_usable():
    g, m, cfg, sd = build(GOLDEN[682], "fp32")

    def check():
        y = m(cu(g["fwd_x"]), cu(g["fwd_t"]), {"clusters": cu(g["fwd_label_clusters"])})
        check_err(y.cpu(), g["fwd_out"], TOL_FP32, "eval forward H=682 vs reference golden", FLOOR_TOL["fp32"])
        return y
    _training_is_refused_and_the_handle_stays_usable(m, check)


@pytest.mark.parametrize("multiple_of,H,n_embed", [(5, 685, 256), (2, 1366, 512)])
def test_training_refuses_widths_that_are_no_multiple_of_4(multiple_of, H, n_embed):
    m, cfg, sd = make(multiple_of, "fp32", n_embed=n_embed)
    assert tuple(m.blocks[0].mlp.w1.weight.shape) == (H, n_embed)
    x, t, lab = cells(3, 5)
    if n_embed == 256:      # the fused inference kernels serve the width; the eval route of a wider model is the training forward's
        def check():
            y = m(x, t, lab)
            check_err(y.cpu(), dit_forward(sd, cfg, x.cpu(), t.cpu(), {"clusters": lab["clusters"].cpu()}), TOL_FP32, f"eval forward H={H} vs oracle",
                      FLOOR_TOL["fp32"])
            return y
        _training_is_refused_and_the_handle_stays_usable(m, check)
    else:
        from scldm_amd._lib import ScldmError
        for mode in ("train", "eval"):
            getattr(m, mode)()
            with pytest.raises(ScldmError, match="hidden_dim"):
                m(x, t, lab, force_drop_ids=False)


# ---- h. the generic path with H % 8 == 4 below width 1024 ------------------------------------------------------------------------------------
WIDE = dict(multiple_of=20, n_embed=512, n_head=8, vocab={"cell_line": 4, "gene": 2024}, strategy="joint", seed=97)


@pytest.mark.parametrize("precision,n", [("fp32", 5), ("bf16", 9)])
def test_wide_model_with_padded_hidden_rows_trains_in_its_class(precision, n):
    """512 wide, H = 1380 (1380 % 8 == 4: the bf16 operand arrays pad their rows to 1384).  fp32 at 5 cells under the 1e-4 gate; bf16 at 9
    cells = 144 tokens (the bf16-source route is on from 128) under the gates of test_wider_shapes_bf16_sources_close_to_fp32_oracle."""
    m, cfg, sd = make(precision=precision, **WIDE)
    assert tuple(m.blocks[0].mlp.w1.weight.shape) == (1380, 512) and not m.fused_shape
    trainable(m)
    x1, x0, t, cond = train_case(n, 512 + n, WIDE["vocab"])
    terms = hip_training_step(m, x1, x0, t, cond)
    fn = lambda: oracle_grads(sd, cfg, x1, x0, t, cond)
    exact = exact_result(fn, f"hidden_wide/{n}")
    ours = {"pred": terms["pred"].detach().cpu(), **{k: p.grad.cpu() for k, p in m.named_parameters() if k not in FROZEN}}
    assert set(ours) == set(exact) and all(torch.isfinite(v).all() for v in ours.values())
    if precision == "fp32":
        bad = {k: max_abs_rel(v, exact[k]) for k, v in ours.items() if not max_abs_rel(v, exact[k]) < TOL_FP32}
        assert not bad, bad
        return
    got = distances(ours, exact)
    bad = {k: e for k, e in got.items() if not e < 3e-2}
    assert not bad, bad
    class_gate(got, class_error(fn, 7, exact, per="tensor", tag=f"hidden_wide/{n}"), f"generic bf16 training, n_embed 512, H=1380, {n} cells")


@pytest.mark.parametrize("precision,tol", [("fp32", TOL_FP32), ("bf16", TOL_BF16)])
def test_wide_model_with_padded_hidden_rows_record_free_inference(precision, tol, monkeypatch):
    """Eval-mode forward through scldm_dit_infer_* against the route composed from scldm_dit_train_forward (SCLDM_WIDE_INFER=0): the same
    bits (tests/test_gpu_wide_infer.py: test_trunk_has_the_bits_of_the_training_forward), and against the oracle."""
    mk = lambda: make(precision=precision, **WIDE)[0]
    m, cfg, sd = make(precision=precision, **WIDE)
    m0 = with_env(monkeypatch, mk, SCLDM_WIDE_INFER="0")
    assert m._wide_infer_on() and not m0._wide_infer_on()
    n = 9
    gen = torch.Generator().manual_seed(77)
    x, t = torch.randn(n, 16, 16, generator=gen), torch.rand(n, generator=gen)
    lab = {k: torch.randint(0, v, (n,), generator=gen) for k, v in WIDE["vocab"].items()}
    labg = {k: v.cuda() for k, v in lab.items()}
    y, y0 = m(x.cuda(), t.cuda(), labg), m0(x.cuda(), t.cuda(), labg)
    assert torch.isfinite(y).all() and torch.equal(y, y0), float((y - y0).abs().max())
    fn = lambda: dit_forward(sd, cfg, x, t, lab)
    exact = exact_result(fn, "hidden_wide_infer")
    check_err(y.cpu(), exact, tol, f"wide eval forward H=1380 [{precision}] vs oracle", FLOOR_TOL[precision])
    if precision == "bf16":
        gate_tensor(y.cpu(), exact, fn, 7, "wide eval forward H=1380 vs oracle", tag="hidden_wide_infer")

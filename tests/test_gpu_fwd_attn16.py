"""The attention phase of the fused forward on 16x16 MFMA tiles (dit_forward.hpp: kM16QK / kM16V; bf16 / fp16, FT = 2, the default)
against the all-32x32 stream and kernels (SCLDM_FWD_MFMA=32, read once when the native handle is created).

The Q / K / V passes, the scores, the softmax and the P V product of the 16x16 form multiply the same 16-bit operands and add the
products of one output element in the same k slots into one fp32 accumulator chain that starts from the same bias
(tests/test_attn16_lanes_cpu.py restates the lane algebra): not a bit may move.  Sizes are the smallest that reach each tile shape
of the phase: 1, 3 and 35 sample-forwards run 32-token tiles (one cell pair per tile; 1, 3 and 35 leave an odd cell whose pair
partner is padding), 515 runs 64-token tiles (two pairs) with three cells in the ragged last tile.  Inputs scaled by 8 peak the
softmax rows (one key takes nearly all the weight; the others' exponentials underflow towards zero)."""
import pytest
import torch

from conftest import golden_json
from test_gpu_dit import build, cu
from test_gpu_fwd_mfma16_passes import _inputs, _model

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 35, 515)


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_forward_matches_the_all_32x32_form(precision, monkeypatch):
    m16 = _model(precision, monkeypatch)
    m32 = _model(precision, monkeypatch, SCLDM_FWD_MFMA="32")
    for n in SIZES:
        x, t, lab = _inputs(n, 311 + n)
        for scale in (1.0, 8.0):
            with torch.no_grad():
                y16, y32 = m16(x * scale, t, lab), m32(x * scale, t, lab)
            diff = float((y16 - y32).abs().max() / y32.abs().max())
            print(f"[attn16] {precision}: max|16x16 - 32x32| / max|32x32| = {diff:.3e} over {n} sample-forwards, inputs x{scale:g} "
                  f"(bit-identical: {torch.equal(y16, y32)})")
            assert torch.isfinite(y16).all()
            assert torch.equal(y16, y32), (n, scale, diff)


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_cfg_sampler_matches_the_all_32x32_form(precision, monkeypatch):
    """sample_ode_cfg, 9 cells x 4 Euler steps: the (2 + P) B sample-forwards of every evaluation, the blend and the update."""
    m16 = _model(precision, monkeypatch)
    m32 = _model(precision, monkeypatch, SCLDM_FWD_MFMA="32")
    gen = torch.Generator(device="cuda").manual_seed(9)
    z0 = torch.randn(9, 16, 16, device="cuda", generator=gen)
    z2 = torch.cat([z0, z0])
    cond = {"clusters": torch.randint(0, 14, (9,), device="cuda", generator=gen).repeat(2)}
    with torch.no_grad():
        a = m16.sample_ode_cfg(z2, cond, {"clusters": 1.5}, 4, "euler")
        b = m32.sample_ode_cfg(z2, cond, {"clusters": 1.5}, 4, "euler")
    assert torch.isfinite(a).all() and torch.equal(a, b)


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_joint_strategy_golden_matches_the_all_32x32_form(precision, monkeypatch):
    """The reference's golden inputs of the joint conditioning strategy (dit_joint): another set of adaLN vectors, same kernels."""
    g, m16, _, _ = build("dit_joint", precision)
    m16._native_handle()
    monkeypatch.setenv("SCLDM_FWD_MFMA", "32")
    _, m32, _, _ = build("dit_joint", precision)
    m32._native_handle()
    monkeypatch.delenv("SCLDM_FWD_MFMA")
    cond = {k: cu(g[f"fwd_label_{k}"]) for k in golden_json(g, "fwd_classes")}
    with torch.no_grad():
        y16, y32 = m16(cu(g["fwd_x"]), cu(g["fwd_t"]), cond), m32(cu(g["fwd_x"]), cu(g["fwd_t"]), cond)
    assert y16.shape == g["fwd_out"].shape and torch.isfinite(y16).all()
    assert torch.equal(y16, y32)

"""The whole-pass 16x16-tile GEMMs of the fused forward (dit_forward.hpp: gemm_pass16 + relayout16; bf16 / fp16, FT = 2, the
default) against the all-32x32 stream and kernels (SCLDM_FWD_MFMA=32, read once when the native handle is created).

A moved pass multiplies the same 16-bit operands and adds the products of one output element in the same k order into one fp32
accumulator chain that starts from the same bias, and hands its tiles back in the 32x32 accumulator layout with lane swaps: not
a bit may move, at any tile shape, in any layer slot of a launch, in the inference and in the recording (training) kernels.
Sizes are the smallest that reach each instantiation and its ragged tails (tests/test_gpu_fwd_mfma16.py holds the bench size)."""
import pytest
import torch

from test_gpu_dit import build
from test_gpu_train import build as build_train, hip_training_step

pytestmark = pytest.mark.gpu

# sample-forwards: 1 = one sample in a padded 32-token tile; 37 = ragged 32-token tiles; 513 = the smallest launch on 64-token
# tiles (launches of at most 512 run the 32-token instantiation), ragged last tile; 577 = whole 64-token tiles plus a ragged one
SIZES = (1, 37, 513, 577)


def _inputs(n, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(n, 16, 16, device="cuda", generator=gen)
    t = torch.rand(n, device="cuda", generator=gen)
    return x, t, {"clusters": torch.randint(0, 14, (n,), device="cuda", generator=gen)}


def _model(precision, monkeypatch, **env):
    """dit_base (eight layers, the bench workload's shape) with run-time knobs, which the lazily created handle reads once"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _, m, _, _ = build("dit_base", precision)
    m._native_handle()
    for k in env:
        monkeypatch.delenv(k)
    return m


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_forward_matches_the_all_32x32_form_at_every_tile_shape(precision, monkeypatch):
    m16 = _model(precision, monkeypatch)
    m32 = _model(precision, monkeypatch, SCLDM_FWD_MFMA="32")
    for n in SIZES:
        x, t, lab = _inputs(n, 91 + n)
        with torch.no_grad():
            y16, y32 = m16(x, t, lab), m32(x, t, lab)
        diff = float((y16 - y32).abs().max() / y32.abs().max())
        print(f"[mfma16 passes] {precision}: max|16x16 - 32x32| / max|32x32| = {diff:.3e} over {n} sample-forwards "
              f"(bit-identical: {torch.equal(y16, y32)})")
        assert torch.isfinite(y16).all()
        assert torch.equal(y16, y32), (n, diff)


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_layer_slot_independence(precision, monkeypatch):
    """The down-projection's relayout sits at the end of a layer slot: one and three layers per launch against the default eight."""
    n = 513
    x, t, lab = _inputs(n, 17)
    with torch.no_grad():
        ref = _model(precision, monkeypatch)(x, t, lab)
        for lpl in ("1", "3"):
            y = _model(precision, monkeypatch, SCLDM_LPL=lpl)(x, t, lab)
            assert torch.equal(y, ref), lpl


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
@pytest.mark.parametrize("n", [8, 520])      # 32-token / 64-token recording tiles (the switch is at 512 cells)
def test_recording_forward_gives_the_same_training_step(n, precision, monkeypatch):
    """One fused training step (recording forward -> fused backward): loss and every gradient, default against SCLDM_FWD_MFMA=32."""
    vocab = {"cell_line": 4, "gene": 2024}
    gen = torch.Generator().manual_seed(23)
    x1, x0 = torch.randn(n, 16, 16, generator=gen), torch.randn(n, 16, 16, generator=gen)
    t = torch.rand(n, generator=gen)
    cond = {k: torch.randint(0, v + 1, (n,), generator=gen) for k, v in vocab.items()}
    monkeypatch.setenv("SCLDM_TRAIN_FUSED", "1")
    res = {}
    for knob in (None, "32"):
        if knob:
            monkeypatch.setenv("SCLDM_FWD_MFMA", knob)
        m, _, _ = build_train(vocab, "joint", 8, 82)
        m.precision = precision
        terms = hip_training_step(m, x1, x0, t, cond)
        res[knob] = (terms["loss"].detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None})
        if knob:
            monkeypatch.delenv("SCLDM_FWD_MFMA")
    (loss16, g16), (loss32, g32) = res[None], res["32"]
    assert torch.isfinite(loss16).all() and len(g16) == len(g32) > 0
    assert torch.equal(loss16, loss32)
    for k in g16:
        assert torch.equal(g16[k], g32[k]), k

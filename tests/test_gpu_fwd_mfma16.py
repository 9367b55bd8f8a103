"""The 16x16-tile SwiGLU up-projection of the fused forward (bf16 / fp16, the default) against the 32x32 form it replaced
(SCLDM_FWD_MFMA=32, read once when the native handle is created): the same network at the bench's full size and at two batch
sizes that take the other tile shapes, results EQUAL BIT FOR BIT, and bit-repeatable.

Both forms multiply the same 16-bit operands and add the products of one output element in the same k order into an fp32
accumulator, so the tile shape does not change a bit (profiles/r7_fwd_mfma16_ab.txt records it at the bench size).  That makes
this test the oracle for any further tile move: a move that keeps the summation order must keep the bits; one that changes the
order has to replace the equality BY A DERIVED BOUND for the shape it changes - 1.5 x the rel-L2 distance between the 7-bit-operand
oracle (10-bit for fp16) accumulated in fp32 and the same oracle accumulated in fp64, on the same inputs - not by a flat one."""
import pytest
import torch

from test_gpu_dit import build

pytestmark = pytest.mark.gpu

# sample-forwards per launch: one bench evaluation (4 096 cells x 3 CFG branches, 3 072 whole 64-token tiles); 2 049 -> 512.25
# 64-token tiles (ragged last tile of the 64-token instantiation); 509 -> 254.5 32-token tiles (launches of at most 512
# sample-forwards run the 32-token instantiation, ragged here)
SIZES = (12288, 2049, 509)


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_mfma16_forward_matches_the_32x32_form_at_bench_size(precision, monkeypatch):
    _, m16, _, _ = build("dit_base", precision)             # eight layers, the bench workload's shape
    monkeypatch.setenv("SCLDM_FWD_MFMA", "32")
    _, m32, _, _ = build("dit_base", precision)
    m32._native_handle()                                     # the handle (and the knob) is created lazily: create it now
    monkeypatch.delenv("SCLDM_FWD_MFMA")
    gen = torch.Generator(device="cuda").manual_seed(57)
    for n in SIZES:
        x = torch.randn(n, 16, 16, device="cuda", generator=gen)
        t = torch.rand(n, device="cuda", generator=gen)
        lab = {"clusters": torch.randint(0, 14, (n,), device="cuda", generator=gen)}
        with torch.no_grad():
            y16 = m16(x, t, lab)
            y32 = m32(x, t, lab)
            again = m16(x, t, lab)
            small = m16(x[:100], t[:100], {"clusters": lab["clusters"][:100]})   # the 32-token-tile instantiation
        diff = float((y16 - y32).abs().max() / y32.abs().max())
        print(f"[mfma16] {precision}: max|16x16 - 32x32| / max|32x32| = {diff:.3e} over {n} sample-forwards "
              f"(bit-identical: {torch.equal(y16, y32)})")
        assert torch.isfinite(y16).all()
        assert torch.equal(y16, y32), (n, diff)
        assert torch.equal(y16, again)
        assert torch.equal(small, y16[:100])

"""The 16x16-tile SwiGLU up-projection of the fused forward (bf16 / fp16, the default) against the 32x32 form it replaced
(SCLDM_FWD_MFMA=32, read once when the native handle is created): the same network at the bench's full size, results equal
within the suite's tolerances, and bit-repeatable."""
import pytest
import torch

from conftest import max_abs_rel
from test_gpu_dit import TOL_BF16, build

pytestmark = pytest.mark.gpu

# fp16: the bound test_fp16_forward_is_in_the_references_tf32_class puts on the fp16 forward against the exact reference
TOL = {"bf16": TOL_BF16, "fp16": 5e-3}


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_mfma16_forward_matches_the_32x32_form_at_bench_size(precision, monkeypatch):
    _, m16, _, _ = build("dit_base", precision)             # eight layers, the bench workload's shape
    monkeypatch.setenv("SCLDM_FWD_MFMA", "32")
    _, m32, _, _ = build("dit_base", precision)
    m32._native_handle()                                     # the handle (and the knob) is created lazily: create it now
    monkeypatch.delenv("SCLDM_FWD_MFMA")
    gen = torch.Generator(device="cuda").manual_seed(57)
    n = 12288                                                # 4 096 cells x 3 CFG branches: one bench evaluation
    x = torch.randn(n, 16, 16, device="cuda", generator=gen)
    t = torch.rand(n, device="cuda", generator=gen)
    lab = {"clusters": torch.randint(0, 14, (n,), device="cuda", generator=gen)}
    with torch.no_grad():
        y16 = m16(x, t, lab)
        y32 = m32(x, t, lab)
        again = m16(x, t, lab)
        small = m16(x[:100], t[:100], {"clusters": lab["clusters"][:100]})   # the 32-token-tile instantiation
    err = max_abs_rel(y16, y32)
    print(f"[mfma16] {precision}: max|16x16 - 32x32| / max|32x32| = {err:.3e} over {n} sample-forwards "
          f"(bit-identical: {torch.equal(y16, y32)})")
    assert torch.isfinite(y16).all()
    assert err < TOL[precision]
    assert torch.equal(y16, again)
    assert torch.equal(small, y16[:100])

"""CPU-side checks of ScviVAE's fp16-operand training path: the third opt-in switch, the new C entries (declared, exported, refusing
bad arguments before any HIP call), the operand-rounding training helper (tests/scvi_train_class_ref.py) against the plain
restatement, and the mutation table of the class gate on the inputs of tests/test_gpu_scvi_train_fp16.py.

The mutation table emulates the kernels' operand policy in torch - a half cast in front of an fp32 product, it is not kernel code:
every operand of the three products of a Linear goes through a saturating .half() cast; the gradient operand either as it is
("plain"), or multiplied by its tensor's power of two first, 2^e with e = 10 - floor(log2(max |d|)), and the product by 2^-e
("scaled": what the kernels do)."""
import ctypes as C
import math
import os
import re
from unittest import mock

import pytest
import torch

import oracle.dit
import scvi_train_class_ref as ref
from conftest import ROOT, max_abs_rel
from oracle.dit import matmul_operand_bits
from precision_class import class_gate, rel_l2
from scvi_ref import build_scvi
from scvi_train_ref import TRAIN_CASES, scvi_train_step

NEW_EXPORTS = ("scldm_scvi_train_forward_ex", "scldm_scvi_train_backward_ex", "scldm_scvi_train_set_found_inf")
SMALL = 2.0 ** -20


def test_fp16_training_is_a_third_opt_in_and_the_refusal_keeps_its_words():
    from scldm_amd.vae import ScviVAE
    assert ScviVAE.train_fp16_enabled is False
    vae = build_scvi(203, 96, 10, 2, True)
    vae.fp16_enabled = vae.train_enabled = True
    vae.precision = "fp16"
    vae.train()
    counts, lib = torch.ones(3, 203), torch.full((3,), 203.0)
    with pytest.raises(NotImplementedError, match=re.escape("ScviVAE trains in exact fp32 only (precision='fp16')")):
        vae(counts, None, lib)
    vae.train_fp16_enabled = True                       # on this module only; past the refusal the path needs the device
    assert ScviVAE.train_fp16_enabled is False
    with pytest.raises(Exception, match="CUDA") as info:
        vae(counts, None, lib)
    assert not isinstance(info.value, NotImplementedError)
    vae.train_fp16_enabled = False
    with pytest.raises(NotImplementedError, match="fp32 only"):
        vae(counts, None, lib)
    import copy
    vae.__dict__["_found_inf"], vae.__dict__["_found_inf_handle"] = torch.zeros(()), 1      # (what found_inf_flag() caches)
    twin = copy.deepcopy(vae)
    assert "_found_inf" not in twin.__dict__ and "_found_inf_handle" not in twin.__dict__ and twin._handle is None


def test_abi_declares_the_new_entries_and_refuses_bad_arguments_without_a_gpu():
    from scldm_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "scldm_hip.h")).read()
    declared = set(re.findall(r"\b(scldm_[a-z_0-9]+)\s*\(", hdr))
    L = _lib.lib()
    for name in NEW_EXPORTS:
        assert name in declared and name in _lib.EXPORTS and hasattr(L, name), name
    assert len(_lib.EXPORTS) == len(set(_lib.EXPORTS))
    err = lambda: L.scldm_last_error().decode()      # noqa: E731
    h = C.c_void_p()
    assert L.scldm_scvi_create(1, 1, 203, 96, 10, 1, 1e-5, C.byref(h)) == 0 and h.value      # allocates nothing on the device
    try:
        buf = (C.c_char * 8192)()
        base = (C.addressof(buf) + 255) & ~255        # host memory: never dereferenced, a rejected call launches nothing
        p, ws, rec = base + 2048, base, base + 1024
        layer = (_lib.ScviLayerGrads * 1)(_lib.ScviLayerGrads(p, p, p, p))
        g = _lib.ScviGrads(layer, layer, p, p, p, p, p, p, p, None)

        def fwd(prec, hh=h, B=5, n_lib=5, w=ws):
            return L.scldm_scvi_train_forward_ex(hh, p, p, n_lib, B, p, 0.0, 0.0, 3, None, 0, 0.1, rec, p, p, p, p, p, prec, w, None)

        def bwd(prec, hh=h, B=5, n_lib=5, w=ws, grads=g):
            return L.scldm_scvi_train_backward_ex(hh, p, p, n_lib, B, p, 0.0, 0.0, None, rec, p, p, p, p, p, None, None, None, p,
                                                  C.byref(grads) if grads is not None else None, prec, w, None)
        for prec in (_lib.PREC_FP32, _lib.PREC_FP16):
            for call in (fwd, bwd):
                assert call(prec, hh=None) == -1 and "handle" in err()
                assert call(prec, B=1, n_lib=1) == -1 and "B >= 2" in err()
                assert call(prec, n_lib=4) == -1 and "library_size has 4 entries for 5 cells" in err()
                assert call(prec, w=ws + 64) == -1 and "256-byte" in err()
                assert call(prec) == -3 and "scldm_scvi_pack" in err()      # well-formed before pack: a state error, not a launch
            assert "scldm_scvi_train_backward_ex" in err()
            assert bwd(prec, grads=None) == -1 and "grads is NULL" in err()
        for prec in (_lib.PREC_BF16, _lib.PREC_BF16X3, 4, -1):              # not built: a shape error whatever the state
            assert fwd(prec) == -1 and "precision" in err() and "scldm_scvi_train_forward_ex" in err()
            assert bwd(prec) == -1 and "precision" in err() and "scldm_scvi_train_backward_ex" in err()
        assert L.scldm_scvi_train_set_found_inf(None, None) == -1 and "handle" in err()
        assert L.scldm_scvi_train_set_found_inf(h, p + 2) == -1 and "aligned" in err()
        assert L.scldm_scvi_train_set_found_inf(h, p) == 0 and L.scldm_scvi_train_set_found_inf(h, None) == 0
    finally:
        L.scldm_scvi_destroy(h)


@pytest.mark.parametrize("name", sorted(TRAIN_CASES))
def test_helper_equals_the_restatement_with_rounding_off(name):
    """The helper is the restatement with another matmul call: compared in float64, where `x @ w.T` against F.linear (another
    summation order, which depends on the host's BLAS and thread count) is 1e-13 and a wrong helper is not.  The float32 figures are
    printed beside it: they are that summation noise seen through a five-row BatchNorm's backward (1e-7 to 2.3e-6 rel-L2 on the two
    hosts this ran on), not a property of the helper."""
    sd, counts, lib, eps, masks, p = ref.case(name)
    errs = {}
    for dtype in (torch.float64, torch.float32):
        w_out, w_stats, _, w_grads = scvi_train_step(sd, counts, lib, eps, masks, p, dtype=dtype)
        with matmul_operand_bits(None):
            out, stats, grads = ref.step(sd, counts, lib, eps, masks, p, dtype=dtype)
        want, got = ref.flat(w_out, w_stats, w_grads, sd), ref.flat(out, stats, grads, sd)
        assert set(want) == set(got) and len(got) == 5 + len(w_stats) + len(w_grads) - len(w_stats) // 2
        assert all(v.dtype == dtype for v in got.values())
        errs[dtype] = {k: max(rel_l2(got[k], want[k]), max_abs_rel(got[k], want[k])) for k in want}      # both metrics, per tensor
    e64, e32 = errs[torch.float64], errs[torch.float32]
    worst, worst32 = max(e64, key=e64.get), max(e32, key=e32.get)
    print(f"[parity] {name}: operand-rounding training helper (rounding off) vs scvi_train_ref, float64: worst {worst} {e64[worst]:.3e} "
          f"(gate 1e-6); float32 (summation order of the host's BLAS): worst {worst32} {e32[worst32]:.3e}")
    assert all(e <= 1e-6 for e in e64.values()), {k: e for k, e in e64.items() if not e <= 1e-6}


# ---- the emulation of the operand policy ------------------------------------------------------------------------------------------
def _half(x):
    return x.clamp(-65504.0, 65504.0).half().float()


def _truncate10(x):
    return (x.contiguous().view(torch.int32) & ~((1 << 13) - 1)).view(torch.float32)


def _scaled_half(g):
    m = float(g.abs().max())
    e = 0 if m == 0.0 or not math.isfinite(m) else max(-126, min(126, 10 - math.floor(math.log2(m))))
    return _half(g * 2.0 ** e) * 2.0 ** -e


def _emulated_matmul(cast, cast_grad):
    class Emu(torch.autograd.Function):
        @staticmethod
        def forward(ctx, a, b):
            ctx.save_for_backward(a, b)
            return cast(a) @ cast(b)

        @staticmethod
        def backward(ctx, g):
            a, b = ctx.saved_tensors
            rg = cast_grad(g.contiguous())
            return (rg @ cast(b).transpose(-1, -2)).sum_to_size(a.shape), (cast(a).transpose(-1, -2) @ rg).sum_to_size(b.shape)
    return Emu.apply


POLICIES = {"scaled": (_half, _scaled_half), "plain": (_half, _half), "truncating": (_truncate10, _truncate10)}


def _table(name, upstream):
    """(class error, {policy: error}) per tensor of one step of case `name`, every error a rel-L2 to the exact step."""
    sd, counts, lib, eps, masks, p = ref.case(name)
    run = lambda: ref.flat(*ref.step(sd, counts, lib, eps, masks, p, upstream=upstream), sd)      # noqa: E731
    with matmul_operand_bits(None):
        exact = run()
    with matmul_operand_bits(10):
        cls = {k: rel_l2(v, exact[k]) for k, v in run().items()}
    errs = {}
    for policy, (cast, cast_grad) in POLICIES.items():
        with matmul_operand_bits(None), mock.patch.object(oracle.dit, "matmul", _emulated_matmul(cast, cast_grad)):
            errs[policy] = {k: rel_l2(v, exact[k]) for k, v in run().items()}
    return cls, errs


@pytest.mark.parametrize("name", sorted(TRAIN_CASES))
def test_class_gate_passes_the_scaled_half_cast_and_fails_truncation(name):
    """The ELBO step of the GPU class gate: both half-cast policies are inside 1.5 x the 10-bit-operand class error on every tensor
    (the ELBO's gradients sit inside fp16's exponent range), truncation to 10 bits is outside on at least one."""
    cls, errs = _table(name, None)
    fed = [v for k, v in cls.items() if k.startswith("grad:") and v > 0]
    print(f"[parity] {name}: class error of the matmul-fed gradients {min(fed):.2e} ... {max(fed):.2e}")
    for policy in ("scaled", "plain"):
        ratio = class_gate(errs[policy], cls, f"{name}: {policy} half-cast emulation", bits=10)
        assert 0.5 <= ratio <= 1.5
    with pytest.raises(AssertionError):
        class_gate(errs["truncating"], cls, f"{name}: truncating cast (must fail)", bits=10)


@pytest.mark.parametrize("name", ["scvi_train_rows", "scvi_train_tiles"])
def test_small_upstream_gradients_need_the_per_tensor_scale(name):
    """The inputs of the scale-covariance test, upstream gradients of 2^-20 N(0, 1): the per-tensor scale keeps the step inside the
    class, the plain half cast loses the gradient operands to fp16's five exponent bits and lands far outside (tens of times the
    class error on the worst tensor)."""
    up = {k: v * SMALL for k, v in ref.upstream_grads(name).items()}
    cls, errs = _table(name, up)
    class_gate(errs["scaled"], cls, f"{name}: scaled half-cast emulation, upstream x 2^-20", bits=10)
    worst = max(errs["plain"][k] for k in cls if k.startswith("grad:"))
    print(f"[parity] {name}: plain half cast, upstream x 2^-20: worst gradient rel-L2 {worst:.3e} (class worst {max(cls.values()):.3e})")
    with pytest.raises(AssertionError):
        class_gate(errs["plain"], cls, f"{name}: plain half cast, upstream x 2^-20 (must fail)", bits=10)

"""CPU-side checks of ScviVAE's fp16-operand inference path: the opt-in switch, the three scldm_scvi_*_ex entries (declared,
exported, refusing bad arguments before any HIP call), the operand-rounding helper (tests/scvi_class_ref.py) against the plain
restatement, and the mutation demonstration of the class gate on the inputs of tests/test_gpu_scvi_fp16.py."""
import ctypes as C
import os
import re
from unittest import mock

import pytest
import torch

import oracle.dit
import scvi_class_ref as ref
from conftest import ROOT, max_abs_rel
from oracle.dit import matmul_operand_bits
from precision_class import class_gate, rel_l2
from scvi_ref import OUTPUTS, build_scvi, scvi_forward

NEW_EXPORTS = ("scldm_scvi_encode_ex", "scldm_scvi_decode_ex", "scldm_scvi_forward_ex")


def test_fp16_is_opt_in_and_the_refusals_keep_their_words():
    from scldm_amd.vae import ScviVAE
    assert ScviVAE.fp16_enabled is False
    vae = build_scvi(203, 96, 10, 2, True)
    for value in ("fp16", "bf16", "bf16x3"):                      # switch off: exactly as before
        with pytest.raises(NotImplementedError, match="fp32 only"):
            vae.precision = value
    assert vae.precision == "fp32"
    vae.fp16_enabled = True                                       # on this module only
    assert ScviVAE.fp16_enabled is False
    vae.precision = "fp16"
    assert vae.precision == "fp16"
    vae.precision = "fp32"
    assert vae.precision == "fp32"
    for value in ("bf16", "bf16x3", "fp64"):
        with pytest.raises(NotImplementedError, match="bf16 operands are not built"):
            vae.precision = value
        assert vae.precision == "fp32"
    # training stays fp32 whatever the switch says
    vae.precision = "fp16"
    vae.train_enabled = True
    vae.train()
    counts, lib = torch.ones(3, 203), torch.full((3,), 203.0)
    with pytest.raises(NotImplementedError, match="fp32 only"):
        vae(counts, None, lib)
    vae.eval()                                                    # the fp16 eval path needs the device like the fp32 one
    with pytest.raises(RuntimeError, match="CUDA"):
        vae(counts, None, lib)
    vae.fp16_enabled = False                                      # switching off again refuses the next assignment
    with pytest.raises(NotImplementedError, match="fp32 only"):
        vae.precision = "fp16"


def test_abi_declares_the_ex_entries_and_refuses_bad_arguments_without_a_gpu():
    from scldm_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "scldm_hip.h")).read()
    declared = set(re.findall(r"\b(scldm_[a-z_0-9]+)\s*\(", hdr))
    L = _lib.lib()
    for name in NEW_EXPORTS:
        assert name in declared and name in _lib.EXPORTS and hasattr(L, name), name
    assert len(_lib.EXPORTS) == len(set(_lib.EXPORTS))
    err = lambda: L.scldm_last_error().decode()      # noqa: E731
    h = C.c_void_p()
    assert L.scldm_scvi_create(2, 1, 203, 96, 10, 0, 1e-5, C.byref(h)) == 0 and h.value      # allocates nothing on the device
    try:
        buf = (C.c_char * 4096)()
        base = (C.addressof(buf) + 255) & ~255        # host memory: never dereferenced, a rejected call launches nothing
        p, ws = base + 1024, base
        for prec in (_lib.PREC_FP32, _lib.PREC_FP16):
            # the checks of the plain entries, under the new names
            assert L.scldm_scvi_encode_ex(None, p, 5, None, p, p, p, None, prec, ws, None) == -1 and "handle" in err()
            assert L.scldm_scvi_encode_ex(h, p, 0, None, p, p, p, None, prec, ws, None) == -1 and "B >= 1" in err()
            assert L.scldm_scvi_encode_ex(h, None, 5, None, p, p, p, None, prec, ws, None) == -1 and "counts is NULL" in err()
            assert L.scldm_scvi_encode_ex(h, p, 5, p, p, p, p, None, prec, ws, None) == -1 and "z is NULL" in err()
            assert L.scldm_scvi_encode_ex(h, p, 5, None, p, p, p, None, prec, ws + 64, None) == -1 and "256-byte" in err()
            assert "scldm_scvi_encode_ex" in err()
            assert L.scldm_scvi_decode_ex(h, p, p, 4, 5, p, p, prec, ws, None) == -1 and "library_size has 4 entries for 5 cells" in err()
            assert L.scldm_scvi_decode_ex(h, p, p, 5, 5, p + 1, p, prec, ws, None) == -1 and "aligned" in err()
            assert L.scldm_scvi_forward_ex(h, p, p, 5, 5, None, p, p, p, p, p, p, prec, ws, None) == -1 and "eps is NULL" in err()
            assert L.scldm_scvi_forward_ex(h, p, p, 6, 5, p, p, p, p, p, p, p, prec, ws, None) == -1 and "library_size" in err()
            # a well-formed call before pack is a state error, not a launch
            assert L.scldm_scvi_encode_ex(h, p, 5, None, p, p, p, None, prec, ws, None) == -3 and "scldm_scvi_pack" in err()
            assert L.scldm_scvi_decode_ex(h, p, p, 5, 5, p, p, prec, ws, None) == -3 and "scldm_scvi_pack" in err()
            assert L.scldm_scvi_forward_ex(h, p, p, 5, 5, p, p, p, p, p, p, p, prec, ws, None) == -3 and "scldm_scvi_pack" in err()
        # a precision that is not built is a shape error whatever the state
        for prec in (_lib.PREC_BF16, _lib.PREC_BF16X3, 4, -1):
            assert L.scldm_scvi_encode_ex(h, p, 5, None, p, p, p, None, prec, ws, None) == -1 and "precision" in err()
            assert L.scldm_scvi_decode_ex(h, p, p, 5, 5, p, p, prec, ws, None) == -1 and "precision" in err()
            assert L.scldm_scvi_forward_ex(h, p, p, 5, 5, p, p, p, p, p, p, p, prec, ws, None) == -1 and "precision" in err()
    finally:
        L.scldm_scvi_destroy(h)


@pytest.mark.parametrize("name", ref.ALL_CASES)
def test_helper_equals_the_restatement_with_rounding_off(name):
    sd, counts, lib, eps = ref.case_inputs(name)
    want = scvi_forward(sd, counts, lib, eps)
    with matmul_operand_bits(None):
        got = ref.forward(sd, counts, lib, eps)
        h, loc, scale, z = ref.encode(sd, counts, eps)
        mu, theta = ref.decode(sd, z, lib)
    halves = {"h": h, "loc": loc, "scale": scale, "z": z, "mu": mu, "theta": theta}
    for k in OUTPUTS:
        assert torch.equal(halves[k], got[k]), k              # the halves are the forward's
        e = max_abs_rel(got[k], want[k])
        print(f"[parity] {name}: operand-rounding helper (rounding off) vs scvi_ref  {k} {e:.3e}")
        if name in ("scvi_small", "scvi_small_unshared"):
            assert torch.equal(got[k], want[k]), k
        else:
            assert e <= 1e-6, (k, e)                          # x @ w.T against F.linear: another summation order at most


def _truncate(bits):
    drop = 23 - bits

    def f(x):
        return (x.contiguous().view(torch.int32) & ~((1 << drop) - 1)).view(torch.float32)
    return f


@pytest.mark.parametrize("name", ref.ALL_CASES)
def test_class_gate_passes_the_half_cast_and_fails_truncation_and_seven_bits(name):
    """On the inputs of the GPU tests: a chain whose operands go through a plain .half() cast (what the kernel does) is inside
    1.5 x the 10-bit-operand class error on every tensor; truncating to 10 bits, or rounding to 7, is outside on at least one."""
    sd, counts, lib, eps = ref.case_inputs(name)
    run = lambda: ref.forward(sd, counts, lib, eps)      # noqa: E731
    with matmul_operand_bits(None):
        exact = run()
    with matmul_operand_bits(10):
        cls = {k: rel_l2(v, exact[k]) for k, v in run().items()}
    shared = "decoder_head.theta" in sd
    assert (cls["theta"] == 0.0) == shared and all(cls[k] > 0 for k in OUTPUTS if k != "theta")

    def errs(round_fn=None, bits=10):
        with matmul_operand_bits(bits):
            if round_fn is None:
                out = run()
            else:
                with mock.patch.object(oracle.dit, "round_operand", round_fn):
                    out = run()
        return {k: rel_l2(v, exact[k]) for k, v in out.items()}

    ratio = class_gate(errs(lambda x: x.half().float()), cls, f"{name}: half-cast chain", bits=10)
    assert 0.5 <= ratio <= 1.5
    for what, e in (("truncation to 10 bits", errs(_truncate(10))), ("7-bit operands", errs(bits=7))):
        with pytest.raises(AssertionError):
            class_gate(e, cls, f"{name}: {what} (must fail)", bits=10)

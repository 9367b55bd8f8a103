"""CPU checks of the precision argument of the VAE training entry points (scldm_vae_train_forward_ex / _backward_ex): argument
validation happens before any device work, so these run without a GPU."""
import os
import subprocess
import sys

from conftest import ROOT


def _call_forward(L, precision):
    return L.scldm_vae_train_forward_ex(None, None, None, 1, 1, None, None, 1, None, None, None, None, None, precision, None)


def _call_backward(L, precision):
    return L.scldm_vae_train_backward_ex(None, None, None, None, None, 1, 1, None, None, 1, None, None, None, None, None, None, None, None,
                                         precision, None)


def test_training_precision_is_validated():
    from scldm_amd import _lib
    L = _lib.lib()
    for call in (_call_forward, _call_backward):
        for prec in (_lib.PREC_BF16, _lib.PREC_BF16X3, 7, -1):
            assert call(L, prec) == -1 and b"unsupported VAE training precision" in L.scldm_last_error()
        # fp32 / fp16 pass the precision check and stop at the null handle
        for prec in (_lib.PREC_FP32, _lib.PREC_FP16):
            assert call(L, prec) == -1 and b"precision" not in L.scldm_last_error()
    assert L.scldm_vae_train_set_found_inf(None, None) == -1


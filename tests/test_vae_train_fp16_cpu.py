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


def test_fp16_training_refuses_the_earlier_kernel_generations():
    code = ("from scldm_amd import _lib\n"
            "from test_vae_train_fp16_cpu import _call_forward, _call_backward\n"
            "L = _lib.lib()\n"
            "for call in (_call_forward, _call_backward):\n"
            "    assert call(L, _lib.PREC_FP16) == -3, L.scldm_last_error()\n"
            "    assert b'default kernel generations' in L.scldm_last_error()\n"
            "    assert call(L, _lib.PREC_FP32) == -1\n")
    for env in ({"SCLDM_VAE_GENE_MFMA": "1"}, {"SCLDM_VAE_GENE_MFMA": "0"}, {"SCLDM_VAE_GENE_WIDE": "0"}, {"SCLDM_VAE_CELL_WIDE": "0"}):
        e = dict(os.environ, **env)
        e["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests")])
        r = subprocess.run([sys.executable, "-c", code], env=e, cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (env, r.stderr[-2000:])

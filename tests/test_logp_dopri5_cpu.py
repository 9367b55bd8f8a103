"""CPU-side checks of the adaptive log-likelihood solve (scldm_logp_ode_dopri5 / DiT.log_likelihood_cfg(..., "dopri5")): the ABI
surface, the argument checks that run before any HIP call, the Python signature, and the float64 restatement the GPU tests measure against
(tests/logp_dopri5_ref.py) beside the generic `Sampler.sample_ode_likelihood("dopri5")` on a toy field."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

import logp_dopri5_ref
import logp_ref
from conftest import ROOT

ENTRIES = ["scldm_logp_ode_dopri5_workspace_bytes", "scldm_logp_ode_dopri5"]


def test_header_declares_and_library_exports_the_entries():
    from scldm_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "scldm_hip.h")).read()
    declared = set(re.findall(r"\b(scldm_[a-z_0-9]+)\s*\(", hdr))
    L = _lib.lib()
    for name in ENTRIES:
        assert name in declared, f"include/scldm_hip.h does not declare {name}"
        assert hasattr(L, name), f"libscldm_hip.so does not export {name}"
        assert name in _lib.EXPORTS
    assert len(_lib.EXPORTS) == len(set(_lib.EXPORTS))
    assert L.scldm_version() == 5 and C.sizeof(_lib.Dopri5Stats) == 40
    assert L.scldm_logp_ode_dopri5_workspace_bytes(None, 4, 1, 0) == 0


def test_bad_arguments_are_refused_before_any_hip_call():
    """A null handle, a null z and atol = 0 each return SCLDM_ERR_SHAPE with a message and touch nothing: host buffers stand in for z,
    logp, the record and the workspace and stay as they are (no device exists here: any launch or copy would fail another way).  The
    handle is one outside the fused family, which holds no device memory - it is refused too, after the argument checks."""
    from scldm_amd import _lib
    L = _lib.lib()
    cfg = _lib.DitConfig(n_embed=512, n_embed_input=16, n_layer=2, n_head=8, seq_len=16, hidden_dim=1368, layernorm_eps=1e-8, n_classes=1,
                         has_null_row=1)
    cfg.class_vocab[0] = 4
    h = C.c_void_p()
    assert L.scldm_dit_create(C.byref(cfg), C.byref(h)) == 0
    try:
        zbuf = (C.c_float * 520)(*([1.5] * 520))
        z = (C.addressof(zbuf) + 15) & ~15
        lbuf = (C.c_float * 4)(*([2.5] * 4))
        buf, sbuf = (C.c_char * 4096)(), (C.c_char * 64)()
        ws = (C.addressof(buf) + 255) & ~255
        w = _lib.DitWeights()
        stats = _lib.Dopri5Stats(evaluations=7)

        def call(handle=h, zp=z, atol=1e-6, rtol=1e-3, B=1, cells_total=1, probe=None, per_solve=0):
            stats.evaluations = 7
            return L.scldm_logp_ode_dopri5(handle, C.byref(w), zp, None, 0, None, B, 0, None, None, atol, rtol, 0.0, probe, per_solve, 1, 0,
                                           cells_total, C.addressof(lbuf), None, C.byref(stats), None, 0, 0, C.addressof(sbuf), ws, None)

        for what, kw, word in (("null handle", dict(handle=None), "null"), ("null z", dict(zp=None), "null"), ("atol = 0", dict(atol=0.0), "atol"),
                               ("rtol < 0", dict(rtol=-1.0), "rtol"), ("no cells", dict(B=0), "B must"),
                               ("cells_total too small", dict(cells_total=0), "cells_total"),
                               ("probe without probe_per_solve", dict(probe=z), "probe_per_solve"), ("misaligned z", dict(zp=z + 4), "aligned"),
                               ("wide handle", {}, "fused family")):
            rc = call(**kw)
            assert rc == -1, (what, rc)                               # SCLDM_ERR_SHAPE
            assert word in L.scldm_last_error().decode(), (what, L.scldm_last_error())
            assert stats.evaluations == 0, what
        assert all(v == 1.5 for v in zbuf) and all(v == 2.5 for v in lbuf) and buf.raw == bytes(4096)
        assert L.scldm_logp_ode_dopri5_workspace_bytes(h, 4, 1, 0) == 0       # (no fused route for this shape)
    finally:
        L.scldm_dit_destroy(h)


def test_python_surface():
    from scldm_amd.nnets import DiT
    from scldm_amd.transport import Sampler
    sig = inspect.signature(DiT.log_likelihood_cfg).parameters
    assert sig["num_steps"].default == 50 and sig["sampling_method"].default == "euler"
    want = {"atol": 1e-6, "rtol": 1e-3, "first_step": None, "probe_per": "evaluation", "seed": None, "probe": None, "cell_offset": 0,
            "cells_total": None, "return_trace": False}
    for name, default in want.items():
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default == default, name
    assert list(sig)[-len(want):] == list(want)
    doc = " ".join(DiT.log_likelihood_cfg.__doc__.split())
    assert "shard of a dopri5 solve does NOT reproduce" in doc and "step size is shared" in doc
    gen = inspect.signature(Sampler.sample_ode_likelihood).parameters
    assert gen["sampling_method"].default == "dopri5" and gen["atol"].default == 1e-6 and gen["rtol"].default == 1e-3 and gen["first_step"].default is None
    m = DiT(n_embed=256, n_embed_input=16, n_layer=1, n_head=8, seq_len=16, dropout=0.0, bias=True, norm_layer="layernorm", multiple_of=4,
            layernorm_eps=1e-8, class_vocab_sizes={"a": 3}, cfg_dropout_prob=0.8).eval()
    with pytest.raises(RuntimeError, match="CUDA"):
        m.log_likelihood_cfg(torch.zeros(2, 16, 16), {"a": torch.zeros(2, dtype=torch.long)}, {"a": 2.0}, 2, "dopri5")


@pytest.mark.parametrize("atol,rtol", [(1e-5, 1e-5), (1e-6, 1e-3)])
def test_restatement_and_generic_sampler_take_the_same_steps_on_a_toy_field(atol, rtol):
    """logp_ref.toy_model on a 6 x 64 float64 state, one fixed probe: the helper (the float64 oracle's Dormand-Prince solve on the packed
    state) and `Sampler.sample_ode_likelihood("dopri5")` take the same accepted and rejected steps with the same evaluation count, and
    logp agrees to 1e-12 relative.  Both are float64, but the oracle forms a stage point as y0 + (dt beta) @ k and the sampler as
    ((y0 + c0 k0) + c1 k1) + ...: the last bits of the states differ, and the error estimate (a combination whose weights cancel, about
    tol x |k| in size) hands them to the step size amplified by ~1 / tol, / 5 through the fifth root: ~1e-16 / 1e-6 / 5 = 2e-11 at
    most.  So the (s0, h) entries are held to 1e-9 relative (tests/test_oracle_transport.py holds the same pair of solvers to 1e-6) and
    the list lengths and evaluation counts exactly.  Measured: steps within 7.0e-14 / 3.0e-14 relative, logp 4.1e-15 / 6.6e-15,
    26 / 38 evaluations at 1e-5, 1e-5 / 1e-6, 1e-3."""
    from scldm_amd.transport import Sampler, create_transport
    gen = torch.Generator().manual_seed(logp_ref.TOY_SEED)
    x = torch.randn(6, 64, generator=gen, dtype=torch.float64)
    eps = (torch.randint(2, x.shape, generator=gen) * 2 - 1).double()
    logp_h, x_h, st_h = logp_dopri5_ref.logp_dopri5_ref(x, logp_ref.toy_model, eps, atol, rtol, num_steps=50)
    fn = Sampler(create_transport()).sample_ode_likelihood(sampling_method="dopri5", num_steps=50, atol=atol, rtol=rtol)
    logp_s, x_s = fn(x, logp_ref.toy_model, _probe=lambda xc: eps)
    st_s = fn.last_stats
    pairs = list(zip(st_s["accepted_steps"] + st_s["rejected_steps"], st_h["accepted"] + st_h["rejected"]))
    worst = max(max(abs(ta - tb) / max(1.0, abs(tb)), abs(ha - hb) / hb) for (ta, ha), (tb, hb) in pairs)
    print(f"[logp dopri5 toy] atol {atol:g} rtol {rtol:g}: {len(st_h['accepted'])} accepted, {len(st_h['rejected'])} rejected, {st_h['evaluations']} evaluations; "
          f"steps within {worst:.3e} relative; max |logp difference| / max |logp| = {float((logp_s - logp_h).abs().max() / logp_h.abs().max()):.3e}")
    assert len(st_h["accepted"]) >= 2 and logp_s.dtype == torch.float64
    assert len(st_s["accepted_steps"]) == len(st_h["accepted"]) and len(st_s["rejected_steps"]) == len(st_h["rejected"])
    assert worst <= 1e-9
    assert st_s["evaluations"] == st_h["evaluations"] == len(fn.last_trace["logp_grad"])
    assert float((logp_s - logp_h).abs().max()) <= 1e-12 * float(logp_h.abs().max())
    assert float((x_s - x_h).abs().max()) <= 1e-12 * float(x_h.abs().max())
    # a given first step is the first attempted one and saves the initial-step evaluation
    fn1 = Sampler(create_transport()).sample_ode_likelihood(sampling_method="dopri5", num_steps=2, atol=atol, rtol=rtol, first_step=0.0625)
    fn1(x, logp_ref.toy_model, _probe=lambda xc: eps)
    st1 = fn1.last_stats
    assert sorted(st1["accepted_steps"] + st1["rejected_steps"])[0] == (0.0, 0.0625) and (st1["evaluations"] - 1) % 6 == 0

"""CPU-side checks of the wide TransformerVAE training backward (scldm_vaew_train_*): the chunk plan (host arithmetic, no HIP call),
the exported symbols, the opt-in switch and the refusal of a CPU module."""
import ctypes as C
import os
import re

import pytest
import torch

from vae_wide_cases import CASES, build_module

NEW = ["scldm_vaew_train_plan", "scldm_vaew_train_workspace_bytes", "scldm_vaew_train_rows_bytes", "scldm_vaew_train_backward"]


def _create(**kw):
    from scldm_amd import _lib
    d = dict(n_genes=300, n_embed=64, n_inducing=16, n_embed_latent=16, n_layer=2, n_head=8, n_head_cross=4, hidden_dim=172,
             layernorm_eps=1e-8, positional_encoding=1, nb_temperature=1.0)
    d.update(kw)
    L = _lib.lib()
    h = C.c_void_p()
    assert L.scldm_vaew_create(C.byref(_lib.VaeConfig(**d)), C.byref(h)) == 0, L.scldm_last_error()
    return L, h


def _plan(L, h, B, S, G, cap):
    cells, chunks, nbytes = C.c_int(), C.c_int(), C.c_size_t()
    rc = L.scldm_vaew_train_plan(h, B, S, G, cap, C.byref(cells), C.byref(chunks), C.byref(nbytes))
    return rc, cells.value, chunks.value, nbytes.value


def test_plan_bytes_grow_with_the_cells_and_the_chunk_is_the_largest_under_the_cap():
    L, h = _create(n_embed=256, n_genes=36130, hidden_dim=684, n_layer=8)
    for S, G in ((8000, 36130), (1, 1), (600, 300), (65, 4099)):
        sizes = [_plan(L, h, B, S, G, 1 << 62) for B in (1, 2, 3, 7)]
        assert all(rc == 0 and cells == B and chunks == 1 for (rc, cells, chunks, _), B in zip(sizes, (1, 2, 3, 7)))
        nbytes = [s[3] for s in sizes]
        assert nbytes == sorted(nbytes) and len(set(nbytes)) == 4 and nbytes[0] > 0
        one = nbytes[0]
        for B in (1, 5, 16, 33):
            for cap in (one, one + 1, 2 * one + 4096, 3 * one, 7 * one // 2, 1 << 50):
                rc, cells, chunks, nb = _plan(L, h, B, S, G, cap)
                assert rc == 0 and 1 <= cells <= B and nb <= cap
                assert (chunks - 1) * cells < B <= chunks * cells       # every cell once, no empty chunk
                if cells < B:                                           # one cell more would not fit
                    rc2, _, _, more = _plan(L, h, cells + 1, S, G, 1 << 62)
                    assert rc2 == 0 and more > cap
        rc, *_ = _plan(L, h, 4, S, G, one - 1)                          # one cell above the cap is an error that names the bytes
        assert rc == -1 and b"one cell" in L.scldm_last_error() and str(one).encode() in L.scldm_last_error()
    # the census shape (256 wide, 8 + 8 layers, S = 8 000, G = 36 130) under the default cap of 1024 MiB
    rc, cells, chunks, nb = _plan(L, h, 16, 8000, 36130, 0)
    one = _plan(L, h, 1, 8000, 36130, 1 << 62)[3]
    print(f"[plan] wide VAE training record at the census shape: {one} bytes ({one / 2**20:.0f} MiB) per cell; B = 16 under 1024 MiB: "
          f"{cells} cell(s) per chunk, {chunks} chunks")
    assert rc == 0 and nb <= 1024 << 20 and cells * chunks >= 16 and cells == (1024 << 20) // one
    assert L.scldm_vaew_train_workspace_bytes(h, 16, 8000, 36130) == nb
    assert L.scldm_vaew_train_rows_bytes(h, 16, 8000, 36130) == 4 * (16 * (36130 + 8000) * 256 + 16 * 36130)
    assert _plan(L, h, 0, 10, 10, 0)[0] == -1 and _plan(L, h, 2, 0, 10, 0)[0] == -1 and _plan(L, h, 2, 10, 0, 0)[0] == -1
    L.scldm_vaew_destroy(h)


def test_plan_reads_the_handles_cap(monkeypatch):
    monkeypatch.setenv("SCLDM_VAEW_WS_MB", "2")
    L, h = _create(n_layer=1)
    monkeypatch.delenv("SCLDM_VAEW_WS_MB")
    rc, cells, chunks, nb = _plan(L, h, 5, 150, 200, 0)
    assert rc == 0 and nb <= 2 << 20 and chunks >= 3 and 5 % cells != 0
    assert L.scldm_vaew_train_workspace_bytes(h, 5, 150, 200) == nb
    monkeypatch.setenv("SCLDM_VAEW_WS_MB", "1")
    L2, h2 = _create(n_layer=8)
    assert L2.scldm_vaew_train_workspace_bytes(h2, 5, 600, 300) == 0 and b"one cell" in L2.scldm_last_error()
    for x in (h, h2):
        L.scldm_vaew_destroy(x)


def test_new_symbols_are_exported_and_declared():
    from scldm_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "scldm_hip.h")).read()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert re.search(rf"\b(int|size_t)\s+{name}\s*\(", header), name
    # before weights are loaded the backward refuses with SCLDM_ERR_STATE, ahead of any launch
    L, h = _create()
    assert L.scldm_vaew_train_backward(h, None, None, None, 1, 1, None, None, 1, *([None] * 8), 0, None, None, None) == -3
    L.scldm_vaew_destroy(h)


def test_train_wide_is_opt_in_and_a_cpu_module_refuses():
    from scldm_amd.vae import TransformerVAE
    assert TransformerVAE.train_wide is False
    vae = build_module(CASES["vae_wide_64"])
    B, S, G = 2, 5, 7
    counts, genes = torch.ones(B, S), torch.zeros(B, S, dtype=torch.long)
    lib, full = torch.ones(B, 1), torch.zeros(B, G, dtype=torch.long)
    with pytest.raises(NotImplementedError, match="inference only"):
        vae(torch.ones(B, G), full, lib, counts, genes)
    vae.train_wide = True
    with pytest.raises(RuntimeError, match="no CPU path"):
        vae(torch.ones(B, G), full, lib, counts, genes)
    vae.precision = "fp16"
    with pytest.raises(NotImplementedError, match="fp16"):
        vae(torch.ones(B, G), full, lib, counts, genes)

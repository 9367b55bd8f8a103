"""CPU-side checks of the wide TransformerVAE route (scldm_vaew_*): the oracle reproduces the four reference fixtures, the handle's
shape family and the chunk plan (host arithmetic, no HIP call), and the Python guards."""
import ctypes as C

import pytest
import torch

from conftest import golden_json, load_golden, max_abs_rel
from oracle.vae import decode, encode
from oracle.weights import make_state_dict
from vae_wide_cases import CASES, HIDDEN, build_module, oracle_config


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_reproduces_the_wide_fixtures(name):
    """The gate of test_oracle_vae.py (5e-5 scale-relative; measured <= 5.7e-7)."""
    g, c = load_golden(name), CASES[name]
    shapes = {k: tuple(v) for k, v in golden_json(g, "shapes_json").items()}
    assert shapes["encoder.ca_layer.mlp.w1.weight"] == (HIDDEN[name], c["n_embed"]) and HIDDEN[name] % 32 != 0
    assert ("decoder_head.theta.weight" in shapes) == c["shared_theta"]
    sd, cfg = make_state_dict(shapes, int(g["seed"])), oracle_config(c)
    t = lambda k: torch.from_numpy(g[k])   # noqa: E731
    z = encode(sd, cfg, t("counts_subset"), t("genes_subset"))
    assert z.shape == (c["B"], c["n_inducing"], c["n_embed_latent"]) and max_abs_rel(z, g["z"]) < 5e-5
    mu, theta = decode(sd, cfg, t("z"), t("genes"), t("library_size"))
    assert max_abs_rel(mu, g["mu"]) < 5e-5 and max_abs_rel(theta, g["theta"]) < 1e-6
    mu2, _ = decode(sd, cfg, t("zrand"), t("genes"), t("library_size"))
    assert max_abs_rel(mu2, g["mu_rand"]) < 5e-5


def _cfg(**kw):
    from scldm_amd import _lib
    d = dict(n_genes=300, n_embed=64, n_inducing=16, n_embed_latent=16, n_layer=2, n_head=8, n_head_cross=4, hidden_dim=172,
             layernorm_eps=1e-8, positional_encoding=1, nb_temperature=1.0)
    d.update(kw)
    return _lib.VaeConfig(**d)


def _create(**kw):
    from scldm_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    rc = L.scldm_vaew_create(C.byref(_cfg(**kw)), C.byref(h))
    return L, h, rc


@pytest.mark.parametrize("kw, words", [
    (dict(n_embed=48, n_head=2, n_head_cross=2), "n_embed % 32 == 0"),
    (dict(n_embed=2048), "64 <= n_embed <= 1024"),
    (dict(n_embed=64, n_head=16), "head dim"),                      # 64 / 16 = 4
    (dict(n_embed=64, n_head_cross=16), "head dim"),
    (dict(n_inducing=65), "n_inducing_points <= 64"),
    (dict(n_embed_latent=65), "n_embed_latent <= n_embed"),
    (dict(n_embed=96, n_head=5), "n_embed % n_head == 0"),
    (dict(n_layer=-1), "n_layer >= 0"),
])
def test_create_names_the_violated_condition(kw, words):
    L, h, rc = _create(**kw)
    assert rc == -1 and words in L.scldm_last_error().decode(), L.scldm_last_error()


def test_create_accepts_the_family_without_a_gpu_and_the_narrow_handle_keeps_rejecting():
    from scldm_amd import _lib
    for kw in (dict(), dict(n_embed=128, n_head=4, n_head_cross=2, n_inducing=32, n_embed_latent=24, hidden_dim=344),
               dict(n_embed=96, n_head=3, n_head_cross=6, n_inducing=8, n_embed_latent=8, hidden_dim=260, n_layer=0, positional_encoding=0),
               dict(n_embed=1024, n_head=4, n_head_cross=4, n_inducing=64, n_embed_latent=1024, hidden_dim=2732),
               dict(n_embed=64, n_head=1, n_head_cross=8, n_inducing=1, n_embed_latent=1, hidden_dim=1)):
        L, h, rc = _create(**kw)
        assert rc == 0, L.scldm_last_error()
        # no weights yet: the calls refuse with SCLDM_ERR_STATE before any launch
        assert L.scldm_vaew_encode(h, None, None, 1, 1, None, 0, None, None) == -3
        L.scldm_vaew_destroy(h)
    L = _lib.lib()
    h = C.c_void_p()
    assert L.scldm_vae_create(C.byref(_cfg()), C.byref(h)) == -1 and b"n_embed=32" in L.scldm_last_error()


def _plan(L, h, decode_, B, T, cap):
    cells, chunks, nbytes = C.c_int(), C.c_int(), C.c_size_t()
    rc = L.scldm_vaew_plan(h, decode_, B, T, cap, C.byref(cells), C.byref(chunks), C.byref(nbytes))
    return rc, cells.value, chunks.value, nbytes.value


def test_plan_covers_every_cell_once_under_the_cap():
    L, h, rc = _create(n_embed=256, n_genes=36130, hidden_dim=684, n_layer=8)
    assert rc == 0
    for decode_, T in ((1, 36130), (0, 8000), (1, 1), (0, 1), (1, 4099)):
        rc, _, _, one = _plan(L, h, decode_, 1, T, 1 << 62)
        assert rc == 0 and one > 0
        for B in (1, 5, 16, 33):
            for cap in (one, one + 1, 2 * one + 4096, 3 * one, 7 * one // 2, 1 << 40):
                rc, cells, chunks, nbytes = _plan(L, h, decode_, B, T, cap)
                assert rc == 0 and 1 <= cells <= B and nbytes <= cap
                # chunk i holds cells [i * cells, min(B, (i + 1) * cells)): together every cell exactly once, no empty chunk
                assert (chunks - 1) * cells < B <= chunks * cells
                if cells < B:       # the largest chunk under the cap: one cell more would not fit
                    rc2, _, _, more = _plan(L, h, decode_, cells + 1, T, 1 << 62)
                    assert rc2 == 0 and more > cap
            # a cell that alone exceeds the cap is an error, not a loop
            rc, *_ = _plan(L, h, decode_, 4, T, one - 1)
            assert rc == -1 and b"one cell" in L.scldm_last_error()
    # the notebook's shape under the default cap (1024 MiB): 36 130 genes x (2 x 256 + 684) floats = 173 MB per cell -> 6 cells per chunk
    rc, cells, chunks, nbytes = _plan(L, h, 1, 16, 36130, 0)
    assert rc == 0 and (cells, chunks) == (6, 3) and nbytes <= 1024 << 20
    assert L.scldm_vaew_workspace_bytes(h, 16, 8000, 36130) == nbytes
    assert _plan(L, h, 1, 0, 10, 0)[0] == -1 and _plan(L, h, 0, 2, 0, 0)[0] == -1
    L.scldm_vaew_destroy(h)


def test_workspace_cap_knob_is_read_at_handle_creation(monkeypatch):
    monkeypatch.setenv("SCLDM_VAEW_WS_MB", "8")
    L, h, rc = _create()
    assert rc == 0
    monkeypatch.delenv("SCLDM_VAEW_WS_MB")            # read when the handle was made, not at the call
    rc, cells, chunks, nbytes = _plan(L, h, 1, 64, 4099, 0)
    assert rc == 0 and nbytes <= 8 << 20 and cells < 64 and (chunks - 1) * cells < 64 <= chunks * cells
    L.scldm_vaew_destroy(h)
    L, h, rc = _create()
    assert _plan(L, h, 1, 64, 4099, 0)[1:3] == (64, 1)  # the default cap holds the whole batch
    L.scldm_vaew_destroy(h)
    monkeypatch.setenv("SCLDM_VAEW_WS_MB", "0")
    assert _create()[2] == -1


def test_python_guards_of_the_wide_route():
    from scldm_amd.stochastic_layers import GaussianTransformerLayer
    c = CASES["vae_wide_64"]
    vae = build_module(c)
    assert vae.wide and not build_module(dict(c, n_embed=32)).wide
    B, S, G = 2, 5, 7
    counts, genes = torch.zeros(B, S), torch.zeros(B, S, dtype=torch.long)
    z, lib = torch.zeros(B, 16, 16), torch.ones(B, 1)
    with pytest.raises(NotImplementedError, match="inference only"):           # training
        vae(counts, genes, lib, counts, genes)
    vae.precision = "bf16"
    with pytest.raises(NotImplementedError, match="bf16"):
        vae.encode(counts, genes)
    with pytest.raises(NotImplementedError, match="bf16"):
        vae.decode(z, torch.zeros(B, G, dtype=torch.long), lib)
    vae.precision = "fp32"
    with pytest.raises(RuntimeError, match="CUDA"):                            # a valid shape: the handle is made, then no CPU path
        vae.encode(counts, genes)
    vae.decoder_head = GaussianTransformerLayer(n_embed=64, norm_layer="layernorm", layernorm_eps=1e-8)
    for call in (lambda: vae.decode(z, torch.zeros(B, G, dtype=torch.long), lib), lambda: vae.encode(counts, genes),
                 lambda: vae.decode_sample(z, torch.zeros(B, G, dtype=torch.long), lib, seed=1)):
        with pytest.raises(NotImplementedError, match="Gaussian"):
            call()
    # a shape outside the family: NotImplementedError naming the condition, when the native handle is made
    bad = build_module(dict(c, n_embed=48, n_head=2, n_head_cross=2, n_embed_latent=16))
    with pytest.raises(NotImplementedError, match="n_embed % 32 == 0"):
        bad.encode(counts, genes)
    bad = build_module(dict(c, n_inducing=65))
    with pytest.raises(NotImplementedError, match="n_inducing_points <= 64"):
        bad.decode(torch.zeros(B, 65, 16), torch.zeros(B, G, dtype=torch.long), lib)


@pytest.mark.parametrize("name", list(CASES))
def test_wide_state_dict_is_checkpoint_compatible(name):
    g = load_golden(name)
    shapes = {k: tuple(v) for k, v in golden_json(g, "shapes_json").items()}
    vae = build_module(CASES[name])
    assert {k: tuple(v.shape) for k, v in vae.state_dict().items()} == shapes
    vae.load_state_dict(make_state_dict(shapes, int(g["seed"])), strict=True)

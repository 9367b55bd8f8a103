"""The shape-generic TransformerVAE inference route (scldm_vaew_*, csrc/vae_wide.hpp) on the MI355X: reference fixtures at four widths,
ragged sizes around every tile / chunk boundary of its kernels, the census-like shapes, chunking, fp16 operands, the draw."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import check_err, golden_json, load_golden, max_abs_rel
from oracle.vae import decode, encode
from oracle.weights import make_state_dict
from precision_class import class_gate, rel_l2
from vae_wide_cases import CASES, HIDDEN, build_module, oracle_config

pytestmark = pytest.mark.gpu
TOL = 1e-4
_BUILT: dict = {}


def cu(a):
    return torch.from_numpy(np.asarray(a)).cuda()


def build(name):
    """(fixture, module on the GPU, state dict, oracle config) of a golden case; built once per session and left unchanged."""
    if name not in _BUILT:
        g, c = load_golden(name), CASES[name]
        shapes = {k: tuple(v) for k, v in golden_json(g, "shapes_json").items()}
        sd = make_state_dict(shapes, int(g["seed"]))
        vae = build_module(c)
        vae.load_state_dict(sd, strict=True)            # strict: the reference's keys and shapes, nothing missing or extra
        _BUILT[name] = (g, vae.cuda().eval(), sd, oracle_config(c))
    return _BUILT[name]


def fresh(c, seed, positional_encoding=True):
    """A module of shape `c` with make_state_dict weights, its state dict and the oracle's config."""
    vae = build_module(c, positional_encoding)
    shapes = {k: tuple(v.shape) for k, v in vae.state_dict().items()}
    sd = make_state_dict(shapes, seed)
    vae.load_state_dict(sd, strict=True)
    return vae.cuda().eval(), sd, oracle_config(c, positional_encoding)


def inputs(c, B, S, G, seed):
    rng = np.random.default_rng(seed)
    n_rows = c["n_genes"] + 1
    genes_s = rng.integers(0, n_rows, (B, S)).astype(np.int64)
    counts_s = rng.poisson(1.5, (B, S)).astype(np.float32)
    genes = np.stack([rng.permutation(n_rows)[:G] if G <= n_rows else rng.integers(0, n_rows, G) for _ in range(B)]).astype(np.int64)
    lib = rng.uniform(100, 2000, (B, 1)).astype(np.float32)
    zr = rng.standard_normal((B, c["n_inducing"], c["n_embed_latent"])).astype(np.float32)
    return genes_s, counts_s, genes, lib, zr


@pytest.mark.parametrize("name", list(CASES))
def test_golden_parity_fp32(name):
    g, vae, sd, cfg = build(name)
    assert vae.wide and vae.precision == "fp32"
    z = vae.encode(cu(g["counts"]), cu(g["genes"]), cu(g["counts_subset"]), cu(g["genes_subset"]))
    assert z.shape == g["z"].shape
    check_err(z.cpu(), g["z"], TOL, f"{name} encode z")
    nb = vae.decode(cu(g["z"]), cu(g["genes"]), cu(g["library_size"]))
    assert type(nb).__name__ == "NegativeBinomial" and nb.mu.shape == g["mu"].shape == nb.theta.shape
    check_err(nb.mu.cpu(), g["mu"], TOL, f"{name} decode mu")
    assert max_abs_rel(nb.theta.cpu(), g["theta"]) < 1e-5
    nb2 = vae.decode(cu(g["zrand"]), cu(g["genes"]), cu(g["library_size"]))
    check_err(nb2.mu.cpu(), g["mu_rand"], TOL, f"{name} decode mu (random latents)")
    for d in (nb, nb2):
        assert torch.allclose(d.mu.sum(1).cpu(), torch.from_numpy(g["library_size"][:, 0]), rtol=1e-4)
    with torch.no_grad():
        params, z2 = vae(cu(g["counts"]), cu(g["genes"]), cu(g["library_size"]), cu(g["counts_subset"]), cu(g["genes_subset"]))
    assert set(params) == {"mu", "theta"} and torch.equal(z2, z)
    check_err(params["mu"].cpu(), g["mu"], TOL, f"{name} forward mu")
    assert max_abs_rel(params["theta"].cpu(), g["theta"]) < 1e-5
    with pytest.raises(NotImplementedError, match="inference only"):
        vae(cu(g["counts"]), cu(g["genes"]), cu(g["library_size"]), cu(g["counts_subset"]), cu(g["genes_subset"]))


def test_golden_hidden_widths_are_no_multiple_of_32():
    got = [int(build(n)[1].encoder.ca_layer.mlp.w1.weight.shape[0]) for n in CASES]
    assert got == [172, 344, 684, 260] == list(HIDDEN.values()) and all(h % 32 for h in got)


# The kernels' boundaries: the GEMM tile is 64 rows x 64 columns (rows = B * S, B * G and B * n_inducing) with k stages of 32 / 64;
# attention folds keys in chunks of 64 (head dims <= 64), handles 16 queries at a time and 256 per workgroup; the head forms one
# (max, sum exp) pair per 256 genes and finalizes 1024 genes per workgroup; a key axis above 8 chunks = 512 keys (the pooling's S) is
# split over workgroups and merged in split order.  The issue's four sizes first, then each boundary +-1.
RAGGED = [(1, 1, 1), (3, 31, 33), (2, 257, 1025), (5, 100, 4099),
          (1, 63, 255), (1, 64, 256), (1, 65, 257), (2, 129, 15), (3, 127, 17), (4, 16, 1023), (1, 128, 1024),
          (1, 511, 1), (2, 512, 2), (2, 513, 3), (3, 1025, 4)]


@pytest.mark.parametrize("B,S,G", RAGGED)
@pytest.mark.parametrize("name", ["vae_wide_64", "vae_wide_96"])
def test_ragged_sizes_vs_oracle(name, B, S, G):
    g, vae, sd, cfg = build(name)
    genes_s, counts_s, genes, lib, zr = inputs(CASES[name], B, S, G, B * 1000 + S + G)
    z_ref = encode(sd, cfg, torch.from_numpy(counts_s), torch.from_numpy(genes_s))
    check_err(vae.encode(cu(counts_s), cu(genes_s)).cpu(), z_ref, TOL, f"{name} ({B},{S},{G}) z")
    mu_ref, th_ref = decode(sd, cfg, torch.from_numpy(zr), torch.from_numpy(genes), torch.from_numpy(lib))
    nb = vae.decode(cu(zr), cu(genes), cu(lib))
    check_err(nb.mu.cpu(), mu_ref, TOL, f"{name} ({B},{S},{G}) mu")
    assert max_abs_rel(nb.theta.cpu(), th_ref) < 1e-5


def test_head_dims_above_64_and_more_inducing_points_than_a_key_chunk():
    """Head dims 256 (trunk) and 128 (cross) shorten the key chunk to 16 and 32 keys: with 40 inducing points the trunk's
    self-attention and the unpooling walk three / two chunks, the last one ragged.  No positional encoding, theta unshared."""
    c = dict(n_embed=256, n_head=1, n_head_cross=2, n_inducing=40, n_embed_latent=12, n_layer=1, n_genes=120, multiple_of=4, shared_theta=False)
    vae, sd, cfg = fresh(c, 31, positional_encoding=False)
    assert "encoder.pos_embed" not in sd
    genes_s, counts_s, genes, lib, zr = inputs(c, 2, 70, 50, 5)
    check_err(vae.encode(cu(counts_s), cu(genes_s)).cpu(), encode(sd, cfg, torch.from_numpy(counts_s), torch.from_numpy(genes_s)), TOL, "z")
    mu_ref, th_ref = decode(sd, cfg, torch.from_numpy(zr), torch.from_numpy(genes), torch.from_numpy(lib))
    nb = vae.decode(cu(zr), cu(genes), cu(lib))
    check_err(nb.mu.cpu(), mu_ref, TOL, "mu")
    assert max_abs_rel(nb.theta.cpu(), th_ref) < 1e-5


def test_long_gene_axis_properties():
    """The census gene axis on the 64-wide model with the full 8 + 8 layers: G = 36 130, S = 8 000, B = 3."""
    G, S, B = 36130, 8000, 3
    c = dict(CASES["vae_wide_64"], n_layer=8, n_genes=G)
    vae, sd, cfg = fresh(c, 77)
    rng = np.random.default_rng(3)
    genes = np.tile(np.arange(G, dtype=np.int64), (B, 1))
    counts = rng.poisson(0.7, (B, G)).astype(np.float32)
    sub = np.stack([np.sort(rng.permutation(G)[:S]) for _ in range(B)])
    lib = counts.sum(1, keepdims=True) + 1
    cs, gs = np.take_along_axis(counts, sub, 1), np.take_along_axis(genes, sub, 1)
    z = vae.encode(cu(cs), cu(gs))
    assert torch.equal(z, vae.encode(cu(cs), cu(gs)))
    nb = vae.decode(z, cu(genes), cu(lib))
    nb_again = vae.decode(z, cu(genes), cu(lib))
    assert torch.equal(nb.mu, nb_again.mu) and torch.equal(nb.theta, nb_again.theta)
    assert torch.allclose(nb.mu.sum(1), cu(lib[:, 0]), rtol=2e-4)
    perm = rng.permutation(G)
    nb_p = vae.decode(z, cu(genes[:, perm]), cu(lib))
    assert max_abs_rel(nb_p.mu.cpu(), nb.mu.cpu()[:, perm]) < 1e-5        # same values up to the softmax-sum order
    z_ref = encode(sd, cfg, torch.from_numpy(cs[:1]), torch.from_numpy(gs[:1]))
    check_err(z.cpu()[:1], z_ref, TOL, "long axis z, one cell")
    mu_ref, th_ref = decode(sd, cfg, z.cpu()[:1], torch.from_numpy(genes[:1]), torch.from_numpy(lib[:1]))
    check_err(nb.mu.cpu()[:1], mu_ref, TOL, "long axis mu, one cell")
    assert max_abs_rel(nb.theta.cpu()[:1], th_ref) < 1e-5


def test_census_like_layer_shape_vs_oracle():
    """256 wide, 8 + 8 layers (the shape the 20M checkpoint's parameter count points to), G = 2 000, S = 500, B = 2."""
    c = dict(CASES["vae_wide_256"], n_layer=8, n_genes=3000)
    vae, sd, cfg = fresh(c, 91)
    genes_s, counts_s, genes, lib, zr = inputs(c, 2, 500, 2000, 17)
    check_err(vae.encode(cu(counts_s), cu(genes_s)).cpu(), encode(sd, cfg, torch.from_numpy(counts_s), torch.from_numpy(genes_s)), TOL, "z")
    mu_ref, th_ref = decode(sd, cfg, torch.from_numpy(zr), torch.from_numpy(genes), torch.from_numpy(lib))
    nb = vae.decode(cu(zr), cu(genes), cu(lib))
    check_err(nb.mu.cpu(), mu_ref, TOL, "mu")
    assert max_abs_rel(nb.theta.cpu(), th_ref) < 1e-5


def _plan(vae, decode_, B, T):
    from scldm_amd import _lib
    cells, chunks, nbytes = C.c_int(), C.c_int(), C.c_size_t()
    _lib.check(_lib.lib().scldm_vaew_plan(vae.__dict__["_whandle"], decode_, B, T, 0, C.byref(cells), C.byref(chunks), C.byref(nbytes)), "plan")
    return cells.value, chunks.value


def test_chunking_and_batch_independence_are_bit_exact(monkeypatch):
    """A 4 MiB workspace cap (the knob, set before the module's first call) cuts B = 5 into three chunks of two cells: encode and
    decode equal the uncapped module's results and each cell run alone, bit for bit."""
    name, B, S, G = "vae_wide_64", 5, 2500, 1500
    g, vae, sd, cfg = build(name)
    genes_s, counts_s, genes, lib, zr = inputs(CASES[name], B, S, G, 41)
    monkeypatch.setenv("SCLDM_VAEW_WS_MB", "4")
    capped = build_module(CASES[name])
    capped.load_state_dict(sd, strict=True)
    capped = capped.cuda().eval()
    z_c = capped.encode(cu(counts_s), cu(genes_s))
    monkeypatch.delenv("SCLDM_VAEW_WS_MB")
    nb_c = capped.decode(cu(zr), cu(genes), cu(lib))
    assert _plan(capped, 0, B, S)[1] >= 3 and _plan(capped, 1, B, G)[1] >= 3
    z = vae.encode(cu(counts_s), cu(genes_s))
    nb = vae.decode(cu(zr), cu(genes), cu(lib))
    assert _plan(vae, 0, B, S) == (B, 1) and _plan(vae, 1, B, G) == (B, 1)
    assert torch.equal(z_c, z) and torch.equal(nb_c.mu, nb.mu) and torch.equal(nb_c.theta, nb.theta)
    for i in range(B):
        assert torch.equal(vae.encode(cu(counts_s[i:i + 1]), cu(genes_s[i:i + 1])), z[i:i + 1])
        one = vae.decode(cu(zr[i:i + 1]), cu(genes[i:i + 1]), cu(lib[i:i + 1]))
        assert torch.equal(one.mu, nb.mu[i:i + 1]) and torch.equal(one.theta, nb.theta[i:i + 1])


@pytest.mark.parametrize("name", list(CASES))
def test_fp16_policy_within_the_tf32_operand_oracle(name):
    """precision_class's gate: rel-L2(kernel, exact) <= 1.5 x rel-L2(TF32-operand oracle, exact), exact = the reference fixture."""
    from oracle.dit import matmul_operand_bits
    g, vae, sd, cfg = build(name)
    t = torch.from_numpy
    with matmul_operand_bits(10):
        z_tf = encode(sd, cfg, t(g["counts_subset"]), t(g["genes_subset"]))
        mu_tf, _ = decode(sd, cfg, t(g["z"]), t(g["genes"]), t(g["library_size"]))
        mu_tf_r, _ = decode(sd, cfg, t(g["zrand"]), t(g["genes"]), t(g["library_size"]))
    vae.precision = "fp16"
    try:
        z = vae.encode(cu(g["counts"]), cu(g["genes"]), cu(g["counts_subset"]), cu(g["genes_subset"]))
        nb = vae.decode(cu(g["z"]), cu(g["genes"]), cu(g["library_size"]))
        nb_r = vae.decode(cu(g["zrand"]), cu(g["genes"]), cu(g["library_size"]))
    finally:
        vae.precision = "fp32"
    class_gate(rel_l2(z, g["z"]), rel_l2(z_tf, g["z"]), f"{name} encode z", bits=10)
    class_gate(rel_l2(nb.mu, g["mu"]), rel_l2(mu_tf, g["mu"]), f"{name} decode mu", bits=10)
    class_gate(rel_l2(nb_r.mu, g["mu_rand"]), rel_l2(mu_tf_r, g["mu_rand"]), f"{name} decode mu (random latents)", bits=10)
    if CASES[name]["shared_theta"]:
        assert max_abs_rel(nb.theta.cpu(), g["theta"]) < 1e-5      # theta = exp(table[gene]): no contraction, exact in every policy
    assert torch.allclose(nb.mu.sum(1).cpu(), t(g["library_size"][:, 0]), rtol=1e-4)
    assert rel_l2(z, g["z"]) > 0 and not torch.equal(nb.mu.cpu(), t(g["mu"]))      # (the fp16 kernels ran, not the fp32 ones)


def test_decode_sample_is_decode_then_the_seeded_draw():
    g, vae, sd, cfg = build("vae_wide_128")
    args = (cu(g["z"]), cu(g["genes"]), cu(g["library_size"]))
    c1 = vae.decode_sample(*args, seed=5)
    assert c1.shape == g["mu"].shape and (c1 >= 0).all() and torch.equal(c1, torch.round(c1))
    assert torch.equal(c1, vae.decode(*args).sample(seed=5)) and torch.equal(c1, vae.decode_sample(*args, seed=5))
    assert not torch.equal(c1, vae.decode_sample(*args, seed=6))


def test_in_place_weight_update_is_seen_by_the_next_call():
    c = CASES["vae_wide_96"]
    vae, sd, cfg = fresh(c, 12)
    genes_s, counts_s, genes, lib, zr = inputs(c, 2, 20, 30, 8)
    z0 = vae.encode(cu(counts_s), cu(genes_s))
    mu0 = vae.decode(cu(zr), cu(genes), cu(lib)).mu
    with torch.no_grad():           # through .data: invisible to the version counters
        vae.decoder.decoder_cross_attention.attn.c_attn_q.weight.data.mul_(1.5)
        vae.encoder.ca_layer.inducing_points.data.add_(0.25)
        vae.input_layer.gene_embedding.weight.data.mul_(0.5)
    sd = {k: v.detach().cpu().clone() for k, v in vae.state_dict().items()}
    z1 = vae.encode(cu(counts_s), cu(genes_s))
    mu1 = vae.decode(cu(zr), cu(genes), cu(lib)).mu
    assert not torch.equal(z0, z1) and not torch.equal(mu0, mu1)
    check_err(z1.cpu(), encode(sd, cfg, torch.from_numpy(counts_s), torch.from_numpy(genes_s)), TOL, "z after the update")
    check_err(mu1.cpu(), decode(sd, cfg, torch.from_numpy(zr), torch.from_numpy(genes), torch.from_numpy(lib))[0], TOL, "mu after the update")


def test_sample_cells_with_a_wide_vae_matches_oracle_chain():
    """test_gpu_vae.test_sample_cells_harness_matches_oracle_chain with the 64-wide VAE (16 x 16 latents, the fused DiT's input)."""
    from oracle.dit import DiTConfig, dit_forward_with_cfg
    from oracle.transport import sample_ode_fixed
    from scldm_amd.nnets import DiT
    from scldm_amd.sampling import sample_cells
    g, vae, sd_v, cfg_v = build("vae_wide_64")
    gd = load_golden("dit_base")
    kw = golden_json(gd, "kwargs_json")
    shapes = {k: tuple(v) for k, v in golden_json(gd, "shapes_json").items()}
    sd_d = make_state_dict(shapes, int(gd["seed"]))
    dit = DiT(**kw)
    dit.load_state_dict(sd_d, strict=True)
    dit = dit.cuda().eval()
    cfg_d = DiTConfig(class_vocab_sizes=kw["class_vocab_sizes"], condition_strategy=kw["condition_strategy"])
    rng = np.random.default_rng(9)
    B, G = 3, 250
    z0 = rng.standard_normal((B, 16, 16)).astype(np.float32)
    lab = rng.integers(0, 14, B).astype(np.int64)
    genes = np.stack([rng.permutation(300)[:G] for _ in range(B)]).astype(np.int64)
    logsf = rng.normal(7.0, 0.3, B).astype(np.float32)
    scales = {"clusters": 2.0}
    nb, z = sample_cells(dit, vae, {"clusters": cu(lab)}, scales, B, cu(genes), cu(logsf), num_steps=4, sampling_method="euler",
                         z0=cu(z0), draw_counts=False)
    z2 = torch.from_numpy(np.concatenate([z0, z0]))
    cond2 = {"clusters": torch.from_numpy(np.concatenate([lab, lab]))}
    z_ref = sample_ode_fixed(z2, lambda x, t: dit_forward_with_cfg(sd_d, cfg_d, x, t, cond2, scales), 4, "euler")
    lib = torch.exp(torch.from_numpy(np.concatenate([logsf, logsf]))).view(-1, 1)
    mu_ref, th_ref = decode(sd_v, cfg_v, z_ref, torch.from_numpy(np.concatenate([genes, genes])), lib)
    assert z.shape == (2 * B, 16, 16) and max_abs_rel(z.cpu(), z_ref) < TOL
    assert max_abs_rel(nb.mu.cpu(), mu_ref) < 2e-4 and max_abs_rel(nb.theta.cpu(), th_ref) < 1e-5
    counts, _ = sample_cells(dit, vae, {"clusters": cu(lab)}, scales, B, cu(genes), cu(logsf), num_steps=4, sampling_method="euler",
                             z0=cu(z0), seed=3)
    assert counts.shape == (2 * B, G) and torch.equal(counts, nb.sample(seed=3))


def test_the_32_wide_shape_keeps_its_route_and_its_bits():
    from scldm_amd import _lib
    from test_gpu_vae import build as build_narrow
    g, vae, sd, cfg = build_narrow("vae_2000")
    assert not vae.wide
    vae.kernel_timing(True)
    z = vae.encode(cu(g["counts"]), cu(g["genes"]), cu(g["counts_subset"]), cu(g["genes_subset"]))
    nb = vae.decode(cu(g["z"]), cu(g["genes"]), cu(g["library_size"]))
    torch.cuda.synchronize()
    timing = vae.kernel_timing()
    vae.kernel_timing(False)
    assert set(timing) == set(vae.KERNEL_KINDS) and all(n == 1 for n, _ in timing.values()), timing     # the MCAB kernels were launched
    assert vae.__dict__.get("_whandle") is None
    # the module's results are those of the narrow C entry, bit for bit
    L, h = vae._native()
    zz, genes, lib = cu(g["z"]), cu(g["genes"]), cu(g["library_size"]).reshape(-1)
    B, G = genes.shape
    mu, theta = torch.empty(B, G, device="cuda"), torch.empty(B, G, device="cuda")
    ws = torch.empty(L.scldm_vae_workspace_bytes(h, B, G), dtype=torch.uint8, device="cuda")
    _lib.check(L.scldm_vae_decode(h, zz.data_ptr(), genes.data_ptr(), lib.data_ptr(), B, G, mu.data_ptr(), theta.data_ptr(), _lib.PREC_FP32,
                                  ws.data_ptr(), torch.cuda.current_stream().cuda_stream), "scldm_vae_decode")
    assert torch.equal(mu, nb.mu) and torch.equal(theta, nb.theta)
    assert max_abs_rel(nb.mu.cpu(), g["mu"]) < TOL and max_abs_rel(z.cpu(), g["z"]) < TOL

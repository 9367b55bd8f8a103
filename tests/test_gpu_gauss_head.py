"""GPU tests of the Gaussian decoder head (`decoder_name: gaussian`): decode / decode_sample / forward of a TransformerVAE built with
GaussianTransformerLayer against the reference's golden vectors and the CPU restatement (tests/gauss_head_ref.py), the stand-alone
draw, the fused reconstruction loss, the guards between the two head kinds and the sampling harness.

Tolerances: fp32 1e-4 scale-relative max error (BASELINE.json north_star gate); the 16-bit operand policies are held to the error of
the restatement run with 10-bit / 7-bit matmul operands on the same inputs (precision_class.class_gate, factor CLASS_FACTOR = 1.5);
the loss to 1e-4 * max(1, |ref|) against float64 (the gate of test_gpu_eval_metrics.py).  The draw's bounds are 5 sigma of the
estimators' own sampling distributions for N standard normals: mean sigma = 1 / sqrt(N), variance sigma = sqrt(2 / N), tail share
sigma = sqrt(p (1 - p) / N) with p = P(|n| > 1.96) = 0.05."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from conftest import check_err, golden_json, load_golden, max_abs_rel
from gauss_head_ref import decode_gaussian, recon_loss_rows
from oracle.vae import VAEConfig, encode
from oracle.weights import make_state_dict
from precision_class import class_error, class_gate, rel_l2
from test_gauss_head_cpu import build_gauss_vae

pytestmark = pytest.mark.gpu
TOL = 1e-4
RAGGED = [(1, 1), (3, 33), (2, 1025), (5, 4099)]      # partial 32-gene tiles, a second 1 024-gene chunk, an odd cell pair (test_gpu_vae.py)


def cu(a):
    return torch.from_numpy(np.asarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def case(name):
    g = load_golden(name)
    shapes = {k: tuple(v) for k, v in golden_json(g, "shapes_json").items()}
    return g, make_state_dict(shapes, int(g["seed"])), VAEConfig(n_genes=int(g["n_genes"]))


def fresh_vae(name):
    g, sd, cfg = case(name)
    vae = build_gauss_vae(int(g["n_genes"]))
    vae.load_state_dict(sd, strict=True)
    return vae.cuda().eval()


@functools.lru_cache(maxsize=None)
def shared_vae(name):
    """One module per golden for the tests that leave its weights alone (its `precision` is set by every test that reads it)."""
    return fresh_vae(name)


@functools.lru_cache(maxsize=None)
def ragged(B, G):
    """Inputs at a ragged shape on the gauss_2000 weights and the exact restatement's mu for them (computed once, never written to)."""
    g, sd, cfg = case("gauss_2000")
    rng = np.random.default_rng(B * 1000 + G)
    genes = np.stack([rng.permutation(2001)[:G] if G <= 2001 else rng.integers(0, 2001, G) for _ in range(B)]).astype(np.int64)
    zr = rng.standard_normal((B, 16, 16)).astype(np.float32)
    counts = rng.poisson(0.7, (B, G)).astype(np.float32)
    counts[:, 0] += 1.0                                       # no all-zero row (that case has a test of its own)
    mu_ref = decode_gaussian(sd, cfg, torch.from_numpy(zr), torch.from_numpy(genes))
    return genes, zr, counts, mu_ref


@pytest.mark.parametrize("name", ["gauss_small", "gauss_2000"])
def test_fp32_parity_with_the_reference_golden(name):
    g, sd, cfg = case(name)
    vae = shared_vae(name)
    vae.precision = "fp32"
    z = vae.encode(cu(g["counts"]), cu(g["genes"]), cu(g["counts_subset"]), cu(g["genes_subset"]))
    assert z.shape == g["z"].shape
    check_err(z.cpu(), g["z"], TOL, f"{name} encode")
    d = vae.decode(cu(g["z"]), cu(g["genes"]), cu(g["library_size"]))
    assert isinstance(d, torch.distributions.Normal) and torch.equal(d.scale, torch.ones_like(d.mu)) and d.mu is d.loc
    check_err(d.mu.cpu(), g["mu"], TOL, f"{name} decode mu")
    d2 = vae.decode(cu(g["zrand"]), cu(g["genes"]), cu(g["library_size"]))
    check_err(d2.mu.cpu(), g["mu_rand"], TOL, f"{name} decode mu (random latents)")
    with torch.no_grad():
        params, z2 = vae(cu(g["counts"]), cu(g["genes"]), cu(g["library_size"]), cu(g["counts_subset"]), cu(g["genes_subset"]))
    assert set(params) == {"mu"} and torch.equal(z2, z)
    check_err(params["mu"].cpu(), g["mu"], TOL, f"{name} forward mu")
    assert torch.equal(params["mu"], vae.decode(z, cu(g["genes"]), cu(g["library_size"])).mu)


@pytest.mark.parametrize("B,G", RAGGED)
def test_ragged_shapes_in_every_operand_policy(B, G):
    g, sd, cfg = case("gauss_2000")
    vae = shared_vae("gauss_2000")
    genes, zr, counts, mu_ref = ragged(B, G)
    lib = torch.ones(B, 1, device="cuda")
    vae.precision = "fp32"
    mu = vae.decode(cu(zr), cu(genes), lib).mu
    assert mu.shape == (B, G) and torch.isfinite(mu).all()
    check_err(mu.cpu(), mu_ref, TOL, f"gaussian decode B={B} G={G} fp32 vs restatement")
    errs = {}
    for prec, bits in (("fp16", 10), ("bf16", 7)):
        vae.precision = prec
        mu_p = vae.decode(cu(zr), cu(genes), lib).mu
        assert torch.isfinite(mu_p).all()
        cls = class_error(lambda: decode_gaussian(sd, cfg, torch.from_numpy(zr), torch.from_numpy(genes)), bits, mu_ref,
                          tag=f"gauss_2000/decode/{B}x{G}")
        errs[prec] = rel_l2(mu_p, mu_ref)
        print(f"[parity] gaussian decode B={B} G={G} [{prec}]: kernel rel-L2 {errs[prec]:.3e}, max_abs_rel {max_abs_rel(mu_p.cpu(), mu_ref):.3e}; "
              f"{bits}-bit-operand restatement rel-L2 {cls['rel_l2']:.3e}, max_abs_rel {cls['max_abs_rel']:.3e}")
        class_gate(errs[prec], cls["rel_l2"], f"gaussian decode B={B} G={G} vs exact restatement", bits=bits)
    vae.precision = "fp32"
    assert errs["fp16"] < errs["bf16"], errs


@pytest.mark.parametrize("prec", ["fp32", "fp16", "bf16"])
def test_genes_are_independent(prec):
    """No reduction runs across the genes: a decode repeats bit for bit, and permuting the gene list permutes mu exactly."""
    vae = shared_vae("gauss_2000")
    genes, zr, counts, mu_ref = ragged(5, 4099)
    lib = torch.ones(5, 1, device="cuda")
    vae.precision = prec
    mu = vae.decode(cu(zr), cu(genes), lib).mu
    assert torch.equal(vae.decode(cu(zr), cu(genes), lib).mu, mu)
    perm = np.random.default_rng(4).permutation(4099)
    mu_perm = vae.decode(cu(zr), cu(genes[:, perm]), lib).mu
    vae.precision = "fp32"
    assert torch.equal(mu_perm, mu[:, cu(perm)])


def test_fused_draw_is_seeded_and_equals_decode_then_sample():
    g, sd, cfg = case("gauss_2000")
    vae = shared_vae("gauss_2000")
    vae.precision = "fp32"
    genes, zr, counts, mu_ref = ragged(5, 4099)
    lib = torch.ones(5, 1, device="cuda")
    a = vae.decode_sample(cu(zr), cu(genes), lib, seed=42)
    assert a.shape == (5, 4099) and torch.isfinite(a).all()
    assert torch.equal(vae.decode_sample(cu(zr), cu(genes), lib, seed=42), a)
    assert not torch.equal(vae.decode_sample(cu(zr), cu(genes), lib, seed=43), a)
    d = vae.decode(cu(zr), cu(genes), lib)
    assert torch.equal(d.sample(seed=42), a)
    assert not torch.equal(a, d.mu) and float((a - d.mu).std()) > 0.9           # a unit normal was added
    torch.manual_seed(3); s1 = d.sample()
    torch.manual_seed(3); s2 = d.sample()
    assert torch.equal(s1, s2)                                                  # the default seed comes from torch's global generator


def test_normal_draw_statistics():
    from scldm_amd.stochastic_layers import Normal
    N = 5 * 4099
    n = Normal(torch.zeros(5, 4099, device="cuda"), 1.0).sample(seed=1234).double().cpu().numpy().reshape(-1)
    mean, var, tail = n.mean(), n.var(), float((np.abs(n) > 1.96).mean())
    print(f"[draw] N={N}: mean {mean:+.4e} (bound {5 / np.sqrt(N):.4e})  var-1 {var - 1:+.4e} (bound {5 * np.sqrt(2 / N):.4e})  "
          f"P(|n|>1.96) {tail:.5f} (0.05 +- {5 * np.sqrt(0.05 * 0.95 / N):.5f})")
    assert abs(mean) <= 5 / np.sqrt(N)
    assert abs(var - 1) <= 5 * np.sqrt(2 / N)
    assert abs(tail - 0.05) <= 5 * np.sqrt(0.05 * 0.95 / N)
    # the first elements do not depend on how many more are drawn (counter = element index)
    few = Normal(torch.zeros(100, device="cuda"), 1.0).sample(seed=1234).double().cpu().numpy()
    assert np.array_equal(few, n[:100])


def test_inplace_update_of_the_head_layernorm_reaches_the_next_decode():
    g, sd, cfg = case("gauss_2000")
    vae = fresh_vae("gauss_2000")
    z, genes, lib = cu(g["z"]), cu(g["genes"]), cu(g["library_size"])
    mu0 = vae.decode(z, genes, lib).mu
    versions = [p._version for p in vae.parameters()]
    vae.decoder_head.ln.weight.data.mul_(1.5).add_(0.01)          # EMA-style: no version bump, same storage
    vae.decoder_head.ln.bias.data.add_(0.02)
    assert [p._version for p in vae.parameters()] == versions
    mu1 = vae.decode(z, genes, lib).mu
    assert not torch.equal(mu1, mu0)
    sd2 = {k: v.detach().cpu() for k, v in vae.state_dict().items()}
    check_err(mu1.cpu(), decode_gaussian(sd2, cfg, z.cpu(), genes.cpu()), TOL, "gaussian decode after an in-place update of decoder_head.ln")


def test_training_forward_raises_for_the_gaussian_head():
    g, sd, cfg = case("gauss_small")
    vae = fresh_vae("gauss_small")
    vae.train()
    with pytest.raises(NotImplementedError, match="Gaussian"):
        vae(cu(g["counts"]), cu(g["genes"]), cu(g["library_size"]), cu(g["counts_subset"]), cu(g["genes_subset"]))
    # the CSR-assembling prediction loop refuses the head before it touches the diffusion model (dense reals are not counts)
    from types import SimpleNamespace
    from scldm_amd.sampling import generate_cells_stream
    with pytest.raises(NotImplementedError, match="Gaussian"):
        next(generate_cells_stream(SimpleNamespace(pos_embed=torch.zeros(1, device="cuda")), vae, [], {}, cu(g["genes"])))


def test_c_entries_refuse_the_wrong_head_and_the_nb_head_is_untouched():
    from scldm_amd import _lib
    from test_gpu_vae import build as build_nb
    L = _lib.lib()
    g, sd, cfg = case("gauss_small")
    gv = fresh_vae("gauss_small")
    gn, nv, _, _ = build_nb("vae_small")
    B, G = g["genes"].shape
    S = g["genes_subset"].shape[1]
    z, genes, lib = cu(g["z"]), cu(g["genes"]), cu(g["library_size"]).reshape(-1)
    cs, gs = cu(g["counts_subset"]), cu(g["genes_subset"])
    out, out2 = torch.empty(B, G, device="cuda"), torch.empty(B, G, device="cuda")
    zb = torch.empty(B, 16, 16, device="cuda")
    ws = torch.empty(1 << 24, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    mu_g = gv.decode(z, genes, lib).mu                 # (builds and loads both handles)
    mu_n = nv.decode(cu(gn["z"]), cu(gn["genes"]), cu(gn["library_size"])).mu
    hg, hn = gv._handle, nv._handle
    p = lambda t: t.data_ptr()
    # the negative-binomial and training entry points on a Gaussian handle
    assert L.scldm_vae_decode(hg, p(z), p(genes), p(lib), B, G, p(out), p(out2), 0, p(ws), st) == -1
    assert b"Gaussian" in L.scldm_last_error()
    assert L.scldm_vae_decode_sample(hg, p(z), p(genes), p(lib), B, G, p(out), 7, 0, p(ws), st) == -1 and b"Gaussian" in L.scldm_last_error()
    assert L.scldm_vae_train_forward(hg, p(cs), p(gs), B, S, p(genes), p(lib), G, p(out), p(out2), p(zb), p(ws), p(ws), st) == -1
    assert b"Gaussian" in L.scldm_last_error()
    assert L.scldm_vae_train_forward_ex(hg, p(cs), p(gs), B, S, p(genes), p(lib), G, p(out), p(out2), p(zb), p(ws), p(ws), 3, st) == -1
    assert b"Gaussian" in L.scldm_last_error()
    w, keep = gv._weights_struct(lambda t: t.data_ptr())
    back = (hg, C.byref(w), C.byref(w), p(cs), p(gs), B, S, p(genes), p(lib), G, p(out), p(out2), p(zb), p(out), p(out2), p(zb), p(ws), p(ws))
    assert L.scldm_vae_train_backward(*back, st) == -1 and b"Gaussian" in L.scldm_last_error()
    assert L.scldm_vae_train_backward_ex(*back, 0, st) == -1 and b"Gaussian" in L.scldm_last_error()
    assert L.scldm_vae_train_backward_ordered(*back, 0, p(ws), p(ws), 0, p(ws), st) == -1 and b"Gaussian" in L.scldm_last_error()
    assert L.scldm_vae_train_set_found_inf(hg, p(out)) == -1 and b"Gaussian" in L.scldm_last_error()
    # the Gaussian entry points on a negative-binomial handle
    zn, genes_n = cu(gn["z"]), cu(gn["genes"])
    Bn, Gn = gn["genes"].shape
    out_n = torch.empty(Bn, Gn, device="cuda")
    assert L.scldm_vae_decode_gaussian(hn, p(zn), p(genes_n), Bn, Gn, p(out_n), 0, p(ws), st) == -1 and b"negative-binomial" in L.scldm_last_error()
    assert L.scldm_vae_decode_gaussian_sample(hn, p(zn), p(genes_n), Bn, Gn, p(out_n), 7, 0, p(ws), st) == -1
    assert b"negative-binomial" in L.scldm_last_error()
    torch.cuda.synchronize()
    # nothing was launched or broken: both modules still decode, the NB one its golden
    assert torch.equal(gv.decode(z, genes, lib).mu, mu_g)
    nb = nv.decode(cu(gn["z"]), cu(gn["genes"]), cu(gn["library_size"]))
    assert torch.equal(nb.mu, mu_n) and max_abs_rel(nb.mu.cpu(), gn["mu"]) < TOL and max_abs_rel(nb.theta.cpu(), gn["theta"]) < 1e-5
    assert set(nv(cu(gn["counts"]), cu(gn["genes"]), cu(gn["library_size"]), cu(gn["counts_subset"]), cu(gn["genes_subset"]))[0]) == {"mu", "theta"}
    # encode is the same for both head kinds
    check_err(gv.encode(cu(g["counts"]), cu(g["genes"]), cs, gs).cpu(), g["z"], TOL, "gaussian-head encode")


def _loss_close(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    print(f"[parity] gaussian_recon_loss: max |got - ref| / max(1, |ref|) = {err.max():.3e}  (gate 1e-4; |ref| up to {np.abs(ref).max():.4g})")
    assert got.shape == ref.shape and (err <= 1e-4).all(), (got, ref)


@pytest.mark.parametrize("B,G", RAGGED)
def test_recon_loss_vs_float64(B, G):
    from scldm_amd.distributions import gaussian_recon_loss
    genes, zr, counts, mu_ref = ragged(B, G)
    mu = mu_ref.float().contiguous().cuda()
    loss = gaussian_recon_loss(cu(counts), mu)
    assert loss.shape == (B,) and loss.dtype == torch.float32
    _loss_close(loss.cpu().numpy(), recon_loss_rows(counts, mu.cpu().numpy()))
    assert torch.equal(gaussian_recon_loss(cu(counts), mu), loss)


def test_recon_loss_golden_zero_row_and_metrics_composition():
    from scldm_amd.distributions import gaussian_recon_loss, log_gaussian
    from scldm_amd.evaluations import count_metrics, normalize_log1p, reconstruction_metrics
    g, sd, cfg = case("gauss_2000")
    counts, mu = cu(g["counts"]), cu(g["mu"])
    loss = gaussian_recon_loss(counts, mu)
    _loss_close(loss.cpu().numpy(), g["loss_rows"])
    _loss_close(loss.cpu().numpy(), log_gaussian(normalize_log1p(counts), mu).sum(1).cpu().numpy())     # the unfused form
    # an all-zero row: what scldm_log1p_normalize makes of it (0 / 0), in that row only
    cz = counts.clone()
    cz[1] = 0
    lz = gaussian_recon_loss(cz, mu)
    yz = normalize_log1p(cz)
    assert torch.equal(lz[0], loss[0]) and torch.isnan(yz[1]).all() and torch.isnan(lz[1])
    m = reconstruction_metrics(mu, counts, head="gaussian")
    ref = count_metrics(mu, normalize_log1p(counts), target_sum=0.0)
    assert set(m) == {"mse", "pcc", "zeros_accuracy"} and all(torch.equal(m[k], ref[k]) for k in m)
    assert abs(float(m["mse"]) - float(loss.double().sum()) / counts.numel()) <= 1e-4 * max(1.0, float(m["mse"]))
    nb_m = reconstruction_metrics(counts, counts)                           # the default head is unchanged
    assert all(torch.equal(nb_m[k], count_metrics(counts, counts)[k]) for k in nb_m)


def test_sample_cells_harness_with_a_gaussian_vae():
    from scldm_amd.nnets import DiT
    from scldm_amd.sampling import sample_cells
    from scldm_amd.stochastic_layers import Normal
    vae = shared_vae("gauss_2000")
    vae.precision = "fp32"
    gd = load_golden("dit_base")
    kw = golden_json(gd, "kwargs_json")
    dit = DiT(**kw)
    dit.load_state_dict(make_state_dict({k: tuple(v) for k, v in golden_json(gd, "shapes_json").items()}, int(gd["seed"])), strict=True)
    dit = dit.cuda().eval()
    rng = np.random.default_rng(9)
    B, G = 3, 300
    z0 = cu(rng.standard_normal((B, 16, 16)).astype(np.float32))
    lab = {"clusters": cu(rng.integers(0, 14, B).astype(np.int64))}
    genes = cu(np.stack([rng.permutation(2000)[:G] for _ in range(B)]).astype(np.int64))
    logsf = cu(rng.normal(7.0, 0.3, B).astype(np.float32))
    x, z = sample_cells(dit, vae, lab, {"clusters": 2.0}, B, genes, logsf, num_steps=5, sampling_method="euler", z0=z0, draw_counts=True, seed=5)
    assert x.shape == (2 * B, G) and x.dtype == torch.float32 and torch.isfinite(x).all() and z.shape == (2 * B, 16, 16)
    d, z2 = sample_cells(dit, vae, lab, {"clusters": 2.0}, B, genes, logsf, num_steps=5, sampling_method="euler", z0=z0, draw_counts=False)
    assert isinstance(d, Normal) and torch.equal(z2, z)
    genes2 = torch.cat([genes, genes])
    assert torch.equal(d.mu, vae.decode(z2, genes2, torch.ones(2 * B, 1, device="cuda")).mu)
    assert torch.equal(x, d.sample(seed=5))

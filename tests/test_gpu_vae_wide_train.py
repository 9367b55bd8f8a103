"""Training of the wide TransformerVAE shapes on the MI355X (`TransformerVAE.train_wide`, scldm_vaew_train_backward, csrc/vae_wide_train.hpp):
every parameter gradient against
  (a) digests of the REFERENCE's own autograd gradients (tests/golden/vae_wide_train_{64,128}.npz), and
  (b) autograd over the CPU oracle (oracle/vae_train.py) at the four wide fixture shapes and on ragged sizes around the kernels' tile,
      chunk and split boundaries, always with a loss term on the returned latent;
then chunking under a workspace cap, run-to-run bit equality, the forward's bits, an optimiser step and the refusals.
Exact fp32; the project's standing gate for such gradients (tests/test_gpu_vae_train.py): 1e-4 of each tensor's scale (max |entry|, or
l2 / sqrt(numel) for the digests), the loss 1e-4 relative, mu and z 1e-4.  Under shared theta decoder_head.params.bias has a
mathematically zero gradient (softmax over genes is shift-invariant): |grad| <= 1e-3 x the norm of decoder_head.params.weight's
gradient, as in that file.  No tensor but the frozen encoder.pos_embed is left out."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import golden_json, load_golden, max_abs_rel
from oracle.train import grad_digest
from oracle.vae_train import FROZEN, log_nb_positive as log_nb_oracle, vae_training_grads
from oracle.weights import make_state_dict
from vae_wide_cases import CASES, build_module, oracle_config

pytestmark = pytest.mark.gpu
TOL = 1e-4
BIAS = "decoder_head.params.bias"
_ORACLE: dict = {}


def cu(a):
    return torch.from_numpy(np.asarray(a)).cuda()


def fresh(c, seed, positional_encoding=True):
    """A trainable module of shape `c` with make_state_dict weights, its state dict and the oracle's config."""
    vae = build_module(c, positional_encoding)
    sd = make_state_dict({k: tuple(v.shape) for k, v in vae.state_dict().items()}, seed)
    vae.load_state_dict(sd, strict=True)
    vae = vae.cuda().train()
    vae.train_wide = True
    return vae, sd, oracle_config(c, positional_encoding)


def from_fixture(name):
    g, c = load_golden(name), CASES[name]
    vae = build_module(c)
    sd = make_state_dict({k: tuple(v) for k, v in golden_json(g, "shapes_json").items()}, int(g["seed"]))
    vae.load_state_dict(sd, strict=True)
    vae = vae.cuda().train()
    vae.train_wide = True
    return g, vae, sd, oracle_config(c)


def hip_step(vae, counts, genes, lib, counts_s, genes_s, z_weight, fused_loss=False):
    for p in vae.parameters():
        p.grad = None
    params, z = vae(cu(counts), cu(genes), cu(lib), cu(counts_s), cu(genes_s))
    if fused_loss:
        from scldm_amd.distributions import log_nb_positive
        recon = -log_nb_positive(cu(counts), params["mu"], params["theta"])
    else:
        recon = -log_nb_oracle(cu(counts), params["mu"], params["theta"])
    loss = recon.sum(dim=1).mean() + (z * cu(z_weight)).sum()
    loss.backward()
    assert vae.last_table_gradient_mode == "ordered"
    return loss.detach(), params, z.detach()


def oracle_step(key, sd, cfg, counts, genes, lib, counts_s, genes_s, zw):
    """The oracle's (loss, (mu, theta, z), grads), computed once per key and left unchanged."""
    if key not in _ORACLE:
        t = torch.from_numpy
        _ORACLE[key] = vae_training_grads(sd, cfg, t(counts), t(genes), t(lib), t(counts_s), t(genes_s), z_weight=t(zw))
    return _ORACLE[key]


def check_against_oracle(vae, loss, params, z, ref, what, shared_theta):
    loss_o, (mu_o, th_o, z_o), grads = ref
    assert abs(float(loss) - float(loss_o)) <= TOL * abs(float(loss_o)), (what, float(loss), float(loss_o))
    assert max_abs_rel(z.cpu(), z_o) < TOL and max_abs_rel(params["mu"].detach().cpu(), mu_o) < TOL, what
    wn = float(grads["decoder_head.params.weight"].norm())
    bad, worst, seen = {}, 0.0, 0
    for name_, p in vae.named_parameters():
        if name_ in FROZEN:
            assert p.grad is None
            continue
        ref_g = grads[name_]
        seen += 1
        assert p.grad is not None and p.grad.shape == ref_g.shape and torch.isfinite(p.grad).all(), name_
        if name_ == BIAS and shared_theta:
            if not float(p.grad.abs().max()) <= 1e-3 * wn:
                bad[name_] = float(p.grad.abs().max())
            continue
        e = max_abs_rel(p.grad.cpu(), ref_g) if float(ref_g.abs().max()) > 0 else float(p.grad.abs().max())
        worst = max(worst, e)
        if not e < TOL:
            bad[name_] = e
    assert seen == len(grads)
    print(f"[parity] wide VAE training {what}: worst of {seen} gradients {worst:.2e}, outside {TOL:g}: {bad}")
    assert not bad, bad


def draw(c, B, S, G, seed, repeat=False, zero_tail=False):
    rng = np.random.default_rng(seed)
    n_rows = c["n_genes"] + 1
    genes = rng.integers(0, n_rows, (B, G)).astype(np.int64)
    genes_s = rng.integers(0, n_rows, (B, S)).astype(np.int64)
    if repeat:                                  # the same gene several times inside a cell, on both sides
        genes[:, G // 2:] = genes[:, :G - G // 2]
        genes_s[:, S // 2:] = genes_s[:, :S - S // 2]
    counts = rng.poisson(0.9, (B, G)).astype(np.float32)
    counts_s = rng.poisson(0.9, (B, S)).astype(np.float32)
    if S == 1:
        counts_s[:] = 2.0
    if zero_tail:                               # padding-style tokens; the last one carries a gene that nothing else does
        counts_s[:, -max(1, S // 5):] = 0.0
        genes[genes == n_rows - 1] = 0
        genes_s[genes_s == n_rows - 1] = 0
        genes_s[:, -1] = n_rows - 1
    lib = (counts.sum(1, keepdims=True) + 1.0).astype(np.float32)
    zw = (0.3 * rng.standard_normal((B, c["n_inducing"], c["n_embed_latent"]))).astype(np.float32)
    return counts, genes, lib, counts_s, genes_s, zw


@pytest.mark.parametrize("case,name", [("vae_wide_64", "vae_wide_train_64"), ("vae_wide_128", "vae_wide_train_128")])
def test_gradients_match_reference_digests(case, name):
    g, vae, sd, cfg = from_fixture(case)
    gt = load_golden(name)
    loss, params, z = hip_step(vae, g["counts"], g["genes"], g["library_size"], g["counts_subset"], g["genes_subset"], gt["z_weight"])
    assert abs(float(loss) - float(gt["loss"])) <= TOL * abs(float(gt["loss"]))
    assert max_abs_rel(params["mu"].detach().cpu(), gt["mu"]) < TOL and max_abs_rel(z.cpu(), gt["z"]) < TOL
    assert golden_json(gt, "frozen_json") == list(FROZEN)
    wn = gt["grad_decoder_head.params.weight"][1]
    bad, seen = {}, 0
    for name_, p in vae.named_parameters():
        if name_ in FROZEN:
            assert p.grad is None
            continue
        seen += 1
        assert p.grad is not None and torch.isfinite(p.grad).all(), name_
        ref, ours = gt[f"grad_{name_}"], grad_digest(p.grad)
        if name_ == BIAS and CASES[case]["shared_theta"]:
            if not abs(ours[0]) <= 1e-3 * wn:
                bad[name_] = ours[0]
            continue
        scale = max(np.abs(ref[2:]).max(), ref[1] / np.sqrt(p.numel()))
        e = max(np.abs(ours[2:] - ref[2:]).max() / scale, abs(ours[1] - ref[1]) / (ref[1] + 1e-30))
        if not e <= TOL:
            bad[name_] = e
    assert seen == sum(k.startswith("grad_") for k in gt)
    print(f"[parity] wide VAE training {name}: {len(bad)} of {seen} gradients outside {TOL:g}")
    assert not bad, bad


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("fused_loss", [False, True])
def test_gradients_match_oracle_at_the_wide_fixture_shapes(name, fused_loss):
    g, vae, sd, cfg = from_fixture(name)
    c = CASES[name]
    zw = (0.3 * np.random.default_rng(c["seed"]).standard_normal((c["B"], c["n_inducing"], c["n_embed_latent"]))).astype(np.float32)
    args = (g["counts"], g["genes"], g["library_size"], g["counts_subset"], g["genes_subset"], zw)
    loss, params, z = hip_step(vae, *args, fused_loss=fused_loss)
    check_against_oracle(vae, loss, params, z, oracle_step(name, sd, cfg, *args), f"{name} (fused loss {fused_loss})", c["shared_theta"])


ONE_LAYER_64 = dict(CASES["vae_wide_64"], n_layer=1)


@pytest.mark.parametrize("B,S,G,repeat,zero_tail", [(5, 600, 300, False, False), (3, 65, 257, True, True), (1, 1, 1, False, False)])
def test_gradients_match_oracle_on_ragged_sizes(B, S, G, repeat, zero_tail):
    """64 wide (cross head dim 16: the pooling and its backward split at 512 keys), one layer.  (5, 600, 300): two key splits, 300 genes
    cross the 256-query block, the 256-gene NB chunk and several 64-row column partials; (3, 65, 257): one past each 64 / 256 boundary,
    genes repeated inside a cell and a tail of zero-count tokens; (1, 1, 1)."""
    vae, sd, cfg = fresh(ONE_LAYER_64, 500 + B)
    args = draw(ONE_LAYER_64, B, S, G, B * 1000 + S + G, repeat, zero_tail)
    loss, params, z = hip_step(vae, *args)
    check_against_oracle(vae, loss, params, z, oracle_step(("ragged", B, S, G), sd, cfg, *args), f"ragged ({B},{S},{G})", True)
    if zero_tail:       # a zero-count token contributes exactly zero: a gene seen only there and in no decoder slot keeps a zero row
        counts, genes, lib, counts_s, genes_s, zw = args
        live = set(genes.reshape(-1).tolist()) | set(genes_s[counts_s != 0].tolist())
        dead = sorted(set(genes_s[counts_s == 0].tolist()) - live)
        assert dead, "the draw leaves no gene that only zero-count tokens carry"
        assert not vae.input_layer.gene_embedding.weight.grad[dead].any()


def test_gradients_match_oracle_at_head_dim_128_with_40_inducing_points():
    """128 wide with n_head_cross = 1: head dim 128, 32-key chunks, the pooling split at 256 keys (S = 300: two splits); 40 inducing
    points; unshared theta, no positional encoding."""
    c = dict(n_embed=128, n_head=4, n_head_cross=1, n_inducing=40, n_embed_latent=12, n_layer=1, n_genes=150, multiple_of=4, shared_theta=False)
    vae, sd, cfg = fresh(c, 61, positional_encoding=False)
    args = draw(c, 2, 300, 70, 13)
    loss, params, z = hip_step(vae, *args)
    check_against_oracle(vae, loss, params, z, oracle_step("hd128", sd, cfg, *args), "head dim 128, 40 inducing points", False)


def _plan(vae, B, S, G, cap):
    from scldm_amd import _lib
    L, h = vae._native_wide()
    cells, chunks, nbytes = C.c_int(), C.c_int(), C.c_size_t()
    _lib.check(L.scldm_vaew_train_plan(h, B, S, G, cap, C.byref(cells), C.byref(chunks), C.byref(nbytes)), "scldm_vaew_train_plan")
    return cells.value, chunks.value, nbytes.value


def test_chunking_under_a_cap_and_bit_equal_repeats(monkeypatch):
    """B = 5 under a 2 MiB cap: chunks of two cells, the last one ragged.  The capped gradients match the oracle and the uncapped run
    (the weight gradients accumulate over the chunks: last bits may differ, nothing more), and two backward passes on the same inputs
    give bit-equal gradients, capped and uncapped."""
    c, B, S, G = ONE_LAYER_64, 5, 150, 200
    args = draw(c, B, S, G, 77)
    free, sd, cfg = fresh(c, 88)
    assert _plan(free, B, S, G, 0)[:2] == (B, 1)
    cap_mb = 2
    cells, chunks, nbytes = _plan(free, B, S, G, cap_mb << 20)
    assert chunks >= 3 and B % cells != 0 and nbytes <= cap_mb << 20, (cells, chunks, nbytes)
    monkeypatch.setenv("SCLDM_VAEW_WS_MB", str(cap_mb))
    capped = build_module(c)
    capped.load_state_dict(sd, strict=True)
    capped = capped.cuda().train()
    capped.train_wide = True
    assert _plan(capped, B, S, G, 0) == (cells, chunks, nbytes)        # the knob is read when the handle is made
    monkeypatch.delenv("SCLDM_VAEW_WS_MB")
    ref = oracle_step("chunked", sd, cfg, *args)
    got = {}
    for tag, vae in (("capped", capped), ("uncapped", free)):
        loss, params, z = hip_step(vae, *args)
        check_against_oracle(vae, loss, params, z, ref, f"B = 5, {tag}", True)
        got[tag] = {k: p.grad.clone() for k, p in vae.named_parameters() if p.grad is not None}
        hip_step(vae, *args)
        for k, p in vae.named_parameters():
            if p.grad is not None:
                assert torch.equal(p.grad, got[tag][k]), f"{tag}: {k} differs between two backward passes"
    wn = float(ref[2]["decoder_head.params.weight"].norm())
    for k, v in got["uncapped"].items():
        if k == BIAS:
            assert float((got["capped"][k] - v).abs().max()) <= 1e-3 * wn
        else:
            assert max_abs_rel(got["capped"][k].cpu(), v.cpu()) < TOL, k


def test_outputs_under_autograd_are_the_no_grad_forward_bit_for_bit():
    g, vae, sd, cfg = from_fixture("vae_wide_96")
    args = tuple(cu(g[k]) for k in ("counts", "genes", "library_size", "counts_subset", "genes_subset"))
    with torch.no_grad():
        p0, z0 = vae(*args)
    p1, z1 = vae(*args)
    assert p1["mu"].requires_grad and p1["theta"].requires_grad and z1.requires_grad and not p0["mu"].requires_grad
    assert torch.equal(p1["mu"], p0["mu"]) and torch.equal(p1["theta"], p0["theta"]) and torch.equal(z1, z0)
    for p in vae.parameters():
        p.requires_grad_(False)
    assert not vae(*args)[0]["mu"].requires_grad        # a frozen VAE: plain inference


def test_an_adamw_step_is_seen_by_the_next_forward():
    from scldm_amd.optim import AdamW
    g, vae, sd, cfg = from_fixture("vae_wide_64")
    args = tuple(cu(g[k]) for k in ("counts", "genes", "library_size", "counts_subset", "genes_subset"))
    opt = AdamW([p for p in vae.parameters() if p.requires_grad], lr=1e-2)
    params, z = vae(*args)
    loss = (-log_nb_oracle(args[0], params["mu"], params["theta"])).sum(dim=1).mean()
    loss.backward()
    opt.step()
    params2, z2 = vae(*args)                            # the wide route reads the parameters live
    assert not torch.equal(z2, z) and not torch.equal(params2["mu"], params["mu"])
    with torch.no_grad():
        p3, z3 = vae(*args)
    assert torch.equal(p3["mu"], params2["mu"]) and torch.equal(p3["theta"], params2["theta"]) and torch.equal(z3, z2)
    loss2 = (-log_nb_oracle(args[0], params2["mu"], params2["theta"])).sum(dim=1).mean()
    assert torch.isfinite(loss2) and float(loss2.detach()) < float(loss.detach())


def test_refusals():
    from scldm_amd.stochastic_layers import GaussianTransformerLayer
    g, vae, sd, cfg = from_fixture("vae_wide_64")
    args = tuple(cu(g[k]) for k in ("counts", "genes", "library_size", "counts_subset", "genes_subset"))
    vae.train_wide = False
    with pytest.raises(NotImplementedError, match="inference only"):
        vae(*args)
    vae.train_wide = True
    vae.precision = "fp16"
    with pytest.raises(NotImplementedError, match="fp16"):
        vae(*args)
    vae.precision = "fp32"
    params, z = vae(*args)
    with torch.no_grad():
        vae.decoder_head.params.weight.mul_(1.5)       # moves the version counter
    with pytest.raises(RuntimeError, match="modified between forward and backward"):
        params["mu"].sum().backward()
    vae.decoder_head = GaussianTransformerLayer(n_embed=64, norm_layer="layernorm", layernorm_eps=1e-8).cuda()
    with pytest.raises(NotImplementedError, match="Gaussian"):
        vae(*args)

"""ScviVAE (the scVI-style baseline) on the MI355X against the reference's golden vectors (tests/golden/scvi_*.npz, written by
make_golden_scvi.py from the reference's own classes): parity of forward / encode / decode, the row sums of mu, run-to-run and
batch-composition bit-equality, the fingerprint-guarded re-pack, the fused negative-binomial draw and graph capture."""
import functools

import numpy as np
import pytest
import torch

from conftest import check_err, golden_json, load_golden
from scvi_ref import CASES, OUTPUTS, build_scvi, make_scvi_state_dict, scvi_forward

pytestmark = pytest.mark.gpu
TOL = 1e-4          # the project's standing fp32 gate: max abs error over max abs reference


@functools.lru_cache(maxsize=None)
def case(name):
    """(golden arrays, state dict, eval-mode model on the device, device inputs): built once per fixture and never modified -
    the re-pack test works on a copy of its own."""
    g = load_golden(name)
    shapes = {k: tuple(v) for k, v in golden_json(g, "shapes_json").items()}
    sd = make_scvi_state_dict(shapes, int(g["seed"]))
    return g, sd, fresh_model(name, sd), {k: torch.from_numpy(g[k]).cuda() for k in ("counts", "library_size", "eps")}


def fresh_model(name, sd):
    n_genes, n_hidden, n_latent, n_layers, B, shared, seed = CASES[name]
    vae = build_scvi(n_genes, n_hidden, n_latent, n_layers, shared)
    vae.load_state_dict(sd, strict=True)
    return vae.cuda().eval()


def run_forward(vae, x, rows=slice(None)):
    lik, post, z = vae(x["counts"][rows], None, x["library_size"][rows], eps=x["eps"][rows])
    # h as the forward entry itself writes it (forward drops it); encode_hidden's copy is compared against it in the parity test
    h = vae.forward_outputs(x["counts"][rows], x["library_size"][rows], x["eps"][rows])["h"]
    return {"h": h, "loc": post.loc, "scale": post.scale, "z": z, "mu": lik.mu, "theta": lik.theta}


@pytest.mark.parametrize("name", sorted(CASES))
def test_forward_encode_decode_match_the_reference(name):
    g, sd, vae, x = case(name)
    n_genes, n_hidden, n_latent, n_layers, B, shared, seed = CASES[name]
    out = run_forward(vae, x)
    for k in OUTPUTS:
        assert out[k].shape == g[k].shape and out[k].dtype == torch.float32, k
        check_err(out[k].cpu(), g[k], TOL, f"{name} forward {k}")
    assert type(vae(x["counts"], None, x["library_size"])[0]).__name__ == "NegativeBinomial"       # eps drawn by the module
    # mu.sum(1) equals library_size
    row = out["mu"].double().sum(1).cpu().numpy()
    rel = np.abs(row / g["library_size"].astype(np.float64) - 1).max()
    print(f"[parity] {name}: max |mu.sum(1) / library_size - 1| = {rel:.3e}")
    assert rel < 1e-5
    # encode: the posterior alone; decode: from the reference's z, library_size as (B, 1)
    post = vae.encode(x["counts"])
    assert isinstance(post, torch.distributions.Normal)
    assert torch.equal(post.loc, out["loc"]) and torch.equal(post.scale, out["scale"])
    h2, loc2, scale2, z2 = vae.encode_hidden(x["counts"], x["eps"])
    assert torch.equal(h2, out["h"]) and torch.equal(z2, out["z"]) and torch.equal(loc2, out["loc"])
    nb = vae.decode(torch.from_numpy(g["z"]).cuda(), None, x["library_size"][:, None])
    check_err(nb.mu.cpu(), g["mu"], TOL, f"{name} decode mu")
    check_err(nb.theta.cpu(), g["theta"], TOL, f"{name} decode theta")
    assert nb.theta.shape == ((n_genes,) if shared else (B, n_genes))


@pytest.mark.parametrize("name", sorted(CASES))
def test_two_runs_and_split_batches_give_the_same_bits(name):
    g, sd, vae, x = case(name)
    B = CASES[name][4]
    a, b = run_forward(vae, x), run_forward(vae, x)
    for k in OUTPUTS:
        assert torch.equal(a[k], b[k]), f"{name} {k}: two runs differ"
    cut = 3 if B == 5 else 64            # [0, 3) + [3, 5); one full row tile + the tail
    lo, hi = run_forward(vae, x, slice(0, cut)), run_forward(vae, x, slice(cut, B))
    for k in OUTPUTS:
        if a[k].dim() == 1:              # shared theta (G): no batch axis
            assert torch.equal(lo[k], a[k]) and torch.equal(hi[k], a[k])
        else:
            assert torch.equal(torch.cat([lo[k], hi[k]]), a[k]), f"{name} {k}: a row's bits depend on the batch's other rows"


def test_changed_running_var_is_repacked_by_the_fingerprint_guard():
    name = "scvi_small"
    g, sd, _, x = case(name)
    vae = fresh_model(name, sd)
    before = run_forward(vae, x)
    check_err(before["mu"].cpu(), g["mu"], TOL, "before the update: mu")
    key = "encoder.encoder_mlp.1.running_var"
    bn = vae.encoder.encoder_mlp[1]
    ptr = bn.running_var.data_ptr()
    bn.running_var.mul_(1.7).add_(0.05)                  # in place: same storage
    assert bn.running_var.data_ptr() == ptr
    sd2 = dict(sd)
    sd2[key] = sd[key] * 1.7 + 0.05
    t = torch.from_numpy
    ref = scvi_forward(sd2, t(g["counts"]), t(g["library_size"]), t(g["eps"]))
    after = run_forward(vae, x)
    assert not torch.equal(after["h"], before["h"]) and not torch.equal(after["mu"], before["mu"])
    for k in OUTPUTS:
        check_err(after[k].cpu(), ref[k], TOL, f"after the running_var update: {k}")
    # ... and a parameter of the decoder, through .data (invisible to the version counters)
    vae.decoder.decoder_mlp[1].bias.data.add_(0.25)
    sd2["decoder.decoder_mlp.1.bias"] = sd["decoder.decoder_mlp.1.bias"] + 0.25
    ref = scvi_forward(sd2, t(g["counts"]), t(g["library_size"]), t(g["eps"]))
    check_err(run_forward(vae, x)["mu"].cpu(), ref["mu"], TOL, "after the decoder BatchNorm bias update: mu")


@pytest.mark.parametrize("name", ["scvi_small", "scvi_small_unshared"])
def test_sample_of_the_likelihood_is_the_fused_negative_binomial_draw(name):
    g, sd, vae, x = case(name)
    n_genes, B = CASES[name][0], CASES[name][4]
    lik = vae(x["counts"], None, x["library_size"], eps=x["eps"])[0]
    s = lik.sample(seed=11)
    assert s.shape == (B, n_genes) and s.dtype == torch.float32 and s.is_cuda
    assert bool((s >= 0).all()) and torch.equal(s, s.round()) and float(s.sum()) > 0
    assert torch.equal(s, lik.sample(seed=11))


def test_forward_is_captured_into_a_graph_and_replays_to_the_same_bits():
    name = "scvi_tiles"
    g, sd, vae, x = case(name)
    eager = run_forward(vae, x)
    static = {k: v.clone() for k, v in x.items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                         # warm-up on the capture stream (workspace, packed vectors)
        vae(static["counts"], None, static["library_size"], eps=static["eps"])
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lik, post, z = vae(static["counts"], None, static["library_size"], eps=static["eps"])
    for k in ("mu", "z"):
        (lik.mu if k == "mu" else z).zero_()
    graph.replay()
    torch.cuda.synchronize()
    got = {"loc": post.loc, "scale": post.scale, "z": z, "mu": lik.mu, "theta": lik.theta}
    for k, v in got.items():
        assert torch.equal(v, eager[k]), f"graph replay: {k} differs from the eager call"
    # new inputs in the static buffers: the replay computes them
    static["counts"].copy_(x["counts"].flip(0))
    static["library_size"].copy_(x["library_size"].flip(0))
    static["eps"].copy_(x["eps"].flip(0))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(lik.mu, eager["mu"].flip(0)) and torch.equal(z, eager["z"].flip(0))

"""GPU gates of the TransformerVAE training step at precision="fp16": the reference's own training arithmetic
(experiments/scripts/train.py:18, set_float32_matmul_precision("high") = TF32 operands, fp32 accumulation).  fp16 operands carry
TF32's 10 mantissa bits; the yardstick is autograd over the oracle with every matmul operand - forward and both backward products -
rounded to 10 bits (oracle.dit.matmul_operand_bits), both measured against the exact-fp32 oracle: every gradient within 1.5 x the
TF32 oracle's error (the DiT precedent, test_gpu_train.py) on the 2 000-gene fixture.  On a few dozen genes (the 50-gene fixture, the
ragged shapes) both errors are sums of few rounding errors with large cancellation (the cell side's gradients arrive through
dK | dV = sums over the genes of outer products whose rows sum to zero), so the per-parameter ratio of two such random quantities
spreads: measured 1.6-2.5 for single small tensors there (LayerNorm vectors of the trunks), 0.3-1.7 for the whole step's worst
gradient.  Those shapes are gated at 3 x per tensor and 2 x for the worst gradient."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle.dit import matmul_operand_bits
from oracle.vae_train import FROZEN, log_nb_positive as log_nb_oracle, vae_training_grads
from test_gpu_vae_train import BIAS, build, cu, hip_step

pytestmark = pytest.mark.gpu
ATOMIC = ("input_layer.gene_embedding.weight", "decoder_head.theta.weight")   # scatter-added with float atomics (README "Parity")


def rel_l2(a, b) -> float:
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    n = float(b.norm())
    return float((a - b).norm()) / n if n > 0 else float(a.norm())


def oracles(sd, cfg, counts, genes, lib, counts_s, genes_s, zw=None):
    t = lambda a: None if a is None else torch.from_numpy(np.asarray(a))
    args = (sd, cfg, t(counts), t(genes), t(lib), t(counts_s), t(genes_s))
    exact = vae_training_grads(*args, z_weight=t(zw))
    with matmul_operand_bits(10):
        tf32 = vae_training_grads(*args, z_weight=t(zw))
    return exact, tf32


def errors(vae, loss, mu, z, exact, tf32, grad_div=1.0):
    """{name: (error of the HIP step, error of the TF32-operand oracle)} against the exact oracle, for loss, mu, z and every gradient"""
    (loss_e, (mu_e, _, z_e), g_e), (loss_t, (mu_t, _, z_t), g_t) = exact, tf32
    out = {"loss": (abs(float(loss) - float(loss_e)) / abs(float(loss_e)), abs(float(loss_t) - float(loss_e)) / abs(float(loss_e))),
           "mu": (rel_l2(mu, mu_e), rel_l2(mu_t, mu_e)), "z": (rel_l2(z, z_e), rel_l2(z_t, z_e))}
    for name, p in vae.named_parameters():
        if name in FROZEN or name == BIAS:
            continue
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
        out[name] = (rel_l2(p.grad / grad_div, g_e[name]), rel_l2(g_t[name], g_e[name]))
    return out


def check_gate(vae, errs, g_exact, what, factor=1.5, worst_factor=1.5):
    worst = max(v[0] for k, v in errs.items() if k not in ("loss", "mu", "z"))
    worst_t = max(v[1] for k, v in errs.items() if k not in ("loss", "mu", "z"))
    rk, rv = max(errs.items(), key=lambda kv: kv[1][0] / (kv[1][1] + 1e-5))
    print(f"[parity] VAE fp16 training {what}: worst gradient rel-L2 fp16 {worst:.2e}, TF32-operand oracle {worst_t:.2e}, ratio "
          f"{worst / max(worst_t, 1e-30):.2f}; largest per-tensor ratio {rv[0] / (rv[1] + 1e-5):.2f} ({rk}); mu {errs['mu'][0]:.2e} / "
          f"{errs['mu'][1]:.2e}, z {errs['z'][0]:.2e} / {errs['z'][1]:.2e}")
    bad = {k: v for k, v in errs.items() if not v[0] <= factor * v[1] + 1e-5}
    assert not bad, bad
    assert worst <= worst_factor * worst_t + 1e-5
    wn = float(g_exact["decoder_head.params.weight"].norm())
    assert abs(float(vae.decoder_head.params.bias.grad)) <= 1e-3 * wn     # mathematically zero (softmax over genes is shift-invariant)
    return worst


_ORACLES = {}


def fixture(name):
    """golden inputs, the HIP module and the two oracles of one fixture (one oracle evaluation per fixture and module)"""
    g = load_golden(name)
    vae, sd, cfg = build(int(g["n_genes"]), int(g["seed"]))
    inputs = (g["counts"], g["genes"], g["library_size"], g["counts_subset"], g["genes_subset"])
    if name not in _ORACLES:
        _ORACLES[name] = oracles(sd, cfg, *inputs)
    return vae, inputs, _ORACLES[name]


@pytest.mark.parametrize("name", ["vae_train_small", "vae_train_2000"])
def test_fp16_training_is_in_the_references_tf32_class(name):
    vae, inputs, (exact, tf32) = fixture(name)
    vae.precision = "fp16"
    flag = vae.found_inf_flag()
    loss, params, z = hip_step(vae, *inputs)
    errs = errors(vae, loss, params["mu"], z, exact, tf32)
    worst16 = check_gate(vae, errs, exact[2], name, *((1.5, 1.5) if name == "vae_train_2000" else (3.0, 2.0)))
    assert float(flag) == 0.0
    # the same inputs in fp32: several times closer (the fp16 operands are really used)
    vae.precision = "fp32"
    loss32, params32, z32 = hip_step(vae, *inputs)
    worst32 = max(v[0] for k, v in errors(vae, loss32, params32["mu"], z32, exact, tf32).items() if k not in ("loss", "mu", "z"))
    print(f"[parity] VAE training {name}: worst gradient rel-L2 fp32 {worst32:.2e} vs fp16 {worst16:.2e}")
    assert 5 * worst32 <= worst16


@pytest.mark.parametrize("B,S,G,n_genes", [(5, 70, 130, 200), (9, 64, 65, 300), (1, 1, 1, 50)])
def test_fp16_gradients_on_ragged_sizes_with_a_gradient_through_z(B, S, G, n_genes):
    """Batches and gene axes that fill no tile, S = G = 1, repeated genes in a cell (scatter-add into one embedding row), padding
    tokens with zero counts, and a loss term on the returned latent."""
    vae, sd, cfg = build(n_genes, 300 + B)
    vae.precision = "fp16"
    rng = np.random.default_rng(B * 100 + G)
    genes = rng.integers(0, n_genes + 1, (B, G)).astype(np.int64)
    genes[:, -1] = genes[:, 0]
    counts = rng.poisson(0.9, (B, G)).astype(np.float32)
    genes_s = rng.integers(0, n_genes + 1, (B, S)).astype(np.int64)
    counts_s = rng.poisson(0.9, (B, S)).astype(np.float32)
    counts_s[:, -max(1, S // 5):] = 0.0
    lib = (counts.sum(1, keepdims=True) + 1.0).astype(np.float32)
    zw = (0.3 * rng.standard_normal((B, 16, 16))).astype(np.float32)
    exact, tf32 = oracles(sd, cfg, counts, genes, lib, counts_s, genes_s, zw)
    loss, params, z = hip_step(vae, counts, genes, lib, counts_s, genes_s, z_weight=zw)
    check_gate(vae, errors(vae, loss, params["mu"], z, exact, tf32), exact[2], f"B={B} S={S} G={G}", 3.0, 2.0)
    assert float(vae.found_inf_flag()) == 0.0


def test_tiny_gradients_keep_their_precision():
    """Loss times 1e-6: without the per-cell power-of-two scale the fp16 gradient operands would underflow."""
    vae, inputs, (exact, tf32) = fixture("vae_train_small")
    vae.precision = "fp16"
    for p in vae.parameters():
        p.grad = None
    counts, genes, lib, counts_s, genes_s = inputs
    params, z = vae(cu(counts), cu(genes), cu(lib), cu(counts_s), cu(genes_s))
    loss = (-log_nb_oracle(cu(counts), params["mu"], params["theta"])).sum(dim=1).mean()
    (loss * 1e-6).backward()
    errs = errors(vae, loss.detach(), params["mu"], z.detach(), exact, tf32, grad_div=1e-6)
    errs.pop("loss")
    check_gate(vae, errs, {k: v * 1e-6 for k, v in exact[2].items()}, "loss x 1e-6", 3.0, 2.0)
    assert float(vae.found_inf_flag()) == 0.0


def test_overflow_sets_the_flag_and_adamw_skips_the_step():
    """Gene embeddings and the decoder's two c_proj weights times 1e-3, the head weight scaled to |w| <= 1000 (every weight inside the
    fp16 range, the logits of the forward unsaturated): d y = dlogit * w_head + ... of the scaled backward leaves the fp16 range.  The
    flag reads 1, scldm_amd.optim.AdamW with found_inf leaves every parameter bit-identical, and the next clean step resets the
    flag.  (A numeric inf, not a GPU fault.)"""
    from scldm_amd.optim import AdamW
    g = load_golden("vae_train_2000")
    vae, sd, cfg = build(int(g["n_genes"]), int(g["seed"]))
    inputs = (g["counts"], g["genes"], g["library_size"], g["counts_subset"], g["genes_subset"])
    clean = {k: v.clone() for k, v in vae.state_dict().items()}
    with torch.no_grad():
        vae.input_layer.gene_embedding.weight.mul_(1e-3)
        vae.decoder.decoder_cross_attention.attn.c_proj.weight.mul_(1e-3)
        vae.decoder.decoder_cross_attention.mlp.c_proj.weight.mul_(1e-3)
        w = vae.decoder_head.params.weight
        w.mul_(1e3 / float(w.abs().max()))
        assert all(float(p.abs().max()) < 65504 for p in vae.parameters())
    vae.precision = "fp16"
    flag = vae.found_inf_flag()
    loss, params, z = hip_step(vae, *inputs)
    mu = params["mu"].detach()
    assert torch.isfinite(mu).all() and torch.isfinite(loss)
    assert int(((mu / mu.sum(1, keepdim=True)) > 1e-4).sum(1).min()) >= 10      # the softmax over genes is not saturated
    assert float(flag) == 1.0
    opt = AdamW(vae.parameters(), lr=1e-3)
    opt.found_inf = flag
    before = [p.detach().clone() for p in vae.parameters()]
    opt.step()
    torch.cuda.synchronize()
    assert all(torch.equal(a, p.detach()) for a, p in zip(before, vae.parameters()))
    with torch.no_grad():
        vae.load_state_dict(clean)
    hip_step(vae, *inputs)
    assert float(flag) == 0.0 and all(torch.isfinite(p.grad).all() for p in vae.parameters() if p.grad is not None)


def test_switching_precision_on_one_module():
    """fp32 -> fp16 -> fp32 on the same module: the second fp32 step reproduces the first bit for bit; two fp16 steps agree bit for bit
    (both except the two atomically accumulated tables, which vary in the last bits in fp32 as well)."""
    g = load_golden("vae_train_2000")
    vae, sd, cfg = build(int(g["n_genes"]), int(g["seed"]))
    inputs = (g["counts"], g["genes"], g["library_size"], g["counts_subset"], g["genes_subset"])

    def grads(prec):
        vae.precision = prec
        hip_step(vae, *inputs)
        return {n: p.grad.clone() for n, p in vae.named_parameters() if p.grad is not None}

    a32, a16, b32, b16 = grads("fp32"), grads("fp16"), grads("fp32"), grads("fp16")
    for n in a32:
        if n in ATOMIC:
            continue
        assert torch.equal(a32[n], b32[n]), n
        assert torch.equal(a16[n], b16[n]), n
    assert any(not torch.equal(a32[n], a16[n]) for n in a32)


def test_training_loop_at_the_dentate_shape_in_fp16():
    """BASELINE configs[0] shape at fp16: batch 32, G = 17 002, S = 6 147; 20 steps of scldm_amd.optim.AdamW with the overflow flag
    as found_inf.  The loss falls as in the fp32 loop (test_gpu_vae_train.py) and the flag stays 0."""
    from scldm_amd.datamodule import tokenize_cells_expressed
    from scldm_amd.distributions import log_nb_positive
    from scldm_amd.optim import AdamW
    G, S, B, n_genes = 17002, 6147, 32, 17002
    vae, sd, cfg = build(n_genes, 401)
    with torch.no_grad():
        vae.input_layer.gene_embedding.weight.normal_(0, 1.0)
        vae.encoder.ca_layer.inducing_points.normal_(0, 1.0)
        vae.decoder_head.theta.weight.fill_(1.0)
    vae.precision = "fp16"
    rng = np.random.default_rng(5)
    rate = rng.gamma(0.3, 2.0, (1, G)).astype(np.float32)
    counts = rng.poisson(rate * rng.uniform(0.5, 1.5, (B, 1))).astype(np.float32)
    genes = np.tile(np.arange(G, dtype=np.int64), (B, 1))
    tok = tokenize_cells_expressed(cu(counts), cu(genes[0]), S, n_genes)
    lib = cu(counts).sum(1, keepdim=True)
    opt = AdamW(vae.parameters(), lr=2e-3)
    opt.found_inf = vae.found_inf_flag()
    losses, flags = [], []
    for _ in range(20):
        opt.zero_grad(set_to_none=True)
        params, z = vae(cu(counts), cu(genes), lib, tok["counts_subset"], tok["genes_subset"])
        loss = (-log_nb_positive(cu(counts), params["mu"], params["theta"])).sum(dim=1).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss))
        flags.append(float(opt.found_inf))
    print(f"[parity] VAE fp16 training loop (B=32, G=17002, S=6147): loss {losses[0]:.1f} -> {losses[-1]:.1f}")
    assert flags == [0.0] * 20
    assert all(np.isfinite(losses)) and losses[-1] < 0.97 * losses[0] and min(losses[10:]) < min(losses[:5])


def test_bf16_training_and_the_unshared_head_still_raise():
    from test_gpu_vae import build as build_inference
    g = load_golden("vae_train_small")
    vae, sd, cfg = build(int(g["n_genes"]), int(g["seed"]))
    vae.precision = "bf16"
    with pytest.raises(NotImplementedError, match="fp32 or fp16"):
        hip_step(vae, g["counts"], g["genes"], g["library_size"], g["counts_subset"], g["genes_subset"])
    gu, vu, _, _ = build_inference("vae_unshared")
    vu.train()
    for prec in ("fp16", "bf16", "fp32"):
        vu.precision = prec
        with pytest.raises(NotImplementedError, match="shared-theta"):
            vu(cu(gu["counts"]), cu(gu["genes"]), cu(gu["library_size"]), cu(gu["counts_subset"]), cu(gu["genes_subset"]))

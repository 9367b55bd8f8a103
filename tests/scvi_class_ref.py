"""The eval-mode forward of tests/scvi_ref.py with every product routed through `oracle.dit.linear`, so that
`oracle.dit.matmul_operand_bits(b)` rounds both operands of all its products to b explicit mantissa bits (b = 10: the reference's
TF32 class, which ScviVAE's fp16 path is gated against; None: exact).  BatchNorm, SiLU, hardtanh / exp, softmax and softplus stay
plain torch.  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle.dit import linear
from scvi_ref import BN_EPS


def _mlp(sd, prefix, x, bn_eps):
    i = 0
    while f"{prefix}.{4 * i}.weight" in sd:
        lin, bn = f"{prefix}.{4 * i}", f"{prefix}.{4 * i + 1}"
        x = linear(x, sd[lin + ".weight"], sd[lin + ".bias"])
        x = F.batch_norm(x, sd[bn + ".running_mean"], sd[bn + ".running_var"], sd[bn + ".weight"], sd[bn + ".bias"], False, 0.0, bn_eps)
        x = F.silu(x)
        i += 1
    return x


def encode(sd, counts, eps=None, bn_eps=BN_EPS):
    """(h, loc, scale, z) - z is None without eps."""
    h = _mlp(sd, "encoder.encoder_mlp", torch.log1p(counts), bn_eps)
    loc = linear(h, sd["encoder_head.loc.weight"], sd["encoder_head.loc.bias"])
    log_scale = linear(h, sd["encoder_head.scale.weight"], sd["encoder_head.scale.bias"])
    scale = torch.exp(F.hardtanh(log_scale, min_val=-7.0, max_val=5.0))
    return h, loc, scale, (loc + eps * scale if eps is not None else None)


def decode(sd, z, library_size, bn_eps=BN_EPS):
    """(mu, theta)."""
    g = _mlp(sd, "decoder.decoder_mlp", z, bn_eps)
    logits = linear(g, sd["decoder_head.mu.weight"], sd["decoder_head.mu.bias"])
    if "decoder_head.theta" in sd:
        theta = F.softplus(sd["decoder_head.theta"])
    else:
        theta = F.softplus(linear(g, sd["decoder_head.theta.weight"], sd["decoder_head.theta.bias"]))
    return F.softmax(logits, dim=1) * library_size.reshape(-1, 1), theta


def forward(sd, counts, library_size, eps, bn_eps=BN_EPS):
    """{h, loc, scale, z, mu, theta} of the eval-mode forward, under whatever operand rounding is active."""
    h, loc, scale, z = encode(sd, counts, eps, bn_eps)
    mu, theta = decode(sd, z, library_size, bn_eps)
    return {"h": h, "loc": loc, "scale": scale, "z": z, "mu": mu, "theta": theta}


# ---- the inputs the GPU tests (tests/test_gpu_scvi_fp16.py) and the CPU mutation test share ---------------------------------------
# the case without a fixture: K > 1 024 outside the first layer (n_hidden 1 030), in both dual-weight epilogues (POST and LIK2)
WIDE = ("scvi_wide_hidden", (67, 1030, 4, 2, 3, False, 704))      # name, (n_genes, n_hidden, n_latent, n_layers, B, shared_theta, seed)


def case_inputs(name):
    """(state dict, counts, library_size, eps) as CPU tensors of a case of scvi_ref.CASES or of WIDE, from the deterministic
    builders of scvi_ref (which the fixtures were generated with)."""
    from scvi_ref import CASES, make_inputs, make_scvi_state_dict, scvi_shapes
    n_genes, n_hidden, n_latent, n_layers, B, shared, seed = WIDE[1] if name == WIDE[0] else CASES[name]
    sd = make_scvi_state_dict(scvi_shapes(n_genes, n_hidden, n_latent, n_layers, shared), seed)
    counts, lib, eps = (torch.from_numpy(v) for v in make_inputs(n_genes, n_latent, B, seed))
    return sd, counts, lib, eps


def case_dims(name):
    from scvi_ref import CASES
    return WIDE[1] if name == WIDE[0] else CASES[name]


ALL_CASES = ("scvi_small", "scvi_small_unshared", "scvi_tiles", WIDE[0])

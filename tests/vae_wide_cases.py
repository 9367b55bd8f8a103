"""The four wide TransformerVAE fixtures (tests/golden/vae_wide_*.npz), shared by tests/golden/make_golden_vae_wide.py and the tests
that read them, and the builders of our module / the oracle's config for a shape of the family."""
from __future__ import annotations

# name: n_embed, n_head, n_head_cross, n_inducing, n_embed_latent, n_layer, n_genes, G, S, B, multiple_of, shared_theta, seed
CASES = {
    "vae_wide_64": dict(n_embed=64, n_head=8, n_head_cross=4, n_inducing=16, n_embed_latent=16, n_layer=2, n_genes=300, G=97, S=41, B=3,
                        multiple_of=4, shared_theta=True, seed=7101),
    "vae_wide_128": dict(n_embed=128, n_head=4, n_head_cross=2, n_inducing=32, n_embed_latent=24, n_layer=2, n_genes=300, G=130, S=70, B=2,
                         multiple_of=4, shared_theta=False, seed=7102),
    "vae_wide_256": dict(n_embed=256, n_head=8, n_head_cross=4, n_inducing=16, n_embed_latent=16, n_layer=1, n_genes=500, G=200, S=100, B=2,
                         multiple_of=4, shared_theta=True, seed=7103),
    "vae_wide_96": dict(n_embed=96, n_head=3, n_head_cross=6, n_inducing=8, n_embed_latent=8, n_layer=1, n_genes=200, G=65, S=33, B=2,
                        multiple_of=5, shared_theta=True, seed=7104),
}
HIDDEN = {"vae_wide_64": 172, "vae_wide_128": 344, "vae_wide_256": 684, "vae_wide_96": 260}   # the SwiGLU widths: none a multiple of 32


def module_kwargs(c: dict, positional_encoding: bool = True):
    """(Encoder kwargs, Decoder kwargs, head kwargs, input-layer kwargs) in the reference's constructor vocabulary."""
    common = dict(n_embed=c["n_embed"], n_embed_latent=c["n_embed_latent"], n_head=c["n_head"], n_head_cross=c["n_head_cross"],
                  n_layer=c["n_layer"], n_inducing_points=c["n_inducing"], dropout=0.0, bias=False, multiple_of=c["multiple_of"],
                  layernorm_eps=1e-8, norm_layer="layernorm")
    enc = dict(common, positional_encoding=positional_encoding)
    dec = dict(common, n_genes=c["n_genes"], shared_embedding=True, use_adaln=False)
    head = dict(n_genes=c["n_genes"], shared_theta=c["shared_theta"], n_embed=c["n_embed"], norm_layer="layernorm", layernorm_eps=1e-8)
    inp = dict(n_genes=c["n_genes"], n_embed=c["n_embed"], agg_func="log1p")
    return enc, dec, head, inp


def build_module(c: dict, positional_encoding: bool = True):
    """scldm_amd.vae.TransformerVAE of a case (parameters on the CPU, default initialisation)."""
    from scldm_amd.layers import InputTransformerVAE
    from scldm_amd.nnets import Decoder, Encoder
    from scldm_amd.stochastic_layers import NegativeBinomialTransformerLayer
    from scldm_amd.vae import TransformerVAE
    enc, dec, head, inp = module_kwargs(c, positional_encoding)
    return TransformerVAE(encoder=Encoder(**enc), decoder=Decoder(**dec), decoder_head=NegativeBinomialTransformerLayer(**head),
                          input_layer=InputTransformerVAE(**inp))


def oracle_config(c: dict, positional_encoding: bool = True):
    from oracle.vae import VAEConfig
    return VAEConfig(n_genes=c["n_genes"], n_embed=c["n_embed"], n_inducing_points=c["n_inducing"], n_embed_latent=c["n_embed_latent"],
                     n_layer=c["n_layer"], n_head=c["n_head"], n_head_cross=c["n_head_cross"], multiple_of=c["multiple_of"],
                     positional_encoding=positional_encoding)

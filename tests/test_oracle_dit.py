"""Pin the CPU oracle (oracle/dit.py) against golden vectors produced by the reference's own
DiT (tests/golden/make_golden.py).  CPU only."""
import numpy as np
import pytest
import torch

from conftest import golden_json, load_golden, max_abs_rel
from oracle.dit import DiTConfig, dit_flops_per_sample, dit_forward, dit_forward_with_cfg, layer_norm, mlp_hidden_dim
from oracle.weights import make_state_dict

CASES = ["dit_tiny", "dit_base", "dit_joint", "dit_me2", "dit_me2_256"]
TOL = 2e-5  # fp32 oracle vs fp32 reference, different summation order


def setup(name, dtype=torch.float32):
    g = load_golden(name)
    kw = golden_json(g, "kwargs_json")
    shapes = {k: tuple(v) for k, v in golden_json(g, "shapes_json").items()}
    sd = make_state_dict(shapes, int(g["seed"]), dtype=dtype)
    cfg = DiTConfig(n_embed=kw["n_embed"], n_embed_input=kw["n_embed_input"], n_layer=kw["n_layer"], n_head=kw["n_head"],
                    seq_len=kw["seq_len"], multiple_of=kw["multiple_of"], layernorm_eps=kw["layernorm_eps"],
                    class_vocab_sizes=kw["class_vocab_sizes"], condition_strategy=kw["condition_strategy"])
    return g, cfg, sd


@pytest.mark.parametrize("name", CASES)
def test_forward_matches_reference(name):
    g, cfg, sd = setup(name)
    cond = {k: torch.from_numpy(g[f"fwd_label_{k}"]) for k in golden_json(g, "fwd_classes")}
    taps = {}
    y = dit_forward(sd, cfg, torch.from_numpy(g["fwd_x"]), torch.from_numpy(g["fwd_t"]), cond, taps=taps)
    assert max_abs_rel(y, g["fwd_out"]) < TOL
    for ours, theirs in (("block0.mod1", "tap_block0.mod1"), ("block0.attn_out", "tap_block0.attn_out"),
                         ("block0.mod2", "tap_block0.mod2"), ("block0.mlp_out", "tap_block0.mlp_out")):
        assert max_abs_rel(taps[ours], g[theirs]) < TOL, ours


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("tag", ["s1", "s2"])
def test_forward_with_cfg_matches_reference(name, tag):
    g, cfg, sd = setup(name)
    cond = {k: torch.from_numpy(g[f"cfg_label_{k}"]) for k in cfg.class_vocab_sizes}
    scales = golden_json(g, f"cfg_scales_{tag}")
    y = dit_forward_with_cfg(sd, cfg, torch.from_numpy(g["cfg_x"]), torch.from_numpy(g["cfg_t"]), cond, scales)
    assert max_abs_rel(y, g[f"cfg_out_{tag}"]) < TOL


# SwiGLU hidden widths other than the 684 of multiple_of=4 (tests/golden/make_golden_hidden.py): name -> (multiple_of, hidden width)
HIDDEN_CASES = {"dit_h768": (256, 768), "dit_h704": (64, 704), "dit_h700": (100, 700), "dit_h832": (832, 832), "dit_h682": (2, 682)}


@pytest.mark.parametrize("name", sorted(HIDDEN_CASES))
def test_other_hidden_widths_match_reference(name):
    """Forward, the SwiGLU output of block 0 and the CFG forward at the reference's own hidden width for this multiple_of: pins
    oracle.dit.mlp_hidden_dim (and, below, scldm_amd's swiglu_hidden) to the reference module's w1 row count."""
    from scldm_amd.layers import swiglu_hidden
    g, cfg, sd = setup(name)
    multiple_of, hidden = HIDDEN_CASES[name]
    assert cfg.multiple_of == multiple_of and int(g["hidden"]) == hidden
    assert golden_json(g, "shapes_json")["blocks.0.mlp.w1.weight"] == [hidden, 256]           # the reference module's own shape
    assert mlp_hidden_dim(256, multiple_of) == hidden == swiglu_hidden(256, multiple_of)
    assert tuple(sd["blocks.1.mlp.c_proj.weight"].shape) == (256, hidden)
    cond = {"clusters": torch.from_numpy(g["fwd_label_clusters"])}
    taps = {}
    y = dit_forward(sd, cfg, torch.from_numpy(g["fwd_x"]), torch.from_numpy(g["fwd_t"]), cond, taps=taps)
    assert max_abs_rel(y, g["fwd_out"]) < TOL
    assert max_abs_rel(taps["block0.mlp_out"], g["tap_block0.mlp_out"]) < TOL
    cond2 = {"clusters": torch.from_numpy(g["cfg_label_clusters"])}
    y2 = dit_forward_with_cfg(sd, cfg, torch.from_numpy(g["cfg_x"]), torch.from_numpy(g["cfg_t"]), cond2, golden_json(g, "cfg_scales_s2"))
    assert max_abs_rel(y2, g["cfg_out_s2"]) < TOL


def test_oracle_and_package_agree_on_the_hidden_width():
    from scldm_amd.layers import swiglu_hidden
    for n_embed in (256, 512, 1024):
        for multiple_of in (1, 2, 4, 5, 7, 64, 100, 256, 683, 832, 1024):
            h = mlp_hidden_dim(n_embed, multiple_of)
            assert h == swiglu_hidden(n_embed, multiple_of) and h % multiple_of == 0 and 0 <= h - int(8 * n_embed / 3) < multiple_of


def test_fp64_oracle_is_closer_than_tolerance():
    g, cfg, sd = setup("dit_base", torch.float64)
    cond = {k: torch.from_numpy(g[f"fwd_label_{k}"]) for k in golden_json(g, "fwd_classes")}
    y = dit_forward(sd, cfg, torch.from_numpy(g["fwd_x"]), torch.from_numpy(g["fwd_t"]), cond)
    assert y.dtype == torch.float64 and max_abs_rel(y, g["fwd_out"]) < TOL


def test_modulate_argument_swap_kat():
    """chunk 0 acts as the SCALE in Block; 'fixing' the order must break parity."""
    g, cfg, sd = setup("dit_tiny")
    x = torch.from_numpy(g["fwd_x"])
    cond = {k: torch.from_numpy(g[f"fwd_label_{k}"]) for k in golden_json(g, "fwd_classes")}
    taps = {}
    dit_forward(sd, cfg, x, torch.from_numpy(g["fwd_t"]), cond, taps=taps)
    c = taps["c"]
    m = torch.nn.functional.silu(c) @ sd["blocks.0.adaln_modulation.1.weight"].T + sd["blocks.0.adaln_modulation.1.bias"]
    a0, a1 = m.chunk(6, dim=-1)[:2]
    ln = layer_norm(taps["h0"], cfg.layernorm_eps)
    as_reference = ln * (1 + a0) + a1
    as_named = ln * (1 + a1) + a0
    assert max_abs_rel(as_reference, g["tap_block0.mod1"]) < TOL
    assert max_abs_rel(as_named, g["tap_block0.mod1"]) > 1e-2


def test_shapes_and_flops():
    assert mlp_hidden_dim(256, 4) == 684 and mlp_hidden_dim(32, 4) == 88
    assert dit_flops_per_sample(DiTConfig(class_vocab_sizes={"clusters": 14})) == 210_763_776
    g = load_golden("dit_base")
    shapes = golden_json(g, "shapes_json")
    assert len(shapes) == 84 and shapes["blocks.0.mlp.w1.weight"] == [684, 256]
    assert sum(int(np.prod(v)) for v in shapes.values()) == 9_745_424

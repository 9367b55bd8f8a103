"""CPU checks of the arithmetic-class gate (tests/precision_class.py), no GPU.

1. The oracle's operand rounding IS the 16-bit cast: matmul_operand_bits(7) equals `.to(bfloat16)` bit for bit over magnitudes,
   both signs and exact ties; 10 bits equals `.to(float16)` inside fp16's normal range.
2. The gate has teeth on exactly the inputs the GPU tests use (forward at 96 cells, training gradients at 48 cells): simulated
   kernels that keep 7 or 8 mantissa bits pass; one that loses a bit (6) and one that truncates its 7-bit pack instead of
   rounding fail - which the flat 3e-2 they replace accepted (recorded rel-L2 of the forward: 5.6e-3 / 1.1e-2 / 2.1e-2 for
   7-bit RNE / 6-bit / 7-bit truncation; gradients worst tensor 1.0e-2 / 2.0e-2 / 5.7e-2).
"""
import numpy as np
import pytest
import torch

import oracle.dit as od
from oracle.dit import DiTConfig, dit_forward, matmul_operand_bits, round_operand
from oracle.weights import make_state_dict
from precision_class import (CLASS_FACTOR, TRAIN_VOCAB, class_error, class_gate, distances, exact_result, forward_case, oracle_grads,
                             train_case)
from test_oracle_dit import setup


def _magnitudes(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g) * torch.exp2(torch.randint(-100, 100, (n,), generator=g).float())


def _ties(drop):
    """fp32 values exactly half-way between two neighbours of the shortened format, low kept bit even and odd, many exponents."""
    g = torch.Generator().manual_seed(3)
    keep = torch.randint(0, 1 << (23 - drop), (4096,), generator=g, dtype=torch.int32)
    expo = torch.randint(113, 140, (4096,), generator=g, dtype=torch.int32)            # 2^-14 .. 2^12: normal in fp16 too
    sign = torch.randint(0, 2, (4096,), generator=g, dtype=torch.int32)
    bits = (sign << 31) | (expo << 23) | (keep << drop) | (1 << (drop - 1))
    return bits.view(torch.float32)


def test_seven_bit_rounding_is_the_bfloat16_cast_bit_for_bit():
    x = torch.cat([_magnitudes(1 << 20, 1), -_magnitudes(1 << 18, 2), _ties(16), torch.tensor([0.0, -0.0, 1.0, -1.0])])
    assert torch.isfinite(x).all()
    with matmul_operand_bits(7):
        r = round_operand(x)
    assert torch.equal(r.view(torch.int32), x.to(torch.bfloat16).float().view(torch.int32))
    t = _ties(16)
    with matmul_operand_bits(7):
        rt = round_operand(t)
    assert bool((rt != t).all()) and bool(((rt.view(torch.int32) >> 16) & 1 == 0).all())     # ties moved, to the even neighbour


def test_ten_bit_rounding_is_the_float16_cast_in_its_normal_range():
    g = torch.Generator().manual_seed(4)
    n = 1 << 20
    x = (torch.rand(n, generator=g) + 1.0) * torch.exp2(torch.randint(-14, 15, (n,), generator=g).float())     # [2^-14, 2^15)
    x = torch.cat([x * (torch.randint(0, 2, (n,), generator=g).float() * 2 - 1), _ties(13)])
    x = x[x.abs() < 65000.0]
    with matmul_operand_bits(10):
        r = round_operand(x)
    assert torch.equal(r.view(torch.int32), x.to(torch.float16).float().view(torch.int32))


def _truncating(monkeypatch):
    """A pack that drops the low bits instead of rounding to nearest-even: what `(uint16_t)(bits >> 16)` does."""
    def trunc(x):
        if od._OPERAND_BITS is None:
            return x
        drop = 23 - od._OPERAND_BITS
        return (x.contiguous().view(torch.int32) & ~((1 << drop) - 1)).view(torch.float32)
    monkeypatch.setattr(od, "round_operand", trunc)


def _truncating_activations_only(monkeypatch):
    """The narrower defect a fused kernel can really have: its ACTIVATION pack truncates while the weight stream (packed once, by
    another kernel) is rounded to nearest-even.  Linears: activation truncated, weight RNE; the attention products: both operands
    are activations."""
    rne = od.round_operand

    def trunc(x):
        return (x.contiguous().view(torch.int32) & ~((1 << (23 - od._OPERAND_BITS)) - 1)).view(torch.float32)

    def linear(x, w, b=None):
        y = (trunc(x) if od._OPERAND_BITS is not None else x) @ rne(w).transpose(-1, -2)
        return y if b is None else y + b
    monkeypatch.setattr(od, "linear", linear)
    monkeypatch.setattr(od, "round_operand", lambda x: x if od._OPERAND_BITS is None else trunc(x))


def test_gate_on_simulated_forward_defects(monkeypatch):
    """The 96-cell forward of test_bf16_vs_oracle_medium_batch (dit_base weights, seed 5)."""
    g, cfg, sd = setup("dit_base")
    x, t, lab = (torch.from_numpy(a) for a in forward_case(96, 5))
    fn = lambda: dit_forward(sd, cfg, x, t, {"clusters": lab})
    exact = exact_result(fn, "cpu/fwd96")
    cls = class_error(fn, 7, exact, tag="cpu/fwd96")["rel_l2"]
    assert 3e-3 < cls < 9e-3                                   # recorded 5.59e-3: the inputs leave the class where it was measured
    assert class_error(fn, 7, exact, tag="cpu/fwd96")["rel_l2"] == cls          # (the session cache)
    cells = class_error(fn, 7, exact, per="cell", tag="cpu/fwd96")
    assert len(cells) == 96 and max(cells) < 3 * cls
    class_gate(cls, cls, "simulated 7-bit RNE forward")
    class_gate(class_error(fn, 8, exact)["rel_l2"], cls, "simulated 8-bit forward")
    e6 = class_error(fn, 6, exact)["rel_l2"]
    with pytest.raises(AssertionError):
        class_gate(e6, cls, "simulated 6-bit forward (one mantissa bit lost)")
    _truncating(monkeypatch)
    et = class_error(fn, 7, exact)["rel_l2"]
    with pytest.raises(AssertionError):
        class_gate(et, cls, "simulated truncating 7-bit forward")
    assert e6 < 3e-2 and et < 3e-2                             # both were inside the flat bound the class gate stands beside
    assert e6 > 1.7 * cls and et > 3.0 * cls
    # Truncation of the activations alone (weights still rounded) is a smaller defect; here, where it also hits the conditioning
    # path (timestep embedder, adaLN projection), it reads 2.3 x.  In the fused kernels that path is split-bf16 and has no such pack: a
    # library built with a truncating OpBF16 pack measured 1.16-1.50 on the single-forward GPU tests (inside the gate, narrowly),
    # 1.45-1.68 over 50-200 evaluations, where its bias accumulates, and 1.6-2.2 on the fused-route gradients; the clean kernels read
    # 0.82-1.01.  Printed, and placed between the clean class and the both-operand truncation; the factor is not moved to catch more.
    monkeypatch.undo()
    _truncating_activations_only(monkeypatch)
    ea = class_error(fn, 7, exact)["rel_l2"]
    print(f"[parity] simulated truncating ACTIVATION pack, weights RNE: {ea:.3e} (ratio {ea / cls:.2f}; gate {CLASS_FACTOR})")
    assert 1.1 * cls < ea < et


def test_gate_on_simulated_training_gradient_defects(monkeypatch):
    """The 48-cell training step of test_bf16_training_gradients_close_to_fp32_oracle (joint vocabulary, 8 layers, seed 81)."""
    from scldm_amd.nnets import DiT
    m = DiT(n_embed=256, n_embed_input=16, n_layer=8, n_head=8, seq_len=16, class_vocab_sizes=TRAIN_VOCAB, condition_strategy="joint",
            dropout=0.0, bias=True, norm_layer="layernorm", multiple_of=4, layernorm_eps=1e-8, cfg_dropout_prob=0.8)
    sd = make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, 81)
    cfg = DiTConfig(n_layer=8, class_vocab_sizes=TRAIN_VOCAB, condition_strategy="joint")
    x1, x0, t, cond = train_case(48)
    fn = lambda: oracle_grads(sd, cfg, x1, x0, t, cond)
    exact = fn()
    cls = class_error(fn, 7, exact, per="tensor")
    assert set(cls) == set(exact) and len(cls) == 85               # pred + 84 trainable tensors
    assert 5e-3 < max(cls.values()) < 1.6e-2                   # recorded worst tensor 1.03e-2
    class_gate(cls, cls, "simulated 7-bit RNE training step")
    class_gate(class_error(fn, 8, exact, per="tensor"), cls, "simulated 8-bit training step")
    e6 = class_error(fn, 6, exact, per="tensor")
    with pytest.raises(AssertionError):
        class_gate(e6, cls, "simulated 6-bit training step")
    n6 = sum(e6[k] > CLASS_FACTOR * cls[k] for k in cls)
    _truncating(monkeypatch)
    et = class_error(fn, 7, exact, per="tensor")
    with pytest.raises(AssertionError):
        class_gate(et, cls, "simulated truncating 7-bit training step")
    nt = sum(et[k] > CLASS_FACTOR * cls[k] for k in cls)
    print(f"tensors outside the gate: 6-bit {n6} / {len(cls)}, truncating {nt} / {len(cls)}; 6-bit worst {max(e6.values()):.2e}")
    assert n6 >= 1 and nt >= 1
    assert max(e6.values()) < 3e-2                             # the one-bit loss passed every flat gradient gate


def test_distances_and_gate_bookkeeping():
    a = torch.arange(24.0).reshape(2, 3, 4) + 1
    b = a.clone()
    b[1] *= 1.01
    rec = distances(b, a)
    assert rec["per_cell"][0] == 0.0 and abs(rec["per_cell"][1] - 0.01) < 1e-6 and 0 < rec["rel_l2"] < 0.01
    assert abs(rec["max_abs_rel"] - 0.01) < 1e-6
    assert distances({"w": b, "extra": b}, {"w": a}) == {"w": rec["rel_l2"]}
    assert class_gate(1.5, 1.0, "edge of the gate") == 1.5
    with pytest.raises(AssertionError):
        class_gate(1.5001, 1.0, "just outside")
    with pytest.raises(AssertionError):
        class_gate({"w": 1.0, "v": 3.1}, {"w": 1.0, "v": 2.0}, "one tensor outside")
    assert class_gate({"w": 1.0, "b": 9e-5}, {"w": 1.0, "b": 0.0}, "a tensor no matmul feeds: the fp32 gate") == 1.0
    with pytest.raises(AssertionError):
        class_gate({"w": 1.0, "b": 2e-4}, {"w": 1.0, "b": 0.0}, "a tensor no matmul feeds, outside the fp32 gate")
    assert np.isclose(class_gate({"w": 1.0, "v": 2.9}, {"w": 1.0, "v": 2.0}, "all inside", bits=10), 1.45)

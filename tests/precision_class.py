"""Arithmetic-class gates for the reduced-precision paths.  TEST INFRASTRUCTURE ONLY (a helper module the tests import).

A 16-bit product path is held to the error of the ORACLE run in the same arithmetic class, not to a flat number:
`oracle.dit.matmul_operand_bits(b)` rounds both operands of every matmul (forward and, under autograd, both backward products)
to b explicit mantissa bits, round-to-nearest-even, and accumulates exact products in fp32 - b = 7 is bf16 (bit for bit the
`bfloat16` cast, tests/test_precision_class_cpu.py), b = 10 is fp16 / TF32.  The gate is

    rel-L2(kernel, exact)  <=  CLASS_FACTOR x rel-L2(b-bit-operand oracle, exact)        on the same inputs,

per tensor for gradients, over the whole batch for forwards and samplers.  Relative L2 and not max-abs: on the 96-cell forward the
7-bit oracle's rel-L2 moves by 2 % between seeds, its max-abs by 60 %.  One lost mantissa bit doubles the left side and truncation
instead of rounding quadruples it, so both land outside 1.5 x (tests/test_precision_class_cpu.py shows it on the inputs of the GPU
tests); the kernels' own extra roundings (activations stored in 16 bits between fused GEMMs) have to fit in the remaining 50 %.
"""
from __future__ import annotations

import numpy as np
import torch

from oracle.dit import matmul_operand_bits

# The project's TF32_FACTOR and the 1.5 of test_gpu_vae._tf32_gate, same derivation: the product path must be in the arithmetic
# class of the operand-rounded oracle.  Not a tuning knob.
CLASS_FACTOR = 1.5
CLASS_NAME = {7: "bf16", 10: "fp16"}
ORACLE_NAME = {7: "bf16-operand", 10: "TF32-operand"}
# A tensor that no matmul feeds (the gradient of the last bias under a loss that is linear in the output: a plain sum of the loss
# weights) is EXACT in the operand-rounded oracle - its class error is 0 and says nothing.  Such a tensor is held to the project's
# fp32 parity gate instead (1e-4, BASELINE.json north_star: what the fp32 route is held to on the same tensor).
EXACT_TOL = 1e-4
MAX_THREADS = 16     # the cap the CPU oracle chains of the GPU tests run under (an all-cores OpenMP team is pathological there)

_CACHE: dict = {}


def rel_l2(a, b) -> float:
    a = torch.as_tensor(a).detach().cpu().double()
    b = torch.as_tensor(b).detach().cpu().double()
    return float((a - b).norm() / b.norm())


def distances(got, exact) -> dict:
    """Distance record of a result to the exact one.  A dict of tensors (gradients): {name: rel-L2} over the names of `exact`
    that `got` has.  A tensor: {"rel_l2", "max_abs_rel", "per_cell"} - per_cell is the rel-L2 of every index of the first axis."""
    if isinstance(exact, dict):
        return {k: rel_l2(got[k], v) for k, v in exact.items() if k in got and got[k] is not None}
    a = torch.as_tensor(np.asarray(got) if isinstance(got, np.ndarray) else got).detach().cpu().double()
    b = torch.as_tensor(exact).detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    d = a - b
    rec = {"rel_l2": float(d.norm() / b.norm()), "max_abs_rel": float(d.abs().max() / b.abs().max())}
    if b.dim() >= 2:
        rec["per_cell"] = (d.flatten(1).norm(dim=1) / b.flatten(1).norm(dim=1).clamp_min(1e-300)).tolist()
    return rec


def _capped(fn):
    n_thr = torch.get_num_threads()
    torch.set_num_threads(min(MAX_THREADS, n_thr))
    try:
        return fn()
    finally:
        torch.set_num_threads(n_thr)


def exact_result(fn, tag: str):
    """fn() in exact arithmetic under the thread cap, once per session per tag (small results only: it is kept)."""
    key = (tag, None)
    if key not in _CACHE:
        with matmul_operand_bits(None):
            _CACHE[key] = _capped(fn)
    return _CACHE[key]


def class_error(fn, bits: int, exact, per: str | None = None, tag: str | None = None):
    """Distance of the `bits`-bit-operand oracle to `exact`: fn() (a CPU oracle chain) under matmul_operand_bits(bits).

    per=None      -> the record of `distances` ({"rel_l2", "max_abs_rel", "per_cell"} for a tensor, {name: rel-L2} for a dict)
    per="tensor"  -> {name: rel-L2} (fn returns a dict of gradients)
    per="cell"    -> [rel-L2 of each cell of the batch]
    With a `tag`, the record is kept for the session under (tag, bits): tests that share inputs run each chain once.  Only the
    distances are kept, never fn's result (the gradients of a 24-layer model are gigabytes)."""
    key = (tag, bits)
    rec = _CACHE.get(key) if tag is not None else None
    if rec is None:
        with matmul_operand_bits(bits):
            out = _capped(fn)
        rec = distances(out, exact)
        del out
        if tag is not None:
            _CACHE[key] = rec
    if per == "tensor":
        assert "per_cell" not in rec and "rel_l2" not in rec, "per='tensor' needs a dict of tensors"
        return rec
    if per == "cell":
        return rec["per_cell"]
    return rec


def class_gate(err, err_class, what: str, factor: float = CLASS_FACTOR, bits: int = 7, note: str = ""):
    """The class assertion: err <= factor x err_class, printed in the style of the fp16 lines.  Floats, or two {name: rel-L2} dicts
    (every tensor is gated; the line shows the worst ratio and the worst error).  Returns the (worst) ratio."""
    cls, orc = CLASS_NAME[bits], ORACLE_NAME[bits]
    if isinstance(err, dict):
        assert set(err) <= set(err_class) and err, (sorted(set(err) - set(err_class)), what)
        exact = {k: err[k] for k in err if err_class[k] == 0.0}        # no matmul feeds these: the fp32 gate (EXACT_TOL)
        for k, e in exact.items():
            print(f"[parity] {what} [{cls}] {k}: exact in the {orc} oracle (no matmul feeds it); kernel rel-L2 {e:.3e}, fp32 gate {EXACT_TOL:g}")
            assert e <= EXACT_TOL, (what, k, e)
        err = {k: v for k, v in err.items() if k not in exact}
        ratios = {k: err[k] / err_class[k] for k in err}
        k_r, k_e = max(ratios, key=ratios.get), max(err, key=err.get)
        print(f"[parity] {what} [{cls}] {len(err)} tensors rel-L2: worst kernel {err[k_e]:.3e} ({k_e}); {orc} oracle worst "
              f"{max(err_class[k] for k in err):.3e}; (ratio worst {ratios[k_r]:.2f} on {k_r}, median "
              f"{float(np.median(list(ratios.values()))):.2f}; gate {factor:g}){note}")
        bad = {k: (err[k], err_class[k]) for k in err if not err[k] <= factor * err_class[k]}
        assert not bad, (what, bad)
        return ratios[k_r]
    assert err_class > 0.0, (what, "the operand-rounded oracle is exact here: nothing to gate against")
    ratio = err / err_class
    print(f"[parity] {what} [{cls}] rel-L2: kernel {err:.3e}; {orc} oracle vs the same exact result: {err_class:.3e} "
          f"(ratio {ratio:.2f}; gate {factor:g}){note}")
    assert err <= factor * err_class, (what, err, err_class)
    return ratio


def gate_tensor(got, exact, fn, bits: int, what: str, tag: str | None = None):
    """Whole-batch class gate of one forward / sampler result, worst cell printed beside it.  Returns the kernel's record."""
    rec = distances(got, exact)
    cls = class_error(fn, bits, exact, tag=tag)
    note = ""
    if "per_cell" in rec:
        i = int(np.argmax(rec["per_cell"]))
        note = f"   worst cell {i}: kernel {rec['per_cell'][i]:.3e}, oracle's worst cell {max(cls['per_cell']):.3e}"
    class_gate(rec["rel_l2"], cls["rel_l2"], what, bits=bits, note=note)
    return rec


# ---- the two input sets the CPU mutation tests share with the GPU tests ------------------------------------------------------------
def forward_case(n: int = 96, seed: int = 5):
    """The medium-batch forward of tests/test_gpu_dit.py: n cells, dentate labels, numpy stream `seed`."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, 16, 16)).astype(np.float32)
    t = rng.uniform(0, 1, n).astype(np.float32)
    lab = rng.integers(0, 14, n).astype(np.int64)
    return x, t, lab


TRAIN_VOCAB = {"cell_line": 4, "gene": 2024}


def train_case(n: int, seed: int = 9, vocab: dict = TRAIN_VOCAB):
    """The training-step inputs of tests/test_gpu_train.py (_bf16_step_vs_oracle and the fp16 class test): x1, x0, t, labels
    (null tokens included)."""
    gen = torch.Generator().manual_seed(seed)
    x1, x0 = torch.randn(n, 16, 16, generator=gen), torch.randn(n, 16, 16, generator=gen)
    t = torch.rand(n, generator=gen)
    cond = {k: torch.randint(0, v + 1, (n,), generator=gen) for k, v in vocab.items()}
    return x1, x0, t, cond


def oracle_grads(sd, cfg, x1, x0, t, cond) -> dict:
    """{"pred": prediction, name: gradient} of the flow-matching step through the oracle (under whatever operand rounding is active)."""
    from oracle.train import training_grads
    _, pred, grads, _ = training_grads(sd, cfg, x1, x0, t, cond)
    return {"pred": pred, **grads}

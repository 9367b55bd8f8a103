"""ScviVAE's fp16-operand inference path (F16Operands of csrc/scvi_tile.hpp, scldm_scvi_*_ex) on the MI355X, held to the arithmetic class of the
reference: per tensor, rel-L2(kernel, exact) <= 1.5 x rel-L2(10-bit-operand helper, exact), exact being the helper
(tests/scvi_class_ref.py) with no rounding - precision_class.class_gate, whose CLASS_FACTOR is not a tuning knob.  Also: the fp32
route behind the new entries is bit-equal to the old one, run-to-run and batch-composition bit-equality, graph capture, the
saturation of an out-of-range weight, and the refusals."""
import ctypes as C
import functools

import pytest
import torch

import scvi_class_ref as ref
from conftest import load_golden
from oracle.dit import matmul_operand_bits
from precision_class import class_gate, rel_l2
from scvi_ref import CASES, OUTPUTS, build_scvi

pytestmark = pytest.mark.gpu
ENC, DEC = ("h", "loc", "scale", "z"), ("mu", "theta")


def model(name, sd, fp16=True):
    n_genes, n_hidden, n_latent, n_layers, B, shared, seed = ref.case_dims(name)
    vae = build_scvi(n_genes, n_hidden, n_latent, n_layers, shared)
    vae.load_state_dict(sd, strict=True)
    vae = vae.cuda().eval()
    if fp16:
        vae.fp16_enabled = True
        vae.precision = "fp16"
    return vae


def class_pair(fn):
    """(exact, {name: rel-L2 of the 10-bit-operand chain against exact}) of a helper chain returning a dict."""
    with matmul_operand_bits(None):
        exact = fn()
    with matmul_operand_bits(10):
        cls = {k: rel_l2(v, exact[k]) for k, v in fn().items()}
    return exact, cls


@functools.lru_cache(maxsize=None)
def case(name):
    """(state dict, CPU inputs, device inputs, fp16 model, exact forward, class error per tensor): built once per case, never modified."""
    sd, counts, lib, eps = ref.case_inputs(name)
    x = {"counts": counts, "library_size": lib, "eps": eps}
    exact, cls = class_pair(lambda: ref.forward(sd, counts, lib, eps))
    return sd, x, {k: v.cuda() for k, v in x.items()}, model(name, sd), exact, cls


def errors(got, exact, keys=OUTPUTS):
    return {k: rel_l2(got[k], exact[k]) for k in keys}


def run(vae, xd, rows=slice(None)):
    return vae.forward_outputs(xd["counts"][rows], xd["library_size"][rows], xd["eps"][rows])


@pytest.mark.parametrize("name", ref.ALL_CASES)
def test_forward_outputs_in_fp16_is_in_the_tf32_operand_class(name):
    sd, x, xd, vae, exact, cls = case(name)
    out = run(vae, xd)
    for k in OUTPUTS:
        assert out[k].shape == exact[k].shape and out[k].dtype == torch.float32 and bool(torch.isfinite(out[k]).all()), k
    err = errors(out, exact)
    class_gate(err, cls, f"{name}: fp16 forward_outputs", bits=10)
    # the operands really were rounded (the half-cast chain measures 0.99-1.00 x the class error of h): not the fp32 kernels
    print(f"[parity] {name}: fp16 h rel-L2 {err['h']:.3e} against the class error {cls['h']:.3e} (ratio {err['h'] / cls['h']:.2f}; floor 0.5)")
    assert err["h"] >= 0.5 * cls["h"], (err["h"], cls["h"])
    lik, post, z = vae(xd["counts"], None, xd["library_size"], eps=xd["eps"])           # forward wraps the same call
    assert torch.equal(lik.mu, out["mu"]) and torch.equal(lik.theta, out["theta"]) and torch.equal(post.loc, out["loc"])
    assert torch.equal(post.scale, out["scale"]) and torch.equal(z, out["z"])
    row = (out["mu"].double().sum(1).cpu() / x["library_size"].double() - 1).abs().max()
    assert float(row) < 1e-5, float(row)                                                 # the softmax stays fp32


@pytest.mark.parametrize("name", ref.ALL_CASES)
def test_encode_and_decode_alone_are_in_the_class(name):
    sd, x, xd, vae, exact, cls = case(name)
    h, loc, scale, z = vae.encode_hidden(xd["counts"], xd["eps"])
    class_gate(errors({"h": h, "loc": loc, "scale": scale, "z": z}, exact, ENC), {k: cls[k] for k in ENC}, f"{name}: fp16 encode_hidden", bits=10)
    post = vae.encode(xd["counts"])
    assert torch.equal(post.loc, loc) and torch.equal(post.scale, scale)
    # decode from the fixture's fp32 z (the case without a fixture: the helper's exact z)
    z32 = torch.from_numpy(load_golden(name)["z"]) if name in CASES else exact["z"]
    dexact, dcls = class_pair(lambda: dict(zip(DEC, ref.decode(sd, z32, x["library_size"]))))
    nb = vae.decode(z32.cuda(), None, xd["library_size"][:, None])
    class_gate(errors({"mu": nb.mu, "theta": nb.theta}, dexact, DEC), dcls, f"{name}: fp16 decode", bits=10)
    s = nb.sample(seed=11)                                                               # the fused negative-binomial draw
    assert s.shape == nb.mu.shape and bool((s >= 0).all()) and torch.equal(s, s.round()) and torch.equal(s, nb.sample(seed=11))


@pytest.mark.parametrize("name", ["scvi_small_unshared", "scvi_tiles"])
def test_the_fp32_route_is_untouched(name):
    from scldm_amd import _lib
    sd, x, xd, _, _, _ = case(name)
    plain = model(name, sd, fp16=False)                     # never saw the switch
    want = run(plain, xd)
    vae = model(name, sd)
    run(vae, xd)                                            # an fp16 call in between
    vae.precision = "fp32"
    got = run(vae, xd)
    for k in OUTPUTS:
        assert torch.equal(got[k], want[k]), k
    h2, loc2, scale2, z2 = vae.encode_hidden(xd["counts"], xd["eps"])
    nb = vae.decode(want["z"], None, xd["library_size"])
    assert torch.equal(h2, want["h"]) and torch.equal(z2, want["z"]) and torch.equal(nb.mu, want["mu"]) and torch.equal(nb.theta, want["theta"])
    # each _ex entry with SCLDM_PREC_FP32 against its plain entry, through ctypes
    L, h = plain._native()
    B = xd["counts"].shape[0]
    ws = plain._workspace(L, B)
    st = torch.cuda.current_stream().cuda_stream
    new = lambda: {k: torch.full_like(v, float("nan")) for k, v in want.items()}      # noqa: E731
    p = lambda t: t.data_ptr()      # noqa: E731
    c, lib, eps = xd["counts"], xd["library_size"], xd["eps"]
    a, b = new(), new()
    assert L.scldm_scvi_forward(h, p(c), p(lib), B, B, p(eps), p(a["h"]), p(a["loc"]), p(a["scale"]), p(a["z"]), p(a["mu"]), p(a["theta"]), ws, st) == 0
    assert L.scldm_scvi_forward_ex(h, p(c), p(lib), B, B, p(eps), p(b["h"]), p(b["loc"]), p(b["scale"]), p(b["z"]), p(b["mu"]), p(b["theta"]),
                                   _lib.PREC_FP32, ws, st) == 0
    for k in OUTPUTS:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], want[k]), f"forward_ex {k}"
    a, b = new(), new()
    assert L.scldm_scvi_encode(h, p(c), B, p(eps), p(a["h"]), p(a["loc"]), p(a["scale"]), p(a["z"]), ws, st) == 0
    assert L.scldm_scvi_encode_ex(h, p(c), B, p(eps), p(b["h"]), p(b["loc"]), p(b["scale"]), p(b["z"]), _lib.PREC_FP32, ws, st) == 0
    assert L.scldm_scvi_decode(h, p(want["z"]), p(lib), B, B, p(a["mu"]), p(a["theta"]), ws, st) == 0
    assert L.scldm_scvi_decode_ex(h, p(want["z"]), p(lib), B, B, p(b["mu"]), p(b["theta"]), _lib.PREC_FP32, ws, st) == 0
    for k in OUTPUTS:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], want[k]), f"encode_ex / decode_ex {k}"


@pytest.mark.parametrize("name", ["scvi_small", "scvi_tiles"])
def test_two_fp16_runs_and_split_batches_give_the_same_bits(name):
    sd, x, xd, vae, _, _ = case(name)
    B = CASES[name][4]
    a, b = run(vae, xd), run(vae, xd)
    for k in OUTPUTS:
        assert torch.equal(a[k], b[k]), f"{name} {k}: two runs differ"
    cut = 3 if B == 5 else 64            # [0, 3) + [3, 5); one full row tile + the tail
    lo, hi = run(vae, xd, slice(0, cut)), run(vae, xd, slice(cut, B))
    for k in OUTPUTS:
        if a[k].dim() == 1:              # shared theta (G): no batch axis
            assert torch.equal(lo[k], a[k]) and torch.equal(hi[k], a[k])
        else:
            assert torch.equal(torch.cat([lo[k], hi[k]]), a[k]), f"{name} {k}: a row's bits depend on the batch's other rows"


def test_fp16_forward_is_captured_into_a_graph_and_replays_to_the_same_bits():
    name = "scvi_tiles"
    sd, x, xd, vae, _, _ = case(name)
    eager = run(vae, xd)
    static = {k: v.clone() for k, v in xd.items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                         # warm-up on the capture stream (workspace, packed vectors)
        run(vae, static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run(vae, static)
    for v in out.values():
        v.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for k in OUTPUTS:
        assert torch.equal(out[k], eager[k]), f"graph replay: {k} differs from the eager call"


def test_a_weight_beyond_the_fp16_range_saturates_at_65504():
    """encoder_head.loc.weight[0, 0] = 1e6 is staged as 65 504: finite outputs, in the class of the helper run with 65 504 there.
    On scvi_small_unshared, where the latent this weight inflates stays inside the fp16 range (|z| <= 27 614 with the weight at
    65 504; on scvi_small and scvi_tiles it reaches 68 780 and 75 749, so the next layer's OPERAND would leave the range, which
    is another matter than the weight)."""
    name = "scvi_small_unshared"
    sd, x, xd, _, _, _ = case(name)
    key = "encoder_head.loc.weight"
    big, sat = dict(sd), dict(sd)
    big[key], sat[key] = sd[key].clone(), sd[key].clone()
    big[key][0, 0], sat[key][0, 0] = 1e6, 65504.0
    exact, cls = class_pair(lambda: ref.forward(sat, x["counts"], x["library_size"], x["eps"]))
    assert float(exact["z"].abs().max()) < 65504
    out = run(model(name, big), xd)
    for k in OUTPUTS:
        assert bool(torch.isfinite(out[k]).all()), k
    class_gate(errors(out, exact), cls, f"{name}: fp16 forward_outputs with a saturated weight", bits=10)


def test_refusals_and_an_intact_call_after_a_refused_one():
    from scldm_amd import _lib
    name = "scvi_small"
    sd, x, xd, vae, _, _ = case(name)
    plain = model(name, sd, fp16=False)
    with pytest.raises(NotImplementedError, match="fp32 only"):          # switch off
        plain.precision = "fp16"
    on = model(name, sd)
    with pytest.raises(NotImplementedError, match="bf16"):               # switch on: bf16 is still refused
        on.precision = "bf16"
    assert on.precision == "fp16"
    on.train_enabled = True
    on.train()
    with pytest.raises(NotImplementedError, match="fp32 only"):
        on(xd["counts"], None, xd["library_size"], eps=xd["eps"])
    on.eval()
    want = run(vae, xd)
    L, h = on._native()
    B = xd["counts"].shape[0]
    ws = on._workspace(L, B)
    st = torch.cuda.current_stream().cuda_stream
    out = {k: torch.full_like(v, -1.0) for k, v in want.items()}
    p = lambda t: t.data_ptr()      # noqa: E731
    args = (h, p(xd["counts"]), p(xd["library_size"]), B, B, p(xd["eps"]), p(out["h"]), p(out["loc"]), p(out["scale"]), p(out["z"]),
            p(out["mu"]), p(out["theta"]))
    assert L.scldm_scvi_forward_ex(*args, _lib.PREC_BF16, ws, st) == -1 and "precision" in L.scldm_last_error().decode()
    assert L.scldm_scvi_encode_ex(h, p(xd["counts"]), B, None, p(out["h"]), p(out["loc"]), p(out["scale"]), None, _lib.PREC_BF16, ws, st) == -1
    assert L.scldm_scvi_decode_ex(h, p(want["z"]), p(xd["library_size"]), B, B, p(out["mu"]), p(out["theta"]), _lib.PREC_BF16X3, ws, st) == -1
    torch.cuda.synchronize()
    for k in OUTPUTS:
        assert bool((out[k] == -1.0).all()), f"a refused call wrote {k}"
    assert L.scldm_scvi_forward_ex(*args, _lib.PREC_FP16, ws, st) == 0      # the next valid call is intact
    for k in OUTPUTS:
        assert torch.equal(out[k], want[k]), k

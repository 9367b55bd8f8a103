"""ScviVAE training on fp16 operands on the MI355X (scldm_scvi_train_forward_ex / _backward_ex behind ScviVAE.forward with
`train_enabled`, `fp16_enabled`, `train_fp16_enabled` and precision "fp16"), held to the arithmetic class the reference trains in:
per tensor, rel-L2(kernel, exact) <= 1.5 x rel-L2(10-bit-operand helper, exact), the helper being tests/scvi_train_class_ref.py
(autograd over oracle.dit.linear: forward product and both backward products rounded) and exact the same helper without rounding -
precision_class.class_gate, whose CLASS_FACTOR is not a tuning knob.  Also: exact covariance under a power-of-two scale of the
upstream gradients (the per-tensor operand scale), the overflow flag, the fp32 route bit-equal behind the new switch and the new
entries, bit-equal repeats, the eval path after an fp16 step, and the refusals."""
import copy
import ctypes as C
import functools

import pytest
import torch

import scvi_class_ref
import scvi_train_class_ref as ref
from oracle.dit import matmul_operand_bits
from precision_class import class_error, class_gate, exact_result, rel_l2
from scvi_ref import build_scvi
from scvi_train_ref import pre_bn_biases

pytestmark = pytest.mark.gpu
FIRST = "grad:encoder.encoder_mlp.0.weight"


@functools.lru_cache(maxsize=None)
def device_inputs(name):
    sd, counts, lib, eps, masks, p = ref.case(name)
    x = {"counts": counts.cuda(), "library_size": lib.cuda(), "eps": eps.cuda()}
    return x, ([torch.from_numpy(m).cuda() for m in masks] if masks else None)


def fresh_model(name, precision="fp16", switches=True, dropout=None):
    n_genes, n_hidden, n_latent, n_layers, B, shared, p, seed = ref.ALL_TRAIN_CASES[name]
    vae = build_scvi(n_genes, n_hidden, n_latent, n_layers, shared, dropout=p if dropout is None else dropout)
    vae.load_state_dict(ref.case(name)[0], strict=True)
    vae = vae.cuda().train()
    if switches:
        vae.train_enabled = vae.fp16_enabled = vae.train_fp16_enabled = True
        vae.precision = precision
    return vae


def params_of(vae):
    return {k: p for k, p in vae.named_parameters() if p.requires_grad}


def step(vae, x, masks=None, seed=None, upstream=None):
    """One training step on the device: (outputs, {key: gradient}, {key: running statistic}).  upstream=None: the ELBO's gradient."""
    from scldm_amd.training import scvi_loss
    for p in vae.parameters():
        p.grad = None
    lik, post, z = vae(x["counts"], None, x["library_size"][:, None], eps=x["eps"], dropout_masks=masks, seed=seed)
    out = {"loc": post.loc, "scale": post.scale, "z": z, "mu": lik.mu, "theta": lik.theta}
    named = params_of(vae)
    if upstream is None:
        got = torch.autograd.grad(sum(scvi_loss(vae, x["counts"], lik, post, z).values()), list(named.values()), allow_unused=True)
    else:
        got = torch.autograd.grad([out[k] for k in ref.OUTPUTS], list(named.values()), grad_outputs=[upstream[k] for k in ref.OUTPUTS],
                                  allow_unused=True)
    grads = dict(zip(named, got))
    assert all(g is not None for g in grads.values())
    stats = {k: v.clone() for k, v in vae.state_dict().items() if "running_" in k}
    return {k: v.detach() for k, v in out.items()}, grads, stats


def oracle(name):
    """(exact step, class error per tensor) of the ELBO step of a case on the CPU: computed once per session, under the thread cap."""
    sd, counts, lib, eps, masks, p = ref.case(name)
    fn = lambda: ref.flat(*ref.step(sd, counts, lib, eps, masks, p), sd)      # noqa: E731
    exact = exact_result(fn, "scvi_train_fp16:" + name)
    return exact, class_error(fn, 10, exact, per="tensor", tag="scvi_train_fp16:" + name)


def assert_same_bits(a, b, what):
    for da, db in zip(a, b):
        assert set(da) == set(db)
        for k in da:
            assert torch.equal(da[k], db[k]), f"{what}: {k}"


@pytest.mark.parametrize("name", sorted(ref.ALL_TRAIN_CASES))
def test_fp16_training_step_is_in_the_tf32_operand_class(name):
    sd = ref.case(name)[0]
    x, masks = device_inputs(name)
    exact, cls = oracle(name)
    vae = fresh_model(name)
    out, grads, stats = step(vae, x, masks)
    zero = pre_bn_biases(sd)
    n_layers = ref.ALL_TRAIN_CASES[name][3]
    assert len(zero) == 2 * n_layers and len(stats) == 4 * n_layers
    for k in zero:
        assert torch.count_nonzero(grads[k]) == 0, k          # exact zeros, not None and not roundoff
    got = ref.flat(out, stats, grads, sd)
    assert set(got) == set(exact)
    for k, v in got.items():
        assert v.shape == exact[k].shape and v.dtype == torch.float32 and bool(torch.isfinite(v).all()), k
    err = {k: rel_l2(got[k], exact[k]) for k in exact}
    for kind in ("out:", "stat:", "grad:"):
        class_gate({k: e for k, e in err.items() if k.startswith(kind)}, cls, f"{name}: fp16 training step, {kind[:-1]}", bits=10)
    # the operands really were rounded: not the fp32 kernels behind the fp16 switch
    print(f"[parity] {name}: fp16 {FIRST} rel-L2 {err[FIRST]:.3e} against the class error {cls[FIRST]:.3e} "
          f"(ratio {err[FIRST] / cls[FIRST]:.2f}; floor 0.5)")
    assert err[FIRST] >= 0.5 * cls[FIRST], (err[FIRST], cls[FIRST])
    tracked = {int(v) for k, v in vae.state_dict().items() if k.endswith("num_batches_tracked")}
    assert len(tracked) == 1
    row = (out["mu"].double().sum(1) / x["library_size"].double() - 1).abs().max()
    assert float(row) < 1e-5, float(row)                       # the softmax stays fp32


@pytest.mark.parametrize("name", ["scvi_train_rows", "scvi_train_tiles"])
def test_parameter_gradients_are_covariant_under_a_power_of_two_upstream_scale(name):
    """Upstream gradients g and 2^-20 g: every parameter gradient of the second is bit-equal to 2^-20 times that of the first.  The
    fp32 stages are covariant under powers of two and every operand scale moves by exactly 20, so the staged fp16 operands are the
    same bits; an operand cast without its scale loses most of 2^-20 g to fp16's exponent range."""
    x, masks = device_inputs(name)
    up = {k: v.cuda() for k, v in ref.upstream_grads(name).items()}
    small = {k: v * 2.0 ** -20 for k, v in up.items()}
    _, g1, _ = step(fresh_model(name), x, masks, upstream=up)
    _, g2, _ = step(fresh_model(name), x, masks, upstream=small)
    moved = 0
    for k in g1:
        assert torch.equal(g2[k], g1[k] * 2.0 ** -20), k
        moved += int(torch.count_nonzero(g1[k]) > 0)
    assert moved >= len(g1) - len(pre_bn_biases(ref.case(name)[0]))


def test_overflow_flag_is_set_by_a_non_finite_upstream_gradient_and_reset_by_the_next_backward():
    name = "scvi_train_rows"
    x, masks = device_inputs(name)
    up = {k: v.cuda() for k, v in ref.upstream_grads(name).items()}
    bad = dict(up)
    bad["mu"] = up["mu"].clone()
    bad["mu"][3, 17] = float("inf")
    vae = fresh_model(name)
    flag = vae.found_inf_flag()
    assert flag.shape == () and flag.dtype == torch.float32 and flag.is_cuda and flag is vae.found_inf_flag() and float(flag) == 0.0
    step(vae, x, masks, upstream=bad)
    assert float(flag) == 1.0
    _, grads, _ = step(vae, x, masks, upstream=up)
    assert float(flag) == 0.0 and all(bool(torch.isfinite(g).all()) for g in grads.values())
    # a copy registers a flag of its own with its own handle
    twin = copy.deepcopy(vae)
    assert "_found_inf" not in twin.__dict__
    flag2 = twin.found_inf_flag()
    assert flag2 is not flag
    step(twin, x, masks, upstream=bad)
    assert float(flag2) == 1.0 and float(flag) == 0.0
    # the fp32 backward never touches it
    twin.precision = "fp32"
    step(twin, x, masks, upstream=up)
    assert float(flag2) == 1.0


# ---- the C entries through ctypes --------------------------------------------------------------------------------------------------
def raw_forward(vae, x, masks, prec, ex, fill):
    """(rc, outputs, record) of scldm_scvi_train_forward (ex=False) / _forward_ex on buffers filled with `fill`."""
    L, h = vae._native()
    c, lib, eps = x["counts"], x["library_size"], x["eps"]
    B = c.shape[0]
    G, H, nl = vae._dims
    new = lambda *s: torch.full(s, fill, device="cuda", dtype=torch.float32)      # noqa: E731
    out = {"loc": new(B, nl), "scale": new(B, nl), "z": new(B, nl), "mu": new(B, G)}
    out["theta"] = new(G) if vae.decoder_head.shared_theta else new(B, G)
    record = torch.zeros(L.scldm_scvi_train_record_bytes(h, B), dtype=torch.uint8, device="cuda")
    n = len(vae.encoder.encoder_mlp) // 4 + len(vae.decoder.decoder_mlp) // 4
    mask_ptrs = (C.c_void_p * n)(*[m.data_ptr() for m in masks]) if masks else None
    args = (h, c.data_ptr(), lib.data_ptr(), B, B, eps.data_ptr(), float(vae.encoder.dropout), float(vae.decoder.dropout), C.c_uint64(0),
            mask_ptrs, 1, 0.1, record.data_ptr(), out["loc"].data_ptr(), out["scale"].data_ptr(), out["z"].data_ptr(), out["mu"].data_ptr(),
            out["theta"].data_ptr())
    ws, st = vae._train_workspace(L, B), torch.cuda.current_stream().cuda_stream
    rc = L.scldm_scvi_train_forward_ex(*args, prec, ws, st) if ex else L.scldm_scvi_train_forward(*args, ws, st)
    return rc, out, record


def raw_backward(vae, x, masks, out, record, up, prec, ex, fill):
    """(rc, {parameter key: gradient}) of scldm_scvi_train_backward (ex=False) / _backward_ex on gradients filled with `fill`."""
    from scldm_amd import _lib
    L, h = vae._native()
    c, lib, eps = x["counts"], x["library_size"], x["eps"]
    B = c.shape[0]
    params = vae._train_params()
    grads = [torch.full_like(p, fill) for p in params]
    it = iter(grads)
    n_enc, n_dec = len(vae.encoder.encoder_mlp) // 4, len(vae.decoder.decoder_mlp) // 4

    def layers(n):
        return (_lib.ScviLayerGrads * n)(*[_lib.ScviLayerGrads(*[next(it).data_ptr() for _ in range(4)]) for _ in range(n)])
    ea = layers(n_enc)
    head = [next(it).data_ptr() for _ in range(4)]
    da = layers(n_dec)
    shared = vae.decoder_head.shared_theta
    lik = [next(it).data_ptr() for _ in range(3 if shared else 4)] + ([None] if shared else [])
    g = _lib.ScviGrads(ea, da, *head, *lik)
    mask_ptrs = (C.c_void_p * (n_enc + n_dec))(*[m.data_ptr() for m in masks]) if masks else None
    args = (h, c.data_ptr(), lib.data_ptr(), B, B, eps.data_ptr(), float(vae.encoder.dropout), float(vae.decoder.dropout), mask_ptrs,
            record.data_ptr(), out["scale"].data_ptr(), out["z"].data_ptr(), out["mu"].data_ptr(), out["theta"].data_ptr(),
            *[up[k].data_ptr() for k in ("mu", "theta", "loc", "scale", "z")], C.byref(g))
    ws, st = vae._train_workspace(L, B), torch.cuda.current_stream().cuda_stream
    rc = L.scldm_scvi_train_backward_ex(*args, prec, ws, st) if ex else L.scldm_scvi_train_backward(*args, ws, st)
    by_id = {id(p): k for k, p in vae.named_parameters()}
    return rc, {by_id[id(p)]: t for p, t in zip(params, grads)}


@pytest.mark.parametrize("name", ["scvi_train_small_unshared", "scvi_train_tiles"])
def test_the_fp32_route_is_untouched(name):
    from scldm_amd import _lib
    sd = ref.case(name)[0]
    x, masks = device_inputs(name)
    plain = fresh_model(name, switches=False)               # never saw the new switches
    plain.train_enabled = True
    want = step(plain, x, masks)
    vae = fresh_model(name, precision="fp32")               # all three switches on, precision fp32
    assert_same_bits(step(vae, x, masks), want, "all switches on, fp32")
    vae = fresh_model(name)
    step(vae, x, masks)                                     # an fp16 step in between
    vae.load_state_dict(sd, strict=True)
    vae.precision = "fp32"
    assert_same_bits(step(vae, x, masks), want, "fp32 after an fp16 step")

    # each _ex entry with SCLDM_PREC_FP32 against its plain entry, from the same starting statistics
    up = {k: v.cuda() for k, v in ref.upstream_grads(name).items()}
    L = _lib.lib()
    runs = []
    for ex in (False, True):
        vae.load_state_dict(sd, strict=True)
        rc, out, record = raw_forward(vae, x, masks, _lib.PREC_FP32, ex, float("nan"))
        assert rc == 0, L.scldm_last_error().decode()
        rc, grads = raw_backward(vae, x, masks, out, record, up, _lib.PREC_FP32, ex, float("nan"))
        assert rc == 0, L.scldm_last_error().decode()
        runs.append((out, grads, {k: v.clone() for k, v in vae.state_dict().items() if "running_" in k}))
    assert_same_bits(runs[0], runs[1], "plain entries against _ex with SCLDM_PREC_FP32")
    assert all(bool(torch.isfinite(v).all()) for d in runs[0] for v in d.values())
    for k in ref.OUTPUTS:
        assert torch.equal(runs[0][0][k], want[0][k]), k      # and the module's forward is this call

    # a precision that is not built: -1, "precision", nothing written; the next valid call is intact
    vae.load_state_dict(sd, strict=True)
    before = {k: v.clone() for k, v in vae.state_dict().items() if "running_" in k}
    rc, out, _ = raw_forward(vae, x, masks, _lib.PREC_BF16, True, -1.0)
    assert rc == -1 and "precision" in L.scldm_last_error().decode()
    rc, grads = raw_backward(vae, x, masks, runs[1][0], record, up, _lib.PREC_BF16, True, -1.0)
    assert rc == -1 and "precision" in L.scldm_last_error().decode()
    torch.cuda.synchronize()
    for k, v in {**out, **grads}.items():
        assert bool((v == -1.0).all()), f"a refused call wrote {k}"
    for k, v in before.items():
        assert torch.equal(vae.state_dict()[k], v), f"a refused call moved {k}"
    rc, out, record = raw_forward(vae, x, masks, _lib.PREC_FP32, True, -1.0)
    assert rc == 0
    rc, grads = raw_backward(vae, x, masks, out, record, up, _lib.PREC_FP32, True, -1.0)
    assert rc == 0
    assert_same_bits((out, grads), runs[1][:2], "the call after a refused one")


@pytest.mark.parametrize("name", ["scvi_train_small_drop", "scvi_train_tiles"])
def test_two_fresh_fp16_modules_give_the_same_bits(name):
    x, masks = device_inputs(name)
    a, b = step(fresh_model(name), x, masks), step(fresh_model(name), x, masks)
    assert_same_bits(a, b, f"{name}: two fresh fp16 modules")


def test_masks_drawn_from_a_seed_replay_bit_for_bit_in_fp16():
    name = "scvi_train_small_drop"
    x, _ = device_inputs(name)

    def run(seed=None, masks=None):
        vae = fresh_model(name)
        res = step(vae, x, masks=masks, seed=seed)
        return res, [m.clone() for m in vae.last_dropout_masks]
    (a, ma), (b, mb), (c, mc) = run(seed=3), run(seed=3), run(seed=4)
    assert all(torch.equal(p, q) for p, q in zip(ma, mb)) and not all(torch.equal(p, q) for p, q in zip(ma, mc))
    assert_same_bits(a, b, "the same seed")
    assert_same_bits(a, run(masks=ma)[0], "the drawn masks, given back")
    assert not torch.equal(a[0]["mu"], c[0]["mu"])


def test_eval_after_an_fp16_step_uses_the_updated_running_statistics():
    name = "scvi_train_small_drop"
    sd, counts, lib, eps, _, _ = ref.case(name)
    x, masks = device_inputs(name)
    vae = fresh_model(name)
    vae.eval()
    before = vae.forward_outputs(x["counts"], x["library_size"], x["eps"])["mu"].clone()
    vae.train()
    step(vae, x, masks)
    vae.eval()
    got = vae.forward_outputs(x["counts"], x["library_size"], x["eps"])
    now = {k: v.detach().cpu() for k, v in vae.state_dict().items()}
    key = "encoder.encoder_mlp.1.running_mean"
    assert rel_l2(now[key], sd[key]) > 1e-2
    fn = lambda: scvi_class_ref.forward(now, counts, lib, eps)      # noqa: E731
    with matmul_operand_bits(None):
        exact = fn()
    with matmul_operand_bits(10):
        cls = {k: rel_l2(v, exact[k]) for k, v in fn().items()}
    class_gate({k: rel_l2(got[k], exact[k]) for k in exact}, cls, f"{name}: fp16 eval forward after an fp16 training step", bits=10)
    assert rel_l2(before, exact["mu"]) > 1e-3                  # the statistics matter to the result


def test_switch_off_keeps_the_old_refusal():
    name = "scvi_train_small"
    x, _ = device_inputs(name)
    vae = fresh_model(name)
    vae.train_fp16_enabled = False
    with pytest.raises(NotImplementedError, match=r"ScviVAE trains in exact fp32 only \(precision='fp16'\)"):
        vae(x["counts"], None, x["library_size"], eps=x["eps"])
    vae.train_fp16_enabled = True
    lik, post, z = vae(x["counts"], None, x["library_size"], eps=x["eps"])
    assert lik.mu.requires_grad and z.requires_grad
    vae.fp16_enabled = False                                   # the inference switch gates the setter as before
    with pytest.raises(NotImplementedError, match="fp32 only"):
        vae.precision = "fp16"

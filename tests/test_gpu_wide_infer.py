"""GPU parity of the record-free inference path of shapes outside the fused family (scldm_dit_infer_*): the trunk's bit identity with
scldm_dit_train_forward, forward_with_cfg and the fixed-grid sampler against the oracle, weight freshness, rejections and routing.

Shapes are the smallest that reach each route: 512 x 8 (head dim 64), 512 x 16 (head dim 32) and 1 024 x 16 (four 256-column quarters per
LayerNorm row), two layers each.  B in {1, 3, 6} cells give 3 / 9 / 18 sample-forwards under one joint pass = 48 tokens (below the
128-token threshold of the bf16-array route), 144 (on it) and 288 (past 256 tokens, where the 256-tile GEMM becomes eligible).
Gates: conftest.check_err at 1e-4 for fp32 / bf16x3, precision_class.gate_tensor (bf16-operand oracle x 1.5) for bf16."""
import ctypes as C

import pytest
import torch

from conftest import check_err
from oracle.dit import dit_forward_with_cfg
from oracle.transport import sample_ode_fixed
from precision_class import exact_result, gate_tensor
from test_gpu_train import build

pytestmark = pytest.mark.gpu
TOL_FP32 = 1e-4
VOCAB = {"cell_line": 4, "gene": 2024}
SHAPES = [(512, 8), (512, 16), (1024, 16)]
SCALES = {"joint": {"cell_line": 2.0, "gene": 1.0}, "mutually_exclusive": {"cell_line": 2.0, "gene": 0.5}}

_MODELS = {}


def model(n_embed, n_head, strategy="joint"):
    """One eval-mode model per (shape, strategy) for the session: (module, state dict, oracle config)."""
    key = (n_embed, n_head, strategy)
    if key not in _MODELS:
        m, sd, cfg = build(VOCAB, strategy, 2, 70 + n_head + n_embed // 256, n_embed=n_embed, n_head=n_head)
        _MODELS[key] = (m.eval(), sd, cfg)
    return _MODELS[key]


def cfg_case(B, seed, dup=True):
    """Doubled state, doubled labels and a stride-0 scalar t; with `dup` cells 0 and B - 1 share labels AND latents, and the labels
    come from three tuples only (the plan de-duplicates them into fewer rows than cells)."""
    gen = torch.Generator().manual_seed(seed)
    z = torch.randn(B, 16, 16, generator=gen)
    if dup:
        pool = {k: torch.randint(0, v, (3,), generator=gen) for k, v in VOCAB.items()}
        pick = torch.randint(0, 3, (B,), generator=gen)
        pick[-1] = pick[0]
        lab = {k: v[pick] for k, v in pool.items()}
        z[-1] = z[0]
    else:
        lab = {k: torch.randint(0, v, (B,), generator=gen) for k, v in VOCAB.items()}
    return torch.cat([z, z]), {k: torch.cat([v, v]) for k, v in lab.items()}


def cuda(d):
    return {k: v.cuda() for k, v in d.items()}


def gate(got, fn, prec, what, tag):
    """fp32 / bf16x3: check_err against the exact oracle; bf16: the class gate against the bf16-operand oracle."""
    exact = exact_result(fn, tag)
    if prec == "bf16":
        gate_tensor(got.cpu(), exact, fn, 7, what, tag=tag)
    else:
        check_err(got.cpu(), exact, TOL_FP32, f"{what} [{prec}]")


# ---- 1. trunk bit identity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 6])
@pytest.mark.parametrize("n_embed,n_head", SHAPES)
def test_trunk_has_the_bits_of_the_training_forward(n_embed, n_head, B):
    """One conditioning row per sample-forward, row_index NULL, the same n: scldm_dit_infer_cond_rows + scldm_dit_infer_forward_rows return
    the bits of scldm_dit_train_forward, in fp32 and in bf16.  The batch mixes real labels and the null token (index = vocabulary size)."""
    from scldm_amd import _lib
    m, _, _ = model(n_embed, n_head)
    n = 3 * B
    gen = torch.Generator().manual_seed(100 * n_head + n)
    x, t = torch.randn(n, 16, 16, generator=gen).cuda(), torch.rand(n, generator=gen).cuda()
    lab = {k: torch.randint(0, v + 1, (n,), generator=gen).cuda() for k, v in VOCAB.items()}
    ptrs = _lib.ptr_array([lab[c].data_ptr() for c in m._class_names])
    for prec in ("fp32", "bf16"):
        m.precision = prec
        ref = m._generic_forward(x, t, ptrs)          # scldm_dit_train_forward
        got = m._wide_forward(x, t, ptrs)             # scldm_dit_infer_cond_rows + scldm_dit_infer_forward_rows
        assert torch.isfinite(ref).all() and float(ref.abs().max()) > 0
        assert torch.equal(got, ref), (prec, float((got - ref).abs().max()))
    m.precision = "fp32"


# ---- 2. guided forward with de-duplicated labels ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_embed,n_head,strategy,B", [(512, 8, "joint", 1), (512, 8, "joint", 3), (512, 8, "joint", 6),
                                                       (512, 8, "mutually_exclusive", 6), (512, 16, "joint", 6),
                                                       (512, 16, "mutually_exclusive", 3), (1024, 16, "joint", 6),
                                                       (1024, 16, "mutually_exclusive", 6)])
def test_forward_with_cfg_over_deduplicated_rows_matches_oracle(n_embed, n_head, strategy, B):
    m, sd, cfg = model(n_embed, n_head, strategy)
    z2, c2 = cfg_case(B, 7 * B + n_head)
    scales = SCALES[strategy]
    t2 = torch.full((2 * B,), 0.4)
    fn = lambda: dit_forward_with_cfg(sd, cfg, z2, t2, c2, scales)
    t_dev = torch.full((1,), 0.4, device="cuda").expand(2 * B)      # stride 0: one scalar t
    # other labels for the guided half: the unconditional half must not move
    c_other = {k: (v + 1) % VOCAB[k] for k, v in c2.items()}
    for prec in ("fp32", "bf16x3", "bf16"):
        m.precision = prec
        out = m.forward_with_cfg(z2.cuda(), t_dev, cuda(c2), scales)
        gate(out, fn, prec, f"wide forward_with_cfg {n_embed}x{n_head} {strategy} B={B}", f"wide_cfg/{n_embed}/{n_head}/{strategy}/{B}")
        if B > 1:     # cells 0 and B - 1 have equal labels and latents
            assert torch.equal(out[0], out[B - 1]) and torch.equal(out[B], out[2 * B - 1])
        out2 = m.forward_with_cfg(z2.cuda(), t_dev, cuda(c_other), scales)
        assert torch.equal(out2[:B], out[:B]) and not torch.equal(out2[B:], out[B:])
        # a dense t of equal entries takes per-sample rows: same arithmetic class, and the same oracle
        out_d = m.forward_with_cfg(z2.cuda(), t2.cuda(), cuda(c2), scales)
        gate(out_d, fn, prec, f"wide forward_with_cfg {n_embed}x{n_head} {strategy} B={B} per-sample rows", f"wide_cfg/{n_embed}/{n_head}/{strategy}/{B}")
    m.precision = "fp32"


# ---- 3. sampler ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,num_steps", [("euler", 5), ("heun", 4)])
@pytest.mark.parametrize("n_head,strategy", [(8, "joint"), (16, "mutually_exclusive")])
def test_sampler_matches_the_oracle_chain_and_repeats(n_head, strategy, method, num_steps):
    B = 3
    m, sd, cfg = model(512, n_head, strategy)
    z2, c2 = cfg_case(B, 31 + n_head)
    scales = SCALES[strategy]
    fn = lambda: sample_ode_fixed(z2, lambda xx, tt: dit_forward_with_cfg(sd, cfg, xx, tt, c2, scales), num_steps, method)
    for prec in ("fp32", "bf16"):
        m.precision = prec
        out = m.sample_ode_cfg(z2.cuda(), cuda(c2), scales, num_steps, method)
        gate(out, fn, prec, f"wide sampler 512x{n_head} {strategy} {method} {num_steps} points", f"wide_ode/{n_head}/{strategy}/{method}")
        assert torch.equal(m.sample_ode_cfg(z2.cuda(), cuda(c2), scales, num_steps, method), out)
    m.precision = "fp32"


def test_sampler_forms_timestep_embeddings_in_chunks():
    """More evaluations than one pass of the timestep MLP covers (256): a 258-point Euler solve of one cell stays on the composed loop's
    result (both fp32 on the GPU; the two differ in the split-K choices of a few small GEMMs only)."""
    m, _, _ = model(512, 8)
    z2, c2 = cfg_case(1, 5, dup=False)
    out = m.sample_ode_cfg(z2.cuda(), cuda(c2), SCALES["joint"], 258, "euler")
    z, hstep = z2.cuda().clone(), 1.0 / 257
    for i in range(257):
        z = z + hstep * m._generic_forward_with_cfg(z, torch.full((2,), i * hstep, device="cuda"), cuda(c2), SCALES["joint"])
    check_err(out.cpu(), z.cpu(), TOL_FP32, "wide sampler, 257 Euler evaluations vs the composed loop")


# ---- 4. weight freshness ---------------------------------------------------------------------------------------------------------------------
def test_an_in_place_data_update_is_seen_by_the_next_call():
    """The entries read the live parameters (and re-cast the bf16 mirror once per call): a `.data` update, which no version counter
    shows, changes the next result - to what the oracle gives on the new state dict."""
    B = 3          # 9 sample-forwards = 144 tokens: the bf16 policy runs on the weight mirror
    m, sd, cfg = build(VOCAB, "joint", 2, 123, n_embed=512, n_head=8)
    m.eval()
    z2, c2 = cfg_case(B, 11)
    scales = SCALES["joint"]
    t_dev = torch.full((1,), 0.3, device="cuda").expand(2 * B)
    before = {}
    for prec in ("fp32", "bf16"):
        m.precision = prec
        before[prec] = m.forward_with_cfg(z2.cuda(), t_dev, cuda(c2), scales)
    w = m.blocks[1].mlp.c_proj.weight
    version = w._version
    w.data.mul_(1.5)
    assert w._version == version
    sd2 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    fn = lambda: dit_forward_with_cfg(sd2, cfg, z2, torch.full((2 * B,), 0.3), c2, scales)
    for prec in ("fp32", "bf16"):
        m.precision = prec
        after = m.forward_with_cfg(z2.cuda(), t_dev, cuda(c2), scales)
        assert not torch.equal(after, before[prec])
        gate(after, fn, prec, "wide forward_with_cfg after an in-place .data update", "wide_fresh")


# ---- 5. rejections ---------------------------------------------------------------------------------------------------------------------------
def test_rejections_return_err_shape_and_touch_nothing():
    from scldm_amd import _lib
    B = 2
    z2, c2 = cfg_case(B, 3, dup=False)

    def call(m, z, n_steps=3, method=0, null_z=False):
        m.precision = "fp32"
        ul, n_u, cell_row, n_pass, masks, scales, keep = m._cfg_plan(cuda(c2), SCALES["joint"], B, dedup=True)
        L, h = m._native_handle()
        w, _ = m._weights_struct(tuple(m.parameters()))
        ws = torch.zeros(max(L.scldm_dit_infer_workspace_bytes(h, 2 * B + n_pass * B, 1 + n_pass * n_u, 2 * B, 0), 1 << 20), dtype=torch.uint8, device="cuda")
        rc = L.scldm_dit_infer_sample_ode(h, C.byref(w), None if null_z else z.data_ptr(), C.cast(ul, _lib.c_void_pp), n_u, cell_row, B, n_pass, masks,
                                          scales, n_steps, method, 0, ws.data_ptr(), None)
        torch.cuda.synchronize()
        assert int(ws.count_nonzero()) == 0        # nothing was launched
        return rc, L.scldm_last_error().decode()

    wide, _, _ = model(512, 8)
    fused, _, _ = build(VOCAB, "joint", 2, 5)                    # the fused family's shape (256 wide, 8 heads)
    z = z2.cuda()
    z_before = z.clone()
    rc, msg = call(fused.eval(), z)
    assert rc == -1 and "scldm_sample_ode" in msg, msg           # the message names the fused entry
    rc, msg = call(wide, z, n_steps=0)
    assert rc == -1 and "n_steps" in msg, msg
    rc, msg = call(wide, z, method=5)
    assert rc == -1 and "method" in msg, msg
    rc, msg = call(wide, z, null_z=True)
    assert rc == -1 and "null" in msg, msg
    assert torch.equal(z, z_before)
    # the forward entry leaves its output alone as well
    L, h = fused._native_handle()
    w, _ = fused._weights_struct(tuple(fused.parameters()))
    out = torch.full((2 * B, 16, 16), 7.0, device="cuda")
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    tt = torch.zeros(1, device="cuda")
    rc = L.scldm_dit_infer_forward_cfg(h, C.byref(w), z.data_ptr(), tt.data_ptr(), 0, None, 0, None, B, 0, None, None, out.data_ptr(), 0, ws.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == -1 and "scldm_dit_forward_cfg" in L.scldm_last_error().decode()
    assert bool((out == 7.0).all())
    # ... and the fused entries still refuse the wide handle
    Lw, hw = wide._native_handle()
    ww, _ = wide._weights_struct(tuple(wide.parameters()))
    assert Lw.scldm_dit_load_weights(hw, C.byref(ww), None) == -1 and "fused DiT layer" in Lw.scldm_last_error().decode()
    assert Lw.scldm_sample_ode(hw, z.data_ptr(), None, 0, None, B, 0, None, None, 3, 0, 0, ws.data_ptr(), None) != 0
    torch.cuda.synchronize()
    assert torch.equal(z, z_before)


# ---- 6. routing ------------------------------------------------------------------------------------------------------------------------------
class _Count:
    """Counts the calls of one library entry (the ctypes function object is swapped for a forwarding callable)."""

    def __init__(self, monkeypatch, L, name):
        self.n, fn = 0, getattr(L, name)

        def wrapped(*a):
            self.n += 1
            return fn(*a)
        monkeypatch.setattr(L, name, wrapped)


def test_routing_and_the_switch_back_to_the_composed_route(monkeypatch):
    from scldm_amd import _lib
    L = _lib.lib()
    B = 3
    z2, c2 = cfg_case(B, 17)
    scales = SCALES["joint"]
    monkeypatch.setenv("SCLDM_WIDE_INFER", "0")
    m0, _, _ = build(VOCAB, "joint", 2, 55, n_embed=512, n_head=8)      # the knob is read when the native handle is created
    m0.eval()
    m0._native_handle()
    monkeypatch.delenv("SCLDM_WIDE_INFER")
    m1, _, _ = build(VOCAB, "joint", 2, 55, n_embed=512, n_head=8)
    m1.eval()
    ode, train_fwd = _Count(monkeypatch, L, "scldm_dit_infer_sample_ode"), _Count(monkeypatch, L, "scldm_dit_train_forward")
    # switched off: the composed Python loop over scldm_dit_train_forward, as before
    out0 = m0.sample_ode_cfg(z2.cuda(), cuda(c2), scales, 4, "euler")
    assert ode.n == 0 and train_fwd.n == 3 * 2
    z, hstep = z2.cuda().clone(), 1.0 / 3
    for i in range(3):
        z = z + hstep * m0._generic_forward_with_cfg(z, torch.full((2 * B,), i * hstep, device="cuda"), cuda(c2), scales)
    assert torch.equal(out0, z)
    # default: the whole solve is ONE call of the new entry and no training forward
    train_fwd.n = 0
    out1 = m1.sample_ode_cfg(z2.cuda(), cuda(c2), scales, 4, "euler")
    assert ode.n == 1 and train_fwd.n == 0
    check_err(out1.cpu(), out0.cpu(), TOL_FP32, "wide sampler: new route vs composed route")
    # eval-mode forward: the new route has the composed route's bits
    gen = torch.Generator().manual_seed(2)
    x, t = torch.randn(9, 16, 16, generator=gen).cuda(), torch.rand(9, generator=gen).cuda()
    lab = cuda({k: torch.randint(0, v, (9,), generator=gen) for k, v in VOCAB.items()})
    for prec in ("fp32", "bf16"):
        m0.precision = m1.precision = prec
        train_fwd.n = 0
        y1 = m1(x, t, lab)
        assert train_fwd.n == 0
        y0 = m0(x, t, lab)
        assert train_fwd.n == 1
        assert torch.equal(y1, y0), prec
    # training mode keeps the training route
    m1.train()
    train_fwd.n = 0
    with torch.no_grad():
        m1(x, t, lab, force_drop_ids=False)
    assert train_fwd.n == 1

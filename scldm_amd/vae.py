"""TransformerVAE with the reference's API (src/scldm/vae.py:15-87); encode / decode run on the MI355X MCAB kernels."""
from __future__ import annotations

import ctypes as C
import os

import torch
import torch.nn as nn
from torch._utils import _unflatten_dense_tensors

from . import _lib
from .layers import InputTransformerVAE, swiglu_hidden
from .nnets import Decoder, DecoderScvi, Encoder, EncoderScvi, _require_cuda_f32, _stream_ptr
from .stochastic_layers import (GaussianLinearLayer, GaussianTransformerLayer, NegativeBinomial, NegativeBinomialLinearLayer,
                                NegativeBinomialTransformerLayer, Normal)


def table_order(genes: torch.Tensor, genes_subset: torch.Tensor, counts_subset: torch.Tensor, n_rows: int):
    """Index of the ordered table gradients (scldm_vae_train_backward_ordered, include/scldm_hip.h): `(order, seg)`, both int32 on
    the inputs' device.  Entry cell * G + slot is decoder slot (cell, slot) of `genes` (B, G); entry B * G + cell * S + tok is encoder
    token (cell, tok) of `genes_subset` (B, S).  `order` lists the entries sorted by table row (the gene id), ascending entry index
    inside a row (a stable sort); `seg` holds n_rows + 1 offsets, table row r owning order[seg[r]:seg[r + 1]].  Encoder tokens with a
    zero count are left out: their contribution is exactly zero and the atomic path skips them too.  Integer plumbing through torch
    (sort / searchsorted), on CPU tensors as well; it allocates, so it cannot run under stream capture."""
    B, G = genes.shape
    S = genes_subset.shape[1]
    if genes_subset.shape[0] != B or counts_subset.shape != genes_subset.shape:
        raise ValueError(f"expected genes (B,G) and genes_subset / counts_subset (B,S); got {tuple(genes.shape)}, "
                         f"{tuple(genes_subset.shape)}, {tuple(counts_subset.shape)}")
    if B * (G + S) > 2 ** 31 - 65:
        raise ValueError(f"B * (G + S) = {B * (G + S)} entries exceed the int32 entry index")
    dev = genes.device
    keys = torch.cat([genes.reshape(-1), genes_subset.reshape(-1)]).to(torch.long)
    keep = torch.cat([torch.ones(B * G, dtype=torch.bool, device=dev), counts_subset.reshape(-1) != 0])
    entries = torch.arange(B * (G + S), device=dev)[keep]
    keys, perm = torch.sort(keys[keep], stable=True)
    order = entries[perm].to(torch.int32)
    seg = torch.searchsorted(keys, torch.arange(n_rows + 1, device=dev)).to(torch.int32)      # seg[r] = entries with a row below r
    return order, seg


def train_split(B: int, S: int, G: int):
    """((tiles, chunks) of the per-gene decoder backward, (tiles, chunks) of the pooling backward) at batch B, S encoder tokens and G
    decoded genes: every cell gets `chunks` workgroups, each walking `tiles` 64-token tiles (scldm_vae_train_split: the split the
    training backward launches with in this process; host arithmetic, no GPU)."""
    out = (C.c_int * 4)()
    _lib.check(_lib.lib().scldm_vae_train_split(B, S, G, out), "scldm_vae_train_split")
    return (out[0], out[1]), (out[2], out[3])


def _grad_structs(module, params, dev):
    """(flat, w, g) of a training backward: every gradient is a view of ONE zero-initialised buffer `flat` (parameters the kernels do
    not write, e.g. a frozen table, stay 0).  The offsets, the weight-pointer struct `w` and (while the allocator hands back the same
    block) the gradient-pointer struct `g` are cached on the module: building two 175-field ctypes structs per step is host time a
    batch-32 step cannot hide."""
    cache = module.__dict__.setdefault("_train_cache", {})
    pk = tuple(p.data_ptr() for p in params)
    if cache.get("pk") != pk:
        offs, total = {}, 0
        for p in params:       # dense: the kernels write gradients with 4-byte stores / atomics, nothing needs more alignment
            offs[id(p)] = total
            total += p.numel()
        cache.clear()
        cache.update(pk=pk, offs=offs, total=total, w=module._weights_struct(lambda t: t.data_ptr()))
    offs, total = cache["offs"], cache["total"]
    flat = torch.zeros(total, dtype=torch.float32, device=dev)
    base = flat.data_ptr()
    if cache.get("gbase") != base:
        cache["gbase"], cache["g"] = base, module._weights_struct(lambda t: base + 4 * offs[id(t)])
    return flat, cache["w"][0], cache["g"][0]


def _ordered_mode(module) -> bool:
    return bool(module.deterministic) or module.__dict__.get("_env_deterministic", False) or torch.are_deterministic_algorithms_enabled()


class _VAETrainFn(torch.autograd.Function):
    """TransformerVAE.forward with a HIP backward (scldm_vae_train_forward / _backward, include/scldm_hip.h): replaces torch
    autograd over the reference's module tree (vae.py:29-56) inside VAE.training_step (models.py:249-290).  Outputs mu, theta
    (B, G) and z (B, 16, n_lat) are ordinary differentiable tensors: the reference's own `-log_nb_positive(counts, mu, theta)`
    (models.py:243) - or scldm_amd.distributions.log_nb_positive, the fused form - sits on top of them unchanged.  The operand policy
    (`module.precision`, "fp32" or "fp16") is read at the forward and used by the backward of the same step."""

    @staticmethod
    def forward(ctx, module, counts_subset, genes_subset, genes, lib, *params):
        L, h = module._native()
        B, S = counts_subset.shape
        G = genes.shape[1]
        dev = counts_subset.device
        mu = torch.empty(B, G, device=dev, dtype=torch.float32)
        theta = torch.empty(B, G, device=dev, dtype=torch.float32)
        z = torch.empty(B, module.encoder.latent_dim, module.encoder.latent_embedding, device=dev, dtype=torch.float32)
        saved = torch.empty(L.scldm_vae_train_saved_bytes(h, B), dtype=torch.uint8, device=dev)
        ws = torch.empty(L.scldm_vae_train_workspace_bytes(h, B, S, G), dtype=torch.uint8, device=dev)
        prec = _lib.PRECISIONS[module.precision]
        if prec == _lib.PREC_FP16:
            module.found_inf_flag()     # (registers the flag with the handle: the fp16 backward resets and sets it)
        with torch.cuda.device(dev):
            _lib.check(L.scldm_vae_train_forward_ex(h, counts_subset.data_ptr(), genes_subset.data_ptr(), B, S, genes.data_ptr(), lib.data_ptr(),
                                                    G, mu.data_ptr(), theta.data_ptr(), z.data_ptr(), saved.data_ptr(), ws.data_ptr(), prec,
                                                    _stream_ptr()),
                       "scldm_vae_train_forward_ex")
        ctx.module, ctx.saved, ctx.ws, ctx.prec = module, saved, ws, prec
        ctx.inputs = (counts_subset, genes_subset, genes, lib)
        ctx.outs = (mu, theta, z)
        ctx.params = params
        ctx.param_versions = [p._version for p in params]
        return mu, theta, z

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dmu, dtheta, dz):
        module, params = ctx.module, ctx.params
        L, h = _lib.lib(), module._handle
        if [p._version for p in params] != ctx.param_versions:
            raise RuntimeError("TransformerVAE parameters were modified between forward and backward (the HIP backward reads them live)")
        counts_subset, genes_subset, genes, lib = ctx.inputs
        mu, theta, z = ctx.outs
        B, S = counts_subset.shape
        G = genes.shape[1]
        dev = mu.device
        prep = lambda t: None if t is None else t.contiguous().float()
        dmu, dtheta, dz = prep(dmu), prep(dtheta), prep(dz)
        flat, w, g = _grad_structs(module, params, dev)
        ptr = lambda t: None if t is None else t.data_ptr()
        args = (h, C.byref(w), C.byref(g), counts_subset.data_ptr(), genes_subset.data_ptr(), B, S, genes.data_ptr(), lib.data_ptr(), G,
                mu.data_ptr(), theta.data_ptr(), z.data_ptr(), ptr(dmu), ptr(dtheta), ptr(dz), ctx.saved.data_ptr(), ctx.ws.data_ptr(),
                ctx.prec)
        ordered = _ordered_mode(module)
        with torch.cuda.device(dev):
            if ordered:
                order, seg, rows = _ordered_index(module, L, h, genes, genes_subset, counts_subset)
                _lib.check(L.scldm_vae_train_backward_ordered(*args, order.data_ptr(), seg.data_ptr(), order.numel(), rows.data_ptr(),
                                                              _stream_ptr()),
                           "scldm_vae_train_backward_ordered")
            else:
                _lib.check(L.scldm_vae_train_backward_ex(*args, _stream_ptr()), "scldm_vae_train_backward_ex")
        module.last_table_gradient_mode = "ordered" if ordered else "atomic"
        ctx.saved = ctx.ws = None
        views = _unflatten_dense_tensors(flat, params)      # one C++ call instead of 175 slices + views
        out = [v if ctx.needs_input_grad[5 + i] else None for i, v in enumerate(views)]
        return (None, None, None, None, None, *out)


def _ordered_index(module, L, h, genes, genes_subset, counts_subset):
    """(order, seg, rows) of an ordered backward: the table index and the row buffer."""
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("the ordered (deterministic) VAE training backward cannot be captured into a graph: building "
                           "the table index allocates; capture the default (atomic) mode or run this step eagerly")
    B, G = genes.shape
    order, seg = table_order(genes, genes_subset, counts_subset, module.input_layer.gene_embedding.weight.shape[0])
    rows = torch.empty(L.scldm_vae_train_rows_bytes(h, B, genes_subset.shape[1], G), dtype=torch.uint8, device=genes.device)
    return order, seg, rows


class _VAEGaussTrainFn(torch.autograd.Function):
    """`_VAETrainFn` for the Gaussian head (scldm_vae_train_gaussian_forward / _backward): outputs mu (B, G) and z, fp32.  The loss
    on top is the reference's `log_gaussian(log1p(counts / rowsum * 1e4), mu).sum(1).mean()` (models.py:239-245) in torch ops, or
    scldm_amd.distributions.gaussian_recon_loss, the fused form."""

    @staticmethod
    def forward(ctx, module, counts_subset, genes_subset, genes, *params):
        L, h = module._native()
        B, S = counts_subset.shape
        G = genes.shape[1]
        dev = counts_subset.device
        mu = torch.empty(B, G, device=dev, dtype=torch.float32)
        z = torch.empty(B, module.encoder.latent_dim, module.encoder.latent_embedding, device=dev, dtype=torch.float32)
        saved = torch.empty(L.scldm_vae_train_saved_bytes(h, B), dtype=torch.uint8, device=dev)
        ws = torch.empty(L.scldm_vae_train_workspace_bytes(h, B, S, G), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(L.scldm_vae_train_gaussian_forward(h, counts_subset.data_ptr(), genes_subset.data_ptr(), B, S, genes.data_ptr(), G,
                                                          mu.data_ptr(), z.data_ptr(), saved.data_ptr(), ws.data_ptr(), _stream_ptr()),
                       "scldm_vae_train_gaussian_forward")
        ctx.module, ctx.saved, ctx.ws = module, saved, ws
        ctx.inputs = (counts_subset, genes_subset, genes)
        ctx.outs = (mu, z)
        ctx.params = params
        ctx.param_versions = [p._version for p in params]
        return mu, z

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dmu, dz):
        module, params = ctx.module, ctx.params
        L, h = _lib.lib(), module._handle
        if [p._version for p in params] != ctx.param_versions:
            raise RuntimeError("TransformerVAE parameters were modified between forward and backward (the HIP backward reads them live)")
        counts_subset, genes_subset, genes = ctx.inputs
        mu, z = ctx.outs
        B, S = counts_subset.shape
        G = genes.shape[1]
        dev = mu.device
        prep = lambda t: None if t is None else t.contiguous().float()
        dmu, dz = prep(dmu), prep(dz)
        flat, w, g = _grad_structs(module, params, dev)
        ptr = lambda t: None if t is None else t.data_ptr()
        ordered = _ordered_mode(module)
        with torch.cuda.device(dev):
            order = seg = rows = None
            if ordered:
                order, seg, rows = _ordered_index(module, L, h, genes, genes_subset, counts_subset)
            _lib.check(L.scldm_vae_train_gaussian_backward(h, C.byref(w), C.byref(g), counts_subset.data_ptr(), genes_subset.data_ptr(), B, S,
                                                           genes.data_ptr(), G, mu.data_ptr(), z.data_ptr(), ptr(dmu), ptr(dz),
                                                           ctx.saved.data_ptr(), ctx.ws.data_ptr(), ptr(order), ptr(seg),
                                                           order.numel() if ordered else 0, ptr(rows), _stream_ptr()),
                       "scldm_vae_train_gaussian_backward")
        module.last_table_gradient_mode = "ordered" if ordered else "atomic"
        ctx.saved = ctx.ws = None
        views = _unflatten_dense_tensors(flat, params)
        out = [v if ctx.needs_input_grad[4 + i] else None for i, v in enumerate(views)]
        return (None, None, None, None, *out)


class _VAEWideTrainFn(torch.autograd.Function):
    """`_VAETrainFn` for the wide shapes (TransformerVAE.train_wide).  The forward IS the inference route - scldm_vaew_encode on the
    subset, scldm_vaew_decode on all genes, launched as under no_grad, so the outputs are bit-equal to the no_grad forward - and keeps
    only the inputs and (mu, theta, z).  The backward (scldm_vaew_train_backward, exact fp32) rebuilds the record per chunk of cells
    under the workspace cap (SCLDM_VAEW_WS_MB) and walks it back; the two embedding tables' gradients are fixed-order segmented sums
    over `table_order`'s index, so every gradient is bit-equal run to run on one build, one GPU model and one cap (another cap is
    another chunking: the weight gradients may then differ in the last bits).  The step cannot be captured into a graph: building the
    index allocates."""

    @staticmethod
    def forward(ctx, module, counts_subset, genes_subset, genes, lib, *params):
        z = module.encode(counts_subset, genes_subset)
        nb = module.decode(z, genes, lib)
        ctx.module = module
        ctx.inputs = (counts_subset, genes_subset, genes, lib)
        ctx.outs = (nb.mu, nb.theta, z)
        ctx.params = params
        ctx.param_versions = [p._version for p in params]
        return nb.mu, nb.theta, z

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dmu, dtheta, dz):
        module, params = ctx.module, ctx.params
        if [p._version for p in params] != ctx.param_versions:
            raise RuntimeError("TransformerVAE parameters were modified between forward and backward (the HIP backward reads them live)")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("the wide TransformerVAE training backward cannot be captured into a graph: building the table index "
                               "allocates; run this step eagerly")
        L, h = module._native_wide()
        counts_subset, genes_subset, genes, lib = ctx.inputs
        mu, theta, z = ctx.outs
        B, S = counts_subset.shape
        G = genes.shape[1]
        dev = mu.device
        prep = lambda t: None if t is None else t.contiguous().float()
        dmu, dtheta, dz = prep(dmu), prep(dtheta), prep(dz)
        flat, _, g = _grad_structs(module, params, dev)
        ptr = lambda t: None if t is None else t.data_ptr()
        need = L.scldm_vaew_train_workspace_bytes(h, B, S, G)
        if need == 0:
            raise _lib.ScldmError(f"scldm_vaew_train_workspace_bytes failed: {L.scldm_last_error().decode()}")
        ws = module.__dict__.get("_wtrain_ws")
        if ws is None or ws.numel() < need or ws.device != dev:
            module.__dict__["_wtrain_ws"] = None
            ws = module.__dict__["_wtrain_ws"] = torch.empty(need, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            order, seg = table_order(genes, genes_subset, counts_subset, module.input_layer.gene_embedding.weight.shape[0])
            rows = torch.empty(L.scldm_vaew_train_rows_bytes(h, B, S, G), dtype=torch.uint8, device=dev)
            _lib.check(L.scldm_vaew_train_backward(h, C.byref(g), counts_subset.data_ptr(), genes_subset.data_ptr(), B, S, genes.data_ptr(),
                                                   lib.data_ptr(), G, mu.data_ptr(), theta.data_ptr(), z.data_ptr(), ptr(dmu), ptr(dtheta),
                                                   ptr(dz), order.data_ptr(), seg.data_ptr(), order.numel(), rows.data_ptr(), ws.data_ptr(),
                                                   _stream_ptr()),
                       "scldm_vaew_train_backward")
        module.last_table_gradient_mode = "ordered"
        views = _unflatten_dense_tensors(flat, params)
        out = [v if ctx.needs_input_grad[5 + i] else None for i, v in enumerate(views)]
        return (None, None, None, None, None, *out)


class TransformerVAE(nn.Module):
    # Gradients of the two embedding tables (gene_embedding, theta) in training: False = float atomics (torch's own embedding
    # backward does the same), True = a fixed-order segmented sum (scldm_vae_train_backward_ordered): with it EVERY gradient is
    # bit-equal run to run on one build and one GPU model - what the reference trainer's `deterministic:` asks for
    # (experiments/configs/training/default.yaml:14).  Also on with SCLDM_VAE_DETERMINISTIC=1 (read when the native handle is
    # created) or while torch.are_deterministic_algorithms_enabled().  Ordered steps cannot be captured into a graph.
    deterministic: bool = False
    # Training of the Gaussian head (GaussianTransformerLayer): False = forward under autograd raises NotImplementedError, as it did
    # before that head had a backward; True = forward returns differentiable {"mu"}, z through the Gaussian per-gene backward
    # (scldm_vae_train_gaussian_forward / _backward; `precision` "fp32" only).  `deterministic` selects the ordered mode as for NB.
    train_gaussian_head: bool = False
    # Training of the unshared-theta NB head (NegativeBinomialTransformerLayer(shared_theta=False): params is Linear(32, 2), theta =
    # exp of its second output, no table): False = forward under autograd raises NotImplementedError, as it did before that head had a
    # backward; True = forward returns differentiable {"mu", "theta"}, z through `_VAETrainFn` (the C entries route on the handle:
    # wide::dec_gene_bwd_nb2_kernel), `precision` "fp32" or "fp16", `deterministic` as for the shared head.
    train_unshared_theta: bool = False
    # Training of the wide shapes (`wide`: n_embed 64..1024, the route of scldm_vaew_*): False = forward under autograd raises
    # NotImplementedError ("inference only"), as it did before that route had a backward; True = forward returns differentiable
    # {"mu", "theta"}, z through `_VAEWideTrainFn` (scldm_vaew_train_backward): both NB heads, `precision` "fp32" only, the table
    # gradients always in the ordered mode (every gradient bit-equal run to run), so a step cannot be captured into a graph.
    train_wide: bool = False
    last_table_gradient_mode: str | None = None      # "ordered" / "atomic": the mode of the last backward

    def __init__(self, encoder: Encoder, decoder: Decoder, decoder_head: NegativeBinomialTransformerLayer | GaussianTransformerLayer,
                 input_layer: InputTransformerVAE):
        super().__init__()
        self.encoder = encoder
        self.decoder = decoder
        self.decoder_head = decoder_head
        self.input_layer = input_layer
        self._handle = None
        # operand policy of the contractions of encode / decode / decode_sample - the per-gene MCAB / SwiGLU products and the Linears of
        # the 16-token trunks (LayerNorms, softmax, the trunks' 16 x 16 attention and the NB head are fp32 in every policy): "fp32" =
        # exact (parity path); "fp16" = TF32's mantissa, the arithmetic class the reference itself runs the VAE in
        # (set_float32_matmul_precision("high"), experiments/scripts/inference.py:26); "bf16" = 8 bits.  Training (forward under
        # autograd) takes "fp32" or "fp16": the TF32 class of the reference's trainer (experiments/scripts/train.py:18) - fp16 operands in
        # the pooling, the per-gene decoder and every contraction of the per-gene backward, the 16-token trunks exact; see found_inf_flag()
        self.precision = "fp32"
        self._weights_key = None
        self._weights_fp = None
        self.check_weight_fingerprint = True
        self._ws = None
        self._keep = None

    @property
    def gaussian_head(self) -> bool:
        """The head kind, told as the reference tells it: by the class name (vae.py:46-47,82-83)."""
        return self.decoder_head.__class__.__name__ == "GaussianTransformerLayer"

    # ------------------------------------------------------------------ the shape-generic inference route (scldm_vaew_*)
    @property
    def wide(self) -> bool:
        """False: the vae_base shape (n_embed 32, 16 inducing points, heads 8 / 4), which runs on the MCAB kernels (scldm_vae_*).
        True: any other shape; inference (encode / decode / decode_sample / forward under no_grad) runs on the shape-generic route
        (scldm_vaew_*: every product a tile GEMM on the matrix pipe, csrc/vae_wide.hpp), `precision` "fp32" or "fp16", NB head only."""
        enc = self.encoder
        return not (enc.n_embed == 32 and enc.latent_dim == 16 and enc.n_head == 8 and enc.n_head_cross == 4)

    def _native_wide(self):
        if self.gaussian_head:
            raise NotImplementedError("the wide TransformerVAE route (n_embed != 32) decodes the negative-binomial head only: the Gaussian "
                                      "head (GaussianTransformerLayer) is not built for it")
        if self.precision not in ("fp32", "fp16"):
            raise NotImplementedError(f"the wide TransformerVAE route (n_embed != 32) runs in fp32 or fp16 (precision={self.precision!r}); "
                                      "bf16 operands are not built for it")
        L = _lib.lib()
        emb = self.input_layer.gene_embedding.weight
        enc = self.encoder
        if self.__dict__.get("_whandle") is None:
            cfg = _lib.VaeConfig(n_genes=emb.shape[0] - 1, n_embed=emb.shape[1], n_inducing=enc.latent_dim,
                                 n_embed_latent=enc.latent_embedding, n_layer=enc.n_layer, n_head=enc.n_head,
                                 n_head_cross=enc.n_head_cross, hidden_dim=swiglu_hidden(enc.n_embed, enc.multiple_of),
                                 layernorm_eps=enc.layernorm_eps, positional_encoding=int(enc.pos_embed is not None),
                                 nb_temperature=float(self.decoder_head.t))
            h = C.c_void_p()
            rc = L.scldm_vaew_create(C.byref(cfg), C.byref(h))      # host arithmetic: the shape family and the workspace cap
            if rc == -1:                                            # SCLDM_ERR_SHAPE: the message names the violated condition
                raise NotImplementedError(L.scldm_last_error().decode())
            _lib.check(rc, "scldm_vaew_create")
            self.__dict__["_whandle"] = h
            self.__dict__["_wkey"] = None
        if emb.device.type != "cuda":
            raise RuntimeError("TransformerVAE parameters must live on a CUDA (ROCm) device; there is no CPU path")
        h = self.__dict__["_whandle"]
        key = tuple(p.data_ptr() for p in self.parameters())
        if key != self.__dict__.get("_wkey"):       # new storages.  The kernels read the parameters where they live and keep nothing
            for p in self.parameters():             # derived from them, so an in-place update needs no refresh
                if p.dtype != torch.float32 or not p.is_contiguous():
                    raise RuntimeError("TransformerVAE parameters must be contiguous fp32")
            w, keep = self._weights_struct(lambda t: t.data_ptr())
            _lib.check(L.scldm_vaew_load_weights(h, C.byref(w), None), "scldm_vaew_load_weights")
            self.__dict__["_wkey"] = key
        return L, h

    def _wide_workspace(self, L, h, B: int, S: int, G: int) -> int:
        need = L.scldm_vaew_workspace_bytes(h, B, S, G)
        if need == 0:
            raise _lib.ScldmError(f"scldm_vaew_workspace_bytes failed: {L.scldm_last_error().decode()}")
        dev = self.input_layer.gene_embedding.weight.device
        if self._ws is None or self._ws.numel() < need or self._ws.device != dev:
            self._ws = torch.empty(need, dtype=torch.uint8, device=dev)
        return self._ws.data_ptr()

    # ------------------------------------------------------------------ native handle
    def _native(self):
        L = _lib.lib()
        emb = self.input_layer.gene_embedding.weight
        if emb.device.type != "cuda":
            raise RuntimeError("TransformerVAE parameters must live on a CUDA (ROCm) device; there is no CPU path")
        enc = self.encoder
        if self._handle is None:
            cfg = _lib.VaeConfig(n_genes=emb.shape[0] - 1, n_embed=emb.shape[1], n_inducing=enc.latent_dim,
                                 n_embed_latent=enc.latent_embedding, n_layer=enc.n_layer, n_head=enc.n_head,
                                 n_head_cross=enc.n_head_cross, hidden_dim=swiglu_hidden(enc.n_embed, enc.multiple_of),
                                 layernorm_eps=enc.layernorm_eps, positional_encoding=int(enc.pos_embed is not None),
                                 nb_temperature=1.0 if self.gaussian_head else float(self.decoder_head.t))
            h = C.c_void_p()
            with torch.cuda.device(emb.device):
                _lib.check(L.scldm_vae_create(C.byref(cfg), C.byref(h)), "scldm_vae_create")
            self._handle = h
            self.__dict__["_env_deterministic"] = os.environ.get("SCLDM_VAE_DETERMINISTIC", "0") == "1"
        params = list(self.parameters())
        key = tuple(p.data_ptr() for p in params)
        ver = tuple(p._version for p in params)
        if key != self._weights_key:
            self._load_weights(L)             # new storages: the job / fingerprint tables are rebuilt, everything is re-packed
            self._weights_key, self._weights_fp = key, ver
        elif ver != self._weights_fp or self.check_weight_fingerprint:
            # same storages: an optimiser step (version counters moved) or possibly an in-place update through `.data` (EMA-style,
            # invisible to the counters).  Either way the C side compares a device-side fingerprint of every source tensor with that
            # of the packed copies and re-packs in stream order if it moved: five small launches, no host synchronisation (round 3
            # compared per-tensor norms on the host - one sync per encode / decode call - and re-issued ~150 launches per re-pack).
            with torch.cuda.device(emb.device):
                _lib.check(L.scldm_vae_refresh_weights(self._handle, _stream_ptr()), "scldm_vae_refresh_weights")
            self._weights_fp = ver
        return L, self._handle

    def invalidate_weights(self) -> None:
        """Force the next encode / decode to re-derive the packed weight copies from the parameters."""
        self._weights_key = None

    # copies / pickling: the native handle never travels (the copy builds its own at its first call)
    def __getstate__(self):
        state = self.__dict__.copy()
        state.update(_handle=None, _weights_key=None, _weights_fp=None, _ws=None, _keep=None)
        for k in ("_train_cache", "_found_inf", "_found_inf_handle", "_env_deterministic", "_whandle", "_wkey", "_wtrain_ws"):    # (the flag is registered with the handle that does not travel)
            state.pop(k, None)
        return state

    def __setstate__(self, state):
        super().__setstate__(state)
        for k in ("_handle", "_weights_key", "_weights_fp", "_ws", "_keep"):
            self.__dict__.setdefault(k, None)

    def found_inf_flag(self) -> torch.Tensor:
        """Device float the fp16 training backward sets to 1.0 when the per-gene backward produced a non-finite gradient (reset to 0.0
        at the start of every fp16 backward): hand it to an optimizer that understands GradScaler's `found_inf`
        (`scldm_amd.optim.AdamW`: `optimizer.found_inf = vae.found_inf_flag()`), which then skips the step on device, no host read.
        The contract of DiT.found_inf_flag()."""
        L, h = (_lib.lib(), self._handle) if self._handle is not None else self._native()
        dev = self.input_layer.gene_embedding.weight.device
        flag = self.__dict__.get("_found_inf")
        if flag is None or flag.device != dev:
            flag = self.__dict__["_found_inf"] = torch.zeros((), dtype=torch.float32, device=dev)
            self.__dict__["_found_inf_handle"] = None
        if self.__dict__.get("_found_inf_handle") != h.value:     # (re-)register with THIS handle (a copy starts with none)
            _lib.check(L.scldm_vae_train_set_found_inf(h, flag.data_ptr()), "scldm_vae_train_set_found_inf")
            self.__dict__["_found_inf_handle"] = h.value
        return flag

    def _weights_struct(self, dp):
        """scldm_vae_weights filled with dp(parameter) -> device pointer (the same struct, with writable pointers, receives the
        gradients in scldm_vae_train_backward).  Returns (struct, keepalive)."""
        enc, dec = self.encoder, self.decoder
        n = enc.n_layer

        def block(b):
            return _lib.VaeBlock(ln1_w=dp(b.ln_1.weight), ln1_b=dp(b.ln_1.bias), attn_w=dp(b.attn.c_attn.weight),
                                 proj_w=dp(b.attn.c_proj.weight), ln2_w=dp(b.ln_2.weight), ln2_b=dp(b.ln_2.bias), w1=dp(b.mlp.w1.weight),
                                 w2=dp(b.mlp.w2.weight), cproj=dp(b.mlp.c_proj.weight))

        def cross(c):
            return _lib.VaeCross(ln1_w=dp(c.ln_1.weight), ln1_b=dp(c.ln_1.bias), ln1q_w=dp(c.ln_1q.weight), ln1q_b=dp(c.ln_1q.bias),
                                 attn_kv=dp(c.attn.c_attn.weight), attn_q=dp(c.attn.c_attn_q.weight), attn_proj=dp(c.attn.c_proj.weight),
                                 ln2_w=dp(c.ln_2.weight), ln2_b=dp(c.ln_2.bias), w1=dp(c.mlp.w1.weight), w2=dp(c.mlp.w2.weight),
                                 cproj=dp(c.mlp.c_proj.weight))

        eb = (_lib.VaeBlock * max(n, 1))(*[block(b) for b in enc.encoder_layers])
        db = (_lib.VaeBlock * max(n, 1))(*[block(b) for b in dec.decoder_layers])
        head = self.decoder_head
        gauss = self.gaussian_head      # (no theta table, params (1, 32), and decoder_head.ln in the two appended fields)
        w = _lib.VaeWeights(gene_embedding=dp(self.input_layer.gene_embedding.weight), inducing_points=dp(enc.ca_layer.inducing_points),
                            enc_pos_embed=dp(enc.pos_embed) if enc.pos_embed is not None else None,
                            enc_latent_w=dp(enc.encoder_latent_input[0].weight), dec_latent_w=dp(dec.decoder_latent_input[1].weight),
                            theta=dp(head.theta.weight) if not gauss and head.theta is not None else None,   # NULL = unshared theta
                            head_w=dp(head.params.weight),
                            head_b=dp(head.params.bias), enc_cross=cross(enc.ca_layer),
                            dec_cross=cross(dec.decoder_cross_attention), enc_blocks=eb, dec_blocks=db,
                            head_ln_w=dp(head.ln.weight) if gauss else None, head_ln_b=dp(head.ln.bias) if gauss else None)
        return w, (eb, db)

    def _load_weights(self, L):
        for p in self.parameters():
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError("TransformerVAE parameters must be contiguous fp32")
        w, keep = self._weights_struct(lambda t: t.data_ptr())
        self._keep = keep
        with torch.cuda.device(self.input_layer.gene_embedding.weight.device):
            _lib.check(L.scldm_vae_load_weights(self._handle, C.byref(w), _stream_ptr()), "scldm_vae_load_weights")

    def _workspace(self, L, B: int, G: int) -> int:
        need = L.scldm_vae_workspace_bytes(self._handle, B, G)
        dev = self.input_layer.gene_embedding.weight.device
        if self._ws is None or self._ws.numel() < need or self._ws.device != dev:
            self._ws = torch.empty(need, dtype=torch.uint8, device=dev)
        return self._ws.data_ptr()

    KERNEL_KINDS = ("enc_pool", "enc_cell", "dec_cell", "dec_gene", "dec_finalize")

    def kernel_timing(self, enable: bool | None = None):
        """Measurement hook (bench.py): `kernel_timing(True / False)` switches HIP-event pairs around every MCAB kernel launch on /
        off; `kernel_timing()` drains them and returns {kernel: (launches, total ms)} (scldm_vae_kernel_timing)."""
        L, h = self._native()
        if enable is not None:
            L.scldm_vae_kernel_timing_enable(h, int(enable))
            return None
        out = {}
        for k, name in enumerate(self.KERNEL_KINDS):
            n, ms = C.c_int(), C.c_double()
            _lib.check(L.scldm_vae_kernel_timing(h, k, C.byref(n), C.byref(ms)), "scldm_vae_kernel_timing")
            out[name] = (n.value, ms.value)
        return out

    def __del__(self):
        try:
            if self._handle is not None:
                _lib.lib().scldm_vae_destroy(self._handle)
            if self.__dict__.get("_whandle") is not None:
                _lib.lib().scldm_vaew_destroy(self.__dict__["_whandle"])
        except Exception:
            pass

    # ------------------------------------------------------------------ reference API (vae.py:29-87)
    @torch.no_grad()
    def encode(self, counts: torch.Tensor, genes: torch.Tensor, counts_subset: torch.Tensor | None = None,
               genes_subset: torch.Tensor | None = None) -> torch.Tensor:
        c = counts_subset if counts_subset is not None else counts
        g = genes_subset if genes_subset is not None else genes
        wide = self.wide
        L, h = self._native_wide() if wide else self._native()
        c = _require_cuda_f32("counts", c)
        if not g.is_cuda:
            raise RuntimeError("genes must be a CUDA (ROCm) tensor")
        g = g.to(torch.long).contiguous()
        if c.dim() != 2 or g.shape != c.shape:
            raise ValueError(f"counts and genes must both be (B,S); got {tuple(c.shape)} and {tuple(g.shape)}")
        B, S = c.shape
        z = torch.empty(B, self.encoder.latent_dim, self.encoder.latent_embedding, device=c.device, dtype=torch.float32)
        if wide:
            ws = self._wide_workspace(L, h, B, S, 0)
            with torch.cuda.device(c.device):
                _lib.check(L.scldm_vaew_encode(h, c.data_ptr(), g.data_ptr(), B, S, z.data_ptr(), _lib.PRECISIONS[self.precision], ws,
                                               _stream_ptr()), "scldm_vaew_encode")
            return z
        ws = self._workspace(L, B, 1)
        with torch.cuda.device(c.device):
            _lib.check(L.scldm_vae_encode(h, c.data_ptr(), g.data_ptr(), B, S, z.data_ptr(), _lib.PRECISIONS[self.precision], ws,
                                          _stream_ptr()), "scldm_vae_encode")
        return z

    @torch.no_grad()
    def decode(self, z: torch.Tensor, genes: torch.Tensor, library_size: torch.Tensor,
               condition: dict[str, torch.Tensor] | None = None) -> torch.distributions.Distribution:
        wide = self.wide
        L, h = self._native_wide() if wide else self._native()
        z = _require_cuda_f32("z", z)
        if not genes.is_cuda:
            raise RuntimeError("genes must be a CUDA (ROCm) tensor")
        g = genes.to(torch.long).contiguous()
        lib = _require_cuda_f32("library_size", library_size).reshape(-1)
        B, G = g.shape
        if z.shape != (B, self.encoder.latent_dim, self.encoder.latent_embedding) or lib.shape[0] != B:
            raise ValueError(f"expected z (B,{self.encoder.latent_dim},{self.encoder.latent_embedding}) and library_size (B,1); got "
                             f"{tuple(z.shape)}, {tuple(library_size.shape)} for genes {tuple(g.shape)}")
        mu = torch.empty(B, G, device=z.device, dtype=torch.float32)
        if wide:
            theta = torch.empty(B, G, device=z.device, dtype=torch.float32)
            ws = self._wide_workspace(L, h, B, 0, G)
            with torch.cuda.device(z.device):
                _lib.check(L.scldm_vaew_decode(h, z.data_ptr(), g.data_ptr(), lib.data_ptr(), B, G, mu.data_ptr(), theta.data_ptr(),
                                               _lib.PRECISIONS[self.precision], ws, _stream_ptr()), "scldm_vaew_decode")
            return NegativeBinomial(mu=mu, theta=theta)
        ws = self._workspace(L, B, G)
        if self.gaussian_head:      # Normal(mu, 1) (vae.py:83-85); library_size is accepted and unused, as in the reference
            with torch.cuda.device(z.device):
                _lib.check(L.scldm_vae_decode_gaussian(h, z.data_ptr(), g.data_ptr(), B, G, mu.data_ptr(), _lib.PRECISIONS[self.precision], ws,
                                                       _stream_ptr()), "scldm_vae_decode_gaussian")
            return Normal(mu, 1.0)
        theta = torch.empty(B, G, device=z.device, dtype=torch.float32)
        with torch.cuda.device(z.device):
            _lib.check(L.scldm_vae_decode(h, z.data_ptr(), g.data_ptr(), lib.data_ptr(), B, G, mu.data_ptr(), theta.data_ptr(),
                                          _lib.PRECISIONS[self.precision], ws, _stream_ptr()), "scldm_vae_decode")
        return NegativeBinomial(mu=mu, theta=theta)

    @torch.no_grad()
    def decode_sample(self, z: torch.Tensor, genes: torch.Tensor, library_size: torch.Tensor, seed: int | None = None) -> torch.Tensor:
        """`decode(z, genes, library_size).sample()` in one call (models.py:819 after vae.py:71-87): the negative-binomial draw is
        fused into the decoder's normalisation pass, mu / theta never reach HBM.  Returns counts (B, G) fp32.  Gaussian head: mu + n
        from the per-gene kernel's epilogue, bit for bit `decode(...).sample(seed=seed)`.  The wide route (`wide`) has no fused
        draw: it is decode followed by scldm_nb_sample."""
        if self.wide:
            if seed is None:
                seed = int(torch.randint(0, 2 ** 62, (), dtype=torch.int64).item())
            return self.decode(z, genes, library_size).sample(seed=seed)
        L, h = self._native()
        z = _require_cuda_f32("z", z)
        if not genes.is_cuda:
            raise RuntimeError("genes must be a CUDA (ROCm) tensor")
        g = genes.to(torch.long).contiguous()
        lib = _require_cuda_f32("library_size", library_size).reshape(-1)
        B, G = g.shape
        if z.shape != (B, self.encoder.latent_dim, self.encoder.latent_embedding) or lib.shape[0] != B:
            raise ValueError(f"expected z (B,{self.encoder.latent_dim},{self.encoder.latent_embedding}) and library_size (B,1); got "
                             f"{tuple(z.shape)}, {tuple(library_size.shape)} for genes {tuple(g.shape)}")
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (), dtype=torch.int64).item())
        counts = torch.empty(B, G, device=z.device, dtype=torch.float32)
        ws = self._workspace(L, B, G)
        if self.gaussian_head:
            with torch.cuda.device(z.device):
                _lib.check(L.scldm_vae_decode_gaussian_sample(h, z.data_ptr(), g.data_ptr(), B, G, counts.data_ptr(), C.c_uint64(seed),
                                                              _lib.PRECISIONS[self.precision], ws, _stream_ptr()),
                           "scldm_vae_decode_gaussian_sample")
            return counts
        with torch.cuda.device(z.device):
            _lib.check(L.scldm_vae_decode_sample(h, z.data_ptr(), g.data_ptr(), lib.data_ptr(), B, G, counts.data_ptr(), C.c_uint64(seed),
                                                 _lib.PRECISIONS[self.precision], ws, _stream_ptr()), "scldm_vae_decode_sample")
        return counts

    def forward(self, counts, genes, library_size, counts_subset=None, genes_subset=None):
        """(params, z) with params = {"mu", "theta"}, or {"mu"} for the Gaussian head (vae.py:29-56).  With gradients enabled and trainable parameters the outputs
        are differentiable.  A wide shape: with `train_wide = True`, in exact fp32, through `_VAEWideTrainFn`.  The 32-wide shape:
        forward on the inference kernels + a hand-derived HIP backward (`_VAETrainFn`), in `precision` "fp32"
        (exact) or "fp16" (the reference's TF32 class; overflow flag: found_inf_flag()); the Gaussian head with
        `train_gaussian_head = True`, in fp32 (`_VAEGaussTrainFn`); the unshared-theta NB head with `train_unshared_theta = True`
        (`_VAETrainFn`: theta is then the per-element (B, G) dispersion).  As in the
        reference, the encoder reads counts_subset / genes_subset (vae.py:37-40: no fallback to the full vectors in forward)."""
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            wide = self.wide
            if wide and not self.train_wide:
                raise NotImplementedError("the wide TransformerVAE route (n_embed != 32) is inference only: there is no HIP backward for "
                                          "it; call forward under torch.no_grad()")
            if wide:        # `train_wide`: the NB heads in exact fp32 (scldm_vaew_train_backward)
                if not self.gaussian_head and self.precision != "fp32":
                    raise NotImplementedError(f"the wide TransformerVAE route trains in exact fp32 only (precision={self.precision!r})")
                self._native_wide()     # refuses the Gaussian head, a shape outside the family and a CPU module
            if self.gaussian_head and not self.train_gaussian_head:
                raise NotImplementedError("training the Gaussian head (GaussianTransformerLayer) is switched off: set "
                                          "`train_gaussian_head = True` on the module (fp32), or call forward under torch.no_grad()")
            if self.gaussian_head and self.precision != "fp32":
                raise NotImplementedError(f"the Gaussian head trains in fp32 only (precision={self.precision!r})")
            if counts_subset is None or genes_subset is None:
                raise ValueError("TransformerVAE.forward needs counts_subset / genes_subset (the reference passes them to the input layer, vae.py:37-40)")
            cs = _require_cuda_f32("counts_subset", counts_subset)
            if not genes_subset.is_cuda or not genes.is_cuda:
                raise RuntimeError("genes / genes_subset must be CUDA (ROCm) tensors")
            gs = genes_subset.to(torch.long).contiguous()
            g = genes.to(torch.long).contiguous()
            lib = _require_cuda_f32("library_size", library_size).reshape(-1)
            if cs.dim() != 2 or gs.shape != cs.shape or g.dim() != 2 or g.shape[0] != cs.shape[0] or lib.shape[0] != cs.shape[0]:
                raise ValueError(f"expected counts_subset / genes_subset (B,S), genes (B,G), library_size (B,1); got {tuple(cs.shape)}, "
                                 f"{tuple(gs.shape)}, {tuple(g.shape)}, {tuple(library_size.shape)}")
            if wide:
                mu, theta, z = _VAEWideTrainFn.apply(self, cs, gs, g, lib, *tuple(self.parameters()))
                return {"mu": mu, "theta": theta}, z
            if self.gaussian_head:
                mu, z = _VAEGaussTrainFn.apply(self, cs, gs, g, *tuple(self.parameters()))
                return {"mu": mu}, z
            if self.decoder_head.theta is None and not self.train_unshared_theta:
                raise NotImplementedError("the HIP training backward runs the shared-theta NB head (vae_base.yaml:62) by default; training "
                                          "the unshared-theta head (stochastic_layers.py:94-96) is switched off: set "
                                          "`train_unshared_theta = True` on the module, or call forward under torch.no_grad()")
            if self.precision not in ("fp32", "fp16"):
                raise NotImplementedError(f"TransformerVAE training runs in fp32 or fp16 (precision={self.precision!r})")
            params = tuple(self.parameters())
            mu, theta, z = _VAETrainFn.apply(self, cs, gs, g, lib, *params)
            return {"mu": mu, "theta": theta}, z
        with torch.no_grad():
            z = self.encode(counts, genes, counts_subset, genes_subset)
            nb = self.decode(z, genes, library_size)
            if self.gaussian_head:
                return {"mu": nb.mu}, z        # vae.py:47-49
            return {"mu": nb.mu, "theta": nb.theta}, z


class ScviVAE(nn.Module):
    """The scVI-style baseline with the reference's API (src/scldm/vae.py:90-128): `EncoderScvi` -> `GaussianLinearLayer` ->
    `DecoderScvi` -> `NegativeBinomialLinearLayer`, plus the prior the training loss uses.  Inference: eval mode, exact fp32, on
    the kernels of csrc/scvi.hpp (scldm_scvi_*).  The weights are read where they live; the BatchNorm affine and running statistics
    and the Linear bias of every MLP layer are folded into one scale / shift pair per column by a fingerprint-guarded packing launch
    in front of every call, so `load_state_dict`, an optimiser step or an in-place `.data` / buffer update is picked up by the next
    call.

    Training is opt-in: with `train_enabled = True` a module in training mode runs `forward` through one autograd function on the
    kernels of csrc/scvi_train.hpp (scldm_scvi_train_forward / _backward: BatchNorm batch statistics, dropout, the whole backward).
    With the default, training mode is refused as before.

    fp16 operands are opt-in as well: with `fp16_enabled = True`, `precision = "fp16"` runs every product of the eval-mode calls on
    the same kernel on csrc/scvi_tile.hpp's F16Operands (operands rounded to fp16, fp32 accumulate and epilogues: the reference's TF32 class).  With the
    default the setter refuses everything but "fp32" as before; training is fp32 whatever that switch says.

    Training on fp16 operands is a third opt-in: with `train_enabled`, `fp16_enabled` and `train_fp16_enabled = True`,
    `precision = "fp16"` runs the training forward and backward through scldm_scvi_train_forward_ex / _backward_ex on fp16 operands
    (the class the reference trains in).  Gradient operands carry one power of two per tensor, formed on the device, so callers pass
    unscaled gradients and use no loss scale; `found_inf_flag()` is the overflow flag.  With the default, training at
    `precision = "fp16"` is refused as before."""

    train_enabled = False
    fp16_enabled = False
    train_fp16_enabled = False

    def __init__(self, encoder: EncoderScvi, encoder_head: GaussianLinearLayer, decoder: DecoderScvi,
                 decoder_head: NegativeBinomialLinearLayer, prior: nn.Module):
        super().__init__()
        self.encoder = encoder
        self.encoder_head = encoder_head
        self.decoder = decoder
        self.decoder_head = decoder_head
        self.prior = prior
        self._precision = "fp32"
        self._handle = None
        self._weights_key = None
        self._ws = None
        self._keep = None
        self._train_ws = None
        self.last_dropout_masks = None

    @property
    def precision(self) -> str:
        return self._precision

    @precision.setter
    def precision(self, value: str) -> None:
        if value != "fp32" and not self.fp16_enabled:
            raise NotImplementedError(f"ScviVAE runs in exact fp32 only (precision={value!r}); fp16 / bf16 operands are not built for it")
        if value not in ("fp32", "fp16"):
            raise NotImplementedError(f"ScviVAE runs in fp32 or, with fp16_enabled, on fp16 operands (precision={value!r}); "
                                      "bf16 operands are not built for it")
        self._precision = value

    # ------------------------------------------------------------------ native handle
    def _layers(self, mlp):
        return [(mlp[4 * i], mlp[4 * i + 1]) for i in range(len(mlp) // 4)]

    def _tensors(self):
        """Every parameter and buffer the kernels read."""
        out = []
        for mlp in (self.encoder.encoder_mlp, self.decoder.decoder_mlp):
            for lin, bn in self._layers(mlp):
                out += [lin.weight, lin.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var]
        eh, dh = self.encoder_head, self.decoder_head
        out += [eh.loc.weight, eh.loc.bias, eh.scale.weight, eh.scale.bias, dh.mu.weight, dh.mu.bias]
        out += [dh.theta] if dh.shared_theta else [dh.theta.weight, dh.theta.bias]
        return out

    def _check_mode(self, *inputs) -> None:
        if self.training:
            drop = max(float(self.encoder.dropout), float(self.decoder.dropout))
            extra = f" (dropout={drop:g} would also need a mask kernel)" if drop > 0 else ""
            raise NotImplementedError("ScviVAE has no training path: BatchNorm1d batch statistics and the backward are not built; call "
                                      f".eval() first{extra}")
        if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in inputs):
            raise NotImplementedError("ScviVAE is inference only: an input requires grad under enabled autograd, and there is no HIP "
                                      "backward for this model; detach the input or call it under torch.no_grad()")

    def _native(self):
        L = _lib.lib()
        w0 = self.decoder_head.mu.weight
        if w0.device.type != "cuda":
            raise RuntimeError("ScviVAE parameters must live on a CUDA (ROCm) device; there is no CPU path")
        enc_layers, dec_layers = self._layers(self.encoder.encoder_mlp), self._layers(self.decoder.decoder_mlp)
        if self._handle is None:
            eps = {float(bn.eps) for _, bn in enc_layers + dec_layers}
            if len(eps) != 1:
                raise NotImplementedError(f"the packed BatchNorm fold takes one eps for every layer (got {sorted(eps)})")
            G, H = w0.shape
            h = C.c_void_p()
            _lib.check(L.scldm_scvi_create(len(enc_layers), len(dec_layers), G, H, self.encoder_head.loc.weight.shape[0],
                                           int(self.decoder_head.shared_theta), eps.pop(), C.byref(h)), "scldm_scvi_create")
            self._handle = h
        tensors = self._tensors()
        key = tuple(t.data_ptr() for t in tensors)
        if key != self._weights_key:
            for t in tensors:
                if t.dtype != torch.float32 or not t.is_contiguous() or t.device != w0.device:
                    raise RuntimeError("ScviVAE parameters and buffers must be contiguous fp32 on one device")

            def layer(lin, bn):
                return _lib.ScviLayer(w=lin.weight.data_ptr(), b=lin.bias.data_ptr(), bn_w=bn.weight.data_ptr(), bn_b=bn.bias.data_ptr(),
                                      bn_mean=bn.running_mean.data_ptr(), bn_var=bn.running_var.data_ptr())
            ea = (_lib.ScviLayer * len(enc_layers))(*[layer(*l) for l in enc_layers])
            da = (_lib.ScviLayer * len(dec_layers))(*[layer(*l) for l in dec_layers])
            eh, dh = self.encoder_head, self.decoder_head
            shared = dh.shared_theta
            p = _lib.ScviParams(enc=ea, dec=da, loc_w=eh.loc.weight.data_ptr(), loc_b=eh.loc.bias.data_ptr(),
                                scale_w=eh.scale.weight.data_ptr(), scale_b=eh.scale.bias.data_ptr(), mu_w=dh.mu.weight.data_ptr(),
                                mu_b=dh.mu.bias.data_ptr(), theta_w=dh.theta.data_ptr() if shared else dh.theta.weight.data_ptr(),
                                theta_b=None if shared else dh.theta.bias.data_ptr())
            with torch.cuda.device(w0.device):
                _lib.check(L.scldm_scvi_pack(self._handle, C.byref(p), _stream_ptr()), "scldm_scvi_pack")
            self._weights_key = key
        return L, self._handle

    def _workspace(self, L, B: int) -> int:
        need = L.scldm_scvi_workspace_bytes(self._handle, B)
        dev = self.decoder_head.mu.weight.device
        if self._ws is None or self._ws.numel() < need or self._ws.device != dev:
            self._ws = torch.empty(need, dtype=torch.uint8, device=dev)
        return self._ws.data_ptr()

    def __getstate__(self):
        state = self.__dict__.copy()
        state.update(_handle=None, _weights_key=None, _ws=None, _keep=None, _train_ws=None, last_dropout_masks=None)
        for k in ("_found_inf", "_found_inf_handle"):      # (the flag is registered with the handle that does not travel)
            state.pop(k, None)
        return state

    def found_inf_flag(self) -> torch.Tensor:
        """Device float the fp16 training backward sets to 1.0 when an upstream gradient, an intermediate gradient tensor or a
        parameter gradient it produced is non-finite (reset to 0.0 at the start of every fp16 backward): hand it to an optimizer that
        understands GradScaler's `found_inf` (`scldm_amd.optim.AdamW`: `optimizer.found_inf = vae.found_inf_flag()`), which then
        skips the step on device, no host read.  The contract of TransformerVAE.found_inf_flag()."""
        L, h = (_lib.lib(), self._handle) if self._handle is not None else self._native()
        dev = self.decoder_head.mu.weight.device
        flag = self.__dict__.get("_found_inf")
        if flag is None or flag.device != dev:
            flag = self.__dict__["_found_inf"] = torch.zeros((), dtype=torch.float32, device=dev)
            self.__dict__["_found_inf_handle"] = None
        if self.__dict__.get("_found_inf_handle") != h.value:     # (re-)register with THIS handle (a copy starts with none)
            _lib.check(L.scldm_scvi_train_set_found_inf(h, flag.data_ptr()), "scldm_scvi_train_set_found_inf")
            self.__dict__["_found_inf_handle"] = h.value
        return flag

    def __del__(self):
        try:
            if self._handle is not None:
                _lib.lib().scldm_scvi_destroy(self._handle)
        except Exception:
            pass

    @property
    def _dims(self):
        G, H = self.decoder_head.mu.weight.shape
        return G, H, self.encoder_head.loc.weight.shape[0]

    def _counts(self, counts: torch.Tensor) -> torch.Tensor:
        c = _require_cuda_f32("counts", counts)
        G = self._dims[0]
        if c.dim() != 2 or c.shape[1] != G:
            raise ValueError(f"counts must be (B, {G}); got {tuple(c.shape)}")
        return c

    def _library(self, library_size: torch.Tensor, B: int) -> torch.Tensor:
        lib = _require_cuda_f32("library_size", library_size).reshape(-1)
        if lib.shape[0] != B:
            raise ValueError(f"library_size must hold one value per cell, (B,) or (B, 1) with B = {B}; got {tuple(library_size.shape)}")
        return lib

    def _encode(self, counts: torch.Tensor, eps: torch.Tensor | None):
        L, h = self._native()
        c = self._counts(counts)
        B = c.shape[0]
        G, H, nl = self._dims
        new = lambda *s: torch.empty(*s, device=c.device, dtype=torch.float32)   # noqa: E731
        hz, loc, scale = new(B, H), new(B, nl), new(B, nl)
        z = None
        if eps is not None:
            eps = _require_cuda_f32("eps", eps)
            if eps.shape != (B, nl):
                raise ValueError(f"eps must be (B, n_latent) = ({B}, {nl}); got {tuple(eps.shape)}")
            z = new(B, nl)
        ws = self._workspace(L, B)
        with torch.cuda.device(c.device):
            _lib.check(L.scldm_scvi_encode_ex(h, c.data_ptr(), B, eps.data_ptr() if eps is not None else None, hz.data_ptr(), loc.data_ptr(),
                                              scale.data_ptr(), z.data_ptr() if z is not None else None, _lib.PRECISIONS[self._precision],
                                              ws, _stream_ptr()), "scldm_scvi_encode_ex")
        return hz, loc, scale, z

    # ------------------------------------------------------------------ reference API (vae.py:90-128)
    @torch.no_grad()
    def _encode_checked(self, counts, eps=None):
        return self._encode(counts, eps)

    def encode(self, counts: torch.Tensor) -> torch.distributions.Normal:
        """The variational posterior Normal(loc, scale) of `counts` (B, n_genes) (encoder, then encoder_head)."""
        self._check_mode(counts)
        _, loc, scale, _ = self._encode_checked(counts)
        return Normal(loc, scale)

    def encode_hidden(self, counts: torch.Tensor, eps: torch.Tensor | None = None):
        """(h, loc, scale, z): the encoder MLP's output next to the posterior's parameters; z = loc + eps scale when eps is given."""
        self._check_mode(counts)
        return self._encode_checked(counts, eps)

    def decode(self, z: torch.Tensor, genes: torch.Tensor | None, library_size: torch.Tensor,
               condition: dict[str, torch.Tensor] | None = None) -> NegativeBinomial:
        """NegativeBinomial(mu, theta) of latents z (B, n_latent): decoder, then decoder_head (what VAEScvi.sample calls,
        models.py; `genes` and `condition` are accepted and unused, as the reference's head ignores them)."""
        self._check_mode(z, library_size)
        with torch.no_grad():
            L, h = self._native()
            z = _require_cuda_f32("z", z)
            G, H, nl = self._dims
            if z.dim() != 2 or z.shape[1] != nl:
                raise ValueError(f"z must be (B, {nl}); got {tuple(z.shape)}")
            B = z.shape[0]
            lib = self._library(library_size, B)
            mu = torch.empty(B, G, device=z.device, dtype=torch.float32)
            theta = torch.empty((G,) if self.decoder_head.shared_theta else (B, G), device=z.device, dtype=torch.float32)
            ws = self._workspace(L, B)
            with torch.cuda.device(z.device):
                _lib.check(L.scldm_scvi_decode_ex(h, z.data_ptr(), lib.data_ptr(), lib.shape[0], B, mu.data_ptr(), theta.data_ptr(),
                                                  _lib.PRECISIONS[self._precision], ws, _stream_ptr()), "scldm_scvi_decode_ex")
        return NegativeBinomial(mu=mu, theta=theta)

    def forward_outputs(self, counts: torch.Tensor, library_size: torch.Tensor, eps: torch.Tensor | None = None) -> dict[str, torch.Tensor]:
        """Every array one scldm_scvi_forward call writes, by name: the encoder MLP's output `h` (B, n_hidden), `loc`, `scale`, `z`
        (B, n_latent), `mu` (B, n_genes) and `theta` ((n_genes,) shared, else (B, n_genes)).  `forward` wraps this and drops `h`, which
        the reference's forward does not return."""
        self._check_mode(counts, library_size)
        with torch.no_grad():
            L, h = self._native()
            c = self._counts(counts)
            B = c.shape[0]
            G, H, nl = self._dims
            lib = self._library(library_size, B)
            if eps is None:
                eps = torch.randn(B, nl, device=c.device, dtype=torch.float32)
            eps = _require_cuda_f32("eps", eps)
            if eps.shape != (B, nl):
                raise ValueError(f"eps must be (B, n_latent) = ({B}, {nl}); got {tuple(eps.shape)}")
            new = lambda *s: torch.empty(*s, device=c.device, dtype=torch.float32)   # noqa: E731
            hz, loc, scale, z, mu = new(B, H), new(B, nl), new(B, nl), new(B, nl), new(B, G)
            theta = new(G) if self.decoder_head.shared_theta else new(B, G)
            ws = self._workspace(L, B)
            with torch.cuda.device(c.device):
                _lib.check(L.scldm_scvi_forward_ex(h, c.data_ptr(), lib.data_ptr(), lib.shape[0], B, eps.data_ptr(), hz.data_ptr(),
                                                   loc.data_ptr(), scale.data_ptr(), z.data_ptr(), mu.data_ptr(), theta.data_ptr(),
                                                   _lib.PRECISIONS[self._precision], ws, _stream_ptr()), "scldm_scvi_forward_ex")
        return {"h": hz, "loc": loc, "scale": scale, "z": z, "mu": mu, "theta": theta}

    # ------------------------------------------------------------------ training (opt-in)
    def _train_params(self):
        """The trainable parameters in the order _ScviTrainFn returns their gradients."""
        out = []
        eh, dh = self.encoder_head, self.decoder_head
        for lin, bn in self._layers(self.encoder.encoder_mlp):
            out += [lin.weight, lin.bias, bn.weight, bn.bias]
        out += [eh.loc.weight, eh.loc.bias, eh.scale.weight, eh.scale.bias]
        for lin, bn in self._layers(self.decoder.decoder_mlp):
            out += [lin.weight, lin.bias, bn.weight, bn.bias]
        out += [dh.mu.weight, dh.mu.bias]
        out += [dh.theta] if dh.shared_theta else [dh.theta.weight, dh.theta.bias]
        return out

    def _train_workspace(self, L, B: int) -> int:
        need = L.scldm_scvi_train_workspace_bytes(self._handle, B)
        dev = self.decoder_head.mu.weight.device
        if self._train_ws is None or self._train_ws.numel() < need or self._train_ws.device != dev:
            self._train_ws = torch.empty(need, dtype=torch.uint8, device=dev)
        return self._train_ws.data_ptr()

    def _train_forward(self, counts, library_size, eps, seed, dropout_masks):
        if self._precision != "fp32" and not (self.train_fp16_enabled and self.fp16_enabled and self._precision == "fp16"):
            raise NotImplementedError(f"ScviVAE trains in exact fp32 only (precision={self._precision!r})")
        for name, t in (("counts", counts), ("library_size", library_size), ("eps", eps)):
            if isinstance(t, torch.Tensor) and t.requires_grad:
                raise NotImplementedError(f"ScviVAE training forms no gradient with respect to its inputs ({name} requires grad); detach it")
        bns = [bn for mlp in (self.encoder.encoder_mlp, self.decoder.decoder_mlp) for _, bn in self._layers(mlp)]
        if any(bn.momentum is None for bn in bns):
            raise NotImplementedError("ScviVAE training takes a numeric BatchNorm momentum (momentum=None, the cumulative average, is not built)")
        if len({float(bn.momentum) for bn in bns}) != 1:
            raise NotImplementedError(f"ScviVAE training takes one BatchNorm momentum for every layer (got {sorted({float(bn.momentum) for bn in bns})})")
        if len({float(bn.eps) for bn in bns}) != 1:
            raise NotImplementedError(f"the packed BatchNorm fold takes one eps for every layer (got {sorted({float(bn.eps) for bn in bns})})")
        if counts.dim() == 2 and counts.shape[0] < 2:
            raise ValueError(f"BatchNorm1d in training mode needs at least two cells per batch (got B = {counts.shape[0]})")
        c = self._counts(counts)
        B = c.shape[0]
        G, H, nl = self._dims
        lib = self._library(library_size, B)
        if eps is None:
            eps = torch.randn(B, nl, device=c.device, dtype=torch.float32)
        eps = _require_cuda_f32("eps", eps)
        if eps.shape != (B, nl):
            raise ValueError(f"eps must be (B, n_latent) = ({B}, {nl}); got {tuple(eps.shape)}")
        n_enc, n_dec = len(self.encoder.encoder_mlp) // 4, len(self.decoder.decoder_mlp) // 4
        rates = [float(self.encoder.dropout)] * n_enc + [float(self.decoder.dropout)] * n_dec
        if dropout_masks is not None:
            dropout_masks = list(dropout_masks)
            if len(dropout_masks) != n_enc + n_dec:
                raise ValueError(f"dropout_masks must hold one (B, {H}) uint8 mask per MLP layer, encoder first ({n_enc + n_dec}); got {len(dropout_masks)}")
            masks = []
            for p, m in zip(rates, dropout_masks):
                if p > 0:
                    if not isinstance(m, torch.Tensor) or not m.is_cuda or m.shape != (B, H):
                        raise ValueError(f"every dropout mask of an MLP with dropout > 0 must be a CUDA (ROCm) tensor of shape ({B}, {H})")
                    m = m.to(torch.uint8).contiguous()
                masks.append(m if p > 0 else None)
        else:
            masks = [torch.empty(B, H, dtype=torch.uint8, device=c.device) if p > 0 else None for p in rates]
            if seed is None:
                seed = int(torch.randint(0, 2 ** 62, (), dtype=torch.int64).item()) if any(p > 0 for p in rates) else 0
        mu, theta, loc, scale, z = _ScviTrainFn.apply(self, c, lib, eps, int(seed or 0), masks, dropout_masks is not None,
                                                      *self._train_params())
        for bn in bns:
            bn.num_batches_tracked += 1
        self.last_dropout_masks = masks
        return NegativeBinomial(mu=mu, theta=theta), Normal(loc, scale), z

    def forward(self, counts: torch.Tensor, genes: torch.Tensor | None, library_size: torch.Tensor,
                condition: dict[str, torch.Tensor] | None = None, counts_subset: torch.Tensor | None = None,
                genes_subset: torch.Tensor | None = None, masking_prop: float = 0.0, mask_token_idx: int = 0, *,
                eps: torch.Tensor | None = None, seed: int | None = None, dropout_masks=None):
        """(NegativeBinomial(mu, theta), Normal(loc, scale), z) as the reference's forward returns them (vae.py:106-128);
        `eps` (B, n_latent) is the reparameterisation noise (default: torch.randn on the device).  genes, condition, counts_subset,
        genes_subset, masking_prop and mask_token_idx are accepted and ignored, as in the reference.  The encoder's hidden `h`, which
        the same call computes, is dropped here: `forward_outputs` returns it.

        In training mode with `train_enabled` the five tensors are differentiable with respect to the parameters (one HIP forward, one
        HIP backward), the BatchNorm running statistics and `num_batches_tracked` advance, and dropout keeps an element with the
        module's rates: the keep masks are drawn on the device from `seed` (default: a draw from torch's global generator) or given as
        `dropout_masks`, one (B, n_hidden) uint8 tensor per MLP layer, encoder first; the masks used are left in
        `last_dropout_masks`.  `seed` and `dropout_masks` mean nothing in eval mode."""
        if self.training and self.train_enabled:
            return self._train_forward(counts, library_size, eps, seed, dropout_masks)
        o = self.forward_outputs(counts, library_size, eps)
        return NegativeBinomial(mu=o["mu"], theta=o["theta"]), Normal(o["loc"], o["scale"]), o["z"]


class _ScviTrainFn(torch.autograd.Function):
    """ScviVAE's training forward and backward: scldm_scvi_train_forward_ex / scldm_scvi_train_backward_ex (include/scldm_hip.h), the
    backward in the precision its forward ran in."""

    @staticmethod
    def forward(ctx, module, counts, lib, eps, seed, masks, masks_given, *params):
        L, h = module._native()
        B = counts.shape[0]
        G, H, nl = module._dims
        dev = counts.device
        new = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)   # noqa: E731
        loc, scale, z, mu = new(B, nl), new(B, nl), new(B, nl), new(B, G)
        theta = new(G) if module.decoder_head.shared_theta else new(B, G)
        record = torch.empty(L.scldm_scvi_train_record_bytes(h, B), dtype=torch.uint8, device=dev)
        mask_ptrs = (C.c_void_p * len(masks))(*[m.data_ptr() if m is not None else None for m in masks])
        p_enc, p_dec = float(module.encoder.dropout), float(module.decoder.dropout)
        momentum = float(module.encoder.encoder_mlp[1].momentum)
        ws = module._train_workspace(L, B)
        prec = _lib.PRECISIONS[module._precision]
        with torch.cuda.device(dev):
            _lib.check(L.scldm_scvi_train_forward_ex(h, counts.data_ptr(), lib.data_ptr(), lib.shape[0], B, eps.data_ptr(), p_enc, p_dec,
                                                     C.c_uint64(seed), mask_ptrs, int(masks_given), momentum, record.data_ptr(),
                                                     loc.data_ptr(), scale.data_ptr(), z.data_ptr(), mu.data_ptr(), theta.data_ptr(),
                                                     prec, ws, _stream_ptr()), "scldm_scvi_train_forward_ex")
        ctx.module, ctx.masks, ctx.rates, ctx.prec = module, masks, (p_enc, p_dec), prec
        # the parameters too: the backward reads the weights through the handle's pointers, so an in-place update between forward
        # and backward (an optimizer step before a second backward with retain_graph) must raise autograd's version error
        ctx.save_for_backward(counts, lib, eps, record, scale, z, mu, theta, *params)
        ctx.set_materialize_grads(False)
        return mu, theta, loc, scale, z

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dmu, dtheta, dloc, dscale, dz):
        module = ctx.module
        counts, lib, eps, record, scale, z, mu, theta, *params = ctx.saved_tensors
        L, h = module._native()
        B = counts.shape[0]
        ups = [None if g is None else g.contiguous().float() for g in (dmu, dtheta, dloc, dscale, dz)]
        grads = [torch.empty_like(p) for p in params]
        it = iter(grads)
        n_enc, n_dec = len(module.encoder.encoder_mlp) // 4, len(module.decoder.decoder_mlp) // 4

        def layers(n):
            return (_lib.ScviLayerGrads * n)(*[_lib.ScviLayerGrads(*[next(it).data_ptr() for _ in range(4)]) for _ in range(n)])
        ea = layers(n_enc)
        head = [next(it).data_ptr() for _ in range(4)]
        da = layers(n_dec)
        shared = module.decoder_head.shared_theta
        lik = [next(it).data_ptr() for _ in range(3 if shared else 4)] + ([None] if shared else [])
        g = _lib.ScviGrads(ea, da, *head, *lik)
        mask_ptrs = (C.c_void_p * len(ctx.masks))(*[m.data_ptr() if m is not None else None for m in ctx.masks])
        ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        ws = module._train_workspace(L, B)
        with torch.cuda.device(counts.device):
            _lib.check(L.scldm_scvi_train_backward_ex(h, counts.data_ptr(), lib.data_ptr(), lib.shape[0], B, eps.data_ptr(), ctx.rates[0],
                                                      ctx.rates[1], mask_ptrs, record.data_ptr(), scale.data_ptr(), z.data_ptr(),
                                                      mu.data_ptr(), theta.data_ptr(), *[ptr(t) for t in ups], C.byref(g), ctx.prec, ws,
                                                      _stream_ptr()), "scldm_scvi_train_backward_ex")
        return (None,) * 7 + tuple(g_ if p.requires_grad else None for g_, p in zip(grads, params))

"""Flow-matching transport with the reference's API (src/scldm/transport/): the Linear and GVP paths, velocity / noise / score models.

`create_transport(...)`, `Transport.training_losses`, `Sampler(transport).sample_ode(...)` / `.sample_sde(...)` keep the
reference signatures (transport/__init__.py:6-12, transport.py:110,269-332).  Differences, by design:
  * path_type "Linear" | "GVP" x prediction "velocity" | "noise" | "score" x loss_weight None | "velocity" | "likelihood" exist;
    (Linear, velocity) is the combination every reference config uses (ldm_base.yaml:30-35) and keeps its own kernels.  The VP
    path raises NotImplementedError.  `sample_sde` and `sample_ode_likelihood` serve the default (Linear, velocity) transport, and every
    other one created with `create_transport(..., samplers_enabled=True)` (off by default: without it they raise NotImplementedError
    there).  Under such a transport every update of the SDE solve is one affine map x' = a_x x + a_m m + a_w w of the state, the model
    output and the step's normals (score = s_x x + s_m m per model type, D(t) per form - "SBDM" = norm Dv included -, SDE drift
    = probability-flow drift + D score), over linspace(t0, t1, num_steps) with (t0, t1) = check_interval(sde=True, eval=True); the
    likelihood integrates -(a x + b m) over solver time linspace(t0, t1) with the model at t = 1 - s.  A solve one of whose scalars is not
    finite (SBDM for a velocity model, a score at t = 1, sample_eps = 0 for a noise / score model) raises ValueError before any model call,
    naming the evaluation and its time.  A scldm_amd DiT of the fused family runs both as one C call (`DiT.sample_sde_cfg(...,
    transport=)` -> scldm_sample_sde_transport, `DiT.log_likelihood_cfg(..., transport=)` -> scldm_logp_ode_transport);
  * the reference hands stepping to third-party torchdiffeq (integrators.py:111, default dopri5); here the
    fixed-grid "euler" / "heun" schemes are built in (definition + KAT: oracle/transport.py), and when the
    model is a scldm_amd DiT bound through `forward_with_cfg` the whole loop runs inside one C call
    (scldm_sample_ode); the reference's default, adaptive dopri5, is a host-driven Dormand-Prince 5(4) over the
    fused `forward_with_cfg` (parity unpinned like the fixed grids: torchdiffeq is un-vendored).
"""
from __future__ import annotations

import enum

import torch


class ModelType(enum.Enum):
    NOISE = enum.auto()
    SCORE = enum.auto()
    VELOCITY = enum.auto()


class PathType(enum.Enum):
    LINEAR = enum.auto()
    GVP = enum.auto()
    VP = enum.auto()


class WeightType(enum.Enum):
    NONE = enum.auto()
    VELOCITY = enum.auto()
    LIKELIHOOD = enum.auto()


def _expand_like(t: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    return t.view(t.shape[0], *([1] * (x.dim() - 1)))


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


class _FlowMatchLoss(torch.autograd.Function):
    """loss_b = mean((pred - ut)^2) over everything but the batch axis (mean_flat, utils.py:15-17) with its gradient w.r.t. pred,
    one HIP kernel each (scldm_fm_loss / scldm_fm_loss_bwd) instead of the ~8 elementwise / reduction launches of the eager form."""

    @staticmethod
    def forward(ctx, pred, ut):
        import ctypes as C
        from .. import _lib
        pred, ut = pred.contiguous(), ut.contiguous()
        n, e = pred.shape[0], pred[0].numel()
        loss = torch.empty(n, dtype=torch.float32, device=pred.device)
        with torch.cuda.device(pred.device):
            _lib.check(_lib.lib().scldm_fm_loss(pred.data_ptr(), ut.data_ptr(), loss.data_ptr(), n, e, _stream()), "scldm_fm_loss")
        ctx.save_for_backward(pred, ut)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gloss):
        from .. import _lib
        pred, ut = ctx.saved_tensors
        n, e = pred.shape[0], pred[0].numel()
        gloss = gloss.contiguous().float()
        dpred = torch.empty_like(pred)
        with torch.cuda.device(pred.device):
            _lib.check(_lib.lib().scldm_fm_loss_bwd(pred.data_ptr(), ut.data_ptr(), gloss.data_ptr(), dpred.data_ptr(), n, e, _stream()),
                       "scldm_fm_loss_bwd")
        return dpred, None


class _WeightedFlowMatchLoss(torch.autograd.Function):
    """loss_b = w_b mean((c_b m - tgt)^2) with its gradient w.r.t. m (scldm_fm_wloss / scldm_fm_wloss_bwd); rowc (n, 2) holds {c, w}."""

    @staticmethod
    def forward(ctx, pred, tgt, rowc):
        from .. import _lib
        pred = pred.contiguous()
        n, e = pred.shape[0], pred[0].numel()
        loss = torch.empty(n, dtype=torch.float32, device=pred.device)
        with torch.cuda.device(pred.device):
            _lib.check(_lib.lib().scldm_fm_wloss(pred.data_ptr(), tgt.data_ptr(), rowc.data_ptr(), loss.data_ptr(), n, e, _stream()), "scldm_fm_wloss")
        ctx.save_for_backward(pred, tgt, rowc)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gloss):
        from .. import _lib
        pred, tgt, rowc = ctx.saved_tensors
        n, e = pred.shape[0], pred[0].numel()
        gloss = gloss.contiguous().float()
        dpred = torch.empty_like(pred)
        with torch.cuda.device(pred.device):
            _lib.check(_lib.lib().scldm_fm_wloss_bwd(pred.data_ptr(), tgt.data_ptr(), rowc.data_ptr(), gloss.data_ptr(), dpred.data_ptr(), n, e,
                                                     _stream()), "scldm_fm_wloss_bwd")
        return dpred, None, None


SDE_DIFFUSION_FORMS = ("sigma", "linear", "constant", "decreasing", "inccreasing-decreasing")   # (the reference's spelling, path.py:69)
SDE_LAST_STEPS = (None, "Mean", "Tweedie", "Euler")


class LinearPath:
    """The Linear path x_t = t x1 + (1 - t) x0 (path.py:14-151: alpha_t = t, sigma_t = 1 - t) - the members the SDE sampler reads."""

    def compute_diffusion(self, x, t, form="constant", norm=1.0):
        """D(t) of path.py:52-77, broadcast against x.  "SBDM" is not offered: under this path it is (1 - t) / t, infinite at the
        t0 = 0 the sampler starts from; "constant" returns a tensor (the reference's Python float breaks its own `th.sqrt`)."""
        te = _expand_like(t, x)
        if form in ("sigma", "linear"):
            return norm * (1 - te)
        if form == "constant":
            return torch.full_like(te, float(norm))
        if form == "decreasing":
            return 0.25 * (norm * torch.cos(torch.pi * te) + 1) ** 2
        if form == "inccreasing-decreasing":
            return norm * torch.sin(torch.pi * te) ** 2
        raise NotImplementedError(f"Diffusion form {form} not implemented")

    def get_score_from_velocity(self, velocity, x, t):
        """score = (alpha/alpha' v - x) / (sigma^2 - alpha/alpha' sigma' sigma) = (t v - x) / (1 - t)  (path.py:79-95)."""
        te = _expand_like(t, x)
        sigma = 1 - te
        return (te * velocity - x) / (sigma ** 2 + te * sigma)

    # the reference's member names (path.py:24-151: ICPlan), same expressions in the same order
    def compute_alpha_t(self, t):
        return t, 1

    def compute_sigma_t(self, t):
        return 1 - t, -1

    def compute_d_alpha_alpha_ratio_t(self, t):
        return 1 / t

    def compute_drift(self, x, t):
        """(-alpha'/alpha x, Dv = alpha'/alpha sigma^2 - sigma sigma')  (path.py:42-50)."""
        t = _expand_like(t, x)
        alpha_ratio = self.compute_d_alpha_alpha_ratio_t(t)
        sigma_t, d_sigma_t = self.compute_sigma_t(t)
        return -(alpha_ratio * x), alpha_ratio * (sigma_t ** 2) - sigma_t * d_sigma_t

    def get_noise_from_velocity(self, velocity, x, t):
        t = _expand_like(t, x)
        alpha_t, d_alpha_t = self.compute_alpha_t(t)
        sigma_t, d_sigma_t = self.compute_sigma_t(t)
        reverse_alpha_ratio = alpha_t / d_alpha_t
        return (reverse_alpha_ratio * velocity - x) / (reverse_alpha_ratio * d_sigma_t - sigma_t)

    def get_velocity_from_score(self, score, x, t):
        drift, var = self.compute_drift(x, t)
        return var * score - drift

    def compute_mu_t(self, t, x0, x1):
        t = _expand_like(t, x1)
        return self.compute_alpha_t(t)[0] * x1 + self.compute_sigma_t(t)[0] * x0

    def compute_xt(self, t, x0, x1):
        return self.compute_mu_t(t, x0, x1)

    def compute_ut(self, t, x0, x1, xt):
        t = _expand_like(t, x1)
        return self.compute_alpha_t(t)[1] * x1 + self.compute_sigma_t(t)[1] * x0

    def plan(self, t, x0, x1):
        xt = self.compute_xt(t, x0, x1)
        return t, xt, self.compute_ut(t, x0, x1, xt)


class GVPPath(LinearPath):
    """The GVP path x_t = sin(pi t / 2) x1 + cos(pi t / 2) x0 (path.py:190-208: GVPCPlan)."""

    def compute_alpha_t(self, t):
        import math
        return torch.sin(t * math.pi / 2), math.pi / 2 * torch.cos(t * math.pi / 2)

    def compute_sigma_t(self, t):
        import math
        return torch.cos(t * math.pi / 2), -math.pi / 2 * torch.sin(t * math.pi / 2)

    def compute_d_alpha_alpha_ratio_t(self, t):
        import math
        return math.pi / (2 * torch.tan(t * math.pi / 2))

    def compute_diffusion(self, x, t, form="constant", norm=1.0):
        if form == "sigma":
            return norm * self.compute_sigma_t(_expand_like(t, x))[0]
        return super().compute_diffusion(x, t, form=form, norm=norm)

    def get_score_from_velocity(self, velocity, x, t):
        """(alpha/alpha' v - x) / (sigma^2 - alpha/alpha' sigma' sigma)  (path.py:79-95)."""
        t = _expand_like(t, x)
        alpha_t, d_alpha_t = self.compute_alpha_t(t)
        sigma_t, d_sigma_t = self.compute_sigma_t(t)
        reverse_alpha_ratio = alpha_t / d_alpha_t
        return (reverse_alpha_ratio * velocity - x) / (sigma_t ** 2 - reverse_alpha_ratio * d_sigma_t * sigma_t)


_C_PATH = {PathType.LINEAR: 0, PathType.GVP: 1}                                      # SCLDM_PATH_*
_C_MODEL = {ModelType.VELOCITY: 0, ModelType.NOISE: 1, ModelType.SCORE: 2}           # SCLDM_MODEL_*
_C_WEIGHT = {WeightType.NONE: 0, WeightType.VELOCITY: 1, WeightType.LIKELIHOOD: 2}   # SCLDM_WEIGHT_*


class Transport:
    samplers_enabled = False   # opt-in: sample_sde / sample_ode_likelihood under a transport other than (Linear, velocity)

    def __init__(self, *, model_type, path_type, loss_type, train_eps, sample_eps, samplers_enabled=False):
        if path_type not in _C_PATH:
            raise NotImplementedError("the VP path is not provided: path_type 'Linear' and 'GVP' are (its fp32 arithmetic forms 1 - exp(...) "
                                      "next to t = 1 and needs a design of its own)")
        if model_type not in _C_MODEL or loss_type not in _C_WEIGHT:
            raise NotImplementedError(f"model_type={model_type!r}, loss_type={loss_type!r}")
        for name, eps in (("train_eps", train_eps), ("sample_eps", sample_eps)):
            if not 0 <= eps < 0.5:
                raise ValueError(f"{name} must lie in [0, 0.5), got {eps}")
        self.model_type, self.path_type, self.loss_type = model_type, path_type, loss_type
        self.train_eps, self.sample_eps = train_eps, sample_eps
        self.path_sampler = LinearPath() if path_type is PathType.LINEAR else GVPPath()
        self.samplers_enabled = bool(samplers_enabled)

    @property
    def is_default(self) -> bool:
        """The Linear path with a velocity model: the combination with its own kernels and one-call samplers."""
        return self.path_type is PathType.LINEAR and self.model_type is ModelType.VELOCITY

    def c_struct(self):
        """The scldm_transport of the C ABI (include/scldm_hip.h)."""
        from .. import _lib
        return _lib.TransportC(path=_C_PATH[self.path_type], model=_C_MODEL[self.model_type], weight=_C_WEIGHT[self.loss_type],
                               train_eps=float(self.train_eps), sample_eps=float(self.sample_eps))

    def prior_logp(self, z: torch.Tensor) -> torch.Tensor:
        """Standard multivariate normal log-density of every row of a batched z: -N/2 log 2 pi - sum z^2 / 2 (transport.py:59-67)."""
        import math
        n = z[0].numel()
        return z.new_tensor(-n / 2.0) * math.log(2 * math.pi) - z.pow(2).flatten(1).sum(1) / 2.0

    def check_interval(self, train_eps=None, sample_eps=None, *, diffusion_form="SBDM", sde=False, reverse=False, eval=False,
                       last_step_size=0.0):
        """(t0, t1) of transport.py:69-95 for the Linear and GVP paths: a velocity model integrates and trains over exactly [0, 1];
        noise / score models over [eps, 1 - eps] (eps = train_eps, or sample_eps with eval=True).  Arguments left None are the
        transport's own."""
        train_eps = self.train_eps if train_eps is None else train_eps
        sample_eps = self.sample_eps if sample_eps is None else sample_eps
        t0, t1 = 0, 1
        eps = train_eps if not eval else sample_eps
        if self.model_type != ModelType.VELOCITY:
            # (a velocity model answers (0, 1) with sde=True too, as it always has here: sample_sde forms its own grid end
            # 1 - last_step_size; the reference's values are returned for sde=False)
            t0 = eps
            t1 = 1 - eps if (not sde or last_step_size == 0) else 1 - last_step_size
        if reverse:
            t0, t1 = 1 - t0, 1 - t1
        return t0, t1

    def sample(self, x1: torch.Tensor):
        """x0 ~ N(0, I), t ~ U[t0, t1] as `rand * (t1 - t0) + t0` (transport.py:97-108); [0, 1] for a velocity model."""
        x0 = torch.randn_like(x1)
        t0, t1 = self.check_interval(self.train_eps, self.sample_eps)
        scaled = (t0, t1) != (0, 1)
        if x1.is_cuda and torch.cuda.is_current_stream_capturing():
            # inside a HIP-graph capture (scldm_amd.training.GraphedTrainStep) host code does not run again at replay: t comes from
            # the device generator (whose captured draws advance per replay); same distribution as the reference's CPU draw
            t = torch.rand((x1.shape[0],), device=x1.device, dtype=x1.dtype)
            if scaled:
                t = t * (t1 - t0) + t0
        elif x1.is_cuda:
            # same CPU generator draw as the reference's `torch.rand((B,)).to(x1)`, but through pinned memory and an asynchronous
            # copy: a pageable host-to-device copy blocks the host until everything queued on the stream has finished, which
            # serialises the host's kernel enqueueing with the previous step's device work
            t = torch.rand((x1.shape[0],), pin_memory=True)
            if scaled:
                t = (t * (t1 - t0) + t0).pin_memory()
            t = t.to(x1, non_blocking=True)
        else:
            t = torch.rand((x1.shape[0],))
            if scaled:
                t = t * (t1 - t0) + t0
            t = t.to(x1)
        return t, x0, x1

    def training_losses(self, model, x1, model_kwargs=None):
        """{"pred", "loss"} (transport.py:110-150).  Velocity: loss_b = mean((m - ut)^2), ut = alpha' x1 + sigma' x0 (the loss weight
        is ignored, as in the reference); noise: w mean((m - x0)^2); score: w mean((m sigma + x0)^2); w = 1 | (Dv/sigma)^2 |
        Dv/sigma^2.  CUDA fp32 tensors that need no gradient of their own: one kernel plans (scldm_fm_mix on the default transport,
        scldm_fm_plan otherwise), one forms the row loss, one its gradient; anything else takes the eager expressions."""
        model_kwargs = model_kwargs or {}
        t, x0, x1 = self.sample(x1)
        fused = (x1.is_cuda and x1.dtype == torch.float32 and x0.dtype == torch.float32 and t.dtype == torch.float32
                 and not x1.requires_grad and not x0.requires_grad and not t.requires_grad)
        if not self.is_default:
            return self._training_losses_general(model, t, x0, x1, model_kwargs, fused)
        if fused:
            # same arithmetic as below, two launches instead of five (xt bit-identical: every intermediate rounded separately)
            from .. import _lib
            x1c, x0c, tc = x1.contiguous(), x0.contiguous(), t.contiguous()
            xt, ut = torch.empty_like(x1c), torch.empty_like(x1c)
            with torch.cuda.device(x1.device):
                _lib.check(_lib.lib().scldm_fm_mix(x1c.data_ptr(), x0c.data_ptr(), tc.data_ptr(), xt.data_ptr(), ut.data_ptr(),
                                                   x1c.shape[0], x1c[0].numel(), _stream()), "scldm_fm_mix")
        else:
            te = _expand_like(t, x1)
            xt = te * x1 + (1 - te) * x0
            ut = x1 - x0
        pred = model(xt, t, **model_kwargs)
        assert pred.shape == xt.shape
        if fused and pred.is_cuda and pred.dtype == torch.float32:
            return {"pred": pred, "loss": _FlowMatchLoss.apply(pred, ut)}
        return {"pred": pred, "loss": ((pred - ut) ** 2).mean(dim=list(range(1, pred.dim())))}

    def _training_losses_general(self, model, t, x0, x1, model_kwargs, fused):
        import ctypes as C
        path = self.path_sampler
        if fused:
            from .. import _lib
            x1c, x0c, tc = x1.contiguous(), x0.contiguous(), t.contiguous()
            xt, tgt = torch.empty_like(x1c), torch.empty_like(x1c)
            rowc = torch.empty(x1c.shape[0], 2, dtype=torch.float32, device=x1.device)
            tr = self.c_struct()
            with torch.cuda.device(x1.device):
                _lib.check(_lib.lib().scldm_fm_plan(C.byref(tr), x1c.data_ptr(), x0c.data_ptr(), tc.data_ptr(), xt.data_ptr(), tgt.data_ptr(),
                                                    rowc.data_ptr(), x1c.shape[0], x1c[0].numel(), _stream()), "scldm_fm_plan")
            pred = model(xt, t, **model_kwargs)
            assert pred.shape == xt.shape
            if pred.is_cuda and pred.dtype == torch.float32:
                return {"pred": pred, "loss": _WeightedFlowMatchLoss.apply(pred, tgt, rowc)}
            ut = tgt                      # (a model that answers in another dtype: the eager loss below on the planned tensors)
        else:
            t, xt, ut = path.plan(t, x0, x1)
            pred = model(xt, t, **model_kwargs)
            assert pred.shape == xt.shape
        dims = list(range(1, pred.dim()))
        if self.model_type == ModelType.VELOCITY:
            return {"pred": pred, "loss": ((pred - ut) ** 2).mean(dim=dims)}
        _, drift_var = path.compute_drift(xt, t)
        sigma_t, _ = path.compute_sigma_t(_expand_like(t, xt))
        weight = {WeightType.VELOCITY: (drift_var / sigma_t) ** 2, WeightType.LIKELIHOOD: drift_var / (sigma_t ** 2), WeightType.NONE: 1}[self.loss_type]
        if self.model_type == ModelType.NOISE:
            return {"pred": pred, "loss": (weight * ((pred - x0) ** 2)).mean(dim=dims)}
        return {"pred": pred, "loss": (weight * ((pred * sigma_t + x0) ** 2)).mean(dim=dims)}

    def get_drift(self):
        """body_fn(x, t, model, **kw): the probability-flow drift (transport.py:152-183) - the model output of a velocity model,
        alpha'/alpha x + Dv m of a score model, alpha'/alpha x + Dv (m / -sigma) of a noise model."""
        path, model_type = self.path_sampler, self.model_type

        def body_fn(x, t, model, **model_kwargs):
            if model_type == ModelType.VELOCITY:
                out = model(x, t, **model_kwargs)
            else:
                drift_mean, drift_var = path.compute_drift(x, t)
                out = model(x, t, **model_kwargs)
                if model_type == ModelType.NOISE:
                    out = out / -path.compute_sigma_t(_expand_like(t, x))[0]
                out = -drift_mean + drift_var * out
            assert out.shape == x.shape, "Output shape from ODE solver must match input shape"
            return out

        return body_fn

    def get_score(self):
        """score_fn(x, t, model, **kw) (transport.py:185-202): m / -sigma of a noise model, m of a score model, a velocity model's through the path."""
        path = self.path_sampler
        if self.model_type == ModelType.NOISE:
            return lambda x, t, model, **kw: model(x, t, **kw) / -path.compute_sigma_t(_expand_like(t, x))[0]
        if self.model_type == ModelType.SCORE:
            return lambda x, t, model, **kw: model(x, t, **kw)
        return lambda x, t, model, **kw: path.get_score_from_velocity(model(x, t, **kw), x, t)


def create_transport(path_type="Linear", prediction="velocity", loss_weight=None, train_eps=None, sample_eps=None, *, samplers_enabled=False):
    """Same call as scldm.transport.create_transport.  A velocity model on the Linear or GVP path: both eps forced to 0
    (transport/__init__.py:55-57).  A noise / score model: train_eps and sample_eps default to 1e-3 each.  (The reference's line
    `sample_eps = 1e-3 if train_eps is None else sample_eps` runs after train_eps was reassigned, so it leaves sample_eps = None
    unless the caller passes one and then fails with TypeError in check_interval(eval=True); None becomes 1e-3 here, the value that
    line evidently intends.)  path_type="VP" raises NotImplementedError.
    `samplers_enabled=True` (not in the reference's call) opts into `Sampler.sample_sde` / `.sample_ode_likelihood`, `DiT.sample_sde_cfg` and
    `DiT.log_likelihood_cfg` under a transport other than (Linear, velocity); without it they raise NotImplementedError there, and the
    default transport behaves the same either way."""
    model_type = {"noise": ModelType.NOISE, "score": ModelType.SCORE}.get(prediction, ModelType.VELOCITY)
    loss_type = {"velocity": WeightType.VELOCITY, "likelihood": WeightType.LIKELIHOOD}.get(loss_weight, WeightType.NONE)
    ptype = {"Linear": PathType.LINEAR, "GVP": PathType.GVP, "VP": PathType.VP}[path_type]
    if model_type is ModelType.VELOCITY:
        train_eps = sample_eps = 0
    else:
        train_eps = 1e-3 if train_eps is None else train_eps
        sample_eps = 1e-3 if sample_eps is None else sample_eps
    return Transport(model_type=model_type, path_type=ptype, loss_type=loss_type, train_eps=train_eps, sample_eps=sample_eps,
                     samplers_enabled=samplers_enabled)


# Dormand-Prince 5(4) tableau (Dormand & Prince 1980) and the mid-point weights of the quartic dense output used by
# torchdiffeq's dopri5 (the solver behind the reference's default `sample_ode()`, integrators.py:111).
_DP_A = ((1 / 5,), (3 / 40, 9 / 40), (44 / 45, -56 / 15, 32 / 9), (19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729),
         (9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656), (35 / 384, 0.0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84))
_DP_C = (1 / 5, 3 / 10, 4 / 5, 8 / 9, 1.0, 1.0)
_DP_B = (35 / 384, 0.0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84, 0.0)
_DP_E = (35 / 384 - 1951 / 21600, 0.0, 500 / 1113 - 22642 / 50085, 125 / 192 - 451 / 720, -2187 / 6784 - -12231 / 42400,
         11 / 84 - 649 / 6300, -1.0 / 60.0)
_DP_MID = (6025192743 / 30085553152 / 2, 0.0, 51252292925 / 65400821598 / 2, -2691868925 / 45128329728 / 2,
           187940372067 / 1594534317056 / 2, -1776094331 / 19743644256 / 2, 11237099 / 235043384 / 2)


def _rms(v: torch.Tensor) -> float:
    return float(v.double().pow(2).mean().sqrt())


class Sampler:
    def __init__(self, transport: Transport):
        self.transport = transport
        self.drift = transport.get_drift()
        self.score = transport.get_score()

    def _ode_interval(self) -> tuple[float, float]:
        """(t0, t1) the ODE samplers integrate over: check_interval(..., sde=False, eval=True) - (0, 1) for a velocity model."""
        t0, t1 = self.transport.check_interval(self.transport.train_eps, self.transport.sample_eps, sde=False, eval=True, reverse=False)
        return float(t0), float(t1)

    def _default_only(self, what: str) -> bool:
        """True: the default transport's code path.  False: another transport that opted in (`samplers_enabled`).  Otherwise raises."""
        if self.transport.is_default:
            return True
        if not self.transport.samplers_enabled:
            raise NotImplementedError(f"{what} serves the Linear path with a velocity model only; under another transport use sample_ode")
        return False

    # ---- the SDE sampler and the likelihood under the other transports (opt-in: Transport.samplers_enabled) ----
    def sde_plan(self, *, sampling_method, diffusion_form, diffusion_norm, last_step, last_step_size, num_steps):
        """The grid and the refusal scan of an SDE solve under this transport: (ts fp32 tensor, dt, t1, evaluation times).  (t0, t1) =
        check_interval(sde=True, eval=True, last_step_size) - (0, 1 - last_step_size) for a velocity model.  Every scalar of every update
        x' = a_x x + a_m m + a_w w is formed (scldm_sde_coef_at / scldm_sde_last_coef_at: double, from the fp32 time); one that is not
        finite raises ValueError naming the evaluation and its time, before any model call."""
        import ctypes as C
        import math
        from .. import _lib
        tr = self.transport
        method = str(sampling_method).lower()
        if method not in ("euler", "heun"):
            raise NotImplementedError(f"Sampler type {sampling_method!r} not implemented: 'Euler' and 'Heun' are")
        if diffusion_form not in _lib.SDE_FORMS:
            raise NotImplementedError(f"Diffusion form {diffusion_form} not implemented")
        if last_step not in SDE_LAST_STEPS:
            raise NotImplementedError(f"last_step={last_step!r}: one of {SDE_LAST_STEPS}")
        if last_step is None:
            last_step_size = 0.0
        if num_steps < 2:
            raise ValueError("num_steps must be >= 2 (grid points)")
        if not 0.0 <= last_step_size < 1.0:
            raise ValueError(f"last_step_size must be in [0, 1), got {last_step_size}")
        t0, t1 = tr.check_interval(tr.train_eps, tr.sample_eps, diffusion_form=diffusion_form, sde=True, eval=True, last_step_size=last_step_size)
        if tr.model_type == ModelType.VELOCITY:
            t1 = 1 - last_step_size
        if not t0 < t1:
            raise ValueError(f"the solve's interval [{t0}, {t1}] is empty (sample_eps against 1 - last_step_size)")
        ts = torch.linspace(t0, t1, num_steps)
        dt = ts[1] - ts[0]
        L, trc, form = _lib.lib(), tr.c_struct(), _lib.SDE_FORMS[diffusion_form]
        out4, out2 = (C.c_double * 4)(), (C.c_double * 2)()
        f32ok = lambda v: math.isfinite(v) and abs(v) <= 3.4028234663852886e38
        times = []

        def refuse(tv, what):
            raise ValueError(f"evaluation {len(times)} of the solve, at t = {tv:.9g}, has a non-finite coefficient ({what}): the transport "
                             "is singular there")

        for i in range(num_steps - 1):
            tv = float(ts[i])
            _lib.check(L.scldm_sde_coef_at(C.byref(trc), form, float(diffusion_norm), tv, float(dt), out4), "scldm_sde_coef_at")
            D, c_x, c_m, a_w = out4
            step = (c_x, c_m) if method == "heun" else (1.0 + float(dt) * c_x, float(dt) * c_m)
            if not all(map(f32ok, (D, a_w, *step))):
                refuse(tv, "D, c_x, c_m or sqrt(2 D dt)")
            times.append(tv)
            if method == "heun":
                t2 = float(ts[i] + dt)
                _lib.check(L.scldm_sde_coef_at(C.byref(trc), form, float(diffusion_norm), t2, float(dt), out4), "scldm_sde_coef_at")
                if not all(map(f32ok, out4[:3])):
                    refuse(t2, "D, c_x or c_m of Heun's K2")
                times.append(t2)
        t1f = float(torch.tensor(t1, dtype=torch.float32))
        if last_step is not None:
            _lib.check(L.scldm_sde_last_coef_at(C.byref(trc), form, float(diffusion_norm), _lib.SDE_LAST_STEPS[last_step], float(last_step_size), t1f,
                                                out2), "scldm_sde_last_coef_at")
            if not all(map(f32ok, out2)):
                refuse(t1f, "a_x or a_m of the last step")
            times.append(t1f)
        return ts, dt, t1, times

    def _sample_sde_transport(self, sampling_method, diffusion_form, diffusion_norm, last_step, last_step_size, num_steps):
        """sample_sde under a transport other than (Linear, velocity): the reference's expressions (transport.py:222-322, integrators.py:7-75)
        on one model call per evaluation.  SBDM's D = norm Dv is formed here (the paths' compute_diffusion does not offer it)."""
        ts, dt, t1, _ = self.sde_plan(sampling_method=sampling_method, diffusion_form=diffusion_form, diffusion_norm=diffusion_norm,
                                      last_step=last_step, last_step_size=last_step_size, num_steps=num_steps)
        method = str(sampling_method).lower()
        if last_step is None:
            last_step_size = 0.0
        path, model_type = self.transport.path_sampler, self.transport.model_type

        def diffusion(x, tv):
            if diffusion_form == "SBDM":
                return diffusion_norm * path.compute_drift(x, tv)[1]
            return path.compute_diffusion(x, tv, form=diffusion_form, norm=diffusion_norm)

        def evaluate(x, tval, model, model_kwargs):
            """(probability-flow drift, score, SDE drift) at one time, from ONE model call."""
            tv = torch.as_tensor(tval, dtype=torch.float32).to(x.device).reshape(()).expand(x.shape[0])
            m = model(x, tv, **model_kwargs)
            assert m.shape == x.shape, "Output shape from SDE solver must match input shape"
            if model_type == ModelType.VELOCITY:
                f_ode, score = m, path.get_score_from_velocity(m, x, tv)
            else:
                drift_mean, drift_var = path.compute_drift(x, tv)
                score = m / -path.compute_sigma_t(_expand_like(tv, x))[0] if model_type == ModelType.NOISE else m
                f_ode = -drift_mean + drift_var * score
            return f_ode, score, f_ode + diffusion(x, tv) * score, tv

        @torch.no_grad()
        def _sample(init, model, _draw=None, **model_kwargs):
            import contextlib
            from ..nnets import weights_unchanged
            x, xs = init, []
            with contextlib.ExitStack() as stack:
                for i in range(num_steps - 1):
                    ti = ts[i]
                    w = torch.randn(x.size()).to(x) if _draw is None else _draw(x)
                    dw = w * torch.sqrt(dt)
                    tv = ti.to(x.device).expand(x.shape[0])
                    D = diffusion(x, tv)
                    if method == "euler":
                        _, _, f, _ = evaluate(x, ti, model, model_kwargs)
                        x = x + f * dt.to(x.device) + torch.sqrt(2 * D) * dw
                    else:
                        xhat = x + torch.sqrt(2 * D) * dw
                        _, _, k1, _ = evaluate(xhat, ti, model, model_kwargs)
                        _, _, k2, _ = evaluate(xhat + dt.to(x.device) * k1, ti + dt, model, model_kwargs)
                        x = xhat + 0.5 * dt.to(x.device) * (k1 + k2)
                    if i == 0:
                        stack.enter_context(weights_unchanged())
                    xs.append(x)
                if last_step is not None:
                    f_ode, score, f, tv = evaluate(x, torch.tensor(t1, dtype=torch.float32), model, model_kwargs)
                    if last_step == "Mean":
                        x = x + f * last_step_size
                    elif last_step == "Tweedie":
                        alpha, sigma = path.compute_alpha_t(tv)[0][0], path.compute_sigma_t(tv)[0][0]
                        x = x / alpha + (sigma ** 2) / alpha * score
                    else:
                        x = x + f_ode * last_step_size
                xs.append(x)
            assert len(xs) == num_steps, "Samples does not match the number of steps"
            return xs

        return _sample

    def logp_plan(self, *, sampling_method, num_steps, row_elems=None):
        """The refusal scan of a likelihood solve under this transport: a noise / score model needs sample_eps > 0 (as sample_ode's one-call
        form refuses it), and on the fixed grids
        (a, b) of every evaluation's model time t = fp32(1 - s) must be finite (ValueError naming the evaluation and its time)."""
        import ctypes as C
        import math
        from .. import _lib
        tr = self.transport
        t_lo, t_hi = self._ode_interval()
        if tr.model_type != ModelType.VELOCITY and not tr.sample_eps > 0:
            raise ValueError("a noise / score model needs sample_eps > 0: its drift is singular at t = 0 (alpha'/alpha) and at t = 1 (noise: 1 / sigma)")
        method = str(sampling_method).lower()
        if method == "dopri5":
            return t_lo, t_hi
        ss = torch.linspace(t_lo, t_hi, num_steps)
        L, trc, k = _lib.lib(), tr.c_struct(), _lib.TransportCoef()
        n = 0
        for i in range(num_steps - 1):
            for j in range(2 if method == "heun" else 1):
                tv = float(1 - ss[i + j])
                _lib.check(L.scldm_transport_coef_at(C.byref(trc), tv, C.byref(k)), "scldm_transport_coef_at")
                if not (math.isfinite(k.a) and math.isfinite(k.b) and math.isfinite(k.a * (row_elems or 1))):
                    raise ValueError(f"evaluation {n} of the solve, at t = {tv:.9g}, has a non-finite coefficient (a, b of the probability-flow "
                                     "drift): the transport is singular there")
                n += 1
        return t_lo, t_hi

    def _sample_dopri5(self, num_steps: int, atol: float, rtol: float, first_step: float | None = None):
        """Adaptive Dormand-Prince 5(4) - what `torchdiffeq.odeint(method="dopri5")` computes for the reference's default
        `sample_ode()` (integrators.py:100-112; models.py:793).  The driver follows torchdiffeq's documented scheme step for
        step (oracle/transport.py: sample_ode_dopri5 is its float64 restatement and the checker): FSAL tableau, mixed rms error
        ratio over the whole state (all cells share one step size), accept iff ratio <= 1, next step
        dt * min(10, max(0.9 / ratio^(1/5), 0.2 - or 1 after an accepted step)), automatic initial step, steps never clipped to
        the save times (the solver steps past them, past t = 1 too) and the quartic interpolant of the last accepted step
        evaluated at the float32 `linspace(0, 1, num_steps)` save times.  PARITY UNPINNED at torchdiffeq itself (un-vendored,
        unpinned).  State arithmetic in the state's dtype on its device; times and step sizes are host float64; every step
        costs one host read of the error ratio.  `fn.last_stats` = evaluations, accepted / rejected (t0, dt) lists.
        `first_step` (None: the automatic initial step) is taken as the first attempted step size and saves that step's extra
        evaluation: two solves started from the same value can be compared step for step.  A scldm_amd DiT of the fused shape
        family runs this solve as one C call (`DiT.sample_ode_cfg(..., "dopri5")` -> scldm_sample_ode_dopri5)."""
        drift = self.drift
        t_lo, t_hi = self._ode_interval()

        @torch.no_grad()
        def _sample(x, model, **model_kwargs):
            n_eval = 0

            def f(xc, tval):
                # one scalar broadcast to (B,) as a stride-0 view: any model reads it as the reference's `ones(B) * t`
                # (integrators.py:103-104), and a scldm_amd DiT can tell without a device round trip that t is uniform
                nonlocal n_eval
                n_eval += 1
                tv = torch.full((), float(tval), device=xc.device, dtype=torch.float32).expand(xc.shape[0])
                return drift(xc, tv, model, **model_kwargs)

            def comb(base, w, ks, h):       # base + h * sum_i w_i k_i, skipping structural zeros
                for wi, k in zip(w, ks):
                    if wi != 0.0:
                        base = base + (h * wi) * k
                return base

            # Device state arithmetic (round 5): on a CUDA fp32 state the stage points, the error ratio and the dense output are four
            # HIP kernels (scldm_rk_*: csrc/ode_rk.hpp) that perform the SAME fp32 operations in the same order as the torch
            # expressions of the host-composed path below (kept for CPU tensors, i.e. the oracle-side tests): ~40 elementwise
            # launches per step -> 4, the error ratio still read back once per step.
            dev = x.is_cuda and x.dtype == torch.float32 and x.numel() % 4 == 0
            if dev:
                import ctypes as C
                import numpy as np
                from .. import _lib
                L = _lib.lib()
                x = x.contiguous()
                n_el = x.numel()
                ws = torch.zeros(1024, dtype=torch.float64, device=x.device)
                f32 = lambda v: float(np.float32(v))

                def _tab(w, ks, h):
                    pairs = [(k, f32(h * wi)) for wi, k in zip(w, ks) if wi != 0.0]
                    ptrs = (C.c_void_p * len(pairs))(*[k.data_ptr() for k, _ in pairs])
                    return ptrs, (C.c_float * len(pairs))(*[c for _, c in pairs]), len(pairs), [k for k, _ in pairs]

                def _st():
                    return C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)

                def comb(base, w, ks, h):
                    ks = [k.contiguous() for k in ks]
                    ptrs, cs, nk, keep = _tab(w, ks, h)
                    out = torch.empty_like(base)
                    with torch.cuda.device(x.device):
                        _lib.check(L.scldm_rk_combine(out.data_ptr(), base.data_ptr(), ptrs, cs, nk, n_el, _st()), "scldm_rk_combine")
                    return out

                def error_ratio(y0_, y1_, ks, h):
                    ptrs, cs, nk, keep = _tab(_DP_E, ks, h)
                    with torch.cuda.device(x.device):
                        _lib.check(L.scldm_rk_error(y0_.data_ptr(), y1_.data_ptr(), ptrs, cs, nk, n_el, atol, rtol, ws.data_ptr(), _st()), "scldm_rk_error")
                    return float(ws[1022]) ** 0.5                      # the step's one host read

                def dense_fit(y0_, y1_, ks, h):
                    ptrs, cs, nk, keep = _tab(_DP_MID, ks, h)
                    cf = [torch.empty_like(y0_) for _ in range(4)]
                    with torch.cuda.device(x.device):
                        _lib.check(L.scldm_rk_dense(y0_.data_ptr(), y1_.data_ptr(), ptrs, cs, nk, ks[0].data_ptr(), ks[6].data_ptr(), f32(h), f32(2 * h),
                                                    n_el, cf[0].data_ptr(), cf[1].data_ptr(), cf[2].data_ptr(), cf[3].data_ptr(), _st()), "scldm_rk_dense")
                    return (y0_, *cf)

                def dense_eval(coeff, s_):
                    out = torch.empty_like(coeff[0])
                    with torch.cuda.device(x.device):
                        _lib.check(L.scldm_rk_poly(out.data_ptr(), *[c.data_ptr() for c in coeff], f32(s_), f32(s_ * s_), f32(s_ * s_ * s_),
                                                   f32(s_ * s_ * s_ * s_), n_el, _st()), "scldm_rk_poly")
                    return out
            else:
                def error_ratio(y0_, y1_, ks, h):
                    err = sum((h * e) * k for e, k in zip(_DP_E, ks) if e != 0.0)
                    return _rms(err / (atol + rtol * torch.maximum(y0_.abs(), y1_.abs())))

                def dense_fit(y0_, y1_, ks, h):
                    ymid = comb(y0_, _DP_MID, ks, h)
                    fa, fb = ks[0], ks[6]
                    return (y0_, h * fa, h * (fb - 4 * fa) - 11 * y0_ - 5 * y1_ + 16 * ymid,
                            h * (5 * fa - 3 * fb) + 18 * y0_ + 14 * y1_ - 32 * ymid, 2 * h * (fb - fa) - 8 * (y1_ + y0_) + 16 * ymid)

                def dense_eval(coeff, s_):
                    total, sp = coeff[0] + s_ * coeff[1], s_
                    for cf in coeff[2:]:
                        sp = sp * s_
                        total = total + sp * cf
                    return total

            ts = [float(v) for v in torch.linspace(t_lo, t_hi, num_steps).double()]   # integrators.py:95, cast as the solver does
            y0 = x
            f0 = f(y0, ts[0])
            # (the first evaluation checked the packed weights against the parameters; no parameter changes inside a solve, so the
            # remaining ~110 evaluations skip the device-side fingerprint pass: scldm_amd.nnets.weights_unchanged)
            from ..nnets import weights_unchanged
            with weights_unchanged():
                return _solve(f, comb, error_ratio, dense_fit, dense_eval, ts, x, y0, f0, lambda: n_eval)

        def _solve(f, comb, error_ratio, dense_fit, dense_eval, ts, x, y0, f0, n_eval_now):
            dev = x.is_cuda and x.dtype == torch.float32 and x.numel() % 4 == 0
            # initial step (Hairer / Norsett / Wanner II.4, rms norm, exponent 1 / 5)
            if first_step is not None and first_step > 0:
                h = float(first_step)
            else:
                scale = atol + rtol * y0.abs()
                d0, d1 = _rms(y0 / scale), _rms(f0 / scale)
                h0 = 1e-6 if (d0 < 1e-5 or d1 < 1e-5) else 0.01 * d0 / d1
                d2 = _rms((f(y0 + h0 * f0, ts[0] + h0) - f0) / scale) / h0
                h1 = max(1e-6, h0 * 1e-3) if (d1 <= 1e-15 and d2 <= 1e-15) else (0.01 / max(d1, d2)) ** (1.0 / 5.0)
                h = min(100.0 * h0, h1)
            t0 = t1 = ts[0]
            coeff = None
            out = [x]
            accepted, rejected = [], []
            for next_t in ts[1:]:
                while next_t > t1:            # advance until the save time lies inside the last accepted step
                    if not (t1 + h > t1) or n_eval_now() > 100000:
                        raise RuntimeError("dopri5: step size underflow / too many evaluations")
                    ta = t1
                    ks = [f0]
                    for a_row, c in zip(_DP_A, _DP_C):
                        yi = comb(y0, a_row, ks, h)
                        ks.append(f(yi, ta + h if c == 1.0 else ta + c * h))
                    y1 = yi                   # the last stage point is the 5th-order solution (FSAL: ks[6] = f(ta + h, y1))
                    if dev:
                        ks = [k.contiguous() for k in ks]
                    ratio = error_ratio(y0, y1, ks, h)
                    if ratio <= 1.0:
                        accepted.append((ta, h))
                        coeff = dense_fit(y0, y1, ks, h)
                        t0, t1, y0, f0 = ta, ta + h, y1, ks[6]
                    else:
                        rejected.append((ta, h))
                    if ratio == 0.0:
                        h = h * 10.0
                    else:
                        h = h * min(10.0, max(0.9 / ratio ** 0.2, 1.0 if ratio < 1.0 else 0.2))
                out.append(dense_eval(coeff, (next_t - t0) / (t1 - t0)))
            _sample.last_stats = {"evaluations": n_eval_now(), "rejected": len(rejected), "accepted_steps": accepted, "rejected_steps": rejected}
            return torch.stack(out)

        return _sample

    def sample_sde(self, *, sampling_method="Euler", diffusion_form="SBDM", diffusion_norm=1.0, last_step="Mean", last_step_size=0.04,
                   num_steps=250):
        """Returns fn(init, model, **model_kwargs) -> list of `num_steps` states: the reference's stochastic sampler
        (transport.py:269-322, integrators.py:7-75) for the Linear path with a velocity model - Euler-Maruyama ("Euler") or stochastic
        Heun ("Heun") steps over linspace(0, 1 - last_step_size, num_steps), then a noise-free last step ("Mean", "Tweedie", "Euler"
        or None).  Signature and defaults are the reference's.  Any callable, CPU or GPU tensors; the noise is drawn as the reference
        draws it (`torch.randn(x.size()).to(x)` once per step, in order), so the same `torch.manual_seed` gives the same stream.
        One model call per evaluation (the reference makes two identical ones for drift and score), t as a stride-0 (B,) view.
        A scldm_amd DiT runs the whole solve on device through `DiT.sample_sde_cfg` instead.

        Three corners of the reference return NaN under this transport and raise here: diffusion_form="SBDM" - the DEFAULT - is
        (1 - t) / t at the t0 = 0 the solve starts from; "Heun" with last_step=None and "Mean" / "Tweedie" with last_step_size=0
        evaluate the score at t = 1."""
        if not self._default_only("sample_sde"):
            return self._sample_sde_transport(sampling_method, diffusion_form, diffusion_norm, last_step, last_step_size, num_steps)
        method = str(sampling_method).lower()
        if method not in ("euler", "heun"):
            raise NotImplementedError(f"Sampler type {sampling_method!r} not implemented: 'Euler' and 'Heun' are")
        if diffusion_form == "SBDM":
            raise ValueError("diffusion_form='SBDM' (the reference's default) is (1 - t) / t under the Linear path: infinite at the t = 0 the "
                             f"solve starts from, the reference returns NaN; choose one of {SDE_DIFFUSION_FORMS}")
        if diffusion_form not in SDE_DIFFUSION_FORMS:
            raise NotImplementedError(f"Diffusion form {diffusion_form} not implemented")
        if last_step not in SDE_LAST_STEPS:
            raise NotImplementedError(f"last_step={last_step!r}: one of {SDE_LAST_STEPS}")
        if method == "heun" and last_step is None:
            raise ValueError("sampling_method='Heun' with last_step=None evaluates the score at t = 1 in its final K2 (NaN / inf in the "
                             "reference); use last_step 'Mean', 'Tweedie' or 'Euler', or sampling_method='Euler'")
        if last_step is None:
            last_step_size = 0.0
        if num_steps < 2:
            raise ValueError("num_steps must be >= 2 (grid points)")
        if not 0.0 <= last_step_size < 1.0:
            raise ValueError(f"last_step_size must be in [0, 1), got {last_step_size}")
        if last_step in ("Mean", "Tweedie") and last_step_size == 0.0:
            raise ValueError(f"last_step={last_step!r} with last_step_size=0 evaluates the score at t = 1; give a positive last_step_size")
        path = self.transport.path_sampler
        t1 = 1 - last_step_size
        ts = torch.linspace(0, t1, num_steps)
        dt = ts[1] - ts[0]

        def evaluate(x, tval, model, model_kwargs):
            """(v, sde drift v + D score) at one time."""
            tv = torch.as_tensor(tval, dtype=torch.float32).to(x.device).reshape(()).expand(x.shape[0])
            v = model(x, tv, **model_kwargs)
            assert v.shape == x.shape, "Output shape from SDE solver must match input shape"
            D = path.compute_diffusion(x, tv, form=diffusion_form, norm=diffusion_norm)
            return v, v + D * path.get_score_from_velocity(v, x, tv), tv

        @torch.no_grad()
        def _sample(init, model, _draw=None, **model_kwargs):
            # _draw (internal): x -> the step's normals, in place of the host generator (DiT.sample_sde_cfg's per-evaluation route)
            import contextlib
            from ..nnets import weights_unchanged
            x, xs = init, []
            with contextlib.ExitStack() as stack:
                for i in range(num_steps - 1):
                    ti = ts[i]
                    w = torch.randn(x.size()).to(x) if _draw is None else _draw(x)
                    dw = w * torch.sqrt(dt)
                    tv = ti.to(x.device).expand(x.shape[0])
                    D = path.compute_diffusion(x, tv, form=diffusion_form, norm=diffusion_norm)
                    if method == "euler":
                        _, f, _ = evaluate(x, ti, model, model_kwargs)
                        x = x + f * dt.to(x.device) + torch.sqrt(2 * D) * dw
                    else:
                        xhat = x + torch.sqrt(2 * D) * dw
                        _, k1, _ = evaluate(xhat, ti, model, model_kwargs)
                        _, k2, _ = evaluate(xhat + dt.to(x.device) * k1, ti + dt, model, model_kwargs)
                        x = xhat + 0.5 * dt.to(x.device) * (k1 + k2)
                    if i == 0:    # the first evaluation checked the packed weights against the parameters: the rest of the solve skips that pass
                        stack.enter_context(weights_unchanged())
                    xs.append(x)
                if last_step is not None:
                    v, f, _ = evaluate(x, torch.tensor(t1, dtype=torch.float32), model, model_kwargs)
                    if last_step == "Mean":
                        x = x + f * last_step_size
                    elif last_step == "Tweedie":      # x / t1 + (1 - t1)^2 / t1 score  =  x + (1 - t1) v
                        x = x + (1 - t1) * v
                    else:
                        x = x + v * last_step_size
                xs.append(x)
            assert len(xs) == num_steps, "Samples does not match the number of steps"
            return xs

        return _sample

    def sample_ode_likelihood(self, *, sampling_method="dopri5", num_steps=50, atol=1e-6, rtol=1e-3, first_step=None):
        """Returns fn(x, model, **model_kwargs) -> (logp, x_end): the reference's likelihood sampler (transport.py:371-430), signature and
        defaults included.  The augmented state (x, delta_logp) is integrated over solver time s from 0 to 1 with

            d x / d s = -v,   d delta_logp / d s = eps . (d v / d x)^T eps,   v = model(x, 1 - s),

        one fresh Rademacher probe eps per evaluation (Hutchinson's estimator of the divergence: unbiased, noisy), and
        logp = prior_logp(x_end) - delta_logp.  x_end is the noise-end latent of x (the inversion).  `model` is any differentiable
        callable (x, t (n,)) -> v; the vector-Jacobian product comes from torch.autograd.grad.  The probe is drawn as the reference
        draws it (`torch.randint(2, x.size(), dtype=float, device=x.device) * 2 - 1`), or comes from `_probe=` (internal: x -> eps,
        one call per evaluation, as `_draw=` of sample_sde).  One model call per evaluation (the reference makes a second, identical one).
        "euler" / "heun" step on this project's fixed grid linspace(0, 1, num_steps) (num_steps grid points; Heun's second evaluation
        at the next grid point); "dopri5" runs the Dormand-Prince driver of sample_ode on the packed state (n, x[0].numel() + 1) - the
        reference passes one atol / rtol for both components, i.e. one mixed rms norm over the packed state (parity with torchdiffeq
        unpinned, as for sample_ode).  After a call `fn.last_trace` = {"t": [...], "logp_grad": [...]} of every evaluation, and after a
        "dopri5" solve `fn.last_stats` = the driver's evaluations and accepted / rejected (t0, dt) lists.  `first_step` ("dopri5" only;
        None: the automatic initial step) is the first attempted step size, as for `_sample_dopri5`.
        A scldm_amd DiT runs these solves on device through `DiT.log_likelihood_cfg` (fixed grid: scldm_logp_ode; "dopri5":
        scldm_logp_ode_dopri5)."""
        default = self._default_only("sample_ode_likelihood")
        method = str(sampling_method).lower()
        if method not in ("euler", "heun", "dopri5"):
            raise NotImplementedError(f"sampling_method={sampling_method!r}: 'euler', 'heun' (fixed grid) and 'dopri5' (adaptive) are provided")
        if num_steps < 2:
            raise ValueError("num_steps must be >= 2 (grid points)")
        # solver time runs over [t0, t1] = check_interval(sde=False, eval=True): (0, 1) under the default transport
        s_lo, s_hi = (0.0, 1.0) if default else self.logp_plan(sampling_method=method, num_steps=num_steps)
        drift, transport = self.drift, self.transport

        def _sample_fn(x, model, _probe=None, **model_kwargs):
            trace = {"t": [], "logp_grad": []}

            def likelihood_drift(xc, s):
                """(-v, logp_grad) at solver time s (a (n,) tensor): _likelihood_drift of the reference."""
                eps = (torch.randint(2, xc.size(), dtype=torch.float, device=xc.device) * 2 - 1).to(xc.dtype) if _probe is None else _probe(xc)
                t = torch.ones_like(s) * (1 - s)
                with torch.enable_grad():
                    xr = xc.detach().requires_grad_(True)
                    v = drift(xr, t, model, **model_kwargs)
                    grad = torch.autograd.grad(torch.sum(v * eps), xr)[0]
                lg = torch.sum(grad * eps, dim=tuple(range(1, xc.dim())))
                trace["t"].append(t.detach())
                trace["logp_grad"].append(lg.detach())
                return -v.detach(), lg.detach()

            def at(xc, tval):   # one scalar broadcast to (n,) as a stride-0 view (see sample_ode)
                return likelihood_drift(xc, torch.full((), float(tval), device=xc.device, dtype=torch.float32).expand(xc.shape[0]))

            x = x.detach()
            dl = torch.zeros(x.size(0)).to(x)
            if method == "dopri5":
                n, shape = x.shape[0], x.shape

                def packed(y, s):
                    dxv, lg = likelihood_drift(y[:, :-1].reshape(shape), s)
                    return torch.cat([dxv.reshape(n, -1), lg.reshape(n, 1).to(dxv.dtype)], dim=1)

                solve = Sampler(transport)._sample_dopri5(num_steps, atol, rtol, first_step)
                y = solve(torch.cat([x.reshape(n, -1), dl.reshape(n, 1)], dim=1), packed)[-1]
                _sample_fn.last_stats = solve.last_stats
                x, dl = y[:, :-1].reshape(shape), y[:, -1]
            else:
                ts = torch.linspace(s_lo, s_hi, num_steps)
                with torch.no_grad():
                    for i in range(num_steps - 1):
                        h = float(ts[i + 1] - ts[i])
                        k1x, k1l = at(x, ts[i])
                        if method == "euler":
                            x, dl = x + h * k1x, dl + h * k1l
                        else:
                            k2x, k2l = at(x + h * k1x, ts[i + 1])
                            x, dl = x + (0.5 * h) * (k1x + k2x), dl + (0.5 * h) * (k1l + k2l)
            _sample_fn.last_trace = trace
            return transport.prior_logp(x) - dl, x

        return _sample_fn

    def sample_ode(self, *, sampling_method="dopri5", num_steps=50, atol=1e-5, rtol=1e-5, reverse=False):
        """Returns fn(x, model, **model_kwargs) -> (num_steps, *x.shape) trajectory; callers take [-1] (models.py:812).
        The transport's drift is integrated over linspace(t0, t1, num_steps), (t0, t1) = (0, 1) for a velocity model and
        (sample_eps, 1 - sample_eps) for a noise / score model (transport.py:324-369); host-driven, any callable.

        `num_steps` grid points = num_steps-1 steps (integrators.py:95).  The model sees t broadcast to a (B,)
        vector (integrators.py:103-104) - here as a stride-0 view of one device scalar, which a scldm_amd DiT
        recognises as uniform and shares the conditioning work across the batch.
        """
        method = sampling_method.lower()
        if method not in ("euler", "heun", "dopri5"):
            raise NotImplementedError(f"sampling_method={sampling_method!r}: 'euler', 'heun' (fixed grid) and 'dopri5' (adaptive) are provided")
        if reverse:
            raise NotImplementedError("reverse-time ODE has no caller in the reference")
        if method == "dopri5":
            return self._sample_dopri5(num_steps, atol, rtol)
        drift = self.drift
        t_lo, t_hi = self._ode_interval()

        @torch.no_grad()
        def _sample(x, model, **model_kwargs):
            ts = torch.linspace(t_lo, t_hi, num_steps)
            traj = [x]

            def f(xc, tval):
                # one scalar broadcast to (B,) as a stride-0 view: any model reads it as the reference's `ones(B) * t`
                # (integrators.py:103-104), and a scldm_amd DiT can tell without a device round trip that t is uniform
                tv = torch.full((), float(tval), device=xc.device, dtype=torch.float32).expand(xc.shape[0])
                return drift(xc, tv, model, **model_kwargs)

            from ..nnets import weights_unchanged
            import contextlib
            with contextlib.ExitStack() as stack:
                for i in range(num_steps - 1):
                    h = float(ts[i + 1] - ts[i])
                    k1 = f(x, ts[i])
                    if i == 0:    # the first evaluation checked the packed weights against the parameters: the rest of the loop skips that pass
                        stack.enter_context(weights_unchanged())
                    if method == "euler":
                        x = x + h * k1
                    else:
                        k2 = f(x + h * k1, ts[i + 1])
                        x = x + (0.5 * h) * (k1 + k2)
                    traj.append(x)
            return torch.stack(traj)

        return _sample

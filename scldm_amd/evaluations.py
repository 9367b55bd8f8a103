"""Generation-evaluation MMD metrics - drop-in for the classes of `scldm.evaluations` (src/scldm/evaluations.py:10-82;
SURVEY.md section 8f row N4).  Same class names, constructor arguments and call signatures: `kernel(x, y)` returns the
(Bx, By) kernel matrix, `MMDLoss(kernel)(x, y)` = mean k(x,x) + mean k(y,y) - 2 mean k(x,y).

The reference kernels broadcast to (Bx, By, D) tensors (for count matrices that is Bx*By*G floats per term); here one
fused HIP kernel per term streams D through LDS and keeps the pair accumulators in registers (scldm_mmd_kernel_sum);
MMDLoss never materialises a kernel matrix.  No CPU fallback.  `wasserstein(..., method="sinkhorn")` - the only form the
reference calls (models.py:47-48) - runs the Sinkhorn-Knopp iteration on device (scldm_wasserstein_sinkhorn); the exact
`emd` network-simplex solver of third-party POT is not provided.

The regression metrics of the same two call sites - `REGRESSION_METRICS` (mse, pcc) and zeros accuracy of `VAE.shared_step`
(models.py:315-331), `R2_METRICS` of `LatentDiffusion.on_validation_epoch_end` (models.py:892-928) - and the log1p
normalisation in front of them are one fused, bit-reproducible streaming pass (`count_metrics`, scldm_eval_count_metrics;
`normalize_log1p`, scldm_log1p_normalize).  torchmetrics is not needed.
"""
from __future__ import annotations

import ctypes as C
import math
import warnings
from functools import partial

import torch
from torch import nn

from . import _lib

_KIND = {"rbf": 0, "braycurtis": 1, "tanimoto": 2, "ruzicka": 3}


def _pair_sum(x: torch.Tensor, y: torch.Tensor, kind: int, scale: float, want_matrix: bool):
    if x.device.type != "cuda" or y.device != x.device:
        raise RuntimeError("scldm_amd.evaluations works on CUDA (ROCm) tensors; there is no CPU path")
    if x.dim() != 2 or y.dim() != 2 or x.shape[1] != y.shape[1]:
        raise ValueError(f"expected x (Bx,D) and y (By,D), got {tuple(x.shape)} and {tuple(y.shape)}")
    x, y = x.float().contiguous(), y.float().contiguous()
    nx, ny, D = x.shape[0], y.shape[0], x.shape[1]
    L = _lib.lib()
    ws = torch.empty(max(L.scldm_mmd_workspace_bytes(nx, ny), 256), dtype=torch.uint8, device=x.device)
    out = torch.empty(1, dtype=torch.float64, device=x.device)
    kmat = torch.empty((nx, ny), dtype=torch.float32, device=x.device) if want_matrix else None
    with torch.cuda.device(x.device):
        _lib.check(L.scldm_mmd_kernel_sum(x.data_ptr(), nx, y.data_ptr(), ny, D, kind, float(scale), out.data_ptr(),
                                          kmat.data_ptr() if kmat is not None else None, ws.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream), "scldm_mmd_kernel_sum")
    return out, kmat


class _PairKernel(nn.Module):
    kind = -1
    scale = 1.0

    def forward(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        return _pair_sum(x, y, self.kind, self.scale, True)[1]

    def mean(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """mean_ij k(x_i, y_j) as a 0-d fp32 tensor, without the matrix."""
        return (_pair_sum(x, y, self.kind, self.scale, False)[0][0] / (x.shape[0] * y.shape[0])).float()


class RBFKernel(_PairKernel):
    kind = _KIND["rbf"]

    def __init__(self, scale: float = 1.0):
        super().__init__()
        self.scale = scale


class BrayCurtisKernel(_PairKernel):
    kind = _KIND["braycurtis"]


class TanimotoKernel(_PairKernel):
    kind = _KIND["tanimoto"]


class RuzickaKernel(_PairKernel):
    kind = _KIND["ruzicka"]


class MMDLoss(nn.Module):
    def __init__(self, kernel):
        super().__init__()
        self.kernel = kernel

    def forward(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        k = self.kernel
        if isinstance(k, _PairKernel):
            return k.mean(x, x) + k.mean(y, y) - 2 * k.mean(x, y)
        return k(x, x).mean() + k(y, y).mean() - 2 * k(x, y).mean()   # any other callable kernel, as in the reference


def wasserstein(x0: torch.Tensor, x1: torch.Tensor, method: str | None = "emd", reg: float = 0.05, power: int = 2,
                num_iter_max: int = int(1e7), stop_thr: float = 1e-9) -> float:
    """Drop-in for `scldm.evaluations.wasserstein` (src/scldm/evaluations.py:85-108): uniform marginals, M = cdist(x0, x1) ** power,
    entropic OT by Sinkhorn-Knopp scaling as POT's `ot.sinkhorn2(a, b, M, reg, numItermax=1e7)` iterates it, sqrt for power 2.
    Cost matrix, Gibbs kernel and both matrix-vector sweeps per iteration are HIP kernels; the host only reads the marginal
    error every 10th iteration (POT's schedule).  `method="emd"` (exact network simplex, third-party POT C++) is not built:
    the reference only binds "sinkhorn" (models.py:47-48).  PARITY UNPINNED (POT is not vendored) - see oracle/evaluations.py."""
    assert power == 1 or power == 2
    if method == "emd" or method is None:
        raise NotImplementedError("wasserstein(method='emd') needs POT's exact network-simplex solver, which is not part of the MI355X "
                                  "path; the reference's metrics use method='sinkhorn' (src/scldm/models.py:47-48)")
    if method != "sinkhorn":
        raise ValueError(f"Unknown method: {method}")
    if x0.device.type != "cuda" or x1.device != x0.device:
        raise RuntimeError("scldm_amd.evaluations works on CUDA (ROCm) tensors; there is no CPU path")
    if x0.dim() != 2 or x1.dim() != 2 or x0.shape[1] != x1.shape[1]:
        raise ValueError(f"expected x0 (n,D) and x1 (m,D), got {tuple(x0.shape)} and {tuple(x1.shape)}")
    x0, x1 = x0.float().contiguous(), x1.float().contiguous()
    n, m, D = x0.shape[0], x1.shape[0], x0.shape[1]
    L = _lib.lib()
    ws = torch.empty(L.scldm_sinkhorn_workspace_bytes(n, m), dtype=torch.uint8, device=x0.device)
    cost, iters, status = C.c_double(), C.c_longlong(), C.c_int()
    with torch.cuda.device(x0.device):
        _lib.check(L.scldm_wasserstein_sinkhorn(x0.data_ptr(), n, x1.data_ptr(), m, D, power, float(reg), int(num_iter_max), float(stop_thr),
                                                C.byref(cost), C.byref(iters), C.byref(status), ws.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream), "scldm_wasserstein_sinkhorn")
    wasserstein.last_stats = {"iterations": iters.value, "status": status.value}
    if status.value == 2:   # POT warns here too ("numerical errors ... try a larger reg") and returns the last good scalings
        warnings.warn("Sinkhorn: a scaling vector became zero or non-finite (reg too small for this cost scale); "
                      "returning the transport cost of the last good iterate", RuntimeWarning)
    ret = cost.value
    if power == 2:
        ret = math.sqrt(ret) if ret >= 0 else float("nan")
    return ret


# ---- regression / r2 metrics of the validation step and the generation evaluation -----------------------------------------
_EVAL_MSE, _EVAL_PCC, _EVAL_ZEROS, _EVAL_R2_MEAN, _EVAL_R2_VAR, _EVAL_PCC_VALID, _EVAL_N = range(7)   # SCLDM_EVAL_* (scldm_hip.h)


def _check_matrix(name: str, x: torch.Tensor, like: torch.Tensor | None = None) -> None:
    if not isinstance(x, torch.Tensor) or x.device.type != "cuda" or (like is not None and x.device != like.device):
        raise RuntimeError("scldm_amd.evaluations works on CUDA (ROCm) tensors; there is no CPU path")
    if x.dim() != 2 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError(f"{name} must be a contiguous fp32 matrix (cells, genes), got {x.dtype} {tuple(x.shape)} "
                         f"contiguous={x.is_contiguous()}")
    if x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"{name} needs at least one cell and one gene, got {tuple(x.shape)}")
    if like is not None and x.shape[1] != like.shape[1]:
        raise ValueError(f"gene counts differ: {tuple(like.shape)} and {tuple(x.shape)}")


def _divisor(name: str, d: torch.Tensor | None, x: torch.Tensor) -> torch.Tensor | None:
    """Per-row divisor as a contiguous fp32 (n,) vector on x's device; (n,) and (n, 1) are accepted."""
    if d is None:
        return None
    if not isinstance(d, torch.Tensor) or d.device != x.device:
        raise RuntimeError("scldm_amd.evaluations works on CUDA (ROCm) tensors; there is no CPU path")
    if d.numel() != x.shape[0] or d.dim() > 2:
        raise ValueError(f"{name} must hold one divisor per row ({x.shape[0]}), got {tuple(d.shape)}")
    return d.reshape(-1).float().contiguous()


def normalize_log1p(counts: torch.Tensor, library_size: torch.Tensor | None = None, target_sum: float = 1e4) -> torch.Tensor:
    """log1p(counts / library_size * target_sum) as one HIP pass; library_size None: the row's own sum (models.py:321-322),
    a (N,) or (N, 1) vector: models.py:899-900.  target_sum <= 0 returns a copy."""
    _check_matrix("counts", counts)
    div = _divisor("library_size", library_size, counts)
    out = torch.empty_like(counts)
    with torch.cuda.device(counts.device):
        _lib.check(_lib.lib().scldm_log1p_normalize(counts.data_ptr(), counts.shape[0], counts.shape[1], div.data_ptr() if div is not None else None,
                                                    float(target_sum), out.data_ptr(), torch.cuda.current_stream().cuda_stream),
                   "scldm_log1p_normalize")
    return out


def count_metrics(pred: torch.Tensor, true: torch.Tensor, pred_size: torch.Tensor | None = None, true_size: torch.Tensor | None = None,
                  target_sum: float = 1e4, per_gene: bool = False) -> dict:
    """mse, pcc (nanmean of the per-gene Pearson correlation), zeros_accuracy, r2_mean and r2_var of
    U = log1p(pred / pred_size * target_sum) against V = log1p(true / true_size * target_sum) in one fused pass
    (a size of None is the row's own sum; target_sum <= 0: the inputs are already scaled).  r2 takes pred's per-gene statistic
    as `preds` and true's as `target`.  Returns 0-dim float64 device tensors (views of one buffer; nothing synchronises), plus
    `pcc_valid_genes`; per_gene=True adds `pcc_per_gene`, `mean_pred`, `var_pred`, `mean_true`, `var_true` (fp32, (G,)).
    pred and true may have different row counts: then only r2_mean / r2_var are defined and the paired metrics are NaN."""
    _check_matrix("pred", pred)
    _check_matrix("true", true, pred)
    raw = not target_sum > 0
    dp = None if raw else _divisor("pred_size", pred_size, pred)
    dt = None if raw else _divisor("true_size", true_size, true)
    n_pred, n_true, G = pred.shape[0], true.shape[0], pred.shape[1]
    L = _lib.lib()
    ws = torch.empty(L.scldm_eval_workspace_bytes(n_pred, n_true, G), dtype=torch.uint8, device=pred.device)
    out = torch.empty(_EVAL_N, dtype=torch.float64, device=pred.device)
    pcc = torch.empty(G, dtype=torch.float32, device=pred.device) if per_gene else None
    stats = torch.empty((4, G), dtype=torch.float32, device=pred.device) if per_gene else None
    with torch.cuda.device(pred.device):
        _lib.check(L.scldm_eval_count_metrics(pred.data_ptr(), n_pred, true.data_ptr(), n_true, G, dp.data_ptr() if dp is not None else None,
                                              dt.data_ptr() if dt is not None else None, float(target_sum), out.data_ptr(),
                                              pcc.data_ptr() if per_gene else None, stats.data_ptr() if per_gene else None, ws.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream), "scldm_eval_count_metrics")
    res = {"mse": out[_EVAL_MSE], "pcc": out[_EVAL_PCC], "zeros_accuracy": out[_EVAL_ZEROS], "r2_mean": out[_EVAL_R2_MEAN],
           "r2_var": out[_EVAL_R2_VAR], "pcc_valid_genes": out[_EVAL_PCC_VALID]}
    if per_gene:
        res.update(pcc_per_gene=pcc, mean_pred=stats[0], var_pred=stats[1], mean_true=stats[2], var_true=stats[3])
    return res


def _scaled_metric(key: str):
    def fn(preds: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        return count_metrics(preds, target, target_sum=0.0)[key]
    fn.__name__ = key
    return fn


# The reference's metric dictionaries (models.py:32-37 and :52-55): same keys, callables fn(preds, target) on already-scaled
# matrices, so a caller's `for k, fn in self.metric_fns.items(): fn(pred_scaled, true_scaled)` loop keeps working.  Each call
# is one fused pass; `pcc` is already the nanmean over genes (the caller's torch.nanmean of a 0-dim tensor is the identity).
REGRESSION_METRICS = {"mse": _scaled_metric("mse"), "pcc": _scaled_metric("pcc")}
R2_METRICS = {"r2_mean": _scaled_metric("r2_mean"), "r2_var": _scaled_metric("r2_var")}

MMD_METRICS = {"mmd_braycurtis_counts": MMDLoss(kernel=BrayCurtisKernel()), "mmd_tanimoto": MMDLoss(kernel=TanimotoKernel()),
               "mmd_ruzicka_counts": MMDLoss(kernel=RuzickaKernel()), "mmd_rbf": MMDLoss(kernel=RBFKernel())}   # models.py:39-44
WASSERSTEIN_METRICS = {"wasserstein1_sinkhorn": partial(wasserstein, method="sinkhorn", power=1),
                       "wasserstein2_sinkhorn": partial(wasserstein, method="sinkhorn", power=2)}   # models.py:46-49


def reconstruction_metrics(counts_pred: torch.Tensor, counts: torch.Tensor, head: str = "nb") -> dict:
    """The metric block of `VAE.shared_step` (models.py:315-331); returns mse, pcc, zeros_accuracy.  head="nb": `counts_pred` are
    drawn counts and both matrices are scaled by their own row sums.  head="gaussian": `counts_pred` is the head's mu, used as it
    is (models.py:316-318) - only the true counts are scaled."""
    if head == "gaussian":
        m = count_metrics(counts_pred, normalize_log1p(counts), target_sum=0.0)
    elif head == "nb":
        m = count_metrics(counts_pred, counts)
    else:
        raise ValueError(f"head must be 'nb' or 'gaussian', got {head!r}")
    return {k: m[k] for k in ("mse", "pcc", "zeros_accuracy")}


def generation_metrics(counts: torch.Tensor, counts_generated: torch.Tensor, library_size: torch.Tensor, mmd: bool = True,
                       wasserstein: bool = True) -> dict:
    """The metric block of `LatentDiffusion.on_validation_epoch_end` (models.py:899-928): both matrices are scaled by the TRUE
    library size; r2_mean / r2_var are called as the reference calls them, fn(counts_true_scaled, counts_generated_scaled), i.e.
    with the true cells as `preds`.  mmd / wasserstein add the four MMDs (the "counts" ones on the scaled matrices, the others on
    the raw counts, models.py:902-906) and the two Sinkhorn distances (scaled matrices; these synchronise, see `wasserstein`);
    `total_samples` is the row count the reference logs beside them (models.py:930)."""
    _check_matrix("counts", counts)
    _check_matrix("counts_generated", counts_generated, counts)
    if counts_generated.shape[0] != counts.shape[0]:
        raise ValueError(f"counts {tuple(counts.shape)} and counts_generated {tuple(counts_generated.shape)} must pair row by row "
                         "(both are divided by the true library size)")
    m = count_metrics(counts, counts_generated, pred_size=library_size, true_size=library_size)
    res = {"r2_mean": m["r2_mean"], "r2_var": m["r2_var"]}
    if mmd or wasserstein:
        true_scaled, gen_scaled = normalize_log1p(counts, library_size), normalize_log1p(counts_generated, library_size)
        if mmd:
            for k, fn in MMD_METRICS.items():
                res[k] = fn(true_scaled, gen_scaled) if "counts" in k else fn(counts, counts_generated)
        if wasserstein:
            for k, fn in WASSERSTEIN_METRICS.items():
                res[k] = fn(true_scaled, gen_scaled)
    res["total_samples"] = counts.shape[0]   # models.py:930
    return res

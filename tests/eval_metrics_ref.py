"""Float64 numpy definitions of the evaluation metrics and the test-input recipe.  TEST INFRASTRUCTURE ONLY (a helper module the
tests import).

The definitions restate the reference's call sites (src/scldm/models.py:315-331 and :892-928) with the documented torchmetrics
formulas written out (torchmetrics itself is not importable beside this project):

    U = log1p(P / dP * target_sum),  V = log1p(T / dT * target_sum)         dP, dT: the row's own sum or a supplied vector;
                                                                            target_sum <= 0: U = P, V = T
    mse             mean over all entries of (U - V)^2
    pcc             per gene cov / sqrt(var_u var_v) over the cells, clamped to [-1, 1], NaN where a variance is 0 or N < 2;
                    the scalar is the mean over the genes that are not NaN (NaN if there is none)
    zeros_accuracy  mean of ((P == 0) == (T == 0)) on the untransformed inputs
    r2_mean         r2(U.mean(0), V.mean(0)),  r2(preds, target) = 1 - sum (target - preds)^2 / sum (target - mean(target))^2
    r2_var          the same on the unbiased per-gene variances; NaN for N < 2

A zero divisor gives the NaN / inf of the expression itself.  With different row counts only r2_mean / r2_var are defined; the
paired metrics are NaN.

tests/test_eval_metrics_cpu.py holds these definitions against scipy and scikit-learn.
"""
from __future__ import annotations

import numpy as np

CASES = [(300, 1000, 1), (257, 515, 2), (65, 1001, 5), (1030, 333, 4)]   # (N, G, seed): no extent is a multiple of a tile or row block
TOL = 1e-4           # the project's fp32 gate (tests/test_mmd.py, tests/test_gpu_vae_train.py)
MAX_NAN_SHARE = 0.05  # a condition on the inputs: nanmean must not be able to hide a kernel that returns NaN where it should not
SCALARS = ("mse", "pcc", "zeros_accuracy", "r2_mean", "r2_var")
PER_GENE = ("pcc_per_gene", "mean_pred", "var_pred", "mean_true", "var_true")


def make_counts(N: int, G: int, seed: int):
    """(pred, true) fp32 count matrices with correlated genes (plain Poisson pairs have a correlation near 0, which tests nothing):
    gene rates x 8 cell programs, `pred` a binomial thinning of `true` plus independent noise.  The first 3 genes of `true` and the
    next 3 of `pred` are all zero (zero variance: NaN correlations the nanmean must skip); the last gene is >= 1, so no row is empty."""
    rng = np.random.default_rng(seed)
    rate = rng.lognormal(-1, 1.5, G)
    prog = rng.lognormal(0, 0.8, (N, 8)) @ rng.dirichlet(0.3 * np.ones(8), G).T
    lam = rate * prog
    true = rng.poisson(lam)
    pred = rng.binomial(true, 0.7) + rng.poisson(0.3 * lam)
    true[:, :3] = 0
    pred[:, 3:6] = 0
    true[:, -1] += 1
    pred[:, -1] += 1
    return pred.astype(np.float32), true.astype(np.float32)


def scale(x, div=None, target_sum: float = 1e4):
    x = np.asarray(x, dtype=np.float64)
    if not target_sum > 0:
        return x
    d = x.sum(1, keepdims=True) if div is None else np.asarray(div, dtype=np.float64).reshape(-1, 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log1p(x / d * target_sum)


def r2(preds, target) -> float:
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(1.0 - np.sum((target - preds) ** 2) / np.sum((target - target.mean()) ** 2))


def _var(x):
    n = x.shape[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.sum((x - x.mean(0)) ** 2, axis=0) / (n - 1) if n >= 2 else np.full(x.shape[1], np.nan)


def pearson_per_gene(U, V):
    n = U.shape[0]
    if n < 2:
        return np.full(U.shape[1], np.nan)
    with np.errstate(divide="ignore", invalid="ignore"):
        du, dv = U - U.mean(0), V - V.mean(0)
        su, sv, c = np.sum(du * du, 0), np.sum(dv * dv, 0), np.sum(du * dv, 0)
        r = np.clip(c / (np.sqrt(su) * np.sqrt(sv)), -1.0, 1.0)
    r[~((su > 0) & (sv > 0))] = np.nan
    return r


def count_metrics(pred, true, pred_div=None, true_div=None, target_sum: float = 1e4) -> dict:
    """The float64 reference of scldm_amd.evaluations.count_metrics(..., per_gene=True)."""
    pred, true = np.asarray(pred, dtype=np.float64), np.asarray(true, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        U, V = scale(pred, pred_div, target_sum), scale(true, true_div, target_sum)
        mean_p, mean_t, var_p, var_t = U.mean(0), V.mean(0), _var(U), _var(V)
        out = {"mean_pred": mean_p, "var_pred": var_p, "mean_true": mean_t, "var_true": var_t,
               "r2_mean": r2(mean_p, mean_t), "r2_var": r2(var_p, var_t)}
        if pred.shape[0] == true.shape[0]:
            pcc = pearson_per_gene(U, V)
            ok = ~np.isnan(pcc)
            out.update(mse=float(np.mean((U - V) ** 2)), pcc_per_gene=pcc, pcc=float(pcc[ok].mean()) if ok.any() else float("nan"),
                       zeros_accuracy=float(np.mean((pred == 0) == (true == 0))))
        else:
            out.update(mse=float("nan"), pcc_per_gene=np.full(pred.shape[1], np.nan), pcc=float("nan"), zeros_accuracy=float("nan"))
    return out


def scalar_close(got: float, ref: float, tol: float = TOL) -> bool:
    """|got - ref| <= tol * max(1, |ref|); NaN matches NaN only, an infinity matches the same infinity only."""
    if np.isnan(ref) or np.isnan(got):
        return bool(np.isnan(ref) and np.isnan(got))
    if np.isinf(ref) or np.isinf(got):
        return bool(got == ref)
    return bool(abs(got - ref) <= tol * max(1.0, abs(ref)))

"""The fused evaluation metrics (scldm_amd.evaluations.count_metrics / normalize_log1p and the blocks built on them) against the
float64 definitions of tests/eval_metrics_ref.py.  Gate: 1e-4, the project's fp32 gate - every scalar within
1e-4 * max(1, |reference|), per-gene vectors within 1e-4 scale-relative, the NaN pattern of the per-gene correlation EQUAL.
(fp32 Welford moments in row blocks with a float64 merge sit two to three orders below the gate; a wrong merge or a one-pass
sum-of-squares variance does not pass it.)"""
import functools
import warnings

import numpy as np
import pytest
import torch

import eval_metrics_ref as ref
from conftest import max_abs_rel

pytestmark = pytest.mark.gpu
TOL = ref.TOL


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def inputs(N, G, seed):
    """(pred, true) of the recipe and their float64 metrics for own-row-sum scaling and for the shared divisor true.sum(1):
    computed once, shared by the tests, never modified."""
    pred, true = ref.make_counts(N, G, seed)
    d = true.sum(1)
    return pred, true, {"own": ref.count_metrics(pred, true), "shared": ref.count_metrics(pred, true, d, d)}


def bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    """torch.equal on the bit patterns (NaN compares equal to the same NaN)."""
    as_int = {torch.float32: torch.int32, torch.float64: torch.int64}[a.dtype]
    return a.dtype == b.dtype and torch.equal(a.contiguous().view(as_int), b.contiguous().view(as_int))


def check_scalars(got: dict, want: dict, what: str, keys=ref.SCALARS):
    for k in keys:
        g, w = float(got[k]), float(want[k])
        print(f"[eval] {what} {k}: got {g:.9g} ref {w:.9g} |diff| {abs(g - w):.3e}")
    for k in keys:
        assert ref.scalar_close(float(got[k]), float(want[k]), TOL), (what, k, float(got[k]), float(want[k]))


def check_per_gene(got: dict, want: dict, what: str):
    pg, pw = got["pcc_per_gene"].cpu().numpy(), want["pcc_per_gene"]
    assert np.array_equal(np.isnan(pg), np.isnan(pw)), (what, "NaN pattern of pcc_per_gene",
                                                        np.flatnonzero(np.isnan(pg) != np.isnan(pw))[:10])
    assert int(got["pcc_valid_genes"]) == int((~np.isnan(pw)).sum())
    ok = ~np.isnan(pw)
    if ok.any():
        e = max_abs_rel(pg[ok], pw[ok])
        print(f"[eval] {what} pcc_per_gene: {e:.3e}")
        assert e < TOL, (what, "pcc_per_gene", e)
    for k in ("mean_pred", "var_pred", "mean_true", "var_true"):
        g, w = got[k].cpu().numpy(), want[k]
        assert np.array_equal(np.isnan(g), np.isnan(w)), (what, k)
        if not np.isnan(w).all() and np.abs(w[~np.isnan(w)]).max() > 0:
            e = max_abs_rel(g[~np.isnan(w)], w[~np.isnan(w)])
            print(f"[eval] {what} {k}: {e:.3e}")
            assert e < TOL, (what, k, e)


@pytest.mark.parametrize("N,G,seed", ref.CASES)
@pytest.mark.parametrize("divisor", ["own", "shared"])
def test_parity_at_ragged_sizes(N, G, seed, divisor):
    from scldm_amd.evaluations import count_metrics
    pred, true, want = inputs(N, G, seed)
    assert np.isnan(want[divisor]["pcc_per_gene"]).mean() <= ref.MAX_NAN_SHARE
    d = cu(true.sum(1)) if divisor == "shared" else None
    got = count_metrics(cu(pred), cu(true), pred_size=d, true_size=d, per_gene=True)
    assert all(got[k].dim() == 0 and got[k].is_cuda for k in ref.SCALARS)
    check_scalars(got, want[divisor], f"N={N} G={G} {divisor}")
    check_per_gene(got, want[divisor], f"N={N} G={G} {divisor}")


@pytest.mark.parametrize("N,G", [(1, 70), (3, 70), (2, 1), (64, 257)])
def test_edge_shapes(N, G):
    from scldm_amd.evaluations import count_metrics
    pred, true, want = inputs(N, G, 9)
    got = count_metrics(cu(pred), cu(true), per_gene=True)
    if N == 1:
        assert np.isnan(float(got["pcc"])) and np.isnan(float(got["r2_var"]))
        assert np.isfinite([float(got[k]) for k in ("mse", "zeros_accuracy", "r2_mean")]).all()
    check_scalars(got, want["own"], f"edge N={N} G={G}")
    check_per_gene(got, want["own"], f"edge N={N} G={G}")


def test_zero_divisor_gives_nan():
    """One row's divisor 0: 0 / 0 = NaN and x / 0 = inf in that row, as the reference's expression gives; the NaN reaches every
    metric that reads the scaled matrices.  (zeros_accuracy reads the untransformed counts: no divisor enters it, and it stays the
    reference's finite value.)"""
    from scldm_amd.evaluations import count_metrics
    pred, true, _ = inputs(300, 1000, 1)
    d = true.sum(1)
    d[17] = 0
    want = ref.count_metrics(pred, true, d, d)
    got = count_metrics(cu(pred), cu(true), pred_size=cu(d), true_size=cu(d), per_gene=True)
    for k in ("mse", "pcc", "r2_mean", "r2_var"):
        assert np.isnan(want[k]) and np.isnan(float(got[k])), k
    assert int(got["pcc_valid_genes"]) == 0 and bool(torch.isnan(got["pcc_per_gene"]).all())
    check_scalars(got, want, "zero divisor")
    # an all-zero row under own-row-sum scaling is the same 0 / 0
    p0 = pred.copy()
    p0[5] = 0
    got = count_metrics(cu(p0), cu(true))
    check_scalars(got, ref.count_metrics(p0, true), "empty row")
    assert np.isnan(float(got["mse"])) and np.isnan(float(got["pcc"]))


def test_unpaired_rows():
    from scldm_amd.evaluations import count_metrics
    pred, true, _ = inputs(300, 515, 3)
    pred = pred[:200]
    want = ref.count_metrics(pred, true)
    got = count_metrics(cu(pred), cu(true), per_gene=True)
    assert all(np.isnan(float(got[k])) for k in ("mse", "pcc", "zeros_accuracy")) and np.isfinite(want["r2_mean"])
    check_scalars(got, want, "n_pred=200 n_true=300")
    check_per_gene(got, want, "n_pred=200 n_true=300")


def test_already_scaled_inputs_and_normalize():
    from scldm_amd.evaluations import R2_METRICS, REGRESSION_METRICS, count_metrics, normalize_log1p
    pred, true, want = inputs(257, 515, 2)
    P, T = cu(pred), cu(true)
    U, V = normalize_log1p(P), normalize_log1p(T)
    for x, y in ((P, U), (T, V)):
        assert max_abs_rel(y.cpu(), torch.log1p(x / x.sum(1, keepdim=True) * 1e4).cpu()) < 1e-6
    d = cu(true.sum(1))
    for lib in (d, d.view(-1, 1)):
        assert max_abs_rel(normalize_log1p(P, lib).cpu(), torch.log1p(P / d.view(-1, 1) * 1e4).cpu()) < 1e-6
    assert torch.equal(normalize_log1p(U, target_sum=0.0), U)
    raw = count_metrics(P, T)
    got = {"pcc": REGRESSION_METRICS["pcc"](U, V), "mse": REGRESSION_METRICS["mse"](U, V), "r2_mean": R2_METRICS["r2_mean"](U, V),
           "r2_var": R2_METRICS["r2_var"](U, V)}
    check_scalars(got, {k: float(v) for k, v in raw.items()}, "scaled vs raw", keys=tuple(got))
    check_scalars(got, want["own"], "scaled vs reference", keys=tuple(got))
    assert float(torch.nanmean(got["pcc"])) == float(got["pcc"])       # the caller's torch.nanmean (models.py:331) is the identity


def test_evaluation_size_and_bit_reproducibility():
    """1 024 cells x 17 002 genes drawn on the device; the reference's own expressions evaluated by torch in float64 on the device."""
    from scldm_amd.evaluations import count_metrics
    gen = torch.Generator(device="cuda").manual_seed(11)
    N, G = 1024, 17002
    lam = torch.exp(torch.randn(G, device="cuda", generator=gen) * 1.2 - 1.0) * torch.exp(torch.randn((N, 1), device="cuda", generator=gen) * 0.5)
    true = torch.poisson(lam, generator=gen).float()
    pred = (torch.poisson(0.7 * true + 0.3 * lam, generator=gen) * (torch.rand((N, G), device="cuda", generator=gen) < 0.9)).float()
    true[:, -1] += 1
    pred[:, -1] += 1
    got = count_metrics(pred, true, per_gene=True)
    again = count_metrics(pred, true, per_gene=True)
    for k in ref.SCALARS + ("pcc_valid_genes",) + ref.PER_GENE:
        assert bits_equal(got[k], again[k]), k
    p, t = pred.double(), true.double()
    U = torch.log1p(p / p.sum(1, keepdim=True) * 10_000)
    V = torch.log1p(t / t.sum(1, keepdim=True) * 10_000)
    du, dv = U - U.mean(0), V - V.mean(0)
    su, sv = (du * du).sum(0), (dv * dv).sum(0)
    pcc = ((du * dv).sum(0) / (su.sqrt() * sv.sqrt())).clamp(-1, 1)
    pcc[~((su > 0) & (sv > 0))] = float("nan")

    def r2(preds, target):
        return 1 - ((target - preds) ** 2).sum() / ((target - target.mean()) ** 2).sum()

    want = {"mse": ((U - V) ** 2).mean(), "pcc": torch.nanmean(pcc), "zeros_accuracy": ((p == 0) == (t == 0)).double().mean(),
            "r2_mean": r2(U.mean(0), V.mean(0)), "r2_var": r2(U.var(0), V.var(0))}
    assert float(torch.isnan(pcc).double().mean()) <= ref.MAX_NAN_SHARE
    check_scalars(got, {k: float(v) for k, v in want.items()}, "N=1024 G=17002")
    assert torch.equal(torch.isnan(got["pcc_per_gene"]), torch.isnan(pcc))
    ok = ~torch.isnan(pcc)
    assert max_abs_rel(got["pcc_per_gene"][ok].cpu(), pcc[ok].cpu()) < TOL


def test_composition_with_decode_sample_and_generation_block():
    from scldm_amd.evaluations import MMDLoss, RBFKernel, BrayCurtisKernel, RuzickaKernel, TanimotoKernel
    from scldm_amd.evaluations import count_metrics, generation_metrics, normalize_log1p, reconstruction_metrics
    from test_gpu_vae import build
    g, vae, _, _ = build("vae_small")
    counts = cu(g["counts"])
    drawn = vae.decode_sample(cu(g["z"]), cu(g["genes"]), cu(g["library_size"]), seed=11)
    rec, direct = reconstruction_metrics(drawn, counts), count_metrics(drawn, counts)
    assert sorted(rec) == ["mse", "pcc", "zeros_accuracy"]
    for k in rec:
        assert bits_equal(rec[k], direct[k]), k
    assert bool(torch.isfinite(rec["mse"])) and bool(torch.isfinite(rec["zeros_accuracy"]))

    pred, true, _ = inputs(65, 1001, 5)
    gen_counts, true_counts = cu(pred), cu(true)
    lib = true_counts.sum(1, keepdim=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)   # Sinkhorn at reg = 0.05 on raw-scale costs reports its breakdown (see wasserstein)
        out = generation_metrics(true_counts, gen_counts, lib)
    assert set(out) == {"mmd_braycurtis_counts", "mmd_tanimoto", "mmd_ruzicka_counts", "mmd_rbf", "wasserstein1_sinkhorn",
                        "wasserstein2_sinkhorn", "r2_mean", "r2_var", "total_samples"}
    assert out["total_samples"] == 65
    ts, gs = normalize_log1p(true_counts, lib), normalize_log1p(gen_counts, lib)
    assert torch.equal(out["mmd_braycurtis_counts"], MMDLoss(BrayCurtisKernel())(ts, gs))
    assert torch.equal(out["mmd_ruzicka_counts"], MMDLoss(RuzickaKernel())(ts, gs))
    assert torch.equal(out["mmd_tanimoto"], MMDLoss(TanimotoKernel())(true_counts, gen_counts))
    assert torch.equal(out["mmd_rbf"], MMDLoss(RBFKernel())(true_counts, gen_counts))
    # the reference calls fn(counts_true_scaled, counts_generated_scaled): the true cells are `preds` (models.py:922)
    d = true.sum(1)
    want = ref.count_metrics(true, pred, d, d)
    check_scalars(out, want, "generation block", keys=("r2_mean", "r2_var"))
    assert set(generation_metrics(true_counts, gen_counts, lib, mmd=False, wasserstein=False)) == {"r2_mean", "r2_var", "total_samples"}


def test_argument_errors_leave_the_library_usable():
    from scldm_amd.evaluations import count_metrics, normalize_log1p
    pred, true, want = inputs(3, 70, 9)
    P, T = cu(pred), cu(true)
    with pytest.raises(ValueError):
        count_metrics(P, T[:, :69].contiguous())                 # mismatched G
    with pytest.raises(ValueError):
        count_metrics(P.t().contiguous().t(), T)                 # not contiguous
    with pytest.raises(RuntimeError):
        count_metrics(P.cpu(), T)                                # a CPU tensor
    with pytest.raises(ValueError):
        count_metrics(P[:, :0], T[:, :0])                        # G = 0
    with pytest.raises(ValueError):
        count_metrics(P.double(), T)
    with pytest.raises(ValueError):
        count_metrics(P, T, pred_size=cu(true.sum(1))[:2])
    with pytest.raises(ValueError):
        normalize_log1p(P[0])
    check_scalars(count_metrics(P, T), want["own"], "after the errors")

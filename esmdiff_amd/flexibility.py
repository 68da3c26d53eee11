"""Residue flexibility of an ensemble on the device: the pairwise RMSF of the reference, the mean structure and the RMSF about it,
Cartesian PCA, and the reference's "ResFlex" correlation statistics.  DESIGN.md §3.21 states every definition.

  pair_rmsf                 analysis/apo_analysis.py:252-260 (the sqrt of the mean over sample pairs of the squared aligned deviation)
                            without its (n, n, L) array: csrc/flex.hip reduces the pairs on the device in O(n L) memory.
  mean_structure, rmsf      the accepted definition, which the reference lacks (slm/utils/eval_utils.py:51-54 takes the variance
                            of unsuperposed coordinates and says "FIXME: not sure if this is correct"; esmdiff_amd.metrics.rmsf
                            restates that and stays as it is): every structure is superposed on an iteratively refined mean
                            structure, and the fluctuation is taken about that mean.  O(n L) per iteration.
  pca                       essential dynamics: the principal components of the coordinates superposed on the mean structure.
  flexibility_correlation   Pearson / Spearman / Kendall tau-b as scipy.stats' defaults compute them (apo_analysis.py:307-311), in
                            plain numpy.
  apo_summary               the numbers apo_analysis.main prints (:304-329) from a list of ensemble.apo_report dicts.

Inputs follow esmdiff_amd/ensemble.py: CA traces (n, L, 3) in Angstrom as arrays, tensors or a path; residues with NaN coordinates
are masked, `mask` (n, L) masks more.  Every fit is the proper rotation.  Results are numpy arrays on the host.  The kernels are
csrc/flex.hip; dense float64 linear algebra (one eigh) goes through torch on the device, as in metrics.tica_fit.  There is no CPU
fallback."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import pairs


# ---- the pairwise RMSF ---------------------------------------------------------------------------------------------------------
def pair_rmsf(samples, mask=None) -> np.ndarray:
    """sqrt(sum_sq / count) per residue -> (L,): over the sample pairs i < j, each fitted (Kabsch, proper) on the residues valid in
    both, the root mean squared deviation of the residue.  Without masks it equals ensemble.apo_report(...)["rmsf"].  With masks it
    averages over the pairs in which the residue is resolved (NaN where there is none, and for fewer than two samples), and a pair
    is fitted on its common residues about their centroid; apo_report's numpy mean yields NaN for any residue masked anywhere, and
    that behaviour stays as it is."""
    A = pairs.coords(samples, "samples")
    sum_sq, count = pairs.pair_msf(A, pairs.valid_mask(A, mask))
    sum_sq, count = sum_sq.cpu().numpy(), count.cpu().numpy()
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(count > 0, np.sqrt(sum_sq / count), np.nan)


# ---- the mean structure --------------------------------------------------------------------------------------------------------
@dataclass
class MeanStructure:
    mean: np.ndarray            # (L, 3), NaN where no structure is resolved
    aligned: np.ndarray         # (n, L, 3) the structures fitted onto the last reference
    rmsf: np.ndarray            # (L,) sqrt of the mean squared distance from `mean` over the structures resolved there
    rmsd_to_mean: np.ndarray    # (n,) RMSD of aligned[i] from `mean` over its resolved residues, without refitting
    count: np.ndarray           # (L,) structures resolved at the residue
    n_iter: int
    converged: bool


def _mean_structure(A, ma, start: int, tol: float, max_iter: int):
    """The iteration on the device -> aligned, valid (bool (n, L)), mean, msf, count, n_iter, converged."""
    n, L = A.shape[:2]
    if not 0 <= start < n:
        raise ValueError(f"start = {start} is not one of the {n} structures")
    if max_iter < 1:
        raise ValueError(f"max_iter = {max_iter} (at least 1)")
    given = torch.ones((n, L), dtype=torch.bool, device=A.device) if ma is None else ma.bool()
    ref, mref = A[start].contiguous(), given[start].to(torch.uint8).contiguous()
    n_iter, converged = 0, False
    while n_iter < max_iter:
        aligned, _ = pairs.fit(A, ma, ref, mref)
        valid = given & ~torch.isnan(aligned).any(-1)             # a structure without two common residues comes back NaN
        mean, msf, count = pairs.moments(aligned, valid.to(torch.uint8).contiguous())
        mnew = count > 0
        both = mnew & mref.bool()
        step = float(torch.sqrt(((mean[both] - ref[both]) ** 2).sum(-1).mean()))   # no refit; the one host read of the iteration
        ref, mref = mean, mnew.to(torch.uint8).contiguous()
        n_iter += 1
        if tol > 0 and step <= tol:
            converged = True
            break
    return aligned, valid, mean, msf, count, n_iter, converged


def mean_structure(samples, mask=None, start: int = 0, tol: float = 1e-6, max_iter: int = 50) -> MeanStructure:
    """The iteratively refined mean structure (generalised Procrustes).  The rule, which tests/flex_ref.py restates:
      1. reference = structure `start` with its valid residues;
      2. each iteration: fit all structures to the reference (on the residues valid in both); the moments of the aligned structures
         give the new mean, valid where count > 0; step = RMSD between the new mean and the old reference over the residues valid in
         both, WITHOUT refitting; the new mean becomes the reference; stop when step <= tol or after max_iter iterations (tol = 0
         runs exactly max_iter iterations);
      3. rmsf = sqrt(msf) of the last iteration's moments.
    `aligned` are the structures as the last iteration fitted them (onto the reference before the last update)."""
    A = pairs.coords(samples, "samples")
    aligned, valid, mean, msf, count, n_iter, converged = _mean_structure(A, pairs.valid_mask(A, mask), start, tol, max_iter)
    d2 = torch.where(valid, ((aligned - mean[None]) ** 2).sum(-1), torch.zeros((), dtype=torch.float64, device=A.device))
    to_mean = torch.sqrt(d2.sum(1) / valid.sum(1))                # 0 / 0 = NaN: a structure with no resolved residue
    return MeanStructure(mean.cpu().numpy(), aligned.cpu().numpy(), torch.sqrt(msf).cpu().numpy(), to_mean.cpu().numpy(),
                         count.cpu().numpy(), n_iter, converged)


def rmsf(samples, mask=None, **kw) -> np.ndarray:
    """The RMSF about the mean structure -> (L,): mean_structure(...).rmsf."""
    return mean_structure(samples, mask, **kw).rmsf


# ---- Cartesian PCA -------------------------------------------------------------------------------------------------------------
@dataclass
class PCA:
    explained_variance: np.ndarray          # (k,) eigenvalues of the covariance (divisor n - 1), descending
    explained_variance_ratio: np.ndarray    # (k,) over the total variance (the covariance's trace)
    modes: np.ndarray                       # (k, L', 3) unit norm, the component of largest magnitude positive
    projections: np.ndarray                 # (n, k) of the samples
    mean: np.ndarray                        # (L, 3) the mean structure
    residues: np.ndarray                    # (L',) indices of the residues valid in every structure

    def _fit(self, x):
        """x (m, L, 3) fitted onto the mean on `residues` (and where x is resolved) -> (m, L', 3) on the host."""
        X = pairs.coords(x, "x")
        L = self.mean.shape[0]
        assert X.shape[1] == L, f"structures of {X.shape[1]} residues, the PCA was fitted on {L}"
        on = torch.zeros(L, dtype=torch.uint8, device=X.device)
        on[torch.as_tensor(self.residues, device=X.device)] = 1
        ref = torch.nan_to_num(torch.as_tensor(self.mean, device=X.device)).contiguous()
        aligned, _ = pairs.fit(X, pairs.valid_mask(X, None), ref, on)
        return aligned.cpu().numpy()[:, self.residues]

    def project(self, x) -> np.ndarray:
        """Other structures (m, L, 3), fitted onto the mean on `residues` -> (m, k).  A structure that lacks one of them gives NaN."""
        d = self._fit(x) - self.mean[self.residues][None]
        return d.reshape(len(d), -1) @ self.modes.reshape(len(self.modes), -1).T

    def displacement_overlap(self, s1, s2) -> dict:
        """How much of the displacement between two states the leading modes span.  Both are fitted onto the mean (x1, x2);
        d = x2 - x1 on the PCA residues resolved in both; -> {"overlap": (k,) the cumulative sum over j <= k of (d . v_j)^2 / |d|^2
        with the modes restricted to those residues, "n_residues": their number}."""
        x1, x2 = self._fit(s1)[0], self._fit(s2)[0]
        ok = np.isfinite(x1).all(-1) & np.isfinite(x2).all(-1)
        d = (x2 - x1)[ok].reshape(-1)
        v = self.modes[:, ok].reshape(len(self.modes), -1)
        with np.errstate(invalid="ignore", divide="ignore"):
            return {"overlap": np.cumsum((v @ d) ** 2) / (d @ d), "n_residues": int(ok.sum())}


def pca(samples, mask=None, n_components: int = 3, **kw) -> PCA:
    """Principal components of the coordinates superposed on the mean structure (mean_structure(samples, mask, **kw)), over the
    residues valid in EVERY structure (`residues`, L' of them).  Centred on the mean; covariance with divisor n - 1 (np.cov's and
    sklearn's convention).  One torch.linalg.eigh on the device: of the n x n Gram matrix when n < 3 L', else of the 3 L' x 3 L'
    covariance.  k = n_components clipped to min(n - 1, 3 L')."""
    A = pairs.coords(samples, "samples")
    aligned, valid, mean, _, _, _, _ = _mean_structure(A, pairs.valid_mask(A, mask), kw.pop("start", 0), kw.pop("tol", 1e-6),
                                                       kw.pop("max_iter", 50))
    assert not kw, f"unknown arguments {sorted(kw)}"
    n = A.shape[0]
    keep = torch.nonzero(valid.all(0)).flatten()
    d = 3 * int(keep.numel())
    k = max(0, min(int(n_components), n - 1, d))
    if k < 1:
        raise ValueError(f"no component to compute: {n} structures, {d // 3} residues valid in all of them, n_components = {n_components}")
    X = (aligned[:, keep] - mean[keep][None]).reshape(n, d)
    total = (X * X).sum() / (n - 1)
    if n < d:
        lam, U = torch.linalg.eigh(X @ X.T / (n - 1))
        lam, V = lam.flip(0)[:k], (X.T @ U.flip(1)[:, :k]).T
        V = V / torch.linalg.norm(V, dim=1, keepdim=True)
    else:
        lam, V = torch.linalg.eigh(X.T @ X / (n - 1))
        lam, V = lam.flip(0)[:k], V.flip(1)[:, :k].T.contiguous()
    big = V.gather(1, V.abs().argmax(1, keepdim=True))
    V = V * torch.where(big < 0, -1.0, 1.0)
    return PCA(lam.cpu().numpy(), (lam / total).cpu().numpy(), V.reshape(k, -1, 3).cpu().numpy(), (X @ V.T).cpu().numpy(),
               mean.cpu().numpy(), keep.cpu().numpy())


# ---- the reference's correlation statistics (host, numpy) ----------------------------------------------------------------------
def _pearson(x: np.ndarray, y: np.ndarray) -> float:
    if len(x) < 2:
        return float("nan")
    a, b = x - x.mean(), y - y.mean()
    den = np.sqrt((a * a).sum() * (b * b).sum())
    return float(np.clip((a * b).sum() / den, -1.0, 1.0)) if den > 0 else float("nan")


def _average_ranks(x: np.ndarray) -> np.ndarray:
    """1-based ranks, ties sharing the average of their positions (scipy.stats.rankdata's default)."""
    order = np.argsort(x, kind="mergesort")
    s = x[order]
    first = np.r_[True, s[1:] != s[:-1]]
    group = np.cumsum(first) - 1
    start = np.flatnonzero(first)
    size = np.diff(np.r_[start, len(x)])
    ranks = np.empty(len(x))
    ranks[order] = (start + 0.5 * (size - 1) + 1.0)[group]
    return ranks


def _kendall_tau_b(x: np.ndarray, y: np.ndarray) -> float:
    """(P - Q) / sqrt((n0 - n1) (n0 - n2)): concordant minus discordant pairs over the pairs untied in x and the pairs untied in y."""
    if len(x) < 2:
        return float("nan")
    num = nx = ny = 0.0
    for i in range(len(x) - 1):                                   # one row of the pair triangle at a time: O(n) memory
        sx, sy = np.sign(x[i + 1:] - x[i]), np.sign(y[i + 1:] - y[i])
        num += float((sx * sy).sum())
        nx += float(np.abs(sx).sum())
        ny += float(np.abs(sy).sum())
    return float(num / np.sqrt(nx * ny)) if nx > 0 and ny > 0 else float("nan")


def _finite_both(x, y):
    x, y = np.asarray(x, np.float64).reshape(-1), np.asarray(y, np.float64).reshape(-1)
    assert x.shape == y.shape, f"{x.shape} and {y.shape} differ"
    ok = np.isfinite(x) & np.isfinite(y)
    return x[ok], y[ok]


def flexibility_correlation(x, y) -> dict:
    """Pearson, Spearman (Pearson of average ranks) and Kendall (tau-b) of two per-residue profiles over the entries finite in
    both, and their number n: scipy.stats' pearsonr / spearmanr / kendalltau defaults, which apo_analysis.py:307-311 applies to the
    apo-holo deviation and the ensemble's RMSF.  NaN when either side is constant or n < 2.  Plain numpy on the host."""
    x, y = _finite_both(x, y)
    return {"pearson": _pearson(x, y), "spearman": _pearson(_average_ranks(x), _average_ranks(y)) if len(x) > 1 else float("nan"),
            "kendall": _kendall_tau_b(x, y), "n": int(len(x))}


def apo_summary(reports, rounded: bool = True) -> dict:
    """apo_analysis.main:304-329 from a list of ensemble.apo_report dicts, one per target ->
      tm_correlation   Pearson(ensvar, tmpair) over the targets (:318)
      rmsd_global      Pearson of the concatenated `rmsd` and `rmsf` over the entries finite in both (:314-319)
      rmsd_pt_mean / rmsd_pt_median   of the per-target Pearson, targets without one left out as pandas does (:320-321)
      tm_ens_mean / tm_ens_median     of tm_ens (:285)
      per_target       the table of :307-311: one flexibility_correlation(rmsd, rmsf) per target (never rounded)
    rounded: to 3 decimals, as the reference prints them."""
    table = [flexibility_correlation(r["rmsd"], r["rmsf"]) for r in reports]
    pt = np.array([t["pearson"] for t in table], np.float64)
    pt = pt[np.isfinite(pt)]
    gx, gy = _finite_both(np.concatenate([np.asarray(r["rmsd"], np.float64).reshape(-1) for r in reports]),
                          np.concatenate([np.asarray(r["rmsf"], np.float64).reshape(-1) for r in reports]))
    tm_ens = np.array([r["tm_ens"] for r in reports], np.float64)
    out = {"tm_correlation": _pearson(*_finite_both([r["ensvar"] for r in reports], [r["tmpair"] for r in reports])),
           "rmsd_global": _pearson(gx, gy),
           "rmsd_pt_mean": float(pt.mean()) if len(pt) else float("nan"),
           "rmsd_pt_median": float(np.median(pt)) if len(pt) else float("nan"),
           "tm_ens_mean": float(np.mean(tm_ens)), "tm_ens_median": float(np.median(tm_ens))}
    if rounded:
        out = {k: round(v, 3) for k, v in out.items()}
    out["per_target"] = table
    return out

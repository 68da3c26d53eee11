"""TEST INFRASTRUCTURE — float64 numpy restatement of esmdiff_amd/csrc/flex.hip and esmdiff_amd/flexibility.py.

pair_msf   for every pair i < j the proper Kabsch fit (tests/ensemble_ref.py, numpy's SVD) on the residues valid in both; per residue
           the sum of the squared deviations and the number of pairs it was valid in.  Pairs with fewer than 2 common residues are
           skipped and not counted.
gpa        the mean-structure iteration, the exact rule of flexibility.mean_structure's docstring.
pca        np.cov's convention (divisor n - 1) through numpy's eigh of the full covariance, whatever n: the kernel side's Gram path
           is checked against it.
pearson / spearman / kendall   written from the definitions (O(n^2) loops for tau-b), pinned against scipy.stats by
           tests/test_flex_cpu.py where scipy is installed."""
from __future__ import annotations

import numpy as np

from tests import ensemble_ref as E


def _valid(A, mask):
    ok = ~np.isnan(A).any(-1)
    return ok if mask is None else ok & np.asarray(mask, bool)


def pair_msf(A, mask=None):
    """A (n, L, 3) -> sum_sq (L,) float64, count (L,) int64."""
    A = np.asarray(A, np.float64)
    ok = _valid(A, mask)
    n, L = A.shape[:2]
    sum_sq, count = np.zeros(L), np.zeros(L, np.int64)
    for i in range(n):
        for j in range(i + 1, n):
            _, sd, _, _ = E.superpose_pair(A[i], A[j], ok[i], ok[j], allow_reflection=False)
            both = ok[i] & ok[j]
            if both.sum() < 2:
                continue
            sum_sq[both] += sd[both]
            count[both] += 1
    return sum_sq, count


def fit(A, ok, ref, mref):
    """Every A[i] onto ref on the residues valid in both -> aligned (n, L, 3) (the whole structure moved; NaN with fewer than 2 common
    residues), rmsd (n,)."""
    aligned, rmsd = np.full(A.shape, np.nan), np.full(len(A), np.nan)
    for i, a in enumerate(A):
        both = ok[i] & mref
        if both.sum() < 2:
            continue
        R, t = E.kabsch(a[both], ref[both], allow_reflection=False)
        aligned[i] = a @ R.T + t
        rmsd[i] = np.sqrt(((aligned[i][both] - ref[both]) ** 2).sum(-1).mean())
    return aligned, rmsd


def moments(X, ok):
    """-> mean (L, 3), msf (L,), count (L,) over the structures valid at each residue; NaN where count is 0."""
    L = X.shape[1]
    mean, msf, count = np.full((L, 3), np.nan), np.full(L, np.nan), ok.sum(0).astype(np.int32)
    for l in range(L):
        if count[l]:
            x = X[ok[:, l], l]
            mean[l] = x.mean(0)
            msf[l] = ((x - mean[l]) ** 2).sum(-1).mean()
    return mean, msf, count


def gpa(A, mask=None, start=0, tol=1e-6, max_iter=50):
    """-> dict(mean, aligned, msf, rmsf, rmsd_to_mean, count, n_iter, converged, steps, valid)."""
    A = np.asarray(A, np.float64)
    given = _valid(A, mask)
    ref, mref = A[start].copy(), given[start].copy()
    steps, converged = [], False
    while len(steps) < max_iter:
        aligned, _ = fit(A, given, ref, mref)
        valid = given & ~np.isnan(aligned).any(-1)
        mean, msf, count = moments(aligned, valid)
        mnew = count > 0
        both = mnew & mref
        steps.append(float(np.sqrt(((mean[both] - ref[both]) ** 2).sum(-1).mean())) if both.any() else float("nan"))
        ref, mref = mean, mnew
        if tol > 0 and steps[-1] <= tol:
            converged = True
            break
    d2 = np.where(valid, ((aligned - mean[None]) ** 2).sum(-1), 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        to_mean = np.sqrt(d2.sum(1) / valid.sum(1))
    return {"mean": mean, "aligned": aligned, "msf": msf, "rmsf": np.sqrt(msf), "rmsd_to_mean": to_mean, "count": count,
            "n_iter": len(steps), "converged": converged, "steps": steps, "valid": valid}


def sign_convention(V):
    """Rows of V (k, d): the component of largest magnitude made positive."""
    V = np.array(V, np.float64)
    for v in V:
        if v[np.abs(v).argmax()] < 0:
            v *= -1
    return V


def pca(A, mask=None, n_components=3, **kw):
    """-> dict(explained_variance (k,), explained_variance_ratio, modes (k, L', 3), projections (n, k), mean, residues, trace)."""
    g = gpa(A, mask, **kw)
    keep = np.flatnonzero(g["valid"].all(0))
    n = len(g["aligned"])
    X = (g["aligned"][:, keep] - g["mean"][keep][None]).reshape(n, -1)
    C = X.T @ X / (n - 1)
    lam, V = np.linalg.eigh(C)
    k = min(n_components, n - 1, X.shape[1])
    lam, V = lam[::-1][:k], sign_convention(V[:, ::-1][:, :k].T)
    return {"explained_variance": lam, "explained_variance_ratio": lam / np.trace(C), "modes": V.reshape(k, -1, 3),
            "projections": X @ V.T, "mean": g["mean"], "residues": keep, "trace": float(np.trace(C))}


def project(p, x, mask=None):
    """x (m, L, 3) fitted onto p's mean on its residues -> the fitted coordinates on those residues (m, L', 3) and projections (m, k)."""
    x = np.asarray(x, np.float64)
    x = x[None] if x.ndim == 2 else x
    on = np.zeros(x.shape[1], bool)
    on[p["residues"]] = True
    aligned, _ = fit(x, _valid(x, mask), np.nan_to_num(p["mean"]), on)
    xr = aligned[:, p["residues"]]
    d = xr - p["mean"][p["residues"]][None]
    return xr, d.reshape(len(d), -1) @ p["modes"].reshape(len(p["modes"]), -1).T


def displacement_overlap(p, s1, s2):
    x1, x2 = project(p, s1)[0][0], project(p, s2)[0][0]
    ok = np.isfinite(x1).all(-1) & np.isfinite(x2).all(-1)
    d = (x2 - x1)[ok].reshape(-1)
    v = p["modes"][:, ok].reshape(len(p["modes"]), -1)
    return np.cumsum((v @ d) ** 2) / (d @ d), int(ok.sum())


# ---- correlations, from the definitions ------------------------------------------------------------------------------------------
def pearson(x, y):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    if len(x) < 2 or np.ptp(x) == 0 or np.ptp(y) == 0:
        return float("nan")
    return float(np.corrcoef(x, y)[0, 1])


def average_ranks(x):
    x = np.asarray(x, np.float64)
    return np.array([(x < v).sum() + ((x == v).sum() + 1) / 2 for v in x])


def spearman(x, y):
    return pearson(average_ranks(x), average_ranks(y))


def kendall(x, y):
    """tau-b = (P - Q) / sqrt((P + Q + T) (P + Q + U)), T / U the pairs tied only in x / only in y."""
    P = Q = T = U = 0
    for i in range(len(x)):
        for j in range(i + 1, len(x)):
            dx, dy = np.sign(x[i] - x[j]), np.sign(y[i] - y[j])
            if dx * dy > 0:
                P += 1
            elif dx * dy < 0:
                Q += 1
            elif dx == 0 and dy != 0:
                T += 1
            elif dy == 0 and dx != 0:
                U += 1
    den = np.sqrt(float((P + Q + T) * (P + Q + U)))
    return float((P - Q) / den) if den > 0 else float("nan")


# ---- seeded test structures ------------------------------------------------------------------------------------------------------
PLANTED_AMPLITUDES = (3.0, 1.5, 0.6)


def planted(rng, n, L, noise=0.05):
    """A base chain plus three fixed unit displacement fields with per-structure amplitudes N(0, 1) sqrt(L) (3.0, 1.5, 0.6) A, 0.05 A
    isotropic noise, and a random rigid motion of every structure -> (n, L, 3)."""
    base = E.ca_chain(rng, L)
    fields = rng.normal(size=(3, L, 3))
    fields /= np.linalg.norm(fields.reshape(3, -1), axis=1)[:, None, None]
    out = []
    for _ in range(n):
        amp = rng.normal(size=3) * np.sqrt(L) * np.array(PLANTED_AMPLITUDES)
        x = base + np.tensordot(amp, fields, 1) + rng.normal(size=(L, 3)) * noise
        out.append(x @ E.random_rotation(rng).T + rng.normal(size=3) * 20)
    return np.stack(out)


def rigid_moves(rng, A):
    """Every structure of A moved by its own random rigid motion."""
    return np.stack([a @ E.random_rotation(rng).T + rng.normal(size=3) * 20 for a in A])

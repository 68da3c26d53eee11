"""TEST INFRASTRUCTURE — a plain numpy restatement of esmdiff_flex_transforms, of the two entries of esmdiff_amd/csrc/aligned.hip
(include/esmdiff_hip.h) and of the comparisons of esmdiff_amd/covariance.py.  No device.

The TRANSFORM is tests/flex_ref.py's Kabsch fit (numpy's SVD), written out as the row [rot (row-major), tr].  The FEATURE is restated
with the published arithmetic, so the tests may ask for the same bits: f_{3l+c} = (((R[c][0] x + R[c][1] y) + R[c][2] z) + tr[c]), every
product and add a numpy ufunc of its own (no FMA); T = None: the coordinate itself.  The MOMENTS are restated in float64 (a plain
matrix product: its order is not the kernel's, the tests bound the difference) and, for integer input, in int64 (exact: the kernel
must equal it).  The residual sum r and the PROJECTION are restated in the kernel's published order:
  sums         chunks of FRAME_CHUNK consecutive t; a chunk's sum is s = 0, s = s + (f(t) - c) over its USED t in increasing order; the
               total is chunk 0's sum, + chunk 1's, + chunk 2's ...
  projection   p_l = 0, p_l = p_l + (f_d - mean_d) * W[d][k] for d = l, l + 64, ... (l = 0 .. 63), then p = p + p[l ^ s] for
               s = 32, 16, 8, 4, 2, 1.
The comparisons are written from the definitions on ALIGNED FRAMES (np.cov, numpy's eigh), not from moments."""
from __future__ import annotations

import itertools

import numpy as np

from tests import ensemble_ref as E

MAX_L, MAX_DIM, FRAME_CHUNK = 1280, 16, 128


def scratch_bytes(L: int, slots: int) -> int:
    return slots * (9 * L * L + 3 * L) * 8


def gamma(k: int) -> float:
    """gamma_k = k u / (1 - k u), u = 2^-53: the standard bound of a sum of k terms in any order, with or without FMA."""
    u = 2.0 ** -53
    return k * u / (1.0 - k * u)


def transforms(A, ok, ref, mref):
    """Every A[i] onto ref on the residues valid in both -> T (n, 12), rmsd (n,), good (n,) bool; NaN rows with fewer than 2 of them."""
    n = len(A)
    T, rmsd, good = np.full((n, 12), np.nan), np.full(n, np.nan), np.zeros(n, bool)
    for i, a in enumerate(A):
        both = ok[i] & mref
        if both.sum() < 2:
            continue
        R, t = E.kabsch(a[both], ref[both], allow_reflection=False)
        T[i], good[i] = np.concatenate([R.reshape(-1), t]), True
        rmsd[i] = np.sqrt((((a @ R.T + t)[both] - ref[both]) ** 2).sum(-1).mean())
    return T, rmsd, good


def signed_permutations() -> np.ndarray:
    """The 24 proper (det = +1) signed permutation matrices (24, 3, 3): the rotations that keep integers integers."""
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((-1.0, 1.0), repeat=3):
            R = np.zeros((3, 3))
            R[np.arange(3), perm] = signs
            if np.linalg.det(R) > 0:
                out.append(R)
    return np.stack(out)


def features(X, T=None) -> np.ndarray:
    """X (n, L, 3), T (n, 12) or None -> the (n, 3L) features with the published bits."""
    X = np.asarray(X, np.float64)
    n, L = X.shape[:2]
    if T is None:
        return X.reshape(n, 3 * L).copy()
    T = np.asarray(T, np.float64)
    x, y, z = X[:, :, 0], X[:, :, 1], X[:, :, 2]
    F = np.empty((n, L, 3))
    for c in range(3):
        r0, r1, r2, tr = T[:, 3 * c][:, None], T[:, 3 * c + 1][:, None], T[:, 3 * c + 2][:, None], T[:, 9 + c][:, None]
        F[:, :, c] = ((r0 * x + r1 * y) + r2 * z) + tr
    return F.reshape(n, 3 * L)


def _used(n, use):
    return np.ones(n, bool) if use is None else np.asarray(use).astype(bool)


def sums(F, use, c) -> np.ndarray:
    """sum over the used t of F[t] - c, in the kernel's order."""
    on = _used(len(F), use)
    total = None
    for t0 in range(0, len(F), FRAME_CHUNK):
        s = np.zeros(F.shape[1])
        for t in range(t0, min(t0 + FRAME_CHUNK, len(F))):
            if on[t]:
                s = s + (F[t] - c)
        total = s if total is None else total + s
    return total


def moments(X, T, use, c) -> dict:
    """float64: S as a plain product of a = F[used] - c; r in the kernel's order; count."""
    F, on = features(X, T), _used(len(X), use)
    a = F[on] - c
    return {"S": a.T @ a, "r": sums(F, use, c), "count": int(on.sum())}


def moments_envelope(X, T, use, c) -> dict:
    """|a|^T |a| and sum |a|: what the rounding bound multiplies."""
    a = np.abs(features(X, T)[_used(len(X), use)] - c)
    return {"S": a.T @ a, "r": a.sum(0)}


def moments_int(X, T, use, c) -> dict:
    """int64, exact: X, T (or None) and c integers."""
    X, c = np.asarray(X, np.int64), np.asarray(c, np.int64)
    n, L = X.shape[:2]
    if T is None:
        F = X.reshape(n, 3 * L)
    else:
        T = np.asarray(T, np.int64)
        F = (np.einsum("ncd,nld->nlc", T[:, :9].reshape(n, 3, 3), X) + T[:, None, 9:]).reshape(n, 3 * L)
    a = F[_used(n, use)] - c
    return {"S": a.T @ a, "r": a.sum(0), "count": int(len(a))}


def project(X, T, mean, W) -> np.ndarray:
    F = features(X, T)
    n, D = F.shape
    W = np.asarray(W, np.float64)
    lanes = np.arange(64)
    out = np.zeros((n, W.shape[1]))
    for k in range(W.shape[1]):
        p = np.zeros((n, 64))
        for d0 in range(0, D, 64):
            w = min(64, D - d0)
            p[:, :w] = p[:, :w] + (F[:, d0:d0 + w] - mean[d0:d0 + w]) * W[d0:d0 + w, k]
        for s in (32, 16, 8, 4, 2, 1):
            p = p + p[:, lanes ^ s]
        out[:, k] = p[:, 0]
    return out


# ---- the comparisons, from the definitions on aligned frames (n, L, 3) -----------------------------------------------------------
def psd_sqrt(A):
    s, U = np.linalg.eigh((A + A.T) / 2.0)
    return (U * np.sqrt(np.clip(s, 0.0, None))) @ U.T


def bures(A, B) -> float:
    """tr A + tr B - 2 tr (A^1/2 B A^1/2)^1/2 by two eigh."""
    root = psd_sqrt(A)
    M = root @ B @ root
    ev = np.clip(np.linalg.eigvalsh((M + M.T) / 2.0), 0.0, None)
    return max(float(np.trace(A) + np.trace(B) - 2.0 * np.sqrt(ev).sum()), 0.0)


def covariance(Xa, ddof=1):
    F = Xa.reshape(len(Xa), -1)
    d = F - F.mean(0)
    return d.T @ d / (len(F) - ddof)


def modes(Xa, k):
    """-> eigenvalues (k,) descending, unit modes (k, 3L) with the component of largest magnitude positive."""
    lam, V = np.linalg.eigh(covariance(Xa))
    V = V[:, ::-1][:, :k].T.copy()
    for v in V:
        if v[np.abs(v).argmax()] < 0:
            v *= -1
    return lam[::-1][:k], V


def rmsf(Xa):
    return np.sqrt(((Xa - Xa.mean(0)) ** 2).sum(-1).mean(0))


def dccm(Xa):
    d = Xa - Xa.mean(0)
    c = np.einsum("nic,njc->ij", d, d) / len(Xa)
    s = np.sqrt(np.diag(c))
    return c / np.outer(s, s)


def residue_w2_sq(Xa, Xb):
    """-> w2_sq, translation, variance, (L,) each."""
    L = Xa.shape[1]
    d = Xa.mean(0) - Xb.mean(0)
    trans = (d * d).sum(-1)
    var = np.array([bures(np.cov(Xa[:, l].T), np.cov(Xb[:, l].T)) for l in range(L)])
    return trans + var, trans, var


def rmwd(Xa, Xb):
    w, t, v = residue_w2_sq(Xa, Xb)
    return np.sqrt(w.mean()), np.sqrt(t.mean()), np.sqrt(v.mean())


def subspace_w2(W, Xa, Xb):
    """The Gaussian W2 of the two sets of frames projected on the rows of W (k, 3L)."""
    ya, yb = Xa.reshape(len(Xa), -1) @ W.T, Xb.reshape(len(Xb), -1) @ W.T
    d = ya.mean(0) - yb.mean(0)
    return float(np.sqrt(d @ d + bures(np.atleast_2d(np.cov(ya.T)), np.atleast_2d(np.cov(yb.T)))))


def pca_w2(Xa, Xb, k=2):
    return subspace_w2(modes(Xa, k)[1], Xa, Xb)


def rmsip(U, V) -> float:
    """Rows of U and V (k, D) orthonormal: sqrt(sum_ij (u_i . v_j)^2 / k)."""
    return float(np.sqrt(((U @ V.T) ** 2).sum() / len(U)))


def projection_w2(a, b, p=2) -> float:
    """1-D, from the definition: the quantile functions sampled on the common refinement of both step grids."""
    a, b = np.sort(np.asarray(a, np.float64)), np.sort(np.asarray(b, np.float64))
    n = len(a) * len(b)
    qa, qb = np.repeat(a, len(b)), np.repeat(b, len(a))          # both quantile functions in steps of 1 / (n1 n2)
    return float((np.abs(qa - qb) ** p).sum() / n) ** (1.0 / p)

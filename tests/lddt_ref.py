"""TEST INFRASTRUCTURE — NumPy float64 restatement of the CA-lDDT counts of esmdiff_amd/csrc/lddt.hip (Mariani et al. 2013; DESIGN.md
§3.20), by broadcasting over whole distance matrices.  Integer outputs; the device is held to them exactly.

  pair set of native j   ordered (a, b): |a - b| >= seq_sep, maskB[j, a] and maskB[j, b], dn = |B[j, a] - B[j, b]| < r0 (strict)
  total_res[j, a]        #{b : (a, b) in the set};  total[j] = its sum over a
  kept_res[i, j, a]      sum over thresholds t of #{b : (a, b) in the set, maskA[i, a] and maskA[i, b], | dm - dn | < t} (strict);
                         kept[i, j] = its sum over a
  a distance             sqrt((dx dx + dy dy) + dz dz), each operation rounded once (no FMA), numpy's correctly rounded sqrt
  scores                 per residue kept_res / (n_thresholds total_res), global kept / (n_thresholds total): NaN where total is 0"""
from __future__ import annotations

import numpy as np

R0 = 15.0
THRESHOLDS = (0.5, 1.0, 2.0, 4.0)


def distances(x) -> np.ndarray:
    """(L, 3) -> (L, L)"""
    x = np.asarray(x, np.float64)
    d = x[:, None, :] - x[None, :, :]
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    return np.sqrt((dx * dx + dy * dy) + dz * dz)


def counts(A, B=None, maskA=None, maskB=None, r0: float = R0, thresholds=THRESHOLDS, seq_sep: int = 1):
    """A (n, L, 3), B (m, L, 3) (None: A against itself, maskB = maskA) -> kept (n, m), total (m,), kept_res (n, m, L),
    total_res (m, L), int64."""
    A = np.asarray(A, np.float64)
    if B is None:
        B, maskB = A, maskA
    B = np.asarray(B, np.float64)
    n, L = A.shape[:2]
    m = B.shape[0]
    assert B.shape[1] == L and seq_sep >= 1
    okA = np.ones((n, L), bool) if maskA is None else np.asarray(maskA).astype(bool)
    okB = np.ones((m, L), bool) if maskB is None else np.asarray(maskB).astype(bool)
    idx = np.arange(L)
    far = np.abs(idx[:, None] - idx[None, :]) >= seq_sep
    kept_res, total_res = np.zeros((n, m, L), np.int64), np.zeros((m, L), np.int64)
    with np.errstate(invalid="ignore"):
        dA = [distances(a) for a in A]
        for j in range(m):
            dn = distances(B[j])
            pairs = far & okB[j][:, None] & okB[j][None, :] & (dn < r0)
            total_res[j] = pairs.sum(1)
            for i in range(n):
                both = pairs & okA[i][:, None] & okA[i][None, :]
                diff = np.abs(dA[i] - dn)
                for t in thresholds:
                    kept_res[i, j] += (both & (diff < t)).sum(1)
    return kept_res.sum(-1), total_res.sum(-1), kept_res, total_res


def scores(A, B=None, maskA=None, maskB=None, r0: float = R0, thresholds=THRESHOLDS, seq_sep: int = 1):
    """-> global lDDT (n, m), per-residue lDDT (n, m, L)"""
    kept, total, kept_res, total_res = counts(A, B, maskA, maskB, r0, thresholds, seq_sep)
    nt = len(thresholds)
    with np.errstate(invalid="ignore", divide="ignore"):
        return kept / (nt * total)[None], kept_res / (nt * total_res)[None]


def chain(rng, L: int) -> np.ndarray:
    """A random walk of 3.8 A steps, (L, 3)."""
    steps = rng.normal(size=(L, 3))
    steps *= 3.8 / np.linalg.norm(steps, axis=1, keepdims=True)
    return np.cumsum(steps, axis=0)


def ensemble(rng, k: int, base: np.ndarray, lo: float = 0.2, hi: float = 2.5) -> np.ndarray:
    """k copies of `base` with Gaussian noise of a standard deviation spread from lo to hi Angstrom (a single copy: hi), (k, L, 3): distance differences
    on both sides of every threshold from 0.25 to 6 A."""
    sigma = (np.linspace(lo, hi, k) if k > 1 else np.array([hi]))[:, None, None]
    return base[None] + sigma * rng.normal(size=(k,) + base.shape)

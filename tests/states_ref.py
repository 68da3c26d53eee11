"""Numpy restatements of the three entries of csrc/msm.hip with their published orders (include/esmdiff_hip.h), of the
Lloyd loop of esmdiff_amd.states.kmeans, of the reversible maximum-likelihood estimator and of the inner-simplex step.  The float sums
are loops in the published order, never np.sum; for integer operands there is an int64 restatement beside each.  A plain helper
module: no test, no device."""
from __future__ import annotations

import numpy as np

MAX_K, CENTRE_TILE, FRAME_CHUNK, MAX_DIM = 4096, 128, 1024, 16
TRANSITION_FRAME_CHUNK, TRANSITION_LDS_MAX_K, TRANSITION_SCRATCH_BYTES = 4096, 128, 8
U = 2.0 ** -53


def gamma(m: int) -> float:
    """Higham's gamma_m = m u / (1 - m u): the relative error bound of a sum of m terms in any order."""
    return m * U / (1.0 - m * U)


def chunks(n: int) -> int:
    return (n + FRAME_CHUNK - 1) // FRAME_CHUNK


def slot_bytes(k: int, d: int) -> int:
    return (k * d + k + 1) * 8


def step_scratch_bytes(k: int, d: int, slots: int) -> int:
    return slots * slot_bytes(k, d)


# ---- the entries ----------------------------------------------------------------------------------------------------------------
def assign(Y, centres):
    """-> labels i32 (n,), dist2 f64 (n,): s = 0, s = s + (y_c - c_jc) * (y_c - c_jc) over c; (minimum, index) from (+inf, -1), replaced
    when s < minimum in increasing j; dist2 NaN where the label is -1."""
    Y, C = np.asarray(Y, np.float64), np.asarray(centres, np.float64)
    n, d = Y.shape
    best, idx = np.full(n, np.inf), np.full(n, -1, np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(C.shape[0]):
            s = np.zeros(n)
            for c in range(d):
                t = Y[:, c] - C[j, c]
                s = s + t * t
            take = s < best
            best[take], idx[take] = s[take], j
    return idx, np.where(idx < 0, np.nan, best)


def assign_int(Y, centres):
    """Integer operands: exact int64 squared distances, the first index of the minimum."""
    Y, C = np.asarray(Y, np.int64), np.asarray(centres, np.int64)
    d2 = ((Y[:, None, :] - C[None, :, :]) ** 2).sum(-1)
    idx = d2.argmin(1).astype(np.int32)                    # numpy's argmin: the first occurrence
    return idx, d2[np.arange(len(Y)), idx]


def step(Y, centres):
    """-> labels, counts i64 (k,), sums f64 (k, d), inertia: per chunk of FRAME_CHUNK frames s = +0.0, s = s + y_tc over the frames of a
    label in increasing t (the inertia: s = s + dist2_t over the frames labelled >= 0); the chunks added in increasing index from
    chunk 0's own sums."""
    Y = np.asarray(Y, np.float64)
    n, d = Y.shape
    k = len(centres)
    labels, dist2 = assign(Y, centres)
    counts, sums, inertia = np.zeros(k, np.int64), np.zeros((k, d)), 0.0
    for ch in range(chunks(n)):
        part, part_inertia = np.zeros((k, d)), 0.0
        for t in range(ch * FRAME_CHUNK, min((ch + 1) * FRAME_CHUNK, n)):
            j = labels[t]
            if j < 0:
                continue
            part[j] = part[j] + Y[t]
            part_inertia = part_inertia + dist2[t]
            counts[j] += 1
        sums, inertia = (part, part_inertia) if ch == 0 else (sums + part, inertia + part_inertia)
    return labels, counts, sums, float(inertia)


def step_int(Y, centres):
    """Integer operands: every sum an exact int64."""
    Y = np.asarray(Y, np.int64)
    labels, d2 = assign_int(Y, centres)
    k = len(centres)
    counts = np.bincount(labels, minlength=k).astype(np.int64)
    sums = np.zeros((k, Y.shape[1]), np.int64)
    np.add.at(sums, labels, Y)
    return labels, counts, sums, int(d2.sum())


def transition_counts(labels, k: int, lag: int) -> np.ndarray:
    """counts[a][b] = the number of t < n - lag with labels[t] = a, labels[t + lag] = b, both >= 0."""
    lab = np.asarray(labels, np.int64)
    out = np.zeros((k, k), np.int64)
    if lag < len(lab):
        a, b = lab[:len(lab) - lag], lab[lag:]
        ok = (a >= 0) & (b >= 0)
        np.add.at(out, (a[ok], b[ok]), 1)
    return out


# ---- the layer above ------------------------------------------------------------------------------------------------------------
def lloyd(Y, init, n_iter: int = 100, tol: float = 1e-8, trace=None):
    """esmdiff_amd.states.kmeans restated on `step`: -> centres, labels, counts, inertia, updates, converged.  trace: a list that
    receives (centres, labels) of every step."""
    Y = np.asarray(Y, np.float64)
    centres = np.array(init, np.float64)
    previous, converged, done, res = None, False, 0, None
    while done < n_iter:
        res = step(Y, centres)
        if trace is not None:
            trace.append((centres.copy(), res[0].copy()))
        if previous is not None and np.array_equal(res[0], previous):
            converged = True
            break
        labels, counts, sums, _ = res
        with np.errstate(invalid="ignore", divide="ignore"):
            new = np.where(counts[:, None] > 0, sums / counts[:, None].astype(np.float64), centres)
        shift = float(np.abs(new - centres).max())
        centres, previous, done, res = new, labels, done + 1, None
        if shift <= tol:
            converged = True
            break
    if res is None:
        res = step(Y, centres)
    return centres, res[0], res[1], res[3], done, converged


def reversible_mle(counts, maxiter: int = 100000, tol: float = 1e-12):
    """x_ij <- (c_ij + c_ji) / (c_i / x_i + c_j / x_j), element by element, from x = C + C^T scaled to sum 1 -> T, pi, sweeps."""
    C = np.asarray(counts, np.float64)
    n = len(C)
    ci = np.array([sum(C[i]) for i in range(n)])
    x = np.array([[C[i, j] + C[j, i] for j in range(n)] for i in range(n)])
    x = x / x.sum()
    T = x / x.sum(1)[:, None]
    for sweep in range(1, maxiter + 1):
        xi = x.sum(1)
        new = np.zeros_like(x)
        for i in range(n):
            for j in range(n):
                if C[i, j] + C[j, i] > 0:
                    new[i, j] = (C[i, j] + C[j, i]) / (ci[i] / xi[i] + ci[j] / xi[j])
        x = new / new.sum()
        Tn = x / x.sum(1)[:, None]
        change = np.abs(Tn - T).max()
        T = Tn
        if change <= tol:
            break
    return T, x.sum(1), sweep


def inner_simplex(evec) -> np.ndarray:
    """Weber's inner-simplex guess, row by row: vertices by Gram-Schmidt, barycentric coordinates, clipped and renormalised."""
    evec = np.asarray(evec, np.float64)
    n, m = evec.shape
    c = evec[:, 1:]
    ortho = c.copy()
    ind = [0] * m
    far = 0.0
    for i in range(n):
        if np.linalg.norm(c[i]) > far:
            far, ind[0] = np.linalg.norm(c[i]), i
    ortho -= c[ind[0]]
    for j in range(1, m):
        far, temp = 0.0, ortho[ind[j - 1]].copy()
        for i in range(n):
            ortho[i] -= np.dot(temp, ortho[i]) * temp
            if np.linalg.norm(ortho[i]) > far:
                far, ind[j] = np.linalg.norm(ortho[i]), i
        ortho /= far
    chi = evec @ np.linalg.inv(evec[ind])
    chi[chi < 0] = 0.0
    return chi / chi.sum(1)[:, None]


def slowest_timescale(labels, k: int, lag: int) -> float:
    """labels -> restated counts -> restated reversible estimator on the states that occur (the caller's chain is connected) -> the
    second eigenvalue's timescale."""
    C = transition_counts(labels, k, lag)
    keep = np.flatnonzero(C.sum(1) + C.sum(0) > 0)
    T, _, _ = reversible_mle(C[np.ix_(keep, keep)])
    lam = np.sort(np.abs(np.linalg.eigvals(T)))[::-1]
    return float(-lag / np.log(lam[1]))


# ---- generators -----------------------------------------------------------------------------------------------------------------
def blobs(n: int, k: int, d: int, seed: int = 0, spread: float = 0.05):
    """k well-separated blobs of n frames in d dimensions, in random time order -> Y (n, d), the blob centres (k, d), the blob of
    every frame."""
    rng = np.random.default_rng(seed)
    centres = np.zeros((k, d))
    centres[:, 0] = 3.0 * np.arange(k)                     # 3 apart on the first axis: 60 standard deviations
    centres[:, 1:] = rng.uniform(-1.0, 1.0, size=(k, d - 1))
    owner = rng.integers(0, k, size=n)
    owner[:k] = np.arange(k)                               # no blob is empty
    return centres[owner] + spread * rng.standard_normal((n, d)), centres, owner


BLOBS = dict(n=2500, k=5, d=3, seed=3)


def blob_problem():
    """The input of the model-level tests: Y and the initial centres, the frames at a uniform stride (some blobs get two centres, some
    none).  tests/test_states_cpu.py asserts that every step of Lloyd's iteration on it is well posed."""
    Y, _, _ = blobs(**BLOBS)
    return Y, Y[(np.arange(BLOBS["k"]) * len(Y)) // BLOBS["k"]].copy()


def two_wells(n: int, D: int = 4, seed: int = 0, hop: float = 0.01):
    """A two-state jump process (hop probability per frame) seen through D noisy features: the well decides the first feature's
    mean (-1 or +1, noise 0.15), the other features are fast noise -> X (n, D), wells (n,)."""
    rng = np.random.default_rng(seed)
    flips = rng.random(n) < hop
    wells = np.cumsum(flips) % 2
    X = 0.3 * rng.standard_normal((n, D))
    X[:, 0] = (2.0 * wells - 1.0) + 0.15 * rng.standard_normal(n)
    return X, wells.astype(np.int64)

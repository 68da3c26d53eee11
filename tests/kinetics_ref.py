"""TEST INFRASTRUCTURE — a plain numpy restatement of the three entries of esmdiff_amd/csrc/lagged.hip (include/esmdiff_hip.h,
DESIGN.md §3.27), and the trajectory generator of the eigen-level tests.  No device.

The features of coordinates are oracle.metrics_ref.pairwise_distance_ca (the bits of esmdiff_metrics_pwd).  The MOMENTS are
restated in float64 (plain matrix products: their order is not the kernel's, the tests bound the difference) and, for integer
input, in int64 (exact: the kernel must equal it).  The MEANS, the residual sums and the PROJECTION are restated in the kernel's
published order, so the tests may ask for the same bits:
  window sums   chunks of FRAME_CHUNK consecutive t; a chunk's sum is s = 0, s = s + (f(x_t) - c) in increasing t; the total is chunk
                0's sum, + chunk 1's, + chunk 2's ...; a mean is the total (c = 0) divided by m once.
  projection    p_l = 0, p_l = p_l + (f_d - mean_d) * W[d][k] for d = l, l + 64, ... (l = 0 .. 63), then p = p + p[l ^ s] for
                s = 32, 16, 8, 4, 2, 1.
The eigen tail of the model-level tests is oracle.metrics_ref.tica_fit, imported where it is used, not copied."""
from __future__ import annotations

import numpy as np

from oracle.metrics_ref import pairwise_distance_ca

MAX_L, MAX_D, MAX_DIM, FRAME_CHUNK = 128, 8192, 16, 2048


def n_features(L: int, k: int) -> int:
    return (L - k) * (L - k + 1) // 2


def scratch_bytes(D: int, slots: int, moments: bool) -> int:
    return D * 8 + slots * ((3 * D * D + 2 * D) if moments else 2 * D) * 8


def features(X: np.ndarray, pwd_offset: int) -> np.ndarray:
    """X (n, D) with pwd_offset 0, or (n, L, 3) -> the (n, D) features."""
    X = np.asarray(X, np.float64)
    return X if pwd_offset == 0 else pairwise_distance_ca(X, pwd_offset)


def window_sums(F: np.ndarray, lag: int, c=None):
    """-> sum over t < m of F[t] - c and of F[t + lag] - c, in the kernel's order."""
    m = F.shape[0] - lag
    c = np.zeros(F.shape[1]) if c is None else np.asarray(c, np.float64)
    total = None
    for t0 in range(0, m, FRAME_CHUNK):
        s0, st = np.zeros(F.shape[1]), np.zeros(F.shape[1])
        for t in range(t0, min(t0 + FRAME_CHUNK, m)):
            s0 = s0 + (F[t] - c)
            st = st + (F[t + lag] - c)
        total = (s0, st) if total is None else (total[0] + s0, total[1] + st)
    return total


def means(X, lag: int, pwd_offset: int = 1):
    F = features(X, pwd_offset)
    s0, st = window_sums(F, lag)
    m = float(F.shape[0] - lag)
    return s0 / m, st / m


def moments(X, lag: int, c, pwd_offset: int = 1) -> dict:
    """float64: S00, S0t, Stt as plain products of a = F[:m] - c and b = F[lag:] - c; r0, rt in the kernel's order."""
    F = features(X, pwd_offset)
    m = F.shape[0] - lag
    a, b = F[:m] - c, F[lag:] - c
    r0, rt = window_sums(F, lag, c)
    return {"S00": a.T @ a, "S0t": a.T @ b, "Stt": b.T @ b, "r0": r0, "rt": rt}


def moments_envelope(X, lag: int, c, pwd_offset: int = 1) -> dict:
    """|a|^T |b| for the three matrices, sum |a| and sum |b| for the residuals: what the rounding bound multiplies."""
    F = features(X, pwd_offset)
    m = F.shape[0] - lag
    a, b = np.abs(F[:m] - c), np.abs(F[lag:] - c)
    return {"S00": a.T @ a, "S0t": a.T @ b, "Stt": b.T @ b, "r0": a.sum(0), "rt": b.sum(0)}


def moments_int(F, lag: int, c) -> dict:
    """int64, exact: F and c integers."""
    F, c = np.asarray(F, np.int64), np.asarray(c, np.int64)
    m = F.shape[0] - lag
    a, b = F[:m] - c, F[lag:] - c
    return {"S00": a.T @ a, "S0t": a.T @ b, "Stt": b.T @ b, "r0": a.sum(0), "rt": b.sum(0)}


def project(X, mean, W, pwd_offset: int = 1) -> np.ndarray:
    F = features(X, pwd_offset)
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


def project_envelope(X, mean, W, pwd_offset: int = 1) -> np.ndarray:
    return np.abs(features(X, pwd_offset) - mean) @ np.abs(np.asarray(W, np.float64))


def gamma(k: int) -> float:
    """gamma_k = k u / (1 - k u), u = 2^-53: the standard bound of a sum of k terms in any order, with or without FMA."""
    u = 2.0 ** -53
    return k * u / (1.0 - k * u)


def covariances(mom: dict, m: int):
    """The reversible estimator from raw moments about a centre."""
    d = (mom["r0"] + mom["rt"]) / (2.0 * m)
    return (mom["S00"] + mom["Stt"]) / (2.0 * m) - np.outer(d, d), (mom["S0t"] + mom["S0t"].T) / (2.0 * m) - np.outer(d, d)


def koopman_singular_values(F: np.ndarray, lag: int, epsilon: float = 1e-6) -> np.ndarray:
    """The singular values of c00^-1/2 c0t ctt^-1/2, each window about its own mean, with the rank cut of the reversible form."""
    m = F.shape[0] - lag
    a, b = F[:m] - F[:m].mean(0), F[lag:] - F[lag:].mean(0)
    c00, c0t, ctt = a.T @ a / m, a.T @ b / m, b.T @ b / m

    def whiten(c):
        s, u = np.linalg.eigh(c)
        keep = s > epsilon
        return u[:, keep] / np.sqrt(s[keep])
    return np.linalg.svd(whiten(c00).T @ c0t @ whiten(ctt), compute_uv=False)


def trajectory(n: int, L: int, seed: int = 0) -> np.ndarray:
    """(n, L, 3): a zig-zag CA chain of 3.8 A steps with a hinge at L // 2 whose angle is 0.6 tanh of an AR(1) process of coefficient
    0.97, a twist at L // 4 driven by an AR(1) process of coefficient 0.85, and Gaussian noise of 0.15 A on every coordinate."""
    rng = np.random.default_rng(seed)

    def ar1(coef):
        z = np.empty(n)
        z[0] = rng.standard_normal()
        for t in range(1, n):
            z[t] = coef * z[t - 1] + np.sqrt(1.0 - coef * coef) * rng.standard_normal()
        return z
    hinge, twist = 0.6 * np.tanh(ar1(0.97)), 0.5 * ar1(0.85)
    i = np.arange(L)
    # 3.8 A between neighbours, 60 degrees off the axis: compact enough that the second-order terms of the noise keep every
    # eigenvalue of c00 a factor 3 above the rank cut of 1e-6 (at 30 degrees the smallest one of L = 12 lies at 1.1e-6)
    base = np.stack([i * 3.8 * np.cos(np.pi / 3), (i % 2) * 3.8 * np.sin(np.pi / 3), np.zeros(L)], axis=1)
    out = np.empty((n, L, 3))
    for t in range(n):
        x = base.copy()
        h, q = L // 2, L // 4
        c, s = np.cos(hinge[t]), np.sin(hinge[t])
        rot_z = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
        x[h:] = (x[h:] - x[h]) @ rot_z.T + x[h]                     # the hinge: everything after L // 2 turns in the plane
        c, s = np.cos(twist[t]), np.sin(twist[t])
        rot_x = np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])
        x[:q] = (x[:q] - x[q]) @ rot_x.T + x[q]                     # the twist: everything before L // 4 turns about the chain axis
        out[t] = x
    return out + 0.15 * rng.standard_normal(out.shape)

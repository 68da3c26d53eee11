"""TEST INFRASTRUCTURE — NumPy float64 restatement of esmdiff_amd/csrc/shape.hip: the per-frame size and shape
descriptors with the device's orders of summation, the pair-distance histogram, the Debye intensity, and the host layer of
esmdiff_amd/shape.py on top of them.  No device.  Integer outputs are held exactly, everything made of +, x, / and sqrt bit for bit, the
Debye intensity to 1e-13 of its envelope.

  valid                  a residue that is not masked and has no NaN coordinate
  a distance             sqrt((dx dx + dy dy) + dz dz), each operation rounded once (no FMA), numpy's correctly rounded sqrt
  ORDER over residues    lane l of 64 adds the residues b = l, l + 64 ... in increasing b from +0.0, a residue that is not valid adding
                         nothing; the lanes are combined by the xor butterfly 32, 16 .. 1
  ORDER over pairs       W = waves(L) (1 up to L = 128, then 8); wave w takes the rows a = w, w + W ...; in row a lane l takes
                         b = a + 1 + l, a + 1 + l + 64 ...; a lane keeps one sum from +0.0 across all its rows, a pair that is not
                         valid adding nothing; the butterfly per wave; for W = 8 ((w0 + w1) + (w2 + w3)) + ((w4 + w5) + (w6 + w7))
  frames                 count N, desc (12): the centroid (sum / N), the six sums of (r - c)(r - c)^T (xx, yy, zz, xy, xz, yz; second
                         pass, not divided), sum_inv_d over pairs, dmax, ree; hist: cell floor(d / width), >= bins into cell `bins`
  debye                  I = sum f^2 + 2 sum_{a<b} f_a f_b s(q d), s(x) = sin(x) / x and 1.0 at x == 0, x one product: math.fsum of numpy's
                         own terms (the correctly rounded sum: no order), and the envelope
                         E = sum f^2 + 2 sum |f_a f_b| min(1, 1 / (q d))"""
from __future__ import annotations

import math

import numpy as np

MAX_L, MAX_BINS, MAX_Q, Q_CHUNK = 4096, 4096, 1024, 8


def waves(L: int) -> int:
    """ESMDIFF_SHAPE_WAVES"""
    return 1 if L <= 128 else 8


def valid(X, mask=None) -> np.ndarray:
    ok = ~np.isnan(X).any(-1)
    return ok if mask is None else ok & np.asarray(mask).astype(bool)


def distances(x) -> np.ndarray:
    """(L, 3) -> (L, L), d[a, b] from r_b - r_a"""
    x = np.asarray(x, np.float64)
    dx, dy, dz = (x[None, :, c] - x[:, None, c] for c in range(3))
    return np.sqrt((dx * dx + dy * dy) + dz * dz)


def _butterfly(v):
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[lanes ^ off]
    return v[0]


def residue_sum(terms, ok) -> float:
    lanes = np.zeros(64)
    for k0 in range(0, len(terms), 64):
        t, o = terms[k0:k0 + 64], ok[k0:k0 + 64]
        lanes[:len(t)] = np.where(o, lanes[:len(t)] + t, lanes[:len(t)])
    return _butterfly(lanes)


def pair_sum(terms, ok) -> float:
    """terms (L, L), used above the diagonal; ok (L,) the valid residues"""
    L = len(ok)
    W = waves(L)
    sums = np.zeros(8)
    for w in range(W):
        lanes = np.zeros(64)
        for a in range(w, L - 1, W):
            if not ok[a]:
                continue
            row, o = terms[a, a + 1:], ok[a + 1:]
            for k0 in range(0, len(row), 64):
                t = row[k0:k0 + 64]
                lanes[:len(t)] = np.where(o[k0:k0 + 64], lanes[:len(t)] + t, lanes[:len(t)])
        sums[w] = _butterfly(lanes)
    return sums[0] if W == 1 else ((sums[0] + sums[1]) + (sums[2] + sums[3])) + ((sums[4] + sums[5]) + (sums[6] + sums[7]))


def frames(X, mask=None, width=None, bins: int = 0, sums: bool = True):
    """X (n, L, 3) -> count int64 (n,), desc float64 (n, 12), hist int64 (bins + 1,) or None (width None).  sums = False: the ordered
    sums (the centroid, the six sums, sum_inv_d) are left NaN — for the longest chains, where only the integers and dmax are compared."""
    X = np.asarray(X, np.float64)
    n, L = X.shape[:2]
    ok = valid(X, mask)
    count, desc = ok.sum(1).astype(np.int64), np.full((n, 12), np.nan)
    hist = None if width is None else np.zeros(bins + 1, np.int64)
    iu = np.triu_indices(L, 1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for i in range(n):
            x, o, N = np.where(ok[i][:, None], X[i], np.nan), ok[i], int(count[i])
            d = distances(x)
            pairs = d[iu]
            pairs = pairs[~np.isnan(pairs)]
            if sums:
                c = np.array([residue_sum(x[:, k], o) / N if N else np.nan for k in range(3)])
                r = x - c
                both = o & ~np.isnan(r).any(-1)
                desc[i, :3] = c
                for k, (u, v) in enumerate(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
                    desc[i, 3 + k] = residue_sum(r[:, u] * r[:, v], both)
                desc[i, 9] = pair_sum(1.0 / d, o)
            desc[i, 10] = pairs.max(initial=0.0)
            e = x[L - 1] - x[0]
            desc[i, 11] = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
            if hist is not None:
                cell = np.floor(pairs / width)
                cell = np.where(cell >= bins, bins, cell).astype(np.int64)
                hist += np.bincount(cell, minlength=bins + 1)
    return count, desc, hist


def sinc(x):
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(x == 0.0, 1.0, np.sin(x) / x)


def debye(X, q, ff=None, mask=None):
    """X (n, L, 3), q (Q,), ff (L, Q) or None -> I (n, Q), E (n, Q)"""
    X, q = np.asarray(X, np.float64), np.asarray(q, np.float64)
    n, L = X.shape[:2]
    f = np.ones((L, len(q))) if ff is None else np.asarray(ff, np.float64)
    ok = valid(X, mask)
    a, b = np.triu_indices(L, 1)
    I, E = np.zeros((n, len(q))), np.zeros((n, len(q)))
    for i in range(n):
        d = distances(np.where(ok[i][:, None], X[i], np.nan))[a, b]
        keep = ~np.isnan(d)
        d, pa, pb = d[keep], a[keep], b[keep]
        for k in range(len(q)):
            x = q[k] * d
            own = (f[ok[i], k] * f[ok[i], k]).tolist()
            ffab = f[pa, k] * f[pb, k]
            I[i, k] = math.fsum(own + (2.0 * (ffab * sinc(x))).tolist())
            with np.errstate(divide="ignore"):
                E[i, k] = math.fsum(own + (2.0 * (np.abs(ffab) * np.minimum(1.0, 1.0 / x))).tolist())
    return I, E


# ---- the host layer -----------------------------------------------------------------------------------------------------------------
def derived(count, desc) -> dict:
    """What esmdiff_amd/shape.py makes of one esmdiff_shape_frames result, NaN where a frame has too few valid residues."""
    count = np.asarray(count, np.int64)
    n = len(count)
    out = {k: np.full(n, np.nan) for k in ("rg", "asphericity", "acylindricity", "anisotropy", "ree", "dmax", "rh")}
    out["eigenvalues"], out["gyration_tensor"] = np.full((n, 3), np.nan), np.full((n, 3, 3), np.nan)
    for i in range(n):
        N = int(count[i])
        out["ree"][i] = desc[i, 11]
        if N < 1:
            continue
        xx, yy, zz, xy, xz, yz = desc[i, 3:9] / N
        S = np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]])
        lam = np.linalg.eigvalsh(S)
        out["gyration_tensor"][i], out["eigenvalues"][i] = S, lam
        out["rg"][i] = math.sqrt((xx + yy) + zz)
        out["asphericity"][i] = lam[2] - 0.5 * (lam[0] + lam[1])
        out["acylindricity"][i] = lam[1] - lam[0]
        tr = lam.sum()
        if tr > 0:
            out["anisotropy"][i] = 1.0 - 3.0 * (lam[0] * lam[1] + lam[1] * lam[2] + lam[2] * lam[0]) / tr ** 2
        if N >= 2:
            out["dmax"][i] = desc[i, 10]
            out["rh"][i] = N * N / (2.0 * desc[i, 9])
    return out


def sphere_series(x, terms: int = 12):
    """3 (sin x - x cos x) / x^3 = sum_k 3 (-1)^k (2k + 2) x^(2k) / (2k + 3)!"""
    x = np.asarray(x, np.float64)
    return sum(3.0 * (-1.0) ** k * (2 * k + 2) / math.factorial(2 * k + 3) * x ** (2 * k) for k in range(terms))


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def chain(rng, L: int) -> np.ndarray:
    """A random walk of 3.8 A steps, (L, 3)."""
    steps = rng.normal(size=(L, 3))
    steps *= 3.8 / np.linalg.norm(steps, axis=1, keepdims=True)
    return np.cumsum(steps, axis=0)


def chains(rng, n: int, L: int) -> np.ndarray:
    return np.stack([chain(rng, L) for _ in range(n)])

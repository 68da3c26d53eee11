"""The numpy float64 restatement of csrc/sasa.hip: esmdiff_sasa_frames and esmdiff_cooccurrence by brute force, every
point of every atom against every other present atom of its frame — no cull, no early exit, no chunking that changes a value — with the
operations and the parenthesisation the header states, and the areas esmdiff_amd/accessibility.py derives from the integer counts.
tests/test_sasa_cpu.py holds it to hand-worked cases; tests/test_gpu_sasa.py holds the device to it exactly."""
import math

import numpy as np

MAX_ATOMS, MAX_POINTS = 4096, 1024       # ESMDIFF_SASA_MAX_ATOMS, ESMDIFF_SASA_MAX_POINTS
FOUR_PI = 4.0 * math.pi
GOLDEN_ANGLE = math.pi * (3.0 - math.sqrt(5.0))
DEFAULT_RADII = (1.65, 1.87, 1.76, 1.40)


def cooccurrence_scratch_bytes(n: int, L: int) -> int:
    """ESMDIFF_COOCC_SCRATCH_BYTES."""
    return ((n + 63) // 64) * L * 16


def sphere_points(P: int) -> np.ndarray:
    """The golden-section spiral: z = 1 - (2k + 1) / P, rho = sqrt(1 - z z), phi = k pi (3 - sqrt 5), u = (rho cos phi, rho sin phi, z)."""
    k = np.arange(P, dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / P
    rho = np.sqrt(1.0 - z * z)
    phi = k * GOLDEN_ANGLE
    return np.stack([rho * np.cos(phi), rho * np.sin(phi), z], axis=1)


def present_atoms(X, mask=None) -> np.ndarray:
    """(n, L, A) bool: the residue is not masked and the atom has no NaN coordinate."""
    X = np.asarray(X, np.float64)
    ok = ~np.isnan(X).any(-1)
    if mask is not None:
        ok &= np.asarray(mask, bool)[:, :, None]
    return ok


def frame_counts(c, R, present, u, block_bytes: int = 1 << 27) -> np.ndarray:
    """One frame: centres c (NA, 3), expanded radii R (NA,), present (NA,) bool, unit points u (P, 3) -> int32 (NA,): the points of each
    atom that no other present atom buries, -1 for an absent atom.  p = c + R u; buried when ((dx dx + dy dy) + dz dz) < R_j R_j."""
    out = np.full(len(c), -1, np.int32)
    at = np.nonzero(present)[0]
    c, R, P, M = c[at], R[at], len(u), len(at)
    if M == 0:
        return out
    r2 = R * R
    rows = max(1, block_bytes // (P * M * 3 * 8))
    with np.errstate(invalid="ignore", over="ignore"):
        for i0 in range(0, M, rows):
            i1 = min(M, i0 + rows)
            p = c[i0:i1, None, :] + R[i0:i1, None, None] * u[None, :, :]
            d = p[:, :, None, :] - c[None, None, :, :]
            dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
            buried = ((dx * dx + dy * dy) + dz * dz) < r2[None, None, :]
            own = np.arange(i1 - i0)
            buried[own, :, i0 + own] = False                      # an atom is never tested against itself
            out[at[i0:i1]] = P - buried.any(2).sum(1)
    return out


def atom_area(R, count, P):
    """((4 pi (R R)) count) / P, count and P as float64."""
    return ((FOUR_PI * (R * R)) * np.asarray(count, np.float64)) / float(P)


def residue_sum(a):
    """(..., A) -> (...): ((a0 + a1) + a2) + a3."""
    s = a[..., 0]
    for k in range(1, a.shape[-1]):
        s = s + a[..., k]
    return s


def areas(count, R, P):
    """count (..., L, A) with -1 for absent atoms, expanded radii R (L, A) -> atom area (NaN where absent), residue area and relative
    exposure (NaN where the residue has no atom), total area per frame (absent residues adding nothing)."""
    count = np.asarray(count)
    here = count >= 0
    with np.errstate(invalid="ignore", divide="ignore"):
        a = np.where(here, atom_area(R, count, P), 0.0)
        alone = np.where(here, atom_area(R, float(P), P), 0.0)
        some = here.any(-1)
        res = np.where(some, residue_sum(a), np.nan)
        rel = np.where(some, residue_sum(a) / residue_sum(alone), np.nan)
    return np.where(here, a, np.nan), res, rel, np.where(some, res, 0.0).sum(-1)


def frames(X, mask, radii, points, threshold=0.2) -> dict:
    """esmdiff_sasa_frames: X (n, L, A, 3), mask (n, L) or None, radii (L, A) expanded, points (P, 3) -> the six outputs."""
    X, R, u = np.asarray(X, np.float64), np.asarray(radii, np.float64), np.asarray(points, np.float64)
    n, L, A = X.shape[:3]
    P = len(u)
    assert L * A <= MAX_ATOMS and 1 <= P <= MAX_POINTS and R.shape == (L, A)
    ok = present_atoms(X, mask)
    count = np.full((n, L, A), -1, np.int32)
    for s in range(n):
        count[s] = frame_counts(X[s].reshape(L * A, 3), R.reshape(-1), ok[s].reshape(-1), u).reshape(L, A)
    here = count >= 0
    rel = areas(count, R, P)[2] if n else np.zeros((0, L))
    with np.errstate(invalid="ignore"):
        exposed = np.where(here.any(-1), rel > threshold, 2).astype(np.uint8)
    return {"count": count, "sum_count": np.where(here, count, 0).astype(np.int64).sum(0), "valid": here.sum(0).astype(np.int32),
            "exposed": exposed, "exposed_count": (exposed == 1).sum(0).astype(np.int32), "present_count": (exposed != 2).sum(0).astype(np.int32)}


def cooccurrence(flags) -> np.ndarray:
    """esmdiff_cooccurrence: flags (n, L), 0 or 1 and anything else undefined -> int32 (3, L, L)."""
    f = np.asarray(flags)
    d, o = (f < 2).astype(np.int64), (f == 1).astype(np.int64)
    return np.stack([d.T @ d, o.T @ d, o.T @ o]).astype(np.int32)


# ---- inputs of the tests --------------------------------------------------------------------------------------------------------------
def coil(rng, L: int, A: int = 4) -> np.ndarray:
    """A random coil: CA 3.8 Angstrom apart in random directions, the other atoms of a residue 1.3 to 1.6 Angstrom from its CA."""
    step = rng.normal(size=(L, 3))
    ca = np.cumsum(3.8 * step / np.linalg.norm(step, axis=1, keepdims=True), axis=0)
    if A == 1:
        return ca[:, None, :]
    off = rng.normal(size=(L, A, 3))
    off = off / np.linalg.norm(off, axis=-1, keepdims=True) * rng.uniform(1.3, 1.6, (L, A, 1))
    off[:, 1] = 0.0
    return ca[:, None, :] + off


def helix(L: int) -> np.ndarray:
    """An ideal alpha helix: N, CA, C, O on cylinders of their own radius, 100 degrees and 1.5 Angstrom a residue (Pauling's geometry)."""
    radius, turn, rise = (1.61, 2.29, 1.68, 2.04), np.deg2rad((-25.6, 0.0, 26.6, 37.2)), (-0.87, 0.0, 1.07, 2.28)
    k = np.arange(L)[:, None]
    ang = np.deg2rad(100.0) * k + np.asarray(turn)[None]
    return np.stack([np.asarray(radius) * np.cos(ang), np.asarray(radius) * np.sin(ang), 1.5 * k + np.asarray(rise)[None]], axis=-1)

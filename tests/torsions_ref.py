"""TEST INFRASTRUCTURE — NumPy float64 restatement of esmdiff_amd/csrc/torsions.hip: the backbone torsions, the
bond lengths and angles, and the Ramachandran maps of an ensemble.  Every product and sum is written out term by term and rounded
once, in the order the header states (no np.cross, no np.dot), so x and y of every dihedral carry the device's bits; only atan2 is
numpy's own.

  X (n, L, A, 3)   N, CA, C (and O, never read), A = 3 or 4;  mask (n, L) or None
  present[i]       mask[i] and N, CA, C finite
  link[i]          i -> i + 1: present[i], present[i + 1] and |C[i] - N[i + 1]| <= break_distance
  dihedral         b1 = p1 - p0, b2 = p2 - p1, b3 = p3 - p2, n1 = b1 x b2, n2 = b2 x b3, x = n1 . n2, y = sqrt(b2 . b2) (b1 . n2);
                   defined iff x and y are finite and not both 0; the angle is atan2(y, x)
  phi[i]           dihedral(C[i-1], N[i], CA[i], C[i]), needs link[i-1];  psi[i] = dihedral(N[i], CA[i], C[i], N[i+1]) and
  omega[i]         dihedral(CA[i], C[i], N[i+1], CA[i+1]) need link[i]
  bin              b = floor((angle * 57.29577951308232 + 180.0) / (360.0 / bins)); b -= bins where b >= bins; b += bins where b < 0
  sums             cos = x / r, sin = y / r, r = sqrt(x x + y y); chunks of chunk_frames(n, L) frames, inside a chunk the defined
                   terms one after another in increasing frame from the first defined one (none: +0.0), then the chunk sums in
                   increasing chunk index from chunk 0's"""
from __future__ import annotations

import numpy as np

from tests.dssp_ref import nerf  # noqa: F401  (the builder of the synthetic chains)

BREAK = 2.5
DEG = 57.29577951308232
MAX_BINS = 72


def _sub(a, b):
    return a - b


def _cross(a, b):
    ax, ay, az = a[..., 0], a[..., 1], a[..., 2]
    bx, by, bz = b[..., 0], b[..., 1], b[..., 2]
    return np.stack([ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx], axis=-1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def dihedral_xy(p0, p1, p2, p3):
    """-> x, y, defined (arrays over the leading axes)."""
    with np.errstate(all="ignore"):
        b1, b2, b3 = _sub(p1, p0), _sub(p2, p1), _sub(p3, p2)
        n1, n2 = _cross(b1, b2), _cross(b2, b3)
        x = _dot(n1, n2)
        y = np.sqrt(_dot(b2, b2)) * _dot(b1, n2)
    return x, y, np.isfinite(x) & np.isfinite(y) & ~((x == 0.0) & (y == 0.0))


def _bond_angle(a, mid, b):
    u, v = _sub(a, mid), _sub(b, mid)
    w = _cross(u, v)
    return np.arctan2(np.sqrt(_dot(w, w)), _dot(u, v))


def chunk_frames(n: int, L: int) -> int:
    cap = min(1024, max(1, 65536 // L))
    return max(16, -(-n // cap))


def chunks(n: int, L: int) -> int:
    return -(-n // chunk_frames(n, L))


def scratch_bytes(n: int, L: int) -> int:
    return 0 if chunks(n, L) <= 1 else chunks(n, L) * L * 48


def _prepare(X, mask):
    X = np.asarray(X, np.float64)
    if X.ndim == 3:
        X = X[None]
    n, L = X.shape[:2]
    assert X.shape[2] in (3, 4) and X.shape[3] == 3
    present = np.isfinite(X[:, :, :3]).all((2, 3))
    if mask is not None:
        present &= np.asarray(mask).astype(bool).reshape(n, L)
    x = np.where(present[:, :, None, None], X[:, :, :3], 0.0)      # an absent residue's coordinates are never looked at
    return x, present


def xy(X, mask=None, break_distance: float = BREAK):
    """-> x, y (3, n, L) of phi, psi, omega (0 where undefined), ok bool (3, n, L), present (n, L)."""
    c, present = _prepare(X, mask)
    n, L = present.shape
    N, CA, C = c[:, :, 0], c[:, :, 1], c[:, :, 2]
    x, y, ok = np.zeros((3, n, L)), np.zeros((3, n, L)), np.zeros((3, n, L), bool)
    if L > 1:
        d = _sub(N[:, 1:], C[:, :-1])
        with np.errstate(all="ignore"):
            link = present[:, :-1] & present[:, 1:] & (np.sqrt(_dot(d, d)) <= break_distance)
        for k, (off, pts) in enumerate(((1, (C[:, :-1], N[:, 1:], CA[:, 1:], C[:, 1:])),
                                        (0, (N[:, :-1], CA[:, :-1], C[:, :-1], N[:, 1:])),
                                        (0, (CA[:, :-1], C[:, :-1], N[:, 1:], CA[:, 1:])))):
            xs, ys, fine = dihedral_xy(*pts)
            fine &= link
            sl = slice(off, L - 1 + off)
            x[k][:, sl], y[k][:, sl], ok[k][:, sl] = np.where(fine, xs, 0.0), np.where(fine, ys, 0.0), fine
    return x, y, ok, present


def torsions(X, mask=None, break_distance: float = BREAK, geometry: bool = False):
    """-> phi, psi, omega f64 (n, L) in radians, NaN where undefined; with geometry also geom f64 (n, L, 6): the lengths N-CA, CA-C,
    C-N(+1) and the angles N-CA-C, CA-C-N(+1), C-N(+1)-CA(+1) in radians, NaN where a residue they touch is absent."""
    x, y, ok, present = xy(X, mask, break_distance)
    ang = np.where(ok, np.arctan2(y, x), np.nan)
    if not geometry:
        return ang[0], ang[1], ang[2]
    c, _ = _prepare(X, mask)
    n, L = present.shape
    N, CA, C = c[:, :, 0], c[:, :, 1], c[:, :, 2]
    geom = np.full((n, L, 6), np.nan)
    with np.errstate(all="ignore"):
        nca, cac = _sub(CA, N), _sub(C, CA)
        geom[:, :, 0] = np.where(present, np.sqrt(_dot(nca, nca)), np.nan)
        geom[:, :, 1] = np.where(present, np.sqrt(_dot(cac, cac)), np.nan)
        geom[:, :, 3] = np.where(present, _bond_angle(N, CA, C), np.nan)
        if L > 1:
            two = present[:, :-1] & present[:, 1:]
            cn = _sub(N[:, 1:], C[:, :-1])
            geom[:, :-1, 2] = np.where(two, np.sqrt(_dot(cn, cn)), np.nan)
            geom[:, :-1, 4] = np.where(two, _bond_angle(CA[:, :-1], C[:, :-1], N[:, 1:]), np.nan)
            geom[:, :-1, 5] = np.where(two, _bond_angle(C[:, :-1], N[:, 1:], CA[:, 1:]), np.nan)
    return ang[0], ang[1], ang[2], geom


def bin_of(angle, bins: int):
    """The cell of angles in radians (every one defined)."""
    deg = np.asarray(angle, np.float64) * DEG
    w = 360.0 / bins
    b = np.floor((deg + 180.0) / w).astype(np.int64)
    b = np.where(b >= bins, b - bins, b)
    return np.where(b < 0, b + bins, b)


def histogram(phi, psi, bins: int):
    """hist i32 (L, bins, bins) of angle arrays (n, L) in radians: the frames in which both are defined (not NaN)."""
    n, L = phi.shape
    hist = np.zeros((L, bins, bins), np.int32)
    both = ~np.isnan(phi) & ~np.isnan(psi)
    f, i = np.nonzero(both)
    np.add.at(hist, (i, bin_of(phi[f, i], bins), bin_of(psi[f, i], bins)), 1)
    return hist


def ordered_sum(terms, defined):
    """terms, defined (n, L): the sum per residue in the published order."""
    n, L = terms.shape
    F = chunk_frames(n, L)
    total = None
    for c in range(chunks(n, L)):
        part, started = np.zeros(L), np.zeros(L, bool)
        for f in range(c * F, min(n, c * F + F)):
            d = defined[f]
            with np.errstate(all="ignore"):
                part = np.where(d, np.where(started, part + terms[f], terms[f]), part)
            started |= d
        total = part if total is None else total + part
    return np.zeros(L) if total is None else total


def ramachandran(X, bins: int, mask=None, break_distance: float = BREAK, sums: bool = True):
    """-> hist i32 (L, bins, bins), counts i32 (L, 5) (phi, psi, both, omega, cis), sums f64 (L, 6) (None without `sums`)."""
    assert 1 <= bins <= MAX_BINS
    x, y, ok, _ = xy(X, mask, break_distance)
    ang = np.where(ok, np.arctan2(y, x), np.nan)
    hist = histogram(ang[0], ang[1], bins)
    cis = ok[2] & (x[2] > 0.0)
    counts = np.stack([ok[0].sum(0), ok[1].sum(0), (ok[0] & ok[1]).sum(0), ok[2].sum(0), cis.sum(0)], axis=1).astype(np.int32)
    out = None
    if sums:
        out = np.zeros((x.shape[2], 6))
        with np.errstate(all="ignore"):
            r = np.sqrt(x * x + y * y)
            co, si = x / r, y / r
        for k in range(3):
            out[:, 2 * k] = ordered_sum(co[k], ok[k])
            out[:, 2 * k + 1] = ordered_sum(si[k], ok[k])
    return hist, counts, out


def js_distance(p, q):
    """scipy.spatial.distance.jensenshannon(p, q) (natural logarithm) in plain numpy, used where scipy is absent."""
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    p, q = p / p.sum(), q / q.sum()
    m = (p + q) / 2.0
    with np.errstate(all="ignore"):
        left = np.where(p > 0, p * np.log(p / m), 0.0)
        right = np.where(q > 0, q * np.log(q / m), 0.0)
    return float(np.sqrt((left.sum() + right.sum()) / 2.0))


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def centred_angles(rng, shape, bins: int = 36, spread: float = 0.4):
    """Angles in degrees at the centres of `bins` cells, moved by at most `spread` cell widths: none near an edge."""
    w = 360.0 / bins
    return -180.0 + (rng.integers(0, bins, shape) + 0.5 + rng.uniform(-spread, spread, shape)) * w


def chains(rng, n: int, L: int, atoms: int = 3, bins: int = 36):
    """n nerf chains of L residues from (phi, psi) centred in the cells of `bins` -> X (n, L, atoms, 3), the prescription (n, L, 2) in
    degrees."""
    pp = centred_angles(rng, (n, L, 2), bins)
    X = np.stack([nerf([tuple(a) for a in pp[k]]) for k in range(n)])
    return np.ascontiguousarray(X[:, :, :atoms]), pp

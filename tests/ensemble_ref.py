"""TEST INFRASTRUCTURE — float64 numpy restatement of the two kernels of esmdiff_amd/csrc/superpose.hip.

superpose_pair / superpose_pairs: the least-squares superposition through numpy's SVD, under both rotation rules
(allow_reflection = True: R = V U^T of the SVD of the covariance with no determinant correction, the reference's
slm/utils/geo_utils.py:91-122; False: the proper rotation, scipy's Rotation.align_vectors).  PINNED by
tests/golden/g13_superposition.npz, which the reference's own functions and scipy wrote (tests/test_ensemble_cpu.py).

tm_pair / tm_matrix: the TM-score with the fixed residue-to-residue correspondence.  [TMSCORE-RECALL], PARITY UNPINNED:
the maximisation is the TMscore program's fragment-seeded search restated from memory; the rule below is the one
DESIGN.md ("Superposition") states, line by line, and the kernel implements the same one:

  aligned set   residues valid in both structures, La of them, in residue order; Ln = valid residues of the native.
                La < 2: NaN.
  d0            max(0.5, 1.24 cbrt(Ln - 15) - 1.8); d0_search = clamp(d0, 4.5, 8).
  score(R, t)   (1 / Ln) sum over the aligned residues of 1 / (1 + d_i^2 / d0^2), d_i = |R a_i + t - b_i|.
  select(c)     the aligned residues with d_i^2 < c^2; while fewer than min(3, La) are selected, c += 0.5 and select again
                (after 16384 widenings the seed is abandoned: non-finite coordinates).
  lengths       l = La; while l > min(4, La): take l, l = l // 2; last, take min(4, La).
  seeds         for every length in that order, for every start 0 .. La - length (step 1): the residues start .. start + length - 1.
  one seed      S = the fragment.  Iteration 0: proper Kabsch on S, score, S' = select(d0_search - 1).  Iterations 1 .. 20: proper
                Kabsch on S', score, S'' = select(d0_search + 1); stop if S'' = S', else S' = S''.
  result        the largest score of any iteration of any seed; ties go to the earliest (length, start), then iteration.

The seeds of one pair are advanced together as one batch (batched SVD): the same rule, not one Python loop per seed."""
from __future__ import annotations

import numpy as np

MAX_WIDEN = 16384


def _masks(a, b, mask_a, mask_b):
    ma = np.ones(len(a), bool) if mask_a is None else np.asarray(mask_a, bool)
    mb = np.ones(len(b), bool) if mask_b is None else np.asarray(mask_b, bool)
    return ma, mb


def kabsch(x: np.ndarray, y: np.ndarray, allow_reflection: bool):
    """x, y (N, 3) -> R (3, 3), t (3,) with R x_i + t ~ y_i."""
    cx, cy = x.mean(0), y.mean(0)
    H = (x - cx).T @ (y - cy)
    U, S, Vt = np.linalg.svd(H)
    V = Vt.T.copy()
    R = V @ U.T
    # the bare V U^T carries the sign of det H; where the smallest singular value vanishes (planar, collinear points) that sign is
    # the SVD's whim and both choices move the points alike: the proper one is taken, as the kernel does
    if (not allow_reflection or S[2] <= 1e-10 * S[0]) and np.linalg.det(R) < 0:
        V[:, 2] = -V[:, 2]
        R = V @ U.T
    return R, cy - R @ cx


def superpose_pair(a, b, mask_a=None, mask_b=None, allow_reflection=False):
    """-> rmsd, sd (L,) NaN where masked, R, t; everything NaN with fewer than 2 aligned residues."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ma, mb = _masks(a, b, mask_a, mask_b)
    ali = ma & mb
    sd = np.full(len(a), np.nan)
    if ali.sum() < 2:
        return np.nan, sd, np.full((3, 3), np.nan), np.full(3, np.nan)
    R, t = kabsch(a[ali], b[ali], allow_reflection)
    sd[ali] = ((a[ali] @ R.T + t - b[ali]) ** 2).sum(-1)
    return float(np.sqrt(sd[ali].mean())), sd, R, t


def superpose_pairs(A, B=None, mask_a=None, mask_b=None, allow_reflection=False):
    """A (n, L, 3), B (m, L, 3) or None (A against itself) -> rmsd (n, m), sd (n, m, L), R (n, m, 3, 3), t (n, m, 3)."""
    A = np.asarray(A, np.float64)
    if B is None:
        B, mask_b = A, mask_a
    B = np.asarray(B, np.float64)
    n, m, L = len(A), len(B), A.shape[1]
    rmsd, sd, R, t = np.empty((n, m)), np.empty((n, m, L)), np.empty((n, m, 3, 3)), np.empty((n, m, 3))
    for i in range(n):
        for j in range(m):
            rmsd[i, j], sd[i, j], R[i, j], t[i, j] = superpose_pair(
                A[i], B[j], None if mask_a is None else mask_a[i], None if mask_b is None else mask_b[j], allow_reflection)
    return rmsd, sd, R, t


def aligned_deviation_pair(a, b, mask_a=None, mask_b=None):
    """The per-residue distances of analysis/apo_analysis.py:235 after get_structures (:201-208): each structure centred on the mean
    of its OWN valid residues, then a rotation-only proper fit on the residues valid in both.  The rotation-only fit is stated the
    way esmdiff_amd.ensemble.aligned_deviation hands it to the kernel: the Kabsch fit of [x, -x] onto [y, -y]."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ma, mb = _masks(a, b, mask_a, mask_b)
    ma, mb = ma & ~np.isnan(a).any(-1), mb & ~np.isnan(b).any(-1)
    ac, bc = a - a[ma].mean(0), b - b[mb].mean(0)
    _, sd, _, _ = superpose_pair(np.concatenate([ac, -ac]), np.concatenate([bc, -bc]), np.concatenate([ma, ma]),
                                 np.concatenate([mb, mb]), allow_reflection=False)
    return np.sqrt(sd[:len(a)])


# ---- TM-score --------------------------------------------------------------------------------------------------------
def tm_d0(Ln: int):
    d0 = max(0.5, 1.24 * float(np.cbrt(Ln - 15.0)) - 1.8)
    return d0, min(max(d0, 4.5), 8.0)


def fragment_lengths(La: int):
    lmin, out, l = min(4, La), [], La
    while l > lmin:
        out.append(l)
        l //= 2
    return out + [lmin]


def _kabsch_batch(x, y, sel):
    """Proper Kabsch of every row of sel (S, La) bool on x, y (La, 3) -> R (S, 3, 3), t (S, 3)."""
    w = sel.astype(np.float64)
    N = w.sum(-1, keepdims=True)
    cx, cy = (w @ x) / N, (w @ y) / N
    xs = (x[None] - cx[:, None]) * w[..., None]
    ys = y[None] - cy[:, None]
    H = np.einsum("sli,slj->sij", xs, ys)
    U, _, Vt = np.linalg.svd(H)
    V = np.swapaxes(Vt, -1, -2).copy()
    V[:, :, 2] *= np.sign(np.linalg.det(V @ np.swapaxes(U, -1, -2)))[:, None]
    R = V @ np.swapaxes(U, -1, -2)
    return R, cy - np.einsum("sij,sj->si", R, cx)


def _dist2(x, y, R, t):
    return ((np.einsum("sij,lj->sli", R, x) + t[:, None] - y[None]) ** 2).sum(-1)


def tm_pair(a, b, mask_a=None, mask_b=None):
    """TM-score of model a against native b (both (L, 3)) -> tm, R, t of the best superposition found."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ma, mb = _masks(a, b, mask_a, mask_b)
    ali = ma & mb
    La, Ln = int(ali.sum()), int(mb.sum())
    if La < 2:
        return np.nan, np.full((3, 3), np.nan), np.full(3, np.nan)
    x, y = a[ali], b[ali]
    d0, d0s = tm_d0(Ln)
    need = min(3, La)
    sel = np.array([[start <= i < start + length for i in range(La)]
                    for length in fragment_lengths(La) for start in range(La - length + 1)])
    S = len(sel)
    best, best_R, best_t = np.full(S, -1.0), np.zeros((S, 3, 3)), np.zeros((S, 3))
    active = np.arange(S)
    for it in range(21):
        cur = sel[active]
        R, t = _kabsch_batch(x, y, cur)
        d2 = _dist2(x, y, R, t)
        sc = (1.0 / (1.0 + d2 / (d0 * d0))).sum(-1) / Ln
        up = sc > best[active]                                   # strict: the earliest iteration keeps a tie
        best[active[up]], best_R[active[up]], best_t[active[up]] = sc[up], R[up], t[up]
        cut = np.full(len(active), d0s - 1.0 if it == 0 else d0s + 1.0)
        nsel = d2 < (cut * cut)[:, None]
        for _ in range(MAX_WIDEN):
            short = nsel.sum(-1) < need
            if not short.any():
                break
            cut[short] += 0.5
            nsel[short] = d2[short] < (cut[short] ** 2)[:, None]
        keep = nsel.sum(-1) >= need
        if it > 0:
            keep &= (nsel != cur).any(-1)
        sel[active] = nsel
        active = active[keep]
        if len(active) == 0:
            break
    g = int(np.argmax(best))                                     # the first maximum: the earliest (length, start)
    return float(best[g]), best_R[g], best_t[g]


def tm_matrix(A, B=None, mask_a=None, mask_b=None):
    """models A (n, L, 3) against natives B (m, L, 3) (None: A against itself) -> (n, m)."""
    A = np.asarray(A, np.float64)
    if B is None:
        B, mask_b = A, mask_a
    B = np.asarray(B, np.float64)
    return np.array([[tm_pair(A[i], B[j], None if mask_a is None else mask_a[i], None if mask_b is None else mask_b[j])[0]
                      for j in range(len(B))] for i in range(len(A))])


def tm_at(a, b, R, t, mask_a=None, mask_b=None):
    """The TM sum of model a against native b at a given superposition (no search)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ma, mb = _masks(a, b, mask_a, mask_b)
    ali = ma & mb
    d0, _ = tm_d0(int(mb.sum()))
    d2 = ((a[ali] @ np.asarray(R).T + t - b[ali]) ** 2).sum(-1)
    return float((1.0 / (1.0 + d2 / (d0 * d0))).sum() / mb.sum())


def tm_at_kabsch(a, b, mask_a=None, mask_b=None):
    """The TM sum at the global least-squares (proper Kabsch) superposition of the aligned residues: a lower bound of tm_pair."""
    _, _, R, t = superpose_pair(a, b, mask_a, mask_b, allow_reflection=False)
    return tm_at(a, b, R, t, mask_a, mask_b)


# ---- seeded test structures (shared by the CPU and GPU tests) ---------------------------------------------------------
def random_rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def ca_chain(rng, L):
    """A random-walk CA trace with 3.8 A steps."""
    step = rng.normal(size=(L, 3))
    return np.cumsum(3.8 * step / np.linalg.norm(step, axis=-1, keepdims=True), axis=0)


def ensemble(rng, n, L, noise=1.5):
    """n rigidly moved, perturbed copies of one chain: (n, L, 3)."""
    base = ca_chain(rng, L)
    return np.stack([(base + rng.normal(size=(L, 3)) * noise) @ random_rotation(rng).T + rng.normal(size=3) * 20 for _ in range(n)])


def core_case(rng, L=100, frac=0.6):
    """frac of the residues rigidly moved exactly, the rest thrown 30-50 A away: the global Kabsch fit is dragged off the core."""
    a = ca_chain(rng, L)
    b = a @ random_rotation(rng).T + rng.normal(size=3) * 20
    k = int(round(frac * L))
    d = rng.normal(size=(L - k, 3))
    b[k:] += d / np.linalg.norm(d, axis=-1, keepdims=True) * rng.uniform(30, 50, size=(L - k, 1))
    return a, b

"""TEST INFRASTRUCTURE — NumPy float64 restatement of esmdiff_amd/csrc/contacts.hip: the contact maps of an ensemble
with the device's order of summation, the native-contact counts, and the host layer of esmdiff_amd/contacts.py on top of them.  Integer
outputs are held exactly, the two sums of the maps bit for bit.

  a distance             sqrt((dx dx + dy dy) + dz dz), each operation rounded once (no FMA), numpy's correctly rounded sqrt
  contact_map            per pair |a - b| >= min_sep, V = the frames with both residues valid (mask, and no NaN coordinate):
                         valid = |V|, count = #{i in V : d_i < cutoff} (strict), sum_d = sum of d_i, sum_d2 = sum of the square root's
                         argument.  ORDER: chunks of chunk_frames(n, L) consecutive frames; inside a chunk frame after frame from the
                         first, an invalid frame adding nothing; then the chunk sums in increasing chunk index from chunk 0's.
  native contacts        C_j = ordered (a, b): |a - b| >= min_sep, both valid in B[j], d0 < cutoff (strict); total[j] = |C_j|;
                         kept[i, j] = #{(a, b) in C_j : both valid in A[i], d_i < lam d0} (strict, one product); per residue a alike;
                         q_soft[i, j] = sum over C_j of 1 / (1 + exp(beta (d_i - lam d0))), 0 for a missing model residue.
                         ORDER of q_soft: the k-th contact of row a (increasing b) goes to lane k % 64, which adds its terms in
                         increasing k; the lanes are combined by the xor butterfly 32, 16 .. 1; wave w adds the rows a = w, w + 8 ...;
                         the eight wave sums are ((w0 + w1) + (w2 + w3)) + ((w4 + w5) + (w6 + w7))."""
from __future__ import annotations

import numpy as np

CUTOFF, MIN_SEP, LAMBDA, BETA = 8.0, 3, 1.2, 5.0
TILE, MAX_CHUNKS, MAX_L = 64, 256, 4096


# ---- the header's macros ------------------------------------------------------------------------------------------------------------
def pair_tiles(L: int) -> int:
    t = (L + TILE - 1) // TILE
    return t * (t + 1) // 2


def chunk_frames(n: int, L: int) -> int:
    cap = min(MAX_CHUNKS, max(1, 1024 // pair_tiles(L)))
    return max(16, -(-n // cap))


def chunks(n: int, L: int) -> int:
    return -(-n // chunk_frames(n, L))


def scratch_bytes(n: int, L: int) -> int:
    c = chunks(n, L)
    return 0 if c == 1 else c * pair_tiles(L) * TILE * TILE * 24


# ---- distances ----------------------------------------------------------------------------------------------------------------------
def squared_distances(x) -> np.ndarray:
    """(L, 3) -> (L, L): (dx dx + dy dy) + dz dz"""
    x = np.asarray(x, np.float64)
    d = x[None, :, :] - x[:, None, :]
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def distances(x) -> np.ndarray:
    return np.sqrt(squared_distances(x))


def _valid(X, mask):
    ok = ~np.isnan(X).any(-1)
    return ok if mask is None else ok & np.asarray(mask).astype(bool)


# ---- contact maps -------------------------------------------------------------------------------------------------------------------
def contact_map(X, mask=None, cutoff: float = CUTOFF, min_sep: int = MIN_SEP):
    """X (n, L, 3) -> valid, count int64 (L, L), sum_d, sum_d2 float64 (L, L), in the device's order."""
    X = np.asarray(X, np.float64)
    n, L = X.shape[:2]
    assert n >= 1 and L >= 2 and min_sep >= 1
    ok = _valid(X, mask)
    idx = np.arange(L)
    far = np.abs(idx[:, None] - idx[None, :]) >= min_sep
    per = chunk_frames(n, L)
    valid, count = np.zeros((L, L), np.int64), np.zeros((L, L), np.int64)
    sum_d = sum_d2 = None
    with np.errstate(invalid="ignore"):
        for f0 in range(0, n, per):
            part_d, part_d2 = np.zeros((L, L)), np.zeros((L, L))
            for f in range(f0, min(n, f0 + per)):
                both = ok[f][:, None] & ok[f][None, :]
                d2 = squared_distances(X[f])
                d = np.sqrt(d2)
                valid += both
                count += both & (d < cutoff)
                part_d[both] += d[both]
                part_d2[both] += d2[both]
            sum_d, sum_d2 = (part_d, part_d2) if sum_d is None else (sum_d + part_d, sum_d2 + part_d2)
    return valid * far, count * far, np.where(far, sum_d, 0.0), np.where(far, sum_d2, 0.0)


def frequency(valid, count):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(valid > 0, count / valid, np.nan)


def per_frame(valid, total):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(valid > 0, total / valid, np.nan)


def contact_error(ensembles, ref_key: str = "target", pwd_offset: int = 3):
    """(mse_contact, mae_contact, mse_pwd, mae_pwd) of eval_utils.idp_metrics, through the maps."""
    def stats(ca):
        valid, count, sum_d, _ = contact_map(ca, None, 8.0, pwd_offset)
        iu = np.triu_indices(valid.shape[0], pwd_offset)
        return np.log(frequency(valid, count)[iu] + 0.01), per_frame(valid, sum_d)[iu]

    ref = stats(ensembles[ref_key])
    out = tuple({} for _ in range(4))
    for name, ca in ensembles.items():
        cur = stats(ca)
        for j in range(2):
            diff = cur[j] - ref[j]
            out[2 * j][name] = float(np.mean(diff ** 2))
            out[2 * j + 1][name] = float(np.mean(np.abs(diff)))
    return out


# ---- native contacts ----------------------------------------------------------------------------------------------------------------
def _butterfly(v):
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[lanes ^ off]
    return v[0]


def native_contacts(A, B=None, maskA=None, maskB=None, cutoff: float = CUTOFF, min_sep: int = MIN_SEP, lam: float = LAMBDA,
                    beta: float = BETA):
    """A (n, L, 3), B (m, L, 3) (None: A against itself, maskB = maskA) -> kept (n, m), total (m,), kept_res (n, m, L),
    total_res (m, L) int64, q_soft (n, m) float64 in the device's order."""
    A = np.asarray(A, np.float64)
    if B is None:
        B, maskB = A, maskA
    B = np.asarray(B, np.float64)
    n, L = A.shape[:2]
    m = B.shape[0]
    assert B.shape[1] == L and min_sep >= 1
    okA = np.ones((n, L), bool) if maskA is None else np.asarray(maskA).astype(bool)
    okB = np.ones((m, L), bool) if maskB is None else np.asarray(maskB).astype(bool)
    idx = np.arange(L)
    far = np.abs(idx[:, None] - idx[None, :]) >= min_sep
    kept_res, total_res = np.zeros((n, m, L), np.int64), np.zeros((m, L), np.int64)
    q_soft = np.zeros((n, m))
    with np.errstate(invalid="ignore", over="ignore"):
        dA = [distances(a) for a in A]
        for j in range(m):
            d0 = distances(B[j])
            pairs = far & okB[j][:, None] & okB[j][None, :] & (d0 < cutoff)
            ld = lam * d0
            total_res[j] = pairs.sum(1)
            for i in range(n):
                both = pairs & okA[i][:, None] & okA[i][None, :]
                kept_res[i, j] = (both & (dA[i] < ld)).sum(1)
                term = np.where(both, 1.0 / (1.0 + np.exp(beta * (dA[i] - ld))), 0.0)
                waves = np.zeros(8)
                for a in range(L):
                    t = term[a][pairs[a]]                                  # the row's contacts in increasing b
                    lanes = np.zeros(64)
                    for k0 in range(0, len(t), 64):
                        lanes[:len(t) - k0] += t[k0:k0 + 64]
                    waves[a % 8] += _butterfly(lanes)
                q_soft[i, j] = ((waves[0] + waves[1]) + (waves[2] + waves[3])) + ((waves[4] + waves[5]) + (waves[6] + waves[7]))
    return kept_res.sum(-1), total_res.sum(-1), kept_res, total_res, q_soft


def q(A, B=None, maskA=None, maskB=None, **kw):
    """-> hard Q (n, m), soft Q (n, m), per-residue hard Q (n, m, L); NaN where a native (a residue) has no contact."""
    kept, total, kept_res, total_res, q_soft = native_contacts(A, B, maskA, maskB, **kw)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (np.where(total[None] > 0, kept / total[None], np.nan), np.where(total[None] > 0, q_soft / total[None], np.nan),
                np.where(total_res[None] > 0, kept_res / total_res[None], np.nan))


# ---- the host layer -----------------------------------------------------------------------------------------------------------------
def contact_switches(S, t1, t2, cutoff: float = CUTOFF, min_sep: int = MIN_SEP):
    """-> [(a, b, state, frequency or None)] for the pairs a < b valid in both targets and in contact in exactly one."""
    valid, count, _, _ = contact_map(S, None, cutoff, min_sep)
    freq = frequency(valid, count)
    m1, m2 = (contact_map(np.asarray(t, np.float64).reshape(1, -1, 3), None, cutoff, min_sep) for t in (t1, t2))
    pick = np.triu((m1[0] > 0) & (m2[0] > 0) & ((m1[1] > 0) != (m2[1] > 0)), 1)
    return [(int(a), int(b), 1 if m1[1][a, b] > 0 else 2, None if np.isnan(freq[a, b]) else float(freq[a, b]))
            for a, b in zip(*np.nonzero(pick))]


def internal_scaling(S, mask=None):
    """-> separation (L - 1,), rms distance (L - 1,)"""
    valid, _, _, sum_d2 = contact_map(S, mask, CUTOFF, 1)
    msd = per_frame(valid, sum_d2)
    L = msd.shape[0]
    rms = np.full(L - 1, np.nan)
    for s in range(1, L):
        d = np.diagonal(msd, s)
        if np.isfinite(d).any():
            rms[s - 1] = np.sqrt(np.nanmean(d))
    return np.arange(1, L), rms


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def line(xs) -> np.ndarray:
    """CA atoms along the x axis, (L, 3)."""
    return np.stack([np.asarray(xs, np.float64), np.zeros(len(xs)), np.zeros(len(xs))], axis=1)


def chain(rng, L: int) -> np.ndarray:
    """A random walk of 3.8 A steps, (L, 3): compact enough to have contacts at every sequence separation."""
    steps = rng.normal(size=(L, 3))
    steps *= 3.8 / np.linalg.norm(steps, axis=1, keepdims=True)
    return np.cumsum(steps, axis=0)


def ensemble(rng, k: int, base: np.ndarray, lo: float = 0.2, hi: float = 2.0) -> np.ndarray:
    """k copies of `base` with Gaussian noise of a standard deviation spread from lo to hi Angstrom, (k, L, 3): contacts that form in some
    frames and not in others."""
    sigma = (np.linspace(lo, hi, k) if k > 1 else np.array([hi]))[:, None, None]
    return base[None] + sigma * rng.normal(size=(k,) + base.shape)

"""TEST INFRASTRUCTURE — inputs that sit on the edges of esmdiff_amd/csrc/metrics.hip, plain numpy.  The reference of every VALUE is
oracle/metrics_ref.py (pinned to the reference project's outputs by g9 / g9b); nothing here restates it.  What is here:

  edge_lattice_columns   columns whose values are the bin edges of their own histogram and the doubles next to them, with values outside
                         the range, infinities and a NaN on the model side
  histogram_fused_edge,  two DELIBERATELY WRONG histograms (tests/test_metrics_edges_cpu.py only): what col_hist_kernel would compute
  histogram_uncorrected  if `i * step + first` were contracted to one rounding, and if the edge correction were missing
  bar_chain, bent_chain  straight CA chains with ONE pair / ONE bond at an exactly representable distance (validity's bar, bonding
                         validity's threshold): the moved atom leaves the axis at a right angle, so the distance is sqrt(d * d) == d
  long ensembles         more frames than one grid extent holds, every distinguishing frame at an index >= TAIL_START"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

SPACING = 3.8                    # validity's chains (the CA - CA distance)
BOND = 3.75                      # bonding validity's chains: BOND * i is exact, so every other bond is exactly BOND
N_LONG, TAIL_START = 70000, 65600
LATTICE_BINS, LATTICE_DS = (1, 3, 7, 50), (1, 255, 256, 257, 600)      # the (n_bins, D) grid of the device test
LATTICE_SEEDS = {(3, 1): 3003}                                         # (n_bins, D) -> seed, where the default one does not bite


def lattice_seed(n_bins: int, D: int) -> int:
    return LATTICE_SEEDS.get((n_bins, D), 1000 * n_bins + D)


# ---- histogram edges ----------------------------------------------------------------------------------------------------------------
def lattice(first: float, last: float, n_bins: int) -> np.ndarray:
    """numpy.histogram's own edges and the doubles next to them, (3 (n_bins + 1),): two of them lie one ulp outside [first, last]."""
    edges = np.linspace(first, last, n_bins + 1)
    return np.concatenate([edges, np.nextafter(edges, np.inf), np.nextafter(edges, -np.inf)])


def model_rows(n_bins: int) -> int:
    return 3 * (n_bins + 1) + 8 + 5


def model_column(rng, first: float, last: float, n_bins: int) -> np.ndarray:
    """The whole lattice and eight in-range values in random order; then, in the same five rows of every column, two values far
    outside the range, +inf, -inf and NaN (the NaN is the last row: frame model_rows(n_bins) - 1 is dropped from every column)."""
    width = last - first
    body = np.concatenate([lattice(first, last, n_bins), rng.uniform(first, last, 8)])
    rng.shuffle(body)
    return np.concatenate([body, [first - 10.0 * width, last + 7.0 * width, np.inf, -np.inf, np.nan]])


def edge_lattice_columns(n_bins: int, D: int, seed: int):
    """-> model (3 (n_bins + 1) + 13, D), ref (3 (n_bins + 1) + 2, D).  Each column has its own (lo, hi); the ref column holds lo, hi and
    a random subset of the lattice inside [lo, hi], padded by repeating values it already holds; the model column is model_column()."""
    rng = np.random.default_rng(seed)
    n_ref = 3 * (n_bins + 1) + 2
    model, ref = np.empty((model_rows(n_bins), D)), np.empty((n_ref, D))
    for d in range(D):
        lo = rng.uniform(-40.0, 40.0)
        hi = lo + rng.uniform(0.05, 30.0)
        lat = lattice(lo, hi, n_bins)
        lat = lat[(lat >= lo) & (lat <= hi)]
        col = np.concatenate([[lo, hi], lat[rng.random(lat.size) < 0.6]])
        col = np.concatenate([col, rng.choice(col, n_ref - col.size)])
        rng.shuffle(col)
        ref[:, d] = col
        model[:, d] = model_column(rng, lo, hi, n_bins)
    return model, ref


def widened_columns(n_bins: int, D: int, seed: int):
    """One reference frame: lo == hi in every column, the range becomes (c - 0.5, c + 0.5).  -> model on that range's lattice, ref (1, D)."""
    rng = np.random.default_rng(seed)
    ref = rng.uniform(-40.0, 40.0, (1, D))
    model = np.stack([model_column(rng, c - 0.5, c + 0.5, n_bins) for c in ref[0]], axis=1)
    return model, ref


def outside_columns(n_bins: int, D: int, seed: int):
    """The edge lattice's reference; every model value of column 0 lies above the range, of column D - 1 below it (only the pseudo count
    is left there)."""
    model, ref = edge_lattice_columns(n_bins, D, seed)
    model = model[:-3].copy()                                    # finite rows only
    model[:, 0] = ref[:, 0].max() + 1.0 + np.arange(model.shape[0])
    model[:, -1] = ref[:, -1].min() - 1.0 - np.arange(model.shape[0])
    return model, ref


def lattice_weights(n_model: int, n_ref: int, seed: int):
    """Per-frame weights: every fourth one 0, and a LARGE weight on the model's last frame — the NaN of every column, which is dropped."""
    rng = np.random.default_rng(seed)
    wm, wr = rng.uniform(0.5, 1.5, n_model), rng.uniform(0.5, 1.5, n_ref)
    wm[1::4] = 0.0
    wr[2::4] = 0.0
    wm[-1] = 1000.0
    return wm, wr


def _histogram(x, n_bins, first, last, weights, edges_of, correct):
    if first == last:
        first, last = first - 0.5, last + 0.5
    edges = edges_of(n_bins, (last - first) / n_bins, first)
    edges[-1] = last
    inside = (x >= first) & (x <= last)
    weights = None if weights is None else np.asarray(weights, dtype=np.float64)[inside]
    x = x[inside]
    idx = (((x - first) / (last - first)) * n_bins).astype(np.intp)
    idx[idx == n_bins] -= 1
    if correct:
        idx[x < edges[idx]] -= 1
        idx[(x >= edges[idx + 1]) & (idx != n_bins - 1)] += 1
    return np.bincount(idx, weights=weights, minlength=n_bins).astype(np.float64)


def _fused_edges(n_bins, step, first):
    """i * step + first rounded ONCE (what a fused multiply-add returns)."""
    return np.array([float(Fraction(i) * Fraction(step) + Fraction(first)) for i in range(n_bins + 1)])


def _plain_edges(n_bins, step, first):
    return np.arange(0, n_bins + 1) * step + first


def histogram_fused_edge(x, n_bins, first, last, weights=None):
    """WRONG ON PURPOSE: the edge correction compares with the correctly rounded i * step + first.  It can differ from numpy only where
    i * step is inexact: never for n_bins <= 3 (the inner edges are i = 1, 2, and edge n_bins is `last` itself)."""
    return _histogram(x, n_bins, first, last, weights, _fused_edges, True)


def histogram_uncorrected(x, n_bins, first, last, weights=None):
    """WRONG ON PURPOSE: the truncated index is used as it is.  It cannot differ for n_bins == 1 (every value goes to bin 0)."""
    return _histogram(x, n_bins, first, last, weights, _plain_edges, False)


def flipped_columns(model, ref, n_bins, wrong) -> int:
    """The columns in which `wrong` puts a value of model or ref into another bin than numpy.histogram does."""
    n = 0
    for d in range(ref.shape[1]):
        lo, hi = ref[:, d].min(), ref[:, d].max()
        with np.errstate(invalid="ignore"):
            n += any(not np.array_equal(wrong(x[:, d], n_bins, lo, hi), np.histogram(x[:, d], bins=n_bins, range=(lo, hi))[0])
                     for x in (model, ref))
    return n


# ---- distances ----------------------------------------------------------------------------------------------------------------------
PWD_FRAMES = 16
PWD_CASES = sorted({(L, k) for L in (2, 23, 24) for k in (0, 1, 3, L - 1)})       # k >= L: no pair, the entry refuses


def full_mantissa_coords(n: int, L: int, seed: int) -> np.ndarray:
    """(n, L, 3) coordinates with all 53 bits in use: dx dx, dy dy and dz dz are inexact, a contracted sum rounds differently."""
    return np.random.default_rng(seed).normal(size=(n, L, 3)) * 11.0


def pwd_contracted(coords: np.ndarray, k: int) -> np.ndarray:
    """WRONG ON PURPOSE: sqrt(fma(dz, dz, fma(dy, dy, dx dx))), the sum a compiler contracts (dx dx + dy dy) + dz dz to."""
    L = coords.shape[-2]
    row, col = np.triu_indices(L, k=k)
    d = coords[..., col, :] - coords[..., row, :]
    flat = d.reshape(-1, 3)
    out = np.empty(len(flat))
    for i, (dx, dy, dz) in enumerate(flat):
        inner = float(Fraction(dy) * Fraction(dy) + Fraction(dx * dx))
        out[i] = float(Fraction(dz) * Fraction(dz) + Fraction(inner))
    return np.sqrt(out).reshape(d.shape[:-1])


def pair_index(L: int, k: int, i: int, j: int) -> int:
    """The column of the pair (i, j) in numpy.triu_indices(L, k) order."""
    row, col = np.triu_indices(L, k=k)
    return int(np.nonzero((row == i) & (col == j))[0][0])


# ---- validity's bar -----------------------------------------------------------------------------------------------------------------
def straight_chain(L: int, spacing: float = SPACING) -> np.ndarray:
    x = np.zeros((L, 3))
    x[:, 0] = spacing * np.arange(L)
    return x


def bar_chain(L: int, i: int, j: int, dist: float, n: int = 1, frames=None) -> np.ndarray:
    """n straight chains along x (SPACING apart); in `frames` (default: all) atom j sits at atom i's x, `dist` up the y axis: the pair
    (i, j) is at sqrt(dist * dist) == dist, every other pair of the frame is farther than SPACING apart."""
    ca = np.repeat(straight_chain(L)[None], n, axis=0)
    frames = range(n) if frames is None else frames
    for f in frames:
        ca[f, j] = (ca[f, i, 0], dist, 0.0)
    return ca


def below(x: float) -> float:
    return float(np.nextafter(x, 0.0))


# ---- bonding validity's threshold ---------------------------------------------------------------------------------------------------
def bent_chain(L: int, bond: int = -1, length: float = BOND) -> np.ndarray:
    """(L, 3): a chain along x with exact bonds of BOND; bond `bond` (atoms bond, bond + 1) instead runs up the y axis and is exactly
    `length` long (0 - length and length - length are exact, whatever x is).  bond = -1: no such bond."""
    ca = np.zeros((L, 3))
    steps = np.full(L - 1, BOND)
    if bond >= 0:
        steps[bond] = 0.0
        ca[bond + 1:, 1] = length
    ca[1:, 0] = np.cumsum(steps)
    return ca


def bonding_case(L: int, bond: int, length: float):
    """-> model (3, L, 3), ref (3, L, 3).  The ref's longest bond (3.875) is the LAST bond of its LAST frame.  The model has a plain frame,
    a frame with a bond of 3.8125 at `bond` (valid only if that longest bond was seen) and a frame with a bond of `length` at `bond`."""
    ref = np.stack([bent_chain(L), bent_chain(L), bent_chain(L, L - 2, 3.875)])
    model = np.stack([bent_chain(L), bent_chain(L, bond, 3.8125), bent_chain(L, bond, length)])
    return model, ref


def bonding_threshold() -> float:
    return 3.875 + 1e-6


# ---- more frames than one grid extent (n = N_LONG, L = 4) ----------------------------------------------------------------------------
TAIL_CLASHES = (TAIL_START, TAIL_START + 1, 67003, N_LONG - 1)       # frames; every one >= TAIL_START, the last frame among them


def long_validity_ensemble() -> np.ndarray:
    """N_LONG straight chains of 4 atoms; the frames TAIL_CLASHES have the pair (0, 2) just below the default bar."""
    return bar_chain(4, 0, 2, below(3.0), N_LONG, TAIL_CLASHES)


def long_bonding_model() -> np.ndarray:
    """N_LONG chains of 4 atoms; the frames TAIL_CLASHES have bond 2 exactly at bonding_threshold() (not below it: broken)."""
    ca = np.repeat(bent_chain(4)[None], N_LONG, axis=0)
    ca[list(TAIL_CLASHES)] = bent_chain(4, 2, bonding_threshold())
    return ca


def long_bonding_ref() -> np.ndarray:
    """N_LONG chains of 4 atoms whose longest bond (3.875) is the last bond of the last frame."""
    ca = np.repeat(bent_chain(4)[None], N_LONG, axis=0)
    ca[-1] = bent_chain(4, 2, 3.875)
    return ca


def walk_ensemble(n: int, seed: int, scale: float = 1.0, noise: float = 0.3) -> np.ndarray:
    """n noisy copies of one 4-atom random walk, stretched by `scale`."""
    rng = np.random.default_rng(seed)
    steps = np.random.default_rng(99).normal(size=(4, 3)) + np.array([2.0, 0, 0])
    base = np.cumsum(SPACING * steps / np.linalg.norm(steps, axis=-1, keepdims=True), 0)
    return scale * base[None] + rng.normal(size=(n, 4, 3)) * noise


def short_js_ensemble(seed: int) -> np.ndarray:
    """300 frames, the last one stretched so far that, as the reference, its ranges hold every frame of long_js_ensemble()."""
    return np.concatenate([walk_ensemble(299, seed, 1.1), walk_ensemble(1, seed + 1, 3.0, 0.0)])


def long_js_ensemble(seed: int) -> np.ndarray:
    """N_LONG frames; the frames from TAIL_START on (the last frame among them) come from a stretched, noisier distribution, the last
    frame stretched the most (it alone sets the upper end of every distance's range)."""
    ca = walk_ensemble(N_LONG, seed)
    ca[TAIL_START:] = walk_ensemble(N_LONG - TAIL_START, seed + 1, 1.25, 0.6)
    ca[-1] = walk_ensemble(1, seed + 2, 2.5, 0.0)[0]
    return ca

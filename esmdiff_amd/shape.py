"""Size, shape and scattering of ensembles on the device: the gyration tensor and its shape descriptors, the end-to-end distance, the
maximum dimension, the hydrodynamic radius, the pair-distance distribution p(r) and the SAXS intensity by the Debye equation.

The layer above csrc/shape.hip.  Two entries carry everything here:

  esmdiff_shape_frames  per frame the number of valid residues, the centroid, the six sums of (r - c)(r - c)^T about it, the sum of
                        1 / d over pairs, the largest d and the end-to-end distance; and, on request, the histogram of all pair
                        distances of the ensemble.  Memory is O(n + bins): no (n, L, L) distance array exists.
  esmdiff_debye_frames  I_i(q) = sum_a f_a^2 + 2 sum_{a<b} f_a f_b sin(q d_ab) / (q d_ab) for every frame and q.  Memory is O(n Q): no
                        (n, pairs, Q) array exists.

Every definition is closed and rests on no recalled program.  Integer outputs are held exactly to the numpy restatement
tests/shape_ref.py, the sums bit for bit, the Debye intensity to 1e-13 of its envelope.  Form factors are a parameter (point scatterers
by default, sphere_form_factor for a bead model): no residue table is recalled from memory.

  frames                 an ensemble -> ShapeFrames (rg, eigenvalues, asphericity, acylindricity, anisotropy, ree, dmax, rh)
  distance_distribution  the ensemble's p(r)
  debye                  the (n, Q) intensities;  saxs_profile: their (weighted) mean over frames
  sphere_form_factor, guinier_rg, kratky, chi2
  js_shape               the Jensen-Shannon distance between ensembles' distributions of each descriptor, js_rg's conventions
  report, saxs_report    the "shape" and "saxs" blocks of `python -m esmdiff_amd.analyze_ensemble --shape --saxs`

Inputs follow esmdiff_amd/ensemble.py: CA coordinates in Angstrom, arrays, tensors or a PDB path, (L, 3) or (n, L, 3); a residue with a
NaN coordinate is absent in that frame, `mask` (n, L) or (L,) removes more.  q is in 1 / Angstrom.  Results are numpy arrays and floats
on the host.  There is no CPU fallback."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _native as N
from . import pairs
from .metrics import js_columns

QUANTITIES = ("rg", "asphericity", "acylindricity", "anisotropy", "ree", "dmax", "rh")


@dataclass
class ShapeFrames:
    """Per frame, over its valid residues; NaN where a frame has too few of them for the quantity (none: everything; one: dmax, rh
    and, with a vanishing tensor, anisotropy)."""
    count: np.ndarray              # (n,) int32: the valid residues
    centroid: np.ndarray           # (n, 3)
    gyration_tensor: np.ndarray    # (n, 3, 3): the mean of (r - c)(r - c)^T
    rg: np.ndarray                 # sqrt(trace)
    eigenvalues: np.ndarray        # (n, 3), ascending l1 <= l2 <= l3 (numpy's eigvalsh)
    asphericity: np.ndarray        # l3 - (l1 + l2) / 2
    acylindricity: np.ndarray      # l2 - l1
    anisotropy: np.ndarray         # kappa^2 = 1 - 3 (l1 l2 + l2 l3 + l3 l1) / (l1 + l2 + l3)^2: 0 a sphere, 1 a rod
    ree: np.ndarray                # |r_last - r_first|, NaN unless both ends are valid
    dmax: np.ndarray               # the largest pair distance
    rh: np.ndarray                 # Kirkwood: 1 / Rh = N^-2 sum_{a != b} 1 / d_ab, so Rh = N^2 / (2 sum_{a<b} 1 / d)
    sum_inv_d: np.ndarray          # the kernel's sum over pairs a < b

    def summary(self) -> dict:
        """{quantity: {mean, std, min, max, n}} over the frames where it is defined."""
        out = {}
        for k in QUANTITIES:
            v = getattr(self, k)
            v = v[np.isfinite(v)]
            out[k] = {"mean": float(v.mean()) if v.size else float("nan"), "std": float(v.std()) if v.size else float("nan"),
                      "min": float(v.min()) if v.size else float("nan"), "max": float(v.max()) if v.size else float("nan"), "n": int(v.size)}
        return out


def _derive(count: np.ndarray, desc: np.ndarray) -> ShapeFrames:
    n = len(count)
    some, two = count >= 1, count >= 2
    with np.errstate(invalid="ignore", divide="ignore"):
        g = desc[:, 3:9] / count[:, None]                                  # the one division the kernel leaves to the host
        xx, yy, zz, xy, xz, yz = g.T
        S = np.stack([np.stack([xx, xy, xz], -1), np.stack([xy, yy, yz], -1), np.stack([xz, yz, zz], -1)], -2)
        S[~some] = np.nan
        lam = np.full((n, 3), np.nan)
        if some.any():
            lam[some] = np.linalg.eigvalsh(S[some])
        tr = lam.sum(-1)
        kappa = np.where(tr > 0, 1.0 - 3.0 * (lam[:, 0] * lam[:, 1] + lam[:, 1] * lam[:, 2] + lam[:, 2] * lam[:, 0]) / tr ** 2, np.nan)
        rg = np.where(some, np.sqrt((xx + yy) + zz), np.nan)
        rh = np.where(two, count.astype(np.float64) ** 2 / (2.0 * desc[:, 9]), np.nan)
    return ShapeFrames(count, desc[:, :3].copy(), S, rg, lam, lam[:, 2] - 0.5 * (lam[:, 0] + lam[:, 1]), lam[:, 1] - lam[:, 0], kappa,
                       desc[:, 11].copy(), np.where(two, desc[:, 10], np.nan), rh, desc[:, 9].copy())


def _inputs(samples, mask):
    X = pairs.coords(samples, "samples")
    return X, pairs.valid_mask(X, mask)


def frames(samples, mask=None) -> ShapeFrames:
    """The descriptors of every frame: one esmdiff_shape_frames call."""
    count, desc, _ = pairs.shape_frames(*_inputs(samples, mask))
    return _derive(count.cpu().numpy(), desc.cpu().numpy())


def distance_distribution(samples, r_max: Optional[float] = None, bins: int = 100, mask=None) -> dict:
    """The ensemble's pair-distance distribution: edges (bins + 1,), counts int64 (bins,) of the pairs a < b of all frames with
    edges[k] <= d < edges[k + 1] (cell floor(d / width) with the one float64 width = r_max / bins), overflow (d beyond r_max) and
    p = counts / (counts.sum() width), the density that integrates to 1 over [0, r_max].  r_max = None: a first call finds the
    ensemble's largest Dmax, and r_max is that rounded up to a whole Angstrom (at least 1)."""
    X, mk = _inputs(samples, mask)
    bins = int(bins)
    if r_max is None:
        top = pairs.shape_frames(X, mk)[1][:, 10].max().item()
        r_max = float(max(1.0, np.ceil(top)))
        if r_max == top:                                                   # a Dmax on the last edge would land in the overflow cell
            r_max += 1.0
    width = float(r_max) / bins if bins >= 1 else 0.0
    hist = pairs.shape_frames(X, mk, width, bins)[2].cpu().numpy()
    counts, total = hist[:bins], int(hist[:bins].sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        p = counts / (total * width) if total else np.full(bins, np.nan)
    return {"r_max": float(r_max), "width": width, "edges": width * np.arange(bins + 1), "counts": counts, "overflow": int(hist[bins]), "p": p}


def _q_array(q) -> np.ndarray:
    q = np.atleast_1d(np.asarray(q.detach().cpu().numpy() if torch.is_tensor(q) else q, np.float64))
    if q.ndim != 1 or q.size == 0 or not np.isfinite(q).all() or (q < 0).any():
        raise ValueError("q should be a 1D array of finite, non-negative values in 1 / Angstrom")
    return q


def debye(samples, q, form_factors=None, mask=None) -> np.ndarray:
    """The Debye intensity of every frame at every q, (n, Q): one esmdiff_debye_frames call per N.DEBYE_MAX_Q values of q.
    form_factors: (L, Q), f_a(q) of every residue (None: point scatterers, f = 1)."""
    X, mk = _inputs(samples, mask)
    q = _q_array(q)
    ff = None
    if form_factors is not None:
        ff = np.asarray(form_factors.detach().cpu().numpy() if torch.is_tensor(form_factors) else form_factors, np.float64)
        if ff.shape != (X.shape[1], q.size) or not np.isfinite(ff).all():
            raise ValueError(f"form_factors should be finite, ({X.shape[1]}, {q.size}): one row per residue, one column per q; got {ff.shape}")
    out = []
    for k0 in range(0, q.size, N.DEBYE_MAX_Q):
        qd = torch.as_tensor(q[k0:k0 + N.DEBYE_MAX_Q], device="cuda")
        fd = None if ff is None else torch.as_tensor(np.ascontiguousarray(ff[:, k0:k0 + N.DEBYE_MAX_Q]), device="cuda")
        out.append(pairs.debye_frames(X, mk, qd, fd).cpu().numpy())
    return np.concatenate(out, axis=1)


def saxs_profile(samples, q, form_factors=None, weights=None) -> dict:
    """The ensemble's profile: q, intensity (the mean of the frames' intensities, weighted by `weights` (n,) if given), i0 (its
    value at q = 0: the first value when q[0] == 0, one more evaluation for point scatterers, NaN with form factors that do not
    include q = 0) and normalised = intensity / i0."""
    q = _q_array(q)
    per_frame = debye(samples, q, form_factors)
    w = np.ones(per_frame.shape[0]) if weights is None else np.asarray(weights, np.float64)
    assert w.shape == (per_frame.shape[0],), f"weights should have one entry per frame ({per_frame.shape[0]})"
    mean = (per_frame * w[:, None]).sum(0) / w.sum()
    if q[0] == 0.0:
        i0 = float(mean[0])
    elif form_factors is None:
        i0 = float((debye(samples, [0.0])[:, 0] * w).sum() / w.sum())
    else:
        i0 = float("nan")
    return {"q": q, "intensity": mean, "i0": i0, "normalised": mean / i0}


def sphere_form_factor(q, radius: float) -> np.ndarray:
    """The amplitude of a homogeneous sphere, 3 (sin x - x cos x) / x^3 with x = q radius, 1 at x = 0.  Below x = 1, where the closed
    form cancels, its series sum_k 3 (-1)^k (2k + 2) x^(2k) / (2k + 3)! to k = 9 (the first term left out is below 1e-17)."""
    x = np.asarray(q, np.float64) * float(radius)
    small = np.abs(x) < 1.0
    xs = np.where(small, 1.0, x)
    x2 = np.where(small, x * x, 0.0)
    series = np.zeros_like(x2)
    for k in range(9, -1, -1):                                             # Horner in x^2
        series = series * x2 + 3.0 * (-1.0) ** k * (2 * k + 2) / math.factorial(2 * k + 3)
    return np.where(small, series, 3.0 * (np.sin(xs) - xs * np.cos(xs)) / xs ** 3)


def guinier_rg(q, intensity, qrg_max: float = 1.3) -> dict:
    """ln I = ln I(0) - q^2 Rg^2 / 3 fitted by least squares on the window q Rg <= qrg_max, iterated to a fixed point from the full
    range -> {rg, i0, q_max (the window's largest q), n_points}; NaN with fewer than 3 points or a slope that is not negative."""
    q, I = np.asarray(q, np.float64), np.asarray(intensity, np.float64)
    ok = np.isfinite(I) & (I > 0) & np.isfinite(q)
    q, y = q[ok], np.log(I[ok])
    nan = {"rg": float("nan"), "i0": float("nan"), "q_max": float("nan"), "n_points": 0}
    use, seen = np.ones(q.size, bool), set()
    while True:
        if use.sum() < 3:
            return dict(nan, n_points=int(use.sum()))
        slope, icpt = np.polyfit(q[use] ** 2, y[use], 1)
        if not slope < 0:
            return dict(nan, n_points=int(use.sum()))
        rg = float(np.sqrt(-3.0 * slope))
        nxt = q * rg <= qrg_max
        key = nxt.tobytes()
        if np.array_equal(nxt, use) or key in seen:                        # a fixed point (or a cycle between two windows: keep this one)
            return {"rg": rg, "i0": float(np.exp(icpt)), "q_max": float(q[use].max()), "n_points": int(use.sum())}
        seen.add(key)
        use = nxt


def kratky(q, intensity, rg: Optional[float] = None, i0: Optional[float] = None):
    """-> (x, y): the plain Kratky curve (q, q^2 I) or, with rg, the dimensionless one (q Rg, (q Rg)^2 I / I(0)); i0 defaults to the
    intensity at the smallest q."""
    q, I = np.asarray(q, np.float64), np.asarray(intensity, np.float64)
    if rg is None:
        return q, q * q * I
    i0 = float(I[np.argmin(q)]) if i0 is None else float(i0)
    x = q * float(rg)
    return x, x * x * I / i0


def chi2(calc, q_exp, i_exp, sigma, fit_constant: bool = False) -> dict:
    """The reduced chi^2 of calculated intensities (Q,) or (n, Q) at the measured q against (i_exp, sigma) after the closed-form
    least-squares scale c (and, with fit_constant, constant b): sum(((c calc + b - i_exp) / sigma)^2) / (Q - parameters).
    -> {chi2, scale, constant} as floats or (n,) arrays, and for (n, Q) also best: the frame with the smallest chi^2."""
    c = np.asarray(calc, np.float64)
    q_exp, y, s = (np.asarray(v, np.float64) for v in (q_exp, i_exp, sigma))
    assert y.shape == s.shape == q_exp.shape and c.shape[-1] == y.shape[0], "calc, q_exp, i_exp and sigma should have one value per q"
    assert (s > 0).all(), "sigma should be positive"
    w = 1.0 / (s * s)
    rows = np.atleast_2d(c)
    params = 2 if fit_constant else 1
    if fit_constant:
        sw, sc, sy = w.sum(), (rows * w).sum(1), (y * w).sum()
        scc, scy = (rows * rows * w).sum(1), (rows * y * w).sum(1)
        det = scc * sw - sc * sc
        scale, const = (scy * sw - sc * sy) / det, (scc * sy - sc * scy) / det
    else:
        scale, const = (rows * y * w).sum(1) / (rows * rows * w).sum(1), np.zeros(rows.shape[0])
    resid = (scale[:, None] * rows + const[:, None] - y) / s
    value = (resid * resid).sum(1) / max(1, y.size - params)
    if c.ndim == 1:
        return {"chi2": float(value[0]), "scale": float(scale[0]), "constant": float(const[0])}
    return {"chi2": value, "scale": scale, "constant": const, "best": int(np.argmin(value))}


def js_shape(ensembles, ref_key: str = "target", quantities=("rg", "ree", "rh", "asphericity"), n_bins: int = 50, rounded: bool = True) -> dict:
    """{quantity: {name: JS distance}}: for every descriptor the Jensen-Shannon distance between the distribution of its values over
    the frames of each ensemble of `ensembles` ({name: (n, L, 3)}) and over those of ensembles[ref_key] — js_rg's conventions (bins
    spanning the reference's range, pseudo count 1e-6, rounded to 4 decimals, the reference against itself 0), through the same
    esmdiff_metrics_js_columns.  Frames where a quantity is undefined are left out of it."""
    desc = {k: frames(v) for k, v in ensembles.items()}
    finite = lambda v: v[np.isfinite(v)]
    return {name: js_columns({k: finite(getattr(d, name)) for k, d in desc.items()}, ref_key, n_bins, rounded) for name in quantities}


def _per_frame(d: ShapeFrames) -> dict:
    return {"count": d.count, "centroid": d.centroid, "eigenvalues": d.eigenvalues, **{k: getattr(d, k) for k in QUANTITIES}}


def report(samples, targets, pr_bins: int = 100) -> dict:
    """The "shape" block of analyze_ensemble: samples (n, L, 3), targets (K, L, 3)."""
    d, t = frames(samples), frames(targets)
    pr = distance_distribution(samples, None, pr_bins)
    js = js_shape({"samples": samples, "target": targets})
    return {"pr_bins": int(pr_bins), "quantities": list(QUANTITIES), "samples": _per_frame(d), "summary": d.summary(),
            "pr": {"r_max": pr["r_max"], "width": pr["width"], "counts": pr["counts"], "overflow": pr["overflow"], "p": pr["p"]},
            "targets": [{k: v[i] if np.ndim(v[i]) else v[i].item() for k, v in _per_frame(t).items()} for i in range(len(t.count))],
            # the targets taken together as one ensemble: thin with few of them (each fills one cell of a quantity's histogram)
            "js_shape": {"n_targets": int(len(t.count)), **{k: v["samples"] for k, v in js.items()}}}


def read_saxs_data(path):
    """Three whitespace-separated columns q, I, sigma; lines starting with # (and empty ones) are ignored -> (q, I, sigma)."""
    rows = []
    for line in open(path):
        line = line.strip()
        if line and not line.startswith("#"):
            rows.append([float(v) for v in line.split()[:3]])
    data = np.asarray(rows, np.float64)
    if data.ndim != 2 or data.shape[1] != 3:
        raise ValueError(f"{path}: expected three columns q, I, sigma")
    return data[:, 0], data[:, 1], data[:, 2]


def saxs_report(samples, q_max: float = 0.5, points: int = 51, data=None) -> dict:
    """The "saxs" block of analyze_ensemble for point scatterers: q (0 .. q_max in `points` steps, or the q of `data` = (q, I, sigma)),
    the mean profile, i0, the Guinier Rg beside the mean coordinate Rg, the dimensionless Kratky curve and, with data, the reduced
    chi^2 of the mean profile and of every sample against it."""
    q = np.linspace(0.0, float(q_max), int(points)) if data is None else np.asarray(data[0], np.float64)
    per_frame = debye(samples, np.concatenate([[0.0], q]))
    mean = per_frame.mean(0)
    i0, I = float(mean[0]), mean[1:]
    fit = guinier_rg(q, I)
    rg = frames(samples).rg
    x, y = kratky(q, I, fit["rg"], i0)
    out = {"q": q, "intensity": I, "i0": i0, "normalised": I / i0, "guinier": fit, "rg_coordinates": float(np.nanmean(rg)),
           "rg_coordinates_rms": float(np.sqrt(np.nanmean(rg ** 2))), "kratky": {"q_rg": x, "y": y}}
    if data is not None:
        out["chi2_mean"] = chi2(I, *data)
        each = chi2(per_frame[:, 1:], *data)
        out["chi2_samples"] = {"chi2": each["chi2"], "scale": each["scale"], "best_model": each["best"]}
    return out

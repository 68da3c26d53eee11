"""Solvent accessibility of ensembles on the device: the backbone's accessible surface by the point test of Shrake & Rupley 1973, per
atom, residue and frame, and over an ensemble the share of frames in which each residue is exposed and the mutual information of the
exposure of residue pairs.

The layer above csrc/sasa.hip.  Two entries carry everything here:

  esmdiff_sasa_frames   per atom the INTEGER number of its sphere points that no other atom of the frame buries; over the frames the
                        sums of those counts, the two-state exposure of every residue and how often it is 1.  Memory for the ensemble
                        outputs is O(L A) whatever n is.
  esmdiff_cooccurrence  for any (n, L) table of two-state flags the (3, L, L) counts of frames in which a and b are both defined, a is
                        1, and both are 1.

The definition is closed: atom (a, k) is a sphere of radius r[a, k] + probe, its P points are the golden-section spiral of
sphere_points (computed here, in numpy, and handed to the kernel), a point is buried when it lies strictly inside another atom's
sphere; all arithmetic float64.  The counts are held exactly to the numpy restatement tests/sasa_ref.py, and every area below is
derived from them in numpy.  Parity with NACCESS / freesasa / mdtraj is UNPINNED: none of them has been run against this, and only
the definition is tested.  The radii are a parameter; the default 1.65 / 1.87 / 1.76 / 1.40 Angstrom for N / CA / C / O is a stated
convention (united-atom radii), as are the probe of 1.4 Angstrom, the 96 points and the exposure threshold of 0.2.  Relative exposure is
the residue's area over the area of its atoms taken alone (every point exposed): no Gly-X-Gly table is recalled from memory, so the
values are lower than the customary relative accessibilities and the threshold is this project's own.

  sphere_points            the P unit points
  sasa                     backbones -> Accessibility (counts, atom_area, residue_area, total, relative)
  exposure                 the fused reduction over an ensemble -> Exposure (mean areas, frequency, joint, mutual_information)
  exposed_jaccard          the Jaccard index of the residue sets two ensembles expose
  exposure_mi_correlation  Spearman correlation of two ensembles' exposure mutual-information matrices
  exposure_switches        the residues exposed in exactly one of two targets, with the ensemble's frequency
  js_sasa                  the Jensen-Shannon distance between ensembles' distributions of total area, js_rg's conventions
  report                   the "sasa" block of `python -m esmdiff_amd.analyze_ensemble --sasa`

Inputs follow esmdiff_amd/ensemble.py and esmdiff_amd/secondary.py: Angstrom; a PDB path (N / CA / C of every MODEL), an array or a
tensor.  (L, A, 3) or (n, L, A, 3) with A = 4 (N, CA, C, O), A = 3 (N, CA, C: O is placed by secondary.infer_oxygen, as the DSSP layer
does) or A = 1 (CA only: there is no default radius, the caller gives one).  A three-axis array whose middle axis is not 1, 3 or 4 is
(n, L, 3) CA traces.  An atom with a NaN coordinate is absent — it has no count and buries nothing — and `mask` (n, L) or (L,)
removes whole residues.  Results are numpy on the host.  There is no CPU fallback."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _native as N
from . import pairs
from .flexibility import flexibility_correlation
from .metrics import js_columns

DEFAULT_RADII = (1.65, 1.87, 1.76, 1.40)     # N, CA, C, O: a stated convention (united-atom radii), not a pinned program
PROBE, POINTS, THRESHOLD = 1.4, 96, 0.2
FOUR_PI = 4.0 * math.pi
GOLDEN_ANGLE = math.pi * (3.0 - math.sqrt(5.0))


def sphere_points(P: int) -> np.ndarray:
    """The P unit points of the golden-section spiral, float64 (P, 3): for k = 0 .. P - 1, z = 1 - (2k + 1) / P, rho = sqrt(1 - z z),
    phi = k pi (3 - sqrt 5), u = (rho cos phi, rho sin phi, z)."""
    P = int(P)
    if not 1 <= P <= N.SASA_MAX_POINTS:
        raise ValueError(f"points should be 1 to {N.SASA_MAX_POINTS}, got {P}")
    k = np.arange(P, dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / P
    rho = np.sqrt(1.0 - z * z)
    phi = k * GOLDEN_ANGLE
    return np.stack([rho * np.cos(phi), rho * np.sin(phi), z], axis=1)


def atom_array(backbone) -> np.ndarray:
    """-> float64 (n, L, A, 3) on the host with A = 4 or 1 (the module's text states what is accepted)."""
    return pairs.atoms(backbone, (1, 3, 4), infer_o=True, ca_traces=True,
                       what="atoms should be (n, L, A, 3) with A = 4 (N, CA, C, O), 3 (N, CA, C) or 1 (CA)")


def expanded_radii(radii, probe: float, L: int, A: int) -> np.ndarray:
    """radii (None: the default of N / CA / C / O; a scalar, (A,) or (L, A)) -> float64 (L, A), each plus the probe."""
    probe = float(probe)
    if not (np.isfinite(probe) and probe >= 0.0):
        raise ValueError(f"the probe radius should be finite and not negative, got {probe}")
    if radii is None:
        if A != 4:
            raise ValueError("CA-only input has no default radius: pass radii (a scalar, (A,) or (L, A))")
        radii = DEFAULT_RADII
    r = np.asarray(radii.detach().cpu().numpy() if torch.is_tensor(radii) else radii, np.float64)
    if r.ndim > 2 or (r.ndim == 1 and r.shape != (A,)) or (r.ndim == 2 and r.shape != (L, A)):
        raise ValueError(f"radii should be a scalar, ({A},) or ({L}, {A}), got {r.shape}")
    r = np.broadcast_to(r, (L, A))
    if not (np.isfinite(r).all() and (r > 0).all()):
        raise ValueError("radii should be finite and positive")
    return np.ascontiguousarray(r + probe)


def atom_area(R, count, P) -> np.ndarray:
    """((4 pi (R R)) count) / P for expanded radii R and float64 counts."""
    return ((FOUR_PI * (R * R)) * np.asarray(count, np.float64)) / float(P)


def _residue_sum(a: np.ndarray) -> np.ndarray:
    """(..., A) -> (...): ((a0 + a1) + a2) + a3."""
    s = a[..., 0]
    for k in range(1, a.shape[-1]):
        s = s + a[..., k]
    return s


def _device_args(backbone, radii, probe, points, mask):
    """-> X f64 (n, L, A, 3), mask u8 or None, expanded radii (L, A) and points (P, 3) on the device, and the last two on the host."""
    pairs.need_device("esmdiff_amd.accessibility")
    x = atom_array(backbone)
    n, L, A = x.shape[:3]
    R, u = expanded_radii(radii, probe, L, A), sphere_points(points)
    mk = pairs.given_mask(mask, n, L)[1]
    return torch.as_tensor(x, device="cuda"), mk, torch.as_tensor(R, device="cuda"), torch.as_tensor(u, device="cuda"), R, u


@dataclass
class Accessibility:
    """Per frame.  counts is what the kernel gives; every area is derived from it here."""
    counts: np.ndarray             # (n, L, A) int32: the exposed points of each atom, -1 for an absent atom
    radii: np.ndarray              # (L, A): the expanded radii, r + probe
    points: int
    probe: float

    def atom_area(self) -> np.ndarray:
        """(n, L, A) Angstrom^2: 4 pi R^2 count / P, NaN for an absent atom."""
        return np.where(self.counts >= 0, atom_area(self.radii, self.counts, self.points), np.nan)

    def _sums(self):
        here = self.counts >= 0
        a = np.where(here, atom_area(self.radii, self.counts, self.points), 0.0)
        alone = np.where(here, atom_area(self.radii, float(self.points), self.points), 0.0)
        return here.any(-1), _residue_sum(a), _residue_sum(alone)

    def residue_area(self) -> np.ndarray:
        """(n, L): the sum over the residue's present atoms in the order ((a0 + a1) + a2) + a3, NaN for a residue without atoms."""
        some, area, _ = self._sums()
        return np.where(some, area, np.nan)

    def total(self) -> np.ndarray:
        """(n,): the area of the frame, absent residues adding nothing."""
        some, area, _ = self._sums()
        return np.where(some, area, 0.0).sum(-1)

    def relative(self) -> np.ndarray:
        """(n, L): the residue's area over the area of its present atoms taken alone (every point exposed), NaN without atoms."""
        some, area, alone = self._sums()
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(some, area / alone, np.nan)

    def exposed(self, threshold: float = THRESHOLD) -> np.ndarray:
        """(n, L) uint8: 1 where relative() > threshold, 0 where not, 2 for a residue without atoms — the kernel's flags."""
        some, area, alone = self._sums()
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(some, area / alone > threshold, 2).astype(np.uint8)


def sasa(backbone, radii=None, probe: float = PROBE, points: int = POINTS, mask=None) -> Accessibility:
    """The accessible surface of every frame: one esmdiff_sasa_frames call."""
    X, mk, Rd, ud, R, u = _device_args(backbone, radii, probe, points, mask)
    count = pairs.sasa_frames(X, mk, Rd, ud, want=("count",))["count"]
    return Accessibility(count.cpu().numpy(), R, len(u), float(probe))


def mutual_information(counts) -> np.ndarray:
    """Co-occurrence counts (3, L, L) -> (L, L): the mutual information, in nats, of the two-state variables of a and b over the frames
    where both are defined (0 ln 0 = 0); 0 where a pair is never jointly defined."""
    both, a_one, both_one = (np.asarray(c, np.float64) for c in counts)
    b_one = a_one.T
    n11, n10, n01 = both_one, a_one - both_one, b_one - both_one
    n00 = both - a_one - b_one + both_one
    out = np.zeros_like(both)
    with np.errstate(invalid="ignore", divide="ignore"):
        for nxy, nx, ny in ((n11, a_one, b_one), (n10, a_one, both - b_one), (n01, both - a_one, b_one), (n00, both - a_one, both - b_one)):
            out += np.where(nxy > 0, (nxy / both) * np.log((nxy * both) / (nx * ny)), 0.0)
    return np.where(both > 0, np.maximum(out, 0.0), 0.0)


@dataclass
class Exposure:
    """An ensemble reduced over its frames on the device; no (n, L, A) array was kept."""
    n: int
    sum_count: np.ndarray          # (L, A) int64: the sum of an atom's exposed points over the frames where it is present
    valid: np.ndarray              # (L, A) int32: those frames
    exposed_count: np.ndarray      # (L,) int32: the frames in which the residue's relative exposure is above the threshold
    present_count: np.ndarray      # (L,) int32: the frames in which the residue has an atom
    radii: np.ndarray              # (L, A), expanded
    points: int
    probe: float
    threshold: float
    cooccurrence: Optional[np.ndarray] = None    # (3, L, L) int32, with joint=True

    def mean_atom_area(self) -> np.ndarray:
        """(L, A): the mean area of each atom over the frames where it is present, NaN where it never is."""
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(self.valid > 0, atom_area(self.radii, self.sum_count / self.valid, self.points), np.nan)

    def mean_residue_area(self) -> np.ndarray:
        """(L,): the sum of the residue's mean atom areas, NaN where no atom of it is ever present."""
        a = self.mean_atom_area()
        some = self.valid > 0
        return np.where(some.any(-1), _residue_sum(np.where(some, a, 0.0)), np.nan)

    def mean_relative(self) -> np.ndarray:
        """(L,): mean_residue_area over the area of those atoms taken alone."""
        some = self.valid > 0
        alone = _residue_sum(np.where(some, atom_area(self.radii, float(self.points), self.points), 0.0))
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(some.any(-1), self.mean_residue_area() / alone, np.nan)

    def frequency(self) -> np.ndarray:
        """(L,): the share of the frames having the residue in which it is exposed, NaN where none has it."""
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(self.present_count > 0, self.exposed_count / self.present_count, np.nan)

    def joint(self) -> np.ndarray:
        assert self.cooccurrence is not None, "exposure(..., joint=True) computes the co-occurrence counts"
        return self.cooccurrence

    def mutual_information(self) -> np.ndarray:
        return mutual_information(self.joint())


def exposure(samples, threshold: float = THRESHOLD, radii=None, probe: float = PROBE, points: int = POINTS, mask=None,
             joint: bool = False) -> Exposure:
    """The ensemble's exposure in one esmdiff_sasa_frames call and, with `joint`, one esmdiff_cooccurrence call on its (n, L) flags."""
    threshold = float(threshold)
    if np.isnan(threshold):
        raise ValueError("the exposure threshold should not be NaN")
    X, mk, Rd, ud, R, u = _device_args(samples, radii, probe, points, mask)
    want = ("sum_count", "valid", "exposed_count", "present_count") + (("exposed",) if joint else ())
    res = pairs.sasa_frames(X, mk, Rd, ud, threshold, want)
    co = pairs.cooccurrence(res["exposed"]).cpu().numpy() if joint else None
    return Exposure(int(X.shape[0]), res["sum_count"].cpu().numpy(), res["valid"].cpu().numpy(), res["exposed_count"].cpu().numpy(),
                    res["present_count"].cpu().numpy(), R, len(u), float(probe), threshold, co)


def _as_exposure(x, joint: bool = False, **kw) -> Exposure:
    return x if isinstance(x, Exposure) else exposure(x, joint=joint, **kw)


def exposed_jaccard(a, b, min_frequency: float = 0.5, **kw) -> float:
    """The Jaccard index of the sets of residues that the two ensembles (Exposure, or anything `exposure` takes) expose in more than
    min_frequency of their frames; NaN when neither exposes any."""
    fa, fb = _as_exposure(a, **kw).frequency(), _as_exposure(b, **kw).frequency()
    assert fa.shape == fb.shape, f"{fa.shape[0]} and {fb.shape[0]} residues: the correspondence is residue to residue"
    with np.errstate(invalid="ignore"):
        sa, sb = fa > min_frequency, fb > min_frequency
    union = int((sa | sb).sum())
    return float((sa & sb).sum() / union) if union else float("nan")


def exposure_mi_correlation(a, b, **kw) -> dict:
    """flexibility.flexibility_correlation (pearson, spearman, kendall, n) of the upper triangles a < b of the two ensembles' exposure
    mutual-information matrices, over the pairs jointly defined in both; the Spearman value is the benchmark's number."""
    ea, eb = _as_exposure(a, True, **kw), _as_exposure(b, True, **kw)
    assert ea.joint().shape == eb.joint().shape, "the correspondence is residue to residue"
    iu = np.triu_indices(ea.joint().shape[1], 1)
    ma = np.where(ea.joint()[0] > 0, ea.mutual_information(), np.nan)[iu]
    mb = np.where(eb.joint()[0] > 0, eb.mutual_information(), np.nan)[iu]
    return flexibility_correlation(ma, mb)


def exposure_switches(samples, t1, t2, threshold: float = THRESHOLD, **kw) -> list:
    """The residues present in both targets and exposed in exactly one of them, each as {"residue": index from 0, "exposed": the two
    targets' flags, "relative": their relative exposures, "frequency": the share of the samples' frames exposing it (None where no
    sample has the residue)} — the accessibility counterpart of secondary.switch_residues."""
    s = _as_exposure(samples, threshold=threshold, **kw)
    a, b = sasa(t1, **kw), sasa(t2, **kw)
    ea, eb, ra, rb, freq = a.exposed(threshold)[0], b.exposed(threshold)[0], a.relative()[0], b.relative()[0], s.frequency()
    out = []
    for l in np.nonzero((ea != 2) & (eb != 2) & (ea != eb))[0]:
        out.append({"residue": int(l), "exposed": [bool(ea[l]), bool(eb[l])], "relative": [float(ra[l]), float(rb[l])],
                    "frequency": None if np.isnan(freq[l]) else float(freq[l])})
    return out


def js_sasa(ensembles, ref_key: str = "target", n_bins: int = 50, rounded: bool = True, **kw) -> dict:
    """{name: JS distance} between the distribution of the total area over the frames of each ensemble of `ensembles` and over those
    of ensembles[ref_key] — js_rg's conventions (bins spanning the reference's range, pseudo count 1e-6, rounded to 4 decimals, the
    reference against itself 0), through the same esmdiff_metrics_js_columns."""
    return js_columns({k: sasa(v, **kw).total() for k, v in ensembles.items()}, ref_key, n_bins, rounded)


def _summary(v: np.ndarray) -> dict:
    v = v[np.isfinite(v)]
    nan = float("nan")
    return {"mean": float(v.mean()) if v.size else nan, "std": float(v.std()) if v.size else nan, "min": float(v.min()) if v.size else nan,
            "max": float(v.max()) if v.size else nan, "n": int(v.size)}


def report(samples, targets=(), points: int = POINTS, probe: float = PROBE, threshold: float = THRESHOLD, radii=None) -> dict:
    """The "sasa" block of analyze_ensemble: samples and each target as `sasa` takes them."""
    kw = {"radii": radii, "probe": probe, "points": points}
    s, per_frame = exposure(samples, threshold, **kw), sasa(samples, **kw)
    total = per_frame.total()
    out = {"points": int(points), "probe": float(probe), "threshold": float(threshold), "radii": np.asarray(DEFAULT_RADII if radii is None else radii, np.float64),
           "parity": "unpinned against NACCESS / freesasa / mdtraj",
           "residue_area": s.mean_residue_area(), "relative": s.mean_relative(), "exposed_frequency": s.frequency(),
           "total_area": total, "summary": _summary(total), "targets": []}
    ts = [sasa(t, **kw) for t in targets]
    for target, t in zip(targets, ts):
        out["targets"].append({"residue_area": t.residue_area()[0], "relative": t.relative()[0],
                               "exposed": [None if f == 2 else bool(f) for f in t.exposed(threshold)[0]],
                               "total_area": float(t.total()[0]), "exposed_jaccard": exposed_jaccard(s, exposure(target, threshold, **kw))})
    if len(ts) == 2:
        out["exposure_switches"] = exposure_switches(s, targets[0], targets[1], threshold, **kw)
    return out

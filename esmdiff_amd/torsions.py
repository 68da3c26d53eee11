"""Backbone torsions of ensembles on the device: phi / psi / omega, bond lengths and angles, per-residue Ramachandran maps, their
circular statistics, region propensities, and the distance between two ensembles' maps.

The layer above csrc/torsions.hip.  Two entries carry everything here:

  esmdiff_backbone_torsions  the three torsions of every residue of every structure, and on request the three bond lengths and
                             three bond angles of the backbone.
  esmdiff_ramachandran       an ensemble reduced over its frames, from the coordinates: per residue a bins x bins histogram of
                             (phi, psi), five counts (phi, psi, both, omega defined, cis) and the sums of the cosines and sines of
                             the three angles.  Memory is O(L bins^2) whatever the number of frames; no (n, L) angle array exists.

The definitions are closed and rest on no recalled program: IUPAC's sign (an alpha helix has phi = -57), a peptide link wherever
|C_i - N_{i+1}| <= break_distance (2.5 Angstrom, the chain-break rule of the secondary-structure layer), a torsion defined wherever
its link exists and its four atoms are not collinear.  Integer outputs are held exactly to the numpy restatement
tests/torsions_ref.py, the sums bit for bit.

  torsions            backbones -> BackboneTorsions
  ramachandran        an ensemble -> RamachandranMap (density, circular_mean, circular_variance, cis_fraction, entropy,
                      region_counts, region_propensity)
  js_ramachandran     the Jensen-Shannon distance between ensembles' maps, residue by residue, js_pwd's conventions
  torsion_agreement   the share of residues of every sample whose phi and psi lie within a tolerance of a target's
  region_switches     the residues whose region differs between two targets, with the ensemble's share in each
  geometry_summary    bond lengths and angles against ideal values
  report              the "torsions" block of `python -m esmdiff_amd.analyze_ensemble --torsions`

Inputs follow esmdiff_amd/secondary.py: Angstrom, arrays, tensors or a PDB path, (L, A, 3) or (n, L, A, 3) with A = 3 (N, CA, C) or 4
(O is never read); residues with NaN backbone atoms are absent, `mask` (n, L) or (L,) removes more.  Results are numpy arrays and
floats on the host.  There is no CPU fallback."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import pairs

BREAK_DISTANCE = 2.5                     # Angstrom: tests/dssp_ref.BREAK, the chain break of csrc/dssp.hip
DEG = 57.29577951308232                  # the factor of the kernel's bin expression
# A stated convention, not a pinned program: a partition of the (phi, psi) plane into rectangles [phi_lo, phi_hi) x [psi_lo, psi_hi)
# in degrees on 10-degree edges.  Left half (phi < 0): the broad alpha basin -120 <= psi < 50; above and below it beta (phi < -90) and
# polyproline II (phi >= -90).  Right half: left-handed helix -50 <= psi < 100, the rest "other".
REGIONS = {
    "alpha": [(-180, 0, -120, 50)],
    "beta": [(-180, -90, 50, 180), (-180, -90, -180, -120)],
    "ppII": [(-90, 0, 50, 180), (-90, 0, -180, -120)],
    "left": [(0, 180, -50, 100)],
    "other": [(0, 180, 100, 180), (0, 180, -180, -50)],
}
REGION_LETTERS = {"alpha": "A", "beta": "B", "ppII": "P", "left": "L", "other": "O"}
# tests/dssp_ref.nerf's set: N-CA, CA-C, C-N in Angstrom; N-CA-C, CA-C-N, C-N-CA in degrees
IDEAL = {"n_ca": 1.458, "ca_c": 1.525, "c_n": 1.329, "n_ca_c": 111.0, "ca_c_n": 116.2, "c_n_ca": 121.7}
QUANTITIES = tuple(IDEAL)


def backbone_array(backbone) -> np.ndarray:
    """A PDB path (N / CA / C of every MODEL), an array or a tensor, (L, A, 3) or (n, L, A, 3) with A = 3 or 4 -> float64 (n, L, A, 3)
    on the host, as it is (no O is inferred: none is read)."""
    return pairs.atoms(backbone, (3, 4), what="backbones should be (n, L, 3, 3) N / CA / C or (n, L, 4, 3) N / CA / C / O")


def _device_args(backbone, mask):
    """-> X f64 on the device, mask u8 on the device or None, present bool (n, L) on the host."""
    x = backbone_array(backbone)
    given, mk = pairs.given_mask(mask, *x.shape[:2])
    return torch.as_tensor(x, device="cuda"), mk, given & np.isfinite(x[:, :, :3]).all((2, 3))


@dataclass
class BackboneTorsions:
    phi: np.ndarray                              # (n, L), NaN where undefined; degrees unless made with degrees=False
    psi: np.ndarray
    omega: np.ndarray                            # of the peptide i -> i + 1, stored at i
    present: np.ndarray                          # (n, L) bool: not masked, N / CA / C resolved
    degrees: bool = True
    bond_lengths: Optional[np.ndarray] = None    # (n, L, 3) Angstrom: N-CA, CA-C, C_i-N_{i+1}
    bond_angles: Optional[np.ndarray] = None     # (n, L, 3): N-CA-C, CA_i-C_i-N_{i+1}, C_i-N_{i+1}-CA_{i+1}

    def cis(self) -> np.ndarray:
        """(n, L) bool: omega defined and within 90 degrees of 0."""
        with np.errstate(invalid="ignore"):
            return np.abs(self.omega) < (90.0 if self.degrees else np.pi / 2)


def torsions(backbone, mask=None, break_distance: float = BREAK_DISTANCE, geometry: bool = False, degrees: bool = True) -> BackboneTorsions:
    """The torsions of every structure: one esmdiff_backbone_torsions call.  geometry: also the bond lengths and bond angles."""
    pairs.need_device("esmdiff_amd.torsions.torsions")
    X, mk, present = _device_args(backbone, mask)
    phi, psi, omega, geom = pairs.backbone_torsions(X, mk, break_distance, geometry)
    scale = DEG if degrees else 1.0
    out = BackboneTorsions(phi.cpu().numpy() * scale, psi.cpu().numpy() * scale, omega.cpu().numpy() * scale, present, bool(degrees))
    if geometry:
        g = geom.cpu().numpy()
        out.bond_lengths, out.bond_angles = g[:, :, :3].copy(), g[:, :, 3:] * scale
    return out


def _region_table(bins: int, regions) -> np.ndarray:
    """int (bins, bins): the index of the region of every cell, -1 where none covers it.  Raises ValueError for an edge off the bin
    grid or overlapping rectangles."""
    w = 360.0 / bins
    table = np.full((bins, bins), -1, np.int64)
    for k, rects in enumerate(regions.values()):
        for rect in rects:
            idx = []
            for edge in rect:
                b = (float(edge) + 180.0) / w
                if not -180 <= edge <= 180 or b != round(b):
                    raise ValueError(f"region edge {edge} is not on the grid of {bins} bins ({w:g} degrees wide) over [-180, 180]")
                idx.append(int(round(b)))
            cells = table[idx[0]:idx[1], idx[2]:idx[3]]
            if (cells >= 0).any():
                raise ValueError(f"region rectangle {rect} overlaps another")
            cells[...] = k
    return table


def _fractions(count, total):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(total > 0, count / total, np.nan)


@dataclass
class RamachandranMap:
    """hist int32 (L, bins, bins) indexed [residue][phi bin][psi bin] over [-180, 180) degrees; counts int32 (L, 5): the frames with
    phi defined, psi defined, both, omega defined, and cis; sums float64 (L, 6): the sums of cos phi, sin phi, cos psi, sin psi,
    cos omega, sin omega over the frames in which that angle is defined."""
    hist: np.ndarray
    counts: np.ndarray
    sums: np.ndarray
    bins: int
    n_frames: int

    def density(self) -> np.ndarray:
        """(L, bins, bins) summing to 1 per residue; NaN rows where no frame has both angles."""
        return _fractions(self.hist.astype(np.float64), self.counts[:, 2].astype(np.float64)[:, None, None])

    def _resultant(self):
        c, s = self.sums[:, 0::2], self.sums[:, 1::2]
        return c, s, self.counts[:, [0, 1, 3]].astype(np.float64)

    def circular_mean(self) -> np.ndarray:
        """(L, 3) degrees, of phi, psi, omega: the direction of the summed unit vectors; NaN where the angle is never defined."""
        c, s, k = self._resultant()
        return np.where(k > 0, np.arctan2(s, c) * DEG, np.nan)

    def circular_variance(self) -> np.ndarray:
        """(L, 3): 1 - |mean unit vector|, 0 for a fixed angle, towards 1 for a uniform one."""
        c, s, k = self._resultant()
        return 1.0 - _fractions(np.sqrt(c * c + s * s), k)

    def cis_fraction(self) -> np.ndarray:
        """(L,): the share of the frames with omega_i defined in which the peptide i -> i + 1 is cis."""
        return _fractions(self.counts[:, 4].astype(np.float64), self.counts[:, 3].astype(np.float64))

    def entropy(self) -> np.ndarray:
        """(L,) nats: -sum p ln p of the normalised map; NaN where no frame has both angles."""
        p = self.density()
        with np.errstate(invalid="ignore", divide="ignore"):
            return -np.where(p > 0, p * np.log(p), 0.0).sum((1, 2)) + np.where(self.counts[:, 2] > 0, 0.0, np.nan)

    def region_counts(self, regions=REGIONS) -> np.ndarray:
        """(L, len(regions)) int: exact sums of histogram cells.  The edges must lie on the bin grid (ValueError otherwise)."""
        table = _region_table(self.bins, regions)
        return np.stack([self.hist[:, table == k].sum(1) for k in range(len(regions))], axis=1).astype(np.int64)

    def region_propensity(self, regions=REGIONS) -> np.ndarray:
        """(L, len(regions)): the share of the frames having both angles; NaN where there is none."""
        return _fractions(self.region_counts(regions).astype(np.float64), self.counts[:, 2].astype(np.float64)[:, None])


def ramachandran(samples, bins: int = 36, mask=None, break_distance: float = BREAK_DISTANCE) -> RamachandranMap:
    """The per-residue Ramachandran maps of an ensemble: one esmdiff_ramachandran call."""
    pairs.need_device("esmdiff_amd.torsions.ramachandran")
    X, mk, _ = _device_args(samples, mask)
    hist, counts, sums = pairs.ramachandran(X, mk, break_distance, bins)
    return RamachandranMap(hist.cpu().numpy(), counts.cpu().numpy(), sums.cpu().numpy(), int(bins), int(X.shape[0]))


def js_distance(p, q) -> float:
    """scipy.spatial.distance.jensenshannon(p, q): the square root of the Jensen-Shannon divergence in nats, in plain numpy."""
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    p, q = p / p.sum(), q / q.sum()
    m = (p + q) / 2.0
    with np.errstate(invalid="ignore", divide="ignore"):
        left = np.where(p > 0, p * np.log(p / m), 0.0)
        right = np.where(q > 0, q * np.log(q / m), 0.0)
    return float(np.sqrt((left.sum() + right.sum()) / 2.0))


def js_maps(a: RamachandranMap, b: RamachandranMap) -> np.ndarray:
    """(L,): per residue the Jensen-Shannon distance of the two flattened maps, each with 1e-6 added to every cell (js_pwd's
    convention); NaN where either ensemble has no frame with both angles."""
    assert a.hist.shape == b.hist.shape, f"maps of {a.hist.shape} and {b.hist.shape}: the correspondence is residue to residue"
    out = np.full(a.hist.shape[0], np.nan)
    for i in np.nonzero((a.counts[:, 2] > 0) & (b.counts[:, 2] > 0))[0]:
        out[i] = js_distance(a.hist[i].ravel() + 1e-6, b.hist[i].ravel() + 1e-6)
    return out


def js_ramachandran(ensembles, ref_key: str = "target", bins: int = 36, rounded: bool = True, per_residue: bool = False,
                    break_distance: float = BREAK_DISTANCE):
    """{name: backbones} -> {name: the mean over residues of the Jensen-Shannon distance between the name's Ramachandran map and
    ensembles[ref_key]'s}, results[ref_key] = 0.0, rounded to 4 decimals (js_pwd's conventions).  A residue without a (phi, psi) frame
    in either ensemble is left out of the mean (NaN when none is left).  per_residue: ({name: mean}, {name: (L,) array})."""
    maps = {k: v if isinstance(v, RamachandranMap) else ramachandran(v, bins, break_distance=break_distance) for k, v in ensembles.items()}
    ref = maps[ref_key]
    res, rows = {}, {}
    for k, m in maps.items():
        if k == ref_key:
            continue
        rows[k] = js_maps(m, ref)
        some = np.isfinite(rows[k])
        res[k] = float(rows[k][some].mean()) if some.any() else float("nan")
    res[ref_key] = 0.0
    rows[ref_key] = np.where(ref.counts[:, 2] > 0, 0.0, np.nan)
    if rounded:
        res = {k: round(v, 4) for k, v in res.items()}
    return (res, rows) if per_residue else res


def _as_torsions(x) -> BackboneTorsions:
    t = x if isinstance(x, BackboneTorsions) else torsions(x)
    assert t.degrees, "angles in degrees are compared"
    return t


def circular_difference(a, b):
    """|a - b| on the circle, degrees, in [0, 180]."""
    d = np.abs(np.asarray(a) - np.asarray(b)) % 360.0
    return np.minimum(d, 360.0 - d)


def torsion_agreement(samples, target, tolerance: float = 30.0) -> dict:
    """samples, target: BackboneTorsions, or anything `torsions` takes (the target's first structure is used) ->
      share        (n,) of the residues with phi and psi defined in both, the share whose phi and psi both lie within `tolerance`
                   degrees (circular difference) of the target's (NaN when there is none)
      share_mean, share_best, best_model
      per_residue  (L,) the share of the samples, among those with both angles there, that agree with the target (NaN where the target
                   lacks an angle or no sample has both)"""
    s, t = _as_torsions(samples), _as_torsions(target)
    assert s.phi.shape[1] == t.phi.shape[1], f"{s.phi.shape[1]} and {t.phi.shape[1]} residues: the correspondence is residue to residue"
    with np.errstate(invalid="ignore"):
        dphi, dpsi = circular_difference(s.phi, t.phi[0][None]), circular_difference(s.psi, t.psi[0][None])
        both = np.isfinite(dphi) & np.isfinite(dpsi)
        same = both & (dphi <= tolerance) & (dpsi <= tolerance)
    share = _fractions(same.sum(1).astype(np.float64), both.sum(1).astype(np.float64))
    per_residue = _fractions(same.sum(0).astype(np.float64), both.sum(0).astype(np.float64))
    some = np.isfinite(share)
    best = int(np.where(some, share, -1.0).argmax()) if some.any() else -1
    return {"tolerance": float(tolerance), "share": share, "share_mean": float(share[some].mean()) if some.any() else float("nan"),
            "share_best": float(share[best]) if best >= 0 else float("nan"), "best_model": best, "per_residue": per_residue}


def regions_of(t: BackboneTorsions, bins: int = 36, regions=REGIONS) -> np.ndarray:
    """(n, L) int: the region of every residue's (phi, psi) cell on the grid of `bins`, -1 where an angle is undefined."""
    table = _region_table(bins, regions)
    w = 360.0 / bins
    out = np.full(t.phi.shape, -1, np.int64)
    ok = np.isfinite(t.phi) & np.isfinite(t.psi)
    scale = 1.0 if t.degrees else DEG
    cell = []
    for a in (t.phi, t.psi):
        b = np.floor((a[ok] * scale + 180.0) / w).astype(np.int64)
        cell.append(np.clip(np.where(b >= bins, b - bins, b), 0, bins - 1))
    out[ok] = table[cell[0], cell[1]]
    return out


def region_string(t: BackboneTorsions, bins: int = 36, regions=REGIONS, letters=REGION_LETTERS) -> list:
    names = list(regions)
    return ["".join("-" if r < 0 else letters.get(names[r], "?") for r in row) for row in regions_of(t, bins, regions)]


def region_switches(samples, t1, t2, bins: int = 36, regions=REGIONS) -> list:
    """The residues with phi and psi defined in both targets whose region differs between them, each as {"residue": index from 0,
    "regions": the two names, "share": the fraction of the samples (having both angles) in target 1's region and in target 2's; None
    where no sample has them}: the torsion analogue of secondary.switch_residues and contacts.contact_switches."""
    m = samples if isinstance(samples, RamachandranMap) else ramachandran(samples, bins)
    a, b = (regions_of(_as_torsions(t), m.bins, regions)[0] for t in (t1, t2))
    prop, names = m.region_propensity(regions), list(regions)
    assert len(a) == len(b) == len(prop), "structures of different lengths (the correspondence is residue to residue)"
    out = []
    for l in np.nonzero((a >= 0) & (b >= 0) & (a != b))[0]:
        share = [None if np.isnan(prop[l, r]) else float(prop[l, r]) for r in (a[l], b[l])]
        out.append({"residue": int(l), "regions": [names[a[l]], names[b[l]]], "share": share})
    return out


def geometry_summary(backbone, ideal=IDEAL, length_tol: float = 0.05, angle_tol: float = 6.0, mask=None,
                     break_distance: float = BREAK_DISTANCE) -> dict:
    """Bond lengths (Angstrom) and bond angles (degrees) of backbones (or a BackboneTorsions made with geometry=True) against `ideal`:
      per quantity of QUANTITIES  mean, std, min, max over all defined instances, and `ideal`
      cis_fraction                the share of the defined omega that are cis
      outliers                    (n,) per structure the number of quantities further from ideal than length_tol / angle_tol; the C-N
                                  length counts only across a link (a chain break is no stretched bond)
      share_without_outliers
    The tolerances are parameters, not a pinned program: 0.05 Angstrom and 6 degrees are about 4 sigma of the Engh & Huber spreads."""
    t = backbone if isinstance(backbone, BackboneTorsions) else torsions(backbone, mask, break_distance, geometry=True)
    assert t.bond_lengths is not None and t.degrees, "a BackboneTorsions made with geometry=True, in degrees"
    values = np.concatenate([t.bond_lengths, t.bond_angles], axis=2)
    out, outliers = {}, np.zeros(values.shape[0], np.int64)
    for k, name in enumerate(QUANTITIES):
        v = values[:, :, k]
        ok = np.isfinite(v)
        if name == "c_n":
            ok &= v <= break_distance
        d = v[ok]
        out[name] = {"ideal": float(ideal[name]), "n": int(ok.sum()),
                     **{s: float(f(d)) if d.size else float("nan") for s, f in (("mean", np.mean), ("std", np.std), ("min", np.min), ("max", np.max))}}
        with np.errstate(invalid="ignore"):
            outliers += (ok & (np.abs(v - ideal[name]) > (length_tol if k < 3 else angle_tol))).sum(1)
    defined = np.isfinite(t.omega)
    out["cis_fraction"] = float(t.cis().sum() / defined.sum()) if defined.any() else float("nan")
    out["length_tol"], out["angle_tol"] = float(length_tol), float(angle_tol)
    out["outliers"] = outliers
    out["share_without_outliers"] = float((outliers == 0).mean()) if len(outliers) else float("nan")
    return out


def report(samples, targets=(), bins: int = 36, break_distance: float = BREAK_DISTANCE) -> dict:
    """The "torsions" block of analyze_ensemble: samples (n, L, A, 3), targets [(L, A, 3)].  js_ramachandran takes the targets together
    as one ensemble: with few targets that reference map is thin (a handful of cells per residue)."""
    pairs.need_device("esmdiff_amd.torsions.report")
    samples = backbone_array(samples)
    m = ramachandran(samples, bins, break_distance=break_distance)
    s = torsions(samples, break_distance=break_distance, geometry=True)
    out = {"bins": int(bins), "break_distance": float(break_distance), "n_frames": m.n_frames,
           "regions": {k: [list(r) for r in v] for k, v in REGIONS.items()}, "region_letters": "".join(REGION_LETTERS[k] for k in REGIONS),
           "counts": m.counts, "circular_mean": m.circular_mean(), "circular_variance": m.circular_variance(),
           "region_propensity": m.region_propensity(), "cis_fraction": m.cis_fraction(), "entropy": m.entropy(),
           "geometry": geometry_summary(s, break_distance=break_distance)}
    ts = [torsions(t, break_distance=break_distance) for t in targets]
    if ts:
        out["targets"] = [{"phi": t.phi[0], "psi": t.psi[0], "regions": region_string(t, bins)[0], "agreement": torsion_agreement(s, t)}
                          for t in ts]
        both = np.stack([backbone_array(t)[0][:, :3] for t in targets])
        res, rows = js_ramachandran({"samples": m, "target": ramachandran(both, bins, break_distance=break_distance)}, per_residue=True)
        out["js_ramachandran"] = {"mean": res["samples"], "per_residue": rows["samples"], "n_targets": len(ts)}
    if len(ts) == 2:
        out["region_switches"] = region_switches(m, ts[0], ts[1], bins)
    return out

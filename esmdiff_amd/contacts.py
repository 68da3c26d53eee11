"""Contacts of ensembles on the device: contact maps, native-contact fractions Q, switching contacts and internal scaling.

The layer above csrc/contacts.hip.  Two launches carry everything here:

  esmdiff_contact_map       an ensemble (n, L, 3) reduced over its frames into (L, L) maps: in how many frames a pair of residues is
                            resolved, in how many it is closer than the cutoff, and the sums of its distance and squared distance.
                            Memory is O(L^2) whatever the number of frames; the reference's PED evaluation
                            (eval_utils.idp_metrics, analysis/ped_analysis.py) and esmdiff_amd.metrics.idp_metrics build the whole
                            (n_frames, n_pairs) distance array for the same numbers.
  esmdiff_native_contacts   every sample against every native: how many of the native's contacts the sample keeps (integers), and
                            the smooth count of Best, Hummer & Eaton (PNAS 2013).

The fraction of native contacts Q has a closed definition and rests on no recalled program: a native contact is an ordered pair
(a, b), |a - b| >= min_separation, both resolved in the native and closer than `cutoff` there (d0); a sample keeps it when both are
resolved in the sample and d < lam * d0; the soft form adds 1 / (1 + exp(beta (d - lam d0))) per contact.  lam = 1.2 and
beta = 5 / Angstrom are the convention for CA contact maps; lam = 1.8 is the all-atom value of Best et al.  They are parameters,
not a pinned program.  The counts are held exactly to the numpy restatement tests/contacts_ref.py, the sums bit for bit.

Inputs are those of esmdiff_amd/ensemble.py: CA traces (n, L, 3) in Angstrom as arrays, tensors or a path (a multi-MODEL PDB or a
directory of PDBs); residues with NaN coordinates are masked, `mask` arguments (n, L) mask more.  Results are numpy arrays and floats
on the host.  There is no CPU fallback."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import pairs

CUTOFF = 8.0             # Angstrom between CA atoms: the reference's contact (eval_utils.idp_metrics)
MIN_SEPARATION = 3       # |a - b| of the closest pair looked at: the reference's pwd_offset
LAMBDA, BETA = 1.2, 5.0  # the CA convention of the soft / hard Q (all-atom: lam = 1.8)


@dataclass
class ContactMap:
    """count, valid int32 (L, L); sum_d, sum_d2 float64 (L, L): over the frames in which both residues are resolved (`valid` of them),
    the number with d < cutoff and the sums of d and d^2.  Symmetric; 0 where |a - b| < min_separation."""
    count: np.ndarray
    valid: np.ndarray
    sum_d: np.ndarray
    sum_d2: np.ndarray
    cutoff: float
    min_separation: int
    n_frames: int

    def _per_frame(self, total):
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(self.valid > 0, total / self.valid, np.nan)

    def frequency(self) -> np.ndarray:
        """The share of frames in contact, NaN where no frame has both residues."""
        return self._per_frame(self.count.astype(np.float64))

    def mean_distance(self) -> np.ndarray:
        return self._per_frame(self.sum_d)

    def std_distance(self) -> np.ndarray:
        """The population standard deviation sqrt(<d^2> - <d>^2), floored at 0."""
        return np.sqrt(np.maximum(self._per_frame(self.sum_d2) - self.mean_distance() ** 2, 0.0))

    def log_probability(self, pseudo_count: float = 0.01) -> np.ndarray:
        """The reference's log(mean(d < cutoff) + pseudo_count) (eval_utils.idp_metrics)."""
        return np.log(self.frequency() + pseudo_count)

    def pairs(self, offset: Optional[int] = None):
        """The index arrays (a, b) of the pairs b >= a + offset (default: min_separation), in numpy's triu order."""
        return np.triu_indices(self.count.shape[0], self.min_separation if offset is None else offset)


def contact_map(samples, cutoff: float = CUTOFF, min_separation: int = MIN_SEPARATION, mask=None) -> ContactMap:
    """The contact map of an ensemble: one esmdiff_contact_map call."""
    X = pairs.coords(samples, "samples")
    valid, count, sum_d, sum_d2 = pairs.contact_map(X, pairs.valid_mask(X, mask), cutoff, min_separation)
    return ContactMap(count.cpu().numpy(), valid.cpu().numpy(), sum_d.cpu().numpy(), sum_d2.cpu().numpy(), float(cutoff),
                      int(min_separation), int(X.shape[0]))


def contact_error(ensembles, ref_key: str = "target", pwd_offset: int = 3):
    """eval_utils.py:191-224's contact and distance numbers from the maps: the dictionaries (mse_contact, mae_contact, mse_pwd,
    mae_pwd) over the ensembles of `ensembles` ({name: (n, L, 3)}), each against ensembles[ref_key] — the mean squared / absolute
    difference, over the pairs j >= i + pwd_offset, of log(P(d < 8 A) + 0.01) and of the mean distance.  What
    esmdiff_amd.metrics.idp_metrics returns for those four, in O(L^2) memory."""
    def stats(ca):
        m = contact_map(ca, CUTOFF, pwd_offset)
        idx = m.pairs()
        return m.log_probability(0.01)[idx], m.mean_distance()[idx]

    ref = stats(ensembles[ref_key])
    out = tuple({} for _ in range(4))
    for name, ca in ensembles.items():
        cur = stats(ca)
        for j in range(2):
            diff = cur[j] - ref[j]
            out[2 * j][name] = float(np.mean(diff ** 2))
            out[2 * j + 1][name] = float(np.mean(np.abs(diff)))
    return out


@dataclass
class NativeContacts:
    """q, q_soft float64 (n, m): the hard and the soft fraction of native j's contacts that sample i keeps, NaN where the native has no
    contact; q_residue (n, m, L) (with per_residue, else None): the hard fraction of the contacts of residue a, NaN where it has none;
    kept (n, m), total (m,): the integer counts behind q."""
    q: np.ndarray
    q_soft: np.ndarray
    q_residue: Optional[np.ndarray]
    kept: np.ndarray
    total: np.ndarray


def native_contacts(samples, natives, cutoff: float = CUTOFF, min_separation: int = MIN_SEPARATION, lam: float = LAMBDA,
                    beta: float = BETA, per_residue: bool = False, mask_samples=None, mask_natives=None) -> NativeContacts:
    """The fraction of native contacts Q of every sample against every native (natives = None: the samples against themselves), no
    superposition: one esmdiff_native_contacts launch.  lam = 1.2 and beta = 5 / Angstrom are the convention for CA maps (lam = 1.8
    is the all-atom value of Best, Hummer & Eaton 2013): parameters, not a pinned program.  A contact whose residue is missing in the
    sample keeps nothing, adds 0 to the soft count, and stays in the denominator."""
    kept, total, kept_res, total_res, q_soft = pairs.native_contacts(*pairs.pair_args(samples, natives, mask_samples, mask_natives),
                                                                     cutoff, min_separation, lam, beta, per_residue)
    kept, total = kept.cpu().numpy(), total.cpu().numpy()
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(total[None] > 0, kept / total[None], np.nan)
        soft = np.where(total[None] > 0, q_soft.cpu().numpy() / total[None], np.nan)
        res = None
        if per_residue:
            total_res = total_res.cpu().numpy()
            res = np.where(total_res[None] > 0, kept_res.cpu().numpy() / total_res[None], np.nan)
    return NativeContacts(q, soft, res, kept, total)


def q_ensemble(samples, natives, **kwargs):
    """For every native the best sample's hard Q, and the mean of those over the natives -> (best (m,), mean): lddt_ensemble with Q for
    the lDDT.  A native without contacts is NaN in `best` and left out of the mean."""
    best = native_contacts(samples, natives, **kwargs).q.max(0)        # a column is NaN as a whole or not at all
    return best, float(np.mean(best[np.isfinite(best)])) if np.isfinite(best).any() else float("nan")


def contact_switches(samples, t1, t2, cutoff: float = CUTOFF, min_separation: int = MIN_SEPARATION, mask=None) -> list:
    """The contacts that switch between two states: the pairs a < b, resolved in both targets, in contact in exactly one of them, each
    as {"pair": [a, b], "state": 1 or 2 (the target that has the contact), "frequency": the share of the samples (having both
    residues) in which the contact is formed, None where no sample has them}.  The frequencies are contact_map's counts: the
    contact analogue of secondary.switch_residues."""
    ens = contact_map(samples, cutoff, min_separation, mask)
    s1, s2 = (contact_map(pairs.coords(t, f"t{k}")[:1], cutoff, min_separation) for k, t in ((1, t1), (2, t2)))
    assert s1.count.shape == s2.count.shape == ens.count.shape, "structures of different lengths (the correspondence is residue to residue)"
    both = (s1.valid > 0) & (s2.valid > 0)
    freq = ens.frequency()
    out = []
    for a, b in zip(*np.nonzero(np.triu(both & ((s1.count > 0) != (s2.count > 0)), 1))):
        out.append({"pair": [int(a), int(b)], "state": 1 if s1.count[a, b] > 0 else 2,
                    "frequency": None if np.isnan(freq[a, b]) else float(freq[a, b])})
    return out


@dataclass
class Scaling:
    """separation (L - 1,) = 1 .. L - 1; rms_distance (L - 1,): sqrt of the mean over the pairs (a, a + s) of <d^2>, NaN where no frame
    resolves any pair of that separation."""
    separation: np.ndarray
    rms_distance: np.ndarray


def internal_scaling(samples, mask=None) -> Scaling:
    """The internal scaling profile of an ensemble: the rms distance between residues s apart in sequence, from contact_map's
    sum_d2 / valid averaged over each diagonal (the pairs no frame resolves are left out)."""
    m = contact_map(samples, CUTOFF, 1, mask)
    msd = m._per_frame(m.sum_d2)
    L = msd.shape[0]
    rms = np.full(L - 1, np.nan)
    for s in range(1, L):
        d = np.diagonal(msd, s)
        if np.isfinite(d).any():
            rms[s - 1] = np.sqrt(np.nanmean(d))
    return Scaling(np.arange(1, L), rms)


def flory_exponent(scaling: Scaling, fit_range=None) -> float:
    """The Flory exponent nu of R(s) ~ s^nu: the least-squares slope of log R against log s over the separations lo <= s <= hi of
    fit_range = (lo, hi) (default: all with a finite, positive R).  Plain numpy on L - 1 numbers."""
    s, r = np.asarray(scaling.separation, np.float64), np.asarray(scaling.rms_distance, np.float64)
    ok = np.isfinite(r) & (r > 0)
    if fit_range is not None:
        ok &= (s >= fit_range[0]) & (s <= fit_range[1])
    if ok.sum() < 2:
        return float("nan")
    x, y = np.log(s[ok]), np.log(r[ok])
    x, y = x - x.mean(), y - y.mean()
    return float((x * y).sum() / (x * x).sum())


def report(samples, targets, cutoff: float = CUTOFF, min_separation: int = MIN_SEPARATION) -> dict:
    """The "contacts" block of analyze_ensemble: samples (n, L, 3), targets (K, L, 3)."""
    m = contact_map(samples, cutoff, min_separation)
    freq, mean = m.frequency(), m.mean_distance()
    a, b = np.nonzero(np.triu(m.count > 0, 1))
    scaling = internal_scaling(samples)
    nc = native_contacts(samples, targets, cutoff, min_separation)
    best, q_ens = q_ensemble(samples, targets, cutoff=cutoff, min_separation=min_separation)
    out = {"cutoff": float(cutoff), "min_separation": int(min_separation), "lam": LAMBDA, "beta": BETA,
           "contacts": [[int(i), int(j), float(freq[i, j]), float(mean[i, j])] for i, j in zip(a, b)],
           "scaling": {"separation": scaling.separation, "rms_distance": scaling.rms_distance},
           "flory_exponent": flory_exponent(scaling), "q_ens": q_ens,
           "targets": [{"n_contacts": int(nc.total[k]) // 2, "q": nc.q[:, k], "q_soft": nc.q_soft[:, k],
                        "q_mean": float(np.mean(nc.q[:, k])), "q_soft_mean": float(np.mean(nc.q_soft[:, k])),
                        "q_best": float(best[k]), "best_model": int(np.argmax(np.where(np.isnan(nc.q[:, k]), -1.0, nc.q[:, k])))}
                       for k in range(len(targets))]}
    if len(targets) == 2:
        out["contact_switches"] = contact_switches(samples, targets[0], targets[1], cutoff, min_separation)
    return out

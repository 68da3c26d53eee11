"""Superposition of ensembles on the device: all-pairs Kabsch RMSD and TM-score, with the reference's call shapes.

The layer the reference's two headline evaluations are written in — analysis/bpti_analysis.py:107-165 (TM-ens, RMSD-ens,
TM-div through slm/utils/tm_utils.py and slm/utils/geo_utils.py:58-122) and analysis/apo_analysis.py:182-288 (best TM to each
of two states, mean pairwise TM, per-residue "RMSF" from aligned sample pairs).  There every TM-score is a `TMscore -seq`
subprocess on two temporary PDB files and every alignment a scipy call; here one launch of csrc/superpose.hip (float64) scores
all pairs.  There is no CPU fallback.

[TMSCORE-RECALL], PARITY UNPINNED: the TM-score uses the fixed residue-to-residue correspondence (`TMscore -seq` on identical
sequences), the program's normalisation (the second, "native", structure's length; d0 = 1.24 (Ln - 15)^(1/3) - 1.8, floored at
0.5) and its fragment-seeded heuristic maximisation restated from memory — DESIGN.md ("Superposition") states the rule, and
tests/ensemble_ref.py restates it on the host.  The TMscore binary is in no tree this project can reach, so no value here has
been compared with the program's.  The RMSD side IS pinned: tests/golden/g13_superposition.npz holds the outputs of the
reference's own squared_deviation and of scipy's Rotation.align_vectors.

The lDDT functions at the end (csrc/lddt.hip) need no superposition and no recalled program: the score is a ratio of integer counts
of preserved distances, and those counts are held exactly to the numpy restatement tests/lddt_ref.py.

Coordinates are CA traces (n, L, 3) in Angstrom: arrays, tensors, or a path (a multi-MODEL PDB or a directory of PDBs, read by
pdbio.load_coords).  Residues with NaN coordinates are masked; `mask_*` arguments (n, L) mask more.  Results are numpy arrays /
floats on the host."""
from __future__ import annotations

import numpy as np
import torch

from . import pairs
from .pairs import LDDT_R0, LDDT_THRESHOLDS  # noqa: F401  (the defaults of the lDDT functions below)


def squared_deviation(xyz1, xyz2, reduction: str = "none"):
    """geo_utils.py:58-89: xyz1[k] aligned onto xyz2[k] ((B, L, 3) each, pair by pair) with the reference's rotation rule
    (reflections allowed, :116-119) -> per-residue squared deviation (B, L), or with reduction='rmsd' the RMSD (B,).
    numpy in, numpy out; tensors in, a float64 tensor on xyz1's device out."""
    if reduction not in ("none", "rmsd"):
        raise NotImplementedError(reduction)
    as_np = not torch.is_tensor(xyz1)
    A, B = pairs.coords(xyz1, "xyz1"), pairs.coords(xyz2, "xyz2")
    assert A.shape == B.shape, f"xyz1 {tuple(A.shape)} and xyz2 {tuple(B.shape)} differ"
    assert A.shape[1] > 1                                   # geo_utils.py:108
    nb, L = A.shape[:2]
    name = "sd" if reduction == "none" else "rmsd"
    out = torch.empty((nb, 1, L) if reduction == "none" else (nb, 1), dtype=torch.float64, device="cuda")
    for k in range(nb):                                     # the reference's shape is pair k with pair k, not all against all
        pairs.superpose(A[k:k + 1], B[k:k + 1], None, None, True, (name,), {name: out[k:k + 1]})
    out = out.squeeze(1)
    if as_np:
        return out.cpu().numpy()
    return out.to(xyz1.device)


def pairwise_rmsd(a, b=None, mask_a=None, mask_b=None, reflection: bool = False) -> np.ndarray:
    """RMSD after least-squares superposition of every a[i] onto every b[j] (b = None: a against itself) -> (n, m).
    reflection=False: proper rotations (scipy's align_vectors, the RMSD TMscore prints); True: the reference's geo_utils rule."""
    return pairs.superpose(*pairs.pair_args(a, b, mask_a, mask_b), reflection, ("rmsd",))["rmsd"].cpu().numpy()


def superposition(a, b=None, mask_a=None, mask_b=None, reflection: bool = False):
    """-> (R (n, m, 3, 3), t (n, m, 3)) with R a[i] + t ~ b[j]."""
    out = pairs.superpose(*pairs.pair_args(a, b, mask_a, mask_b), reflection, ("R", "t"))
    return out["R"].cpu().numpy(), out["t"].cpu().numpy()


def aligned_deviation(a, b=None, mask_a=None, mask_b=None) -> np.ndarray:
    """The per-residue distances (not squared) apo_analysis.py:235,257 takes after get_structures (:201-208) -> (n, m, L), NaN where
    either residue is masked.  get_structures centres each structure on the mean of its OWN resolved residues and then fits a
    rotation only (scipy's align_vectors, proper) on the residues resolved in both.  With equal masks that is the Kabsch
    superposition; with different masks it is not, and it is reproduced as it stands: a rotation-only fit about the origin is the
    Kabsch fit of the point sets doubled with their mirror images through the origin (centroids 0, the same covariance twice),
    so the kernel sees [x, -x] of length 2 L.  As everywhere here, unequal lengths of a and b and a mask_b without b are refused."""
    A, B, ma, mb = pairs.pair_args(a, b, mask_a, mask_b)
    L = A.shape[1]

    def doubled(x, m):
        w = torch.ones(x.shape[:2], dtype=torch.float64, device="cuda") if m is None else m.to(torch.float64)
        xc = torch.where(w[..., None] > 0, x, torch.zeros_like(x))
        xc = x - (xc * w[..., None]).sum(1, keepdim=True) / w.sum(1, keepdim=True)[..., None]      # nanmean over its own residues
        return torch.cat([xc, -xc], dim=1).contiguous(), None if m is None else torch.cat([m, m], dim=1).contiguous()

    A2, ma2 = doubled(A, ma)
    B2, mb2 = (None, None) if B is None else doubled(B, mb)
    sd = pairs.superpose(A2, B2, ma2, mb2, False, ("sd",))["sd"]
    return torch.sqrt(sd[..., :L]).cpu().numpy()


def tm_matrix(models, natives=None, mask_models=None, mask_natives=None, return_transform: bool = False):
    """TM-score of every model against every native (natives = None: the models against themselves) -> (n, m), normalised by
    the native's number of valid residues.  [TMSCORE-RECALL], parity unpinned (module docstring).  return_transform: also R, t of
    the best superposition found (R model + t ~ native)."""
    out = pairs.tm(*pairs.pair_args(models, natives, mask_models, mask_natives), transform=return_transform)
    if return_transform:
        return tuple(x.cpu().numpy() for x in out)
    return out.cpu().numpy()


def tm_score(model, native, mask_model=None, mask_native=None) -> float:
    """tm_utils.py:46-59 `tmscore(model, native)` for two (L, 3) traces of the same sequence."""
    return float(tm_matrix(model, native, mask_model, mask_native)[0, 0])


# ---- the reference's ensemble functions (tm_utils.py:62-154) -----------------------------------------------------------
def tm_ensemble(samples, t1, t2) -> float:
    """tm_utils.py:62-86: 0.5 max_i TM(sample_i, t1) + 0.5 max_i TM(sample_i, t2)."""
    natives = torch.cat([pairs.coords(t1, "t1")[:1], pairs.coords(t2, "t2")[:1]], dim=0)
    tm = tm_matrix(samples, natives)
    return float(0.5 * tm[:, 0].max() + 0.5 * tm[:, 1].max())


def tm_n_ensemble(samples, natives, max_n_model: int = 100, rng=0, verbose: bool = False):
    """tm_utils.py:88-135: for every native the best TM-score and the best RMSD (the proper-rotation RMSD TMscore prints) over the
    samples -> (best_tm_list, best_rmsd_list).  More than max_n_model samples are down-sampled without replacement from `rng`
    (a numpy Generator or a seed; the reference draws from the global np.random)."""
    S = pairs.coords(samples, "samples")
    K = pairs.coords(natives, "natives")
    if S.shape[0] > max_n_model:
        gen = rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)
        keep = gen.choice(S.shape[0], max_n_model, replace=False)
        if verbose:
            print(f"Downsample {S.shape[0]} models to {max_n_model} models.")
        S = S[torch.as_tensor(keep, device="cuda")].contiguous()
    tm, rmsd = tm_matrix(S, K), pairwise_rmsd(S, K)
    best_tm, best_rmsd = [float(v) for v in tm.max(0)], [float(v) for v in rmsd.min(0)]
    if verbose:
        print("Best-TM-score", ",".join(map(str, best_tm)))
        print("Best-RMSD", ",".join(map(str, best_rmsd)))
        print("Best-TM-ids", ",".join(map(str, tm.argmax(0))))
        print("Best-RMSD-ids", ",".join(map(str, rmsd.argmin(0))))
        print("TM-ensemble", np.mean(best_tm))
        print("RMSD-ensemble", np.mean(best_rmsd))
    return best_tm, best_rmsd


def tm_diversity(samples) -> float:
    """tm_utils.py:137-154: the mean of TM(sample_i, sample_j) over i < j."""
    tm = tm_matrix(samples)
    iu = np.triu_indices(tm.shape[0], 1)
    return float(np.mean(tm[iu]))


def apo_report(samples, struct1, struct2, mask1=None, mask2=None) -> dict:
    """One target's row of apo_analysis.analyze (:222-272): samples (n, L, 3), the two states (L, 3) each (unresolved residues NaN
    or masked) -> tm1max / tm2max (best TM of a state against the samples, :247-250, :265), tm_ens (:266), ensvar (mean TM over
    sample pairs j < k, :252-255, :262), tmpair (mean of both normalisations of the two states, :267-272), rmsd (per-residue
    distance between the states after get_structures, :234-235) and rmsf (sqrt of the mean over sample pairs of the squared
    aligned deviation, :256-260)."""
    S = pairs.coords(samples, "samples")
    s1, s2 = pairs.coords(struct1, "struct1")[:1], pairs.coords(struct2, "struct2")[:1]
    states = torch.cat([s1, s2], dim=0)
    ms = None
    if mask1 is not None or mask2 is not None:
        L = S.shape[1]
        ms = np.stack([np.ones(L, bool) if m is None else np.asarray(m, bool).reshape(L) for m in (mask1, mask2)])
    tm_states = tm_matrix(states, S, mask_models=ms)                 # tmscore(path1 / path2, sample): the sample is the native
    tm1max, tm2max = float(tm_states[0].max()), float(tm_states[1].max())
    n = S.shape[0]
    lo = np.tril_indices(n, -1)                                      # tmscore(path4 = sample k, path3 = sample j), j < k
    pair_tm = tm_matrix(S)
    dev = aligned_deviation(S)
    iu = np.triu_indices(n, 1)
    cross = tm_matrix(states, mask_models=ms)
    return {"tm1max": tm1max, "tm2max": tm2max, "tm_ens": (tm1max + tm2max) / 2,
            "ensvar": float(np.mean(pair_tm[lo])) if n > 1 else float("nan"),
            "tmpair": float((cross[0, 1] + cross[1, 0]) / 2),
            "rmsd": aligned_deviation(s1, s2, None if ms is None else ms[:1], None if ms is None else ms[1:])[0, 0],
            "rmsf": np.sqrt(np.mean(dev[iu] ** 2, axis=0)) if n > 1 else np.full(S.shape[1], np.nan)}


# ---- lDDT: the superposition-free score (csrc/lddt.hip) ------------------------------------------------------------------
def lddt_matrix(models, natives=None, mask_models=None, mask_natives=None, per_residue: bool = False, r0: float = LDDT_R0,
                thresholds=LDDT_THRESHOLDS, seq_sep: int = 1):
    """CA-lDDT (Mariani et al. 2013) of every model against every native (natives = None: the models against themselves) -> (n, m)
    float64, no superposition.  For native j the ordered residue pairs (a, b), |a - b| >= seq_sep, both resolved, closer than r0 in
    the native are its pair set; a pair is kept once per threshold t with |d_model - d_native| < t (a pair whose model residue is
    missing keeps nothing); the score is kept / (n_thresholds * pairs), pooled over the chain.  per_residue: also the (n, m, L) array
    of the same ratio per residue a.  NaN where a native (a residue) has no pair.  The device returns the integer counts
    (csrc/lddt.hip, equal to tests/lddt_ref.py's); the one division is done here."""
    kept, total, kept_res, total_res = pairs.lddt_counts(*pairs.pair_args(models, natives, mask_models, mask_natives), per_residue, r0,
                                                         thresholds, seq_sep)
    nt = len(thresholds)
    with np.errstate(invalid="ignore", divide="ignore"):
        score = kept.cpu().numpy() / (nt * total.cpu().numpy())[None]
        if not per_residue:
            return score
        return score, kept_res.cpu().numpy() / (nt * total_res.cpu().numpy())[None]


def lddt(model, native, mask_model=None, mask_native=None, r0: float = LDDT_R0, thresholds=LDDT_THRESHOLDS, seq_sep: int = 1) -> float:
    """The lDDT of one (L, 3) CA trace against one native."""
    return float(lddt_matrix(model, native, mask_model, mask_native, False, r0, thresholds, seq_sep)[0, 0])


def lddt_ensemble(samples, natives) -> float:
    """For every native the best sample's lDDT, averaged over the natives: tm_n_ensemble's TM-ensemble with lDDT for the TM-score."""
    return float(np.mean(lddt_matrix(samples, natives).max(0)))


def lddt_diversity(samples) -> float:
    """The mean of the symmetric lDDT (l[i, j] + l[j, i]) / 2 over the sample pairs i < j (NaN for fewer than two samples)."""
    l = lddt_matrix(samples)
    iu = np.triu_indices(l.shape[0], 1)
    return float(np.mean(0.5 * (l + l.T)[iu])) if len(iu[0]) else float("nan")


def plddt_agreement(samples, native, plddt, scale: float = 1.0) -> dict:
    """The decoder's per-residue confidence against what it predicts.  samples (n, L, 3), native (L, 3), plddt (n, L) as written
    into the samples' B-factors, divided by `scale` to reach [0, 1] ->
      observed (L,)    the mean over the samples of the per-residue lDDT against `native` (NaN: a residue without pairs)
      predicted (L,)   the mean over the samples of plddt / scale
      pearson_r        of the two over the residues where both are finite (NaN if either is constant)
      mean_abs_diff    the mean |observed - predicted| over the same residues"""
    _, res = lddt_matrix(samples, native, per_residue=True)
    res = res[:, 0]
    pred = np.asarray(plddt, np.float64) / float(scale)
    if pred.ndim == 1:
        pred = pred[None]
    assert pred.shape == res.shape, f"plddt {pred.shape} does not match the samples {res.shape}"
    observed, predicted = res.mean(0), pred.mean(0)
    ok = np.isfinite(observed) & np.isfinite(predicted)
    o, q = observed[ok] - observed[ok].mean(), predicted[ok] - predicted[ok].mean()
    den = np.sqrt((o * o).sum() * (q * q).sum())
    return {"observed": observed, "predicted": predicted, "pearson_r": float((o * q).sum() / den) if den > 0 else float("nan"),
            "mean_abs_diff": float(np.mean(np.abs(observed[ok] - predicted[ok])))}

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

import ctypes
import os
from pathlib import Path
from typing import Optional

import numpy as np
import torch

from . import _native as N


def _coords(x) -> np.ndarray:
    if isinstance(x, (str, os.PathLike)):
        from .pdbio import load_coords
        return load_coords(Path(x), max_n_model=None, verbose=False)
    return x


def _dev(x, what: str = "coords") -> torch.Tensor:
    if not torch.cuda.is_available():
        raise RuntimeError("esmdiff_amd.ensemble needs an MI355X (gfx950); there is no CPU fallback")
    x = _coords(x)
    t = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))
    if t.dim() == 2:
        t = t[None]
    if t.dim() != 3 or t.shape[-1] != 3 or t.shape[0] == 0 or t.shape[1] == 0:
        raise AssertionError(f"{what} should be (n, L, 3) CA coordinates, got {tuple(t.shape)}")
    return t.to(device="cuda", dtype=torch.float64).contiguous()


def _mask(t: torch.Tensor, mask) -> Optional[torch.Tensor]:
    """u8 (n, L): resolved (no NaN coordinate) and not masked by the caller; None when every residue is valid."""
    ok = ~torch.isnan(t).any(-1)
    if mask is not None:
        m = torch.as_tensor(np.asarray(mask) if not torch.is_tensor(mask) else mask).to("cuda").bool()
        if m.dim() == 1:
            m = m[None]
        assert m.shape == ok.shape, f"mask {tuple(m.shape)} does not match the coordinates {tuple(ok.shape)}"
        ok = ok & m
    return None if bool(ok.all()) else ok.to(torch.uint8).contiguous()


def _p(t: Optional[torch.Tensor], offset: int = 0):
    return ctypes.c_void_p(0 if t is None else t.data_ptr() + offset)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check(code: int, what: str, L: int):
    if code == -5:
        raise RuntimeError(f"{what}: L = {L} is beyond the kernel's limit ({N.TM_MAX_L} residues: both structures of a pair are "
                           f"staged in LDS); there is no slow path")
    if code != 0:
        raise RuntimeError(f"libesmdiff_hip {what} failed ({code})")


def _pair_args(a, b, mask_a, mask_b):
    A = _dev(a)
    ma = _mask(A, mask_a)
    if b is None:
        assert mask_b is None, "mask_b without b"
        return A, None, ma, None, A.shape[0], A.shape[0]
    B = _dev(b)
    assert B.shape[1] == A.shape[1], f"structures of different lengths: {A.shape[1]} and {B.shape[1]} (the correspondence is residue to residue)"
    return A, B, ma, _mask(B, mask_b), A.shape[0], B.shape[0]


def _superpose(a, b, mask_a, mask_b, reflection: bool, want):
    """One esmdiff_superpose_pairs launch -> {name: device tensor} for the names in `want` (rmsd, sd, R, t)."""
    A, B, ma, mb, n, m = _pair_args(a, b, mask_a, mask_b)
    L = A.shape[1]
    shapes = {"rmsd": (n, m), "sd": (n, m, L), "R": (n, m, 3, 3), "t": (n, m, 3)}
    out = {k: torch.empty(shapes[k], dtype=torch.float64, device="cuda") for k in want}
    code = N.lib().esmdiff_superpose_pairs(_p(A), n, _p(B), m, L, _p(ma), _p(mb), int(bool(reflection)), _p(out.get("rmsd")),
                                           _p(out.get("sd")), _p(out.get("R")), _p(out.get("t")), _stream())
    _check(code, "esmdiff_superpose_pairs", L)
    return out


def squared_deviation(xyz1, xyz2, reduction: str = "none"):
    """geo_utils.py:58-89: xyz1[k] aligned onto xyz2[k] ((B, L, 3) each, pair by pair) with the reference's rotation rule
    (reflections allowed, :116-119) -> per-residue squared deviation (B, L), or with reduction='rmsd' the RMSD (B,).
    numpy in, numpy out; tensors in, a float64 tensor on xyz1's device out."""
    if reduction not in ("none", "rmsd"):
        raise NotImplementedError(reduction)
    as_np = not torch.is_tensor(xyz1)
    A, B = _dev(xyz1, "xyz1"), _dev(xyz2, "xyz2")
    assert A.shape == B.shape, f"xyz1 {tuple(A.shape)} and xyz2 {tuple(B.shape)} differ"
    assert A.shape[1] > 1                                   # geo_utils.py:108
    nb, L = A.shape[:2]
    out = torch.empty((nb, L) if reduction == "none" else (nb,), dtype=torch.float64, device="cuda")
    fn, row = N.lib().esmdiff_superpose_pairs, L * 3 * 8
    for k in range(nb):                                     # the reference's shape is pair k with pair k, not all against all
        if reduction == "none":
            code = fn(_p(A, k * row), 1, _p(B, k * row), 1, L, None, None, 1, None, _p(out, k * L * 8), None, None, _stream())
        else:
            code = fn(_p(A, k * row), 1, _p(B, k * row), 1, L, None, None, 1, _p(out, k * 8), None, None, None, _stream())
        _check(code, "esmdiff_superpose_pairs", L)
    if as_np:
        return out.cpu().numpy()
    return out.to(xyz1.device)


def pairwise_rmsd(a, b=None, mask_a=None, mask_b=None, reflection: bool = False) -> np.ndarray:
    """RMSD after least-squares superposition of every a[i] onto every b[j] (b = None: a against itself) -> (n, m).
    reflection=False: proper rotations (scipy's align_vectors, the RMSD TMscore prints); True: the reference's geo_utils rule."""
    return _superpose(a, b, mask_a, mask_b, reflection, ("rmsd",))["rmsd"].cpu().numpy()


def superposition(a, b=None, mask_a=None, mask_b=None, reflection: bool = False):
    """-> (R (n, m, 3, 3), t (n, m, 3)) with R a[i] + t ~ b[j]."""
    out = _superpose(a, b, mask_a, mask_b, reflection, ("R", "t"))
    return out["R"].cpu().numpy(), out["t"].cpu().numpy()


def aligned_deviation(a, b=None, mask_a=None, mask_b=None) -> np.ndarray:
    """The per-residue distances (not squared) apo_analysis.py:235,257 takes after get_structures (:201-208) -> (n, m, L), NaN where
    either residue is masked.  get_structures centres each structure on the mean of its OWN resolved residues and then fits a
    rotation only (scipy's align_vectors, proper) on the residues resolved in both.  With equal masks that is the Kabsch
    superposition; with different masks it is not, and it is reproduced as it stands: a rotation-only fit about the origin is the
    Kabsch fit of the point sets doubled with their mirror images through the origin (centroids 0, the same covariance twice),
    so the kernel sees [x, -x] of length 2 L."""
    A = _dev(a)
    ma = _mask(A, mask_a)
    B, mb = (A, ma) if b is None else (_dev(b), None)
    if b is not None:
        mb = _mask(B, mask_b)
    L = A.shape[1]

    def doubled(x, m):
        w = torch.ones(x.shape[:2], dtype=torch.float64, device="cuda") if m is None else m.to(torch.float64)
        xc = torch.where(w[..., None] > 0, x, torch.zeros_like(x))
        xc = x - (xc * w[..., None]).sum(1, keepdim=True) / w.sum(1, keepdim=True)[..., None]      # nanmean over its own residues
        return torch.cat([xc, -xc], dim=1).contiguous(), None if m is None else torch.cat([m, m], dim=1).contiguous()

    A2, ma2 = doubled(A, ma)
    B2, mb2 = (A2, ma2) if b is None else doubled(B, mb)
    n, m = A2.shape[0], B2.shape[0]
    sd = torch.empty(n, m, 2 * L, dtype=torch.float64, device="cuda")
    code = N.lib().esmdiff_superpose_pairs(_p(A2), n, _p(B2), m, 2 * L, _p(ma2), _p(mb2), 0, None, _p(sd), None, None, _stream())
    _check(code, "esmdiff_superpose_pairs", L)
    return torch.sqrt(sd[..., :L]).cpu().numpy()


def tm_matrix(models, natives=None, mask_models=None, mask_natives=None, return_transform: bool = False):
    """TM-score of every model against every native (natives = None: the models against themselves) -> (n, m), normalised by
    the native's number of valid residues.  [TMSCORE-RECALL], parity unpinned (module docstring).  return_transform: also R, t of
    the best superposition found (R model + t ~ native)."""
    A, B, ma, mb, n, m = _pair_args(models, natives, mask_models, mask_natives)
    L = A.shape[1]
    tm = torch.empty(n, m, dtype=torch.float64, device="cuda")
    R = torch.empty(n, m, 3, 3, dtype=torch.float64, device="cuda") if return_transform else None
    t = torch.empty(n, m, 3, dtype=torch.float64, device="cuda") if return_transform else None
    _check(N.lib().esmdiff_tm_pairs(_p(A), n, _p(B), m, L, _p(ma), _p(mb), _p(tm), _p(R), _p(t), _stream()), "esmdiff_tm_pairs", L)
    if return_transform:
        return tm.cpu().numpy(), R.cpu().numpy(), t.cpu().numpy()
    return tm.cpu().numpy()


def tm_score(model, native, mask_model=None, mask_native=None) -> float:
    """tm_utils.py:46-59 `tmscore(model, native)` for two (L, 3) traces of the same sequence."""
    return float(tm_matrix(model, native, mask_model, mask_native)[0, 0])


# ---- the reference's ensemble functions (tm_utils.py:62-154) -----------------------------------------------------------
def tm_ensemble(samples, t1, t2) -> float:
    """tm_utils.py:62-86: 0.5 max_i TM(sample_i, t1) + 0.5 max_i TM(sample_i, t2)."""
    natives = torch.cat([_dev(t1, "t1")[:1], _dev(t2, "t2")[:1]], dim=0)
    tm = tm_matrix(samples, natives)
    return float(0.5 * tm[:, 0].max() + 0.5 * tm[:, 1].max())


def tm_n_ensemble(samples, natives, max_n_model: int = 100, rng=0, verbose: bool = False):
    """tm_utils.py:88-135: for every native the best TM-score and the best RMSD (the proper-rotation RMSD TMscore prints) over the
    samples -> (best_tm_list, best_rmsd_list).  More than max_n_model samples are down-sampled without replacement from `rng`
    (a numpy Generator or a seed; the reference draws from the global np.random)."""
    S = _dev(samples, "samples")
    K = _dev(natives, "natives")
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
    S = _dev(samples, "samples")
    s1, s2 = _dev(struct1, "struct1")[:1], _dev(struct2, "struct2")[:1]
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
LDDT_R0 = 15.0
LDDT_THRESHOLDS = (0.5, 1.0, 2.0, 4.0)


def _lddt_counts(A, B, ma, mb, n: int, m: int, per_residue: bool = False, r0: float = LDDT_R0, thresholds=LDDT_THRESHOLDS,
                 seq_sep: int = 1):
    """One esmdiff_lddt_pairs launch on device tensors (B None: A against itself) -> int32 device tensors kept (n, m),
    total (m,), and with per_residue kept_res (n, m, L) and total_res (m, L) (else None, and never allocated)."""
    L = A.shape[1]
    thr = [float(t) for t in thresholds]
    kept = torch.empty((n, m), dtype=torch.int32, device="cuda")
    total = torch.empty((m,), dtype=torch.int32, device="cuda")
    kept_res = torch.empty((n, m, L), dtype=torch.int32, device="cuda") if per_residue else None
    total_res = torch.empty((m, L), dtype=torch.int32, device="cuda") if per_residue else None
    code = N.lib().esmdiff_lddt_pairs(_p(A), n, _p(B), m, L, _p(ma), _p(mb), float(r0), (ctypes.c_double * len(thr))(*thr), len(thr),
                                      int(seq_sep), _p(kept), _p(total), _p(kept_res), _p(total_res), _stream())
    if code == -5:
        raise RuntimeError(f"esmdiff_lddt_pairs: L = {L} is beyond the kernel's limit ({N.LDDT_MAX_L} residues: a model is staged in "
                           f"LDS); there is no slow path")
    if code == -1:
        raise RuntimeError(f"esmdiff_lddt_pairs: invalid argument: L = {L} (at least 2), seq_sep = {seq_sep} (at least 1), "
                           f"{len(thr)} thresholds (1 to {N.LDDT_MAX_THRESHOLDS})")
    if code != 0:
        raise RuntimeError(f"libesmdiff_hip esmdiff_lddt_pairs failed ({code})")
    return kept, total, kept_res, total_res


def _lddt_device(A, B, ma, mb, r0: float = LDDT_R0, thresholds=LDDT_THRESHOLDS, seq_sep: int = 1) -> torch.Tensor:
    """lDDT (n, m) float64 on the device: kept / (n_thresholds total), NaN where the native has no pair."""
    n, m = A.shape[0], (A if B is None else B).shape[0]
    kept, total, _, _ = _lddt_counts(A, B, ma, mb, n, m, False, r0, thresholds, seq_sep)
    return kept.to(torch.float64) / (len(thresholds) * total).to(torch.float64)[None]


def lddt_matrix(models, natives=None, mask_models=None, mask_natives=None, per_residue: bool = False, r0: float = LDDT_R0,
                thresholds=LDDT_THRESHOLDS, seq_sep: int = 1):
    """CA-lDDT (Mariani et al. 2013) of every model against every native (natives = None: the models against themselves) -> (n, m)
    float64, no superposition.  For native j the ordered residue pairs (a, b), |a - b| >= seq_sep, both resolved, closer than r0 in
    the native are its pair set; a pair is kept once per threshold t with |d_model - d_native| < t (a pair whose model residue is
    missing keeps nothing); the score is kept / (n_thresholds * pairs), pooled over the chain.  per_residue: also the (n, m, L) array
    of the same ratio per residue a.  NaN where a native (a residue) has no pair.  The device returns the integer counts
    (csrc/lddt.hip, equal to tests/lddt_ref.py's); the one division is done here."""
    A, B, ma, mb, n, m = _pair_args(models, natives, mask_models, mask_natives)
    kept, total, kept_res, total_res = _lddt_counts(A, B, ma, mb, n, m, per_residue, r0, thresholds, seq_sep)
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

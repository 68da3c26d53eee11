"""Slow coordinates of a trajectory on the device: time-lagged moments fused from the CA coordinates, TICA / VAMP models, implied
timescales, VAMP-2 scores, free-energy grids and the reference's js_tica through them.

The reference's BPTI evaluation opens with js_tica(..., lagtime=500) on the whole MD trajectory (analysis/bpti_analysis.py,
eval_utils.py:258-289).  esmdiff_amd.metrics.js_tica does that with an (n, D) distance matrix, two centred copies and four library
products; here the three entries of csrc/lagged.hip recompute the distances inside their kernels, so a fit costs O(D^2) memory
whatever the number of frames, every sum has a published order (two runs agree bit for bit), and the model is an object a caller
can keep: eigenvalues, timescales, transform.  The one or two dense (D, D) eigenproblems stay torch.linalg calls on the device, as in
metrics.tica_fit and flexibility.pca.  There is no CPU fallback.

The features are the CA distances of the pairs (i, j >= i + pwd_offset) in numpy.triu_indices order (pwd_offset = 1: the reference's
js_tica), or, with features=True, the columns of an (n, D) matrix given as it is."""
from __future__ import annotations

import os
from dataclasses import dataclass
from pathlib import Path
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native as N
from . import pairs


# ---- host-only arithmetic -------------------------------------------------------------------------------------------------------
def timescales_from_eigenvalues(eigenvalues, lagtime: int) -> np.ndarray:
    """-lagtime / ln |lambda|; NaN where |lambda| >= 1 or lambda <= 0 (no relaxation time belongs to such a value)."""
    lam = np.asarray(eigenvalues, np.float64)
    out = np.full(lam.shape, np.nan)
    ok = (lam > 0.0) & (np.abs(lam) < 1.0)
    out[ok] = -float(lagtime) / np.log(np.abs(lam[ok]))
    return out


def free_energy(proj, bins=50, kT: float = 1.0, range=None):
    """proj (n,) or (n, k) -> (edges, F): the equal-width histogram's edges (a list of k arrays; numpy.histogramdd's) and
    F = -kT ln p with p the share of the frames in each cell, +inf in an empty cell."""
    p = np.asarray(proj, np.float64)
    p = p[:, None] if p.ndim == 1 else p
    if p.ndim != 2 or p.shape[0] == 0 or not np.isfinite(p).all():
        raise ValueError(f"free_energy takes finite projections (n,) or (n, k) with n >= 1, got {p.shape}")
    counts, edges = np.histogramdd(p, bins=bins, range=range)
    total = counts.sum()
    if total == 0:
        raise ValueError("free_energy: no frame falls into the range")
    with np.errstate(divide="ignore"):
        F = -float(kT) * np.log(counts / total)
    F[counts == 0] = np.inf
    return edges, F


def chunk_spans(n: int, lagtime: int, chunk_frames: int) -> List[Tuple[int, int]]:
    """The frame ranges [start, stop) a trajectory of n frames is uploaded in: every range holds the pairs (t, t + lagtime) of
    chunk_frames consecutive t, so consecutive ranges overlap by lagtime frames and every pair t < n - lagtime is in exactly one."""
    if chunk_frames < 1:
        raise ValueError(f"chunk_frames must be at least 1, got {chunk_frames}")
    m = n - lagtime
    return [(s, min(s + chunk_frames, m) + lagtime) for s in range(0, max(m, 0), chunk_frames)]


def pair_count(lengths: Sequence[int], lagtime: int) -> int:
    """The pairs (t, t + lagtime) of a list of trajectories: pairs never cross a boundary."""
    return sum(max(int(n) - lagtime, 0) for n in lengths)


# ---- input ----------------------------------------------------------------------------------------------------------------------
def _check_lag(lagtime) -> int:
    if int(lagtime) != lagtime or int(lagtime) < 1:
        raise ValueError(f"lagtime must be an integer >= 1, got {lagtime}")
    return int(lagtime)


def _device(x, features: bool, pwd_offset: int) -> torch.Tensor:
    """One trajectory (an array or a tensor) -> f64 on the device, (n, D) with features else (n, L, 3); finite, within the limits."""
    if not torch.is_tensor(x):
        x = np.asarray(x)
        x = x if x.flags.writeable else x.copy()                   # a read-only memmap's piece: torch wants a writable array
    t = x if torch.is_tensor(x) else torch.as_tensor(x)
    if features:
        if t.dim() != 2 or t.shape[1] < 1:
            raise ValueError(f"features=True takes (n, D) features, got {tuple(t.shape)}")
        if t.shape[1] > N.LAGGED_MAX_D:
            raise ValueError(f"D = {t.shape[1]} features are beyond the kernel's limit ({N.LAGGED_MAX_D})")
    else:
        if t.dim() != 3 or t.shape[2] != 3:
            raise ValueError(f"a trajectory should be (n, L, 3) CA coordinates, got {tuple(t.shape)}")
        if not 1 <= pwd_offset < t.shape[1]:
            raise ValueError(f"pwd_offset = {pwd_offset} leaves no pair of {t.shape[1]} residues (1 <= pwd_offset < L)")
        if t.shape[1] > N.LAGGED_MAX_L:
            raise ValueError(f"L = {t.shape[1]} residues are beyond the kernel's limit ({N.LAGGED_MAX_L}: D <= {N.LAGGED_MAX_D} features)")
    pairs.need_device("esmdiff_amd.kinetics")
    t = t.to(device="cuda", dtype=torch.float64).contiguous()
    if not bool(torch.isfinite(t).all()):
        raise ValueError("coords should not contain nan or inf")
    return t


def _trajectories(x, features: bool) -> list:
    """x: an array or tensor, a PDB path (every MODEL a frame), or a list of those -> a list of host arrays / tensors / memmaps."""
    if isinstance(x, (str, os.PathLike)):
        from .pdbio import load_coords
        return [load_coords(Path(x), max_n_model=None, verbose=False)]
    if isinstance(x, (list, tuple)):
        if not x:
            raise ValueError("an empty list of trajectories")
        return [_trajectories(t, features)[0] for t in x]
    return [x]


def _pieces(traj, lagtime: int, chunk_frames: Optional[int]):
    """One trajectory -> the pieces it is uploaded in (chunk_spans; one piece without chunk_frames)."""
    n = traj.shape[0]
    if chunk_frames is None:
        yield traj
    else:
        for s, e in chunk_spans(n, lagtime, int(chunk_frames)):
            yield np.ascontiguousarray(traj[s:e]) if not torch.is_tensor(traj) else traj[s:e]


# ---- moments --------------------------------------------------------------------------------------------------------------------
@dataclass
class LaggedMoments:
    """The raw time-lagged moments of a trajectory's features about `center` (tensors on the device, float64): with a = f(x_t) - center
    and b = f(x_{t + lagtime}) - center over the m pairs, S00 = sum a a^T, S0t = sum a b^T, Stt = sum b b^T, r0 = sum a, rt = sum b;
    mean0 and meant are the means of the two windows."""
    m: int
    lagtime: int
    mean0: torch.Tensor
    meant: torch.Tensor
    center: torch.Tensor
    S00: torch.Tensor
    S0t: torch.Tensor
    Stt: torch.Tensor
    r0: torch.Tensor
    rt: torch.Tensor

    def mean(self, reversible: bool = True) -> torch.Tensor:
        """The estimator's own mean: of both windows together (reversible) or of the first window."""
        return self.center + ((self.r0 + self.rt) / (2.0 * self.m) if reversible else self.r0 / float(self.m))

    def covariances(self, reversible: bool = True):
        """-> c00, c0t (reversible: the symmetrised estimator of metrics.tica_fit, one mean for both windows) or c00, c0t, ctt (each
        window about its own mean), corrected from the centre to the estimator's means with the residual sums."""
        m = float(self.m)
        if reversible:
            d = (self.r0 + self.rt) / (2.0 * m)
            dd = torch.outer(d, d)
            return (self.S00 + self.Stt) / (2.0 * m) - dd, (self.S0t + self.S0t.T) / (2.0 * m) - dd
        d0, dt = self.r0 / m, self.rt / m
        return self.S00 / m - torch.outer(d0, d0), self.S0t / m - torch.outer(d0, dt), self.Stt / m - torch.outer(dt, dt)


def lagged_moments(x, lagtime: int, center=None, pwd_offset: int = 1, features: bool = False, chunk_frames: Optional[int] = None) -> LaggedMoments:
    """x: (n, L, 3) CA coordinates (an array, a tensor, a PDB path, or a host numpy.memmap read chunk_frames pairs at a time), or a
    list of such trajectories -> LaggedMoments.  center=None: one pass for the window means (esmdiff_lagged_means), the centre
    (mean0 + meant) / 2, then the moments pass: no cancellation.  A list: pairs never cross a boundary; raw sums and pair counts
    are added in list order.  chunk_frames: pieces overlapping by lagtime, one means pass then one moments pass, sums added in
    piece order."""
    lagtime = _check_lag(lagtime)
    pwd = 0 if features else int(pwd_offset)
    trajs = _trajectories(x, features)
    usable = [t for t in trajs if t.shape[0] > lagtime]
    if not usable:
        raise ValueError(f"TICA needs more than lagtime = {lagtime} frames in a trajectory, got {[int(t.shape[0]) for t in trajs]}")
    m = pair_count([t.shape[0] for t in usable], lagtime)
    whole = len(usable) == 1 and chunk_frames is None
    held = _device(usable[0], features, pwd) if whole else None      # a single in-memory trajectory is uploaded once
    load = lambda piece: held if whole else _device(piece, features, pwd)

    sum0 = sumt = None
    for traj in usable:                                             # the means pass
        for piece in _pieces(traj, lagtime, chunk_frames):
            X = load(piece)
            a, b = pairs.lagged_means(X, lagtime, pwd)
            w = float(X.shape[0] - lagtime)
            sum0, sumt = (a * w, b * w) if sum0 is None else (sum0 + a * w, sumt + b * w)
    mean0, meant = (a, b) if whole else (sum0 / float(m), sumt / float(m))
    if center is None:
        c = (mean0 + meant) / 2.0
    else:
        c = torch.as_tensor(np.asarray(center, np.float64) if not torch.is_tensor(center) else center).to(device="cuda", dtype=torch.float64).contiguous()
        if tuple(c.shape) != tuple(mean0.shape) or not bool(torch.isfinite(c).all()):
            raise ValueError(f"center should be {tuple(mean0.shape)} finite values, got {tuple(c.shape)}")

    total = None
    for traj in usable:                                             # the moments pass
        for piece in _pieces(traj, lagtime, chunk_frames):
            part = pairs.lagged_moments(load(piece), lagtime, c, pwd)
            total = part if total is None else {k: total[k] + part[k] for k in total}
    return LaggedMoments(m, lagtime, mean0, meant, c, **total)


# ---- models ---------------------------------------------------------------------------------------------------------------------
def _whiten(c: torch.Tensor, epsilon: float):
    s, u = torch.linalg.eigh(c)
    keep = s > epsilon                                              # rank truncation, as metrics.tica_fit
    return u[:, keep] / torch.sqrt(s[keep]), int(keep.sum())


@dataclass
class TICAModel:
    """[DEEPTIME-RECALL], PARITY UNPINNED: deeptime's TICA / VAMP estimators restated (deeptime is neither in the reference tree nor
    installable here), the reversible form exactly as esmdiff_amd.metrics.tica_fit and oracle/metrics_ref.tica_fit restate it:
    symmetrised covariances about one mean, rank cut of c00 at epsilon, whitening, symmetric eigenproblem, eigenvalues ordered by
    |lambda|, kinetic-map scaling (components = whitened eigenvectors times their eigenvalues).  reversible=False: the Koopman /
    VAMP form, `eigenvalues` the singular values of c00^-1/2 c0t ctt^-1/2.  Sign: the entry of largest magnitude of every component
    is positive.  eigenvalues, timescales and components hold the `dim` leading ones; all_eigenvalues every kept one."""
    lagtime: int
    dim: int
    reversible: bool
    scaling: Optional[str]
    pwd_offset: int                 # 0: the model was fitted on a feature matrix
    m: int
    n_kept: int
    mean: torch.Tensor              # (D,)
    components: torch.Tensor        # (D, dim)
    eigenvalues: np.ndarray         # (dim,)
    all_eigenvalues: np.ndarray     # (n_kept,) (reversible) or (min of both ranks,)
    timescales: np.ndarray          # (dim,)
    cumulative_kinetic_variance: np.ndarray     # (len(all_eigenvalues),)

    def transform(self, coords) -> np.ndarray:
        """(n, L, 3) coordinates (or (n, D) features for a model fitted on features) -> the (n, dim) projection, through
        esmdiff_lagged_project: fused from the coordinates, a frame's row independent of the batch."""
        return self.transform_device(_device(_trajectories(coords, self.pwd_offset == 0)[0], self.pwd_offset == 0, self.pwd_offset)).cpu().numpy()

    def transform_device(self, X: torch.Tensor) -> torch.Tensor:
        return pairs.lagged_project(X, self.mean, self.components, self.pwd_offset)

    def vamp2(self, dim: Optional[int] = None) -> float:
        """1 + the sum of the squares of the `dim` leading eigenvalues (singular values); the 1 is the constant function's."""
        lam = self.all_eigenvalues if dim is None else self.all_eigenvalues[:dim]
        return float(1.0 + np.sum(lam ** 2))


def fit(moments: LaggedMoments, dim: int = 2, epsilon: float = 1e-6, reversible: bool = True, scaling: Optional[str] = "kinetic_map",
        pwd_offset: int = 1) -> TICAModel:
    """LaggedMoments -> TICAModel (the dense tail: one eigh of c00 and one of the whitened c0t, or two eigh and one SVD)."""
    if scaling not in ("kinetic_map", None):
        raise ValueError(f"scaling is 'kinetic_map' or None, got {scaling!r}")
    if not 1 <= int(dim) <= N.LAGGED_MAX_DIM:
        raise ValueError(f"dim must be 1 to {N.LAGGED_MAX_DIM}, got {dim}")
    dim = int(dim)
    if reversible:
        c00, c0t = moments.covariances(True)
        wh, kept = _whiten(c00, epsilon)
        if kept < dim:
            raise ValueError("reference ensemble has fewer than `dim` directions above the TICA rank cut-off")
        lam, v = torch.linalg.eigh(wh.T @ c0t @ wh)
        order = torch.argsort(lam.abs(), descending=True)
        lam_all, vecs = lam[order], wh @ v[:, order[:dim]]
    else:
        c00, c0t, ctt = moments.covariances(False)
        wh, kept0 = _whiten(c00, epsilon)
        wt, keptt = _whiten(ctt, epsilon)
        kept = min(kept0, keptt)
        if kept < dim:
            raise ValueError("reference ensemble has fewer than `dim` directions above the rank cut-off")
        u, sv, _ = torch.linalg.svd(wh.T @ c0t @ wt, full_matrices=False)
        lam_all, vecs = sv, wh @ u[:, :dim]
    if scaling == "kinetic_map":
        vecs = vecs * lam_all[:dim]
    top = vecs.abs().argmax(0)
    vecs = (vecs * torch.sign(vecs[top, torch.arange(dim, device=vecs.device)])).contiguous()
    lam_np = lam_all.cpu().numpy()
    sq = lam_np ** 2
    return TICAModel(moments.lagtime, dim, bool(reversible), scaling, int(pwd_offset), moments.m, kept, moments.mean(reversible).contiguous(),
                     vecs, lam_np[:dim].copy(), lam_np, timescales_from_eigenvalues(lam_np[:dim], moments.lagtime), np.cumsum(sq) / sq.sum())


def tica(x, lagtime: int, dim: int = 2, epsilon: float = 1e-6, reversible: bool = True, scaling: Optional[str] = "kinetic_map",
         pwd_offset: int = 1, features: bool = False, chunk_frames: Optional[int] = None) -> TICAModel:
    """Fit on x (everything lagged_moments takes) -> TICAModel."""
    mom = lagged_moments(x, lagtime, None, pwd_offset, features, chunk_frames)
    return fit(mom, dim, epsilon, reversible, scaling, 0 if features else int(pwd_offset))


def implied_timescales(x, lagtimes, k: int = 3, epsilon: float = 1e-6, pwd_offset: int = 1, features: bool = False,
                       chunk_frames: Optional[int] = None) -> np.ndarray:
    """-> (len(lagtimes), k): the k leading implied timescales -lag / ln lambda of the reversible fit at every lag time, NaN where
    |lambda| >= 1 or lambda <= 0 or fewer than k directions are kept."""
    out = np.full((len(lagtimes), int(k)), np.nan)
    for r, lag in enumerate(lagtimes):
        model = fit(lagged_moments(x, lag, None, pwd_offset, features, chunk_frames), 1, epsilon, True, None, 0 if features else int(pwd_offset))
        ts = timescales_from_eigenvalues(model.all_eigenvalues[:k], model.lagtime)
        out[r, :len(ts)] = ts
    return out


def vamp2(x, lagtime: int, dim: Optional[int] = None, epsilon: float = 1e-6, pwd_offset: int = 1, features: bool = False,
          chunk_frames: Optional[int] = None) -> float:
    """The VAMP-2 score of the features at a lag time: 1 + the squared singular values of c00^-1/2 c0t ctt^-1/2 (the `dim` leading
    ones, or all)."""
    mom = lagged_moments(x, lagtime, None, pwd_offset, features, chunk_frames)
    return fit(mom, 1, epsilon, False, None, 0 if features else int(pwd_offset)).vamp2(dim)


def js_tica(ca_coords_dict, ref_key: str = "target", n_bins: int = 50, lagtime: int = 20, return_tic: bool = True,
            weights: Optional[dict] = None, rounded: bool = True, dim: int = 2):
    """eval_utils.py:258-289 with esmdiff_amd.metrics.js_tica's call shape and its esmdiff_metrics_js_columns tail; the fit on the
    reference ensemble and every projection go through the fused entries: no (n, D) distance matrix."""
    from . import metrics as M
    L_ = N.lib()
    dev = {k: _device(v, False, 1) for k, v in ca_coords_dict.items()}
    model = fit(lagged_moments(dev[ref_key], lagtime), dim)
    dr = {k: model.transform_device(v) for k, v in dev.items()}
    ref = dr[ref_key]
    wr = M._wdev(weights, ref_key, ref.shape[0])
    res = {k: M._call(L_.esmdiff_metrics_js_columns, M._p(v), v.shape[0], M._p(M._wdev(weights, k, v.shape[0])), M._p(ref), ref.shape[0],
                      M._p(wr), dim, n_bins, 0) for k, v in dr.items() if k != ref_key}
    res[ref_key] = 0.0
    res = M._round(res, rounded)
    if return_tic:
        return res, {k: v.cpu().numpy() for k, v in dr.items()}
    return res


# ---- the command line's block ---------------------------------------------------------------------------------------------------
def report(trajectory, samples, targets, lagtime: int = 20, dim: int = 2, lagtimes=None, n_bins: int = 50,
           chunk_frames: Optional[int] = None) -> dict:
    """The "tica" block of analyze_ensemble: trajectory (n, L, 3) (an array, a memmap or a PDB path), samples (n_s, L, 3) and targets
    (K, L, 3)."""
    model = tica(trajectory, lagtime, dim, chunk_frames=chunk_frames)
    traj = _trajectories(trajectory, False)[0]
    spans = [(0, traj.shape[0])] if chunk_frames is None else [(s, min(s + chunk_frames, traj.shape[0])) for s in range(0, traj.shape[0], chunk_frames)]
    proj_traj = np.concatenate([model.transform(np.asarray(traj[s:e])) for s, e in spans], axis=0)
    proj_samples, proj_targets = model.transform(samples), model.transform(targets)
    js = _js_per_tic(proj_samples, proj_traj, n_bins)
    out = {"lagtime": int(lagtime), "dim": int(dim), "pwd_offset": 1, "epsilon": 1e-6, "frames": int(traj.shape[0]), "pairs": int(model.m),
           "n_kept": int(model.n_kept), "eigenvalues": model.eigenvalues, "timescales": model.timescales,
           "cumulative_kinetic_variance": model.cumulative_kinetic_variance[:dim],
           "vamp2": vamp2(trajectory, lagtime, dim, chunk_frames=chunk_frames),
           "js_tic": js, "js_tica": float(np.mean(js)), "samples_tic": proj_samples, "targets_tic": proj_targets}
    if lagtimes:
        out["implied_timescales"] = {"lagtimes": [int(l) for l in lagtimes], "timescales": implied_timescales(trajectory, lagtimes, chunk_frames=chunk_frames)}
    edges, F = free_energy(proj_traj[:, :2], bins=n_bins)
    out["free_energy"] = {"edges": edges, "F": np.where(np.isinf(F), np.nan, F), "kT": 1.0}
    return out


def _js_per_tic(proj, proj_ref, n_bins: int) -> np.ndarray:
    """Per TIC, the Jensen-Shannon distance of the samples' projection against the trajectory's (metrics.js_columns, unrounded)."""
    from . import metrics as M
    return np.array([M.js_columns({"s": proj[:, k], "target": proj_ref[:, k]}, "target", n_bins, rounded=False)["s"] for k in range(proj.shape[1])])

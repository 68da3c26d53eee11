"""Nearest neighbours between two ensembles in structure space, on the device: for every frame of one ensemble the closest frame of the
other under the least-squares (Kabsch) RMSD, with counts within cutoffs, sums and a histogram, and with no (n, m) matrix.

The reference asks "how close does the MD come to each sample" of five BPTI clusters (analysis/bpti_analysis.py:151-159: rmsd.min(dim=0)
and argmin over the samples).  Here both directions are one call for whole trajectories: coverage (recall: the share of MD frames with a
sample within a cutoff; precision: the share of samples within a cutoff of some MD frame), the nearest pairs, and the mean pairwise RMSD
of an ensemble with itself.  A minimum over RMSDs needs neither the rotation nor the matrix: with both sides centred on ONE residue set
of N residues, msd(i, j) = max(0, (G_a[i] + G_b[j] - 2 (s1 + s2 + sigma s3)) / N), G = sum |x - c|^2 and s the singular values of the
3 x 3 H_ij = sum_l a_il b_jl^T; all the H_ij together are nine GEMMs on the f64 MFMA (csrc/rmsd_nn.hip), and the singular values, minima,
counts and sums stay in registers and LDS.  sigma = sign(det H_ij) for proper rotations, +1 when reflections are allowed
(geo_utils._find_rigid_alignment, reflection=True).

ONE residue set: the GEMM form needs the same residues in every frame, so per-frame masks are NOT supported here.  A frame with a
non-finite coordinate on the set is left out (used_a / used_b say which).  For ensembles whose frames resolve different residues use
ensemble.pairwise_rmsd, which aligns every pair on the residues the two share.

Memory: the centred, compacted copy P of each side ((n, 3, K) float64, K the selected count rounded up to a multiple of 4) stays on the
device and is the only O(n L) allocation; chunk_frames bounds the upload of the coordinates themselves (a host numpy.memmap is read that
many frames at a time).  A frame's row of P depends on that frame alone, so the result has the same bits for every chunk_frames; ties
go to the lowest index.  numpy and torch only.  There is no CPU fallback."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from . import _native as N
from . import kinetics, pairs

PSEUDO_C = 1e-6                  # the pseudo count of metrics.js_pwd


@dataclass
class Neighbours:
    """Host arrays.  *_a: per frame of a (n,), *_b: per frame of b (m,), None for an ensemble against itself.  rmsd / index: the nearest
    frame of the other side and its RMSD (NaN and -1 for an unused frame, or when the other side has no used frame); count (·, T): the
    frames of the other side within each cutoff; sum / pairs: the sum of the RMSDs to every used frame of the other side and their
    number; used: the frame is finite on the residue set; hist / edges: the histogram of every pair's RMSD (an ensemble against itself:
    every unordered pair once; the last bin also holds everything beyond edges[-1]), None without hist_bins; n_pairs: the pairs
    compared; select: the residue set."""
    rmsd_a: np.ndarray
    index_a: np.ndarray
    rmsd_b: Optional[np.ndarray]
    index_b: Optional[np.ndarray]
    count_a: np.ndarray
    count_b: Optional[np.ndarray]
    sum_a: np.ndarray
    sum_b: Optional[np.ndarray]
    pairs_a: np.ndarray
    pairs_b: Optional[np.ndarray]
    used_a: np.ndarray
    used_b: Optional[np.ndarray]
    hist: Optional[np.ndarray]
    edges: Optional[np.ndarray]
    n_pairs: int
    select: np.ndarray
    cutoffs: tuple


def _host(x):
    return np.asarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x)


def _first_frame(trajs) -> np.ndarray:
    return np.asarray(_host(trajs[0][0:1]), np.float64)[0]


def _prepared(trajs, sel_dev, n_sel, L, chunk_frames) -> dict:
    """Every piece of every trajectory through esmdiff_rmsd_prepare -> one prepared side (P, info, use over all frames in order)."""
    parts = []
    for traj in trajs:
        if traj.ndim != 3 or tuple(traj.shape[1:]) != (L, 3) or traj.shape[0] == 0:
            raise ValueError(f"a trajectory should be (n, {L}, 3) CA coordinates with n >= 1, got {tuple(traj.shape)}")
        for piece in kinetics._pieces(traj, 0, chunk_frames):
            if not torch.is_tensor(piece):
                piece = np.asarray(piece)
                piece = torch.as_tensor(piece if piece.flags.writeable else piece.copy())
            parts.append(pairs.rmsd_prepare(piece.to(device="cuda", dtype=torch.float64).contiguous(), sel_dev, n_sel))
    if len(parts) == 1:
        return parts[0]
    return {"P": torch.cat([p["P"] for p in parts]), "info": torch.cat([p["info"] for p in parts]), "use": torch.cat([p["use"] for p in parts]),
            "n_sel": n_sel}


def nearest(a, b=None, select=None, reflection: bool = False, cutoffs: Sequence[float] = (), hist_bins: int = 0,
            hist_max: Optional[float] = None, chunk_frames: Optional[int] = None) -> Neighbours:
    """a, b: (n, L, 3) CA coordinates (an array, a tensor, a PDB path, a list of trajectories, or a host numpy.memmap read chunk_frames
    frames at a time); b None: a against itself over pairs i != j.  select: bool (L,), the ONE residue set; default: the residues whose
    coordinates are finite in the first frame of a and in the first frame of b.  A frame with a non-finite coordinate on the set is left
    out.  cutoffs: up to N.RMSD_NN_MAX_CUTOFFS RMSD cutoffs (count_a, count_b).  hist_bins bins of width hist_max / hist_bins."""
    ta = kinetics._trajectories(a, False)
    tb = None if b is None else kinetics._trajectories(b, False)
    first = _first_frame(ta)
    if first.ndim != 2 or first.shape[1] != 3:
        raise ValueError(f"a should be (n, L, 3) CA coordinates, got frames of {first.shape}")
    L = first.shape[0]
    if select is None:
        sel = np.isfinite(first).all(-1)
        if tb is not None:
            fb = _first_frame(tb)
            if fb.shape != first.shape:
                raise ValueError(f"structures of different lengths: {first.shape[0]} and {fb.shape[0]} (the correspondence is residue to residue)")
            sel &= np.isfinite(fb).all(-1)
    else:
        sel = _host(select).astype(bool).reshape(-1)
        if sel.shape != (L,):
            raise ValueError(f"select should be ({L},), got {sel.shape}")
    n_sel = int(sel.sum())
    if n_sel < 2:
        raise ValueError(f"the residue set has {n_sel} residues (at least 2)")
    if len(cutoffs) > N.RMSD_NN_MAX_CUTOFFS:
        raise ValueError(f"{len(cutoffs)} cutoffs (at most {N.RMSD_NN_MAX_CUTOFFS})")
    if hist_bins and not (hist_max is not None and hist_max > 0 and 0 < hist_bins <= N.RMSD_NN_MAX_BINS):
        raise ValueError(f"a histogram needs hist_max > 0 and 1 to {N.RMSD_NN_MAX_BINS} bins, got hist_bins = {hist_bins}, hist_max = {hist_max}")
    pairs.need_device("esmdiff_amd.neighbours")
    sel_dev = None if sel.all() else torch.as_tensor(sel.astype(np.uint8), device="cuda")
    pa = _prepared(ta, sel_dev, n_sel, L, chunk_frames)
    pb = None if tb is None else _prepared(tb, sel_dev, n_sel, L, chunk_frames)
    if pa["P"].shape[0] >= 2 ** 31 or (pb is not None and pb["P"].shape[0] >= 2 ** 31):
        raise ValueError("more than 2^31 - 1 frames on a side")
    width = float(hist_max) / hist_bins if hist_bins else 1.0
    res = pairs.rmsd_nearest(pa, pb, reflection, cutoffs, int(hist_bins), width)
    h = lambda k: res[k].cpu().numpy() if k in res else None
    used_a = pa["use"].cpu().numpy().astype(bool)
    used_b = None if pb is None else pb["use"].cpu().numpy().astype(bool)
    ua = int(used_a.sum())
    ub = ua if used_b is None else int(used_b.sum())
    n_pairs = ua * (ua - 1) // 2 if pb is None else ua * ub
    return Neighbours(h("row_rmsd"), h("row_index"), h("col_rmsd"), h("col_index"), h("row_count"), h("col_count"), h("row_sum"), h("col_sum"),
                      h("row_pairs"), h("col_pairs"), used_a, used_b, h("hist"),
                      np.linspace(0.0, float(hist_max), hist_bins + 1) if hist_bins else None, n_pairs, sel, tuple(float(c) for c in cutoffs))


def _share(hit: np.ndarray, used: np.ndarray, weights) -> float:
    w = np.ones(len(used)) if weights is None else np.asarray(weights, np.float64)
    total = w[used].sum()
    return float((w * hit)[used].sum() / total) if total > 0 else float("nan")


def coverage_from(nb: Neighbours, weights=None) -> dict:
    """The host half of `coverage`: a Neighbours of (samples = a, trajectory = b) with cutoffs -> the coverage block."""
    if weights is not None and np.asarray(weights).shape != nb.used_b.shape:
        raise ValueError(f"weights should be one per trajectory frame {nb.used_b.shape}, got {np.asarray(weights).shape}")
    T = len(nb.cutoffs)
    out = {"cutoffs": list(nb.cutoffs),
           "recall": [_share(nb.count_b[:, t] > 0, nb.used_b, weights) for t in range(T)],
           "precision": [_share(nb.count_a[:, t] > 0, nb.used_a, None) for t in range(T)],
           "mat_r": _share(np.where(nb.used_b & (nb.pairs_b > 0), nb.rmsd_b, 0.0), nb.used_b & (nb.pairs_b > 0), weights),
           "mat_p": _share(np.where(nb.used_a & (nb.pairs_a > 0), nb.rmsd_a, 0.0), nb.used_a & (nb.pairs_a > 0), None),
           "nearest_frame": nb.index_a, "nearest_frame_rmsd": nb.rmsd_a, "nearest_sample": nb.index_b, "nearest_sample_rmsd": nb.rmsd_b,
           "samples_used": int(nb.used_a.sum()), "samples_dropped": int((~nb.used_a).sum()),
           "frames_used": int(nb.used_b.sum()), "frames_dropped": int((~nb.used_b).sum())}
    if T:
        order = int(np.argmax(nb.cutoffs))
        out["novel"] = np.flatnonzero(nb.used_a & (nb.count_a[:, order] == 0))
        out["unrecalled"] = [np.flatnonzero(nb.used_b & (nb.count_b[:, t] == 0)) for t in range(T)]
        frames = max(int(nb.used_b.sum()), 1)
        out["density"] = np.where(nb.used_a[:, None], nb.count_a / float(frames), np.nan)
    return out


def coverage(samples, trajectory, cutoffs: Sequence[float] = (1.0, 2.0, 3.0), weights=None, select=None, reflection: bool = False,
             chunk_frames: Optional[int] = None) -> dict:
    """How well `samples` cover `trajectory` and the other way round.  Per cutoff: recall, the (weighted: `weights`, one per trajectory
    frame, e.g. MSM weights) share of used trajectory frames with a sample within the cutoff, and precision, the share of used samples
    with a frame within it.  mat_r / mat_p: the (weighted) mean nearest RMSD of the frames / of the samples.  nearest_frame (per sample)
    and nearest_sample (per frame) with their RMSDs; novel: the samples beyond the largest cutoff of every frame; unrecalled: per cutoff
    the frames no sample reaches; density (n, T): per sample the share of used frames within each cutoff (UNWEIGHTED: a weighted share
    would need the per-pair values, which are never kept)."""
    return coverage_from(nearest(samples, trajectory, select, reflection, cutoffs, chunk_frames=chunk_frames), weights)


def mean_pairwise_rmsd(x, select=None, reflection: bool = False, chunk_frames: Optional[int] = None) -> float:
    """The mean RMSD over the unordered pairs of an ensemble's used frames (the diversity number), holding no (n, n) array."""
    nb = nearest(x, None, select, reflection, chunk_frames=chunk_frames)
    total = int(nb.pairs_a.sum())
    return float(nb.sum_a.sum() / total) if total else float("nan")


def rmsd_distribution(x, bins: int = 50, r_max: float = 20.0, select=None, reflection: bool = False, chunk_frames: Optional[int] = None):
    """-> (hist i64 (bins,), edges (bins + 1,)) of the RMSD of every unordered pair of x's used frames; the last bin holds the overflow."""
    nb = nearest(x, None, select, reflection, hist_bins=bins, hist_max=r_max, chunk_frames=chunk_frames)
    return nb.hist, nb.edges


def _js(p: np.ndarray, q: np.ndarray) -> float:
    p, q = p / p.sum(), q / q.sum()
    mid = (p + q) / 2.0
    return float(np.sqrt(max(((p * np.log(p / mid)).sum() + (q * np.log(q / mid)).sum()) / 2.0, 0.0)))


def js_pairwise_rmsd(ensembles: dict, ref_key: str = "target", n_bins: int = 50, select=None, reflection: bool = False, rounded: bool = True) -> dict:
    """{name: ensemble} -> {name: the Jensen-Shannon distance between the distributions of its pairwise RMSD and of ensembles[ref_key]'s}
    in metrics.js_pwd's conventions (natural logarithm, square root, the pseudo count 1e-6 on every bin, 4 decimals, the reference
    against itself 0).  The bins span 0 to the reference's largest pairwise RMSD as a first pass of N.RMSD_NN_MAX_BINS bins finds it
    (the upper edge of the highest occupied bin); values beyond fall in the last bin.  An ensemble with fewer than 2 used frames: NaN."""
    first = nearest(ensembles[ref_key], None, select, reflection)
    if first.n_pairs < 1:
        return {k: (0.0 if k == ref_key else float("nan")) for k in ensembles}
    top = 2.0 * float(np.nanmax(first.sum_a / np.maximum(first.pairs_a, 1))) + 1.0     # twice the largest mean distance bounds every distance
    coarse, edges = rmsd_distribution(ensembles[ref_key], N.RMSD_NN_MAX_BINS, top, select, reflection)
    r_max = float(edges[int(np.flatnonzero(coarse)[-1]) + 1])
    href, _ = rmsd_distribution(ensembles[ref_key], n_bins, r_max, select, reflection)
    out = {}
    for k, v in ensembles.items():
        if k == ref_key:
            out[k] = 0.0
            continue
        h, _ = rmsd_distribution(v, n_bins, r_max, select, reflection)
        out[k] = _js(h + PSEUDO_C, href + PSEUDO_C) if h.sum() else float("nan")
    return {k: (round(v, 4) if rounded and v == v else v) for k, v in out.items()}


def best_per_state(samples, states, select=None, reflection: bool = False, chunk_frames: Optional[int] = None):
    """analysis/bpti_analysis.py:151-159 for any number of states: states (K, L, 3) -> (rmsd (K,), index (K,)): for each state the RMSD
    of the closest sample and which one (the reference's rmsd.min(dim=0) and argmin).  reflection=True is the reference's alignment
    (geo_utils._find_rigid_alignment has no determinant correction)."""
    nb = nearest(samples, states, select, reflection, chunk_frames=chunk_frames)
    return nb.rmsd_b, nb.index_b

"""A sampled ensemble against an MD ensemble in Cartesian space, on the device: the mean and the 3L x 3L covariance of the frames
superposed on one reference structure, and everything that is a function of those two.

The reference ships loaders for MD data sets (load_atlas_targets, load_atlas_processed, load_mdcath_processed in
slm/utils/eval_utils.py) with no metric behind them.  Conformation generators are usually scored against such data by four things: a
per-residue Gaussian Wasserstein distance (the root mean Wasserstein distance, RMWD, with its translation and variance parts), the W2
distance in the MD's and in the joint PCA space, the overlap of the leading modes, and the dynamic cross-correlation map.  All four are
functions of ONE object, AlignedMoments: the raw sums S = sum a a^T, r = sum a of a = (R x + t) - ref over the frames, each fitted
onto ref.  esmdiff_flex_transforms writes the fits as (n, 12) transforms and esmdiff_aligned_moments applies them inside its staging:
no aligned (n, L, 3) array exists, a fit costs O(L^2) memory whatever the number of frames, and every sum has a published order (two
runs agree bit for bit).  The dense eigenproblems stay torch.linalg calls, as in flexibility.pca and kinetics.fit.  numpy and torch
only.  There is no CPU fallback for the moments; the comparisons are plain float64 arithmetic on whatever device the moments live on.

[ALPHAFLOW-RECALL], PARITY UNPINNED: the Wasserstein metrics (rmwd, pca_w2, joint_pca_w2) follow the published formulas of Jing et
al. 2024 ("AlphaFold meets flow matching for generating protein ensembles") as DESIGN.md §3.29 writes them; no script of that project
is available here and none has been run."""
from __future__ import annotations

import os
from dataclasses import dataclass, field
from pathlib import Path
from typing import Optional

import numpy as np
import torch

from . import _native as N
from . import flexibility, kinetics, pairs


# ---- dense float64 arithmetic, on the host or the device ------------------------------------------------------------------------
def _t(x) -> torch.Tensor:
    return x.to(torch.float64) if torch.is_tensor(x) else torch.as_tensor(np.asarray(x, np.float64))


def _out(t: torch.Tensor):
    a = t.detach().cpu().numpy()
    return float(a) if a.ndim == 0 else a


def _bures(A: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    s, U = torch.linalg.eigh((A + A.transpose(-1, -2)) / 2.0)
    root = (U * torch.sqrt(s.clamp_min(0.0))[..., None, :]) @ U.transpose(-1, -2)
    M = root @ B @ root
    ev = torch.linalg.eigvalsh((M + M.transpose(-1, -2)) / 2.0).clamp_min(0.0)
    tr = lambda X: torch.diagonal(X, dim1=-2, dim2=-1).sum(-1)
    return (tr(A) + tr(B) - 2.0 * torch.sqrt(ev).sum(-1)).clamp_min(0.0)


def bures(A, B):
    """The squared Bures distance of two symmetric positive semi-definite matrices, tr A + tr B - 2 tr (A^1/2 B A^1/2)^1/2: the
    covariance part of the W2 distance of two Gaussians.  Two eigh: A's for the root, then the eigenvalues of A^1/2 B A^1/2, both clipped
    at 0 (a rank-deficient matrix is allowed), and the result clipped at 0.  (..., d, d) batches over the leading dimensions.  The error is
    ABSOLUTE (the three terms cancel when A is close to B): a few eps (tr A + tr B) times the condition number for full-rank arguments,
    and of the order sqrt(eps) (tr A + tr B) for a rank-deficient one, whose zero eigenvalue comes out as +- eps |A| |B| before the root."""
    return _out(_bures(_t(A), _t(B)))


def gaussian_w2_sq(mu1, cov1, mu2, cov2):
    """|mu1 - mu2|^2 + bures(cov1, cov2): the squared W2 distance of two Gaussians."""
    d = _t(mu1) - _t(mu2)
    return _out((d * d).sum(-1) + _bures(_t(cov1), _t(cov2)))


def projection_w2(y1, y2, p: int = 2) -> np.ndarray:
    """The exact 1-D Wasserstein-p distance of two samples per component: y1 (n1,) or (n1, k), y2 (n2,) or (n2, k) -> (k,), the p-th root
    of the integral over q in (0, 1) of |F1^-1(q) - F2^-1(q)|^p, the quantile functions those of the sorted samples (steps at i / n).
    The joint 2-D distance (an assignment problem) is out of scope: this is per component."""
    a, b = np.asarray(y1, np.float64), np.asarray(y2, np.float64)
    a, b = (a[:, None] if a.ndim == 1 else a), (b[:, None] if b.ndim == 1 else b)
    if a.ndim != 2 or b.ndim != 2 or a.shape[1] != b.shape[1] or not len(a) or not len(b) or not (np.isfinite(a).all() and np.isfinite(b).all()):
        raise ValueError(f"projection_w2 takes finite (n1, k) and (n2, k) projections, got {a.shape} and {b.shape}")
    a, b = np.sort(a, axis=0), np.sort(b, axis=0)
    n1, n2 = len(a), len(b)
    cuts = np.unique(np.concatenate([np.arange(n1 + 1) * n2, np.arange(n2 + 1) * n1]))      # the steps of both, in units of 1 / (n1 n2)
    width = np.diff(cuts) / float(n1 * n2)
    i, j = cuts[:-1] // n2, cuts[:-1] // n1
    return ((np.abs(a[i] - b[j]) ** p * width[:, None]).sum(0)) ** (1.0 / p)


# ---- the moments ------------------------------------------------------------------------------------------------------------------
@dataclass
class AlignedMoments:
    """The raw moments of an ensemble's frames fitted onto `ref` (tensors on the device where the device made them, float64): with
    a = (R x + t) - ref on the residues `residues` (those valid in ref), S = sum a a^T (3L', 3L') and r = sum a (3L',) over the `count`
    frames that entered; n_dropped frames did not (a failed fit, or a residue of the set unresolved)."""
    count: int
    n_dropped: int
    ref: torch.Tensor               # (L', 3) the reference on the residue set: the centre of the sums
    residues: np.ndarray            # (L',) indices into the L residues of the input
    n_residues: int                 # L
    S: torch.Tensor
    r: torch.Tensor
    rmsd: np.ndarray                # (n,) of every frame to ref over the residues valid in both, NaN where the fit failed
    transforms: Optional[np.ndarray] = None     # (n, 12) with keep_transforms
    _modes: dict = field(default_factory=dict, repr=False)

    @property
    def mean(self) -> np.ndarray:
        """(L', 3): ref + r / count."""
        return _out(self._mean().reshape(-1, 3))

    def _mean(self) -> torch.Tensor:
        return self.ref.reshape(-1) + self.r / float(self.count)

    def _cov(self, ddof: int = 1) -> torch.Tensor:
        m = float(self.count)
        if self.count - ddof < 1:
            raise ValueError(f"a covariance with ddof = {ddof} needs more than {ddof} frames, got {self.count}")
        return (self.S - torch.outer(self.r, self.r) / m) / (m - ddof)

    def covariance(self, ddof: int = 1) -> np.ndarray:
        """(3L', 3L'): (S - r r^T / m) / (m - ddof), the residual-sum correction from the centre to the mean."""
        return _out(self._cov(ddof))

    def _blocks(self, ddof: int = 1) -> torch.Tensor:
        L = len(self.residues)
        return torch.diagonal(self._cov(ddof).reshape(L, 3, L, 3), dim1=0, dim2=2).permute(2, 0, 1).contiguous()

    def residue_covariance(self, ddof: int = 1) -> np.ndarray:
        """(L', 3, 3): the diagonal blocks."""
        return _out(self._blocks(ddof))

    def rmsf(self) -> np.ndarray:
        """(L',): sqrt of the mean squared distance from the mean position (divisor m, as flexibility.rmsf)."""
        return np.sqrt(np.clip(np.trace(self.residue_covariance(0), axis1=1, axis2=2), 0.0, None))

    def dccm(self) -> np.ndarray:
        """(L', L'): C_ij = tr Sigma_ij / sqrt(tr Sigma_ii tr Sigma_jj), the dynamic cross-correlation map."""
        L = len(self.residues)
        c = torch.diagonal(self._cov(0).reshape(L, 3, L, 3), dim1=1, dim2=3).sum(-1)
        d = torch.sqrt(torch.diagonal(c))
        return _out(c / torch.outer(d, d))

    def _eig(self, k: int):
        D = 3 * len(self.residues)
        if not 1 <= int(k) <= D:
            raise ValueError(f"k = {k} modes of a {D}-dimensional covariance")
        if "all" not in self._modes:
            lam, V = torch.linalg.eigh(self._cov(1))
            lam, V = lam.flip(0), V.flip(1).T.contiguous()
            big = V.gather(1, V.abs().argmax(1, keepdim=True))
            self._modes["all"] = (lam, V * torch.where(big < 0, -1.0, 1.0))
        lam, V = self._modes["all"]
        return lam[:k], V[:k]

    def modes(self, k: int):
        """-> eigenvalues (k,) of covariance(1), descending, and the unit modes (k, L', 3), the component of largest magnitude of each
        positive (flexibility.pca's convention).  One torch.linalg.eigh, kept."""
        lam, V = self._eig(k)
        return _out(lam), _out(V.reshape(int(k), -1, 3))

    def project(self, x, k: int = 2, mask=None, chunk_frames: Optional[int] = None) -> np.ndarray:
        """Other frames (m, L, 3), each fitted onto the same ref on its residues -> (m, k): their coordinates in the k leading modes about
        this ensemble's mean, through esmdiff_aligned_project.  A frame whose fit fails, or that lacks a residue of the set, gives NaN."""
        if not 1 <= int(k) <= N.ALIGNED_MAX_DIM:
            raise ValueError(f"k must be 1 to {N.ALIGNED_MAX_DIM}, got {k}")
        _, V = self._eig(k)
        keep = torch.as_tensor(self.residues, device="cuda")
        out = []
        for X, given in _device_pieces(kinetics._trajectories(x, False), mask, chunk_frames, self.n_residues):
            Xg, T, _, _, whole = _fit(X, given, keep, self.ref)
            Y = pairs.aligned_project(Xg, T, self._mean().contiguous(), V.T.contiguous())
            out.append(torch.where(whole[:, None], Y, torch.full_like(Y, float("nan"))).cpu().numpy())
        return np.concatenate(out)


def _reference(ref, first) -> np.ndarray:
    if ref is None:
        ref = first[0]
    elif isinstance(ref, (str, os.PathLike)):
        from .pdbio import load_coords
        ref = load_coords(Path(ref), max_n_model=1, verbose=False)[0]
    ref = np.asarray(ref.detach().cpu().numpy() if torch.is_tensor(ref) else ref, np.float64)
    if ref.ndim != 2 or ref.shape[1] != 3:
        raise ValueError(f"ref should be (L, 3) CA coordinates, got {ref.shape}")
    return ref


def _device_pieces(trajs, mask, chunk_frames, L):
    """Every piece of every trajectory -> (f64 (n, L, 3) on the device, bool (n, L) the residues given and resolved)."""
    total = sum(int(t.shape[0]) for t in trajs)
    if mask is not None:
        mask = np.asarray(mask.detach().cpu().numpy() if torch.is_tensor(mask) else mask).astype(bool)
        if mask.shape not in ((L,), (total, L)):
            raise ValueError(f"mask should be ({L},) or ({total}, {L}), got {mask.shape}")
    at = 0
    for traj in trajs:
        if traj.ndim != 3 or tuple(traj.shape[1:]) != (L, 3):
            raise ValueError(f"a trajectory should be (n, {L}, 3) CA coordinates, got {tuple(traj.shape)}")
        for piece in kinetics._pieces(traj, 0, chunk_frames):
            if not torch.is_tensor(piece):
                piece = np.asarray(piece)
                piece = torch.as_tensor(piece if piece.flags.writeable else piece.copy())
            pairs.need_device("esmdiff_amd.covariance")
            X = piece.to(device="cuda", dtype=torch.float64).contiguous()
            given = ~torch.isnan(X).any(-1)
            if mask is not None:
                given &= torch.as_tensor(mask if mask.ndim == 1 else mask[at:at + len(X)], device="cuda")
            at += len(X)
            yield X, given


def _fit(X, given, keep, ref):
    """The residue set gathered, then one esmdiff_flex_transforms call -> Xg (n, L', 3), T, rmsd, use u8 (n,): the fit succeeded and
    the frame is resolved on the whole set."""
    Xg, g = X[:, keep].contiguous(), given[:, keep]
    whole = g.all(1)
    T, rmsd, ok = pairs.flex_transforms(Xg, None if bool(whole.all()) else g.to(torch.uint8).contiguous(), ref, None)
    return Xg, T, rmsd, (ok.bool() & whole).to(torch.uint8).contiguous(), whole


def aligned_moments(x, ref=None, mask=None, chunk_frames: Optional[int] = None, keep_transforms: bool = False) -> AlignedMoments:
    """x: (n, L, 3) CA coordinates (an array, a tensor, a PDB path, or a host numpy.memmap read chunk_frames frames at a time), or a
    list of such trajectories -> AlignedMoments about `ref` ((L, 3) or a PDB path; None: frame 0).  mask: (L,) or (n, L) over all the
    frames in order, False where a residue is not to be used; a NaN coordinate makes a residue invalid.  The residue set is the residues
    valid in ref, gathered before the device calls; a frame enters when its fit succeeded and it is valid on the whole set.  The centre
    of the sums is ref: no mean pass, no cancellation worth the name after a superposition.  Pieces and list members are added in order."""
    trajs = kinetics._trajectories(x, False)
    if any(t.ndim != 3 or t.shape[0] == 0 for t in trajs):
        raise ValueError(f"a trajectory should be (n, L, 3) CA coordinates with n >= 1, got {[tuple(t.shape) for t in trajs]}")
    ref = _reference(ref, trajs[0])
    L = ref.shape[0]
    if any(tuple(t.shape[1:]) != (L, 3) for t in trajs):
        raise ValueError(f"trajectories of {[tuple(t.shape[1:]) for t in trajs]} per frame, the reference has ({L}, 3): the correspondence is residue to residue")
    if L > N.ALIGNED_MAX_L:
        raise ValueError(f"L = {L} residues are beyond the kernel's limit ({N.ALIGNED_MAX_L})")
    residues = np.flatnonzero(~np.isnan(ref).any(-1))
    if len(residues) < 2:
        raise ValueError(f"the reference has {len(residues)} resolved residues (at least 2)")
    pairs.need_device("esmdiff_amd.covariance")
    keep = torch.as_tensor(residues, device="cuda")
    refd = torch.as_tensor(np.ascontiguousarray(ref[residues]), device="cuda")
    center = refd.reshape(-1).contiguous()
    total, count, dropped, rmsds, transforms = None, 0, 0, [], []
    for X, given in _device_pieces(trajs, mask, chunk_frames, L):
        Xg, T, rmsd, use, _ = _fit(X, given, keep, refd)
        part = pairs.aligned_moments(Xg, T, use, center)
        m = int(part.pop("count")[0])
        count, dropped = count + m, dropped + len(X) - m
        total = part if total is None else {k: total[k] + part[k] for k in total}
        rmsds.append(rmsd.cpu().numpy())
        if keep_transforms:
            transforms.append(T.cpu().numpy())
    if count < 1:
        raise ValueError(f"no frame could be fitted onto the reference on its {len(residues)} residues ({dropped} dropped)")
    return AlignedMoments(count, dropped, refd, residues, L, total["S"], total["r"], np.concatenate(rmsds),
                          np.concatenate(transforms) if keep_transforms else None)


# ---- comparisons: functions of two AlignedMoments on the same reference -----------------------------------------------------------
def _same_ref(m1: AlignedMoments, m2: AlignedMoments):
    if m1.n_residues != m2.n_residues or not np.array_equal(m1.residues, m2.residues) or not torch.equal(m1.ref.cpu(), m2.ref.cpu()):
        raise ValueError("the two ensembles were not superposed on the same reference: their moments cannot be compared")


def pooled(m1: AlignedMoments, m2: AlignedMoments) -> AlignedMoments:
    """The moments of the two ensembles' frames taken together: the raw sums about the shared centre simply add."""
    _same_ref(m1, m2)
    return AlignedMoments(m1.count + m2.count, m1.n_dropped + m2.n_dropped, m1.ref, m1.residues, m1.n_residues, m1.S + m2.S.to(m1.S.device),
                          m1.r + m2.r.to(m1.r.device), np.concatenate([m1.rmsd, m2.rmsd]))


def residue_w2(m1: AlignedMoments, m2: AlignedMoments) -> dict:
    """Per residue, the squared W2 distance of the two Gaussians N(mu_i, Sigma_ii) -> {"w2_sq", "translation", "variance"}, (L',) each:
    W2^2 = |mu1 - mu2|^2 + bures(Sigma1, Sigma2)."""
    _same_ref(m1, m2)
    d = (m1._mean() - m2._mean().to(m1.r.device)).reshape(-1, 3)
    translation = (d * d).sum(-1)
    variance = _bures(m1._blocks(), m2._blocks().to(m1.S.device))
    return {"w2_sq": _out(translation + variance), "translation": _out(translation), "variance": _out(variance)}


def rmwd(m1: AlignedMoments, m2: AlignedMoments) -> dict:
    """The root mean over the residues of W2^2, and of its two parts -> {"rmwd", "translation", "variance"}; rmwd^2 is the sum of the
    other two squared."""
    w = residue_w2(m1, m2)
    return {"rmwd": float(np.sqrt(w["w2_sq"].mean())), "translation": float(np.sqrt(w["translation"].mean())),
            "variance": float(np.sqrt(w["variance"].mean()))}


def _subspace_w2(W: torch.Tensor, m1: AlignedMoments, m2: AlignedMoments) -> float:
    d = W @ (m1._mean() - m2._mean().to(W.device))
    return float(np.sqrt(_out((d * d).sum() + _bures(W @ m1._cov() @ W.T, W @ m2._cov().to(W.device) @ W.T))))


def pca_w2(m_ref: AlignedMoments, m: AlignedMoments, k: int = 2) -> float:
    """The Gaussian W2 distance of the two ensembles in m_ref's k leading modes, from the moments alone: W^T (mu1 - mu2) and W^T Sigma W."""
    _same_ref(m_ref, m)
    return _subspace_w2(m_ref._eig(k)[1], m_ref, m)


def pooled_covariance(m1: AlignedMoments, m2: AlignedMoments) -> torch.Tensor:
    """The covariance of the equal-weight mixture of the two ensembles: (Sigma1 + Sigma2) / 2 + d d^T / 4 with d = mu1 - mu2 and the
    population covariances (ddof 0).  With equal counts it is the covariance (ddof 0) of pooled(m1, m2)."""
    _same_ref(m1, m2)
    d = m1._mean() - m2._mean().to(m1.r.device)
    return (m1._cov(0) + m2._cov(0).to(m1.S.device)) / 2.0 + torch.outer(d, d) / 4.0


def joint_pca_w2(m1: AlignedMoments, m2: AlignedMoments, k: int = 2) -> float:
    """pca_w2 in the k leading modes of pooled_covariance(m1, m2): derived from the two moment sets, no second pass over the frames."""
    lam, V = torch.linalg.eigh(pooled_covariance(m1, m2))
    return _subspace_w2(V.flip(1)[:, :int(k)].T.contiguous(), m1, m2)


def ensemble_w2(m1: AlignedMoments, m2: AlignedMoments) -> float:
    """The Gaussian W2 distance in all 3L' dimensions."""
    _same_ref(m1, m2)
    d = m1._mean() - m2._mean().to(m1.r.device)
    return float(np.sqrt(_out((d * d).sum() + _bures(m1._cov(), m2._cov().to(m1.S.device)))))


def mode_cosines(m1: AlignedMoments, m2: AlignedMoments, k: int = 10) -> np.ndarray:
    """(k, k): |u_i . v_j| of the k leading modes of each."""
    _same_ref(m1, m2)
    return np.abs(_out(m1._eig(k)[1] @ m2._eig(k)[1].to(m1.S.device).T)).reshape(int(k), int(k))


def rmsip(m1: AlignedMoments, m2: AlignedMoments, k: int = 10) -> float:
    """The root mean square inner product of the k leading modes (Amadei et al. 1999): sqrt(sum_ij (u_i . v_j)^2 / k)."""
    c = mode_cosines(m1, m2, k)
    return float(np.sqrt((c * c).sum() / int(k)))


def dccm_correlation(m1: AlignedMoments, m2: AlignedMoments) -> float:
    """Pearson's r of the two cross-correlation maps over the residue pairs i < j."""
    _same_ref(m1, m2)
    i, j = np.triu_indices(len(m1.residues), 1)
    return flexibility.flexibility_correlation(m1.dccm()[i, j], m2.dccm()[i, j])["pearson"]


def compare(trajectory, samples, ref=None, k: int = 2, chunk_frames: Optional[int] = None, targets=None) -> dict:
    """An MD trajectory and a sampled ensemble, both superposed on `ref` (None: the trajectory's frame 0) -> every comparison above,
    the Pearson correlation of the two RMSF profiles, the counts, and the projections of the samples (and of `targets`) on the
    trajectory's k leading modes."""
    first = kinetics._trajectories(trajectory, False)[0]
    ref = _reference(ref, first)
    md = aligned_moments(trajectory, ref, chunk_frames=chunk_frames)
    sm = aligned_moments(samples, ref)
    D = 3 * len(md.residues)
    k = int(k)
    km = min(10, D, N.ALIGNED_MAX_DIM)
    per_residue = residue_w2(md, sm)
    out = {"n_residues": int(len(md.residues)), "residues": md.residues, "modes": k,
           "trajectory": {"count": md.count, "n_dropped": md.n_dropped}, "samples": {"count": sm.count, "n_dropped": sm.n_dropped},
           "residue_w2": {n.replace("w2_sq", "w2"): np.sqrt(v) for n, v in per_residue.items()}, **rmwd(md, sm),
           "pca_w2": pca_w2(md, sm, k), "joint_pca_w2": joint_pca_w2(md, sm, k), "ensemble_w2": ensemble_w2(md, sm),
           "rmsip": rmsip(md, sm, km), "rmsip_modes": km, "mode_cosines": mode_cosines(md, sm, min(k, km)),
           "dccm_correlation": dccm_correlation(md, sm),
           "rmsf_correlation": flexibility.flexibility_correlation(md.rmsf(), sm.rmsf())["pearson"],
           "rmsf": {"trajectory": md.rmsf(), "samples": sm.rmsf()},
           "explained_variance": md.modes(k)[0], "samples_projection": md.project(samples, k)}
    finite = lambda y: y[np.isfinite(y).all(1)]
    own, theirs = finite(md.project(trajectory, k, chunk_frames=chunk_frames)), finite(out["samples_projection"])
    out["projection_w2"] = projection_w2(own, theirs) if len(own) and len(theirs) else np.full(k, np.nan)
    if targets is not None:
        out["targets_projection"] = md.project(targets, k)
    return out

"""Metastable states of a trajectory on the device: k-means on the slow coordinates, lagged transition counts, a Markov state model
(MSM) with its stationary distribution and timescales, metastable sets, and the comparison of a sampled ensemble's state populations
with the model's.

esmdiff_amd.kinetics ends at continuous coordinates.  The standard next steps are k-means on them, the lagged transition counts of the
labels and the MSM on the counts.  The three entries of csrc/msm.hip do the parts that touch every frame: the nearest centre, one
Lloyd step in a single pass (labels, cluster sizes, cluster sums, inertia) and the count matrix.  Nothing of size (n, k) exists, the
integer outputs equal a numpy restatement exactly, and every float sum has a published order, so two runs agree bit for bit
(tests/states_ref.py).  What is left is O(k^2) and O(k^3) arithmetic on the host in numpy: the connected set, the reversible
estimator, the eigenvalues and the inner-simplex step of PCCA+.  There is no CPU fallback for the parts on the device, and neither
scipy nor scikit-learn is needed."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _native as N
from . import kinetics, pairs

PSEUDO_C = 1e-6      # the pseudo count metrics.js_pwd adds to every histogram cell


# ---- input ----------------------------------------------------------------------------------------------------------------------
def _frames(y) -> torch.Tensor:
    """(n, d) or (n,) coordinates, an array or a tensor, or a list of such trajectories (taken together: k-means knows no time) -> f64
    (n, d) on the device, finite, 1 <= d <= 16."""
    if isinstance(y, (list, tuple)):
        if not y:
            raise ValueError("an empty list of trajectories")
        parts = [_frames(t) for t in y]
        if len({p.shape[1] for p in parts}) != 1:
            raise ValueError(f"trajectories of different dimensions: {[tuple(p.shape) for p in parts]}")
        return torch.cat(parts, 0).contiguous()
    t = y if torch.is_tensor(y) else torch.as_tensor(np.ascontiguousarray(np.asarray(y)))
    t = t[:, None] if t.dim() == 1 else t
    if t.dim() != 2 or not 1 <= t.shape[1] <= N.LAGGED_MAX_DIM:
        raise ValueError(f"coordinates should be (n, d) with 1 <= d <= {N.LAGGED_MAX_DIM}, got {tuple(t.shape)}")
    pairs.need_device("esmdiff_amd.states")
    t = t.to(device="cuda", dtype=torch.float64).contiguous()
    if not bool(torch.isfinite(t).all()):
        raise ValueError("coordinates should not contain nan or inf")
    return t


def _labels_host(labels) -> np.ndarray:
    a = labels.detach().cpu().numpy() if torch.is_tensor(labels) else np.asarray(labels)
    if a.ndim != 1 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"labels should be a vector of integers, got {a.dtype} {a.shape}")
    return a


def _label_list(labels) -> list:
    """One label vector or a list of them -> a list."""
    if isinstance(labels, (list, tuple)) and len(labels) and not np.isscalar(labels[0]):
        return list(labels)
    return [labels]


# ---- k-means --------------------------------------------------------------------------------------------------------------------
@dataclass
class KMeansModel:
    """centres (k, d), and for the frames the model was fitted on: labels (n,) int32, counts (k,) int64, inertia (the sum of the squared
    distances to the assigned centres), all of the FINAL centres; n_iter centre updates; converged."""
    centres: np.ndarray
    labels: np.ndarray
    counts: np.ndarray
    inertia: float
    n_iter: int
    converged: bool

    def assign_device(self, Y: torch.Tensor) -> torch.Tensor:
        centres = torch.as_tensor(self.centres, device="cuda")
        return pairs.kmeans_assign(Y, centres, dist2=False)[0]

    def assign(self, y) -> np.ndarray:
        """(n, d) coordinates -> labels (n,) int32 through esmdiff_kmeans_assign: the smallest index of a nearest centre."""
        return self.assign_device(_frames(y)).cpu().numpy()


def _init_centres(Y: torch.Tensor, k: int, init, seed: int) -> torch.Tensor:
    n, d = Y.shape
    if not isinstance(init, str):
        c = np.asarray(init.detach().cpu().numpy() if torch.is_tensor(init) else init, np.float64)
        if c.shape != (k, d) or not np.isfinite(c).all():
            raise ValueError(f"init should be ({k}, {d}) finite centres, got {c.shape}")
        return torch.as_tensor(np.ascontiguousarray(c), device="cuda")
    if init == "uniform":                                               # frames at a uniform time stride
        return Y[torch.as_tensor((np.arange(k) * n) // k, device="cuda")].contiguous()
    if init != "kmeans++":
        raise ValueError(f"init is an array (k, d), 'uniform' or 'kmeans++', got {init!r}")
    rng = np.random.default_rng(seed)
    centres = torch.empty((k, d), dtype=torch.float64, device="cuda")
    centres[0] = Y[int(rng.integers(n))]
    nearest = pairs.kmeans_assign(Y, centres[0:1].contiguous())[1]     # the running minimum of dist2 stays on the device
    for j in range(1, k):
        cum = torch.cumsum(nearest, 0)
        total = float(cum[-1])
        if total > 0.0:                                                 # D^2 sampling: a frame with probability dist2 / sum
            at = int(torch.searchsorted(cum, torch.as_tensor([rng.random() * total], dtype=torch.float64, device="cuda"), right=True)[0])
            at = min(at, n - 1)
        else:                                                           # every frame is a centre already
            at = int(rng.integers(n))
        centres[j] = Y[at]
        nearest = torch.minimum(nearest, pairs.kmeans_assign(Y, centres[j:j + 1].contiguous())[1])
    return centres


def kmeans(y, k: int, n_iter: int = 100, tol: float = 1e-8, init="kmeans++", seed: int = 0) -> KMeansModel:
    """Lloyd's algorithm on y ((n, d), d <= 16; an array, a device tensor or a list of trajectories) with k <= 4096 centres, one
    esmdiff_kmeans_step per iteration.  init: an array (k, d); "uniform": the frames (j n) // k; "kmeans++": D^2 sampling with
    numpy.random.default_rng(seed) on the host over the device's running minimum of dist2.  A centre is sums / counts, the division
    done once; an EMPTY cluster keeps its previous centre (a stated convention).  The iteration has converged when a step gives the
    labels of the step before, or when the largest change of a centre's component is <= tol; labels, counts and inertia are those of
    the final centres."""
    Y = _frames(y)
    n, d = Y.shape
    if int(k) != k or not 1 <= int(k) <= N.KMEANS_MAX_K:
        raise ValueError(f"k must be an integer from 1 to {N.KMEANS_MAX_K}, got {k}")
    k = int(k)
    if n < k:
        raise ValueError(f"{n} frames cannot seed {k} centres")
    centres = _init_centres(Y, k, init, seed)
    previous, converged, done, res = None, False, 0, None
    while done < int(n_iter):
        res = pairs.kmeans_step(Y, centres)
        if previous is not None and torch.equal(res["labels"], previous):
            converged = True                                            # the centres are the means of these labels already
            break
        counts = res["counts"][:, None]
        new = torch.where(counts > 0, res["sums"] / counts.to(torch.float64), centres)
        shift = float((new - centres).abs().max())
        centres, previous, done, res = new.contiguous(), res["labels"], done + 1, None
        if shift <= tol:
            converged = True
            break
    if res is None:
        res = pairs.kmeans_step(Y, centres)
    return KMeansModel(centres.cpu().numpy(), res["labels"].cpu().numpy(), res["counts"].cpu().numpy(), float(res["inertia"][0]), done, converged)


def discretize(tica_model, coords, kmeans_model: KMeansModel) -> np.ndarray:
    """Coordinates (n, L, 3) (or features for a model fitted on features) -> labels (n,): the projection of
    tica_model.transform_device, then the nearest centre; nothing leaves the device in between."""
    features = tica_model.pwd_offset == 0
    X = kinetics._device(kinetics._trajectories(coords, features)[0], features, tica_model.pwd_offset)
    return kmeans_model.assign_device(tica_model.transform_device(X)).cpu().numpy()


# ---- counts ---------------------------------------------------------------------------------------------------------------------
def transition_counts(labels, lagtime: int, k: Optional[int] = None) -> np.ndarray:
    """labels: one trajectory's (n,) integers (an array or a device tensor) or a list of them -> counts (k, k) int64: the pairs
    (labels[t], labels[t + lagtime]) with both >= 0, sliding window.  Pairs never cross a boundary of the list; integer sums are
    exact, so the trajectories' counts are added on the host.  k: the number of states (default: the largest label + 1)."""
    lagtime = kinetics._check_lag(lagtime)
    trajs = _label_list(labels)
    if k is None:
        k = max([int(_labels_host(t).max()) + 1 for t in trajs if len(t)] + [1])
    if int(k) != k or not 1 <= int(k) <= N.KMEANS_MAX_K:
        raise ValueError(f"k must be an integer from 1 to {N.KMEANS_MAX_K}, got {k}")
    pairs.need_device("esmdiff_amd.states")
    total = np.zeros((int(k), int(k)), np.int64)
    for t in trajs:
        dev = t if torch.is_tensor(t) else torch.as_tensor(np.ascontiguousarray(_labels_host(t).astype(np.int32)))
        total += pairs.transition_counts(dev.to(device="cuda", dtype=torch.int32).contiguous(), int(k), lagtime).cpu().numpy()
    return total


# ---- the Markov state model (host) ----------------------------------------------------------------------------------------------
def strongly_connected_sets(counts) -> List[np.ndarray]:
    """The strongly connected sets of the graph with an edge a -> b where counts[a][b] > 0 (Tarjan's algorithm, without recursion),
    each sorted, the largest first (of equal sizes the one with the smallest state first)."""
    C = np.asarray(counts)
    n = C.shape[0]
    succ = [np.flatnonzero(C[a] > 0).tolist() for a in range(n)]
    index, low, on_stack = [-1] * n, [0] * n, [False] * n
    stack, sets, counter = [], [], 0
    for root in range(n):
        if index[root] >= 0:
            continue
        work = [(root, 0)]
        while work:
            v, at = work.pop()
            if at == 0:
                index[v] = low[v] = counter
                counter += 1
                stack.append(v)
                on_stack[v] = True
            descended = False
            for i in range(at, len(succ[v])):
                w = succ[v][i]
                if index[w] < 0:
                    work.append((v, i + 1))
                    work.append((w, 0))
                    descended = True
                    break
                if on_stack[w]:
                    low[v] = min(low[v], index[w])
            if descended:
                continue
            if low[v] == index[v]:
                members = []
                while True:
                    w = stack.pop()
                    on_stack[w] = False
                    members.append(w)
                    if w == v:
                        break
                sets.append(np.array(sorted(members), np.int64))
            if work:
                u = work[-1][0]
                low[u] = min(low[u], low[v])
    return sorted(sets, key=lambda s: (-len(s), int(s[0])))


def reversible_mle(counts, maxiter: int = 100000, tol: float = 1e-12):
    """The reversible maximum-likelihood transition matrix of a connected count matrix by the fixed-point iteration
    x_ij <- (c_ij + c_ji) / (c_i / x_i + c_j / x_j) with c_i and x_i the row sums, started from x = C + C^T and scaled to sum 1
    after every sweep, until the largest change of T_ij = x_ij / x_i is <= tol -> T, pi = x_i / sum x, sweeps, converged."""
    C = np.asarray(counts, np.float64)
    ci = C.sum(1)
    if C.ndim != 2 or C.shape[0] != C.shape[1] or (ci <= 0).any():
        raise ValueError("reversible_mle takes a square count matrix with no empty row (the connected set's)")
    sym = C + C.T
    x = sym / sym.sum()
    T = x / x.sum(1)[:, None]
    sweeps, converged = 0, False
    while sweeps < int(maxiter):
        q = ci / x.sum(1)
        x = sym / (q[:, None] + q[None, :])
        x = x / x.sum()
        new = x / x.sum(1)[:, None]
        change = float(np.abs(new - T).max())
        T, sweeps = new, sweeps + 1
        if change <= tol:
            converged = True
            break
    return T, x.sum(1), sweeps, converged


@dataclass
class MetastableSets:
    """memberships (n_active, m): the clipped and renormalised inner-simplex memberships; assignment (n_active,): their argmax;
    weights (m,): the stationary weight of every crisp set; sets: the microstates (original labels) of every set."""
    memberships: np.ndarray
    assignment: np.ndarray
    weights: np.ndarray
    sets: List[np.ndarray]


@dataclass
class MSMModel:
    """[DEEPTIME-RECALL], PARITY UNPINNED: the maximum-likelihood Markov state model of deeptime / PyEMMA restated from the
    literature (neither package is installable here): the largest strongly connected set of the count matrix (active_set, the original
    labels, ascending), then the row-normalised counts (reversible=False) or the reversible maximum-likelihood fixed point
    (reversible_mle).  stationary_distribution: pi with pi T = pi; eigenvalues: all of T's, by decreasing magnitude, real for a
    reversible model (the eigenproblem is symmetrised with pi); timescales: -lagtime / ln of the eigenvalues after the first (of their
    magnitude for a complex one; NaN where kinetics.timescales_from_eigenvalues gives NaN).  Indices of transition_matrix,
    stationary_distribution and the memberships are positions in active_set."""
    lagtime: int
    reversible: bool
    counts: np.ndarray                  # (k, k), all states
    active_set: np.ndarray              # (n_active,)
    transition_matrix: np.ndarray       # (n_active, n_active)
    stationary_distribution: np.ndarray
    eigenvalues: np.ndarray
    right_eigenvectors: np.ndarray      # (n_active, n_active), columns in the order of the eigenvalues; the first is constant
    timescales: np.ndarray              # (n_active - 1,)
    n_iter: int
    converged: bool

    def metastable(self, m: int) -> MetastableSets:
        """m metastable sets by the inner-simplex step of PCCA+ (Weber's initial guess): the m rows of the leading right eigenvectors
        that span the largest simplex become the vertices, the memberships are the barycentric coordinates, clipped at zero and
        renormalised, the crisp assignment their argmax.  The optimisation step of PCCA+ is OUT OF SCOPE: memberships of a model
        whose states lie well inside the simplex are the same, others differ from a full PCCA+."""
        n = len(self.active_set)
        if int(m) != m or not 1 <= int(m) <= n:
            raise ValueError(f"m must be an integer from 1 to the {n} active states, got {m}")
        if np.iscomplexobj(self.eigenvalues) and np.abs(self.eigenvalues[:int(m)].imag).max() > 0:
            raise ValueError("metastable sets need real leading eigenvalues (a reversible model)")
        chi = inner_simplex(np.real(self.right_eigenvectors[:, :int(m)]))
        assignment = chi.argmax(1)
        weights = np.array([self.stationary_distribution[assignment == s].sum() for s in range(int(m))])
        return MetastableSets(chi, assignment, weights, [self.active_set[assignment == s] for s in range(int(m))])


def inner_simplex(evec) -> np.ndarray:
    """evec (n, m), the first column constant -> memberships (n, m): the vertex with the largest norm (in the columns after the
    first), then m - 1 times the row farthest from the span of the vertices found so far (Gram-Schmidt); the inverse of the vertices'
    rows maps evec to barycentric coordinates, which are clipped at zero and renormalised."""
    evec = np.asarray(evec, np.float64)
    n, m = evec.shape
    if m == 1:
        return np.ones((n, 1))
    c = evec[:, 1:].copy()
    ind = np.zeros(m, np.int64)
    ind[0] = int(np.argmax(np.sqrt((c * c).sum(1))))
    ortho = c - c[ind[0]]
    for j in range(1, m):
        temp = ortho[ind[j - 1]].copy()
        ortho = ortho - np.outer(ortho @ temp, temp)
        dist = np.sqrt((ortho * ortho).sum(1))
        ind[j] = int(np.argmax(dist))
        ortho = ortho / dist[ind[j]]
    chi = evec @ np.linalg.inv(evec[ind])
    chi = np.clip(chi, 0.0, None)
    return chi / chi.sum(1)[:, None]


def _spectrum(T: np.ndarray, pi: np.ndarray, reversible: bool):
    if reversible:                                                      # D^1/2 T D^-1/2 is symmetric under detailed balance
        s = np.sqrt(pi)
        S = (s[:, None] * T) / s[None, :]
        lam, v = np.linalg.eigh((S + S.T) / 2.0)
        order = np.argsort(-np.abs(lam), kind="stable")
        lam, R = lam[order], v[:, order] / s[:, None]
    else:
        lam, R = np.linalg.eig(T)
        order = np.argsort(-np.abs(lam), kind="stable")
        lam, R = lam[order], R[:, order]
        if np.abs(lam.imag).max() == 0.0:
            lam, R = lam.real, R.real
    R[:, 0] = 1.0                                                       # the eigenvalue 1 belongs to the constant function, exactly
    return lam, R


def _timescales(lam: np.ndarray, lagtime: int) -> np.ndarray:
    rest = lam[1:]
    if np.iscomplexobj(rest):
        rest = np.where(rest.imag == 0.0, rest.real, np.abs(rest))
    return kinetics.timescales_from_eigenvalues(rest, lagtime)


def msm(counts_or_labels, lagtime: int, reversible: bool = True, k: Optional[int] = None, maxiter: int = 100000, tol: float = 1e-12) -> MSMModel:
    """A square 2-D integer array is a count matrix; anything else is a label vector or a list of them, counted at `lagtime` with
    transition_counts (k states) -> MSMModel."""
    lagtime = kinetics._check_lag(lagtime)
    given = counts_or_labels
    is_counts = not isinstance(given, (list, tuple)) and not torch.is_tensor(given) and np.asarray(given).ndim == 2
    if is_counts:
        C = np.asarray(given)
        if C.shape[0] != C.shape[1] or C.shape[0] < 1 or (C < 0).any() or not np.isfinite(C).all():
            raise ValueError(f"a count matrix is square and non-negative, got {C.shape}")
    else:
        C = transition_counts(given, lagtime, k)
    sets = strongly_connected_sets(C)
    active = sets[0]
    sub = np.asarray(C, np.float64)[np.ix_(active, active)]
    if sub.sum() <= 0:
        raise ValueError("the count matrix holds no transition")
    if reversible:
        T, pi, sweeps, converged = reversible_mle(sub, maxiter, tol)
    else:
        T = sub / sub.sum(1)[:, None]
        w, v = np.linalg.eig(T.T)
        pi = np.real(v[:, int(np.argmin(np.abs(w - 1.0)))])
        pi, sweeps, converged = pi / pi.sum(), 0, True
    lam, R = _spectrum(T, pi, bool(reversible))
    return MSMModel(lagtime, bool(reversible), np.asarray(C), active, T, pi, lam, R, _timescales(lam, lagtime), sweeps, converged)


def msm_timescales(labels, lagtimes: Sequence[int], n: int = 3, k: Optional[int] = None, reversible: bool = True) -> np.ndarray:
    """The implied-timescale table -> (len(lagtimes), n): the n slowest timescales of the model at every lag time, NaN where the
    active set has fewer states or no timescale belongs to the eigenvalue."""
    out = np.full((len(lagtimes), int(n)), np.nan)
    if k is None:
        k = max([int(_labels_host(t).max()) + 1 for t in _label_list(labels) if len(t)] + [1])
    for r, lag in enumerate(lagtimes):
        ts = msm(labels, lag, reversible, k).timescales[:int(n)]
        out[r, :len(ts)] = ts
    return out


def _js(p: np.ndarray, q: np.ndarray) -> float:
    """The Jensen-Shannon DISTANCE of metrics.js_pwd: natural logarithm, square root, cells with a pseudo count."""
    p, q = p / p.sum(), q / q.sum()
    mid = (p + q) / 2.0
    left = np.where(p > 0, p * np.log(p / mid), 0.0)
    right = np.where(q > 0, q * np.log(q / mid), 0.0)
    return float(np.sqrt(max((left.sum() + right.sum()) / 2.0, 0.0)))


def compare_populations(sample_labels, model: MSMModel, assignment=None) -> dict:
    """The samples' microstate histogram on the model's active set against its stationary distribution: js (the Jensen-Shannon
    distance in js_pwd's conventions: natural logarithm, the square root, the pseudo count 1e-6 on every cell of both histograms, pi
    scaled to the samples' total), outside (the share of the samples whose label is not in the active set, -1 included), n_inside;
    with assignment (a MetastableSets or its assignment vector) also populations: per set the samples' share and the model's weight."""
    lab = _labels_host(sample_labels)
    position = {int(s): i for i, s in enumerate(model.active_set)}
    at = np.array([position.get(int(v), -1) for v in lab], np.int64)
    inside = at[at >= 0]
    hist = np.bincount(inside, minlength=len(model.active_set)).astype(np.float64)
    pi = model.stationary_distribution
    out = {"n_samples": int(len(lab)), "n_inside": int(len(inside)), "outside": float(1.0 - len(inside) / len(lab)) if len(lab) else float("nan"),
           "js": _js(hist + PSEUDO_C, pi * len(inside) + PSEUDO_C) if len(inside) else float("nan"),
           "sample_populations": hist / len(inside) if len(inside) else np.full(len(pi), np.nan), "stationary_distribution": pi}
    if assignment is not None:
        a = np.asarray(assignment.assignment if isinstance(assignment, MetastableSets) else assignment)
        m = int(a.max()) + 1
        share = np.array([hist[a == s].sum() for s in range(m)]) / len(inside) if len(inside) else np.full(m, np.nan)
        out["populations"] = {"samples": share, "msm": np.array([pi[a == s].sum() for s in range(m)])}
    return out


# ---- the command line's block ---------------------------------------------------------------------------------------------------
def report(trajectory, samples, targets, lagtime: int = 20, dim: int = 2, states: int = 100, msm_lagtime: Optional[int] = None,
           metastable: int = 2, seed: int = 0, chunk_frames: Optional[int] = None, n_eigenvalues: int = 5) -> dict:
    """The "msm" block of analyze_ensemble: trajectory (n, L, 3) (an array, a memmap or a PDB path), samples (n_s, L, 3) and targets
    (K, L, 3).  TICA at `lagtime` with `dim` components, k-means with `states` centres (kmeans++ from `seed`), the counts and the
    reversible model at msm_lagtime (default: lagtime), `metastable` sets."""
    msm_lagtime = int(lagtime if msm_lagtime is None else msm_lagtime)
    model = kinetics.tica(trajectory, lagtime, dim, chunk_frames=chunk_frames)
    traj = kinetics._trajectories(trajectory, False)[0]
    step = traj.shape[0] if chunk_frames is None else int(chunk_frames)
    proj = np.concatenate([model.transform(np.asarray(traj[s:s + step])) for s in range(0, traj.shape[0], step)], axis=0)
    km = kmeans(proj, states, seed=seed)
    counts = transition_counts(km.labels, msm_lagtime, states)
    M = msm(counts, msm_lagtime)
    sample_labels, target_labels = discretize(model, samples, km), discretize(model, targets, km)
    out = {"tica_lagtime": int(lagtime), "tica_dim": int(dim), "states": int(states), "lagtime": msm_lagtime, "seed": int(seed),
           "frames": int(traj.shape[0]), "inertia": km.inertia, "kmeans_iterations": km.n_iter, "kmeans_converged": km.converged,
           "centres": km.centres, "active_set": M.active_set, "active_states": int(len(M.active_set)), "count_total": int(counts.sum()),
           "mle_iterations": M.n_iter, "mle_converged": M.converged, "eigenvalues": M.eigenvalues[:n_eigenvalues],
           "timescales": M.timescales[:n_eigenvalues - 1], "stationary_distribution": M.stationary_distribution,
           "sample_labels": sample_labels, "target_labels": target_labels}
    sets = None
    if 2 <= int(metastable) <= len(M.active_set):
        sets = M.metastable(int(metastable))
        centres = km.centres[M.active_set]
        pi = M.stationary_distribution
        out["metastable"] = [{"states": s, "weight": float(w),
                              "mean_tic": (pi[sets.assignment == i][:, None] * centres[sets.assignment == i]).sum(0) / w if w > 0 else np.full(centres.shape[1], np.nan)}
                             for i, (s, w) in enumerate(zip(sets.sets, sets.weights))]
    out["compare_populations"] = compare_populations(sample_labels, M, sets)
    return out

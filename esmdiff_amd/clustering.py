"""Clustering of ensembles on the device: the GROMOS algorithm (Daura et al. 1999, the `gromos` method of `gmx cluster`) on the
all-pairs layer of esmdiff_amd/ensemble.py, and the populations of given states.

Which distinct conformations are in an ensemble, how populated is each, and which model represents each one.  The reference has
no clustering of its own: analysis/bpti_analysis.py reads the five kinetic clusters of BPTI from files; `state_populations` asks
that question ("how much of my ensemble is in each known basin") of any set of states.  There is no CPU fallback.

The algorithm (DESIGN.md "Clustering"; tests/cluster_ref.py restates it on the host): i < j are neighbours iff d[i, j] <= cutoff
(similarities, `larger_is_closer`: >=) — only the upper triangle of the matrix is ever read, that one entry decides the pair in
both directions, a NaN entry means "not neighbours", every structure is its own neighbour.  Among the structures not yet assigned
the one with the most unassigned neighbours (ties: the lowest index) is the centre of the next cluster; the cluster is the centre
and all its unassigned neighbours; repeat.  csrc/cluster.hip holds the relation as a bit matrix and runs the whole loop in one
launch; the matrix itself never has to exist in full.

metric="tm" is [TMSCORE-RECALL], PARITY UNPINNED, as every TM-score of esmdiff_amd/ensemble.py (its module docstring).
metric="lddt" (csrc/lddt.hip) needs no superposition and rests on no recalled program: integer counts, held exactly to numpy."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, NamedTuple

import numpy as np
import torch

from . import _native as N
from . import pairs

CLUSTER_MAX_N = N.CLUSTER_MAX_N
TM_NOTE = "[TMSCORE-RECALL], parity unpinned"


@dataclass
class Clustering:
    """labels (n,) int32: the cluster of each structure, clusters numbered in order of creation; centres (K,) int32: the structure
    at the centre of each cluster; sizes (K,) int32, non-increasing; n_clusters = K."""
    labels: np.ndarray
    centres: np.ndarray
    sizes: np.ndarray
    n_clusters: int


class Metric(NamedTuple):
    """device(X, Y, mx, my) -> (n, m) on the device, Y = None: X against itself.  one_sided: device(X, Y)[i, j] is normalised by
    Y[j] alone, and the metric is the symmetric mean of the two readings."""
    larger_is_closer: bool
    one_sided: bool
    device: Callable


def _rmsd(X, Y, mx, my, out=None):
    return pairs.superpose(X, Y, mx, my, False, ("rmsd",), None if out is None else {"rmsd": out})["rmsd"]


METRICS = {"rmsd": Metric(False, False, _rmsd), "tm": Metric(True, True, pairs.tm), "lddt": Metric(True, True, pairs.lddt)}


def _rule(metric: str) -> Metric:
    if metric not in METRICS:
        raise ValueError(f"metric should be 'rmsd', 'tm' or 'lddt', got {metric!r}")
    return METRICS[metric]


def _score(rule: Metric, X, Y, mx, my, out=None) -> torch.Tensor:
    """(n, m) on the device: the metric of every X[i] to every Y[j] (Y = None: to every X[j], in one launch); `out`: the buffer a
    two-sided metric's launch writes into."""
    if not rule.one_sided:
        return rule.device(X, Y, mx, my, out)
    s = rule.device(X, Y, mx, my)
    return 0.5 * (s + (s if Y is None else rule.device(Y, X, my, mx)).T)


def _check_n(n: int, what: str):
    if not 1 <= n <= CLUSTER_MAX_N:
        raise ValueError(f"{what}: n = {n} structures, the clustering kernel takes 1 to {CLUSTER_MAX_N} (one count per structure in LDS)")


def _gromos(adj: torch.Tensor) -> Clustering:
    out, k = pairs.gromos(adj)
    K = int(k.item())
    labels, centres, sizes = out.cpu().numpy()
    return Clustering(labels.copy(), centres[:K].copy(), sizes[:K].copy(), K)


def cluster_matrix(d, cutoff: float, larger_is_closer: bool = False, block_rows: int = 1024) -> Clustering:
    """GROMOS clustering of n structures from any square matrix d (numpy, or a tensor on the host or the device) of distances, or
    with larger_is_closer of similarities.  Only d[i, j] with i < j is read.  A host matrix goes to the device `block_rows` rows at
    a time."""
    shape = tuple(d.shape) if hasattr(d, "shape") else np.shape(d)
    if len(shape) != 2 or shape[0] != shape[1]:
        raise ValueError(f"cluster_matrix takes a square matrix, got {shape}")
    n = int(shape[0])
    _check_n(n, "cluster_matrix")
    pairs.need_device("esmdiff_amd.clustering")
    if not torch.is_tensor(d):
        d = np.asarray(d)
    adj = pairs.adjacency(n)
    for r0 in range(0, n, max(1, int(block_rows))):
        rows = d[r0:r0 + max(1, int(block_rows))]
        block = (rows if torch.is_tensor(rows) else torch.as_tensor(np.ascontiguousarray(rows))).to(device="cuda", dtype=torch.float64)
        pairs.threshold(block.contiguous(), r0, cutoff, larger_is_closer, adj)
    return _gromos(adj)


def cluster_ensemble(samples, cutoff: float, metric: str = "rmsd", mask=None, block_rows: int = 1024) -> Clustering:
    """GROMOS clustering of an ensemble: `samples` (n, L, 3) CA traces as everywhere in esmdiff_amd/ensemble.py (array, tensor or
    path), residues with NaN coordinates or masked by `mask` (n, L) left out of every superposition.

    metric="rmsd": cutoff in Angstrom on the RMSD after least-squares superposition with proper rotations (pairwise_rmsd).  The
    relation is built from blocks of `block_rows` rows of the all-pairs matrix (esmdiff_superpose_pairs of the block against all,
    then esmdiff_cluster_threshold): no more than block_rows x n doubles of the matrix exist at any time, and nothing of it crosses
    to the host.
    metric="tm": cutoff on the symmetric mean 0.5 (tm[i, j] + tm[j, i]) of the TM-score, larger is closer.  The mean needs both
    triangles, so the FULL n x n TM matrix is built on the device (8 n^2 bytes, and one workgroup per ordered pair).
    [TMSCORE-RECALL], PARITY UNPINNED (esmdiff_amd/ensemble.py): the TM search restates the TMscore program's heuristic from
    memory and has not been compared with the program.
    metric="lddt": cutoff on the symmetric mean 0.5 (l[i, j] + l[j, i]) of the CA-lDDT (ensemble.lddt_matrix, default radius and
    thresholds), larger is closer; a pair without a defined lDDT (NaN) is not a neighbour.  The same row-block path as the RMSD:
    per block one launch for the block against all and one for all against the block (a block of all rows: one launch in all)."""
    rule = _rule(metric)
    A = pairs.coords(samples, "samples")
    n = A.shape[0]
    _check_n(n, "cluster_ensemble")
    ma = pairs.valid_mask(A, mask)
    adj = pairs.adjacency(n)
    # tm takes no row blocks: the symmetric mean of a block needs the block against all AND all against the block, every ordered
    # pair would be scored twice and the time double; one full n x n launch scores each once (lddt pays that: its launch is cheap)
    step = n if metric == "tm" else max(1, min(int(block_rows), n))
    buf = None if rule.one_sided else torch.empty((step, n), dtype=torch.float64, device="cuda")
    for r0 in range(0, n, step):
        r1 = min(r0 + step, n)
        Y, my = (None, None) if r1 - r0 == n else (A, ma)   # all rows: the ensemble against itself, one launch
        block = _score(rule, A[r0:r1], Y, None if ma is None else ma[r0:r1], my, None if buf is None else buf[:r1 - r0])
        pairs.threshold(block.contiguous(), r0, cutoff, rule.larger_is_closer, adj)
    return _gromos(adj)


def centre_distances(samples, clustering: Clustering, metric: str = "rmsd", mask=None) -> np.ndarray:
    """Each structure's distance to the centre of its own cluster -> (n,): the RMSD in Angstrom (the centres themselves: 0 to
    rounding), or for metric="tm" the symmetric mean TM-score ([TMSCORE-RECALL], parity unpinned), for metric="lddt" the symmetric
    mean lDDT.  One n x K launch (two for a similarity) and a gather."""
    rule = _rule(metric)
    A = pairs.coords(samples, "samples")
    labels = np.asarray(clustering.labels)
    assert labels.shape == (A.shape[0],), f"the clustering is of {labels.shape[0]} structures, the samples are {A.shape[0]}"
    ma = pairs.valid_mask(A, mask)
    centres = torch.as_tensor(np.asarray(clustering.centres), dtype=torch.int64, device="cuda")
    C = A[centres].contiguous()
    mc = None if ma is None else ma[centres].contiguous()
    d = _score(rule, A, C, ma, mc)
    return d.gather(1, torch.as_tensor(labels, dtype=torch.int64, device="cuda")[:, None])[:, 0].cpu().numpy()


def state_populations(samples, states, cutoff=None, metric: str = "rmsd"):
    """Each sample goes to the nearest of K given states (K, L, 3) -> (assignment (n,) int32, populations (K,), distance (n,)):
    the state's index (ties: the lowest), the fraction of the n samples assigned to each state, and the sample's RMSD to its state
    (metric="tm": the symmetric mean TM-score, and nearest means largest; [TMSCORE-RECALL], parity unpinned; metric="lddt": the
    symmetric mean lDDT, nearest means largest).  With a cutoff a sample farther than it from every state (tm, lddt: below it) is
    assigned to none, -1, and the populations sum to less than one; so is a sample with no defined distance to any state (NaN).
    `distance` is to the nearest state either way."""
    rule = _rule(metric)
    A, S = pairs.coords(samples, "samples"), pairs.coords(states, "states")
    assert S.shape[1] == A.shape[1], f"structures of different lengths: {A.shape[1]} and {S.shape[1]} (the correspondence is residue to residue)"
    d = _score(rule, A, S, pairs.valid_mask(A, None), pairs.valid_mask(S, None))
    K, larger = S.shape[0], rule.larger_is_closer
    worst = float("-inf") if larger else float("inf")
    key = torch.where(torch.isnan(d), torch.full_like(d, worst), d)
    best = key.max(1).values if larger else key.min(1).values
    index = torch.arange(K, device="cuda")[None].expand_as(key)
    assignment = torch.where(key == best[:, None], index, torch.full_like(index, K)).min(1).values     # the lowest index on a tie
    none = best == worst
    if cutoff is not None:
        none |= (best < cutoff) if larger else (best > cutoff)
    assignment = torch.where(none, torch.full_like(assignment, -1), assignment)
    populations = torch.bincount(assignment[~none], minlength=K).to(torch.float64) / A.shape[0]
    distance = torch.where(best == worst, torch.full_like(best, float("nan")), best)
    return assignment.to(torch.int32).cpu().numpy(), populations.cpu().numpy(), distance.cpu().numpy()

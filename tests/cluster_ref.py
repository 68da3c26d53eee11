"""TEST INFRASTRUCTURE — NumPy restatement of the GROMOS clustering of esmdiff_amd/csrc/cluster.hip (Daura et al. 1999), in the
NAIVE form: the neighbour count of every remaining structure is taken again from the whole relation for every cluster, O(K n^2).
Deliberately not the kernel's algorithm (counts taken once and maintained as structures leave).

  neighbours   for i < j: d[i, j] <= cutoff (larger_is_closer: d[i, j] >= cutoff).  Only the upper triangle is read; that one
               entry decides the pair in both directions.  A NaN entry: not neighbours.  The diagonal: always neighbours.
  loop         among the structures not yet assigned, the one with the most unassigned neighbours (itself included; ties: the
               lowest index) is the centre of the next cluster; the cluster is the centre and all its unassigned neighbours.
  outputs      labels int32 (n,) in order of creation, centres int32 (K,), sizes int32 (K,), K."""
from __future__ import annotations

import numpy as np


def neighbours(d, cutoff: float, larger_is_closer: bool = False) -> np.ndarray:
    """-> the symmetric relation, bool (n, n)."""
    d = np.asarray(d, np.float64)
    n = d.shape[0]
    assert d.shape == (n, n)
    with np.errstate(invalid="ignore"):
        near = (d >= cutoff) if larger_is_closer else (d <= cutoff)          # NaN compares False
    upper = np.triu(near, 1)
    return upper | upper.T | np.eye(n, dtype=bool)


def gromos(adj: np.ndarray):
    """adj bool (n, n), symmetric with a true diagonal -> labels, centres, sizes, K."""
    adj = np.asarray(adj, bool)
    n = adj.shape[0]
    alive = np.ones(n, bool)
    labels, centres, sizes = np.full(n, -1, np.int32), [], []
    while alive.any():
        count = (adj & alive[None, :]).sum(1)             # every row, again
        count[~alive] = -1
        c = int(np.argmax(count))                          # the first maximum: the lowest index
        members = adj[c] & alive
        labels[members] = len(centres)
        centres.append(c)
        sizes.append(int(members.sum()))
        alive &= ~members
    return labels, np.array(centres, np.int32), np.array(sizes, np.int32), len(centres)


def cluster_matrix(d, cutoff: float, larger_is_closer: bool = False):
    return gromos(neighbours(d, cutoff, larger_is_closer))


def pack(adj: np.ndarray) -> np.ndarray:
    """bool (n, n) -> the kernel's bit matrix, uint64 (n, ceil(n / 64)): bit j % 64 of word j // 64, padding zero."""
    n = adj.shape[0]
    W = (n + 63) // 64
    bits = np.zeros((n, 64 * W), np.uint64)
    bits[:, :n] = adj
    return (bits.reshape(n, W, 64) << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64)

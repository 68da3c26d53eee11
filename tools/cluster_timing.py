#!/usr/bin/env python3
"""Time esmdiff_amd.clustering.cluster_ensemble (metric rmsd) on synthetic ensembles and split it into its three legs.

    python tools/cluster_timing.py [--n 1000 10000] [--L 58] [--states 20] [--noise 1.0] [--cutoff 3.0] [--repeats 3]
                                   [--host_max_n 1000] [--out profiles/cluster_timing.json]

The ensemble: `states` independent random-walk CA chains, every member one of them (uniformly drawn) plus Gaussian noise, rigidly
moved.  Per n:
  call      wall clock of cluster_ensemble, numpy in / Clustering out (upload, the block loop, the clustering loop, download);
  legs      the same block loop written out on device tensors, HIP events around each esmdiff_amd.pairs call: one C-ABI call (the
            entries synchronise the stream themselves) and, for the loop leg, the allocation of its two outputs; no other launch.
            all-pairs (esmdiff_superpose_pairs per row block), threshold (esmdiff_cluster_threshold per row block), loop
            (esmdiff_cluster_gromos: the symmetrisation and the persistent clustering kernel);
  singletons the loop leg again on the relation of a cutoff below every distance: K = n clusters, the most iterations the loop
            kernel can run;
  host      for n <= host_max_n: the naive NumPy restatement of the test suite (tests/cluster_ref.py) on the matrix
            ensemble.pairwise_rmsd returns, timed on this machine's host, and compared with the device's result."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from esmdiff_amd import clustering, ensemble, pairs  # noqa: E402
from tests import cluster_ref as C, ensemble_ref as E  # noqa: E402


def make(rng, n, L, states, noise):
    base = [E.ca_chain(rng, L) for _ in range(states)]
    origin = rng.integers(0, states, size=n)
    return np.stack([(base[k] + rng.normal(size=(L, 3)) * noise) @ E.random_rotation(rng).T + rng.normal(size=3) * 20 for k in origin])


def timed(fn):
    """-> ms between HIP events around fn(), and what it returned."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    got = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), got


def legs(X, cutoff, block_rows):
    """-> ms of the three legs, and the result."""
    A = torch.as_tensor(X).cuda().contiguous()
    n = A.shape[0]
    adj = pairs.adjacency(n)
    buf = torch.empty((min(block_rows, n), n), dtype=torch.float64, device="cuda")
    ms = {"all_pairs": 0.0, "threshold": 0.0}
    for r0 in range(0, n, block_rows):
        block = buf[:min(block_rows, n - r0)]
        ms["all_pairs"] += timed(lambda: pairs.superpose(A[r0:r0 + block.shape[0]], A, None, None, False, ("rmsd",), {"rmsd": block}))[0]
        ms["threshold"] += timed(lambda: pairs.threshold(block, r0, cutoff, False, adj))[0]
    ms["loop"], (out, k) = timed(lambda: pairs.gromos(adj))
    return ms, out.cpu().numpy(), int(k.item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1000, 10000])
    ap.add_argument("--L", type=int, default=58)
    ap.add_argument("--states", type=int, default=20)
    ap.add_argument("--noise", type=float, default=1.0)
    ap.add_argument("--cutoff", type=float, default=3.0)
    ap.add_argument("--block_rows", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host_max_n", type=int, default=1000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"L": a.L, "states": a.states, "noise": a.noise, "cutoff": a.cutoff, "block_rows": a.block_rows, "repeats": a.repeats,
           "device": torch.cuda.get_device_name(0), "runs": []}
    legs(make(np.random.default_rng(1), 130, a.L, 3, a.noise), a.cutoff, a.block_rows)       # warm-up (code object load)
    for n in a.n:
        X = make(np.random.default_rng(n), n, a.L, a.states, a.noise)
        run = {"n": n}
        wall = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            got = clustering.cluster_ensemble(X, a.cutoff, block_rows=a.block_rows)
            wall.append((time.perf_counter() - t0) * 1e3)
        run["call_ms_median"], run["call_ms_all"] = statistics.median(wall), wall
        run["n_clusters"], run["largest"] = got.n_clusters, got.sizes[:5].tolist()
        for name, cutoff in (("legs_ms", a.cutoff), ("singletons_legs_ms", 1e-6)):
            reps = [legs(X, cutoff, a.block_rows) for _ in range(a.repeats)]
            run[name] = {k: statistics.median(r[0][k] for r in reps) for k in ("all_pairs", "threshold", "loop")}
            run[name + "_all"] = [r[0] for r in reps]
            run[name.replace("legs_ms", "n_clusters")] = reps[0][2]
            if name == "legs_ms":
                assert reps[0][2] == got.n_clusters and np.array_equal(reps[0][1][0], got.labels)
        if n <= a.host_max_n:
            d = ensemble.pairwise_rmsd(X)
            host = {}
            for name, cutoff in (("cutoff", a.cutoff), ("singletons", 1e-6)):
                t0 = time.perf_counter()
                want = C.cluster_matrix(d, cutoff)
                host[name + "_s"] = time.perf_counter() - t0
                dev = clustering.cluster_matrix(d, cutoff)
                host[name + "_equal"] = bool(dev.n_clusters == want[3] and np.array_equal(dev.labels, want[0])
                                             and np.array_equal(dev.centres, want[1]) and np.array_equal(dev.sizes, want[2]))
            run["host_restatement"] = host
        res["runs"].append(run)
        print(json.dumps(run), flush=True)
    text = json.dumps(res, indent=1)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")
    print(text)


if __name__ == "__main__":
    main()

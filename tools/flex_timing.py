"""Times the pairwise RMSF of an ensemble on one MI355X by its two routes; a record, not a gate.

    python tools/flex_timing.py [--out profiles/flex_timing.json] [--sizes 100 1000] [--L 256]

  new   esmdiff_amd.flexibility.pair_rmsf: csrc/flex.hip reduces the pairs on the device, O(n L) memory, (L,) doubles to the host
  old   the route ensemble.apo_report takes: ensemble.aligned_deviation(S) (an (n, n, 2 L) array of squared deviations on the device,
        its first L columns square-rooted and copied to the host) and numpy's sqrt(mean(dev[iu] ** 2, 0))

Device tensors in, numpy out; wall clock around each whole call (both end on the host, so both are synchronised); per size one
warm-up of each route, then the two routes alternate; every repeat is kept, in the order it was taken.  `launch` is the one C-ABI
call alone (pairs.pair_msf on prepared tensors: two output allocations, the scratch allocation, both kernels; the entry synchronises
its stream), taken back to back after the alternating block.  Also records the largest difference of the squared results and the
peak device memory of each route."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="profiles/flex_timing.json")
ap.add_argument("--sizes", type=int, nargs="+", default=[100, 1000])
ap.add_argument("--L", type=int, default=256)
args = ap.parse_args()
OUT = Path(args.out)
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from esmdiff_amd import ensemble, flexibility, pairs
from tests import ensemble_ref as E

out = {"device": torch.cuda.get_device_name(0), "L": args.L, "cases": []}


def old_route(S):
    dev = ensemble.aligned_deviation(S)
    iu = np.triu_indices(S.shape[0], 1)
    return np.sqrt(np.mean(dev[iu] ** 2, axis=0))


def timed(fn, S):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t = time.perf_counter()
    r = fn(S)
    return time.perf_counter() - t, torch.cuda.max_memory_allocated(), r


for n in args.sizes:
    S = torch.as_tensor(E.ensemble(np.random.default_rng(n), n, args.L)).cuda()
    reps = 11 if n <= 200 else 5
    timed(flexibility.pair_rmsf, S), timed(old_route, S)           # warm-up of both
    new, old = [], []
    for _ in range(reps):
        tn, mem_new, rn = timed(flexibility.pair_rmsf, S)
        to, mem_old, ro = timed(old_route, S)
        new.append(tn), old.append(to)
    launch = []
    for _ in range(2 * reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        pairs.pair_msf(S, None)
        launch.append(time.perf_counter() - t)
    case = {"n": n, "pairs": n * (n - 1) // 2, "reps": reps, "pair_rmsf_s": new, "aligned_deviation_numpy_s": old, "launch_s": launch,
            "peak_device_bytes_new": int(mem_new), "peak_device_bytes_old": int(mem_old),
            "max_abs_diff_squared": float(np.abs(rn ** 2 - ro ** 2).max()),
            "pairs_per_s_launch_median": n * (n - 1) / 2 / float(np.median(launch))}
    out["cases"].append(case)
    print(json.dumps(case), flush=True)
    OUT.parent.mkdir(parents=True, exist_ok=True)
    OUT.write_text(json.dumps(out, indent=1) + "\n")

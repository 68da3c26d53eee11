"""Times the all-pairs CA-lDDT (esmdiff_amd.ensemble.lddt_matrix, csrc/lddt.hip) on one MI355X and the numpy restatement of the test
suite (tests/lddt_ref.py) on that machine's host; a record, not a gate.

    python tools/lddt_timing.py [--out profiles/lddt_timing.json] [--no-host]

Cases: 100 x 100 and 1 000 x 1 000 models at L = 256, 100 x 100 at L = 1 024 (random-walk chains, 0 - 2.5 A noise); per case every
repeat of the whole call (numpy in, numpy out excluded: device tensors in) and of the one C-ABI launch (which synchronises its
stream), the share of residue pairs inside R0, and the pair rates at the median launch time.  The host leg runs the two
100 x 100 cases native by native and checks that its integers equal the device's."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="profiles/lddt_timing.json")
ap.add_argument("--no-host", action="store_true")
args = ap.parse_args()
OUT = Path(args.out)
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from esmdiff_amd import ensemble, pairs
from tests import lddt_ref as R

out = {"device": torch.cuda.get_device_name(0), "cases": []}
rng = np.random.default_rng(0)


def make(n, m, L):
    base = R.chain(rng, L)
    return R.ensemble(rng, n, base), R.ensemble(rng, m, base, 0.0, 1.5)


def device_case(n, m, L, reps):
    A, B = make(n, m, L)
    a, b = torch.as_tensor(A).cuda(), torch.as_tensor(B).cuda()
    ensemble.lddt_matrix(a, b)                                   # warm-up (module load, LDS attribute)
    call, kern = [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        ensemble.lddt_matrix(a, b)
        call.append(time.perf_counter() - t)
        torch.cuda.synchronize()
        t = time.perf_counter()
        kept, total, _, _ = pairs.lddt_counts(a, b, None, None)                # the launch alone: synchronises the stream
        kern.append(time.perf_counter() - t)
    total = total.cpu().numpy()
    ordered = n * m * L * L
    case = {"n": n, "m": m, "L": L, "reps": reps, "lddt_matrix_s": sorted(call), "launch_s": sorted(kern),
            "ordered_pairs": ordered, "pairs_inside_r0_fraction": float(total.sum() / (m * L * (L - 1))),
            "ordered_pairs_per_s_median": ordered / float(np.median(kern)),
            "scored_pairs_per_s_median": float(n * total.sum()) / float(np.median(kern))}
    out["cases"].append(case)
    print(json.dumps(case), flush=True)
    OUT.parent.mkdir(parents=True, exist_ok=True)
    OUT.write_text(json.dumps(out, indent=1) + "\n")
    return A, B, kept.cpu().numpy(), total


def host_case(A, B, kept, total, case):
    t = time.perf_counter()
    k2 = np.zeros(kept.shape, np.int64)
    for j in range(B.shape[0]):                                   # native by native: progress lines
        kj, tj, _, _ = R.counts(A, B[j:j + 1])
        k2[:, j] = kj[:, 0]
        assert tj[0] == total[j]
        if j % 10 == 9:
            print(f"host {j + 1}/{B.shape[0]} {time.perf_counter() - t:.1f}s", flush=True)
    case["numpy_restatement_s"] = time.perf_counter() - t
    case["equal_to_device"] = bool(np.array_equal(k2, kept))
    print(json.dumps({k: case[k] for k in ("n", "m", "L", "numpy_restatement_s", "equal_to_device")}), flush=True)
    OUT.write_text(json.dumps(out, indent=1) + "\n")


small = device_case(100, 100, 256, 7)
big = device_case(1000, 1000, 256, 5)
long_ = device_case(100, 100, 1024, 7)
if not args.no_host:
    host_case(*small, out["cases"][0])
    host_case(*long_, out["cases"][2])

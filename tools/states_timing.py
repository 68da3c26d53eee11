"""Times one Lloyd step and one transition count on one MI355X by two routes each; a record, not a gate.

    python tools/states_timing.py [--out profiles/states_timing.json] [--shapes 100000x2x100 1000000x16x1000] [--lag 10]

  step, new     esmdiff_amd.pairs.kmeans_step: csrc/msm.hip, one pass over the frames, O(k d) scratch per chunk in flight
  step, old     the route a user would write: torch.cdist(Y, C) (an (n, k) float64 array), argmin, index_add_ for the sums (float
                atomics: the order changes from run to run), bincount for the sizes, and the row minima's sum for the inertia
  counts, new   esmdiff_amd.pairs.transition_counts
  counts, old   torch.bincount(a * k + b, minlength=k * k) on the label pairs

Device tensors in, device tensors out.  Every call is bracketed by events on the current stream and followed by a synchronise; per
shape two warm-up calls of each route, then the routes alternate and the median of the repeats is reported beside every repeat.  Peak
device memory is torch's allocator's over one call, above what is allocated before it (the new route's scratch is a torch tensor, so
it is counted).  The labels of the two step routes are compared: frames on which they differ are counted and the largest relative gap
between the two centres' squared distances (float64, recomputed term by term) is recorded: a difference is a near-tie that the
(n, k) route's rounding decides the other way."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="profiles/states_timing.json")
ap.add_argument("--shapes", nargs="+", default=["100000x2x100", "1000000x16x1000"])
ap.add_argument("--lag", type=int, default=10)
ap.add_argument("--reps", type=int, default=9)
args = ap.parse_args()
OUT = Path(args.out)
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from esmdiff_amd import pairs

out = {"device": torch.cuda.get_device_name(0), "lag": args.lag, "reps": args.reps, "cases": []}


def old_step(Y, C):
    dist = torch.cdist(Y, C)
    best, labels = dist.min(1)
    sums = torch.zeros_like(C).index_add_(0, labels, Y)
    counts = torch.bincount(labels, minlength=C.shape[0])
    return {"labels": labels, "counts": counts, "sums": sums, "inertia": (best * best).sum()}


def old_counts(labels, k, lag):
    a, b = labels[:-lag].long(), labels[lag:].long()
    return torch.bincount(a * k + b, minlength=k * k).view(k, k)


def timed(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), torch.cuda.max_memory_allocated() - base, r


def race(new, old, reps):
    for _ in range(2):
        timed(new), timed(old)
    tn, to = [], []
    for _ in range(reps):
        ms, mem_new, rn = timed(new)
        tn.append(ms)
        ms, mem_old, ro = timed(old)
        to.append(ms)
    return {"new_ms": tn, "old_ms": to, "new_ms_median": float(np.median(tn)), "old_ms_median": float(np.median(to)),
            "old_over_new": float(np.median(to) / np.median(tn)), "peak_bytes_new": int(mem_new), "peak_bytes_old": int(mem_old)}, rn, ro


for shape in args.shapes:
    n, d, k = map(int, shape.split("x"))
    gen = torch.Generator(device="cuda").manual_seed(n + k)
    C = torch.randn(k, d, generator=gen, dtype=torch.float64, device="cuda") * 2.0
    Y = C[torch.randint(0, k, (n,), generator=gen, device="cuda")] + 0.7 * torch.randn(n, d, generator=gen, dtype=torch.float64, device="cuda")
    case = {"n": n, "d": d, "k": k, "slots": pairs.kmeans_slots(k, d, -(-n // 1024))}
    case["step"], rn, ro = race(lambda: pairs.kmeans_step(Y, C), lambda: old_step(Y, C), args.reps)
    differ = torch.nonzero(rn["labels"].long() != ro["labels"]).flatten()
    gap = 0.0
    if len(differ):
        da = ((Y[differ] - C[rn["labels"][differ].long()]) ** 2).sum(1)
        db = ((Y[differ] - C[ro["labels"][differ]]) ** 2).sum(1)
        gap = float(((db - da).abs() / torch.maximum(da, db)).max())
    case["labels_differ"], case["labels_differ_max_relative_gap"] = int(len(differ)), gap
    case["labels_agree"] = bool(len(differ) == 0 or gap <= 1e-9)
    case["counts_equal"] = bool(torch.equal(rn["counts"], ro["counts"])) if len(differ) == 0 else None
    case["sums_max_abs_diff"] = float((rn["sums"] - ro["sums"]).abs().max())
    case["inertia_relative_diff"] = float(((rn["inertia"][0] - ro["inertia"]) / ro["inertia"]).abs())
    again = pairs.kmeans_step(Y, C)
    case["two_runs_bit_equal"] = bool(all(torch.equal(rn[key].view(torch.uint8), again[key].view(torch.uint8)) for key in rn))
    labels = rn["labels"]
    case["transition_counts"], cn, co = race(lambda: pairs.transition_counts(labels, k, args.lag), lambda: old_counts(labels, k, args.lag), args.reps)
    case["transition_counts_equal"] = bool(torch.equal(cn, co))
    del rn, ro, again, cn, co
    out["cases"].append(case)
    print(json.dumps(case), flush=True)
    OUT.parent.mkdir(parents=True, exist_ok=True)
    OUT.write_text(json.dumps(out, indent=1) + "\n")

"""Times the contact layer (esmdiff_amd.contacts, csrc/contacts.hip) on one MI355X against the route esmdiff_amd.metrics.idp_metrics
takes for the same numbers (pairwise_distance_ca, then torch's reductions over the (n_frames, n_pairs) array); a record, not a gate.

    python tools/contacts_timing.py [--out profiles/contacts_timing.json] [--reps 9]

Cases: contact_map with sums at 1 000 x 256 and 100 000 x 58 (the BPTI trajectory's shape) — per repeat the whole call on device tensors
(which ends in the entry's own stream synchronise, then the copy of the four maps to the host) and the one C-ABI call alone; the
distance-array route on the same tensor, alternating with it, ended by a device synchronise; the peak device memory of each route above
what the input holds; and that both give the same mean distances and contact frequencies.  native_contacts at 1 000 models x 5 natives
x 256 residues: the whole call and the launch alone."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="profiles/contacts_timing.json")
ap.add_argument("--reps", type=int, default=9)
args = ap.parse_args()
OUT = Path(args.out)
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from esmdiff_amd import _native as N
from esmdiff_amd import contacts, metrics, pairs
from tests import contacts_ref as R

out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "contact_map": [], "native_contacts": []}
rng = np.random.default_rng(0)


def spread(ts):
    return {"median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts)), "all_s": sorted(float(t) for t in ts)}


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, res


def peak(fn):
    """The peak of torch's allocator during fn, above what was allocated before it."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - before)


def array_route(x):
    pwd = metrics.pairwise_distance_ca(x, k=3)
    return pwd.mean(0), torch.log((pwd < 8.0).to(torch.float64).mean(0) + 0.01)


def map_case(n, L):
    X = torch.as_tensor(R.ensemble(rng, n, R.chain(rng, L))).cuda()
    for _ in range(2):                                           # warm-up of both routes at this shape
        contacts.contact_map(X)
        array_route(X)
    whole, launch, other = [], [], []
    for _ in range(args.reps):                                   # alternating
        whole.append(timed(lambda: contacts.contact_map(X))[0])
        launch.append(timed(lambda: pairs.contact_map(X, None, 8.0, 3))[0])
        other.append(timed(lambda: array_route(X))[0])
    m = contacts.contact_map(X)
    mean, logp = (t.cpu().numpy() for t in array_route(X))
    iu = m.pairs()
    case = {"n": n, "L": L, "chunks": N.contact_chunks(n, L), "chunk_frames": N.contact_chunk_frames(n, L),
            "scratch_bytes": N.contact_scratch_bytes(n, L),
            "contact_map_call": spread(whole), "contact_map_launch": spread(launch), "distance_array_route": spread(other),
            "peak_bytes_contact_map": peak(lambda: pairs.contact_map(X, None, 8.0, 3)), "peak_bytes_distance_array_route": peak(lambda: array_route(X)),
            "pair_frames_per_s_median_launch": n * L * (L - 1) / 2 / float(np.median(launch)),
            "max_abs_diff_mean_distance": float(np.abs(m.mean_distance()[iu] - mean).max()),
            "max_abs_diff_log_probability": float(np.abs(m.log_probability()[iu] - logp).max())}
    out["contact_map"].append(case)
    print(json.dumps(case), flush=True)


def native_case(n, m, L):
    base = R.chain(rng, L)
    A, B = torch.as_tensor(R.ensemble(rng, n, base)).cuda(), torch.as_tensor(R.ensemble(rng, m, base, 0.0, 1.0)).cuda()
    for _ in range(2):
        contacts.native_contacts(A, B)
    whole, launch, hard = [], [], []
    for _ in range(args.reps):
        whole.append(timed(lambda: contacts.native_contacts(A, B))[0])
        launch.append(timed(lambda: pairs.native_contacts(A, B, None, None, 8.0, 3, 1.2, 5.0))[0])
        hard.append(timed(lambda: pairs.native_contacts(A, B, None, None, 8.0, 3, 1.2, 5.0, soft=False))[0])
    total = pairs.native_contacts(A, B, None, None, 8.0, 3, 1.2, 5.0, soft=False)[1].cpu().numpy()
    case = {"n": n, "m": m, "L": L, "native_contacts_call": spread(whole), "launch_with_q_soft": spread(launch),
            "launch_counts_only": spread(hard), "contacts_per_native": total.tolist(),
            "scored_contacts_per_s_median_launch": float(n * total.sum()) / float(np.median(launch))}
    out["native_contacts"].append(case)
    print(json.dumps(case), flush=True)


map_case(1000, 256)
map_case(100000, 58)
native_case(1000, 5, 256)
OUT.parent.mkdir(parents=True, exist_ok=True)
OUT.write_text(json.dumps(out, indent=1) + "\n")
print(OUT)

#!/usr/bin/env python3
"""Time the superposition kernels on one 100 x 256 ensemble in self mode (4 950 distinct pairs; the launch computes all 10 000
ordered ones) and the same pairs through the host restatement (tests/ensemble_ref.py) on a subsample, extrapolated linearly.

    python tools/measure_ensemble.py [--n 100] [--L 256] [--repeats 7] [--host_pairs 24] [--out profiles/ensemble_timing.json]

Kernel time: HIP events around the esmdiff_amd.pairs call on tensors already on the device: one C-ABI call (the entry synchronises
the stream itself) and the allocation of its output.
Call time: wall clock of esmdiff_amd.ensemble.tm_matrix / pairwise_rmsd with numpy in and numpy out (upload, launch, download).
The reference's way — one `TMscore -seq` subprocess per pair — cannot be timed: the program is in no tree this project can reach."""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from esmdiff_amd import ensemble, pairs  # noqa: E402
from tests import ensemble_ref as E  # noqa: E402


def clocks() -> str:
    try:
        return subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=30).stdout.strip()
    except Exception as e:      # the tool is optional
        return f"rocm-smi unavailable: {e}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--L", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host_pairs", type=int, default=24)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    X = E.ensemble(rng, a.n, a.L, noise=2.0)
    Xd = torch.as_tensor(X).cuda()
    launches = {                                                        # one C entry each; what it returns stays on the device
        "tm_pairs": lambda: pairs.tm(Xd, None, None, None),
        "superpose_pairs": lambda: pairs.superpose(Xd, None, None, None, False, ("rmsd",))["rmsd"],
    }
    calls = {"tm_pairs": lambda: ensemble.tm_matrix(X), "superpose_pairs": lambda: ensemble.pairwise_rmsd(X)}
    res = {"n": a.n, "L": a.L, "ordered_pairs": a.n * a.n, "distinct_pairs": a.n * (a.n - 1) // 2, "repeats": a.repeats,
           "device": torch.cuda.get_device_name(0), "clocks_before": clocks()}
    launched = {}
    for name, fn in launches.items():
        fn()                                                         # warm-up (code object load)
        ms = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        wall = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            calls[name]()
            wall.append((time.perf_counter() - t0) * 1e3)
        launched[name] = out.cpu().numpy()
        res[name] = {"kernel_ms_median": statistics.median(ms), "kernel_ms_min": min(ms), "kernel_ms_max": max(ms),
                     "call_ms_median": statistics.median(wall), "kernel_ms_all": ms}
    # the host restatement on a subsample of the distinct pairs, extrapolated linearly to all of them
    iu = np.stack(np.triu_indices(a.n, 1), axis=1)
    pick = iu[rng.choice(len(iu), min(a.host_pairs, len(iu)), replace=False)]
    t0 = time.perf_counter()
    host_tm = [E.tm_pair(X[i], X[j])[0] for i, j in pick]
    t_tm = time.perf_counter() - t0
    t0 = time.perf_counter()
    host_rm = [E.superpose_pair(X[i], X[j])[0] for i, j in pick]
    t_rm = time.perf_counter() - t0
    scale = len(iu) / len(pick)
    tmh, rmh = launched["tm_pairs"], launched["superpose_pairs"]
    res["host_restatement"] = {"pairs_timed": len(pick), "tm_s_per_pair": t_tm / len(pick), "rmsd_s_per_pair": t_rm / len(pick),
                               "tm_s_extrapolated_to_distinct_pairs": t_tm * scale, "rmsd_s_extrapolated_to_distinct_pairs": t_rm * scale,
                               "max_abs_tm_difference": float(max(abs(tmh[i, j] - v) for (i, j), v in zip(pick, host_tm))),
                               "max_rel_rmsd_difference": float(max(abs(rmh[i, j] / v - 1) for (i, j), v in zip(pick, host_rm)))}
    res["clocks_after"] = clocks()
    res["note"] = ("host restatement = numpy, one process; the reference's own path (one TMscore subprocess and one scipy alignment per "
                   "pair) cannot be run: the TMscore program is in no tree this project can reach")
    text = json.dumps(res, indent=1)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")
    print(text)


if __name__ == "__main__":
    main()

"""Times the nearest-neighbour route of esmdiff_amd.neighbours (esmdiff_rmsd_prepare on both sides + esmdiff_rmsd_nearest: minima, indices,
sums, with no (n, m) matrix) against the route a user had before it: pairs.superpose in row blocks of 1 024 (an (n, m) RMSD matrix a
block; narrowed to 2^24 pairs a launch), then torch min / argmin / sum both ways.  Shapes: 1 000 x 100 000 at L = 58 (samples against BPTI), 250 x 30 000 at L = 512, 250 x
250 at L = 256, and 100 000 x 58 against itself, which the old route cannot run (5 x 10^9 pairs, an 80 GB matrix).  Both routes run in
one process, alternating, after a warm-up of each at the shape; times are device events around the whole call (the entries
synchronise, so they include launches and the wait); memory is torch.cuda.max_memory_allocated above what was allocated before the call
(the coordinates are not counted, the results are).  The old route is first timed on a tenth of the columns; where that predicts more
than --old_budget seconds for the whole shape the full run is skipped and the row says so ("old_extrapolated").  Also: the prepare and
nearest calls on their own, the rate of the nearest call against the data sheet's f64 matrix rate from 18 L FLOP a pair, whether the two
routes pick the same neighbours, and whether two runs of the new route give the same bits.  Writes profiles/neighbours_timing.json.

    python scratch/neighbours_timing.py [--out profiles/neighbours_timing.json] [--repeats 5] [--old_budget 20]"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from esmdiff_amd import _native as N          # noqa: E402
from esmdiff_amd import pairs                 # noqa: E402

FP64_MATRIX_PEAK = 78.6e12                    # FLOP / s, the MI355X data sheet's peak double-precision matrix rate (a multiply-add is two)
ROW_BLOCK = 1024
LAUNCH_PAIRS = 1 << 24                        # a row block is narrowed so that one esmdiff_superpose_pairs launch holds at most this many pairs:
                                              # at 1 000 x 100 000 in one launch its values were wrong from pair 32 891 136 on (EXPERIMENTS.md "Neighbours")


def trajectory(n, L, seed):
    """Chains of 3.8 Angstrom steps whose directions drift slowly with the frame index, every frame moved by its own rotation about z
    and its own translation (scratch/aligned_timing.py's)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rand = lambda *s: torch.randn(s, generator=g, device="cuda", dtype=torch.float64)
    drift = torch.cumsum(rand(n, 1, 3) * 0.05, 0)
    steps = rand(1, L, 3) + drift + 0.3 * rand(n, L, 3)
    X = torch.cumsum(steps * (3.8 / steps.norm(dim=-1, keepdim=True)), 1)
    a = rand(n) * 3.0
    rot = torch.zeros((n, 3, 3), device="cuda", dtype=torch.float64)
    rot[:, 0, 0], rot[:, 0, 1], rot[:, 1, 0], rot[:, 1, 1], rot[:, 2, 2] = torch.cos(a), -torch.sin(a), torch.sin(a), torch.cos(a), 1.0
    return (X @ rot.transpose(1, 2) + rand(n, 1, 3) * 20.0).contiguous()


def old_route(A, B):
    """The matrix in row blocks, reduced both ways as soon as a block exists."""
    n, m = A.shape[0], B.shape[0]
    row_min, row_arg, row_sum = (torch.empty(n, device="cuda", dtype=d) for d in (torch.float64, torch.int64, torch.float64))
    col_min = torch.full((m,), float("inf"), device="cuda", dtype=torch.float64)
    col_arg = torch.zeros(m, device="cuda", dtype=torch.int64)
    col_sum = torch.zeros(m, device="cuda", dtype=torch.float64)
    block = max(1, min(ROW_BLOCK, LAUNCH_PAIRS // m))
    for r0 in range(0, n, block):
        r1 = min(n, r0 + block)
        rmsd = pairs.superpose(A[r0:r1], B, None, None, False, ("rmsd",))["rmsd"]
        row_min[r0:r1], row_arg[r0:r1] = rmsd.min(1)
        row_sum[r0:r1] = rmsd.sum(1)
        cm, ca = rmsd.min(0)
        better = cm < col_min
        col_min, col_arg = torch.where(better, cm, col_min), torch.where(better, ca + r0, col_arg)
        col_sum += rmsd.sum(0)
    return row_min, row_arg, row_sum, col_min, col_arg, col_sum


def new_route(A, B):
    pa = pairs.rmsd_prepare(A)
    pb = None if B is None else pairs.rmsd_prepare(B)
    return pairs.rmsd_nearest(pa, pb)


def events(fn, repeats):
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return int(torch.cuda.max_memory_allocated() - before)


def stats(ms):
    return {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "neighbours_timing.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--old_budget", type=float, default=20.0, help="seconds one run of the old route may take at a shape")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a timing elsewhere says nothing"
    result = {"device": torch.cuda.get_device_name(0), "device_bytes": int(torch.cuda.mem_get_info()[1]), "repeats": args.repeats,
              "fp64_matrix_peak_flops": FP64_MATRIX_PEAK, "tile": N.RMSD_NN_TILE, "rectangle": N.RMSD_NN_RECT, "old_row_block": ROW_BLOCK, "old_launch_pairs": LAUNCH_PAIRS,
              "clocks": "as the device held them: not pinned, not read", "shapes": []}
    for n, m, L in ((250, 250, 256), (1000, 100000, 58), (250, 30000, 512), (100000, None, 58)):
        A = trajectory(n, L, 1)
        B = None if m is None else trajectory(m, L, 2)
        new = lambda: new_route(A, B)
        got = new()
        again = new()
        same_new = all(bool(torch.equal(got[k].view(torch.uint8), again[k].view(torch.uint8))) for k in got)
        del again
        pa = pairs.rmsd_prepare(A)
        pb = None if B is None else pairs.rmsd_prepare(B)
        nearest_only = lambda: pairs.rmsd_nearest(pa, pb)
        prepare_only = lambda: (pairs.rmsd_prepare(A), None if B is None else pairs.rmsd_prepare(B))
        pairs_count = n * (n - 1) // 2 if m is None else n * m
        row = {"n": n, "m": m, "L": L, "pairs": pairs_count, "coordinate_bytes": int((A.numel() + (0 if B is None else B.numel())) * 8)}
        t = {"new": [], "old": [], "nearest": [], "prepare": []}
        old = None
        if B is not None:
            sub = B[: max(m // 10, 1)].contiguous()
            old_route(A, sub)                                   # warm-up
            tenth = float(np.median(events(lambda: old_route(A, sub), 2)))
            row["old_ms_on_a_tenth_of_the_columns"] = tenth
            if tenth * (m / sub.shape[0]) * 1e-3 <= args.old_budget:
                old = lambda: old_route(A, B)
                want = old()
                row["same_row_index"] = float((want[1] == got["row_index"].long()).double().mean())
                row["same_col_index"] = float((want[4] == got["col_index"].long()).double().mean())
                row["row_rmsd_max_difference"] = float((want[0] - got["row_rmsd"]).abs().max())
                del want
            else:
                row["old_extrapolated"] = True
                row["old_ms"] = {"median": tenth * (m / sub.shape[0])}
        for _ in range(args.repeats):                           # alternating
            t["new"] += events(new, 1)
            if old is not None:
                t["old"] += events(old, 1)
            t["nearest"] += events(nearest_only, 1)
            t["prepare"] += events(prepare_only, 1)
        med = float(np.median(t["nearest"]))
        flops = 18.0 * L * pairs_count
        blocks = -(-n // N.RMSD_NN_RECT)
        rectangles = blocks * (blocks + 1) // 2 if m is None else blocks * -(-m // N.RMSD_NN_RECT)
        row.update({"rectangles": rectangles, "slots": pairs.rmsd_nn_slots(rectangles), "new_ms": stats(t["new"]), "nearest_call_ms": stats(t["nearest"]),
                    "prepare_calls_ms": stats(t["prepare"]), "new_device_bytes": peak_bytes(new), "new_two_runs_same_bits": same_new,
                    "gemm_flops": flops, "gemm_flops_per_s": flops / (med * 1e-3),
                    "nearest_call_share_of_f64_matrix_peak": flops / (med * 1e-3) / FP64_MATRIX_PEAK,
                    "pairs_per_s": pairs_count / (med * 1e-3)})
        if old is not None:
            row.update({"old_ms": stats(t["old"]), "old_device_bytes": peak_bytes(old),
                        "old_over_new": float(np.median(t["old"])) / float(np.median(t["new"]))})
        elif B is not None:
            row["old_over_new"] = row["old_ms"]["median"] / float(np.median(t["new"]))
        print(json.dumps(row), flush=True)
        result["shapes"].append(row)
        del A, B, pa, pb, got
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(args.out)


if __name__ == "__main__":
    main()

"""Times esmdiff_amd.pairs.debye_frames and esmdiff_amd.pairs.shape_frames (with the histogram) against the routes they replace —
torch float64 on the device: cdist, then sin(q d) / (q d) over an (frames, pairs, Q) array summed over the pairs, chunked over frames as
far as memory demands; and cdist + torch.histc — at 1 000 x 256 and 100 000 x 58 (the BPTI trajectory's shape) with Q = 51 and 100 bins.
Both routes run in one process, alternating; times are device events around the whole call (the entries synchronise, so they include
the launch and the wait).  Also: the Debye kernel's pair terms per second, the float64 instructions the device's FP64 vector rate could
issue per term at that rate, and the static count of float64 instructions per term (stated below) over that budget.  Writes
profiles/shape_timing.json.

    python scratch/shape_timing.py [--out profiles/shape_timing.json] [--repeats 10]"""
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

FP64_VECTOR_PEAK = 78.6e12                    # FLOP / s, the MI355X data sheet's peak double-precision vector rate (an FMA is two)
# float64 VALU instructions in the compiled debye_frames_kernel<false> (1 165 in the body unrolled over 8 q, both branches of sin's argument
# reduction included) per term: an UPPER bound of what a term with a small argument executes
F64_INSTRUCTIONS_PER_TERM = 1165 / 8
CHUNK_BYTES = 2 << 30                         # the torch route's (frames, pairs, Q) array is held below this


def ensemble(n, L, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    steps = torch.randn((n, L, 3), generator=g, device="cuda", dtype=torch.float64)
    steps = steps * (3.8 / steps.norm(dim=-1, keepdim=True))
    return torch.cumsum(steps, 1).contiguous()


def torch_debye(X, q):
    n, L = X.shape[:2]
    a, b = torch.triu_indices(L, L, 1, device="cuda")
    per = max(1, CHUNK_BYTES // (a.numel() * q.numel() * 8))
    out = torch.empty((n, q.numel()), dtype=torch.float64, device="cuda")
    for f0 in range(0, n, per):
        d = torch.cdist(X[f0:f0 + per], X[f0:f0 + per])[:, a, b]
        x = d[:, :, None] * q
        out[f0:f0 + per] = L + 2.0 * torch.where(x == 0, torch.ones_like(x), torch.sin(x) / x).sum(1)
    return out


def torch_frames(X, width, bins):
    n, L = X.shape[:2]
    a, b = torch.triu_indices(L, L, 1, device="cuda")
    per = max(1, CHUNK_BYTES // (L * L * 8 * 2))
    hist = torch.zeros(bins, dtype=torch.float64, device="cuda")
    inv, dmax = torch.empty(n, dtype=torch.float64, device="cuda"), torch.empty(n, dtype=torch.float64, device="cuda")
    for f0 in range(0, n, per):
        d = torch.cdist(X[f0:f0 + per], X[f0:f0 + per])[:, a, b]
        inv[f0:f0 + per], dmax[f0:f0 + per] = (1.0 / d).sum(1), d.max(1).values
        hist += torch.histc(d, bins=bins, min=0.0, max=width * bins)
    c = X - X.mean(1, keepdim=True)
    return (c.transpose(1, 2) @ c), inv, dmax, hist


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
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - before)


def stats(ms):
    return {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "shape_timing.json"))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--q_points", type=int, default=51)
    ap.add_argument("--bins", type=int, default=100)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a timing elsewhere says nothing"
    result = {"device": torch.cuda.get_device_name(0), "Q": args.q_points, "bins": args.bins, "repeats": args.repeats,
              "fp64_vector_peak_flops": FP64_VECTOR_PEAK, "f64_instructions_per_term_upper_bound": F64_INSTRUCTIONS_PER_TERM, "shapes": []}
    q = torch.linspace(0.0, 0.5, args.q_points, dtype=torch.float64, device="cuda")
    for n, L in ((1000, 256), (100000, 58)):
        X = ensemble(n, L, 1)
        width = float(np.ceil(pairs.shape_frames(X, None)[1][:, 10].max().item())) / args.bins
        for _ in range(2):                                           # warm-up of all four at this shape
            fd, td = pairs.debye_frames(X, None, q), torch_debye(X, q)
            ff, tf = pairs.shape_frames(X, None, width, args.bins), torch_frames(X, width, args.bins)
        agree = float(((fd - td).abs() / (L * L)).max().item())      # against N^2, the envelope at q = 0
        cells = int((ff[2][:args.bins].to(torch.float64) - tf[3]).abs().sum().item())   # histc's own edge rule: not the kernel's expression
        t = {k: [] for k in ("debye", "torch_debye", "frames", "torch_frames")}
        for _ in range(args.repeats):                                # alternating
            t["debye"] += events(lambda: pairs.debye_frames(X, None, q), 1)
            t["torch_debye"] += events(lambda: torch_debye(X, q), 1)
            t["frames"] += events(lambda: pairs.shape_frames(X, None, width, args.bins), 1)
            t["torch_frames"] += events(lambda: torch_frames(X, width, args.bins), 1)
        terms = n * (L * (L - 1) // 2) * args.q_points
        med = float(np.median(t["debye"]))
        rate = terms / (med * 1e-3)
        row = {"n": n, "L": L, "waves_per_frame": N.shape_waves(L), "pair_terms": terms,
               "debye_ms": stats(t["debye"]), "torch_debye_ms": stats(t["torch_debye"]),
               "frames_hist_ms": stats(t["frames"]), "torch_frames_hist_ms": stats(t["torch_frames"]),
               "debye_device_bytes": peak_bytes(lambda: pairs.debye_frames(X, None, q)),
               "torch_debye_device_bytes": peak_bytes(lambda: torch_debye(X, q)),
               "frames_hist_device_bytes": peak_bytes(lambda: pairs.shape_frames(X, None, width, args.bins)),
               "torch_frames_hist_device_bytes": peak_bytes(lambda: torch_frames(X, width, args.bins)),
               "debye_terms_per_s": rate,
               "debye_f64_issue_budget_per_term": (FP64_VECTOR_PEAK / 2) / rate,       # instructions the device could issue per term at that rate
               "debye_static_count_over_issue_budget": rate * F64_INSTRUCTIONS_PER_TERM / (FP64_VECTOR_PEAK / 2),
               "debye_largest_difference_from_torch_over_N2": agree, "histogram_cells_differing_from_histc_total": cells,
               "debye_speedup": float(np.median(t["torch_debye"])) / med,
               "frames_hist_speedup": float(np.median(t["torch_frames"])) / float(np.median(t["frames"]))}
        print(json.dumps(row))
        result["shapes"].append(row)
        del X
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(args.out)


if __name__ == "__main__":
    main()

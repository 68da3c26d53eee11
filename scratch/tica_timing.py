"""Times the fused covariances of esmdiff_amd.kinetics (esmdiff_lagged_means + esmdiff_lagged_moments, then the residual-sum correction)
against the route they replace, esmdiff_amd.metrics.tica_fit up to and including its four products: esmdiff_metrics_pwd's (n, D)
distance matrix, two centred copies, four rocBLAS products.  Shapes: 1 000 x 58 at lag 20 (an ensemble's size) and 100 000 x 58 at
lag 500 (the BPTI evaluation's).  Both routes run in one process, alternating, after a warm-up of each at the shape; times are device
events around the whole call (the entries synchronise, so they include launches and the wait); memory is
torch.cuda.max_memory_allocated above what was allocated before the call (the coordinates are not counted, the results are).  Also:
the multiply-adds the moments kernel issues on the f64 MFMA (three products on a diagonal tile pair, four elsewhere, 64 x 64 x m each,
padding included) over the whole moments call's time over the data sheet's f64 matrix rate; how far the two routes' covariances agree;
the moments call on the stored (n, D) distances instead (the same kernel without
its distance arithmetic: what the recomputation costs); and, EXTRAPOLATED from the measured bytes per frame and not tried, the largest n at 58 residues whose old route fits the device.
Writes profiles/tica_timing.json.

    python scratch/tica_timing.py [--out profiles/tica_timing.json] [--repeats 7] [--old_repeats 5]"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from esmdiff_amd import _native as N          # noqa: E402
from esmdiff_amd import kinetics, metrics, pairs   # noqa: E402

FP64_MATRIX_PEAK = 78.6e12                    # FLOP / s, the MI355X data sheet's peak double-precision matrix rate (a multiply-add is two)


def trajectory(n, L, seed):
    """Chains of 3.8 Angstrom steps whose directions drift slowly with the frame index (a random walk in time, smoothed over the chain)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    drift = torch.cumsum(torch.randn((n, 1, 3), generator=g, device="cuda", dtype=torch.float64) * 0.05, 0)
    steps = torch.randn((1, L, 3), generator=g, device="cuda", dtype=torch.float64) + drift + \
        0.3 * torch.randn((n, L, 3), generator=g, device="cuda", dtype=torch.float64)
    return torch.cumsum(steps * (3.8 / steps.norm(dim=-1, keepdim=True)), 1).contiguous()


def old_route(X, lag):
    """metrics.tica_fit's lines up to its four products, on metrics.pairwise_distance_ca's matrix."""
    x = metrics.pairwise_distance_ca(X)
    x0, xt = x[:-lag], x[lag:]
    mean = 0.5 * (x0.mean(0) + xt.mean(0))
    a, b = x0 - mean, xt - mean
    m = a.shape[0]
    return (a.T @ a + b.T @ b) / (2.0 * m), (a.T @ b + b.T @ a) / (2.0 * m)


def new_route(X, lag):
    return kinetics.lagged_moments(X, lag).covariances(True)


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


def mfma_flops(D, m):
    tiles = -(-D // 64)
    products = 3 * tiles + 4 * (tiles * (tiles - 1) // 2)
    frames = -(-m // 32) * 32                               # a chunk's last staged block is padded with zeros
    return 2.0 * products * 64 * 64 * frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "tica_timing.json"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--old_repeats", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a timing elsewhere says nothing"
    total = torch.cuda.mem_get_info()[1]
    result = {"device": torch.cuda.get_device_name(0), "device_bytes": int(total), "repeats": args.repeats, "old_repeats": args.old_repeats,
              "fp64_matrix_peak_flops": FP64_MATRIX_PEAK, "frame_chunk": N.LAGGED_FRAME_CHUNK, "clocks": "as the device held them: not pinned, not read",
              "shapes": []}
    for n, L, lag in ((1000, 58, 20), (100000, 58, 500)):
        X = trajectory(n, L, 1)
        D, m = N.lagged_features(L, 1), n - lag
        old, new = (lambda: old_route(X, lag)), (lambda: new_route(X, lag))
        ref, got = old(), new()                                 # warm-up of both at this shape, and how far they agree
        new()
        scale = float(ref[0].abs().max())
        differ = [float((g - r).abs().max()) / scale for g, r in zip(got, ref)]
        del ref, got
        mean0, meant = pairs.lagged_means(X, lag, 1)
        c = (mean0 + meant) / 2.0
        moments_only = lambda: pairs.lagged_moments(X, lag, c, 1)
        means_only = lambda: pairs.lagged_means(X, lag, 1)
        moments_only()
        F = metrics.pairwise_distance_ca(X)                     # the same moments from stored features: the kernel without its distances
        from_features = lambda: pairs.lagged_moments(F, lag, c, 0)
        same_bits = all(bool((a == b).all()) for a, b in zip(from_features().values(), moments_only().values()))
        t = {"new": [], "old": [], "moments": [], "means": [], "features": []}
        for k in range(args.repeats):                           # alternating
            t["new"] += events(new, 1)
            if k < args.old_repeats:
                t["old"] += events(old, 1)
            t["moments"] += events(moments_only, 1)
            t["means"] += events(means_only, 1)
            t["features"] += events(from_features, 1)
        del F
        chunks = -(-m // N.LAGGED_FRAME_CHUNK)
        slots = pairs.lagged_slots(D, chunks, True)
        med = float(np.median(t["moments"]))
        flops = mfma_flops(D, m)
        row = {"n": n, "L": L, "D": D, "lag": lag, "pairs": m, "coordinate_bytes": int(X.numel() * 8), "chunks": chunks, "slots": slots,
               "rounds": -(-chunks // slots),
               "new_ms": stats(t["new"]), "old_ms": stats(t["old"]), "moments_call_ms": stats(t["moments"]), "means_call_ms": stats(t["means"]),
               "moments_call_from_stored_features_ms": stats(t["features"]), "stored_features_give_the_same_bits": same_bits,
               "new_device_bytes": peak_bytes(new), "old_device_bytes": peak_bytes(old),
               "mfma_flops": flops, "rocblas_flops": 2.0 * 4 * D * D * m, "mfma_flops_per_s": flops / (med * 1e-3),
               "moments_call_share_of_f64_matrix_peak": flops / (med * 1e-3) / FP64_MATRIX_PEAK,
               "old_four_products_share_if_all_time_were_products": 2.0 * 4 * D * D * m / (float(np.median(t["old"])) * 1e-3) / FP64_MATRIX_PEAK,
               "covariances_max_difference_over_max_c00": differ, "speedup": float(np.median(t["old"])) / float(np.median(t["new"]))}
        print(json.dumps(row), flush=True)
        result["shapes"].append(row)
        del X
    big = result["shapes"][-1]
    per_frame = big["old_device_bytes"] / big["n"]
    fits = int((total - 16 * big["D"] ** 2) // (per_frame + L * 24))
    result["largest_n_old_route_extrapolated"] = {"L": 58, "old_bytes_per_frame": per_frame, "n": fits, "coordinate_bytes_at_n": fits * 58 * 24,
                                                  "new_device_bytes_at_n": big["new_device_bytes"],
                                                  "note": "extrapolated from the bytes per frame measured at 100 000 frames; not tried"}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(args.out)


if __name__ == "__main__":
    main()

"""Times the fused aligned moments of esmdiff_amd.covariance (esmdiff_flex_transforms + esmdiff_aligned_moments: S = sum a a^T and r = sum a
of the frames superposed on a reference, the transform applied inside the staging) against the route they replace, flexibility.pca's:
esmdiff_flex_fit's aligned (n, L, 3) array, a centred copy and one rocBLAS product X^T X.  Shapes: 250 x 256 (a sampled ensemble),
100 000 x 58 (BPTI) and 30 000 x 512 (an ATLAS-sized protein).  Both routes run in one process, alternating, after a warm-up of each at
the shape; times are device events around the whole call (the entries synchronise, so they include launches and the wait); memory is
torch.cuda.max_memory_allocated above what was allocated before the call (the coordinates are not counted, the results are).  Also: the
two calls of the new route on their own; how far the two routes' sums agree; whether two runs of each route give the same bits; and,
for every shape, the multiply-adds the moments kernel issues on the f64 MFMA (a diagonal tile pair skips the six blocks left of the
diagonal; 64 x 64 x frames elsewhere, padding included) over the moments call's time over the data sheet's f64 matrix rate.
Writes profiles/aligned_timing.json.

    python scratch/aligned_timing.py [--out profiles/aligned_timing.json] [--repeats 7]"""
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


def trajectory(n, L, seed):
    """Chains of 3.8 Angstrom steps whose directions drift slowly with the frame index, every frame moved by its own rotation about z
    and its own translation."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rand = lambda *s: torch.randn(s, generator=g, device="cuda", dtype=torch.float64)
    drift = torch.cumsum(rand(n, 1, 3) * 0.05, 0)
    steps = rand(1, L, 3) + drift + 0.3 * rand(n, L, 3)
    X = torch.cumsum(steps * (3.8 / steps.norm(dim=-1, keepdim=True)), 1)
    a = rand(n) * 3.0
    rot = torch.zeros((n, 3, 3), device="cuda", dtype=torch.float64)
    rot[:, 0, 0], rot[:, 0, 1], rot[:, 1, 0], rot[:, 1, 1], rot[:, 2, 2] = torch.cos(a), -torch.sin(a), torch.sin(a), torch.cos(a), 1.0
    return (X @ rot.transpose(1, 2) + rand(n, 1, 3) * 20.0).contiguous()


def old_route(X, ref):
    """pairs.fit's aligned array, centred on the reference, and the library product."""
    aligned, _ = pairs.fit(X, None, ref, None)
    a = (aligned - ref[None]).reshape(X.shape[0], -1)
    return a.T @ a, a.sum(0)


def new_route(X, ref):
    T, _, ok = pairs.flex_transforms(X, None, ref, None)
    res = pairs.aligned_moments(X, T, ok, ref.reshape(-1))
    return res["S"], res["r"]


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


def mfma_flops(D, n):
    tiles = -(-D // 64)
    blocks = 10 * tiles + 16 * (tiles * (tiles - 1) // 2)   # 16 x 16 blocks of a tile pair: the diagonal one skips six
    chunk = N.ALIGNED_FRAME_CHUNK
    frames = (n // chunk) * chunk + -(-(n % chunk) // 32) * 32    # a chunk's last staged block is padded with zeros
    return 2.0 * blocks * 16 * 16 * frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "aligned_timing.json"))
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a timing elsewhere says nothing"
    result = {"device": torch.cuda.get_device_name(0), "device_bytes": int(torch.cuda.mem_get_info()[1]), "repeats": args.repeats,
              "fp64_matrix_peak_flops": FP64_MATRIX_PEAK, "frame_chunk": N.ALIGNED_FRAME_CHUNK,
              "clocks": "as the device held them: not pinned, not read", "shapes": []}
    for n, L in ((250, 256), (100000, 58), (30000, 512)):
        X = trajectory(n, L, 1)
        ref = X[0].contiguous()
        D = 3 * L
        old, new = (lambda: old_route(X, ref)), (lambda: new_route(X, ref))
        want, got = old(), new()                                # warm-up of both at this shape, and how far they agree
        again_new, again_old = new(), old()
        scale = float(want[0].abs().max())
        differ = [float((g - w).abs().max()) / s for g, w, s in zip(got, want, (scale, float(want[1].abs().max())))]
        same_new = all(bool((a == b).all()) for a, b in zip(got, again_new))
        same_old = all(bool((a == b).all()) for a, b in zip(want, again_old))
        symmetric = bool((got[0] == got[0].T).all())
        del want, got, again_new, again_old
        T, _, ok = pairs.flex_transforms(X, None, ref, None)
        center = ref.reshape(-1).contiguous()
        moments_only = lambda: pairs.aligned_moments(X, T, ok, center)
        transforms_only = lambda: pairs.flex_transforms(X, None, ref, None)
        fit_only = lambda: pairs.fit(X, None, ref, None)
        moments_only()
        t = {"new": [], "old": [], "moments": [], "transforms": [], "fit": []}
        for _ in range(args.repeats):                           # alternating
            t["new"] += events(new, 1)
            t["old"] += events(old, 1)
            t["moments"] += events(moments_only, 1)
            t["transforms"] += events(transforms_only, 1)
            t["fit"] += events(fit_only, 1)
        chunks = -(-n // N.ALIGNED_FRAME_CHUNK)
        slots = pairs.aligned_slots(L, chunks)
        tiles = -(-D // 64)
        med = float(np.median(t["moments"]))
        flops = mfma_flops(D, n)
        row = {"n": n, "L": L, "D": D, "coordinate_bytes": int(X.numel() * 8), "chunks": chunks, "slots": slots, "rounds": -(-chunks // slots),
               "workgroups_per_round": min(slots, chunks) * tiles * (tiles + 1) // 2,
               "new_ms": stats(t["new"]), "old_ms": stats(t["old"]), "moments_call_ms": stats(t["moments"]),
               "transforms_call_ms": stats(t["transforms"]), "old_fit_call_ms": stats(t["fit"]),
               "new_device_bytes": peak_bytes(new), "old_device_bytes": peak_bytes(old),
               "new_two_runs_same_bits": same_new, "old_two_runs_same_bits": same_old, "new_S_exactly_symmetric": symmetric,
               "mfma_flops": flops, "rocblas_flops": 2.0 * D * D * n, "mfma_flops_per_s": flops / (med * 1e-3),
               "moments_call_share_of_f64_matrix_peak": flops / (med * 1e-3) / FP64_MATRIX_PEAK,
               "sums_max_difference_over_max": differ, "old_over_new": float(np.median(t["old"])) / float(np.median(t["new"]))}
        print(json.dumps(row), flush=True)
        result["shapes"].append(row)
        del X, T, ok
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(args.out)


if __name__ == "__main__":
    main()

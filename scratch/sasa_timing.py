"""Times esmdiff_amd.pairs.sasa_frames (all six outputs) against the route it replaces — torch float64 on the device: the points of
every atom, their distances to every atom of the frame (cdist) in chunks of 2 GiB over frames, then any / sum — at 1 000 x 256 x 4 and
100 000 x 58 x 4 atoms with P = 96; and esmdiff_amd.pairs.cooccurrence at n = 100 000, L = 256 against float64 matrix products of the
flag table.  Both routes run in one process, alternating; times are device events around the whole call (the entries synchronise, so
they include the launch and the wait).  Also: the neighbour visits per second (an atom j inside the cull radius of an atom i, tested
against the wave's 128 point slots; counted with torch on a sample of frames, the early exit ignored), and the float64 instructions
of one visit (counted in the source: 9 per point and slot, 2 slots, and R_j R_j) over what the device's FP64 vector rate can issue.
Writes profiles/sasa_timing.json.

    python scratch/sasa_timing.py [--out profiles/sasa_timing.json] [--repeats 10] [--torch_repeats 3]"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from esmdiff_amd import accessibility         # noqa: E402
from esmdiff_amd import pairs                 # noqa: E402

FP64_VECTOR_PEAK = 78.6e12                    # FLOP / s, the MI355X data sheet's peak double-precision vector rate (an FMA is two)
F64_INSTRUCTIONS_PER_VISIT = 2 * 9 + 1        # per lane: two point slots of 3 subtractions, 3 products, 2 sums, 1 comparison; R_j R_j
LDS_READS_PER_VISIT = 4                       # x, y, z, R of the neighbour, each one 8-byte broadcast read of the wave
CHUNK_BYTES = 2 << 30                         # the torch route's (frames, atoms x points, atoms) array is held below this


def ensemble(n, L, seed):
    """Random coils: CA 3.8 Angstrom apart, N / C / O about 1.45 Angstrom from their CA."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    steps = torch.randn((n, L, 3), generator=g, device="cuda", dtype=torch.float64)
    ca = torch.cumsum(steps * (3.8 / steps.norm(dim=-1, keepdim=True)), 1)
    off = torch.randn((n, L, 4, 3), generator=g, device="cuda", dtype=torch.float64)
    off = off * (1.45 / off.norm(dim=-1, keepdim=True))
    off[:, :, 1] = 0.0
    return (ca[:, :, None, :] + off).contiguous()


def torch_sasa(X, R, u, threshold):
    """-> count (n, L, A), sum_count (L, A), exposed (n, L): the same quantities by torch.cdist's distances (its own arithmetic: a point
    on the boundary may fall on the other side)."""
    n, L, A = X.shape[:3]
    NA, P = L * A, u.shape[0]
    r = R.reshape(-1)
    per = max(1, CHUNK_BYTES // (NA * P * NA * 8))
    count = torch.empty((n, NA), dtype=torch.int32, device="cuda")
    for f0 in range(0, n, per):
        c = X[f0:f0 + per].reshape(-1, NA, 3)
        p = c[:, :, None, :] + r[None, :, None, None] * u[None, None, :, :]
        d = torch.cdist(p.reshape(-1, NA * P, 3), c).view(-1, NA, P, NA)
        d.diagonal(dim1=1, dim2=3).fill_(float("inf"))
        count[f0:f0 + per] = P - (d < r).any(-1).sum(-1)
    count = count.view(n, L, A)
    sphere = 4.0 * np.pi * R * R
    rel = (sphere * count / P).sum(-1) / sphere.sum(-1)
    return count, count.sum(0, dtype=torch.int64), (rel > threshold).to(torch.uint8)


def neighbour_visits(X, R, frames=64):
    """The mean number per frame of ordered pairs (i, j), j != i, with d_ij < R_i + R_j: what the kernel tests against its points."""
    c = X[:frames].reshape(min(frames, X.shape[0]), -1, 3)
    r = R.reshape(-1)
    near = torch.cdist(c, c) < (r[:, None] + r[None, :])
    return float((near.sum((1, 2)) - c.shape[1]).to(torch.float64).mean().item())


def torch_cooccurrence(flags):
    d, o = (flags < 2).to(torch.float64), (flags == 1).to(torch.float64)
    return torch.stack([d.T @ d, o.T @ d, o.T @ o])


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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sasa_timing.json"))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--torch_repeats", type=int, default=3)
    ap.add_argument("--points", type=int, default=96)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a timing elsewhere says nothing"
    result = {"device": torch.cuda.get_device_name(0), "P": args.points, "repeats": args.repeats, "torch_repeats": args.torch_repeats,
              "fp64_vector_peak_flops": FP64_VECTOR_PEAK, "f64_instructions_per_visit": F64_INSTRUCTIONS_PER_VISIT,
              "lds_broadcast_reads_per_visit": LDS_READS_PER_VISIT, "shapes": []}
    u = torch.as_tensor(accessibility.sphere_points(args.points), device="cuda")
    threshold = accessibility.THRESHOLD
    for n, L in ((1000, 256), (100000, 58)):
        X = ensemble(n, L, 1)
        R = torch.as_tensor(accessibility.expanded_radii(None, accessibility.PROBE, L, 4), device="cuda")
        kernel = lambda: pairs.sasa_frames(X, None, R, u, threshold)
        route = lambda: torch_sasa(X, R, u, threshold)
        got, ref = kernel(), route()                                   # warm-up of both at this shape, and how far they agree
        kernel()
        differ = int((got["count"] != ref[0]).sum().item())
        t = {"kernel": [], "torch": []}
        for k in range(args.repeats):                                   # alternating
            t["kernel"] += events(kernel, 1)
            if k < args.torch_repeats:
                t["torch"] += events(route, 1)
        visits = neighbour_visits(X, R) * n
        med = float(np.median(t["kernel"]))
        rate = visits / (med * 1e-3)
        wave_issue = FP64_VECTOR_PEAK / 2 / 64                          # float64 wave instructions the device can issue a second
        row = {"n": n, "L": L, "A": 4, "atoms_per_frame": 4 * L, "brute_force_point_tests": n * (4 * L) * args.points * (4 * L - 1),
               "kernel_ms": stats(t["kernel"]), "torch_ms": stats(t["torch"]),
               "kernel_device_bytes": peak_bytes(kernel), "torch_device_bytes": peak_bytes(route),
               "neighbour_visits": visits, "neighbour_visits_per_atom": visits / (n * 4 * L), "neighbour_visits_per_s": rate,
               "f64_share_of_issue_rate": rate * F64_INSTRUCTIONS_PER_VISIT / wave_issue,
               "counts_differing_from_torch": differ, "counts": int(got["count"].numel()),
               "exposed_flags_differing_from_torch": int((got["exposed"] != ref[2]).sum().item()),
               "speedup": float(np.median(t["torch"])) / med}
        print(json.dumps(row), flush=True)
        result["shapes"].append(row)
        del X, got, ref

    n, L = 100000, 256
    g = torch.Generator(device="cuda").manual_seed(2)
    flags = (torch.rand((n, L), generator=g, device="cuda") * 2.2).to(torch.uint8)
    kernel, route = (lambda: pairs.cooccurrence(flags)), (lambda: torch_cooccurrence(flags))
    single = lambda: flags.T.to(torch.float64) @ flags.to(torch.float64)
    got, ref = kernel(), route()
    single()
    t = {"kernel": [], "torch": [], "single": []}
    for _ in range(args.repeats):
        t["kernel"] += events(kernel, 1)
        t["torch"] += events(route, 1)
        t["single"] += events(single, 1)
    row = {"n": n, "L": L, "kernel_ms": stats(t["kernel"]), "torch_three_products_ms": stats(t["torch"]), "torch_one_product_ms": stats(t["single"]),
           "kernel_device_bytes": peak_bytes(kernel), "torch_three_products_device_bytes": peak_bytes(route),
           "torch_one_product_device_bytes": peak_bytes(single), "cells_differing_from_torch": int((got.to(torch.float64) != ref).sum().item()),
           "speedup_over_three_products": float(np.median(t["torch"])) / float(np.median(t["kernel"])),
           "speedup_over_one_product": float(np.median(t["single"])) / float(np.median(t["kernel"]))}
    print(json.dumps(row), flush=True)
    result["cooccurrence"] = row
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(args.out)


if __name__ == "__main__":
    main()

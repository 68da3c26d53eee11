"""Times esmdiff_amd.pairs.ramachandran (one fused esmdiff_ramachandran call) against the route it replaces — the three (n, L) angle
arrays of esmdiff_backbone_torsions copied to the host and numpy.histogram2d per residue — at 1 000 x 256 and 100 000 x 58 (the
BPTI trajectory's shape), N / CA / C backbones, 36 bins.  Both routes run in one process, alternating; times are device events around
the whole call (the entries synchronise, so they include the two memsets, the launch and the wait), the host route by a host clock
(it ends in host work).  Writes profiles/torsions_timing.json.

    python scratch/torsions_timing.py [--out profiles/torsions_timing.json] [--repeats 20]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from esmdiff_amd import _native as N          # noqa: E402
from esmdiff_amd import pairs                 # noqa: E402
from tests.dssp_ref import nerf               # noqa: E402

HBM_PEAK, HBM_ACHIEVABLE = 8.0e12, 6.3e12     # bytes / s


def ensemble(n, L, seed):
    rng = np.random.default_rng(seed)
    base = nerf([(a, b) for a, b in zip(rng.uniform(-150, -50, L), rng.uniform(-60, 160, L))])[:, :3]
    g = torch.Generator(device="cuda").manual_seed(seed)
    X = torch.as_tensor(base, device="cuda")[None] + 0.1 * torch.randn((n, L, 3, 3), generator=g, device="cuda", dtype=torch.float64)
    return X.contiguous()


def fused(X, bins):
    return pairs.ramachandran(X, None, 2.5, bins)


def host_route(X, bins):
    phi, psi, omega, _ = pairs.backbone_torsions(X, None, 2.5)
    phi, psi, omega = (t.cpu().numpy() * 57.29577951308232 for t in (phi, psi, omega))
    L = phi.shape[1]
    hist = np.zeros((L, bins, bins), np.int32)
    for i in range(L):
        ok = np.isfinite(phi[:, i]) & np.isfinite(psi[:, i])
        hist[i] = np.histogram2d(phi[ok, i], psi[ok, i], bins=bins, range=((-180, 180), (-180, 180)))[0]
    return hist


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "torsions_timing.json"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--bins", type=int, default=36)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a timing elsewhere says nothing"
    result = {"device": torch.cuda.get_device_name(0), "bins": args.bins, "atoms": 3, "repeats": args.repeats, "shapes": []}
    for n, L in ((1000, 256), (100000, 58)):
        X = ensemble(n, L, 1)
        for _ in range(3):                                           # warm-up of both routes at this shape
            f = fused(X, args.bins)
            h = host_route(X, args.bins)
        mismatched = int((f[0].cpu().numpy() != h).sum())            # histogram2d's own edge rule: not the kernel's expression
        t_fused, t_host = [], []
        for _ in range(args.repeats):                                # alternating
            t_fused += events(lambda: fused(X, args.bins), 1)
            t0 = time.perf_counter()
            host_route(X, args.bins)
            t_host.append((time.perf_counter() - t0) * 1e3)
        t_entry1 = events(lambda: pairs.backbone_torsions(X, None, 2.5), args.repeats)
        nbytes = n * L * 3 * 24
        med = float(np.median(t_fused))
        row = {"n": n, "L": L, "chunks": N.rama_chunks(n, L), "chunk_frames": N.rama_chunk_frames(n, L), "input_bytes": nbytes,
               "fused_ms": {"median": med, "min": float(np.min(t_fused)), "max": float(np.max(t_fused))},
               "host_route_ms": {"median": float(np.median(t_host)), "min": float(np.min(t_host)), "max": float(np.max(t_host))},
               "backbone_torsions_ms": {"median": float(np.median(t_entry1)), "min": float(np.min(t_entry1))},
               "fused_bytes_per_s": nbytes / (med * 1e-3), "fused_share_of_hbm_peak": nbytes / (med * 1e-3) / HBM_PEAK,
               "fused_share_of_hbm_achievable": nbytes / (med * 1e-3) / HBM_ACHIEVABLE,
               "fused_device_bytes": peak_bytes(lambda: fused(X, args.bins)),
               "host_route_device_bytes": peak_bytes(lambda: pairs.backbone_torsions(X, None, 2.5)),
               "host_route_host_bytes": 3 * n * L * 8, "cells_differing_from_histogram2d": mismatched,
               "speedup": float(np.median(t_host)) / med}
        print(json.dumps(row))
        result["shapes"].append(row)
        del X
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(args.out)


if __name__ == "__main__":
    main()

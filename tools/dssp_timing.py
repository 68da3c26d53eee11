"""Times the secondary-structure assignment on one MI355X, and the numpy restatement on the same box; a record, not a gate.

    python tools/dssp_timing.py [--out profiles/dssp_timing.json]

Cases: 100 and 1 000 structures of 256 residues, one chain of 4 096.  Inputs: copies of the 1fmf.A backbone of
tests/golden/g14_backbones.npz side by side (60 A apart), cut to L residues, 0.3 A of seeded Gaussian noise per structure, the
chain's proline flags, no mask.
  call_s     wall clock around the one C-ABI call on prepared device tensors (pairs.dssp: four output allocations, the memset of the
             counts, both kernels; the entry synchronises its stream), after a synchronise; one warm-up, then `reps` calls back to back
  device_ms  the same calls between two device events on the call's stream
  numpy_s    tests/dssp_ref.dssp (the vectorised restatement) on the host, whole batch
Every repeat is kept, in the order it was taken.  `exact` records that the device's outputs equal the restatement's (codes,
acceptors, counts, and the energies bit for bit) on the timed inputs."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="profiles/dssp_timing.json")
args = ap.parse_args()
OUT = Path(args.out)
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from esmdiff_amd import pairs
from tests import dssp_ref as R

golden = np.load(ROOT / "tests" / "golden" / "g14_backbones.npz")
xyz, seq = golden["1fmf_A_xyz"], str(golden["1fmf_A_seq"])
out = {"device": torch.cuda.get_device_name(0), "cases": []}

for n, L, reps, host_reps in ((100, 256, 200, 3), (1000, 256, 100, 1), (1, 4096, 200, 2)):
    copies = -(-L // len(xyz))
    base = np.concatenate([xyz + np.array([0.0, 0.0, 60.0 * k]) for k in range(copies)])[:L]
    no_donor = np.array([c == "P" for c in seq * copies], np.uint8)[:L]
    X = base[None] + 0.3 * np.random.default_rng(1000 * n + L).normal(size=(n, L, 4, 3))
    Xd, nd = torch.as_tensor(X).cuda(), torch.as_tensor(no_donor).cuda()
    got = pairs.dssp(Xd, None, nd)                                # warm-up
    call, device = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t = time.perf_counter()
        a.record()
        got = pairs.dssp(Xd, None, nd)
        b.record()
        call.append(time.perf_counter() - t)
        b.synchronize()
        device.append(a.elapsed_time(b))
    host = []
    for _ in range(host_reps):
        t = time.perf_counter()
        ref = R.dssp(X, None, no_donor)
        host.append(time.perf_counter() - t)
    ss, counts, acceptor, energy = (g.cpu().numpy() for g in got)
    exact = bool(np.array_equal(ss, ref[0]) and np.array_equal(counts, ref[1]) and np.array_equal(acceptor, ref[2])
                 and np.array_equal(energy.view(np.int64), ref[3].view(np.int64)))
    case = {"n": n, "L": L, "reps": reps, "call_s": call, "device_ms": device, "numpy_s": host, "exact": exact,
            "call_s_median": float(np.median(call)), "device_ms_median": float(np.median(device)), "numpy_s_median": float(np.median(host)),
            "helix_strand_coil": [float(v) for v in np.bincount(R.reduce3(ref[0]).reshape(-1), minlength=3) / ref[0].size]}
    out["cases"].append(case)
    print(json.dumps({k: v for k, v in case.items() if k not in ("call_s", "device_ms")}), flush=True)
    OUT.parent.mkdir(parents=True, exist_ok=True)
    OUT.write_text(json.dumps(out, indent=1) + "\n")

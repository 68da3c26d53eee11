"""Exhaustive sweep of the shared math (esmdiff_amd/csrc/ed_math.h through the C oracle) against float64: EVERY float32 of
ed_expf's domain [-104, 88.72283] and of ed_logf's domain [1e-10, 8192], in the measure of tests/shared_math_ref.py.  Not a test
(about 10^9 points, minutes on one core); tests/test_shared_math_cpu.py asserts the same measure on a subset of 2^24 .. 2^26 points per
function.  Prints one JSON line per range: the largest error, where, and every break of monotonicity between neighbouring floats.

    python tools/shared_math_sweep.py [--chunk 16777216]

EXPERIMENTS.md ("Shared math, exhaustively") records the output.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from oracle import c_oracle                    # noqa: E402
from tests import shared_math_ref as R         # noqa: E402


def sweep(name, fn, errors, lo, hi, chunk):
    """Every float of [lo, hi]: worst error per class of `errors` (a dict of masks -> error arrays), monotone breaks."""
    lo_o, hi_o = int(R.ordinal(lo)), int(R.ordinal(hi))
    worst, breaks, n, last = {}, [], 0, None
    t0 = time.perf_counter()
    for a in range(lo_o, hi_o + 1, chunk):
        x = R.from_ordinal(np.arange(a, min(a + chunk, hi_o + 1), dtype=np.int64))
        got = fn(x)
        for cls, (err, mask) in errors(x, got).items():
            if mask.any():
                e = np.where(mask, err, -1.0)
                i = int(e.argmax())
                if e[i] > worst.get(cls, (-1.0, None))[0]:
                    worst[cls] = (float(e[i]), float(x[i]))
        if last is not None and got[0] < last[1]:
            breaks.append(float(last[0]))
        breaks += [float(v) for v in x[R.monotone_breaks(x, got)]]
        last = (x[-1], got[-1])
        n += x.size
    print(json.dumps({"function": name, "from": float(lo), "to": float(hi), "floats": n,
                      "worst": {k: {"error": round(v[0], 4), "at": repr(v[1])} for k, v in worst.items()},
                      "monotone_breaks": breaks, "seconds": round(time.perf_counter() - t0, 1)}), flush=True)


def exp_classes(x, got):
    err, normal, sub = R.exp_errors(x, got)
    return {"normal results, ulp": (err, normal), "subnormal results, units of 2^-149": (err, sub)}


def log_classes(x, got):
    return {"ulp": (R.log_errors(x, got), np.ones(x.shape, dtype=bool))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunk", type=int, default=1 << 24)
    chunk = ap.parse_args().chunk
    tiny = np.float32(2.0 ** -20)
    sweep("ed_expf", c_oracle.expf, exp_classes, R.EXP_LO, np.nextafter(R.EXP_SUBNORMAL_BELOW, np.float32(0)), chunk)
    sweep("ed_expf", c_oracle.expf, exp_classes, R.EXP_SUBNORMAL_BELOW, -tiny, chunk)
    sweep("ed_expf", c_oracle.expf, exp_classes, -tiny, tiny, chunk)
    sweep("ed_expf", c_oracle.expf, exp_classes, tiny, R.EXP_HI, chunk)
    sweep("ed_logf", c_oracle.logf, log_classes, R.LOG_LO, np.float32(1.0), chunk)
    sweep("ed_logf", c_oracle.logf, log_classes, np.float32(1.0), R.LOG_HI, chunk)
    u = R.uniforms()
    term = c_oracle.logf(u + R.NOISE_EPS)
    err = R.log_errors(u + R.NOISE_EPS, term)
    nerr, allowed = R.noise_errors(u, R.noise_host(c_oracle.logf, u))
    print(json.dumps({"function": "ed_logf(u + 1e-10f), all 2^24 uniforms", "worst ulp": round(float(err.max()), 4),
                      "at u": repr(float(u[err.argmax()])),
                      "largest absolute error": float(np.abs(term.astype(np.float64) - np.log((u + R.NOISE_EPS).astype(np.float64))).max()),
                      "noise 1e-10f - ed_logf(u + 1e-10f), worst in the term's ulp": round(float(nerr.max()), 4),
                      "noise at u": repr(float(u[nerr.argmax()])), "noise within its allowance": bool((nerr <= allowed).all())}))


if __name__ == "__main__":
    main()

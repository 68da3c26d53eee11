"""The shared math of esmdiff_amd/csrc/ed_math.h on the host (the C oracle's copy) against float64, on the point sets of
tests/shared_math_ref.py: every float of each domain at an odd stride, the ends of every binade, the neighbourhoods of every
reduction boundary (k + 1/2) ln 2, of the sqrt 2 switch of ed_logf in every binade and of the thresholds, and all 2^24 uniforms.

The sampler tests compare the kernels with an oracle that includes the same header, so a flaw in it is invisible to them; this file
holds the header itself to float64.  Bars: the exhaustive maxima of tools/shared_math_sweep.py (EXPERIMENTS.md), rounded up.
tests/test_gpu_shared_math.py holds each unit's device copy to the same bits on the same points."""
import numpy as np
import pytest

from oracle import c_oracle
from tests import shared_math_ref as R


@pytest.fixture(scope="module")
def exp_runs():
    return [(name, x, c_oracle.expf(x)) for name, x in R.exp_pieces()]


@pytest.fixture(scope="module")
def log_runs():
    return [(name, x, c_oracle.logf(x)) for name, x in R.log_pieces()]


def test_point_sets():
    """2^24 .. 2^26 points per function, strides co-prime to the mantissa size, every named region present."""
    for pieces in (R.exp_pieces(), R.log_pieces(), R.noise_pieces()):
        n = sum(x.size for _, x in pieces)
        assert 1 << 24 <= n <= 1 << 26, n
        for _, x in pieces:
            assert x.dtype == np.float32 and (np.diff(R.ordinal(x)) > 0).all()
    assert R.EXP_STRIDE % 2 == 1 and R.LOG_STRIDE % 2 == 1
    x = R.points(R.exp_pieces())
    assert x.min() < R.EXP_LO and x.max() > R.EXP_HI
    for t in (R.EXP_LO, R.EXP_SUBNORMAL_BELOW, R.EXP_TOP_BRANCH, R.EXP_HI, np.float32(0.0)):
        assert (x == t).any()
    ex = set(np.unique(R.points(R.exp_pieces()).view(np.uint32) >> 23 & 0xFF).tolist())
    assert ex >= set(range(0, 134))                         # subnormal inputs up to the binade of 88
    xl = R.points(R.log_pieces())
    assert xl.min() == R.LOG_LO and xl.max() == R.LOG_HI
    m = (xl.view(np.uint32) & 0x7FFFFF) | 0x3F800000
    for e in range(-33, 13):                                # both sides of the switch in every whole binade of the domain
        inb = (xl >= np.float32(2.0 ** e)) & (xl < np.float32(2.0 ** (e + 1)))
        mm = m[inb].view(np.float32)
        assert (mm == R.SQRT2).any() and (mm > R.SQRT2).any() and (mm < R.SQRT2).any(), e


def test_exp_accuracy(exp_runs):
    worst_n, worst_s = (0.0, None), (0.0, None)
    n_sub = 0
    for name, x, got in exp_runs:
        err, normal, sub = R.exp_errors(x, got)
        n_sub += int(sub.sum())
        for mask, kind in ((normal, "n"), (sub, "s")):
            if mask.any():
                e = np.where(mask, err, -1.0)
                i = int(e.argmax())
                if kind == "n" and e[i] > worst_n[0]:
                    worst_n = (float(e[i]), float(x[i]))
                if kind == "s" and e[i] > worst_s[0]:
                    worst_s = (float(e[i]), float(x[i]))
        if name in ("stride", "thresholds"):
            assert R.exp_ends_ok(x, got), name
    print(f"MEASURED shared math host ed_expf: normal results {worst_n[0]:.4f} ulp at x = {worst_n[1]!r}; {n_sub} subnormal results "
          f"{worst_s[0]:.4f} units of 2^-149 at x = {worst_s[1]!r}")
    assert n_sub > 2000000          # the piece "subnormal results" is every float of that branch
    assert worst_n[0] <= R.EXP_BAR_ULP
    assert worst_s[0] <= R.EXP_SUBNORMAL_BAR
    # exact values the callers rely on
    assert c_oracle.expf(np.float32([0.0, -0.0]))[0] == 1.0 and c_oracle.expf(np.float32([0.0, -0.0]))[1] == 1.0


def test_log_accuracy(log_runs):
    worst = (0.0, None)
    for name, x, got in log_runs:
        err = R.log_errors(x, got)
        i = int(err.argmax())
        if err[i] > worst[0]:
            worst = (float(err[i]), float(x[i]))
    print(f"MEASURED shared math host ed_logf: {worst[0]:.4f} ulp at x = {worst[1]!r}")
    assert worst[0] <= R.LOG_BAR_ULP
    assert c_oracle.logf(np.float32([1.0]))[0] == 0.0


def test_noise_accuracy(log_runs):
    """The noise is the float32 composition of its ed_logf term (held to LOG_BAR_ULP here on every uniform), and as a number it is
    within that bar plus the subtraction's own rounding."""
    u = R.uniforms()
    name, arg, term = log_runs[-1]
    assert name == "uniforms + 1e-10f" and np.array_equal(arg, u + R.NOISE_EPS)
    term_err = R.log_errors(arg, term)
    got = R.NOISE_EPS - term
    assert np.array_equal(got.view(np.uint32), R.noise_host(c_oracle.logf, u).view(np.uint32))
    err, allowed = R.noise_errors(u, got)
    print(f"MEASURED shared math host noise: ed_logf term {term_err.max():.4f} ulp at u = {float(u[term_err.argmax()])!r}, largest "
          f"absolute error {np.abs(term.astype(np.float64) - np.log(arg.astype(np.float64))).max():.3g}; noise {err.max():.4f} of the "
          f"term's ulp at u = {float(u[err.argmax()])!r}")
    assert term_err.max() <= R.NOISE_BAR_ULP
    assert (err <= allowed).all()
    assert (got > 0).all() and np.isfinite(got).all()        # the race divides by it
    assert got[0] == R.NOISE_EPS - c_oracle.logf(np.float32([1e-10]))[0] and 23.0 < got[0] < 23.1


def test_monotone(exp_runs, log_runs):
    """Non-decreasing over every run of ascending points (neighbouring floats in all pieces but the strided ones)."""
    for runs in (exp_runs, log_runs):
        for name, x, got in runs:
            breaks = R.monotone_breaks(x, got)
            assert breaks.size == 0, (name, x[breaks][:8])


def test_the_measure_sees_a_one_ulp_flaw(log_runs, exp_runs):
    """Planted: the host's own results moved by one float32 spacing on 1 point in 1000 miss the bars; a swapped neighbour pair is a
    break of monotonicity."""
    name, x, got = log_runs[2]
    bad = got.copy()
    bad[::1000] = np.nextafter(bad[::1000], np.float32(np.inf))
    assert R.log_errors(x, bad).max() > R.LOG_BAR_ULP + 0.1
    name, x, got = exp_runs[2]
    bad = got.copy()
    for _ in range(3):          # exp's bars are above one unit (1.05 ulp; measured + 1 where subnormal): three floats up misses both
        bad[::1000] = np.nextafter(bad[::1000], np.float32(np.inf))
    err, normal, sub = R.exp_errors(x, bad)
    assert err[normal].max() > R.EXP_BAR_ULP + 0.9 and err[sub].max() > R.EXP_SUBNORMAL_BAR + 0.4
    i = int(np.flatnonzero(got[1:] > got[:-1])[0])
    bad = got.copy()
    bad[i], bad[i + 1] = got[i + 1], got[i]
    assert R.monotone_breaks(x, bad).tolist() == [i]


def test_philox_layout_is_the_documented_one():
    """ed_philox_uniform against the layout esmdiff_rng documents, restated in tests/shared_math_ref.py and evaluated through the raw
    Philox4x32-10 (held to the Random123 vectors by tests/test_oracle_golden.py): the oracle and the kernels share ed_philox_uniform
    itself, so only a restatement can see a flaw in it."""
    rs = np.random.RandomState(5)
    cases = [(7, 3, 2, 5), (0x9E3779B900000007, 2 ** 33 + 5, 999, 1279), (1, 2 ** 32 - 1, 0, 0), (1, 2 ** 32, 1, 257)]
    for seed, sample, step, l in cases:
        got = c_oracle.philox_uniforms(seed, sample, step, l, vocab=4353)
        vs = np.concatenate([rs.randint(0, 4101, 60), [0, 3, 4, 4095, 4096, 4100, 4104, 4105, 4352]])
        words = R.philox_words(seed, sample, step, l, vs)
        for v, w in zip(vs.tolist(), words.tolist()):
            out = c_oracle.philox(w[2:6], w[0:2])
            assert got[v] == np.float32((out[w[6]] >> 8) * 2.0 ** -24), (seed, sample, step, l, v)
    # distinct counters across the documented ranges' corners: step < 2^16, sample < 2^48
    grid = [(s, smp, st, l, v) for s in (1, 2 ** 32 + 1) for smp in (0, 1, 2 ** 32, 2 ** 48 - 1) for st in (0, 1, 65535)
            for l in (0, 1) for v in (0, 1, 4, 4352)]
    words = R.philox_words(*[np.array(c, dtype=np.uint64) for c in zip(*grid)])
    assert len({tuple(w) for w in words.tolist()}) == len(grid)

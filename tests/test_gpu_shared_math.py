"""Each unit's device copy of esmdiff_amd/csrc/ed_math.h against the host's, bit for bit (esmdiff_math_eval: the kernel of
csrc/ed_math_eval.inc instantiated inside sampler.hip, score.hip and gibbs.hip, each under its own flags).

That equality is the premise of every bit-exact sampler test; the other tests only infer it from ids, where an arg-max hides a
last-bit difference everywhere but at a near-tie.  Here it is asserted on the whole point set of tests/shared_math_ref.py (every
float of each domain at an odd stride, binade ends, reduction boundaries, the sqrt 2 switch in every binade, the thresholds, every
float of exp's subnormal branch, all 2^24 uniforms) and on the Philox counter layout; the accuracy bars of
tests/test_shared_math_cpu.py are asserted once on the device's own output as well."""
import numpy as np
import pytest
import torch

from oracle import c_oracle
from tests import shared_math_ref as R

pytestmark = pytest.mark.gpu

UNITS = ["sampler", "score", "gibbs"]


@pytest.fixture(scope="module")
def host():
    """kind -> (input f32, the C oracle's output f32) on the whole point set, computed once."""
    x, xl, u = R.points(R.exp_pieces()), R.points(R.log_pieces()), R.uniforms()
    return {"exp": (x, c_oracle.expf(x)), "log": (xl, c_oracle.logf(xl)), "noise": (u, R.noise_host(c_oracle.logf, u))}


def _device(unit, kind, x):
    from esmdiff_amd.engine import math_eval
    out = math_eval(unit, kind, torch.from_numpy(x).cuda())
    return out.cpu().numpy()


@pytest.mark.parametrize("kind", ["exp", "log", "noise"])
@pytest.mark.parametrize("unit", UNITS)
def test_device_bits_equal_the_host(host, unit, kind):
    x, want = host[kind]
    got = _device(unit, kind, x)
    diff = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))      # NaN payloads included
    print(f"MEASURED shared math {unit}.hip {kind}: {x.size} points, {diff.size} differ from the host")
    assert diff.size == 0, [(float(x[i]), float(got[i]), float(want[i])) for i in diff[:8]]


@pytest.mark.parametrize("unit", UNITS)
def test_device_accuracy_against_float64(host, unit):
    """By the equality above the host's bars hold on the device; asserted on the device's own output anyway: ed_logf and the noise on
    all 2^24 uniforms, ed_expf on its whole point set (the uniforms are not arguments of exp)."""
    u = R.uniforms()
    term = _device(unit, "log", u + R.NOISE_EPS)
    term_err = R.log_errors(u + R.NOISE_EPS, term)
    noise = _device(unit, "noise", u)
    nerr, allowed = R.noise_errors(u, noise)
    x = host["exp"][0]
    e = _device(unit, "exp", x)
    err, normal, sub = R.exp_errors(x, e)
    print(f"MEASURED shared math {unit}.hip against float64: ed_logf(u + 1e-10f) {term_err.max():.4f} ulp, noise {nerr.max():.4f} of the "
          f"term's ulp, ed_expf {err[normal].max():.4f} ulp on normal results, {err[sub].max():.4f} units of 2^-149 on subnormal ones")
    assert term_err.max() <= R.LOG_BAR_ULP
    assert np.array_equal(noise.view(np.uint32), (R.NOISE_EPS - term).view(np.uint32)) and (nerr <= allowed).all()
    assert err[normal].max() <= R.EXP_BAR_ULP and err[sub].max() <= R.EXP_SUBNORMAL_BAR
    assert R.exp_ends_ok(x, e)
    assert R.monotone_breaks(u + R.NOISE_EPS, term).size == 0


# ---- the Philox counter layout ----------------------------------------------------------------------------------------------------
PHILOX_V = list(range(4101)) + [4104, 4105, 4352]          # the drawn columns and the reserved ones (esmdiff_hip.h)
PHILOX_L = [0, 1, 257, 1279]
PHILOX_STEP = [0, 1, 999]
PHILOX_SAMPLE = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 33 + 5]
PHILOX_SEED = [0x0000000500000007, 0x9E3779B900000007]     # distinct high words, equal low words


@pytest.fixture(scope="module")
def philox_records():
    from esmdiff_amd import _native as N
    rows = [(seed, sample, step, l) for seed in PHILOX_SEED for sample in PHILOX_SAMPLE for step in PHILOX_STEP for l in PHILOX_L]
    rec = np.zeros((len(rows), len(PHILOX_V)), dtype=N.MATH_EVAL_PHILOX_DTYPE)
    want = np.empty((len(rows), len(PHILOX_V)), dtype=np.float32)
    for i, (seed, sample, step, l) in enumerate(rows):
        rec["seed"][i], rec["sample"][i], rec["step"][i], rec["l"][i], rec["v"][i] = seed, sample, step, l, PHILOX_V
        want[i] = c_oracle.philox_uniforms(seed, sample, step, l, vocab=4353)[PHILOX_V]
    assert rec.dtype.itemsize == 32
    return rec.reshape(-1), want.reshape(-1)


@pytest.mark.parametrize("unit", UNITS)
def test_philox_uniforms_equal_the_host(philox_records, unit):
    from esmdiff_amd.engine import math_eval
    rec, want = philox_records
    got = math_eval(unit, "philox", torch.from_numpy(rec.view(np.uint8).reshape(-1, 32)).cuda()).cpu().numpy()
    assert got.shape == want.shape
    diff = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    print(f"MEASURED shared math {unit}.hip philox: {want.size} records, {diff.size} differ from the host; mean {got.mean():.5f}")
    assert diff.size == 0, [(rec[i].tolist(), float(got[i]), float(want[i])) for i in diff[:8]]
    assert got.min() >= 0.0 and got.max() < 1.0


def test_philox_counters_are_pairwise_distinct(philox_records):
    """No two of the records share (key, counter, lane): esmdiff_rng's layout sends each (seed, sample, step, l, v) within its
    documented ranges (step < 2^16, sample < 2^48) to its own Philox output word."""
    rec, _ = philox_records
    words = R.philox_words(rec["seed"], rec["sample"], rec["step"], rec["l"], rec["v"])
    assert len({tuple(w) for w in words.tolist()}) == rec.size


def test_refusals():
    """Every argument is checked before the first HIP call: ESMDIFF_E_INVALID, output untouched."""
    import ctypes
    from esmdiff_amd import _native as N
    lib = N.lib()
    x = torch.ones(8, device="cuda")
    out = torch.full((8,), -7.0, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for unit, kind, a, b, n in ((3, 0, x, out, 8), (-1, 0, x, out, 8), (0, 4, x, out, 8), (0, -1, x, out, 8), (0, 0, x, out, -1)):
        assert lib.esmdiff_math_eval(unit, kind, p(a), p(b), n, None) == -1
    assert lib.esmdiff_math_eval(0, 0, None, p(out), 8, None) == -1 and lib.esmdiff_math_eval(0, 0, p(x), None, 8, None) == -1
    assert lib.esmdiff_math_eval(0, 0, p(x), p(out), 0, None) == 0
    torch.cuda.synchronize()
    assert (out == -7.0).all()

"""Point sets and the error measure for the shared math of esmdiff_amd/csrc/ed_math.h (ed_expf, ed_logf, the race's noise
1e-10f - ed_logf(u + 1e-10f)), in plain numpy.  Used by tests/test_shared_math_cpu.py on the C oracle, by tests/test_gpu_shared_math.py
on each unit's device copy, and by tools/shared_math_sweep.py for the exhaustive sweep.

Floats are walked through their ORDINAL: a signed integer that grows with the float (the bit pattern for x >= 0, minus the magnitude
bits for x < 0), so that ordinal + 1 is the next float up and "every float at a stride" is an arange.

Error measure (EXPERIMENTS.md, "Shared math"): |got - want64| / spacing(float32(want64)), want64 the float64 libm value of the
float32 input; where exp's correctly rounded result is subnormal the unit is 2^-149 instead.
"""
from __future__ import annotations

import functools

import numpy as np

F32 = np.float32
LN2 = float(np.log(2.0))

# ---- domains and thresholds of ed_math.h ----------------------------------------------------------------------------------------
EXP_LO = F32(-104.0)                  # below: 0
EXP_HI = F32(88.72283)                # above: +inf
EXP_SUBNORMAL_BELOW = F32(-126.0 * LN2)   # -87.33655: exp(x) < 2^-126 below it
EXP_TOP_BRANCH = F32(127.5 * LN2)     # 88.376: n = rint(x log2 e) > 127 above it
LOG_LO, LOG_HI = F32(1e-10), F32(8192.0)
SQRT2 = F32(1.41421356237)            # the m > sqrt 2 switch of ed_logf
NOISE_EPS = F32(1e-10)

# bars (the issue's exhaustive host maxima, rounded up with room for the measure's own rounding only; EXPERIMENTS.md)
EXP_BAR_ULP = 1.05
LOG_BAR_ULP = 0.85
NOISE_BAR_ULP = 0.85                  # of the noise's ed_logf term, in that term's ulps (noise_errors)
EXP_SUBNORMAL_MEASURED = 0.7504       # units of 2^-149, exhaustive on the host over every float of [-104, -87.33655): EXPERIMENTS.md
EXP_SUBNORMAL_BAR = EXP_SUBNORMAL_MEASURED + 1.0

EXP_STRIDE = 131                      # odd: co-prime to 2^23.  2.24e9 floats of [-104, 88.72283] -> 1.7e7 points
LOG_STRIDE = 97                       # 3.9e8 floats of [1e-10, 8192] -> 4.0e6 points (+ the 2^24 uniforms)


def ordinal(x) -> np.ndarray:
    b = np.asarray(x, dtype=F32).view(np.int32).astype(np.int64)
    return np.where(b >= 0, b, -(b & 0x7FFFFFFF))


def from_ordinal(o) -> np.ndarray:
    o = np.asarray(o, dtype=np.int64)
    b = np.where(o >= 0, o, (-o) | 0x80000000).astype(np.uint32)
    return b.view(F32)


def uniforms() -> np.ndarray:
    """All 2^24 values ed_u32_to_uniform can return: k 2^-24, ascending."""
    return (np.arange(1 << 24, dtype=np.float64) * 2.0 ** -24).astype(F32)


def _around(centres, half) -> np.ndarray:
    c = ordinal(np.asarray(centres, dtype=F32)).reshape(-1, 1)
    return (c + np.arange(-half, half + 1, dtype=np.int64)[None, :]).reshape(-1)


def _binade_ends(lo_ord: int, hi_ord: int, n: int = 4096) -> np.ndarray:
    """Ordinals of the first and last n floats of every binade (subnormals: exponent field 0) that meets [lo_ord, hi_ord], both signs."""
    first = (np.arange(0, 255, dtype=np.int64) << 23).reshape(-1, 1)
    k = np.arange(n, dtype=np.int64)[None, :]
    pos = np.concatenate([(first + k).reshape(-1), (first + 0x7FFFFF - k).reshape(-1)])
    o = np.concatenate([pos, -pos])
    return o[(o >= lo_ord) & (o <= hi_ord)]


def _runs(o: np.ndarray, lo_ord: int, hi_ord: int) -> np.ndarray:
    o = np.unique(o)
    return o[(o >= lo_ord) & (o <= hi_ord)]


@functools.lru_cache(None)
def exp_pieces():
    """[(name, x f32 ascending)] for ed_expf: domain [-104, 88.72283] and 64 floats beyond each end."""
    lo, hi = int(ordinal(EXP_LO)) - 64, int(ordinal(EXP_HI)) + 64
    k = np.arange(-150, 129, dtype=np.float64)
    pieces = [
        ("stride", np.arange(lo, hi + 1, EXP_STRIDE, dtype=np.int64)),
        ("binade ends", _runs(_binade_ends(lo, hi), lo, hi)),
        ("reduction boundaries", _runs(_around(((k + 0.5) * LN2).astype(F32), 64), lo, hi)),
        ("thresholds", _runs(_around([EXP_LO, EXP_SUBNORMAL_BELOW, EXP_TOP_BRANCH, EXP_HI, 0.0], 64), lo, hi)),
        # the subnormal branch is small enough to take whole: every float of [-104, -87.33655]
        ("subnormal results", np.arange(int(ordinal(EXP_LO)), int(ordinal(EXP_SUBNORMAL_BELOW)) + 1, dtype=np.int64)),
    ]
    return [(n, from_ordinal(o)) for n, o in pieces]


@functools.lru_cache(None)
def log_pieces():
    """[(name, x f32 ascending)] for ed_logf: domain [1e-10, 8192] and the arguments u + 1e-10f of the race's noise."""
    lo, hi = int(ordinal(LOG_LO)), int(ordinal(LOG_HI))
    e = np.arange(-34, 13, dtype=np.float64)              # 2^-34 <= 1e-10, 2^12 the last binade below 8192
    pieces = [
        ("stride", np.arange(lo, hi + 1, LOG_STRIDE, dtype=np.int64)),
        ("binade ends", _runs(_binade_ends(lo, hi), lo, hi)),
        ("sqrt 2 switch", _runs(_around((float(SQRT2) * 2.0 ** e).astype(F32), 4096), lo, hi)),
        ("thresholds", _runs(_around([LOG_LO, 1.0, LOG_HI], 64), lo, hi)),
    ]
    return [(n, from_ordinal(o)) for n, o in pieces] + [("uniforms + 1e-10f", uniforms() + NOISE_EPS)]


def noise_pieces():
    """[(name, u f32 ascending)] for the race's noise: every uniform."""
    return [("uniforms", uniforms())]


def points(pieces) -> np.ndarray:
    return np.concatenate([x for _, x in pieces])


# ---- the measure ------------------------------------------------------------------------------------------------------------------
def ulp_error(got: np.ndarray, want64: np.ndarray) -> np.ndarray:
    """|got - want64| in units of the float32 spacing at the correctly rounded result (finite arguments)."""
    unit = np.spacing(np.abs(want64).astype(F32)).astype(np.float64)
    return np.abs(got.astype(np.float64) - want64) / unit


def exp_errors(x: np.ndarray, got: np.ndarray):
    """(err, normal, subnormal) over x in [-104, 88.72283]: err in ulps where float32(exp(x)) is normal, in units of 2^-149 where it
    is not; the two masks say which.  Points outside the domain are in neither mask (exp_ends_ok holds them)."""
    want = np.exp(x.astype(np.float64))
    inside = (x >= EXP_LO) & (x <= EXP_HI)
    normal = inside & (want >= 2.0 ** -126 * (1 - 2.0 ** -25))         # float32(exp(x)) is normal
    sub = inside & ~normal
    err = np.zeros(x.shape, dtype=np.float64)
    err[normal] = ulp_error(got[normal], want[normal])
    err[sub] = np.abs(got[sub].astype(np.float64) - want[sub]) / 2.0 ** -149
    return err, normal, sub


def exp_ends_ok(x: np.ndarray, got: np.ndarray) -> bool:
    """Beyond the domain: exactly 0 below -104, exactly +inf above 88.72283."""
    below, above = x < EXP_LO, x > EXP_HI
    return bool(below.any() and above.any() and (got[below].view(np.uint32) == 0).all() and np.isposinf(got[above]).all())


def log_errors(x: np.ndarray, got: np.ndarray) -> np.ndarray:
    return ulp_error(got, np.log(x.astype(np.float64)))


def noise_host(logf, u: np.ndarray) -> np.ndarray:
    """1e-10f - logf(u + 1e-10f) composed in float32, as the kernels and the oracle write it."""
    return NOISE_EPS - logf(u + NOISE_EPS)


def noise_errors(u: np.ndarray, got: np.ndarray):
    """(err, allowed) of the noise g = fl(1e-10f - L), L = ed_logf(u + 1e-10f), against 1e-10 - log(u + 1e-10f) in float64 of the
    SAME float32 argument, both in units of the spacing at the ed_logf term.  The bar of the term itself is LOG_BAR_ULP and is
    asserted on the term (the piece "uniforms + 1e-10f" of log_pieces; the noise is held to be that term's float32 composition bit
    for bit).  The noise as a number carries one rounding more, the subtraction's, of at most half a spacing of g: allowed =
    LOG_BAR_ULP + spacing(g) / (2 spacing(term)), point by point.  Measured on the host: 0.9825 at u = 0.99994224."""
    want_log = np.log((u + NOISE_EPS).astype(np.float64))
    unit = np.spacing(np.abs(want_log).astype(F32)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - (float(NOISE_EPS) - want_log)) / unit
    return err, NOISE_BAR_ULP + 0.5 * np.spacing(np.abs(got)).astype(np.float64) / unit


def monotone_breaks(x: np.ndarray, got: np.ndarray) -> np.ndarray:
    """Indices i of an ascending x with got[i + 1] < got[i]."""
    assert (np.diff(ordinal(x)) > 0).all()
    return np.flatnonzero(got[1:] < got[:-1])


# ---- the Philox counter layout of esmdiff_rng (include/esmdiff_hip.h), restated --------------------------------------------------
def philox_words(seed, sample, step, l, v) -> np.ndarray:
    """u64 [n, 7] = (key0, key1, counter0 .. counter3, lane) of each record: key = the seed's two words, counter = (v >> 2, l, the
    sample's low word, step ^ (the sample's high word << 16)), and the uniform is output word `lane` = v & 3 of Philox4x32-10,
    >> 8, times 2^-24."""
    seed, sample, step, l, v = np.broadcast_arrays(*[np.asarray(a, dtype=np.uint64) for a in (seed, sample, step, l, v)])
    m32 = np.uint64(0xFFFFFFFF)
    c3 = (step ^ ((sample >> np.uint64(32)) << np.uint64(16))) & m32
    return np.stack([seed & m32, seed >> np.uint64(32), v >> np.uint64(2), l, sample & m32, c3, v & np.uint64(3)], axis=-1)

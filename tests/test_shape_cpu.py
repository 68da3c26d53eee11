"""The numpy restatement tests/shape_ref.py against hand-worked cases and the reference's own radius of gyration, and the host-only
functions of esmdiff_amd/shape.py (Guinier fit, chi^2, the sphere's form factor) against closed forms.  No device."""
import math
import re
from pathlib import Path

import numpy as np

from tests import shape_ref as R

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = np.load(ROOT / "tests" / "golden" / "g9_metrics.npz")


def test_rod_of_three_collinear_atoms():
    x = np.array([[[0.0, 0.0, 0.0], [0.0, 0.0, 3.0], [0.0, 0.0, 6.0]]])
    count, desc, hist = R.frames(x, None, 1.5, 4)
    assert count.tolist() == [3] and desc[0, :3].tolist() == [0.0, 0.0, 3.0]
    assert desc[0, 3:9].tolist() == [0.0, 0.0, 18.0, 0.0, 0.0, 0.0]
    assert desc[0, 9] == (1.0 / 3.0 + 1.0 / 6.0) + 1.0 / 3.0 and desc[0, 10] == 6.0 and desc[0, 11] == 6.0
    assert hist.tolist() == [0, 0, 2, 0, 1]                           # 3 / 1.5 = 2, 6 / 1.5 = 4 = bins: the overflow cell
    d = R.derived(count, desc)
    assert d["eigenvalues"][0].tolist() == [0.0, 0.0, 6.0] and d["anisotropy"][0] == 1.0 and d["rg"][0] == math.sqrt(6.0)
    assert d["asphericity"][0] == 6.0 and d["acylindricity"][0] == 0.0 and d["dmax"][0] == 6.0 and d["ree"][0] == 6.0
    assert abs(d["rh"][0] - 9.0 / (2.0 * (5.0 / 6.0))) < 1e-14        # N^2 / (2 (1/3 + 1/3 + 1/6)) = 5.4


def test_regular_tetrahedron():
    x = np.array([[[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]]])
    count, desc, hist = R.frames(x, None, 1.0, 3)
    edge = math.sqrt(8.0)
    assert count.tolist() == [4] and desc[0, :9].tolist() == [0.0, 0.0, 0.0, 4.0, 4.0, 4.0, 0.0, 0.0, 0.0]
    assert desc[0, 10] == edge and desc[0, 11] == edge and hist.tolist() == [0, 0, 6, 0]
    assert abs(desc[0, 9] - 6.0 / edge) < 1e-15
    d = R.derived(count, desc)
    assert d["anisotropy"][0] == 0.0 and d["asphericity"][0] == 0.0 and d["rg"][0] == math.sqrt(3.0)
    assert abs(d["rh"][0] - 16.0 / (12.0 / edge)) < 1e-14
    I, E = R.debye(x, [0.0, 0.3])
    assert I[0, 0] == 16.0 and abs(I[0, 1] - (4.0 + 12.0 * math.sin(0.3 * edge) / (0.3 * edge))) < 1e-14 and E[0, 0] == 16.0


def test_two_atoms_and_the_edge_cases():
    d = 3.8
    x = np.array([[[0.0, 0.0, 0.0], [d, 0.0, 0.0]]])
    q = np.array([0.0, 0.1, 0.5, 2.0])
    I, E = R.debye(x, q)
    want = [2.0 + 2.0 * (1.0 if v == 0 else math.sin(v * d) / (v * d)) for v in q]
    assert np.abs(I[0] - want).max() < 1e-15 and I[0, 0] == 4.0
    assert np.array_equal(E[0], [4.0, 4.0, 2.0 + 2.0 * min(1.0, 1.0 / (0.5 * d)), 2.0 + 2.0 / (2.0 * d)])
    f = np.array([[2.0] * 4, [3.0] * 4])
    assert np.abs(R.debye(x, q, f)[0][0] - [13.0 + 12.0 * (w - 2.0) / 2.0 for w in want]).max() < 1e-14
    # coincident atoms: s(0) = 1, nothing is NaN; a masked residue and a NaN coordinate are the same thing; no residue at all
    same = np.zeros((1, 2, 3))
    assert R.debye(same, q)[0].tolist() == [[4.0] * 4]
    y = np.array([[[0.0, 0.0, 0.0], [d, 0.0, 0.0], [np.nan, 1.0, 1.0]], [[0.0, 0.0, 0.0], [d, 0.0, 0.0], [7.0, 1.0, 1.0]]])
    mask = np.array([[1, 1, 1], [1, 1, 0]], bool)
    count, desc, hist = R.frames(y, mask, 1.0, 5)
    assert count.tolist() == [2, 2] and np.array_equal(desc[0], desc[1], equal_nan=True) and np.isnan(desc[0, 11])
    assert desc[0, 10] == d and hist.tolist() == [0, 0, 0, 2, 0, 0]
    assert np.array_equal(*R.debye(y, q, None, mask)[0])
    count, desc, _ = R.frames(y, np.zeros((2, 3), bool))
    assert count.tolist() == [0, 0] and np.isnan(desc[0, :3]).all() and desc[0, 3:11].tolist() == [0.0] * 8 and np.isnan(desc[0, 11])
    count, desc, _ = R.frames(y[1:], np.array([[0, 1, 0]], bool))      # one valid residue
    assert count.tolist() == [1] and desc[0, :3].tolist() == [d, 0.0, 0.0] and desc[0, 3:11].tolist() == [0.0] * 8
    dd = R.derived(count, desc)
    assert dd["rg"][0] == 0.0 and np.isnan(dd["rh"][0]) and np.isnan(dd["dmax"][0]) and np.isnan(dd["anisotropy"][0])
    assert R.debye(y[1:], q, None, np.array([[0, 1, 0]], bool))[0].tolist() == [[1.0] * 4]


def test_the_published_orders_are_followed():
    """Against plain sums: equal to rounding, and for sums of integers — exact whatever the order — exactly; one and eight waves."""
    rng = np.random.default_rng(3)
    for L in (64, 128, 129, 200):
        ok = rng.random(L) > 0.1
        t = rng.integers(1, 50, (L, L)).astype(np.float64)
        both = ok[:, None] & ok[None, :]
        assert R.pair_sum(t, ok) == np.triu(np.where(both, t, 0.0), 1).sum()
        assert R.residue_sum(t[0], ok) == t[0][ok].sum()
        u = rng.random((L, L))
        assert abs(R.pair_sum(u, ok) - math.fsum(np.triu(np.where(both, u, 0.0), 1).ravel())) < 1e-11
    assert R.waves(128) == 1 and R.waves(129) == 8
    # the order is not the plain one: the bits differ somewhere
    u = rng.random((200, 200))
    ok = np.ones(200, bool)
    assert any(R.pair_sum(u * s, ok) != np.triu(u * s, 1).sum() for s in (1.0, 3.0, 7.0))


def test_rg_equals_the_reference():
    count, desc, _ = R.frames(GOLDEN["ca_target"])
    rg = R.derived(count, desc)["rg"]
    assert np.abs(rg / GOLDEN["rg_target"] - 1.0).max() <= 1e-12


def test_envelope_and_restatement_against_long_double():
    """The restatement's own error: within 1e-15 E of an evaluation in numpy's long double (the issue's derivation found 2e-16 E with
    an 80-bit long double; where long double is float64 the comparison is only between two orders of summation)."""
    rng = np.random.default_rng(5)
    q = np.linspace(0.0, 0.5, 6)
    for L in (3, 65, 130):
        x = R.chain(rng, L)[None]
        I, E = R.debye(x, q)
        a, b = np.triu_indices(L, 1)
        d = np.sqrt(((x[0][b].astype(np.longdouble) - x[0][a].astype(np.longdouble)) ** 2).sum(-1))
        for k, v in enumerate(q):
            xs = np.longdouble(v) * d
            s = np.where(xs == 0, np.longdouble(1), np.sin(xs) / np.where(xs == 0, 1, xs))
            assert abs(float(np.longdouble(L) + 2 * s.sum()) - I[0, k]) <= 1e-15 * E[0, k]
        assert (np.abs(I) <= E).all() and E[0, 0] == L * L


def test_guinier_fit_on_the_exact_curve():
    from esmdiff_amd import shape
    q = np.linspace(0.0, 0.2, 41)
    for rg, i0 in ((14.3, 1.0), (25.0, 3456.0)):
        fit = shape.guinier_rg(q, i0 * np.exp(-q * q * rg * rg / 3.0))
        assert abs(fit["rg"] / rg - 1.0) < 1e-12 and abs(fit["i0"] / i0 - 1.0) < 1e-12
        assert fit["q_max"] * rg <= 1.3 < (fit["q_max"] + 0.005) * rg and fit["n_points"] == int(1.3 / rg / 0.005 + 1e-9) + 1
    assert np.isnan(shape.guinier_rg(q[:2], np.ones(2))["rg"]) and np.isnan(shape.guinier_rg(q, np.ones(41))["rg"])
    x, y = shape.kratky(q, np.exp(-q * q * 100.0 / 3.0), rg=10.0)
    assert np.array_equal(x, q * 10.0) and abs(y[20] - (q[20] * 10.0) ** 2 * math.exp(-q[20] ** 2 * 100.0 / 3.0)) < 1e-15
    assert np.array_equal(shape.kratky(q, np.full(41, 2.0))[1], 2.0 * q * q)


def test_chi2_recovers_the_scale():
    from esmdiff_amd import shape
    rng = np.random.default_rng(9)
    q = np.linspace(0.01, 0.5, 30)
    calc = np.exp(-q * q * 50.0) + 0.05
    sigma = 0.01 + 0.02 * rng.random(30)
    r = shape.chi2(calc, q, 7.5 * calc, sigma)
    assert r["chi2"] < 1e-25 and abs(r["scale"] - 7.5) < 1e-12 and r["constant"] == 0.0
    r = shape.chi2(calc, q, 7.5 * calc + 0.3, sigma, fit_constant=True)
    assert r["chi2"] < 1e-20 and abs(r["scale"] - 7.5) < 1e-9 and abs(r["constant"] - 0.3) < 1e-9
    rows = np.stack([calc + 0.1 * q, calc, calc * calc])
    r = shape.chi2(rows, q, 2.0 * calc, sigma)
    assert r["best"] == 1 and r["chi2"].shape == (3,) and r["chi2"][1] < 1e-25 and r["chi2"][0] > 1.0
    one = shape.chi2(rows[0], q, 2.0 * calc, sigma)                    # a row alone: the same numbers, and the definition
    c = one["scale"]
    assert one["chi2"] == r["chi2"][0] and abs(one["chi2"] - (((c * rows[0] - 2.0 * calc) / sigma) ** 2).sum() / 29) < 1e-12 * one["chi2"]


def test_sphere_form_factor_against_its_series():
    from esmdiff_amd import shape
    x = np.concatenate([[0.0], np.logspace(-8, 0, 200)])
    got = shape.sphere_form_factor(x / 2.5, 2.5)
    assert got[0] == 1.0 and np.abs(got - R.sphere_series(x)).max() < 2e-15
    assert abs(shape.sphere_form_factor(np.array([4.493409457909064 / 3.0]), 3.0)[0]) < 1e-15      # the first zero: tan x = x


def test_both_entries_are_declared_and_exported():
    from esmdiff_amd import _native as N
    header = (ROOT / "include" / "esmdiff_hip.h").read_text()
    for name in ("esmdiff_shape_frames", "esmdiff_debye_frames"):
        assert name in N.EXPORTS and re.search(r"\bint %s\s*\(" % name, header)
    for macro, value in (("ESMDIFF_SHAPE_MAX_L", N.SHAPE_MAX_L), ("ESMDIFF_SHAPE_MAX_BINS", N.SHAPE_MAX_BINS),
                         ("ESMDIFF_DEBYE_MAX_Q", N.DEBYE_MAX_Q), ("ESMDIFF_DEBYE_Q_CHUNK", N.DEBYE_Q_CHUNK)):
        assert re.search(r"#define %s %d\b" % (macro, value), header)
    assert (R.MAX_L, R.MAX_BINS, R.MAX_Q, R.Q_CHUNK) == (N.SHAPE_MAX_L, N.SHAPE_MAX_BINS, N.DEBYE_MAX_Q, N.DEBYE_Q_CHUNK)
    assert all(N.shape_waves(L) == R.waves(L) for L in (1, 64, 128, 129, 4096))
    assert "((L) <= 128 ? 1 : 8)" in header

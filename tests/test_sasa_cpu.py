"""The numpy restatement tests/sasa_ref.py against hand-worked cases, the host-only functions of esmdiff_amd/accessibility.py (the sphere
points, the areas, the mutual information) against closed forms, and the declarations of the two entries of csrc/sasa.hip.  No device."""
import json
import math
import re
from pathlib import Path

import numpy as np
import pytest

from tests import sasa_ref as R

ROOT = Path(__file__).resolve().parent.parent


def _counts(centres, radii, P):
    c = np.asarray(centres, np.float64)
    return R.frame_counts(c, np.asarray(radii, np.float64), np.ones(len(c), bool), R.sphere_points(P)).tolist()


def test_one_atom_and_two_far_apart_expose_every_point():
    for P in (1, 63, 96):
        assert _counts([[1.0, -2.0, 3.0]], [3.27], P) == [P]
        assert _counts([[0.0, 0.0, 0.0], [100.0, 0.0, 0.0]], [3.0, 3.0], P) == [P, P]


def test_a_small_atom_inside_a_large_one():
    assert _counts([[0.1, 0.0, 0.0], [0.0, 0.0, 0.0]], [1.0, 10.0], 96) == [0, 96]


def test_two_overlapping_spheres_against_the_cap_formula():
    P, Rr, d = 96, 3.0, 2.5
    u = R.sphere_points(P)
    lower = int((Rr * u[:, 2] < d / 2.0).sum())                          # the points of the lower sphere below the plane of intersection
    assert lower == 68 == P * (1.0 + d / (2.0 * Rr)) / 2.0
    assert _counts([[0.0, 0.0, 0.0], [0.0, 0.0, d]], [Rr, Rr], P) == [68, 68]
    z = np.sort(Rr * u[:, 2])
    assert z[67] < d / 2.0 - 0.01 and z[68] > d / 2.0 + 0.01            # the boundary lies between two z levels: rounding cannot move it


def test_an_atom_is_not_its_own_neighbour_and_an_absent_one_buries_nothing():
    u = R.sphere_points(96)
    c = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 2.5], [0.0, 0.0, 1.0]])
    got = R.frame_counts(c, np.array([3.0, 3.0, 50.0]), np.array([True, True, False]), u)
    assert got.tolist() == [68, 68, -1]
    X = c[None, :, None, :].copy()                                       # (1, 3, 1, 3): three CA-only residues
    radii = np.array([[3.0], [3.0], [50.0]])
    out = R.frames(X, np.array([[1, 1, 0]], bool), radii, u, 0.5)
    assert out["count"][0, :, 0].tolist() == [68, 68, -1] and out["exposed"].tolist() == [[1, 1, 2]]
    assert out["valid"][:, 0].tolist() == [1, 1, 0] and out["sum_count"][:, 0].tolist() == [68, 68, 0]
    assert out["exposed_count"].tolist() == [1, 1, 0] and out["present_count"].tolist() == [1, 1, 0]
    X[0, 2, 0, 1] = np.nan                                               # a NaN coordinate is the same thing as the mask
    assert all(np.array_equal(a, b) for a, b in zip(R.frames(X, None, radii, u, 0.5).values(), out.values()))
    assert R.frames(X, None, radii, u, 68.0 / 96.0)["exposed"].tolist() == [[0, 0, 2]]      # the comparison is strict


def test_coincident_atoms_are_not_a_trivial_case():
    got = _counts(np.tile([1.3, -2.7, 0.9], (6, 1)), np.full(6, 3.27), 96)
    assert len(set(got)) == 1 and 0 < got[0] < 96                        # points on each other's spheres: rounding decides


def test_sphere_points_and_the_isolated_area():
    from esmdiff_amd import accessibility as acc
    for P in (1, 2, 63, 96, 1024):
        u = acc.sphere_points(P)
        assert np.array_equal(u, R.sphere_points(P)) and u.shape == (P, 3)
        assert np.abs(np.linalg.norm(u, axis=1) - 1.0).max() <= 2.0 ** -52 and abs(u.sum(0)[2]) < 1e-12
    for bad in (0, 1025):
        with pytest.raises(ValueError):
            acc.sphere_points(bad)
    for radius in (1.4, 3.27, 10.0):
        for P in (1, 63, 96):
            area = acc.atom_area(np.float64(radius), P, P)
            assert area == R.atom_area(np.float64(radius), P, P) and abs(area - 4.0 * math.pi * radius ** 2) <= np.spacing(area)
    a = acc.Accessibility(np.array([[[96, 48, -1, 0], [-1, -1, -1, -1]]], np.int32), np.tile(np.add(acc.DEFAULT_RADII, 1.4), (2, 1)), 96, 1.4)
    full = [4.0 * math.pi * (r + 1.4) ** 2 for r in acc.DEFAULT_RADII]
    assert abs(a.residue_area()[0, 0] - (full[0] + 0.5 * full[1])) < 1e-12 and np.isnan(a.residue_area()[0, 1])
    assert abs(a.relative()[0, 0] - (full[0] + 0.5 * full[1]) / (full[0] + full[1] + full[3])) < 1e-15
    assert a.exposed(0.2).tolist() == [[1, 2]] and a.total()[0] == a.residue_area()[0, 0] and np.isnan(a.atom_area()[0, 0, 2])
    ref = R.areas(a.counts, a.radii, 96)
    for got, want in zip((a.atom_area(), a.residue_area(), a.relative(), a.total()), ref):
        assert np.array_equal(got, want, equal_nan=True)


def test_radii_are_a_parameter():
    from esmdiff_amd import accessibility as acc
    assert np.array_equal(acc.expanded_radii(None, 1.4, 3, 4), np.tile(np.add(acc.DEFAULT_RADII, 1.4), (3, 1)))
    with pytest.raises(ValueError, match="no default radius"):
        acc.expanded_radii(None, 1.4, 3, 1)
    assert np.array_equal(acc.expanded_radii(2.0, 1.0, 3, 1), np.full((3, 1), 3.0))
    per = np.arange(1.0, 13.0).reshape(3, 4)
    assert np.array_equal(acc.expanded_radii(per, 0.0, 3, 4), per) and np.array_equal(acc.expanded_radii(per[0], 0.5, 2, 4), np.tile(per[0] + 0.5, (2, 1)))
    for bad in (np.ones(3), np.ones((2, 4)), -1.0, np.nan):
        with pytest.raises(ValueError):
            acc.expanded_radii(bad, 1.4, 3, 4)
    with pytest.raises(ValueError):
        acc.expanded_radii(None, -0.1, 3, 4)
    x = np.zeros((5, 7, 3))
    assert acc.atom_array(x).shape == (5, 7, 1, 3) and acc.atom_array(np.zeros((7, 4, 3))).shape == (1, 7, 4, 3)
    three = acc.atom_array(R.coil(np.random.default_rng(0), 6, 3))
    assert three.shape == (1, 6, 4, 3) and np.isnan(three[0, -1, 3]).all() and np.isfinite(three[0, :-1]).all()


def test_cooccurrence_of_a_table_written_out_by_hand():
    flags = np.array([[1, 0, 1],
                      [1, 1, 2],
                      [0, 1, 0],
                      [2, 1, 1],
                      [1, 0, 0]], np.uint8)
    both, a_one, both_one = R.cooccurrence(flags)
    assert both.tolist() == [[4, 4, 3], [4, 5, 4], [3, 4, 4]]
    assert a_one.tolist() == [[3, 3, 2], [2, 3, 2], [1, 2, 2]]
    assert both_one.tolist() == [[3, 1, 1], [1, 3, 1], [1, 1, 2]]
    assert R.cooccurrence(np.zeros((0, 3), np.uint8)).tolist() == np.zeros((3, 3, 3), int).tolist()


def test_mutual_information():
    from esmdiff_amd import accessibility as acc
    a = np.array([0, 0, 1, 1] * 4, np.uint8)
    b = np.array([0, 1] * 8, np.uint8)
    never = np.full(16, 2, np.uint8)
    mi = acc.mutual_information(R.cooccurrence(np.stack([a, b, a, 1 - a, never], axis=1)))
    assert mi[0, 1] == 0.0 and mi[1, 0] == 0.0                           # independent columns
    assert abs(mi[0, 2] - math.log(2.0)) < 1e-15 and abs(mi[0, 3] - math.log(2.0)) < 1e-15 and abs(mi[0, 0] - math.log(2.0)) < 1e-15
    assert (mi[4] == 0.0).all() and (mi[:, 4] == 0.0).all() and np.array_equal(mi, mi.T)     # never jointly defined: 0
    half = np.array([0, 0, 1, 1, 2, 2, 2, 2] * 2, np.uint8)              # defined in half of the frames only
    assert abs(acc.mutual_information(R.cooccurrence(np.stack([half, half], axis=1)))[0, 1] - math.log(2.0)) < 1e-15


def test_both_entries_are_declared_and_exported():
    from esmdiff_amd import _native as N
    from esmdiff_amd import build
    header = (ROOT / "include" / "esmdiff_hip.h").read_text()
    flat = re.sub(r"\s+", " ", header)
    assert ("int esmdiff_sasa_frames(const double* X, int32_t n, int32_t L, int32_t A, const uint8_t* mask, const double* radii, "
            "const double* points, int32_t P, double threshold, int32_t* count, int64_t* sum_count, int32_t* valid, uint8_t* exposed, "
            "int32_t* exposed_count, int32_t* present_count, void* stream);") in flat
    assert ("int esmdiff_cooccurrence(const uint8_t* flags, int32_t n, int32_t L, int32_t* out, void* scratch, int64_t scratch_bytes, "
            "void* stream);") in flat
    assert re.search(r"#define ESMDIFF_ABI_VERSION 8\b", header)
    pairs_text = (ROOT / "esmdiff_amd" / "pairs.py").read_text()
    for name in ("esmdiff_sasa_frames", "esmdiff_cooccurrence"):
        assert name in N.EXPORTS and f"N.lib().{name}(" in pairs_text
    assert re.search(r"#define ESMDIFF_SASA_MAX_ATOMS %d\b" % N.SASA_MAX_ATOMS, header) and N.SASA_MAX_ATOMS == R.MAX_ATOMS == 4096
    assert re.search(r"#define ESMDIFF_SASA_MAX_POINTS %d\b" % N.SASA_MAX_POINTS, header) and N.SASA_MAX_POINTS == R.MAX_POINTS == 1024
    assert "#define ESMDIFF_COOCC_SCRATCH_BYTES(n, L) ((((int64_t)(n) + 63) / 64) * (int64_t)(L) * 16)" in header
    for n, L in ((0, 5), (1, 1), (64, 3), (65, 3), (100000, 256)):
        assert N.coocc_scratch_bytes(n, L) == R.cooccurrence_scratch_bytes(n, L) == -(-n // 64) * L * 16
    assert build.UNITS["sasa"] == ["-ffp-contract=off"] and (ROOT / "esmdiff_amd" / "csrc" / "sasa.hip").is_file()


def test_command_line_without_the_flag_is_unchanged(tmp_path, monkeypatch):
    from esmdiff_amd import accessibility, analyze_ensemble
    stub = {"TM-ens": 0.5, "best_tm": np.array([0.25, 0.75]), "flex": {"rmsf": np.array([1.0, np.nan])}}
    monkeypatch.setattr(analyze_ensemble, "analyze", lambda *a, **k: dict(stub))
    monkeypatch.setattr(analyze_ensemble, "load_ca", lambda *a, **k: (None, None, 4, np.arange(4)))
    calls = []
    monkeypatch.setattr(accessibility, "report", lambda *a, **k: calls.append((a, k)) or {"points": 96})
    monkeypatch.setattr(analyze_ensemble, "load_coords", lambda *a, **k: np.zeros((4, 5, 3, 3)))
    args = ["--samples", "ens.pdb", "--targets", "a.pdb", "--output"]
    plain = analyze_ensemble.main(args + [str(tmp_path / "plain")])
    assert not calls
    assert plain.read_text() == '{\n "TM-ens": 0.5,\n "best_tm": [\n  0.25,\n  0.75\n ],\n "flex": {\n  "rmsf": [\n   1.0,\n   null\n  ]\n }\n}\n'
    full = analyze_ensemble.main(args + [str(tmp_path / "sasa"), "--sasa", "--sasa_points", "64", "--sasa_probe", "1.2", "--sasa_threshold", "0.3"])
    data = json.loads(full.read_text())
    assert data.pop("sasa") == {"points": 96} and json.dumps(data, indent=1) + "\n" == plain.read_text()
    assert len(calls) == 1 and calls[0][0][2:] == (64, 1.2, 0.3) and calls[0][0][0].shape == (4, 5, 3, 3)
    a = analyze_ensemble.parser().parse_args(args + ["o"])
    assert (a.sasa, a.sasa_points, a.sasa_probe, a.sasa_threshold) == (False, 96, 1.4, 0.2)
    assert "--sasa" in analyze_ensemble.__doc__ and "unpinned" in analyze_ensemble.__doc__

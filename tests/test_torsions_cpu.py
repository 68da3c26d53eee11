"""CPU tests of the torsion layer: the numpy restatement tests/torsions_ref.py (the reference of tests/test_gpu_torsions.py) against
prescribed torsions of NeRF chains and hand-worked cases, the published order of the circular sums, the plain-numpy Jensen-Shannon
distance against scipy's, the region rectangles, the C ABI's declarations, and what needs no device in the Python surface."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import torsions_ref as R

ROOT = Path(__file__).resolve().parent.parent


def _wrap(d):
    return (d + 180.0) % 360.0 - 180.0


def test_restatement_recovers_prescribed_torsions():
    """50 seeded chains of 40 residues built by nerf from (phi, psi) at the centres of 10-degree bins +- 0.4 widths: phi and psi come
    back within 1e-9 degrees (the worst round trip seen is 4.3e-13), omega is +-180 with x < 0 (trans), nothing is cis."""
    rng = np.random.default_rng(20261020)
    X, pp = R.chains(rng, 50, 40)
    phi, psi, omega = (a * R.DEG for a in R.torsions(X))
    assert np.isnan(phi[:, 0]).all() and np.isnan(psi[:, -1]).all() and np.isnan(omega[:, -1]).all()
    assert not np.isnan(phi[:, 1:]).any() and not np.isnan(psi[:, :-1]).any() and not np.isnan(omega[:, :-1]).any()
    worst = max(np.abs(_wrap(phi[:, 1:] - pp[:, 1:, 0])).max(), np.abs(_wrap(psi[:, :-1] - pp[:, :-1, 1])).max())
    print("worst round-trip error (degrees):", worst)
    assert worst < 1e-9
    assert np.abs(np.abs(omega[:, :-1]) - 180.0).max() < 1e-9
    x, y, ok, present = R.xy(X)
    assert present.all() and ok[2][:, :-1].all() and (x[2][:, :-1] < 0).all()
    hist, counts, sums = R.ramachandran(X, 36)
    assert counts[:, 4].sum() == 0 and counts[1:-1, 2].tolist() == [50] * 38 and counts[0].tolist() == [0, 50, 0, 50, 0]
    # the histogram is the prescription's: no angle within 1 degree of an edge, so the cells are those of the prescribed angles
    edge = np.abs(_wrap(np.concatenate([phi[:, 1:].ravel(), psi[:, :-1].ravel()])) / 10.0)
    assert np.abs(edge - np.round(edge)).min() * 10.0 >= 0.999
    want = np.zeros_like(hist)
    for k in range(50):
        for i in range(1, 39):
            want[i, int((pp[k, i, 0] + 180.0) // 10), int((pp[k, i, 1] + 180.0) // 10)] += 1
    assert np.array_equal(hist, want)
    # the sign is IUPAC's: an alpha helix has phi = -57
    helix = R.torsions(R.nerf([(-57.0, -47.0)] * 5)[None, :, :3])
    assert abs(helix[0][0, 2] * R.DEG + 57.0) < 1e-9 and abs(helix[1][0, 2] * R.DEG + 47.0) < 1e-9


def _four(d):
    """p0 .. p3 with the dihedral d (degrees) about the z axis: p0 = (1, 0, 0), p1 = origin, p2 = (0, 0, 1), p3 turned by d."""
    a = np.deg2rad(d)
    return np.array([[1.0, 0, 0], [0.0, 0, 0], [0.0, 0, 1], [np.cos(a), np.sin(a), 1.0]])


def test_hand_worked_dihedrals():
    x, y, ok = R.dihedral_xy(*np.array([[1.0, 0, 0], [0.0, 0, 0], [0.0, 0, 1], [0.0, 1, 1]]))
    assert ok and x == 0.0 and y == 1.0 and np.arctan2(y, x) * R.DEG == 90.0
    x, y, ok = R.dihedral_xy(*np.array([[1.0, 0, 0], [0.0, 0, 0], [0.0, 0, 1], [0.0, -1, 1]]))
    assert ok and x == 0.0 and y == -1.0 and np.arctan2(y, x) * R.DEG == -90.0
    x, y, ok = R.dihedral_xy(*np.array([[1.0, 0, 0], [0.0, 0, 0], [0.0, 0, 1], [1.0, 0, 1]]))       # cis: 0
    assert ok and x == 1.0 and y == 0.0
    x, y, ok = R.dihedral_xy(*np.array([[1.0, 0, 0], [0.0, 0, 0], [0.0, 0, 1], [-1.0, 0, 1]]))      # trans: 180
    assert ok and x == -1.0 and y == 0.0 and np.arctan2(y, x) * R.DEG == 180.0
    # a collinear triple: both cross products of it vanish
    x, y, ok = R.dihedral_xy(*np.array([[0.0, 0, 0], [0.0, 0, 1], [0.0, 0, 2], [1.0, 0, 3]]))
    assert not ok and x == 0.0 and y == 0.0


def _peptide(omega_deg, cn=1.329):
    """Two residues whose CA_0, C_0, N_1, CA_1 have the dihedral omega; C_0 - N_1 is `cn` long along z."""
    p = _four(omega_deg)
    x = np.zeros((1, 2, 3, 3))
    x[0, 0] = [(2.0, 1.0, 0.0), p[0], p[1]]                          # N_0, CA_0, C_0
    n1 = np.array([0.0, 0.0, cn])
    x[0, 1] = [n1, n1 + (p[3] - p[2]), n1 + (p[3] - p[2]) + (0.5, 0.5, 1.0)]
    return x


def test_cis_peptide_bin_of_180_collinear_and_the_break():
    # omega = 0: cis is counted, x > 0
    x, y, ok, _ = R.xy(_peptide(0.0))
    hist, counts, sums = R.ramachandran(_peptide(0.0), 36)
    assert ok[2][0, 0] and x[2][0, 0] > 0 and y[2][0, 0] == 0.0 and counts[0].tolist() == [0, 1, 0, 1, 1]
    assert sums[0, 4] == 1.0 and sums[0, 5] == 0.0
    x, y, ok, _ = R.xy(_peptide(180.0))
    assert ok[2][0, 0] and x[2][0, 0] < 0 and R.ramachandran(_peptide(180.0), 36)[1][0].tolist() == [0, 1, 0, 1, 0]
    # +180 degrees lands in bin 0, -180 too; 179.9 stays in the last bin
    for bins in (1, 7, 36, 72):
        assert R.bin_of(np.array([np.pi, -np.pi, np.deg2rad(179.9), 0.0]), bins).tolist() == [0, 0, bins - 1, bins // 2]
    # a collinear CA_0, C_0, N_1 (psi and omega share it): NaN, counted nowhere, while phi of residue 1 is not touched
    line = _peptide(180.0)
    line[0, 0, 1] = (0.0, 0.0, -1.5)                                 # CA_0 on the C_0 - N_1 axis
    phi, psi, omega = R.torsions(line)
    assert np.isnan(psi[0, 0]) and np.isnan(omega[0, 0])
    assert R.ramachandran(line, 36)[1][0].tolist() == [0, 0, 0, 0, 0] and R.ramachandran(line, 36)[0].sum() == 0
    # |C - N| of exactly 2.5 links, the next float above breaks
    assert R.xy(_peptide(180.0, 2.5))[2][2][0, 0] and not R.xy(_peptide(180.0, np.nextafter(2.5, 3.0)))[2][2][0, 0]
    phi, psi, omega, geom = R.torsions(_peptide(180.0, np.nextafter(2.5, 3.0)), geometry=True)
    assert np.isnan(omega[0, 0]) and np.isnan(phi[0, 1]) and geom[0, 0, 2] == np.nextafter(2.5, 3.0)     # the length needs no link
    assert np.isnan(geom[0, 1, 2]) and np.isnan(geom[0, 1, 4]) and np.isfinite(geom[0, 1, 0])
    # a masked residue takes its neighbours' torsions with it; its coordinates influence nothing
    X, _ = R.chains(np.random.default_rng(1), 1, 6)
    mask = np.ones((1, 6), bool)
    mask[0, 3] = False
    got = R.torsions(X, mask, geometry=True)
    junk = X.copy()
    junk[0, 3] = np.nan
    for g, h in zip(got, R.torsions(junk, mask, geometry=True)):
        assert np.array_equal(g, h, equal_nan=True)
    assert np.isnan(got[0][0, 3:5]).all() and np.isnan(got[1][0, 2:4]).all() and np.isfinite(got[0][0, 1:3]).all()


def test_geometry_is_nerf_s():
    X, _ = R.chains(np.random.default_rng(2), 3, 12)
    geom = R.torsions(X, geometry=True)[3]
    ideal = np.array([1.458, 1.525, 1.329, 111.0, 116.2, 121.7])
    got = geom[:, :-1] * np.array([1, 1, 1, R.DEG, R.DEG, R.DEG])
    assert np.abs(got - ideal).max() < 1e-9
    assert np.isnan(geom[:, -1, [2, 4, 5]]).all() and np.isfinite(geom[:, -1, [0, 1, 3]]).all()


def _macros(tmp_path):
    """The header's function-like macros as C functions: a few lines of C that include the header, compiled by the host compiler."""
    import ctypes
    import shutil
    import subprocess
    cc = next((c for c in (shutil.which("cc"), shutil.which("gcc"), shutil.which("clang"), "/opt/rocm/llvm/bin/clang",
                           "/opt/rocm/lib/llvm/bin/clang") if c and Path(c).exists()), None)
    assert cc, "no host C compiler"
    src = tmp_path / "rama_macros.c"
    src.write_text('#include "esmdiff_hip.h"\n'
                   "int64_t chunks(int64_t n, int64_t L) { return ESMDIFF_RAMA_CHUNKS(n, L); }\n"
                   "int64_t frames(int64_t n, int64_t L) { return ESMDIFF_RAMA_CHUNK_FRAMES(n, L); }\n"
                   "int64_t scratch(int64_t n, int64_t L) { return ESMDIFF_RAMA_SCRATCH_BYTES(n, L); }\n")
    subprocess.run([cc, "-shared", "-fPIC", "-O1", f"-I{ROOT / 'include'}", str(src), "-o", str(tmp_path / "rama_macros.so")], check=True)
    lib = ctypes.CDLL(str(tmp_path / "rama_macros.so"))
    for fn in (lib.chunks, lib.frames, lib.scratch):
        fn.argtypes, fn.restype = [ctypes.c_int64, ctypes.c_int64], ctypes.c_int64
    return lib.chunks, lib.frames, lib.scratch


def test_chunked_order_is_the_one_the_header_states(tmp_path):
    """The sums recomputed with the macros compiled from the header: chunks of F frames, inside a chunk the defined terms one after
    another from the first defined one, the chunk sums from chunk 0's; and the binding mirrors the macros on a grid of (n, L)."""
    from esmdiff_amd import _native as N
    chunks, frames, scratch = _macros(tmp_path)
    seen = set()
    for L in (1, 2, 58, 63, 64, 65, 130, 256, 4096, 4097, 65536, 65537, 100000):
        for n in (0, 1, 15, 16, 17, 32, 33, 100, 1000, 16384, 16385, 100000):
            c = chunks(n, L)
            assert c == N.rama_chunks(n, L) == R.chunks(n, L), (n, L)
            assert frames(n, L) == N.rama_chunk_frames(n, L) == R.chunk_frames(n, L), (n, L)
            assert scratch(n, L) == N.rama_scratch_bytes(n, L) == R.scratch_bytes(n, L), (n, L)
            assert 0 <= c <= 1024 and (n == 0 or (c - 1) * frames(n, L) < n <= c * frames(n, L))      # no chunk is empty
            assert (scratch(n, L) == 0) == (c <= 1) and scratch(n, L) in (0, c * L * 48)
            seen.add(c)
    assert {0, 1, 2, 3, 63, 1021} <= seen and frames(100000, 58) == 98 and chunks(100000, 58) == 1021 and chunks(1000, 256) == 63
    rng = np.random.default_rng(3)
    n, L = 40, 5
    X, _ = R.chains(rng, n, L)
    mask = rng.random((n, L)) > 0.25
    mask[:17, 2] = False                                             # residue 2: chunk 0 (16 frames) has no defined term at all
    F, C = int(frames(n, L)), int(chunks(n, L))
    assert (F, C) == (16, 3)
    x, y, ok, _ = R.xy(X, mask)
    with np.errstate(all="ignore"):
        r = np.sqrt(x * x + y * y)
        terms = [x[0] / r[0], y[0] / r[0], x[1] / r[1], y[1] / r[1], x[2] / r[2], y[2] / r[2]]
    want = np.zeros((L, 6))
    for i in range(L):
        for k in range(6):
            total = None
            for c in range(C):
                part = None
                for f in range(c * F, min(n, (c + 1) * F)):
                    if ok[k // 2][f, i]:
                        part = terms[k][f, i] if part is None else part + terms[k][f, i]
                part = 0.0 if part is None else part
                total = part if total is None else total + part
            want[i, k] = total
    got = R.ramachandran(X, 36, mask)[2]
    assert np.array_equal(got.view(np.int64), want.view(np.int64))
    assert np.abs(got).sum() > 10 and not ok[0][:16, 2].any() and ok[0][17:, 2].any()


def test_js_formula_is_scipys():
    from scipy.spatial.distance import jensenshannon
    from esmdiff_amd import torsions as T
    rng = np.random.default_rng(4)
    for k in range(20):
        a = rng.integers(0, 30, 1296) * (rng.random(1296) < 0.1) + 1e-6
        b = rng.integers(0, 30, 1296) * (rng.random(1296) < 0.1) + 1e-6
        want = jensenshannon(a, b)
        assert abs(T.js_distance(a, b) - want) < 1e-15 and abs(R.js_distance(a, b) - want) < 1e-15, k
    assert T.js_distance(a, a) == 0.0


def test_regions_partition_the_plane_and_stay_on_the_grid():
    from esmdiff_amd import torsions as T
    for bins in (36, 72):
        table = T._region_table(bins, T.REGIONS)
        assert table.min() == 0 and table.max() == len(T.REGIONS) - 1            # every cell in exactly one region (overlap raises)
    area = sum((r[1] - r[0]) * (r[3] - r[2]) for rects in T.REGIONS.values() for r in rects)
    assert area == 360 * 360 and all(e % 10 == 0 for rects in T.REGIONS.values() for r in rects for e in r)
    table, names, w = T._region_table(36, T.REGIONS), list(T.REGIONS), 10
    cell = lambda phi, psi: names[table[int((phi + 180) // w), int((psi + 180) // w)]]
    assert [cell(-57, -47), cell(-120, 130), cell(-75, 145), cell(57, 47), cell(60, -150)] == ["alpha", "beta", "ppII", "left", "other"]
    with pytest.raises(ValueError, match="grid"):
        T._region_table(36, {"a": [(-175, 0, -180, 180)]})
    with pytest.raises(ValueError, match="grid"):
        T._region_table(1, T.REGIONS)
    with pytest.raises(ValueError, match="overlaps"):
        T._region_table(36, {"a": [(-180, 0, -180, 180)], "b": [(-10, 180, -180, 180)]})
    m = T.RamachandranMap(np.zeros((2, 36, 36), np.int32), np.zeros((2, 5), np.int32), np.zeros((2, 6)), 36, 3)
    m.hist[0, 12, 13], m.hist[0, 6, 31], m.counts[0] = 2, 1, (3, 3, 3, 3, 1)
    m.sums[0] = (0.0, 3.0, 3.0, 0.0, -1.0, 0.0)
    assert m.region_counts().tolist() == [[2, 1, 0, 0, 0], [0] * 5] and np.isnan(m.region_propensity()[1]).all()
    assert m.region_propensity()[0].tolist() == [2 / 3, 1 / 3, 0, 0, 0] and m.cis_fraction()[0] == 1 / 3 and np.isnan(m.cis_fraction()[1])
    assert np.allclose(m.circular_mean()[0], [90.0, 0.0, 180.0]) and np.allclose(m.circular_variance()[0], [0.0, 0.0, 2 / 3])
    assert abs(m.entropy()[0] - (np.log(3) - 2 / 3 * np.log(2))) < 1e-15 and np.isnan(m.entropy()[1]) and np.isnan(m.density()[1]).all()


def test_header_binding_and_build_declare_the_unit():
    from esmdiff_amd import _native as N
    from esmdiff_amd import build
    header = (ROOT / "include" / "esmdiff_hip.h").read_text()
    decl = re.search(r"int\s+esmdiff_backbone_torsions\s*\(([^;]*)\)\s*;", header)
    assert decl, "include/esmdiff_hip.h does not declare esmdiff_backbone_torsions"
    args = [a.strip() for a in decl.group(1).split(",")]
    assert len(args) == 11 and args[0] == "const double* X" and args[3] == "int32_t atoms" and args[-1] == "void* stream"
    assert [a for a in args if a.startswith("double*")] == ["double* phi", "double* psi", "double* omega", "double* geom"]
    decl = re.search(r"int\s+esmdiff_ramachandran\s*\(([^;]*)\)\s*;", header)
    assert decl, "include/esmdiff_hip.h does not declare esmdiff_ramachandran"
    args = [a.strip() for a in decl.group(1).split(",")]
    assert len(args) == 13 and args[0] == "const double* X" and args[-1] == "void* stream" and "int32_t bins" in args
    assert [a for a in args if a.startswith("int32_t*")] == ["int32_t* hist", "int32_t* counts"] and "double* sums" in args
    assert "esmdiff_backbone_torsions" in N.EXPORTS and "esmdiff_ramachandran" in N.EXPORTS
    assert re.search(r"#define\s+ESMDIFF_ABI_VERSION\s+8\b", header) and "#define ESMDIFF_ABI_VERSION 8 " in header
    assert int(re.search(r"#define\s+ESMDIFF_RAMA_MAX_BINS\s+(\d+)", header).group(1)) == 72 == N.RAMA_MAX_BINS == R.MAX_BINS
    assert "-ffp-contract=off" in build.UNITS["torsions"]
    src = (ROOT / "esmdiff_amd" / "csrc" / "torsions.hip").read_text()
    assert "57.29577951308232" in src and "acos" not in src
    binding = (ROOT / "esmdiff_amd" / "_native.py").read_text()
    assert "L.esmdiff_backbone_torsions.argtypes" in binding and "L.esmdiff_ramachandran.argtypes" in binding


def test_parser_knows_torsions():
    from esmdiff_amd import analyze_ensemble
    a = analyze_ensemble.parser().parse_args(["--samples", "x.pdb", "--targets", "t.pdb", "--output", "o", "--torsions", "--rama_bins", "72"])
    assert a.torsions is True and a.rama_bins == 72
    a = analyze_ensemble.parser().parse_args(["--samples", "x.pdb", "--targets", "t.pdb", "--output", "o"])
    assert a.torsions is False and a.rama_bins == 36
    assert "--torsions" in analyze_ensemble.__doc__ and "--rama_bins" in analyze_ensemble.__doc__


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_torsions_have_no_cpu_fallback():
    from esmdiff_amd import torsions as T
    x = R.nerf([(-57.0, -47.0)] * 5)[None]
    for call in (lambda: T.torsions(x), lambda: T.ramachandran(x), lambda: T.js_ramachandran({"target": x, "m": x}),
                 lambda: T.torsion_agreement(x, x), lambda: T.region_switches(x, x[0], x[0]), lambda: T.geometry_summary(x),
                 lambda: T.report(x, [x[0]])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()

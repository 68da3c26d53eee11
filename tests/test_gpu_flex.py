"""GPU tests of the flexibility layer: the three kernels of esmdiff_amd/csrc/flex.hip through esmdiff_amd/pairs.py, and
esmdiff_amd/flexibility.py above them, against the float64 numpy restatement tests/flex_ref.py (itself held to hand-worked cases,
sklearn and scipy by tests/test_flex_cpu.py).

Tolerances are those of tests/test_gpu_ensemble.py, not of the new code: squared deviations and msf (A^2) atol 1e-9 (its `sd`
tolerance), coordinates and means (A) atol 1e-7 (its translation tolerance), counts exactly.
Shapes: L = 2, 63, 64, 65, 130 around the wave width (a lane owns residues l, l + 64 ...); n = 2, 5, 7, 37 for a partial last
workgroup of the fit kernel (4 structures each) and both parities of the pair kernel's row pairing (odd n has an unpaired middle
row)."""
import json

import numpy as np
import pytest

from tests import ensemble_ref as E
from tests import flex_ref as F

pytestmark = pytest.mark.gpu

SD_ATOL = 1e-9          # A^2
XYZ_ATOL = 1e-7         # A


@pytest.fixture(scope="module")
def flex():
    from esmdiff_amd import flexibility
    return flexibility


def _device_pair_msf(A, mask=None):
    from esmdiff_amd import pairs
    T = pairs.coords(A)
    s, c = pairs.pair_msf(T, pairs.valid_mask(T, mask))
    return s.cpu().numpy(), c.cpu().numpy()


def _masked_case(rng, n=9, L=70):
    """20 % masked at random, half of it as NaN coordinates; residue 5 valid in no structure; structure 3 keeps one residue."""
    A = E.ensemble(rng, n, L)
    mask = rng.random((n, L)) > 0.2
    mask[:, 5] = False
    mask[3] = False
    mask[3, 11] = True
    nan_too = ~mask & (rng.random((n, L)) < 0.5)
    A[nan_too] = np.nan
    return A, mask


# ---- the pair kernel -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,L", [(2, 2), (2, 63), (5, 64), (7, 65), (37, 130)])
def test_pair_msf_against_the_restatement(n, L):
    A = E.ensemble(np.random.default_rng(100 * n + L), n, L)
    want_sum, want_count = F.pair_msf(A)
    got_sum, got_count = _device_pair_msf(A)
    assert got_count.dtype == np.int64 and np.array_equal(got_count, want_count) and np.all(got_count == n * (n - 1) // 2)
    np.testing.assert_allclose(got_sum / got_count, want_sum / want_count, rtol=0, atol=SD_ATOL)


def test_pair_msf_with_masks_and_nan(flex):
    A, mask = _masked_case(np.random.default_rng(7))
    want_sum, want_count = F.pair_msf(A, mask)
    got_sum, got_count = _device_pair_msf(A, mask)
    assert np.array_equal(got_count, want_count)
    assert got_count[5] == 0 and got_sum[5] == 0
    # structure 3 has one valid residue: none of its 8 pairs is fitted, so residue 11 is counted among the other 8 structures only
    valid = mask & ~np.isnan(A).any(-1)
    others = np.delete(valid[:, 11], 3).sum()
    assert got_count[11] == others * (others - 1) // 2 and got_count.max() <= 8 * 7 // 2
    some = want_count > 0
    np.testing.assert_allclose(got_sum[some] / got_count[some], want_sum[some] / want_count[some], rtol=0, atol=SD_ATOL)
    r = flex.pair_rmsf(A, mask)
    assert np.isnan(r[5]) and np.isfinite(np.delete(r, 5)).all()
    np.testing.assert_allclose(np.delete(r, 5) ** 2, np.delete(want_sum / np.maximum(want_count, 1), 5), rtol=0, atol=SD_ATOL)


def test_pair_rmsf_equals_the_shipped_route(flex):
    from esmdiff_amd import ensemble
    S = E.ensemble(np.random.default_rng(12), 12, 70)
    iu = np.triu_indices(12, 1)
    want = np.mean(ensemble.aligned_deviation(S)[iu] ** 2, axis=0)
    np.testing.assert_allclose(flex.pair_rmsf(S) ** 2, want, rtol=0, atol=SD_ATOL)


def test_pair_msf_is_deterministic_and_order_free():
    rng = np.random.default_rng(21)
    A = E.ensemble(rng, 37, 130)
    first, again = _device_pair_msf(A), _device_pair_msf(A)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    shuffled = _device_pair_msf(A[rng.permutation(37)])
    assert np.array_equal(shuffled[1], first[1])
    np.testing.assert_allclose(shuffled[0] / first[1], first[0] / first[1], rtol=0, atol=SD_ATOL)


def test_pair_msf_edges(flex):
    import torch
    from esmdiff_amd import pairs
    one = E.ensemble(np.random.default_rng(1), 1, 9)
    s, c = _device_pair_msf(one)
    assert np.all(c == 0) and np.all(s == 0) and np.isnan(flex.pair_rmsf(one)).all()
    with pytest.raises(RuntimeError, match="L = 1"):
        pairs.pair_msf(torch.zeros((3, 1, 3), dtype=torch.float64, device="cuda"), None)
    with pytest.raises(RuntimeError, match="L = 1"):
        pairs.fit(torch.zeros((3, 1, 3), dtype=torch.float64, device="cuda"), None, torch.zeros((1, 3), dtype=torch.float64, device="cuda"), None)
    with pytest.raises(RuntimeError, match="L = 1"):
        pairs.moments(torch.zeros((3, 1, 3), dtype=torch.float64, device="cuda"), None)


# ---- the mean structure --------------------------------------------------------------------------------------------------------------
def _compare(ms, ref, n_iter=None):
    assert np.array_equal(ms.count, ref["count"])
    if n_iter is not None:
        assert ms.n_iter == n_iter
    np.testing.assert_allclose(ms.aligned, ref["aligned"], rtol=0, atol=XYZ_ATOL, equal_nan=True)
    np.testing.assert_allclose(ms.mean, ref["mean"], rtol=0, atol=XYZ_ATOL, equal_nan=True)
    np.testing.assert_allclose(ms.rmsf ** 2, ref["msf"], rtol=0, atol=SD_ATOL, equal_nan=True)


@pytest.mark.parametrize("n,L", [(5, 63), (37, 65)])
def test_one_iteration_against_the_restatement(flex, n, L):
    A = E.ensemble(np.random.default_rng(31 * n + L), n, L)
    ms = flex.mean_structure(A, tol=0, max_iter=1)
    ref = F.gpa(A, tol=0, max_iter=1)
    assert not ms.converged
    _compare(ms, ref, 1)
    np.testing.assert_allclose(ms.rmsd_to_mean, ref["rmsd_to_mean"], rtol=1e-9)


@pytest.mark.parametrize("n,L,noise", [(5, 63, 1.5), (12, 130, 3.0), (3, 7, 1.5)])
def test_thirty_iterations_against_the_restatement(flex, n, L, noise):
    A = E.ensemble(np.random.default_rng(17 * n + L), n, L, noise=noise)
    ref = F.gpa(A, tol=0, max_iter=30)
    assert ref["steps"][-1] < 1e-10, ref["steps"][-5:]           # a condition on the inputs: the restatement is at its fixed point
    _compare(flex.mean_structure(A, tol=0, max_iter=30), ref, 30)
    np.testing.assert_allclose(flex.rmsf(A, tol=0, max_iter=30) ** 2, ref["msf"], rtol=0, atol=SD_ATOL)


def test_default_stopping(flex):
    A = E.ensemble(np.random.default_rng(5), 12, 65)
    ms, ref = flex.mean_structure(A), F.gpa(A)
    assert ref["converged"] and ms.converged and ms.n_iter < 50
    assert abs(ms.n_iter - ref["n_iter"]) <= 1                   # a borderline step may fall either side of tol


def test_rigid_motion_of_the_inputs_changes_nothing(flex):
    rng = np.random.default_rng(9)
    A = E.ensemble(rng, 7, 65)
    a = flex.mean_structure(A, tol=0, max_iter=30)
    b = flex.mean_structure(F.rigid_moves(rng, A), tol=0, max_iter=30)
    np.testing.assert_allclose(b.rmsf ** 2, a.rmsf ** 2, rtol=0, atol=SD_ATOL)


def test_mean_structure_with_masks(flex):
    rng = np.random.default_rng(13)
    A = E.ensemble(rng, 9, 70)
    mask = rng.random((9, 70)) > 0.2
    mask[:, 5] = False
    mask[0, :3] = True                                           # the start structure can be fitted
    nan_too = ~mask & (rng.random((9, 70)) < 0.5)
    A[nan_too] = np.nan
    ms = flex.mean_structure(A, mask, tol=0, max_iter=30)
    ref = F.gpa(A, mask, tol=0, max_iter=30)
    assert ref["steps"][-1] < 1e-10, ref["steps"][-5:]
    assert ms.count[5] == 0 and np.isnan(ms.mean[5]).all() and np.isnan(ms.rmsf[5])
    assert np.isfinite(np.delete(ms.mean, 5, 0)).all() and np.isfinite(np.delete(ms.rmsf, 5)).all()
    _compare(ms, ref, 30)
    np.testing.assert_allclose(ms.rmsd_to_mean, ref["rmsd_to_mean"], rtol=1e-9)


# ---- PCA -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[(12, 65), (40, 20), (80, 21)], ids=lambda p: f"n{p[0]}_L{p[1]}")
def planted_case(request, flex):
    n, L = request.param
    A = F.planted(np.random.default_rng(1000 * n + L), n, L)
    k = min(n - 1, 3 * L)
    return A, F.pca(A, n_components=k, tol=0, max_iter=30), flex.pca(A, n_components=k, tol=0, max_iter=30)


def test_pca_against_the_restatement(planted_case):
    A, ref, got = planted_case
    n, L = A.shape[:2]
    k = min(n - 1, 3 * L)
    lam, trace = ref["explained_variance"], ref["trace"]
    gaps = (lam[:2] - lam[1:3]) / trace
    assert np.all(gaps >= 0.05), gaps                            # a condition on the inputs: the two leading modes are well separated
    assert got.explained_variance.shape == (k,) and got.modes.shape == (k, L, 3) and got.projections.shape == (n, k)
    assert np.array_equal(got.residues, np.arange(L))
    np.testing.assert_allclose(got.explained_variance, lam, rtol=0, atol=1e-9 * trace)
    np.testing.assert_allclose(got.explained_variance_ratio, ref["explained_variance_ratio"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(got.mean, ref["mean"], rtol=0, atol=XYZ_ATOL)
    np.testing.assert_allclose(np.linalg.norm(got.modes.reshape(k, -1), axis=1), 1.0, rtol=0, atol=1e-12)
    flat = got.modes.reshape(k, -1)
    assert np.all(flat[np.arange(k), np.abs(flat).argmax(1)] > 0)
    cos = np.abs((flat[:2] * ref["modes"].reshape(k, -1)[:2]).sum(1))
    assert np.all(1 - cos <= 1e-10), 1 - cos
    np.testing.assert_allclose(got.projections[:, :2], ref["projections"][:, :2], rtol=0, atol=XYZ_ATOL * np.sqrt(3 * L))


def test_pca_projection_and_displacement_overlap(planted_case):
    A, ref, got = planted_case
    L = A.shape[1]
    tol = XYZ_ATOL * np.sqrt(3 * L)
    np.testing.assert_allclose(got.project(A)[:, :2], got.projections[:, :2], rtol=0, atol=tol)
    moved = F.rigid_moves(np.random.default_rng(3), A)
    np.testing.assert_allclose(got.project(moved)[:, :2], got.projections[:, :2], rtol=0, atol=tol)
    res = got.displacement_overlap(A[0], A[1])
    want, count = F.displacement_overlap(ref, A[0], A[1])
    assert res["n_residues"] == count == L
    # the leading two are compared mode by mode; the whole span when every mode is there (then both sides reach the same share)
    np.testing.assert_allclose(res["overlap"][:2], want[:2], rtol=0, atol=1e-9)
    np.testing.assert_allclose(res["overlap"][-1], want[-1], rtol=0, atol=1e-9)
    assert np.all(np.diff(res["overlap"]) >= 0) and res["overlap"][-1] <= 1 + 1e-12


# ---- the command line ----------------------------------------------------------------------------------------------------------------
def _write_pdb(path, models):
    lines = []
    for k, xyz in enumerate(models):
        lines.append(f"MODEL     {k + 1:4d}")
        for i, (x, y, z) in enumerate(xyz):
            lines.append(f"ATOM  {i + 1:5d}  CA  ALA A{i + 1:4d}    {x:8.3f}{y:8.3f}{z:8.3f}  1.00  0.00           C")
        lines.append("ENDMDL")
    path.write_text("\n".join(lines) + "\nEND\n")


def test_cli_flex_block(tmp_path, flex):
    from esmdiff_amd import analyze_ensemble
    rng = np.random.default_rng(4)
    S = E.ensemble(rng, 8, 12, noise=1.0)
    S -= S.mean((0, 1))                                          # keep the coordinates inside a PDB column
    _write_pdb(tmp_path / "samples.pdb", S[:6])
    _write_pdb(tmp_path / "apo.pdb", S[6:7])
    _write_pdb(tmp_path / "holo.pdb", S[7:8])
    args = ["--samples", str(tmp_path / "samples.pdb"), "--targets", str(tmp_path / "apo.pdb"), str(tmp_path / "holo.pdb")]
    plain = json.loads(analyze_ensemble.main(args + ["--output", str(tmp_path / "plain")]).read_text())
    assert "flex" not in plain
    out = json.loads(analyze_ensemble.main(args + ["--output", str(tmp_path / "flex"), "--flex", "--pca_components", "2"]).read_text())
    assert {k: v for k, v in out.items() if k != "flex"} == plain
    fx = out["flex"]
    assert set(fx) == {"n_iter", "converged", "rmsd_to_mean", "mean", "rmsf", "pair_rmsf", "pca", "resflex", "resflex_mean_structure",
                       "displacement_overlap"}
    assert fx["converged"] is True and 1 <= fx["n_iter"] < 50
    for key, shape in (("rmsd_to_mean", (6,)), ("mean", (12, 3)), ("rmsf", (12,)), ("pair_rmsf", (12,))):
        v = np.array(fx[key], np.float64)
        assert v.shape == shape and np.isfinite(v).all(), key
    np.testing.assert_allclose(np.square(fx["pair_rmsf"]), np.square(out["rmsf"]), rtol=0, atol=SD_ATOL)   # no masks: apo_report's numbers
    assert set(fx["pca"]) == {"explained_variance", "explained_variance_ratio", "projections", "target_projections"}
    for key, shape in (("explained_variance", (2,)), ("explained_variance_ratio", (2,)), ("projections", (6, 2)),
                       ("target_projections", (2, 2))):
        v = np.array(fx["pca"][key], np.float64)
        assert v.shape == shape and np.isfinite(v).all(), key
    want = flex.flexibility_correlation(np.array(out["rmsd"], np.float64), np.array(out["rmsf"], np.float64))
    assert fx["resflex"] == want and fx["resflex"]["n"] == 12
    assert fx["resflex_mean_structure"] == flex.flexibility_correlation(np.array(out["rmsd"], np.float64), np.array(fx["rmsf"], np.float64))
    ov = fx["displacement_overlap"]
    assert ov["n_residues"] == 12 and len(ov["overlap"]) == 2 and 0 <= ov["overlap"][0] <= ov["overlap"][1] <= 1

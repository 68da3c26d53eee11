"""CPU tests of the flexibility layer (esmdiff_amd/flexibility.py, csrc/flex.hip): the numpy restatement tests/flex_ref.py on
hand-worked cases, the conventions pinned against sklearn and scipy where they are installed, the host statistics of
flexibility.py (plain numpy: they run here), the binding, and the no-GPU failure mode.  The kernels themselves are compared with
the restatement in tests/test_gpu_flex.py."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import ensemble_ref as E
from tests import flex_ref as F

ROOT = Path(__file__).resolve().parent.parent


# ---- hand-worked cases ------------------------------------------------------------------------------------------------------------
def test_rigid_copies_have_no_flexibility():
    rng = np.random.default_rng(0)
    base = E.ca_chain(rng, 9)
    A = F.rigid_moves(rng, np.stack([base] * 5))
    sum_sq, count = F.pair_msf(A)
    assert np.array_equal(count, np.full(9, 5 * 4 // 2))
    # coordinates of ~50 A moved by rounding-grade rotations: squared deviations of (50 x 1e-15)^2 per pair, far below this
    assert np.all(sum_sq < 1e-22)
    g = F.gpa(A, tol=0, max_iter=3)
    assert np.all(g["msf"] < 1e-22) and np.all(g["rmsd_to_mean"] < 1e-11) and np.array_equal(g["count"], np.full(9, 5))


def test_one_residue_moves_alone_by_hand():
    """Three copies of a square pyramid; residue 0 of the third is lifted by 0.3 A, nothing else moves."""
    sq = np.array([[0.0, 0, 0], [2, 0, 0], [2, 2, 0], [0, 2, 0], [1, 1, 1.5]])
    A = np.stack([sq, sq, sq])
    A[2, 0] += [0, 0, 0.3]
    # the fit is on ALL common residues and minimises the summed squared deviation of a pair over rigid motions; moving the centroids
    # onto each other alone (no rotation) leaves 0.3^2 (1 - 1/5) = 0.072 per pair, so two pairs give at most 0.144
    sum_sq, count = F.pair_msf(A)
    assert np.array_equal(count, np.full(5, 3))
    assert 0 < sum_sq.sum() <= 2 * 0.072 and sum_sq.argmax() == 0
    # pairs (0, 1) are identical: everything comes from the two pairs with structure 2, which are equal
    _, sd, _, _ = E.superpose_pair(A[0], A[2])
    np.testing.assert_allclose(sum_sq, 2 * sd, rtol=0, atol=1e-15)
    # masked out of the third structure, the residue is counted in one pair only and contributes nothing
    mask = np.ones((3, 5), bool)
    mask[2, 0] = False
    sum_sq, count = F.pair_msf(A, mask)
    # (identical points of size 2 A under a rotation exact to a few 1e-16: deviations of 1e-15, squared and summed over two pairs)
    assert count.tolist() == [1, 3, 3, 3, 3] and np.all(sum_sq < 1e-26)
    # moments by hand: the mean of residue 0 over z = 0, 0, 0.3 is 0.1; msf = (0.01 + 0.01 + 0.04) / 3
    mean, msf, cnt = F.moments(A, np.ones((3, 5), bool))
    np.testing.assert_allclose(mean[0], [0, 0, 0.1], atol=1e-16)
    np.testing.assert_allclose(msf, [0.02, 0, 0, 0, 0], atol=1e-16)
    assert cnt.tolist() == [3] * 5


def test_gpa_rule_on_a_small_case():
    rng = np.random.default_rng(3)
    A = E.ensemble(rng, 6, 11, noise=1.0)
    g = F.gpa(A)
    assert g["converged"] and g["n_iter"] < 50 and g["steps"][-1] <= 1e-6
    assert F.gpa(A, tol=0, max_iter=4)["n_iter"] == 4            # tol = 0 runs exactly max_iter iterations
    # at the fixed point the mean is the mean of the aligned structures, and rigid motion of the inputs does not change the answer
    far = F.gpa(A, tol=0, max_iter=30)
    assert far["steps"][-1] < 1e-10
    np.testing.assert_allclose(far["aligned"].mean(0), far["mean"], atol=1e-12)
    moved = F.gpa(F.rigid_moves(rng, A), tol=0, max_iter=30)
    np.testing.assert_allclose(moved["msf"], far["msf"], rtol=0, atol=1e-9)
    # a residue masked everywhere has no mean; one masked in a single structure is counted n - 1 times
    mask = np.ones((6, 11), bool)
    mask[:, 4] = False
    mask[2, 7] = False
    gm = F.gpa(A, mask, tol=0, max_iter=5)
    assert gm["count"][4] == 0 and gm["count"][7] == 5 and np.isnan(gm["mean"][4]).all() and np.isnan(gm["rmsf"][4])


# ---- convention pins ---------------------------------------------------------------------------------------------------------------
def test_pca_restatement_uses_sklearns_divisor():
    sk = pytest.importorskip("sklearn.decomposition")
    rng = np.random.default_rng(5)
    A = F.planted(rng, 14, 9)
    p = F.pca(A, n_components=5, tol=0, max_iter=30)
    X = (F.gpa(A, tol=0, max_iter=30)["aligned"]).reshape(14, -1)
    ref = sk.PCA(n_components=5, svd_solver="full").fit(X)
    np.testing.assert_allclose(p["explained_variance"], ref.explained_variance_, rtol=1e-10)
    np.testing.assert_allclose(p["explained_variance_ratio"], ref.explained_variance_ratio_, rtol=1e-10)
    cos = np.abs((p["modes"].reshape(5, -1) * ref.components_).sum(1))
    np.testing.assert_allclose(cos[:3], 1.0, atol=1e-10)
    assert np.all(np.diff(p["explained_variance"]) < 0) and p["explained_variance_ratio"].sum() <= 1 + 1e-12


def _profiles():
    rng = np.random.default_rng(11)
    x = rng.normal(size=40)
    y = 0.6 * x + rng.normal(size=40)
    tied_x, tied_y = np.round(x * 2) / 2, np.round(y)             # many ties on both sides
    return [(x, y), (tied_x, tied_y), (tied_x, y), (x, -x ** 3)]


def test_flexibility_correlation_against_scipy():
    st = pytest.importorskip("scipy.stats")
    from esmdiff_amd.flexibility import flexibility_correlation
    for x, y in _profiles():
        got = flexibility_correlation(x, y)
        assert got["n"] == 40
        np.testing.assert_allclose(got["pearson"], st.pearsonr(x, y)[0], rtol=0, atol=1e-12)
        np.testing.assert_allclose(got["spearman"], st.spearmanr(x, y).correlation, rtol=0, atol=1e-12)
        np.testing.assert_allclose(got["kendall"], st.kendalltau(x, y).correlation, rtol=0, atol=1e-12)
        np.testing.assert_allclose([F.pearson(x, y), F.spearman(x, y), F.kendall(x, y)],
                                   [got["pearson"], got["spearman"], got["kendall"]], rtol=0, atol=1e-12)
    # NaN entries are dropped pairwise, as apo_analysis.py's getmask does
    x, y = _profiles()[0]
    xn, yn = x.copy(), y.copy()
    xn[3], yn[17] = np.nan, np.nan
    ok = np.isfinite(xn) & np.isfinite(yn)
    got = flexibility_correlation(xn, yn)
    assert got["n"] == 38
    np.testing.assert_allclose(got["kendall"], st.kendalltau(x[ok], y[ok]).correlation, rtol=0, atol=1e-12)
    # a constant side: scipy returns NaN (with a warning), and so does this
    const = flexibility_correlation(np.ones(40), y)
    assert np.isnan([const["pearson"], const["spearman"], const["kendall"]]).all() and const["n"] == 40


def test_flexibility_correlation_by_hand():
    from esmdiff_amd.flexibility import _average_ranks, flexibility_correlation
    x = np.array([1.0, 2.0, 2.0, 4.0, 5.0])
    y = np.array([2.0, 1.0, 3.0, 3.0, 5.0])
    # ranks: x -> 1, 2.5, 2.5, 4, 5;  y -> 2, 1, 3.5, 3.5, 5
    assert _average_ranks(x).tolist() == [1, 2.5, 2.5, 4, 5] and _average_ranks(y).tolist() == [2, 1, 3.5, 3.5, 5]
    got = flexibility_correlation(x, y)
    rx, ry = np.array([1, 2.5, 2.5, 4, 5]) - 3, np.array([2, 1, 3.5, 3.5, 5]) - 3
    assert abs(got["spearman"] - (rx * ry).sum() / np.sqrt((rx * rx).sum() * (ry * ry).sum())) < 1e-15
    # the 10 pairs one by one:
    # (0,1) discordant; (0,2) (0,3) (0,4) concordant; (1,2) tied in x; (1,3) (1,4) concordant; (2,3) tied in y; (2,4) (3,4) concordant
    P, Q, T, U = 7, 1, 1, 1
    assert abs(got["kendall"] - (P - Q) / np.sqrt((P + Q + T) * (P + Q + U))) < 1e-15
    assert got["n"] == 5
    # fewer than two entries, or none finite in both
    assert np.isnan(flexibility_correlation([1.0], [2.0])["pearson"])
    none = flexibility_correlation([np.nan, 1.0], [1.0, np.nan])
    assert none["n"] == 0 and np.isnan([none["pearson"], none["spearman"], none["kendall"]]).all()
    # a perfect monotone relation
    mono = flexibility_correlation(np.arange(6.0), np.arange(6.0) ** 3)
    assert mono["spearman"] == 1.0 and mono["kendall"] == 1.0 and mono["pearson"] < 1.0


def test_apo_summary_against_the_statistics_computed_directly():
    from esmdiff_amd.flexibility import apo_summary
    rng = np.random.default_rng(2)
    reports = []
    for k in range(5):
        L = 20 + 3 * k
        rmsd = np.abs(rng.normal(size=L))
        rmsf = 0.5 * rmsd + np.abs(rng.normal(size=L)) * 0.7
        rmsd[k], rmsf[L - 1 - k] = np.nan, np.nan                 # unresolved residues, different on the two sides
        reports.append({"tm1max": 0.8, "tm2max": 0.7, "tm_ens": float(rng.uniform(0.5, 0.9)), "ensvar": float(rng.uniform(0.6, 0.95)),
                        "tmpair": float(rng.uniform(0.5, 0.95)), "rmsd": rmsd, "rmsf": rmsf})
    reports.append({"tm1max": 0.8, "tm2max": 0.7, "tm_ens": 0.75, "ensvar": 0.8, "tmpair": 0.9, "rmsd": np.ones(8),
                    "rmsf": np.abs(rng.normal(size=8))})           # a constant profile: no per-target r, left out of mean / median
    full = apo_summary(reports, rounded=False)
    per = []
    for r in reports[:5]:
        ok = np.isfinite(r["rmsd"]) & np.isfinite(r["rmsf"])
        per.append(np.corrcoef(r["rmsd"][ok], r["rmsf"][ok])[0, 1])
    gx, gy = np.concatenate([r["rmsd"] for r in reports]), np.concatenate([r["rmsf"] for r in reports])
    ok = np.isfinite(gx) & np.isfinite(gy)
    want = {"tm_correlation": np.corrcoef([r["ensvar"] for r in reports], [r["tmpair"] for r in reports])[0, 1],
            "rmsd_global": np.corrcoef(gx[ok], gy[ok])[0, 1], "rmsd_pt_mean": np.mean(per), "rmsd_pt_median": np.median(per),
            "tm_ens_mean": np.mean([r["tm_ens"] for r in reports]), "tm_ens_median": np.median([r["tm_ens"] for r in reports])}
    for k, v in want.items():
        np.testing.assert_allclose(full[k], v, rtol=0, atol=1e-12, err_msg=k)
    assert len(full["per_target"]) == 6 and np.isnan(full["per_target"][5]["pearson"])
    np.testing.assert_allclose([t["pearson"] for t in full["per_target"][:5]], per, rtol=0, atol=1e-12)
    assert full["per_target"][0]["n"] == 18
    rounded = apo_summary(reports)
    for k, v in want.items():
        assert rounded[k] == round(float(v), 3), k


# ---- binding and failure modes -----------------------------------------------------------------------------------------------------
def test_the_three_entries_are_declared_bound_and_built():
    from esmdiff_amd import _native, build
    header = (ROOT / "include" / "esmdiff_hip.h").read_text()
    declared = re.findall(r"\b(esmdiff_[a-z0-9_]+)\s*\(", header)
    for name in ("esmdiff_flex_pair_msf", "esmdiff_flex_fit", "esmdiff_flex_moments"):
        assert declared.count(name) == 1 and name in _native.EXPORTS, name
    assert re.search(r"#define ESMDIFF_ABI_VERSION 8\b", header)
    assert "flex" in build.UNITS and (ROOT / "esmdiff_amd" / "csrc" / "flex.hip").exists()
    # the rotation code is shared, not copied: one definition, in the header both units include
    csrc = ROOT / "esmdiff_amd" / "csrc"
    assert "kabsch_rotation(const double* h" in (csrc / "ed_kabsch.h").read_text()
    for unit in ("superpose.hip", "flex.hip"):
        text = (csrc / unit).read_text()
        assert '#include "ed_kabsch.h"' in text and "void kabsch_rotation(" not in text, unit
    # the scratch rule of the header's macro, restated in the binding: 4 slots per workgroup, 2048 workgroups wanted, 16 chunks at most
    assert [_native.flex_pair_slots(n) for n in (1, 2, 5, 100, 1000, 4096, 4097, 16384)] == [64, 64, 192, 3200, 8000, 8192, 8196, 32768]


def test_cli_takes_flex():
    from esmdiff_amd import analyze_ensemble
    assert "--flex" in analyze_ensemble.__doc__ and "--pca_components" in analyze_ensemble.__doc__
    args = analyze_ensemble.parser().parse_args(["--samples", "s.pdb", "--targets", "a.pdb", "b.pdb", "--output", "o", "--flex"])
    assert args.flex and args.pca_components == 3
    args = analyze_ensemble.parser().parse_args(["--samples", "s.pdb", "--targets", "a.pdb", "--output", "o"])
    assert not args.flex


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_no_cpu_fallback():
    from esmdiff_amd import flexibility
    A = E.ensemble(np.random.default_rng(0), 4, 6)
    for call in (lambda: flexibility.pair_rmsf(A), lambda: flexibility.mean_structure(A), lambda: flexibility.rmsf(A),
                 lambda: flexibility.pca(A)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    p = flexibility.PCA(np.ones(1), np.ones(1), np.zeros((1, 6, 3)), np.zeros((4, 1)), A[0], np.arange(6))
    for call in (lambda: p.project(A), lambda: p.displacement_overlap(A[0], A[1])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()

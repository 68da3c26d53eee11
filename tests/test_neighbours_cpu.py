"""tests/neighbours_ref.py against tests/ensemble_ref.py (and scipy where it is installed), and the host logic of
esmdiff_amd.neighbours.coverage on hand-made minima.  No device."""
import numpy as np
import pytest

from tests import ensemble_ref, neighbours_ref as ref


@pytest.mark.parametrize("reflection", [False, True])
def test_direct_msd_is_ensemble_refs(reflection):
    rng = np.random.default_rng(0)
    A, B = ref.chains(rng, 4, 23), ref.chains(rng, 5, 23)
    B[2] = (A[1] * np.array([1.0, 1.0, -1.0])) @ ref.rotation(rng).T      # a mirror image
    rmsd, _, _, _ = ensemble_ref.superpose_pairs(A, B, allow_reflection=reflection)
    got = ref.msd_direct(A, B, None, reflection)
    assert (np.abs(got - rmsd ** 2) <= ref.bar(A, B)).all()
    assert (got[1, 2] < 1e-20) == reflection


def test_direct_msd_is_scipys():
    transform = pytest.importorskip("scipy.spatial.transform")
    rng = np.random.default_rng(1)
    A, B = ref.chains(rng, 3, 17), ref.chains(rng, 3, 17)
    got = ref.msd_direct(A, B)
    for i in range(3):
        for j in range(3):
            a, b = A[i] - A[i].mean(0), B[j] - B[j].mean(0)
            _, rssd = transform.Rotation.align_vectors(b, a)
            assert abs(got[i, j] - rssd ** 2 / 17) <= 1e-9 * (1 + got[i, j])


def test_gram_form_is_within_13u_of_the_direct_form():
    """numpy's own Gram form lies well inside the bar the device is held to."""
    rng = np.random.default_rng(2)
    worst = 0.0
    for L in (4, 58, 300):
        for noise in (1e-6, 1e-2, 10.0):
            A = ref.chains(rng, 6, L)
            B = np.stack([a @ ref.rotation(rng).T + rng.normal(size=a.shape) * noise for a in A])
            pa, pb = ref.prepare(A), ref.prepare(B)
            H = np.einsum("irl,jcl->ijrc", pa["P"], pb["P"])
            s = np.linalg.svd(H, compute_uv=False)
            sign = np.where(np.linalg.det(H) < 0, -1.0, 1.0)
            gram = np.maximum(0.0, (pa["info"][:, None, 3] + pb["info"][None, :, 3] - 2 * (s[..., 0] + s[..., 1] + sign * s[..., 2])) / L)
            worst = max(worst, float((np.abs(gram - ref.msd_direct(A, B)) / ref.bar(A, B)).max()))
    assert worst <= 1.0, worst


def test_prepare_restates_centroid_and_g():
    rng = np.random.default_rng(3)
    X = ref.chains(rng, 5, 131)
    sel = rng.random(131) < 0.7
    X[3, np.flatnonzero(sel)[4], 1] = np.nan
    X[:, ~sel] = np.nan
    p = ref.prepare(X, sel)
    N = int(sel.sum())
    assert p["n_sel"] == N and p["P"].shape == (5, 3, ref.padded(N)) and list(p["use"]) == [1, 1, 1, 0, 1]
    ok = p["use"].astype(bool)
    c = X[ok][:, sel].mean(1)
    assert np.allclose(p["info"][ok, :3], c, rtol=0, atol=1e-12)
    assert np.allclose(p["info"][ok, 3], ((X[ok][:, sel] - c[:, None]) ** 2).sum((1, 2)), rtol=1e-13)
    assert (p["P"][~ok] == 0).all() and (p["info"][~ok] == 0).all() and (p["P"][:, :, N:] == 0).all()
    assert np.allclose(np.transpose(p["P"][ok][:, :, :N], (0, 2, 1)), X[ok][:, sel] - c[:, None], atol=1e-12)


def test_exact_restatement_and_sums():
    rng = np.random.default_rng(4)
    X = rng.integers(-9, 10, size=(3, 8, 3))
    X[:, -1] += (-X.sum(1)) % 8
    ca, ga, cb, gb, cross = ref.exact(X, X)
    p = ref.prepare(X.astype(np.float64))
    assert (p["info"][:, :3] == ca).all() and (p["info"][:, 3] == ga).all()
    assert (np.einsum("irl,jcl->ijrc", p["P"], p["P"]).reshape(3, 3, 9) == cross).all()

    r = rng.random((ref.RECT + 5, 2 * ref.RECT + 3))
    ua, ub = np.ones(r.shape[0], bool), np.ones(r.shape[1], bool)
    ua[2], ub[ref.RECT] = False, False
    rows, cols = ref.fold_sums(r, ua, ub)
    assert rows[2] == 0 and cols[ref.RECT] == 0
    assert np.allclose(rows[ua], r[:, ub].sum(1)[ua], rtol=1e-13) and np.allclose(cols[ub], r[ua].sum(0)[ub], rtol=1e-13)
    s = r[:, :r.shape[0]] + r[:, :r.shape[0]].T
    rows, none = ref.fold_sums(s, ua, None)
    assert none is None and np.allclose(rows[ua], (s - np.diag(np.diag(s)))[:, ua].sum(1)[ua], rtol=1e-13)


def test_gaps_and_clearance():
    msd = np.array([[1.0, 4.0, np.nan], [9.0, 2.0, np.nan]])
    rg, cg = ref.gaps(msd)
    assert list(rg) == [3.0, 7.0] and list(cg[:2]) == [8.0, 2.0] and np.isinf(cg[2])
    ref.assert_clear(msd, 0.1, [1.5, 2.5])
    with pytest.raises(AssertionError):
        ref.assert_clear(msd, 0.1, [2.01])                # 2.01^2 = 4.04 is within 0.1 of 4
    with pytest.raises(AssertionError):
        ref.assert_separated(np.array([[1.0, 1.1], [5.0, 9.0]]), 0.1)


def test_coverage_on_hand_made_minima():
    from esmdiff_amd.neighbours import Neighbours, coverage_from
    # three samples (one unused), four frames (one unused); cutoffs 1 and 2
    nb = Neighbours(rmsd_a=np.array([0.5, np.nan, 2.5]), index_a=np.array([0, -1, 3], np.int32),
                    rmsd_b=np.array([0.5, 1.5, np.nan, 2.5]), index_b=np.array([0, 0, -1, 2], np.int32),
                    count_a=np.array([[1, 2], [0, 0], [0, 0]]), count_b=np.array([[1, 1], [0, 1], [0, 0], [0, 0]]),
                    sum_a=np.zeros(3), sum_b=np.zeros(4), pairs_a=np.array([3, 0, 3]), pairs_b=np.array([2, 2, 0, 2]),
                    used_a=np.array([True, False, True]), used_b=np.array([True, True, False, True]), hist=None, edges=None, n_pairs=6,
                    select=np.ones(5, bool), cutoffs=(1.0, 2.0))
    c = coverage_from(nb)
    assert c["recall"] == [1 / 3, 2 / 3] and c["precision"] == [0.5, 0.5]
    assert c["mat_r"] == pytest.approx((0.5 + 1.5 + 2.5) / 3) and c["mat_p"] == pytest.approx(1.5)
    assert list(c["novel"]) == [2] and [list(u) for u in c["unrecalled"]] == [[1, 3], [3]]
    assert c["samples_used"] == 2 and c["samples_dropped"] == 1 and c["frames_used"] == 3 and c["frames_dropped"] == 1
    assert np.allclose(c["density"][[0, 2]], [[1 / 3, 2 / 3], [0, 0]]) and np.isnan(c["density"][1]).all()
    w = coverage_from(nb, weights=np.array([0.1, 0.2, 5.0, 0.7]))
    assert w["recall"] == pytest.approx([0.1, 0.3]) and w["mat_r"] == pytest.approx(0.05 + 0.3 + 1.75) and w["precision"] == c["precision"]
    with pytest.raises(ValueError, match="weights"):
        coverage_from(nb, weights=np.ones(3))


def test_command_line_without_the_flag_is_unchanged(tmp_path, monkeypatch):
    import json
    from esmdiff_amd import analyze_ensemble
    stub = {"TM-ens": 0.5, "best_tm": np.array([0.25, 0.75]), "flex": {"rmsf": np.array([1.0, np.nan])}}
    monkeypatch.setattr(analyze_ensemble, "analyze", lambda *a, **k: dict(stub))
    calls = []
    monkeypatch.setattr(analyze_ensemble, "coverage_report", lambda *a: calls.append(a) or {"recall": [0.5, np.nan], "novel": np.array([3])})
    args = ["--samples", "ens.pdb", "--targets", "a.pdb", "--output"]
    plain = analyze_ensemble.main(args + [str(tmp_path / "plain")])
    assert not calls
    assert plain.read_text() == '{\n "TM-ens": 0.5,\n "best_tm": [\n  0.25,\n  0.75\n ],\n "flex": {\n  "rmsf": [\n   1.0,\n   null\n  ]\n }\n}\n'
    full = analyze_ensemble.main(args + [str(tmp_path / "cov"), "--coverage", "--trajectory", "ref.npy", "--coverage_cutoffs", "0.5", "4",
                                         "--tica_chunk", "16"])
    data = json.loads(full.read_text())
    assert data.pop("coverage") == {"recall": [0.5, None], "novel": [3]} and json.dumps(data, indent=1) + "\n" == plain.read_text()
    assert calls == [("ens.pdb", ["a.pdb"], "ref.npy", 100, 0, [0.5, 4.0], 16)]
    with pytest.raises(SystemExit):
        analyze_ensemble.main(args + [str(tmp_path / "bad"), "--coverage"])
    p = analyze_ensemble.parser().parse_args(args + ["o"])
    assert (p.coverage, p.coverage_cutoffs) == (False, [1.0, 2.0, 3.0])
    assert "--coverage" in analyze_ensemble.__doc__


def test_argument_validation():
    from esmdiff_amd import neighbours
    with pytest.raises(ValueError, match="empty list"):
        neighbours.nearest([])
    with pytest.raises(ValueError, match="at least 2"):
        neighbours.nearest(np.zeros((3, 5, 3)), select=np.array([True, False, False, False, False]))
    with pytest.raises(ValueError, match="different lengths"):
        neighbours.nearest(np.zeros((3, 5, 3)), np.zeros((3, 6, 3)))
    with pytest.raises(ValueError, match="cutoffs"):
        neighbours.nearest(np.zeros((3, 5, 3)), cutoffs=range(9))
    with pytest.raises(ValueError, match="hist_max"):
        neighbours.nearest(np.zeros((3, 5, 3)), hist_bins=10)
    with pytest.raises(ValueError, match="select"):
        neighbours.nearest(np.zeros((3, 5, 3)), select=np.ones(4, bool))

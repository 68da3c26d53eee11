"""GPU tests of the lDDT layer (esmdiff_amd/csrc/lddt.hip through the C ABI, esmdiff_amd/ensemble.py, esmdiff_amd/clustering.py and
the two command lines) against the numpy float64 restatement tests/lddt_ref.py (itself held to a hand-worked case by
tests/test_lddt_cpu.py).  The device outputs are integers: every comparison of counts is exact.  No network engine is built."""
import ctypes
import json

import numpy as np
import pytest

from tests import cluster_ref as C
from tests import lddt_ref as R

pytestmark = pytest.mark.gpu

T1 = (2.0,)
T8 = (0.25, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _call(A, B, maskA=None, maskB=None, r0=R.R0, thresholds=R.THRESHOLDS, seq_sep=1, per_residue=True, n=None, m=None, L=None,
          n_thr=None):
    """esmdiff_lddt_pairs on numpy inputs -> (code, kept, total, kept_res, total_res); the outputs start as -7 everywhere."""
    import torch
    from esmdiff_amd import _native as N
    dev = lambda x, dt: None if x is None else torch.as_tensor(np.ascontiguousarray(x, dtype=dt)).cuda()
    a, b = dev(A, np.float64), dev(B, np.float64)
    ma, mb = dev(maskA, np.uint8), dev(maskB, np.uint8)
    n = A.shape[0] if n is None else n
    m = (A if B is None else B).shape[0] if m is None else m
    L = A.shape[1] if L is None else L
    rows, cols, width = max(n, 1), max(m, 1), min(max(L, 1), A.shape[1])
    kept = torch.full((rows, cols), -7, dtype=torch.int32, device="cuda")
    total = torch.full((cols,), -7, dtype=torch.int32, device="cuda")
    kept_res = torch.full((rows, cols, width), -7, dtype=torch.int32, device="cuda") if per_residue else None
    total_res = torch.full((cols, width), -7, dtype=torch.int32, device="cuda") if per_residue else None
    thr = (ctypes.c_double * len(thresholds))(*thresholds)
    code = N.lib().esmdiff_lddt_pairs(_p(a), n, _p(b), m, L, _p(ma), _p(mb), r0, thr, len(thresholds) if n_thr is None else n_thr,
                                      seq_sep, _p(kept), _p(total), _p(kept_res), _p(total_res), None)
    torch.cuda.synchronize()
    out = [None if t is None else t.cpu().numpy() for t in (kept, total, kept_res, total_res)]
    return (code, *out)


def _exact(got, want, tag):
    assert got[0] == 0, tag
    for name, g, w in zip(("kept", "total", "kept_res", "total_res"), got[1:], want):
        if g is not None:
            assert g.dtype == np.int32 and g.shape == w.shape and np.array_equal(g, w), f"{tag}: {name}"


def _inputs(seed, n, m, L):
    rng = np.random.default_rng(seed)
    base = R.chain(rng, L)
    return R.ensemble(rng, n, base), R.ensemble(rng, m, base, 0.0, 1.5), rng


# ---- 1. random shapes, exact ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [2, 3, 5, 63, 64, 65, 130])
def test_counts_equal_the_restatement(L):
    """Random-walk chains (3.8 A steps) plus noise of 0 to 2.5 A: both sides of R0 and of every threshold are populated, which the
    test asserts on the reference's own counts — per threshold, for the plain, the masked and the seq_sep = 3 inputs — wherever a
    chain has the pairs for it (L >= 63).  L = 2, 3, 5 have 1 to 10 residue pairs, all inside R0 (3.8 A steps): a single case
    there cannot sit on both sides of eight thresholds, so those lengths are held to the restatement without that assertion."""
    for n, m in ((1, 1), (3, 7), (7, 3)):
        A, B, rng = _inputs(1000 * L + 10 * n + m, n, m, L)
        if L >= 63:
            idx = np.arange(L)
            for j in range(m):
                inside = (R.distances(B[j]) < R.R0)[np.abs(idx[:, None] - idx[None, :]) >= 1]
                assert 0.02 < inside.mean() < 0.98, "a good share of the native's pairs on each side of R0"
        masks = [(None, None), (rng.random((n, L)) > 0.2, rng.random((m, L)) > 0.2)]
        if L >= 63:
            for ma, mb in masks:
                for seq_sep in (1, 3):
                    for t in sorted(set(T8 + R.THRESHOLDS)):
                        kept, total, _, _ = R.counts(A, B, ma, mb, R.R0, (t,), seq_sep)
                        assert 0 < kept.sum() < np.broadcast_to(total, kept.shape).sum(), f"threshold {t}: all kept or none kept"
        for ma, mb in masks:
            for seq_sep in (1, 3):
                for thr in (T1, R.THRESHOLDS, T8):
                    want = R.counts(A, B, ma, mb, R.R0, thr, seq_sep)
                    _exact(_call(A, B, ma, mb, R.R0, thr, seq_sep), want, f"L={L} n={n} m={m} masks={ma is not None} sep={seq_sep} nt={len(thr)}")


def test_self_comparison_and_masked_coordinates_are_never_read():
    A, _, rng = _inputs(7, 5, 1, 65)
    ma = rng.random((5, 65)) > 0.25
    want = R.counts(A, None, ma)
    holes = A.copy()
    holes[~ma] = np.nan                                          # NaN under the mask changes nothing
    _exact(_call(holes, None, ma), want, "B == NULL")
    _exact(_call(holes, holes, ma, ma), want, "B == A")
    full = _call(A, None)
    assert np.array_equal(np.diag(full[1]), 4 * full[2])        # a structure against itself keeps every pair at every threshold


# ---- 2. ties: both comparisons are strict ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_ties_on_a_lattice(axis):
    """Coordinates on a 1/8 A lattice along one axis: every distance is exact.  A native distance of exactly 15.0 is outside the
    radius, 14.875 inside; a model difference of exactly 0.5, 1, 2, 4 is not kept under that threshold, one lattice step less is."""
    def line(xs):
        out = np.zeros((len(xs), 3))
        out[:, axis] = xs
        return out

    native = line([0, 15.0, 29.875])[None]
    got = _call(native, native)
    assert got[0] == 0 and got[4].tolist() == [[0, 1, 1]] and got[2].tolist() == [2] and got[1].tolist() == [[8]]
    deltas = (0.5, 1, 2, 4, 0.375, 0.875, 1.875, 3.875, -0.5, -1, -2, -4, -0.375, -0.875, -1.875, -3.875)
    models = np.stack([line([0, 10 + d]) for d in deltas])
    got = _call(models, line([0, 10])[None])
    assert got[0] == 0 and got[1][:, 0].tolist() == [6, 4, 2, 0, 8, 6, 4, 2] * 2 and got[2].tolist() == [2]
    assert got[3].reshape(16, 2).tolist() == [[k // 2, k // 2] for k in got[1][:, 0]]
    _exact(got, R.counts(models, line([0, 10])[None]), "the restatement agrees")


# ---- 3. rigid motions ---------------------------------------------------------------------------------------------------------------
def test_rigid_motions_of_lattice_coordinates_change_nothing():
    """Chains on the 1/8 A lattice, 90-degree rotations about the axes, integer translations, permutations of x, y, z: every squared
    distance is exact before and after, so the integers are identical — and the model and the native may move independently."""
    rng = np.random.default_rng(5)

    def lattice(k, L):
        return np.cumsum(rng.integers(-20, 21, size=(k, L, 3)) / 8.0, axis=1)          # steps up to 2.5 A per axis

    A, B = lattice(3, 40), lattice(2, 40)
    B[1] = A[0] + rng.integers(-6, 7, size=(40, 3)) / 8.0
    want = R.counts(A, B)
    assert 0 < want[0].sum() < 4 * want[1].sum() * 3
    first = _call(A, B)
    _exact(first, want, "as given")
    rot_z = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], float)
    rot_x = np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]], float)
    rot_y = np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0]], float)
    moves = [(rot_z, [3, -7, 11], rot_x, [0, 0, 0]), (rot_x @ rot_y, [-20, 5, 1], rot_z @ rot_z, [9, 9, -4]),
             (np.eye(3)[[1, 2, 0]], [0, 0, 0], np.eye(3)[[2, 0, 1]], [1, 2, 3]), (np.eye(3)[[2, 1, 0]], [0, 0, 0], np.eye(3)[[0, 2, 1]], [0, 0, 0])]
    for ra, ta, rb, tb in moves:
        got = _call(A @ ra.T + np.array(ta, float), B @ rb.T + np.array(tb, float))
        for g, f in zip(got, first):
            assert np.array_equal(g, f)


# ---- 4. tiling ------------------------------------------------------------------------------------------------------------------------
def test_long_chain():
    """L = 1026: 17 steps of 64 per row with a ragged last one, rows split over row chunks, 24 KiB of LDS per model."""
    A, B, rng = _inputs(1026, 2, 2, 1026)
    ma, mb = rng.random((2, 1026)) > 0.1, rng.random((2, 1026)) > 0.1
    _exact(_call(A, B, ma, mb), R.counts(A, B, ma, mb), "L=1026")


def test_more_models_than_a_tile_and_two_runs_bit_identical():
    A, B, _ = _inputs(70, 70, 3, 20)
    first = _call(A, B)
    _exact(first, R.counts(A, B), "n=70")
    A2, B2, rng = _inputs(130, 7, 3, 130)
    ma = rng.random((7, 130)) > 0.2
    one, two = _call(A2, B2, ma), _call(A2, B2, ma)
    for g, f in zip(one, two):
        assert np.array_equal(g, f)


# ---- 5. error codes ------------------------------------------------------------------------------------------------------------------
def test_error_codes_and_null_per_residue_outputs():
    from esmdiff_amd import _native as N
    A, B, _ = _inputs(9, 2, 3, 12)
    assert _call(A, B, n=0)[0] == -1 and _call(A, B, m=0)[0] == -1 and _call(A, B, L=1)[0] == -1
    assert _call(A, B, seq_sep=0)[0] == -1 and _call(A, B, n_thr=0)[0] == -1 and _call(A, B, thresholds=T8, n_thr=9)[0] == -1
    assert _call(A, B, L=N.LDDT_MAX_L + 1)[0] == -5             # refused before anything is launched or read
    got = _call(A, B, per_residue=False)
    assert got[3] is None and got[4] is None
    _exact(got, R.counts(A, B), "null kept_res / total_res")


# ---- 6. the Python layer ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ens():
    from esmdiff_amd import ensemble
    return ensemble


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(2024)
    base = R.chain(rng, 30)
    S, K = R.ensemble(rng, 9, base, 0.1, 2.0), R.ensemble(rng, 3, base, 0.0, 0.5)
    K[2, 4] = np.nan                                             # an unresolved native residue
    score, per_res = R.scores(S, K, maskB=~np.isnan(K).any(-1))
    return S, K, score, per_res


def test_lddt_matrix(ens, data):
    S, K, score, per_res = data
    got, got_res = ens.lddt_matrix(S, K, per_residue=True)
    assert got.shape == (9, 3) and got_res.shape == (9, 3, 30) and got.dtype == got_res.dtype == np.float64
    assert np.isnan(per_res[:, 2, 4]).all() and np.array_equal(np.isnan(got_res), np.isnan(per_res))
    assert np.nanmax(np.abs(got_res - per_res)) <= 1e-15 and np.max(np.abs(got - score)) <= 1e-15
    assert np.max(np.abs(ens.lddt_matrix(S, K) - score)) <= 1e-15
    assert abs(ens.lddt(S[3], K[1]) - score[3, 1]) <= 1e-15
    # options reach the kernel
    mask = np.random.default_rng(1).random((9, 30)) > 0.3
    want = R.scores(S, K[:2], maskA=mask, r0=12.0, thresholds=T8, seq_sep=2)[0]
    assert np.max(np.abs(ens.lddt_matrix(S, K[:2], mask_models=mask, r0=12.0, thresholds=T8, seq_sep=2) - want)) <= 1e-15
    # natives = None: the models against themselves; a native without any pair is NaN
    assert np.max(np.abs(ens.lddt_matrix(S) - R.scores(S)[0])) <= 1e-15
    far = np.array([[0.0, 0, 0], [20.0, 0, 0]])
    assert np.isnan(ens.lddt(far, far))
    with pytest.raises(RuntimeError, match="4096"):
        ens.lddt_matrix(np.zeros((1, 4097, 3)))
    with pytest.raises(RuntimeError, match="seq_sep"):
        ens.lddt_matrix(S, seq_sep=0)


def test_ensemble_scores(ens, data):
    S, K, score, _ = data
    assert abs(ens.lddt_ensemble(S, K) - np.mean(score.max(0))) <= 1e-15
    l = R.scores(S)[0]
    iu = np.triu_indices(9, 1)
    assert abs(ens.lddt_diversity(S) - np.mean(0.5 * (l + l.T)[iu])) <= 1e-15
    rng = np.random.default_rng(8)
    plddt = np.round(rng.uniform(20, 95, size=(9, 30)), 2)
    got = ens.plddt_agreement(S, K[2], plddt, scale=100.0)
    res = R.scores(S, K[2:3], maskB=~np.isnan(K[2:3]).any(-1))[1][:, 0]
    observed, predicted = res.mean(0), (plddt / 100.0).mean(0)
    ok = np.isfinite(observed)
    assert not ok[4] and ok.sum() == 29
    assert np.array_equal(np.isnan(got["observed"]), ~ok) and np.max(np.abs(got["observed"][ok] - observed[ok])) <= 1e-15
    assert np.max(np.abs(got["predicted"] - predicted)) <= 1e-15
    assert abs(got["pearson_r"] - np.corrcoef(observed[ok], predicted[ok])[0, 1]) <= 1e-12
    assert abs(got["mean_abs_diff"] - np.mean(np.abs(observed[ok] - predicted[ok]))) <= 1e-15


def test_clustering_with_lddt(data):
    from esmdiff_amd import clustering
    rng = np.random.default_rng(77)
    states = [R.chain(rng, 24) for _ in range(3)]
    S = np.stack([states[k] + rng.normal(size=(24, 3)) * s for k, s in zip((0, 1, 0, 2, 1, 0, 0, 2, 1, 0, 1, 0, 2), np.linspace(0.1, 0.6, 13))])
    l = R.scores(S)[0]
    sym = 0.5 * (l + l.T)
    for cutoff in (0.6, 0.8):
        want = C.cluster_matrix(sym, cutoff, larger_is_closer=True)
        for block_rows in (1024, 5):
            got = clustering.cluster_ensemble(S, cutoff, metric="lddt", block_rows=block_rows)
            assert got.n_clusters == want[3] and np.array_equal(got.labels, want[0])
            assert np.array_equal(got.centres, want[1]) and np.array_equal(got.sizes, want[2])
    assert 1 < want[3] < 13
    got = clustering.cluster_ensemble(S, 0.8, metric="lddt")
    d = clustering.centre_distances(S, got, metric="lddt")
    assert np.max(np.abs(d - sym[np.arange(13), got.centres[got.labels]])) <= 1e-15
    K = np.stack(states)
    lk, kl = R.scores(S, K)[0], R.scores(K, S)[0]
    to_states = 0.5 * (lk + kl.T)
    assignment, populations, distance = clustering.state_populations(S, K, metric="lddt")
    assert np.array_equal(assignment, to_states.argmax(1)) and np.max(np.abs(distance - to_states.max(1))) <= 1e-15
    assert np.array_equal(populations, np.bincount(to_states.argmax(1), minlength=3) / 13)


def test_command_lines(tmp_path):
    from esmdiff_amd import analyze_ensemble, cluster_ensemble, pdbio
    rng = np.random.default_rng(31)
    states = [R.chain(rng, 24) for _ in range(3)]
    conf = np.round(rng.uniform(0.3, 0.95, size=(8, 24)), 2)

    def write(path, ca, b=None):
        bb = np.stack([ca + np.array([-0.5, 1.2, 0.3]), ca, ca + np.array([1.1, 0.9, -0.4])], axis=1)
        pdbio.write_backbone_pdb(path, "A" * len(ca), bb, bfactor=b)

    files = []
    for i, k in enumerate((0, 1, 0, 2, 1, 0, 0, 2)):
        files.append(tmp_path / f"s_{i}.pdb")
        write(files[-1], states[k] + rng.normal(size=(24, 3)) * 0.3, conf[i])
    samples_path = tmp_path / "t7.pdb"
    pdbio.merge_pdbfiles(files, samples_path, verbose=False)
    targets = []
    for k in range(3):
        targets.append(tmp_path / f"state_{k}.pdb")
        write(targets[-1], states[k])
    S = pdbio.load_coords(samples_path, max_n_model=None, verbose=False).astype(np.float64)
    K = np.stack([pdbio.load_coords(t, max_n_model=None, verbose=False)[0] for t in targets]).astype(np.float64)
    l = R.scores(S)[0]
    sym = 0.5 * (l + l.T)

    json_path, pdb_path = cluster_ensemble.main(["--samples", str(samples_path), "--cutoff", "0.7", "--output", str(tmp_path / "c"),
                                                 "--metric", "lddt"])
    doc = json.loads(json_path.read_text())
    want = C.cluster_matrix(sym, 0.7, larger_is_closer=True)
    assert doc["metric"] == "lddt" and doc["n"] == 8 and doc["n_clusters"] == want[3] and "tm_score" not in doc
    assert doc["labels"] == want[0].tolist() and doc["centres"] == want[1].tolist() and doc["sizes"] == want[2].tolist()
    dist = 1.0 - sym[np.arange(8), want[1][want[0]]]
    assert np.allclose(doc["max_distance"], [dist[want[0] == k].max() for k in range(want[3])], rtol=0, atol=1e-15)
    assert pdbio.load_coords(pdb_path, max_n_model=None, verbose=False).shape == (want[3], 24, 3)

    path = analyze_ensemble.main(["--samples", str(samples_path), "--targets", *map(str, targets), "--output", str(tmp_path / "a"), "--lddt"])
    doc = json.loads(path.read_text())
    score, per_res = R.scores(S, K)
    assert {"best_tm", "best_rmsd", "TM-ens", "RMSD-ens", "TM-div", "lddt_ens", "lddt_div", "best_lddt", "best_lddt_model",
            "best_lddt_residue", "plddt_agreement"} == set(doc)
    assert abs(doc["lddt_ens"] - np.mean(score.max(0))) <= 1e-15
    assert abs(doc["lddt_div"] - np.mean(sym[np.triu_indices(8, 1)])) <= 1e-15
    assert doc["best_lddt_model"] == score.argmax(0).tolist()
    for k in range(3):
        assert np.allclose(doc["best_lddt_residue"][k], per_res[score.argmax(0)[k], k], rtol=0, atol=1e-15)
        block = doc["plddt_agreement"][k]
        assert set(block) == {"observed", "predicted", "pearson_r", "mean_abs_diff"}
        assert np.allclose(block["observed"], per_res[:, k].mean(0), rtol=0, atol=1e-15)
        assert np.allclose(block["predicted"], conf.mean(0), rtol=0, atol=1e-15)
        assert abs(block["pearson_r"] - np.corrcoef(per_res[:, k].mean(0), conf.mean(0))[0, 1]) <= 1e-12
    # without --lddt the document is what it was
    path = analyze_ensemble.main(["--samples", str(samples_path), "--targets", *map(str, targets), "--output", str(tmp_path / "b")])
    assert set(json.loads(path.read_text())) == {"best_tm", "best_rmsd", "TM-ens", "RMSD-ens", "TM-div"}

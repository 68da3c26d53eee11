"""The host side of the covariance layer: the declarations and macros of esmdiff_flex_transforms and the two entries of csrc/aligned.hip
against esmdiff_amd/_native.py, the numpy restatement tests/aligned_ref.py against plain numpy, the Bures distance against closed forms
and scipy.linalg.sqrtm, the pooled moments against the concatenated frames, projection_w2 against scipy.stats, RMSIP, the comparisons of
esmdiff_amd/covariance.py on restated moments (they are device-agnostic torch) against the definitions on frames, and the command
line without --compare.  No device."""
import json
import re
from pathlib import Path

import numpy as np
import pytest

from tests import aligned_ref as R

ROOT = Path(__file__).resolve().parent.parent
EPS = 2.0 ** -52


def _held(Xa, ref):
    """AlignedMoments of frames that ARE aligned (T = identity), from the restatement, on the host."""
    import torch
    from esmdiff_amd import covariance
    L = Xa.shape[1]
    mom = R.moments(Xa, None, None, ref.reshape(-1))
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64))
    return covariance.AlignedMoments(mom["count"], 0, T(ref), np.arange(L), L, T(mom["S"]), T(mom["r"]), np.zeros(len(Xa)))


def _frames(rng, n, L, scale=1.0, shift=0.0):
    """A base chain 40 A from the origin and n frames about it with a planted spectrum: standard deviations scale 0.75^i along random
    orthogonal directions (variance ratios of 0.56: gaps that n = 200 frames resolve)."""
    base = np.cumsum(rng.standard_normal((L, 3)) * 2.2, axis=0) + 40.0
    Q = np.linalg.qr(rng.standard_normal((3 * L, 3 * L)))[0]
    mix = (Q * (scale * 0.75 ** np.arange(3 * L))).T
    return base, base[None] + shift + (rng.standard_normal((n, 3 * L)) @ mix).reshape(n, L, 3)


def test_entries_are_declared_and_exported():
    from esmdiff_amd import _native as N
    from esmdiff_amd import build
    header = (ROOT / "include" / "esmdiff_hip.h").read_text()
    flat = re.sub(r"\s+", " ", header)
    decls = ("int esmdiff_flex_transforms(const double* A, int32_t n, int32_t L, const uint8_t* maskA, const double* ref, const uint8_t* mask_ref, "
             "double* T, double* rmsd, uint8_t* ok, void* stream);",
             "int esmdiff_aligned_moments(const double* X, int32_t n, int32_t L, const double* T, const uint8_t* use, const double* center, "
             "double* S, double* r, int64_t* count, void* scratch, int64_t scratch_bytes, void* stream);",
             "int esmdiff_aligned_project(const double* X, int32_t n, int32_t L, const double* T, const double* mean, const double* W, "
             "int32_t dim, double* Y, void* stream);")
    for d in decls:
        assert flat.count(d) == 1, d
    assert re.search(r"#define ESMDIFF_ABI_VERSION 8\b", header)
    pairs_text = (ROOT / "esmdiff_amd" / "pairs.py").read_text()
    for name in ("esmdiff_flex_transforms", "esmdiff_aligned_moments", "esmdiff_aligned_project"):
        assert N.EXPORTS.count(name) == 1 and pairs_text.count(f"N.lib().{name}(") == 1, name
    for wrapper in ("flex_transforms", "aligned_slots", "aligned_moments", "aligned_project"):
        assert f"\ndef {wrapper}(" in pairs_text, wrapper
    for macro, value, ref in (("MAX_L", N.ALIGNED_MAX_L, R.MAX_L), ("MAX_DIM", N.ALIGNED_MAX_DIM, R.MAX_DIM),
                              ("FRAME_CHUNK", N.ALIGNED_FRAME_CHUNK, R.FRAME_CHUNK)):
        assert re.search(r"#define ESMDIFF_ALIGNED_%s %d\b" % (macro, value), header) and value == ref, macro
    assert N.ALIGNED_MAX_L == N.TM_MAX_L == 1280 and N.ALIGNED_MAX_DIM == 16 and N.ALIGNED_FRAME_CHUNK % 32 == 0
    assert ("#define ESMDIFF_ALIGNED_MOMENTS_SCRATCH_BYTES(L, slots) \\\n  ((int64_t)(slots) * (9 * (int64_t)(L) * (int64_t)(L) + "
            "3 * (int64_t)(L)) * 8)") in header
    for L, slots in ((1, 1), (22, 3), (1280, 2)):
        assert N.aligned_scratch_bytes(L, slots) == R.scratch_bytes(L, slots) == slots * (3 * L * 3 * L + 3 * L) * 8
    assert 117e6 < N.aligned_scratch_bytes(1280, 1) < 119e6
    assert build.UNITS["aligned"] == ["-ffp-contract=off", "-fno-slp-vectorize"] and (ROOT / "esmdiff_amd" / "csrc" / "aligned.hip").is_file()
    source = (ROOT / "esmdiff_amd" / "csrc" / "aligned.hip").read_text()
    assert "__builtin_amdgcn_mfma_f64_16x16x4f64" in source and "(lane >> 4) + 4 * reg" in source and "atomicAdd(&s_total" in source
    assert source.count("atomic") == 1                                               # the integer count alone


def test_slots_fill_the_device_within_the_cap():
    from esmdiff_amd import _native as N
    from esmdiff_amd import pairs
    assert pairs.aligned_slots(256, 2) == 2 and pairs.aligned_slots(58, 782) == 342 and pairs.aligned_slots(512, 235) == 7
    assert pairs.aligned_slots(1280, 40) == 2 and N.aligned_scratch_bytes(1280, 2) <= pairs.ALIGNED_SCRATCH_CAP
    assert pairs.aligned_slots(1, 1) == 1
    # an ensemble of 250 frames at L = 256: two chunks of 78 tile pairs
    tiles = (3 * 256 + 63) // 64
    assert -(-250 // N.ALIGNED_FRAME_CHUNK) * (tiles * (tiles + 1) // 2) == 156


def test_the_restatement_against_plain_numpy():
    rng = np.random.default_rng(0)
    n, L = 2 * R.FRAME_CHUNK + 9, 5
    X = rng.standard_normal((n, L, 3)) * 3.0 + 40.0
    rot = np.stack([np.linalg.qr(rng.standard_normal((3, 3)))[0] for _ in range(n)])
    T = np.concatenate([rot.reshape(n, 9), rng.standard_normal((n, 3)) * 20.0], axis=1)
    F = R.features(X, T)
    assert np.abs(F.reshape(n, L, 3) - (np.einsum("ncd,nld->nlc", rot, X) + T[:, None, 9:])).max() < 1e-12
    assert np.array_equal(R.features(X, None), X.reshape(n, -1))
    use = rng.random(n) < 0.8
    c = F.mean(0) + 0.1
    mom = R.moments(X, T, use, c)
    assert mom["count"] == use.sum() and np.abs(mom["r"] - (F[use] - c).sum(0)).max() < 1e-9
    W = rng.standard_normal((3 * L, 3))
    assert np.abs(R.project(X, T, c, W) - (F - c) @ W).max() < 1e-10
    # integers through signed permutations stay integers, and the float64 restatement is then exact
    P = R.signed_permutations()
    assert P.shape == (24, 3, 3) and np.allclose(np.linalg.det(P), 1.0) and len({p.tobytes() for p in P}) == 24
    Xi = rng.integers(-512, 513, size=(n, L, 3)).astype(np.float64)
    Ti = np.concatenate([P[rng.integers(0, 24, n)].reshape(n, 9), rng.integers(-64, 65, size=(n, 3))], axis=1).astype(np.float64)
    ci = rng.integers(-8, 9, size=3 * L).astype(np.float64)
    exact = R.moments_int(Xi, Ti, use, ci)
    assert max(int(np.abs(exact[k]).max()) for k in ("S", "r")) < 2 ** 53
    real = R.moments(Xi, Ti, use, ci)
    assert np.array_equal(real["S"], exact["S"].astype(np.float64)) and np.array_equal(real["r"], exact["r"].astype(np.float64))
    assert real["count"] == exact["count"]
    # the transform restated: the fit of a moved copy recovers the reference
    ref = X[0]
    moved = np.stack([ref @ r.T + 5.0 for r in rot[:4]])
    Tm, rmsd, good = R.transforms(moved, np.ones((4, L), bool), ref, np.ones(L, bool))
    assert good.all() and rmsd.max() < 1e-10 and np.abs(R.features(moved, Tm) - ref.reshape(-1)).max() < 1e-10
    _, _, good = R.transforms(moved[:1], np.eye(1, L, dtype=bool), ref, np.ones(L, bool))
    assert not good[0]


def test_bures_closed_forms():
    from esmdiff_amd import covariance
    # THE BAR of the closed forms: an eigenvalue of A^1/2 B A^1/2 carries an absolute error of a few eps |A| |B| from the products and the
    # eigh, and its square root divides that by 2 sqrt(the eigenvalue) >= 2 sqrt(min A min B): d terms of eps kappa sqrt(|A| |B|), kappa
    # the larger condition number.  8 d kappa eps (tr A + tr B), with the spectra chosen (kappa = 6)
    rng = np.random.default_rng(1)
    Q = np.linalg.qr(rng.standard_normal((6, 6)))[0]
    A = (Q * np.arange(1.0, 7.0)) @ Q.T
    tol = lambda X, Y, kappa: 8 * len(X) * kappa * EPS * (np.trace(X) + np.trace(Y))
    assert covariance.bures(A, A) <= tol(A, A, 6.0)
    a, b = rng.random(5) + 0.2, rng.random(5) + 0.2
    assert abs(covariance.bures(np.diag(a), np.diag(b)) - ((np.sqrt(a) - np.sqrt(b)) ** 2).sum()) <= tol(np.diag(a), np.diag(b), 6.0)
    # an isotropic scaling B = s^2 A: (1 - s)^2 tr A
    for s in (0.5, 2.0, 3.0):
        assert abs(covariance.bures(A, s * s * A) - (1.0 - s) ** 2 * np.trace(A)) <= tol(A, s * s * A, 6.0)
    # batches over the leading dimensions, and symmetric in its arguments
    As, Bs = np.stack([A, np.diag(np.r_[a, 1.0])]), np.stack([4.0 * A, np.diag(np.r_[b, 1.0])])
    got = covariance.bures(As, Bs)
    assert got.shape == (2,) and abs(got[0] - np.trace(A)) <= tol(As[0], Bs[0], 6.0)
    assert abs(got[1] - ((np.sqrt(a) - np.sqrt(b)) ** 2).sum()) <= tol(As[1], Bs[1], 6.0)
    assert np.abs(covariance.bures(Bs, As) - got).max() <= 2 * tol(As[0], Bs[0], 6.0)
    assert covariance.bures(np.zeros((3, 3)), np.zeros((3, 3))) == 0.0
    # a pure translation: rmwd is its length, the variance part nothing
    base, X = _frames(rng, 50, 7)
    delta = np.array([1.5, -2.0, 0.5])
    m1, m2 = _held(X, base), _held(X + delta, base)
    w = covariance.rmwd(m1, m2)
    assert abs(w["rmwd"] - np.linalg.norm(delta)) < 1e-9 and abs(w["translation"] - np.linalg.norm(delta)) < 1e-9 and w["variance"] < 3.2e-6
    per = covariance.residue_w2(m1, m2)
    assert np.abs(per["translation"] - delta @ delta).max() < 1e-9 and per["variance"].max() < 1e-11 and per["w2_sq"].shape == (7,)


SQRTM_BOUND = {"3x3": 82.0, "2x2": 28.0, "30x30": 136.0, "rank_deficient": 3.3e8}     # ten times the measured figures of the docstring below


@pytest.mark.parametrize("case", ["3x3", "2x2", "30x30", "rank_deficient"])
def test_bures_against_sqrtm(case):
    """bures(A, B) against tr A + tr B - 2 tr sqrtm(sqrtm(A) B sqrtm(A)) with scipy.linalg.sqrtm.  The bound is ABSOLUTE, in units of
    eps (tr A + tr B): the three terms cancel, so no relative bound on the (possibly tiny) result can hold.  MEASURED on the host of
    this change, 20 seeds per case, of esmdiff_amd.covariance.bures and of the restatement, the largest |difference| /
    (eps (tr A + tr B)): 3x3 8.16, 2x2 2.76, 30x30 13.6, rank_deficient 3.28e7.  The last is 7e-9 (tr A + tr B), the square root of
    eps: a zero eigenvalue of A^1/2 B A^1/2 comes out of either eigensolver as +- eps |A| |B|, its root is 1e-8 sqrt(|A| |B|) when the
    sign is +, and sqrtm of a singular matrix is no better.  Each case asserts ten times its own figure."""
    sqrtm = pytest.importorskip("scipy.linalg").sqrtm
    from esmdiff_amd import covariance
    worst = 0.0
    for seed in range(20):
        rng = np.random.default_rng(seed)
        d = {"3x3": 3, "2x2": 2, "30x30": 30, "rank_deficient": 6}[case]
        rank = 3 if case == "rank_deficient" else d + 2
        G, H = rng.standard_normal((d, rank)), rng.standard_normal((d, d + 2))
        A, B = G @ G.T, H @ H.T
        root = np.real(sqrtm(A))
        want = np.trace(A) + np.trace(B) - 2.0 * np.trace(np.real(sqrtm(root @ B @ root)))
        worst = max(worst, abs(covariance.bures(A, B) - want) / (EPS * (np.trace(A) + np.trace(B))),
                    abs(R.bures(A, B) - want) / (EPS * (np.trace(A) + np.trace(B))))
    print(f"MEASURED bures vs sqrtm {case}: {worst:.3g} eps (tr A + tr B)")
    assert worst <= SQRTM_BOUND[case]


def test_pooled_moments_are_those_of_the_concatenated_frames():
    import torch
    from esmdiff_amd import covariance
    rng = np.random.default_rng(2)
    base, X1 = _frames(rng, 300, 6)
    _, X2 = _frames(rng, 200, 6, scale=1.7, shift=0.3)
    X2 = X2 - X2.mean(0) + base + 0.3
    m1, m2 = _held(X1, base), _held(X2, base)
    both = covariance.pooled(m1, m2)
    Xc = np.concatenate([X1, X2])
    direct, env = R.moments(Xc, None, None, base.reshape(-1)), R.moments_envelope(Xc, None, None, base.reshape(-1))
    assert both.count == 500 and direct["count"] == 500
    assert (np.abs(both.S.numpy() - direct["S"]) <= 2 * R.gamma(500) * env["S"]).all()
    assert (np.abs(both.r.numpy() - direct["r"]) <= 2 * R.gamma(500) * env["r"]).all()
    assert np.abs(both.covariance() - R.covariance(Xc)).max() < 1e-11 and np.abs(both.mean - Xc.mean(0)).max() < 1e-12
    # equal counts: the equal-weight mixture IS the concatenation, and joint_pca_w2 is the W2 in the concatenation's modes
    X2e = np.concatenate([X2, X2[:100]])
    m2e = _held(X2e, base)
    Xe = np.concatenate([X1, X2e])
    assert np.abs(covariance.pooled_covariance(m1, m2e).numpy() - R.covariance(Xe, 0)).max() < 1e-11
    lam, V = np.linalg.eigh(R.covariance(Xe, 0))
    assert lam[-1] - lam[-2] > 0.05 * lam[-1] and lam[-2] - lam[-3] > 0.05 * lam[-1]
    want = R.subspace_w2(V[:, ::-1][:, :2].T, X1, X2e)
    assert abs(covariance.joint_pca_w2(m1, m2e, 2) - want) < 1e-9
    # another reference: refused
    other = _held(X2, base + 1.0)
    for f in (covariance.pooled, covariance.rmwd, covariance.pca_w2, covariance.joint_pca_w2, covariance.rmsip, covariance.ensemble_w2,
              covariance.dccm_correlation, covariance.mode_cosines, covariance.residue_w2):
        with pytest.raises(ValueError, match="same reference"):
            f(m1, other)
    assert torch.equal(m1.ref, m2.ref)


def test_the_comparisons_on_restated_moments_agree_with_the_definitions_on_frames():
    from esmdiff_amd import covariance, flexibility
    rng = np.random.default_rng(3)
    base, X1 = _frames(rng, 300, 8, scale=2.0)
    _, X2 = _frames(rng, 200, 8, scale=2.6)
    X2 = X2 - X2.mean(0) + base + 0.4
    m1, m2 = _held(X1, base), _held(X2, base)
    assert np.abs(m1.covariance() - R.covariance(X1)).max() < 1e-11 and np.abs(m1.covariance(0) - R.covariance(X1, 0)).max() < 1e-11
    assert np.abs(m1.residue_covariance() - np.stack([np.cov(X1[:, l].T) for l in range(8)])).max() < 1e-11
    assert np.abs(m1.rmsf() - R.rmsf(X1)).max() < 1e-11 and np.abs(m1.dccm() - R.dccm(X1)).max() < 1e-11
    assert np.allclose(np.diag(m1.dccm()), 1.0) and np.array_equal(m1.dccm(), m1.dccm().T)
    lam, V = R.modes(X1, 3)
    assert lam[0] - lam[1] >= 0.05 * lam[0] and lam[1] - lam[2] >= 0.05 * lam[0] and lam[2] - R.modes(X1, 4)[0][3] >= 0.05 * lam[0]
    got_lam, got_V = m1.modes(3)
    assert np.abs(got_lam - lam).max() < 1e-10 and np.abs(got_V.reshape(3, -1) - V).max() < 1e-9
    assert np.abs(np.array(list(covariance.rmwd(m1, m2).values())) - np.array(R.rmwd(X1, X2))).max() < 1e-9
    assert abs(covariance.pca_w2(m1, m2, 2) - R.pca_w2(X1, X2, 2)) < 1e-9
    want = np.sqrt(((X1.mean(0) - X2.mean(0)) ** 2).sum() + R.bures(R.covariance(X1), R.covariance(X2)))
    assert abs(covariance.ensemble_w2(m1, m2) - want) < 1e-8
    i, j = np.triu_indices(8, 1)
    assert abs(covariance.dccm_correlation(m1, m2) - np.corrcoef(R.dccm(X1)[i, j], R.dccm(X2)[i, j])[0, 1]) < 1e-10
    assert abs(covariance.rmsip(m1, m2, 3) - R.rmsip(V, R.modes(X2, 3)[1])) < 1e-9
    assert covariance.mode_cosines(m1, m2, 3).shape == (3, 3)
    assert abs(flexibility.flexibility_correlation(m1.rmsf(), m2.rmsf())["pearson"] - np.corrcoef(R.rmsf(X1), R.rmsf(X2))[0, 1]) < 1e-10
    for bad in (0, 25):
        with pytest.raises(ValueError):
            m1.modes(bad)
    assert "[ALPHAFLOW-RECALL]" in covariance.__doc__ and "UNPINNED" in covariance.__doc__.upper()
    assert "scipy" not in (ROOT / "esmdiff_amd" / "covariance.py").read_text().replace("scipy.", "")


def test_projection_w2():
    from esmdiff_amd import covariance
    rng = np.random.default_rng(4)
    a, b = rng.standard_normal((37, 2)) * 2.0 + 1.0, rng.standard_normal((50, 2))
    for p in (1, 2):
        got = covariance.projection_w2(a, b, p)
        assert got.shape == (2,) and all(abs(got[k] - R.projection_w2(a[:, k], b[:, k], p)) < 1e-12 for k in range(2))
    # three points by hand: sorted (0, 1, 3) against (1, 1, 5): differences 1, 0, 2
    got = covariance.projection_w2([3.0, 0.0, 1.0], [1.0, 5.0, 1.0])
    assert got.shape == (1,) and abs(got[0] - np.sqrt(5.0 / 3.0)) < 1e-15
    assert abs(covariance.projection_w2([3.0, 0.0, 1.0], [1.0, 5.0, 1.0], 1)[0] - 1.0) < 1e-15
    # unequal sizes by hand: (0, 2) against (0, 1, 2, 3): quantile steps at 1/4: |0-0|, |0-1|, |2-2|, |2-3|
    assert abs(covariance.projection_w2([0.0, 2.0], [3.0, 2.0, 1.0, 0.0])[0] - np.sqrt(0.5)) < 1e-15
    assert covariance.projection_w2(a, a)[0] == 0.0
    for bad in (([], [1.0]), ([np.nan], [1.0]), (np.zeros((3, 2)), np.zeros((3, 3)))):
        with pytest.raises(ValueError):
            covariance.projection_w2(*bad)
    stats = pytest.importorskip("scipy.stats")
    for k in range(2):
        assert abs(covariance.projection_w2(a, b, 1)[k] - stats.wasserstein_distance(a[:, k], b[:, k])) < 1e-12


def test_rmsip():
    rng = np.random.default_rng(5)
    D, k = 90, 3
    U = np.linalg.qr(rng.standard_normal((D, k)))[0].T
    mix = np.linalg.qr(rng.standard_normal((k, k)))[0]
    assert abs(R.rmsip(U, U) - 1.0) < 1e-14 and abs(R.rmsip(U, mix @ U) - 1.0) < 1e-14         # the same subspace in another basis
    V = np.linalg.qr(rng.standard_normal((D, k)))[0].T
    assert R.rmsip(U, V) < 0.5                                                                  # sqrt(k / D) = 0.18 in expectation
    # through the moments: an ensemble against itself, and against one with unrelated modes
    from esmdiff_amd import covariance
    base, X1 = _frames(rng, 400, 30, scale=2.0)
    assert 3 * 30 == D
    m1 = _held(X1, base)
    assert abs(covariance.rmsip(m1, m1, k) - 1.0) < 1e-12
    spectrum = np.r_[9.0, 6.0, 4.0, np.full(D - 3, 0.05)]
    planted = lambda Q: base[None] + ((rng.standard_normal((400, D)) * np.sqrt(spectrum)) @ Q.T).reshape(400, 30, 3)
    Qa, Qb = (np.linalg.qr(rng.standard_normal((D, D)))[0] for _ in range(2))
    ma, mb = _held(planted(Qa), base), _held(planted(Qb), base)
    assert covariance.rmsip(ma, mb, k) < 0.5 and covariance.rmsip(ma, _held(planted(Qa), base), k) > 0.95


def test_command_line_without_the_flag_is_unchanged(tmp_path, monkeypatch):
    from esmdiff_amd import analyze_ensemble, covariance
    stub = {"TM-ens": 0.5, "best_tm": np.array([0.25, 0.75]), "flex": {"rmsf": np.array([1.0, np.nan])}}
    monkeypatch.setattr(analyze_ensemble, "analyze", lambda *a, **k: dict(stub))
    samples, target = np.zeros((4, 5, 3)), np.ones((5, 3))
    monkeypatch.setattr(analyze_ensemble, "load_ca", lambda *a, **k: (samples, [target], 4, np.arange(4)))
    calls = []
    monkeypatch.setattr(covariance, "compare", lambda *a, **k: calls.append((a, k)) or {"rmwd": 1.25, "residue_w2": {"w2": np.array([0.5, np.nan])}})
    args = ["--samples", "ens.pdb", "--targets", "a.pdb", "--output"]
    plain = analyze_ensemble.main(args + [str(tmp_path / "plain")])
    assert not calls
    assert plain.read_text() == '{\n "TM-ens": 0.5,\n "best_tm": [\n  0.25,\n  0.75\n ],\n "flex": {\n  "rmsf": [\n   1.0,\n   null\n  ]\n }\n}\n'
    np.save(tmp_path / "ref.npy", np.zeros((50, 5, 3)))
    full = analyze_ensemble.main(args + [str(tmp_path / "cmp"), "--compare", "--trajectory", str(tmp_path / "ref.npy"), "--compare_modes", "3",
                                         "--tica_chunk", "16"])
    data = json.loads(full.read_text())
    assert data.pop("compare") == {"rmwd": 1.25, "residue_w2": {"w2": [0.5, None]}} and json.dumps(data, indent=1) + "\n" == plain.read_text()
    (a, k), = calls
    assert isinstance(a[0], np.memmap) and a[0].shape == (50, 5, 3) and a[1] is samples and a[2] is target and a[3:] == (3, 16)
    assert k["targets"].shape == (1, 5, 3)
    analyze_ensemble.main(args + [str(tmp_path / "first"), "--compare", "--trajectory", str(tmp_path / "ref.npy"), "--compare_ref", "first"])
    assert calls[1][0][2] is None and calls[1][0][3:] == (2, 65536)
    with pytest.raises(SystemExit):
        analyze_ensemble.main(args + [str(tmp_path / "bad"), "--compare"])
    with pytest.raises(SystemExit):
        analyze_ensemble.main(args + [str(tmp_path / "bad"), "--compare", "--trajectory", str(tmp_path / "ref.npy"), "--compare_ref", "mean"])
    np.save(tmp_path / "other.npy", np.zeros((50, 6, 3)))
    with pytest.raises(ValueError, match="residue to residue"):
        analyze_ensemble.main(args + [str(tmp_path / "bad"), "--compare", "--trajectory", str(tmp_path / "other.npy")])
    p = analyze_ensemble.parser().parse_args(args + ["o"])
    assert (p.compare, p.compare_ref, p.compare_modes) == (False, "target", 2)
    assert "--compare" in analyze_ensemble.__doc__ and "[ALPHAFLOW-RECALL]" in analyze_ensemble.__doc__


def test_argument_validation():
    from esmdiff_amd import covariance
    with pytest.raises(ValueError, match="empty list"):
        covariance.aligned_moments([])
    for bad in (np.zeros((4, 5)), np.zeros((4, 5, 2)), np.zeros((0, 5, 3))):
        with pytest.raises(ValueError):
            covariance.aligned_moments(bad, ref=np.zeros((5, 3)))
    with pytest.raises(ValueError, match="beyond the kernel's limit"):
        covariance.aligned_moments(np.zeros((2, 1281, 3)))
    with pytest.raises(ValueError, match="resolved residues"):
        covariance.aligned_moments(np.zeros((2, 3, 3)), ref=np.array([[0.0, 0, 0], [np.nan, 0, 0], [np.nan, 0, 0]]))
    with pytest.raises(ValueError, match=r"\(L, 3\)"):
        covariance.aligned_moments(np.zeros((2, 3, 3)), ref=np.zeros(3))

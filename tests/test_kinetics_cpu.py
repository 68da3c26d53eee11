"""The host side of the kinetics layer: the declarations and macros of the three entries of csrc/lagged.hip against esmdiff_amd/_native.py,
the numpy restatement tests/kinetics_ref.py against plain numpy, the timescale and free-energy arithmetic, the chunk and overlap
bookkeeping of the memmap path against a brute-force index list, the pair count of a list of trajectories, the dense tail of the fit on
restated moments against oracle/metrics_ref.tica_fit, argument validation, and the command line without --tica.  No device."""
import json
import math
import re
from pathlib import Path

import numpy as np
import pytest

from tests import kinetics_ref as R

ROOT = Path(__file__).resolve().parent.parent


def test_entries_are_declared_and_exported():
    from esmdiff_amd import _native as N
    from esmdiff_amd import build
    header = (ROOT / "include" / "esmdiff_hip.h").read_text()
    flat = re.sub(r"\s+", " ", header)
    assert ("int esmdiff_lagged_means(const double* X, int32_t n, int32_t L_or_D, int32_t pwd_offset, int32_t lag, double* mean0, "
            "double* meant, void* scratch, int64_t scratch_bytes, void* stream);") in flat
    assert ("int esmdiff_lagged_moments(const double* X, int32_t n, int32_t L_or_D, int32_t pwd_offset, int32_t lag, const double* center, "
            "double* S00, double* S0t, double* Stt, double* r0, double* rt, void* scratch, int64_t scratch_bytes, void* stream);") in flat
    assert ("int esmdiff_lagged_project(const double* X, int32_t n, int32_t L_or_D, int32_t pwd_offset, const double* mean, const double* W, "
            "int32_t dim, double* Y, void* scratch, int64_t scratch_bytes, void* stream);") in flat
    assert re.search(r"#define ESMDIFF_ABI_VERSION 8\b", header)
    pairs_text = (ROOT / "esmdiff_amd" / "pairs.py").read_text()
    for name in ("esmdiff_lagged_means", "esmdiff_lagged_moments", "esmdiff_lagged_project"):
        assert name in N.EXPORTS and f"N.lib().{name}(" in pairs_text
    for macro, value, ref in (("MAX_L", N.LAGGED_MAX_L, R.MAX_L), ("MAX_D", N.LAGGED_MAX_D, R.MAX_D), ("MAX_DIM", N.LAGGED_MAX_DIM, R.MAX_DIM),
                              ("FRAME_CHUNK", N.LAGGED_FRAME_CHUNK, R.FRAME_CHUNK)):
        assert re.search(r"#define ESMDIFF_LAGGED_%s %d\b" % (macro, value), header) and value == ref, macro
    assert N.LAGGED_MAX_L >= 128 and N.lagged_features(N.LAGGED_MAX_L, 1) <= N.LAGGED_MAX_D and N.LAGGED_MAX_DIM == 16
    assert "#define ESMDIFF_LAGGED_FEATURES(L, k) ((((int64_t)(L) - (k)) * ((int64_t)(L) - (k) + 1)) / 2)" in header
    assert "#define ESMDIFF_LAGGED_TABLE_BYTES(D) ((int64_t)(D) * 8)" in header
    assert "#define ESMDIFF_LAGGED_MEANS_SCRATCH_BYTES(D, slots) (ESMDIFF_LAGGED_TABLE_BYTES(D) + (int64_t)(slots) * 2 * (int64_t)(D) * 8)" in header
    assert ("#define ESMDIFF_LAGGED_MOMENTS_SCRATCH_BYTES(D, slots) \\\n  (ESMDIFF_LAGGED_TABLE_BYTES(D) + (int64_t)(slots) * "
            "(3 * (int64_t)(D) * (int64_t)(D) + 2 * (int64_t)(D)) * 8)") in header
    for L, k in ((2, 1), (12, 1), (12, 3), (58, 1), (128, 1)):
        assert N.lagged_features(L, k) == R.n_features(L, k) == len(np.triu_indices(L, k)[0])
    for D, slots in ((1, 1), (66, 3), (1653, 2)):
        assert N.lagged_scratch_bytes(D, slots, True) == R.scratch_bytes(D, slots, True) == D * 8 + slots * (3 * D * D + 2 * D) * 8
        assert N.lagged_scratch_bytes(D, slots, False) == R.scratch_bytes(D, slots, False) == D * 8 + slots * 2 * D * 8
    assert build.UNITS["lagged"] == ["-ffp-contract=off", "-fno-slp-vectorize"] and (ROOT / "esmdiff_amd" / "csrc" / "lagged.hip").is_file()
    source = (ROOT / "esmdiff_amd" / "csrc" / "lagged.hip").read_text()
    assert "__builtin_amdgcn_mfma_f64_16x16x4f64" in source and "(lane >> 4) + 4 * reg" in source


def test_the_restatement_against_plain_numpy():
    rng = np.random.default_rng(0)
    X = R.trajectory(2 * R.FRAME_CHUNK + 40, 6, seed=1)
    lag, F = 9, R.features(X, 1)
    m = len(F) - lag
    m0, mt = R.means(X, lag, 1)
    assert np.abs(m0 - F[:m].mean(0)).max() < 1e-12 and np.abs(mt - F[lag:].mean(0)).max() < 1e-12
    c = (m0 + mt) / 2.0
    mom = R.moments(X, lag, c, 1)
    assert np.abs(mom["r0"] - (F[:m] - c).sum(0)).max() < 1e-9 and np.allclose(mom["S0t"], (F[:m] - c).T @ (F[lag:] - c))
    W = rng.standard_normal((F.shape[1], 3))
    assert np.abs(R.project(X, c, W, 1) - (F - c) @ W).max() <= (2 * R.gamma(F.shape[1]) * R.project_envelope(X, c, W, 1)).max()
    Fi = rng.integers(-512, 513, size=(700, 70))
    ci = rng.integers(-8, 9, size=70)
    exact = R.moments_int(Fi, 7, ci)
    assert max(int(np.abs(v).max()) for v in exact.values()) < 2 ** 53            # every sum of the exact-operand tests is a float64 integer
    real = R.moments(Fi.astype(np.float64), 7, ci.astype(np.float64), 0)
    assert all(np.array_equal(real[k], exact[k].astype(np.float64)) for k in exact)
    assert np.abs(np.linalg.norm(np.diff(R.trajectory(5, 12, seed=2), axis=1), axis=2) - 3.8).max() < 1.0   # a chain of 3.8 A steps, plus noise


def test_timescales_and_free_energy():
    from esmdiff_amd import kinetics
    ts = kinetics.timescales_from_eigenvalues([0.5, math.exp(-0.1), 1.0, 1.5, 0.0, -0.5], 20)
    assert abs(ts[0] - 20.0 / math.log(2.0)) < 1e-12 and abs(ts[1] - 200.0) < 1e-9 and np.isnan(ts[2:]).all()
    edges, F = kinetics.free_energy([0.1, 0.2, 0.3, 0.9], bins=2, kT=2.0)
    assert np.allclose(edges[0], [0.1, 0.5, 0.9]) and np.allclose(F, [-2.0 * math.log(0.75), -2.0 * math.log(0.25)])
    edges, F = kinetics.free_energy(np.array([[0.0, 0.0], [0.0, 0.0], [1.0, 1.0], [1.0, 0.0]]), bins=2)
    assert len(edges) == 2 and F.shape == (2, 2) and F[0, 1] == np.inf and abs(F[0, 0] - math.log(2.0)) < 1e-15 and abs(F[1, 1] - math.log(4.0)) < 1e-15
    edges, F = kinetics.free_energy([0.1, 0.2, 5.0], bins=4, range=[(0.0, 1.0)])
    assert np.allclose(edges[0], [0.0, 0.25, 0.5, 0.75, 1.0]) and F[0] == 0.0 and np.isinf(F[1:]).all()
    for bad in ([], [np.nan, 1.0], np.zeros((2, 2, 2))):
        with pytest.raises(ValueError):
            kinetics.free_energy(bad)


def test_chunk_spans_cover_every_pair_once():
    from esmdiff_amd import kinetics
    for n, lag, chunk in ((10, 3, 4), (10, 3, 7), (10, 3, 100), (100, 1, 1), (57, 20, 8), (21, 20, 5), (1000, 500, 128)):
        spans = kinetics.chunk_spans(n, lag, chunk)
        got = [(s + t, s + t + lag) for s, e in spans for t in range(e - s - lag)]       # the pairs each uploaded piece sees, in order
        assert got == [(t, t + lag) for t in range(n - lag)], (n, lag, chunk)
        assert all(0 <= s < e <= n and e - s - lag <= chunk for s, e in spans)
        assert all(b[0] == a[1] - lag for a, b in zip(spans, spans[1:]))                  # consecutive pieces overlap by the lag
        assert len(spans) == -(-(n - lag) // chunk)
    assert kinetics.chunk_spans(5, 5, 4) == [] and kinetics.chunk_spans(3, 5, 4) == []
    with pytest.raises(ValueError):
        kinetics.chunk_spans(10, 3, 0)


def test_pair_count_of_a_list():
    from esmdiff_amd import kinetics
    assert kinetics.pair_count([100, 160], 6) == 248 and kinetics.pair_count([260], 6) == 254
    assert kinetics.pair_count([5, 6, 7], 6) == 1 and kinetics.pair_count([], 3) == 0


@pytest.mark.parametrize("shape", [(600, 12, 5), (300, 9, 3)], ids=lambda p: "x".join(map(str, p)))
def test_the_dense_tail_on_restated_moments_agrees_with_the_oracle(shape):
    """covariances() and fit() are device-agnostic torch: on the restatement's moments (about a centre that is NOT the mean) they give the
    oracle's eigenvalues, so the residual-sum correction and the tail are held without a device."""
    import torch
    from esmdiff_amd import kinetics
    from oracle import metrics_ref as O
    n, L, lag = shape
    X = R.trajectory(n, L, seed=0)
    F = R.features(X, 1)
    mean, comp, lam = O.tica_fit(F, lag, dim=4)
    assert abs(lam[0]) - abs(lam[1]) >= 0.05 and abs(lam[1]) - abs(lam[2]) >= 0.05
    c = mean + 0.01 * np.random.default_rng(1).standard_normal(len(mean))
    mom = R.moments(X, lag, c, 1)
    m0, mt = R.means(X, lag, 1)
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a))
    held = kinetics.LaggedMoments(n - lag, lag, T(m0), T(mt), T(c), **{k: T(v) for k, v in mom.items()})
    c00, c0t = (t.numpy() for t in held.covariances(True))
    a, b = F[:-lag] - mean, F[lag:] - mean
    assert np.abs(c00 - (a.T @ a + b.T @ b) / (2.0 * len(a))).max() < 1e-12 and np.abs(c0t - (a.T @ b + b.T @ a) / (2.0 * len(a))).max() < 1e-12
    assert np.array_equal(c00, c00.T) and np.array_equal(c0t, c0t.T)
    k00, k0t, ktt = (t.numpy() for t in held.covariances(False))
    a0, bt = F[:-lag] - F[:-lag].mean(0), F[lag:] - F[lag:].mean(0)
    assert np.abs(k00 - a0.T @ a0 / len(a0)).max() < 1e-12 and np.abs(k0t - a0.T @ bt / len(a0)).max() < 1e-12 and np.abs(ktt - bt.T @ bt / len(a0)).max() < 1e-12
    model = kinetics.fit(held, dim=2)
    assert np.abs(model.eigenvalues - lam[:2]).max() <= 1e-6 and model.n_kept == F.shape[1]
    assert np.abs(model.mean.numpy() - mean).max() < 1e-12
    got = (F - model.mean.numpy()) @ model.components.numpy()
    want = ((F - mean) @ comp[:, :2]) * lam[:2]
    assert (np.abs(got * np.sign((got * want).sum(0)) - want) / (want.max(0) - want.min(0))).max() <= 1e-6
    comp_np = model.components.numpy()
    assert (comp_np[np.abs(comp_np).argmax(0), np.arange(2)] > 0).all()
    assert np.array_equal(model.timescales, kinetics.timescales_from_eigenvalues(model.eigenvalues, lag))
    plain = kinetics.fit(held, dim=2, scaling=None)
    assert np.allclose(plain.components.numpy() * model.eigenvalues, comp_np, atol=1e-12)
    sv = R.koopman_singular_values(F, lag)
    vamp = kinetics.fit(held, dim=3, reversible=False)
    assert np.abs(vamp.eigenvalues - sv[:3]).max() <= 1e-6 and abs(vamp.vamp2() - (1.0 + (sv ** 2).sum())) <= 1e-6 * len(sv)


def test_argument_validation():
    import torch
    from esmdiff_amd import kinetics
    X = R.trajectory(30, 5, seed=0)
    for lag in (0, -1, 2.5):
        with pytest.raises(ValueError, match="lagtime"):
            kinetics.lagged_moments(X, lag)
    with pytest.raises(ValueError, match="more than lagtime"):
        kinetics.lagged_moments(X, 30)
    with pytest.raises(ValueError, match="more than lagtime"):
        kinetics.lagged_moments([X[:4], X[:5]], 5)
    with pytest.raises(ValueError, match="empty list"):
        kinetics.lagged_moments([], 5)
    for bad, kw in ((np.zeros((30, 5)), {}), (np.zeros((30, 5, 2)), {}), (X, {"pwd_offset": 5}), (X, {"pwd_offset": 0}),
                    (np.zeros((30, 129, 3)), {}), (X, {"features": True}), (np.zeros((30, 8193)), {"features": True})):
        with pytest.raises(ValueError):
            kinetics.lagged_moments(bad, 3, **kw)
    T = lambda *s: torch.zeros(*s, dtype=torch.float64)
    held = kinetics.LaggedMoments(10, 2, T(4), T(4), T(4), T(4, 4), T(4, 4), T(4, 4), T(4), T(4))
    for kw in ({"dim": 0}, {"dim": 17}, {"scaling": "commute_map"}):
        with pytest.raises(ValueError):
            kinetics.fit(held, **kw)
    with pytest.raises(ValueError, match="rank cut-off"):
        kinetics.fit(held, dim=2)                           # all-zero moments: nothing above epsilon
    assert "[DEEPTIME-RECALL]" in kinetics.TICAModel.__doc__ and "UNPINNED" in kinetics.TICAModel.__doc__.upper()


def test_command_line_without_the_flag_is_unchanged(tmp_path, monkeypatch):
    from esmdiff_amd import analyze_ensemble, kinetics
    stub = {"TM-ens": 0.5, "best_tm": np.array([0.25, 0.75]), "flex": {"rmsf": np.array([1.0, np.nan])}}
    monkeypatch.setattr(analyze_ensemble, "analyze", lambda *a, **k: dict(stub))
    samples = np.zeros((4, 5, 3))
    monkeypatch.setattr(analyze_ensemble, "load_ca", lambda *a, **k: (samples, [np.zeros((5, 3))], 4, np.arange(4)))
    calls = []
    monkeypatch.setattr(kinetics, "report", lambda *a, **k: calls.append((a, k)) or {"lagtime": a[3], "free_energy": {"F": np.array([0.5, np.nan])}})
    args = ["--samples", "ens.pdb", "--targets", "a.pdb", "--output"]
    plain = analyze_ensemble.main(args + [str(tmp_path / "plain")])
    assert not calls
    assert plain.read_text() == '{\n "TM-ens": 0.5,\n "best_tm": [\n  0.25,\n  0.75\n ],\n "flex": {\n  "rmsf": [\n   1.0,\n   null\n  ]\n }\n}\n'
    np.save(tmp_path / "ref.npy", np.zeros((50, 5, 3)))
    full = analyze_ensemble.main(args + [str(tmp_path / "tica"), "--tica", "--trajectory", str(tmp_path / "ref.npy"), "--lagtime", "7",
                                         "--tica_dim", "3", "--lagtimes", "5", "10", "--tica_chunk", "16"])
    data = json.loads(full.read_text())
    assert data.pop("tica") == {"lagtime": 7, "free_energy": {"F": [0.5, None]}} and json.dumps(data, indent=1) + "\n" == plain.read_text()
    (a, k), = calls
    assert isinstance(a[0], np.memmap) and a[0].shape == (50, 5, 3) and a[1] is samples and a[2].shape == (1, 5, 3)
    assert a[3:] == (7, 3, [5, 10]) and k == {"chunk_frames": 16}
    with pytest.raises(SystemExit):
        analyze_ensemble.main(args + [str(tmp_path / "bad"), "--tica"])
    np.save(tmp_path / "other.npy", np.zeros((50, 6, 3)))
    with pytest.raises(ValueError, match="residue to residue"):
        analyze_ensemble.main(args + [str(tmp_path / "bad"), "--tica", "--trajectory", str(tmp_path / "other.npy")])
    p = analyze_ensemble.parser().parse_args(args + ["o"])
    assert (p.tica, p.trajectory, p.lagtime, p.tica_dim, p.lagtimes, p.tica_chunk) == (False, None, 20, 2, None, 65536)
    assert "--tica" in analyze_ensemble.__doc__ and "unpinned" in analyze_ensemble.__doc__

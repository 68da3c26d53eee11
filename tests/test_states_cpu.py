"""The host side of the states layer: the declarations and macros of the three entries of csrc/msm.hip against esmdiff_amd/_native.py,
the numpy restatement tests/states_ref.py against scikit-learn's Lloyd iteration (where scikit-learn is installed) and against itself
for integer operands, the Markov-model tail of esmdiff_amd/states.py (connected set, reversible estimator, spectrum, metastable sets,
population comparison), and the command line without --msm.  No device."""
import json
import re
from pathlib import Path

import numpy as np
import pytest

from tests import states_ref as R

ROOT = Path(__file__).resolve().parent.parent

def test_entries_are_declared_and_exported():
    from esmdiff_amd import _native as N
    from esmdiff_amd import build
    header = (ROOT / "include" / "esmdiff_hip.h").read_text()
    flat = re.sub(r"\s+", " ", header)
    assert ("int esmdiff_kmeans_assign(const double* Y, int32_t n, int32_t d, const double* centres, int32_t k, int32_t* labels, double* dist2, "
            "void* stream);") in flat
    assert ("int esmdiff_kmeans_step(const double* Y, int32_t n, int32_t d, const double* centres, int32_t k, int32_t* labels, int64_t* counts, "
            "double* sums, double* inertia, void* scratch, int64_t scratch_bytes, void* stream);") in flat
    assert ("int esmdiff_transition_counts(const int32_t* labels, int32_t n, int32_t k, int32_t lag, int64_t* counts, void* scratch, "
            "int64_t scratch_bytes, void* stream);") in flat
    assert re.search(r"#define ESMDIFF_ABI_VERSION 8\b", header)
    pairs_text = (ROOT / "esmdiff_amd" / "pairs.py").read_text()
    native_text = (ROOT / "esmdiff_amd" / "_native.py").read_text()
    for name in ("esmdiff_kmeans_assign", "esmdiff_kmeans_step", "esmdiff_transition_counts"):
        assert name in N.EXPORTS and f"N.lib().{name}(" in pairs_text and f"L.{name}.argtypes = [" in native_text
    for macro, value, ref in (("KMEANS_MAX_K", N.KMEANS_MAX_K, R.MAX_K), ("KMEANS_CENTRE_TILE", N.KMEANS_CENTRE_TILE, R.CENTRE_TILE),
                              ("KMEANS_FRAME_CHUNK", N.KMEANS_FRAME_CHUNK, R.FRAME_CHUNK), ("LAGGED_MAX_DIM", N.LAGGED_MAX_DIM, R.MAX_DIM),
                              ("TRANSITION_FRAME_CHUNK", N.TRANSITION_FRAME_CHUNK, R.TRANSITION_FRAME_CHUNK),
                              ("TRANSITION_LDS_MAX_K", N.TRANSITION_LDS_MAX_K, R.TRANSITION_LDS_MAX_K),
                              ("TRANSITION_SCRATCH_BYTES", N.TRANSITION_SCRATCH_BYTES, R.TRANSITION_SCRATCH_BYTES)):
        assert re.search(r"#define ESMDIFF_%s %d\b" % (macro, value), header) and value == ref, macro
    assert N.KMEANS_MAX_K == 4096 and N.LAGGED_MAX_DIM == 16 and N.TRANSITION_LDS_MAX_K ** 2 * 4 <= 65536
    assert N.KMEANS_FRAME_CHUNK % 256 == 0 and N.KMEANS_CENTRE_TILE * 16 * 8 <= 65536
    assert "#define ESMDIFF_KMEANS_CHUNKS(n) (((int64_t)(n) + ESMDIFF_KMEANS_FRAME_CHUNK - 1) / ESMDIFF_KMEANS_FRAME_CHUNK)" in header
    assert "#define ESMDIFF_KMEANS_SLOT_BYTES(k, d) (((int64_t)(k) * (int64_t)(d) + (int64_t)(k) + 1) * 8)" in header
    assert "#define ESMDIFF_KMEANS_STEP_SCRATCH_BYTES(k, d, slots) ((int64_t)(slots) * ESMDIFF_KMEANS_SLOT_BYTES(k, d))" in header
    for n in (0, 1, 1023, 1024, 1025, 2051):
        assert N.kmeans_chunks(n) == R.chunks(n) == -(-n // 1024)
    for k, d, slots in ((1, 1, 1), (65, 3, 2), (4096, 16, 5)):
        assert N.kmeans_slot_bytes(k, d) == R.slot_bytes(k, d) == (k * d + k + 1) * 8
        assert N.kmeans_step_scratch_bytes(k, d, slots) == R.step_scratch_bytes(k, d, slots) == slots * (k * d + k + 1) * 8
    assert build.UNITS["msm"] == ["-ffp-contract=off", "-fno-slp-vectorize"] and (ROOT / "esmdiff_amd" / "csrc" / "msm.hip").is_file()
    source = (ROOT / "esmdiff_amd" / "csrc" / "msm.hip").read_text()
    assert "if (s < best) best = s, idx = j0 + j;" in source and "atomicAdd" in source
    assert not re.search(r"atomicAdd\([^;]*\b(double|float)\b", source)               # no float atomics: the order is published


def test_the_restatement_for_integer_operands_and_its_rules():
    rng = np.random.default_rng(0)
    Y, C = rng.integers(-512, 513, size=(2 * R.FRAME_CHUNK + 3, 3)), rng.integers(-512, 513, size=(70, 3))
    C[40] = C[7]                                                                      # a duplicate centre: the lower index wins
    labels, counts, sums, inertia = R.step(Y.astype(np.float64), C.astype(np.float64))
    li, ci, si, ii = R.step_int(Y, C)
    assert np.array_equal(labels, li) and np.array_equal(counts, ci) and np.array_equal(sums, si.astype(np.float64)) and inertia == float(ii)
    assert counts[40] == 0 and not (labels == 40).any() and np.array_equal(sums[40], np.zeros(3)) and not np.signbit(sums[40]).any()
    assert abs(ii) < 2 ** 53 and np.abs(si).max() < 2 ** 53                           # every sum of the exact-operand tests is a float64 integer
    lab, d2 = R.assign(np.array([[0.0, 0.0], [np.nan, 0.0], [np.inf, 1.0], [1.0, 1.0]]), np.array([[np.nan, 0.0], [1.0, 1.0], [np.inf, 0.0]]))
    assert lab.tolist() == [1, -1, -1, 1] and d2[0] == 2.0 and np.isnan(d2[1]) and np.isnan(d2[2]) and d2[3] == 0.0
    lab, d2 = R.assign(np.zeros((3, 2)), np.full((2, 2), np.nan))
    assert lab.tolist() == [-1, -1, -1] and np.isnan(d2).all()
    seq = np.array([0, 1, -1, 1, 0, 0, 2, 1])
    assert R.transition_counts(seq, 3, 1).tolist() == [[1, 1, 1], [1, 0, 0], [0, 1, 0]]
    assert R.transition_counts(seq, 3, 7).tolist() == [[0, 1, 0], [0, 0, 0], [0, 0, 0]] and R.transition_counts(seq, 3, 8).sum() == 0


def well_posed(Y, trace, margin=1e-6):
    """At every step every frame's nearest and second-nearest squared distance differ by more than `margin` of the larger, and no
    cluster is empty: the labels then do not depend on the rounding of the distances, nor the centres on an empty-cluster rule."""
    for centres, labels in trace:
        d2 = np.sort(((Y[:, None, :] - centres[None, :, :]) ** 2).sum(-1), axis=1)
        if not ((d2[:, 1] - d2[:, 0]) > margin * d2[:, 1]).all() or len(np.unique(labels)) != len(centres):
            return False
    return True


def test_the_restatement_against_sklearn():
    """Labels equal; centres within 2 gamma_m max|y| with m the largest cluster.  The bound: a centre is a sum of at most m frames
    divided once.  A sum of m terms in ANY order lies within gamma_(m - 1) sum|y| <= gamma_(m - 1) m max|y| of the exact one (Higham,
    Accuracy and Stability, eq. 4.4), the division by m brings that to gamma_(m - 1) max|y| and adds one rounding: below
    gamma_m max|y|.  Two such computations differ by at most twice that.  (scikit-learn also centres the data about its mean and adds
    the mean back, a few roundings of max|y| more, far inside the slack between gamma_m and the three or so roundings that count.)"""
    cluster = pytest.importorskip("sklearn.cluster")
    Y, init = R.blob_problem()
    trace = []
    centres, labels, counts, inertia, updates, converged = R.lloyd(Y, init, trace=trace)
    assert well_posed(Y, trace) and converged and updates >= 2
    km = cluster.KMeans(n_clusters=len(init), init=init, n_init=1, algorithm="lloyd", tol=0.0, max_iter=100).fit(Y)
    assert np.array_equal(km.labels_, labels)
    bound = 2.0 * R.gamma(int(counts.max())) * np.abs(Y).max()
    print(f"MEASURED restated Lloyd against scikit-learn: max centre difference {np.abs(km.cluster_centers_ - centres).max():.3e}, bound {bound:.3e}")
    assert np.abs(km.cluster_centers_ - centres).max() <= bound
    assert abs(km.inertia_ - inertia) <= 1e-9 * inertia


def test_the_blobs_of_the_model_test_are_well_posed():
    """Without scikit-learn too: tests/test_gpu_states.py holds the device's Lloyd loop to the restatement's on this input."""
    Y, init = R.blob_problem()
    trace = []
    centres, labels, counts, inertia, updates, converged = R.lloyd(Y, init, trace=trace)
    assert well_posed(Y, trace) and converged and 2 <= updates < 100 and counts.sum() == len(Y)
    means = np.stack([Y[labels == j].mean(0) for j in range(len(init))])
    assert np.abs(means - centres).max() <= 2.0 * R.gamma(int(counts.max())) * np.abs(Y).max()


def test_reversible_estimator():
    from esmdiff_amd import states
    rng = np.random.default_rng(1)
    A = rng.integers(1, 40, size=(6, 6))
    S = A + A.T
    T, pi, sweeps, converged = states.reversible_mle(S)
    assert converged and np.abs(T - S / S.sum(1)[:, None]).max() <= 1e-12 and np.abs(pi - S.sum(1) / S.sum()).max() <= 1e-12
    C = rng.integers(0, 30, size=(7, 7)) + np.diag(rng.integers(50, 90, size=7))
    C[0, 1], C[1, 0] = 25, 3                                                          # plainly asymmetric
    T, pi, sweeps, converged = states.reversible_mle(C)
    balance = np.abs(pi[:, None] * T - (pi[:, None] * T).T).max()
    print(f"MEASURED reversible MLE: {sweeps} sweeps, detailed balance {balance:.3e}, rows {np.abs(T.sum(1) - 1).max():.3e}, "
          f"pi T - pi {np.abs(pi @ T - pi).max():.3e}")
    assert converged and np.abs(T.sum(1) - 1.0).max() <= 1e-14 and abs(pi.sum() - 1.0) <= 1e-14 and (T >= 0).all()
    assert np.abs(pi @ T - pi).max() <= 1e-10 and balance <= 1e-10                    # three decades above tol = 1e-12
    x = pi[:, None] * T                                                               # the fixed point reproduces itself
    ci = C.sum(1).astype(np.float64)
    again = (C + C.T) / (ci[:, None] / x.sum(1)[:, None] + ci[None, :] / x.sum(1)[None, :])
    again = again / again.sum()
    assert np.abs(again / again.sum(1)[:, None] - T).max() <= 1e-10
    Tr, pir, _ = R.reversible_mle(C)
    assert np.abs(Tr - T).max() <= 1e-10 and np.abs(pir - pi).max() <= 1e-10
    assert not np.allclose(T, C / C.sum(1)[:, None], atol=1e-3)                       # and it is not the plain estimator
    with pytest.raises(ValueError):
        states.reversible_mle(np.array([[1, 0], [0, 0]]))


def test_connected_set():
    from esmdiff_amd import states
    C = np.zeros((6, 6), np.int64)
    C[0, 1] = C[1, 2] = C[2, 0] = 5                                                   # a cycle 0 -> 1 -> 2 -> 0
    C[0, 0] = C[1, 1] = C[2, 2] = 50
    C[2, 3], C[3, 3] = 1, 9                                                           # 3 is absorbing: entered, never left
    C[4, 0], C[4, 4] = 2, 7                                                           # 4 is unreachable: left, never entered
    sets = states.strongly_connected_sets(C)                                         # 5 never occurs
    assert [s.tolist() for s in sets] == [[0, 1, 2], [3], [4], [5]]
    model = states.msm(C, 3)
    assert model.active_set.tolist() == [0, 1, 2] and model.transition_matrix.shape == (3, 3) and model.counts.shape == (6, 6)
    assert np.abs(model.stationary_distribution - 1.0 / 3.0).max() <= 1e-10
    ring = np.roll(np.eye(300, dtype=np.int64), 1, axis=1)                            # one long cycle: no recursion limit
    assert len(states.strongly_connected_sets(ring)) == 1
    two = np.kron(np.eye(2, dtype=np.int64), np.ones((2, 2), np.int64))
    assert [s.tolist() for s in states.strongly_connected_sets(two)] == [[0, 1], [2, 3]]     # equal sizes: the smallest state first
    with pytest.raises(ValueError):
        states.msm(np.zeros((3, 3), np.int64), 1)


def test_non_reversible_chain_with_a_known_spectrum():
    """The circulant chain T = a I + b P + c P^2 on three states has the eigenvalues 1 and a - (b + c) / 2 +- i sqrt(3) / 2 (b - c)."""
    from esmdiff_amd import kinetics, states
    a, b, c = 0.7, 0.2, 0.1
    P = np.roll(np.eye(3), 1, axis=1)
    T = a * np.eye(3) + b * P + c * P @ P
    model = states.msm(np.rint(1000 * T).astype(np.int64), 5, reversible=False)
    assert np.abs(model.transition_matrix - T).max() <= 1e-15 and np.abs(model.stationary_distribution - 1.0 / 3.0).max() <= 1e-12
    want = np.array([1.0, a - (b + c) / 2 + 1j * np.sqrt(3) / 2 * (b - c), a - (b + c) / 2 - 1j * np.sqrt(3) / 2 * (b - c)])
    lam = model.eigenvalues
    assert abs(lam[0] - 1.0) <= 1e-12 and np.abs(np.sort_complex(lam[1:]) - np.sort_complex(want[1:])).max() <= 1e-12
    modulus = abs(want[1])
    assert np.abs(model.timescales - (-5.0 / np.log(modulus))).max() <= 1e-9
    with pytest.raises(ValueError, match="real"):
        model.metastable(2)
    real = states.msm(np.array([[90, 10, 0], [5, 90, 5], [0, 10, 90]]), 2, reversible=False)      # a birth-death chain: real spectrum
    lam = np.sort(np.linalg.eigvals(real.transition_matrix).real)[::-1]
    assert not np.iscomplexobj(real.eigenvalues) and np.abs(real.eigenvalues - lam).max() <= 1e-12
    assert np.array_equal(real.timescales, kinetics.timescales_from_eigenvalues(real.eigenvalues[1:], 2))
    assert "[DEEPTIME-RECALL]" in states.MSMModel.__doc__ and "UNPINNED" in states.MSMModel.__doc__.upper()
    assert "OUT OF SCOPE" in states.MSMModel.metastable.__doc__


@pytest.mark.parametrize("blocks", [2, 3])
def test_metastable_sets_of_a_block_matrix(blocks):
    from esmdiff_amd import states
    rng = np.random.default_rng(blocks)
    size = 4
    n = blocks * size
    C = np.zeros((n, n), np.int64)
    for b in range(blocks):
        C[b * size:(b + 1) * size, b * size:(b + 1) * size] = rng.integers(200, 400, size=(size, size))
    for b in range(blocks):                                                           # weak coupling between neighbouring blocks
        a, z = b * size + size - 1, ((b + 1) % blocks) * size
        C[a, z] += 2
        C[z, a] += 2
    model = states.msm(C, 1)
    assert len(model.active_set) == n and model.converged
    sets = model.metastable(blocks)
    owner = np.arange(n) // size
    assert all(len(set(sets.assignment[owner == b])) == 1 for b in range(blocks)) and len(set(sets.assignment)) == blocks
    assert np.abs(sets.memberships.sum(1) - 1.0).max() <= 1e-12 and (sets.memberships >= 0).all()
    assert abs(sets.weights.sum() - 1.0) <= 1e-12 and sorted(map(len, sets.sets)) == [size] * blocks
    assert np.abs(R.inner_simplex(model.right_eigenvectors[:, :blocks]) - sets.memberships).max() <= 1e-9
    assert model.timescales[blocks - 2] > 10 * model.timescales[blocks - 1]           # the gap after the slow processes


def test_compare_populations():
    from esmdiff_amd import states
    C = np.array([[80, 10, 10, 0], [10, 60, 10, 0], [10, 10, 40, 0], [0, 0, 3, 5]])   # state 3 is left, never entered
    model = states.msm(C, 1)
    pi = model.stationary_distribution
    assert model.active_set.tolist() == [0, 1, 2] and np.abs(pi - np.array([100, 80, 60]) / 240.0).max() <= 1e-10
    exact = np.repeat([0, 1, 2], [50, 40, 30])                                        # in exactly pi's proportions
    res = states.compare_populations(exact, model)
    # "zero" for a DISTANCE, the root of a divergence: p / m and q / m are 1 up to two roundings each (m, the quotient), so every
    # logarithm is within 2 u of 0 and the divergence (sum p log + sum q log) / 2 within 2 u, doubled for the rounding of pi itself
    zero = np.sqrt(4.0 * R.U)
    print(f"MEASURED compare_populations in pi's proportions: js {res['js']:.3e}, bar {zero:.3e}")
    assert res["js"] <= zero and res["outside"] == 0.0 and res["n_inside"] == 120
    mixed = np.concatenate([exact, [3] * 20, [-1] * 10, [7] * 10])
    res = states.compare_populations(mixed, model, assignment=np.array([0, 0, 1]))
    assert res["js"] <= zero and abs(res["outside"] - 40 / 160) <= 1e-15 and res["n_samples"] == 160
    assert np.abs(res["populations"]["samples"] - [0.75, 0.25]).max() <= 1e-12 and np.abs(res["populations"]["msm"] - [0.75, 0.25]).max() <= 1e-10
    skew = states.compare_populations(np.repeat([0, 1, 2], [10, 10, 100]), model)
    p, q = np.array([10, 10, 100]) + 1e-6, pi * 120 + 1e-6                            # js_pwd's conventions: natural log, the distance
    p, q = p / p.sum(), q / q.sum()
    m = (p + q) / 2
    assert abs(skew["js"] - np.sqrt(((p * np.log(p / m)).sum() + (q * np.log(q / m)).sum()) / 2)) <= 1e-12 and skew["js"] > 0.3
    assert np.isnan(states.compare_populations(np.array([3, 3]), model)["js"])


def test_argument_validation():
    from esmdiff_amd import states
    with pytest.raises(ValueError):
        states.kmeans(np.zeros((10, 17)), 2)
    with pytest.raises(ValueError):
        states.kmeans([], 2)
    with pytest.raises(ValueError):
        states.transition_counts(np.array([0, 1, 0]), 0)
    with pytest.raises(ValueError):
        states.transition_counts(np.array([0, 1, 0]), 1, k=4097)
    with pytest.raises(ValueError):
        states.msm(np.ones((2, 3)), 1)
    model = states.msm(np.array([[5, 1], [1, 5]]), 1)
    for m in (0, 3):
        with pytest.raises(ValueError):
            model.metastable(m)
    assert model.metastable(1).memberships.shape == (2, 1)


def test_command_line_without_the_flag_is_unchanged(tmp_path, monkeypatch):
    from esmdiff_amd import analyze_ensemble, kinetics, states
    stub = {"TM-ens": 0.5, "best_tm": np.array([0.25, 0.75])}
    monkeypatch.setattr(analyze_ensemble, "analyze", lambda *a, **k: dict(stub))
    samples = np.zeros((4, 5, 3))
    monkeypatch.setattr(analyze_ensemble, "load_ca", lambda *a, **k: (samples, [np.zeros((5, 3))], 4, np.arange(4)))
    monkeypatch.setattr(kinetics, "report", lambda *a, **k: {"lagtime": a[3]})
    calls = []
    monkeypatch.setattr(states, "report", lambda *a, **k: calls.append((a, k)) or {"states": a[5], "pi": np.array([0.5, np.nan]), "labels": np.array([1, -1])})
    np.save(tmp_path / "ref.npy", np.zeros((50, 5, 3)))
    args = ["--samples", "ens.pdb", "--targets", "a.pdb", "--output"]
    tica = ["--tica", "--trajectory", str(tmp_path / "ref.npy"), "--lagtime", "7", "--tica_dim", "3", "--tica_chunk", "16"]
    bare = analyze_ensemble.main(args + [str(tmp_path / "bare")])
    assert bare.read_text() == '{\n "TM-ens": 0.5,\n "best_tm": [\n  0.25,\n  0.75\n ]\n}\n'
    plain = analyze_ensemble.main(args + [str(tmp_path / "plain")] + tica)
    assert not calls and plain.read_text() == '{\n "TM-ens": 0.5,\n "best_tm": [\n  0.25,\n  0.75\n ],\n "tica": {\n  "lagtime": 7\n }\n}\n'
    full = analyze_ensemble.main(args + [str(tmp_path / "msm")] + tica + ["--msm", "--msm_states", "12", "--msm_lagtime", "4", "--msm_metastable", "3",
                                                                          "--msm_seed", "5"])
    data = json.loads(full.read_text())
    assert data.pop("msm") == {"states": 12, "pi": [0.5, None], "labels": [1, -1]} and json.dumps(data, indent=1) + "\n" == plain.read_text()
    (a, k), = calls
    assert isinstance(a[0], np.memmap) and a[0].shape == (50, 5, 3) and a[1] is samples and a[2].shape == (1, 5, 3)
    assert a[3:] == (7, 3, 12, 4, 3, 5) and k == {"chunk_frames": 16}
    for bad in (["--msm"], ["--msm", "--tica"], ["--msm", "--trajectory", str(tmp_path / "ref.npy")]):
        with pytest.raises(SystemExit):
            analyze_ensemble.main(args + [str(tmp_path / "bad")] + bad)
    p = analyze_ensemble.parser().parse_args(args + ["o"])
    assert (p.msm, p.msm_states, p.msm_lagtime, p.msm_metastable, p.msm_seed) == (False, 100, None, 2, 0)
    assert "--msm" in analyze_ensemble.__doc__

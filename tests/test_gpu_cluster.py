"""GPU tests of the clustering layer (esmdiff_amd/csrc/cluster.hip through esmdiff_amd/clustering.py, the C ABI and the command
line) against the naive host restatement of the GROMOS algorithm (tests/cluster_ref.py, itself held to a hand-worked example by
tests/test_cluster_cpu.py).  The outputs are integers: every comparison is exact.  No network engine is built anywhere in this
file."""
import ctypes
import json

import numpy as np
import pytest

from tests import cluster_ref as C
from tests import ensemble_ref as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cl():
    from esmdiff_amd import clustering
    return clustering


def _same(got, want, tag=""):
    labels, centres, sizes, K = want
    assert got.n_clusters == K, tag
    assert got.labels.dtype == got.centres.dtype == got.sizes.dtype == np.int32
    assert np.array_equal(got.centres, centres), tag
    assert np.array_equal(got.sizes, sizes), tag
    assert np.array_equal(got.labels, labels), tag


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _adj_from_blocks(d, cutoff, larger, block):
    """adj (uint64 numpy) built through esmdiff_cluster_threshold in blocks of `block` rows."""
    import torch
    from esmdiff_amd import _native as N
    n = d.shape[0]
    adj = torch.zeros((n, (n + 63) // 64), dtype=torch.int64, device="cuda")
    for r0 in range(0, n, block):
        rows = torch.as_tensor(np.ascontiguousarray(d[r0:r0 + block])).cuda()
        assert N.lib().esmdiff_cluster_threshold(_p(rows), rows.shape[0], r0, n, cutoff, int(larger), _p(adj), None) == 0
    return adj


def _gromos_raw(adj_np):
    import torch
    from esmdiff_amd import _native as N
    n = adj_np.shape[0]
    adj = torch.as_tensor(adj_np.view(np.int64)).cuda()
    out = torch.full((3, n), -7, dtype=torch.int32, device="cuda")
    k = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert N.lib().esmdiff_cluster_gromos(_p(adj), n, _p(out[0]), _p(out[1]), _p(out[2]), _p(k), None) == 0
    K = int(k.item())
    labels, centres, sizes = out.cpu().numpy()
    return (labels, centres[:K], sizes[:K], K), adj.cpu().numpy().view(np.uint64)


# ---- 1. the matrix path, exact ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 130, 1030])
def test_cluster_matrix_equals_the_restatement(cl, n):
    """Integer entries 0-9 and cutoff 3: neighbour counts tie often.  The lower triangle is NaN: it is never read."""
    import torch
    rng = np.random.default_rng(3000 + n)
    d = rng.integers(0, 10, size=(n, n)).astype(np.float64)
    want = C.cluster_matrix(d, 3.0)
    d[np.tri(n, k=-1, dtype=bool)] = np.nan
    d[np.diag_indices(n)] = np.nan                          # the diagonal is "neighbour" whatever it holds
    _same(cl.cluster_matrix(d, 3.0), want, f"n={n}")
    assert np.array_equal(np.bincount(want[0], minlength=want[3]), want[2])
    # a tensor on the host or on the device, and row blocks that do not divide n, say the same
    _same(cl.cluster_matrix(torch.as_tensor(d), 3.0, block_rows=50), want, f"n={n} host tensor")
    _same(cl.cluster_matrix(torch.as_tensor(d).cuda(), 3.0), want, f"n={n} device tensor")


# ---- 2. the extremes ----------------------------------------------------------------------------------------------------------
def test_all_singletons_and_one_cluster(cl):
    rng = np.random.default_rng(130)
    d = rng.uniform(1.0, 2.0, size=(130, 130))
    got = cl.cluster_matrix(d, 0.5)
    assert got.n_clusters == 130 and np.array_equal(got.centres, np.arange(130)) and np.array_equal(got.labels, np.arange(130))
    assert np.array_equal(got.sizes, np.ones(130, np.int32))
    got = cl.cluster_matrix(d, 2.5)
    assert got.n_clusters == 1 and got.centres.tolist() == [0] and got.sizes.tolist() == [130] and not got.labels.any()


# ---- 3. similarities and NaN ------------------------------------------------------------------------------------------------
def test_larger_is_closer_and_nan_entries(cl):
    rng = np.random.default_rng(77)
    n = 130
    s = rng.integers(0, 10, size=(n, n)).astype(np.float64)
    s[5, :] = s[:, 5] = np.nan                              # structure 5 is NaN to everyone ...
    s[64, 100] = s[3, 129] = np.nan                         # ... and two single pairs are undefined
    want = C.cluster_matrix(s, 7.0, larger_is_closer=True)
    got = cl.cluster_matrix(s, 7.0, larger_is_closer=True)
    _same(got, want)
    assert got.sizes[got.labels[5]] == 1 and got.centres[got.labels[5]] == 5          # a singleton
    # not the same relation as the distance reading of the same numbers
    assert not np.array_equal(C.neighbours(s, 7.0, True), C.neighbours(s, 7.0, False))
    _same(cl.cluster_matrix(s, 7.0), C.cluster_matrix(s, 7.0))


# ---- 4. blocks ----------------------------------------------------------------------------------------------------------------
def test_threshold_in_blocks_is_bit_identical(cl):
    rng = np.random.default_rng(44)
    n = 130
    d = rng.integers(0, 10, size=(n, n)).astype(np.float64)
    d[7, 70] = np.nan
    for larger in (False, True):
        whole = _adj_from_blocks(d, 3.0, larger, n).cpu().numpy().view(np.uint64)
        blocks = _adj_from_blocks(d, 3.0, larger, 7).cpu().numpy().view(np.uint64)
        assert np.array_equal(whole, blocks)
        want = np.triu(C.neighbours(d, 3.0, larger))        # the bits (i, j >= i), nothing below the diagonal, padding zero
        assert np.array_equal(whole, C.pack(want))
        assert not (whole[:, 2] >> np.uint64(2)).any()      # n = 130: bits 2 .. 63 of the last word are padding


def test_entry_points_refuse_bad_sizes(cl):
    import torch
    from esmdiff_amd import _native as N
    buf = torch.zeros(64, dtype=torch.int64, device="cuda")
    d = torch.zeros(64, dtype=torch.float64, device="cuda")
    lib = N.lib()
    big = N.CLUSTER_MAX_N + 1
    assert lib.esmdiff_cluster_threshold(_p(d), 1, 0, big, 1.0, 0, _p(buf), None) == -5
    assert lib.esmdiff_cluster_threshold(_p(d), 1, 0, 0, 1.0, 0, _p(buf), None) == -1
    assert lib.esmdiff_cluster_threshold(_p(d), 2, 7, 8, 1.0, 0, _p(buf), None) == -1          # rows 7, 8 of an 8 x 8 matrix
    assert lib.esmdiff_cluster_gromos(_p(buf), big, _p(buf), _p(buf), _p(buf), _p(buf), None) == -5
    assert lib.esmdiff_cluster_gromos(_p(buf), 0, _p(buf), _p(buf), _p(buf), _p(buf), None) == -1
    assert not buf.any()


# ---- 5. stray bits ------------------------------------------------------------------------------------------------------------
def test_bits_below_the_diagonal_are_ignored():
    rng = np.random.default_rng(55)
    n = 130
    adj = C.neighbours(rng.integers(0, 10, size=(n, n)).astype(np.float64), 2.0)
    want = C.gromos(adj)
    clean, sym = _gromos_raw(C.pack(np.triu(adj)))
    stray = np.triu(adj) | np.tril(rng.random((n, n)) < 0.3, -1)
    assert not np.array_equal(stray, np.triu(adj))
    dirty, sym2 = _gromos_raw(C.pack(stray))
    for got in (clean, dirty):
        assert got[3] == want[3] and all(np.array_equal(g, w) for g, w in zip(got[:3], want[:3]))
    # the relation comes back symmetric, with zero padding, both times
    assert np.array_equal(sym, C.pack(adj)) and np.array_equal(sym2, C.pack(adj))


# ---- 6. the ensemble path -------------------------------------------------------------------------------------------------
CUTOFF = 2.0


@pytest.fixture(scope="module")
def three_states():
    """Three independent random CA chains (L = 40, 3.8 A steps); members = a state + 0.1 A of Gaussian noise per coordinate,
    randomly rotated and translated; populations 50 / 30 / 20 in shuffled order.  Seed 6 was chosen on the CPU so that every
    intra-state RMSD is below CUTOFF / 2 and every inter-state RMSD above 2 CUTOFF (asserted in the test)."""
    rng = np.random.default_rng(6)
    states = [E.ca_chain(rng, 40) for _ in range(3)]
    origin = rng.permutation(np.repeat([0, 1, 2], [50, 30, 20]))
    S = np.stack([(states[k] + rng.normal(size=(40, 3)) * 0.1) @ E.random_rotation(rng).T + rng.normal(size=3) * 20 for k in origin])
    return S, origin, np.stack(states), E.superpose_pairs(S)[0]


def _same_partition(labels, origin):
    pairs = set(zip(labels.tolist(), origin.tolist()))
    return len(pairs) == len(set(labels.tolist())) == len(set(origin.tolist()))


def test_cluster_ensemble_recovers_three_states(cl, three_states):
    from esmdiff_amd import ensemble
    S, origin, states, host_rmsd = three_states
    same = origin[:, None] == origin[None, :]
    off = ~np.eye(100, dtype=bool)
    assert host_rmsd[same & off].max() < CUTOFF / 2 and host_rmsd[~same].min() > 2 * CUTOFF      # no pair near the threshold
    got = cl.cluster_ensemble(S, CUTOFF)
    assert got.n_clusters == 3 and got.sizes.tolist() == [50, 30, 20]
    assert np.array_equal(got.labels, origin)               # state k has the k-th largest population
    assert all(origin[c] == k for k, c in enumerate(got.centres))
    _same(got, C.cluster_matrix(ensemble.pairwise_rmsd(S), CUTOFF))
    _same(cl.cluster_ensemble(S, CUTOFF, block_rows=16), (got.labels, got.centres, got.sizes, 3))
    _same(cl.cluster_ensemble(S, CUTOFF, block_rows=33), (got.labels, got.centres, got.sizes, 3))
    tm = cl.cluster_ensemble(S, 0.5, metric="tm")
    assert tm.n_clusters == 3 and tm.sizes.tolist() == [50, 30, 20] and _same_partition(tm.labels, origin)
    t = ensemble.tm_matrix(S)
    _same(tm, C.cluster_matrix(0.5 * (t + t.T), 0.5, larger_is_closer=True))
    # a masked residue changes no assignment here, and NaN coordinates are the same mask
    mask = np.ones((100, 40), bool)
    mask[:, 3] = False
    Sn = S.copy()
    Sn[:, 3] = np.nan
    _same(cl.cluster_ensemble(S, CUTOFF, mask=mask), (got.labels, got.centres, got.sizes, 3))
    _same(cl.cluster_ensemble(Sn, CUTOFF), (got.labels, got.centres, got.sizes, 3))


@pytest.mark.parametrize("metric", ["rmsd", "tm", "lddt"])
def test_row_blocks_of_every_metric_equal_the_full_matrix(cl, metric):
    """n = 7, L = 12: the smallest ensemble with a ragged last block at block_rows = 3; a NaN residue in row 0 keeps a mask live.
    The cutoff is the median entry of the metric's own matrix; seed 5 was chosen on the CPU (tests/ensemble_ref.py,
    tests/lddt_ref.py, tests/cluster_ref.py) so that every metric finds more than one cluster and fewer than seven."""
    from esmdiff_amd import ensemble
    S = E.ensemble(np.random.default_rng(5), 7, 12)
    S[0, 4] = np.nan
    d = {"rmsd": ensemble.pairwise_rmsd, "tm": ensemble.tm_matrix, "lddt": ensemble.lddt_matrix}[metric](S)
    if metric != "rmsd":
        d = 0.5 * (d + d.T)
    cutoff = float(np.median(d[np.triu_indices(7, 1)]))
    from_matrix = cl.cluster_matrix(d, cutoff, larger_is_closer=metric != "rmsd")
    assert 1 < from_matrix.n_clusters < 7
    whole = cl.cluster_ensemble(S, cutoff, metric=metric, block_rows=1024)
    for block_rows in (1, 3, 7, 1024):
        got = cl.cluster_ensemble(S, cutoff, metric=metric, block_rows=block_rows)
        for want in (whole, from_matrix):
            _same(got, (want.labels, want.centres, want.sizes, want.n_clusters), f"{metric} block_rows={block_rows}")


# ---- 7. distances to centres and to given states ----------------------------------------------------------------------------
def test_centre_distances_and_state_populations(cl, three_states):
    from esmdiff_amd import ensemble
    S, origin, states, _ = three_states
    got = cl.cluster_ensemble(S, CUTOFF)
    rmsd = ensemble.pairwise_rmsd(S)
    dist = cl.centre_distances(S, got)
    assert dist.shape == (100,) and np.array_equal(dist, rmsd[np.arange(100), got.centres[got.labels]])     # the same kernel: bit for bit
    assert dist[got.centres].max() < 1e-11 and dist.max() < CUTOFF / 2
    t = ensemble.tm_matrix(S)
    tm_dist = cl.centre_distances(S, got, metric="tm")
    np.testing.assert_array_equal(tm_dist, (0.5 * (t + t.T))[np.arange(100), got.centres[got.labels]])
    # the nearest of the three generating states, then of two of them under a cutoff
    to_states = ensemble.pairwise_rmsd(S, states)
    assignment, populations, distance = cl.state_populations(S, states)
    assert assignment.dtype == np.int32 and np.array_equal(assignment, to_states.argmin(1)) and np.array_equal(assignment, origin)
    np.testing.assert_array_equal(populations, [0.5, 0.3, 0.2])
    assert np.array_equal(distance, to_states.min(1))
    assignment, populations, distance = cl.state_populations(S, states[:2], cutoff=CUTOFF)
    assert np.array_equal(assignment, np.where(origin == 2, -1, origin)) and (assignment == -1).sum() == 20
    np.testing.assert_array_equal(populations, [0.5, 0.3])
    assert np.array_equal(distance, to_states[:, :2].min(1)) and distance[origin == 2].min() > 2 * CUTOFF
    # without the cutoff the third state's members go to whichever of the two is nearer
    assignment, populations, _ = cl.state_populations(S, states[:2])
    assert np.array_equal(assignment, to_states[:, :2].argmin(1)) and populations.sum() == 1.0
    # tm: nearest is largest, the cutoff is a floor
    tm_to = 0.5 * (ensemble.tm_matrix(S, states) + ensemble.tm_matrix(states, S).T)
    assignment, populations, distance = cl.state_populations(S, states[:2], cutoff=0.5, metric="tm")
    assert np.array_equal(assignment, np.where(origin == 2, -1, origin)) and np.array_equal(distance, tm_to[:, :2].max(1))


# ---- 8. determinism -----------------------------------------------------------------------------------------------------------
def test_two_calls_give_identical_arrays(cl, three_states):
    S = three_states[0]
    rng = np.random.default_rng(8)
    d = rng.integers(0, 10, size=(1030, 1030)).astype(np.float64)
    for call in (lambda: cl.cluster_matrix(d, 1.0), lambda: cl.cluster_ensemble(S, 5.0), lambda: cl.cluster_ensemble(S, 0.3, metric="tm")):
        a, b = call(), call()
        assert a.n_clusters == b.n_clusters
        assert np.array_equal(a.labels, b.labels) and np.array_equal(a.centres, b.centres) and np.array_equal(a.sizes, b.sizes)


# ---- 9. the command line end to end ---------------------------------------------------------------------------------------
def test_cli_end_to_end(cl, three_states, tmp_path):
    from esmdiff_amd import cluster_ensemble as cli, pdbio
    S = three_states[0][:24]
    files = []
    for i, ca in enumerate(S):
        bb = np.stack([ca + np.array([-0.5, 1.2, 0.3]), ca, ca + np.array([1.1, 0.9, -0.4])], axis=1)       # N, CA, C
        files.append(tmp_path / f"s_{i}.pdb")
        pdbio.write_backbone_pdb(files[-1], "A" * len(ca), bb)
    pdbio.merge_pdbfiles(files, tmp_path / "target3.pdb", verbose=False)
    loaded = pdbio.load_coords(tmp_path / "target3.pdb", max_n_model=None, verbose=False)
    assert loaded.shape == (24, 40, 3)
    for metric, cutoff in (("rmsd", CUTOFF), ("tm", 0.5)):
        json_path, pdb_path = cli.main(["--samples", str(tmp_path / "target3.pdb"), "--cutoff", str(cutoff), "--output",
                                        str(tmp_path / metric), "--metric", metric])
        assert json_path == tmp_path / metric / "target3.clusters.json"
        doc = json.loads(json_path.read_text())
        want = cl.cluster_ensemble(loaded, cutoff, metric=metric)
        assert (doc["metric"], doc["cutoff"], doc["n"], doc["n_clusters"]) == (metric, cutoff, 24, want.n_clusters)
        assert doc["n_clusters"] == len(set(three_states[1][:24].tolist()))
        assert doc["labels"] == want.labels.tolist() and doc["centres"] == want.centres.tolist() and doc["sizes"] == want.sizes.tolist()
        dist = cl.centre_distances(loaded, want, metric=metric)
        dist = 1.0 - dist if metric == "tm" else dist
        assert doc["mean_distance"] == [float(dist[want.labels == k].mean()) for k in range(want.n_clusters)]
        assert doc["max_distance"] == [float(dist[want.labels == k].max()) for k in range(want.n_clusters)]
        assert ("tm_score" in doc) == (metric == "tm")
        reps = pdbio.load_coords(pdb_path, max_n_model=None, verbose=False)
        assert reps.shape == (want.n_clusters, 40, 3)
        for k in range(want.n_clusters):
            assert np.array_equal(reps[k], loaded[want.centres[k]])

"""CPU tests of the clustering layer: the host restatement of the GROMOS algorithm (tests/cluster_ref.py), which the GPU tests hold
esmdiff_amd/csrc/cluster.hip to, against a hand-worked example and the properties any implementation must have; the argument
checks of esmdiff_amd.clustering that come before the device is touched; and the command line's parser and writers with the
clustering call replaced by the restatement."""
import json

import numpy as np
import pytest
import torch

from tests import cluster_ref as C
from tests import ensemble_ref as E


def test_hand_worked_example():
    """Seven points on a line, cutoff 1.5.  Neighbours (self included): 0:{0,1} 1:{0,1,2} 2:{1,2,3} 3:{2,3} 4:{4,5} 5:{4,5} 6:{6}.
    Points 1 and 2 tie with three neighbours: the lower index, 1, is the first centre and takes {0, 1, 2}.  Left: 3:{3} 4:{4,5}
    5:{4,5} 6:{6}; 4 and 5 tie with two: 4 takes {4, 5}.  Left: 3 and 6 tie with one: 3 first, then 6.  Point 3 was a neighbour
    of 2 but not of the centre 1: it ends as a singleton."""
    x = np.array([0.0, 1.0, 2.0, 3.0, 10.0, 11.0, 20.0])
    d = np.abs(x[:, None] - x[None, :])
    labels, centres, sizes, K = C.cluster_matrix(d, 1.5)
    assert K == 4
    assert labels.tolist() == [0, 0, 0, 2, 1, 1, 3] and labels.dtype == np.int32
    assert centres.tolist() == [1, 4, 3, 6]
    assert sizes.tolist() == [3, 2, 1, 1]
    # only the upper triangle is read
    lower_nan = np.where(np.tri(7, k=-1, dtype=bool), np.nan, d)
    again = C.cluster_matrix(lower_nan, 1.5)
    assert again[0].tolist() == labels.tolist() and again[1].tolist() == centres.tolist()
    # as similarities: -d >= -1.5 is the same relation
    sim = C.cluster_matrix(-d, -1.5, larger_is_closer=True)
    assert sim[0].tolist() == labels.tolist() and sim[1].tolist() == centres.tolist() and sim[2].tolist() == sizes.tolist()
    # the cutoff itself is inside (<=); a NaN pair is not a pair
    assert C.cluster_matrix(d, 1.0)[3] == 4 and C.cluster_matrix(d, 0.999)[3] == 7
    d_nan = d.copy()
    d_nan[0, 1] = np.nan
    assert not C.neighbours(d_nan, 1.5)[0, 1] and not C.neighbours(d_nan, 1.5)[1, 0]
    assert C.cluster_matrix(d_nan, 1.5)[0].tolist() == [2, 0, 0, 0, 1, 1, 3]       # 2 now leads alone with {1, 2, 3}


@pytest.mark.parametrize("n", [1, 2, 17, 64, 100])
def test_properties_on_random_relations(n):
    rng = np.random.default_rng(n)
    for density in (0.02, 0.2, 0.7):
        d = rng.random((n, n))
        adj = C.neighbours(d, density)
        assert np.array_equal(adj, adj.T) and adj.diagonal().all()
        labels, centres, sizes, K = C.gromos(adj)
        assert K == len(centres) == len(sizes) and 1 <= K <= n
        assert labels.min() == 0 and labels.max() == K - 1                        # a partition: everyone has one cluster ...
        assert np.array_equal(np.bincount(labels, minlength=K), sizes) and sizes.sum() == n      # ... and the sizes are its
        assert all(adj[centres[labels[i]], i] for i in range(n))                  # every member is a neighbour of its centre
        assert (np.diff(sizes) <= 0).all()                                        # non-increasing
        assert np.array_equal(labels[centres], np.arange(K))                      # centre k has label k
        assert len(set(centres.tolist())) == K


def test_pack_layout():
    adj = np.zeros((65, 65), bool)
    adj[0, 0] = adj[0, 63] = adj[0, 64] = adj[64, 1] = True
    p = C.pack(adj)
    assert p.shape == (65, 2) and p.dtype == np.uint64
    assert p[0, 0] == (1 | (1 << 63)) and p[0, 1] == 1 and p[64, 0] == 2 and p[64, 1] == 0


def test_cluster_matrix_checks_the_shape_before_the_device():
    from esmdiff_amd import clustering
    assert clustering.CLUSTER_MAX_N == 16384
    with pytest.raises(ValueError, match="square"):
        clustering.cluster_matrix(np.zeros((3, 4)), 1.0)
    with pytest.raises(ValueError, match="square"):
        clustering.cluster_matrix(np.zeros(5), 1.0)
    with pytest.raises(ValueError, match="square"):
        clustering.cluster_matrix(torch.zeros(2, 3, 3), 1.0)
    n = clustering.CLUSTER_MAX_N + 1
    big = np.broadcast_to(np.zeros((1, 1)), (n, n))                               # zero strides: 8 bytes
    with pytest.raises(ValueError, match="16384"):
        clustering.cluster_matrix(big, 1.0)
    with pytest.raises(ValueError, match="16384"):
        clustering.cluster_matrix(np.zeros((0, 0)), 1.0)
    with pytest.raises(ValueError, match="metric"):
        clustering.cluster_ensemble(np.zeros((2, 5, 3)), 1.0, metric="gdt")


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_clustering_has_no_cpu_fallback():
    from esmdiff_amd import clustering
    x = np.zeros((2, 5, 3))
    for call in (lambda: clustering.cluster_matrix(np.zeros((2, 2)), 1.0), lambda: clustering.cluster_ensemble(x, 1.0),
                 lambda: clustering.state_populations(x, x)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


# ---- the command line, with the clustering call replaced by the restatement ------------------------------------------------
def _write_ensemble(tmp_path, S, name="target9.pdb"):
    from esmdiff_amd import pdbio
    files = []
    for i, ca in enumerate(S):
        bb = np.stack([ca + np.array([-0.5, 1.2, 0.3]), ca, ca + np.array([1.1, 0.9, -0.4])], axis=1)       # N, CA, C
        files.append(tmp_path / f"s_{i}.pdb")
        pdbio.write_backbone_pdb(files[-1], "A" * len(ca), bb)
    pdbio.merge_pdbfiles(files, tmp_path / name, verbose=False)
    return tmp_path / name


def test_cli_parser():
    from esmdiff_amd import cluster_ensemble as cli
    a = cli.parser().parse_args(["--samples", "x.pdb", "--cutoff", "2.5", "--output", "out"])
    assert (a.samples, a.cutoff, a.output, a.metric, a.max_models, a.seed) == ("x.pdb", 2.5, "out", "rmsd", None, 0)
    a = cli.parser().parse_args(["--samples", "x.pdb", "--cutoff", "0.5", "--output", "out", "--metric", "tm", "--max_models", "7", "--seed", "3"])
    assert (a.metric, a.max_models, a.seed) == ("tm", 7, 3)
    for bad in (["--samples", "x.pdb", "--output", "out"], ["--samples", "x.pdb", "--cutoff", "1", "--output", "o", "--metric", "gdt"]):
        with pytest.raises(SystemExit):
            cli.parser().parse_args(bad)


def test_cli_writers_with_the_restatement(tmp_path, monkeypatch):
    from esmdiff_amd import cluster_ensemble as cli, clustering, pdbio
    rng = np.random.default_rng(11)
    states = [E.ca_chain(rng, 12) for _ in range(2)]
    S = np.stack([states[k] + rng.normal(size=(12, 3)) * 0.1 for k in (1, 0, 0, 1, 0, 0, 0)])
    path = _write_ensemble(tmp_path, S)
    loaded = pdbio.load_coords(path, max_n_model=None, verbose=False)
    seen = {}

    def fake_cluster(samples, cutoff, metric="rmsd", **kw):
        seen["n"] = len(samples)
        seen["rmsd"] = E.superpose_pairs(samples)[0]
        return clustering.Clustering(*C.cluster_matrix(seen["rmsd"], cutoff))

    def fake_distances(samples, result, metric="rmsd"):
        return seen["rmsd"][np.arange(len(samples)), result.centres[result.labels]]

    monkeypatch.setattr(clustering, "cluster_ensemble", fake_cluster)
    monkeypatch.setattr(clustering, "centre_distances", fake_distances)
    json_path, pdb_path = cli.main(["--samples", str(path), "--cutoff", "2.0", "--output", str(tmp_path / "out")])
    assert json_path == tmp_path / "out" / "target9.clusters.json" and pdb_path == tmp_path / "out" / "target9.clusters.pdb"
    doc = json.loads(json_path.read_text())
    assert set(doc) == {"metric", "cutoff", "n", "n_clusters", "sizes", "centres", "models", "labels", "mean_distance", "max_distance"}
    assert (doc["metric"], doc["cutoff"], doc["n"], doc["n_clusters"]) == ("rmsd", 2.0, 7, 2)
    assert doc["sizes"] == [5, 2] and doc["labels"] == [1, 0, 0, 1, 0, 0, 0] and doc["models"] == list(range(7))
    assert doc["labels"][doc["centres"][0]] == 0 and doc["labels"][doc["centres"][1]] == 1
    assert all(0 < m <= x < 1.0 for m, x in zip(doc["mean_distance"], doc["max_distance"]))
    reps = pdbio.load_coords(pdb_path, max_n_model=None, verbose=False)
    assert reps.shape == (2, 12, 3)
    for k in range(2):
        assert np.array_equal(reps[k], loaded[doc["centres"][k]])
    assert sum(ln.startswith("MODEL") for ln in pdb_path.read_text().splitlines()) == 2
    # the representatives' ATOM records are the input's
    blocks = pdbio.split_pdbfile(path, verbose=False)
    for k, block in enumerate(pdbio.split_pdbfile(pdb_path, verbose=False)):
        assert block == blocks[doc["centres"][k]]
    # --max_models: the centres and `models` are positions in the INPUT
    json_path, pdb_path = cli.main(["--samples", str(path), "--cutoff", "2.0", "--output", str(tmp_path / "sub"), "--max_models", "4", "--seed", "5"])
    doc = json.loads(json_path.read_text())
    kept = np.sort(np.random.default_rng(5).choice(7, 4, replace=False)).tolist()
    assert seen["n"] == 4 and doc["n"] == 4 and doc["models"] == kept and set(doc["centres"]) <= set(kept)
    reps = pdbio.load_coords(pdb_path, max_n_model=None, verbose=False)
    for k in range(doc["n_clusters"]):
        assert np.array_equal(reps[k], loaded[doc["centres"][k]])
    # tm: the note is carried, and the document holds 1 - TM
    r = clustering.Clustering(np.array([0, 0, 1], np.int32), np.array([0, 2], np.int32), np.array([2, 1], np.int32), 2)
    doc = cli.report(r, np.array([1.0, 0.75, 1.0]), np.arange(3), "tm", 0.5)
    assert doc["tm_score"] == "[TMSCORE-RECALL], parity unpinned"
    assert doc["mean_distance"] == [0.125, 0.0] and doc["max_distance"] == [0.25, 0.0]

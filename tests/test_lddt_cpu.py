"""CPU tests of the lDDT layer: the numpy restatement tests/lddt_ref.py (the reference of tests/test_gpu_lddt.py) against a
hand-worked case and the definition's edge rules, the C ABI's declaration, and what needs no device in the Python surface."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import lddt_ref as R

ROOT = Path(__file__).resolve().parent.parent


def _line(xs):
    return np.stack([np.asarray(xs, np.float64), np.zeros(len(xs)), np.zeros(len(xs))], axis=1)


def test_hand_worked_example():
    """Native CA at x = 0, 10, 20, 30: only neighbours in the chain are closer than 15 A, so total_res = [1, 2, 2, 1].  Model at
    x = 0, 10, 20.6, 34: the three neighbour distances are 10, 10.6, 13.4, off by 0, 0.6, 3.4 — kept under 4, 3 and 1 of the
    thresholds 0.5, 1, 2, 4.  kept_res = [4, 4 + 3, 3 + 1, 1], global 16 / (4 * 6)."""
    kept, total, kept_res, total_res = R.counts(_line([0, 10, 20.6, 34])[None], _line([0, 10, 20, 30])[None])
    assert total_res.tolist() == [[1, 2, 2, 1]] and total.tolist() == [6]
    assert kept_res.tolist() == [[[4, 7, 4, 1]]] and kept.tolist() == [[16]]
    score, per_res = R.scores(_line([0, 10, 20.6, 34])[None], _line([0, 10, 20, 30])[None])
    assert score[0, 0] == 16 / 24 and per_res[0, 0].tolist() == [1.0, 7 / 8, 0.5, 0.25]


def test_self_comparison_scores_one_and_no_pairs_is_nan():
    rng = np.random.default_rng(0)
    X = np.stack([R.chain(rng, 40) for _ in range(3)])
    score, per_res = R.scores(X)
    assert np.array_equal(np.diag(score), np.ones(3)) and np.all(per_res[np.arange(3), np.arange(3)] == 1.0)
    assert np.all(score[~np.eye(3, dtype=bool)] < 1.0)
    far = _line([0, 20])[None]                                  # the native's one pair is farther than R0
    score, per_res = R.scores(far, far)
    assert np.isnan(score[0, 0]) and np.isnan(per_res).all()


def test_strict_comparisons():
    native = _line([0, 15.0, 29.875])                           # 15.0 is out, 14.875 is in
    kept, total, kept_res, total_res = R.counts(native[None], native[None])
    assert total_res.tolist() == [[0, 1, 1]]
    models = np.stack([_line([0, 10 + d]) for d in (0.5, 1, 2, 4, 0.375, 0.875, 1.875, 3.875)])
    kept = R.counts(models, _line([0, 10])[None])[0]
    assert kept[:, 0].tolist() == [6, 4, 2, 0, 8, 6, 4, 2]      # two ordered pairs each


def test_masked_native_residue_leaves_every_pair_set():
    rng = np.random.default_rng(1)
    native, model = R.chain(rng, 12), R.chain(rng, 12)
    mask = np.ones((1, 12), bool)
    mask[0, 5] = False
    kept, total, kept_res, total_res = R.counts(model[None], native[None], maskB=mask)
    sub = np.delete(np.arange(12), 5)
    # the same as the chain without residue 5, with the chain's own sequence separations (all >= 1 anyway)
    k2, t2, kr2, tr2 = R.counts(model[sub][None], native[sub][None])
    assert total_res[0, 5] == 0 and kept_res[0, 0, 5] == 0
    assert np.array_equal(total_res[0, sub], tr2[0]) and np.array_equal(kept_res[0, 0, sub], kr2[0, 0])
    assert total[0] == t2[0] and kept[0, 0] == k2[0, 0]
    native_nan = native.copy()
    native_nan[5] = np.nan                                       # a masked coordinate is never looked at
    assert np.array_equal(R.counts(model[None], native_nan[None], maskB=mask)[2], kept_res)


def test_masked_model_residue_keeps_nothing_but_stays_in_the_denominator():
    rng = np.random.default_rng(2)
    native = R.chain(rng, 12)
    full = R.counts(native[None], native[None])
    mask = np.ones((1, 12), bool)
    mask[0, 3] = False
    kept, total, kept_res, total_res = R.counts(native[None], native[None], maskA=mask)
    assert np.array_equal(total_res, full[3]) and total[0] == full[1][0]
    assert kept_res[0, 0, 3] == 0
    with_3 = R.distances(native)[3] < 15.0
    with_3[3] = False
    assert np.array_equal(kept_res[0, 0], full[2][0, 0] - 4 * with_3 * (np.arange(12) != 3) - full[2][0, 0] * (np.arange(12) == 3))
    assert kept[0, 0] == full[0][0, 0] - 2 * 4 * with_3.sum()


def test_seq_sep():
    native = _line(np.arange(8) * 3.0)                           # neighbours within 15 A: |a - b| <= 4
    for sep, per_row in ((1, [4, 5, 6, 7, 7, 6, 5, 4]), (3, [2, 2, 2, 3, 3, 2, 2, 2]), (5, [0] * 8)):
        kept, total, kept_res, total_res = R.counts(native[None], native[None], seq_sep=sep)
        assert total_res[0].tolist() == per_row and np.array_equal(kept_res[0, 0], 4 * total_res[0])


def test_header_declares_the_entry_and_the_binding_lists_it():
    from esmdiff_amd import _native as N
    header = (ROOT / "include" / "esmdiff_hip.h").read_text()
    decl = re.search(r"int\s+esmdiff_lddt_pairs\s*\(([^;]*)\)\s*;", header)
    assert decl, "include/esmdiff_hip.h does not declare esmdiff_lddt_pairs"
    args = [a.strip() for a in decl.group(1).split(",")]
    assert len(args) == 16 and args[0] == "const double* A" and args[-1] == "void* stream"
    assert sum(a.startswith("int32_t*") for a in args) == 4        # kept, total, kept_res, total_res: integers
    assert "esmdiff_lddt_pairs" in N.EXPORTS
    assert re.search(r"#define\s+ESMDIFF_ABI_VERSION\s+8\b", header)
    limit = int(re.search(r"#define\s+ESMDIFF_LDDT_MAX_L\s+(\d+)", header).group(1))
    assert limit >= 4096 and limit == N.LDDT_MAX_L
    assert int(re.search(r"#define\s+ESMDIFF_LDDT_MAX_THRESHOLDS\s+(\d+)", header).group(1)) == N.LDDT_MAX_THRESHOLDS == 8
    from esmdiff_amd import build
    assert "-ffp-contract=off" in build.UNITS["lddt"]


def test_read_pdb_bfactors(tmp_path):
    from esmdiff_amd import pdbio
    rng = np.random.default_rng(3)
    files, conf = [], np.round(rng.uniform(0.2, 0.95, size=(3, 9)), 2)
    for i in range(3):
        ca = R.chain(rng, 9)
        bb = np.stack([ca + np.array([-0.5, 1.2, 0.3]), ca, ca + np.array([1.1, 0.9, -0.4])], axis=1)
        files.append(tmp_path / f"s_{i}.pdb")
        pdbio.write_backbone_pdb(files[-1], "ACDEFGHIK", bb, bfactor=conf[i])
    assert np.array_equal(pdbio.read_pdb_bfactors(files[1]), conf[1:2])
    pdbio.merge_pdbfiles(files, tmp_path / "all.pdb", verbose=False)
    got = pdbio.read_pdb_bfactors(tmp_path / "all.pdb")
    assert got.shape == pdbio.load_coords(tmp_path / "all.pdb", max_n_model=None, verbose=False).shape[:2] == (3, 9)
    assert np.array_equal(got, conf)


def test_metric_and_parsers_know_lddt():
    from esmdiff_amd import analyze_ensemble, cluster_ensemble, clustering
    assert clustering.METRICS["lddt"].larger_is_closer is True and clustering.METRICS["rmsd"].larger_is_closer is False
    a = cluster_ensemble.parser().parse_args(["--samples", "x.pdb", "--cutoff", "0.7", "--output", "o", "--metric", "lddt"])
    assert a.metric == "lddt"
    assert "--lddt" in analyze_ensemble.__doc__


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_lddt_has_no_cpu_fallback():
    from esmdiff_amd import clustering, ensemble
    x = np.zeros((2, 5, 3))
    for call in (lambda: ensemble.lddt_matrix(x), lambda: ensemble.lddt(x[0], x[1]), lambda: ensemble.lddt_diversity(x),
                 lambda: clustering.cluster_ensemble(x, 0.5, metric="lddt")):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()

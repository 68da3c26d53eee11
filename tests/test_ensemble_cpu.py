"""CPU tests of the superposition layer's host-side restatement (tests/ensemble_ref.py), which the GPU tests hold the kernels of
esmdiff_amd/csrc/superpose.hip to: it reproduces tests/golden/g13_superposition.npz — the outputs of the reference's own
geo_utils.squared_deviation / _find_rigid_alignment and of scipy's Rotation.align_vectors used as apo_analysis.get_structures
uses it (tests/golden/make_goldens_superposition.py) — under both rotation rules, and its TM-score has the properties any
implementation of the rule must have.  [TMSCORE-RECALL]: the TM search itself is unpinned (no TMscore binary exists here)."""
import numpy as np
import pytest
import torch

from tests import ensemble_ref as E

PLAIN, MIRROR, MASKED, PLANAR, TWO = range(5)
# A noise-free copy aligns to rounding only: coordinates up to ~200 A carry 3e-14 A of float64 rounding each, the rotation a few
# ulp more; 1e-11 A is 300 x that (the bar test_g10_rmsd_after_alignment uses for the same situation is 1e-12 at L = 48, noise 0).
ZERO_RMSD = 1e-11


@pytest.fixture(scope="module")
def g13(golden_dir):
    return np.load(golden_dir / "g13_superposition.npz")


def _case(g, c):
    src, tgt = g[f"src_{c}"], g[f"tgt_{c}"]
    return src, tgt, ~np.isnan(src[:, 0]), ~np.isnan(tgt[:, 0])


def test_g13_reference_rule(g13):
    """allow_reflection = True is geo_utils._find_rigid_alignment: RMSD to rtol 1e-9, squared deviations to 1e-9 A^2, R / t on the
    non-degenerate cases."""
    for c, kind in enumerate(g13["kind"]):
        src, tgt, ma, mb = _case(g13, c)
        rmsd, sd, R, t = E.superpose_pair(src, tgt, ma, mb, allow_reflection=True)
        if g13["noise"][c] == 0:
            assert rmsd < ZERO_RMSD and g13[f"rmsd_{c}"] < ZERO_RMSD, (c, rmsd)
        else:
            np.testing.assert_allclose(rmsd, g13[f"rmsd_{c}"], rtol=1e-9, err_msg=str(c))
        np.testing.assert_allclose(g13[f"rmsd_np_entry_{c}"], g13[f"rmsd_{c}"], rtol=0, atol=0)
        np.testing.assert_allclose(sd, g13[f"sd_{c}"], rtol=0, atol=1e-9, equal_nan=True, err_msg=str(c))
        assert np.array_equal(np.isnan(sd), ~(ma & mb))
        np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-12)
        if kind in (PLAIN, MIRROR, MASKED):
            np.testing.assert_allclose(R, g13[f"R_{c}"], atol=1e-9, err_msg=str(c))
            np.testing.assert_allclose(t, g13[f"t_{c}"], atol=1e-7, err_msg=str(c))


def test_g13_proper_rule_and_get_structures(g13):
    """allow_reflection = False is scipy's align_vectors: on full masks the per-residue distances of get_structures are the Kabsch
    ones; on the masked pair (different residues missing in the two structures) get_structures' own-mask centring is reproduced by
    aligned_deviation_pair.  The mirror image separates the two rules."""
    for c, kind in enumerate(g13["kind"]):
        src, tgt, ma, mb = _case(g13, c)
        want = g13[f"scipy_dist_{c}"]
        got = E.aligned_deviation_pair(src, tgt, ma, mb)
        np.testing.assert_allclose(got ** 2, want ** 2, rtol=0, atol=1e-9, equal_nan=True, err_msg=str(c))
        if kind == MASKED:
            continue
        rmsd, sd, R, t = E.superpose_pair(src, tgt, ma, mb, allow_reflection=False)
        np.testing.assert_allclose(sd, want ** 2, rtol=0, atol=1e-9, err_msg=str(c))
        want_rmsd = np.sqrt(np.mean(want ** 2))
        if g13["noise"][c] == 0 and kind != MIRROR:
            assert rmsd < ZERO_RMSD and want_rmsd < ZERO_RMSD
        else:
            np.testing.assert_allclose(rmsd, want_rmsd, rtol=1e-9, err_msg=str(c))
        np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-12)
        np.testing.assert_allclose(np.linalg.det(R), 1.0, atol=1e-12)
        if kind in (PLAIN, MIRROR):
            np.testing.assert_allclose(R, g13[f"scipy_rot_{c}"].T, atol=1e-9, err_msg=str(c))    # scipy's maps tgt onto src
    c = int(np.flatnonzero(g13["kind"] == MIRROR)[0])
    src, tgt, ma, mb = _case(g13, c)
    assert E.superpose_pair(src, tgt, ma, mb, True)[0] < ZERO_RMSD
    assert E.superpose_pair(src, tgt, ma, mb, False)[0] > 1.0


def test_fewer_than_two_aligned_residues_is_nan():
    rng = np.random.default_rng(0)
    a, b = E.ca_chain(rng, 6), E.ca_chain(rng, 6)
    m = np.array([1, 0, 0, 0, 0, 0], bool)
    rmsd, sd, R, t = E.superpose_pair(a, b, m, None)
    assert np.isnan(rmsd) and np.isnan(sd).all() and np.isnan(R).all() and np.isnan(t).all()
    assert np.isnan(E.tm_pair(a, b, m, None)[0])


def test_fragment_lengths():
    assert E.fragment_lengths(1026) == [1026, 513, 256, 128, 64, 32, 16, 8, 4]
    assert E.fragment_lengths(9) == [9, 4] and E.fragment_lengths(8) == [8, 4] and E.fragment_lengths(5) == [5, 4]
    assert E.fragment_lengths(4) == [4] and E.fragment_lengths(3) == [3] and E.fragment_lengths(2) == [2]


def test_tm_properties_of_the_restatement():
    rng = np.random.default_rng(7)
    a = E.ca_chain(rng, 50)
    moved = a @ E.random_rotation(rng).T + rng.normal(size=3) * 20
    tm, R, t = E.tm_pair(a, moved)
    assert abs(tm - 1.0) < 1e-12                                       # a rigidly moved copy scores 1
    np.testing.assert_allclose(a @ R.T + t, moved, atol=1e-9)
    ens = E.ensemble(rng, 4, 33, noise=2.0)
    tm = E.tm_matrix(ens)
    for i in range(4):
        for j in range(4):
            assert tm[i, j] >= E.tm_at_kabsch(ens[i], ens[j]) - 1e-12   # the first seed IS the global Kabsch fit
            assert 0 < tm[i, j] <= 1 + 1e-12
    np.testing.assert_allclose(tm, tm.T, rtol=0, atol=1e-9)            # full masks: both normalisations are the same number
    # the native's valid residues normalise: masking natives' residues changes Ln and d0, masking the model's only the sum
    mb = np.ones(33, bool)
    mb[:5] = False
    assert E.tm_pair(ens[0], ens[1], None, mb)[0] != pytest.approx(E.tm_pair(ens[0], ens[1], mb, None)[0], abs=1e-6)
    a, b = E.core_case(rng)
    assert E.tm_pair(a, b)[0] >= 0.6 - 1e-9                            # the fragment search finds the rigid core ...
    assert E.tm_at_kabsch(a, b) < 0.5                                  # ... which the global fit alone does not


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_ensemble_has_no_cpu_fallback():
    from esmdiff_amd import ensemble
    x = np.zeros((2, 5, 3))
    for call in (lambda: ensemble.pairwise_rmsd(x), lambda: ensemble.tm_matrix(x), lambda: ensemble.squared_deviation(x, x)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()

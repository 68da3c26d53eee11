"""The inputs of tests/test_gpu_metrics_edges.py bite (no GPU): conditions on tests/metrics_edges_ref.py's builders, not measurements.

Edge lattice: on every (n_bins, D) the device test uses, the oracle's histogram equals numpy.histogram column by column, and each of the
two deliberately wrong histograms moves js_columns by more than 1e-9 — wherever it CAN differ from numpy at all:
  n_bins = 1     no variant can differ (one bin; edge 0 is `first` itself in any rounding),
  n_bins = 3     the fused edge cannot differ (the inner edges are 1 * step and 2 * step, exact products; edge 3 is `last`),
and for those the test asserts that the variant equals numpy on every column instead.  Those sizes stay in the device test for what
they do exercise: the single bin, the right edge closed, values outside, weights.
Boundary ensembles: every chain has exactly the pair / bond it claims, at exactly the claimed distance, and the oracle's answer changes
between "at the bar" and "one ulp below"."""
import numpy as np
import pytest

from oracle import metrics_ref as R
from tests import metrics_edges_ref as E

GRID = [(b, D) for b in E.LATTICE_BINS for D in E.LATTICE_DS]
_cases = {}


def _case(n_bins, D):
    if (n_bins, D) not in _cases:
        _cases[n_bins, D] = E.edge_lattice_columns(n_bins, D, E.lattice_seed(n_bins, D))
    return _cases[n_bins, D]


def _numpy_hist(x, n_bins, lo, hi, w=None):
    with np.errstate(invalid="ignore"):
        return np.histogram(x, bins=n_bins, range=(lo, hi), weights=w)[0]


@pytest.mark.parametrize("n_bins,D", GRID)
def test_oracle_histogram_equals_numpy_on_the_lattice(n_bins, D):
    model, ref = _case(n_bins, D)
    wm, wr = E.lattice_weights(model.shape[0], ref.shape[0], 5)
    assert model.shape == (E.model_rows(n_bins), D) and np.isnan(model[-1]).all() and np.isinf(model[-3:-1]).all()
    assert not np.isnan(model[:-1]).any() and np.isfinite(ref).all() and wm[-1] == 1000.0 and (wm == 0).any() and (wr == 0).any()
    for d in range(D):
        lo, hi = ref[:, d].min(), ref[:, d].max()
        edges = np.linspace(lo, hi, n_bins + 1)
        assert np.isin(edges, model[:, d]).all() and np.isin([lo, hi], ref[:, d]).all()
        assert (model[:-1, d] < lo).sum() >= 3 and (model[:-1, d] > hi).sum() >= 3        # one ulp outside, far outside, infinite
        with np.errstate(invalid="ignore"):
            for x, w in ((model[:, d], None), (ref[:, d], None), (model[:, d], wm), (ref[:, d], wr)):
                assert np.array_equal(R.histogram_equal_width(x, n_bins, lo, hi, w), _numpy_hist(x, n_bins, lo, hi, w)), (d, w is None)


@pytest.mark.parametrize("wrong", [E.histogram_fused_edge, E.histogram_uncorrected], ids=["fused_edge", "uncorrected"])
@pytest.mark.parametrize("n_bins,D", GRID)
def test_wrong_histograms_move_js_columns(n_bins, D, wrong, monkeypatch):
    model, ref = _case(n_bins, D)
    flipped = E.flipped_columns(model, ref, n_bins, wrong)
    if n_bins == 1 or (n_bins == 3 and wrong is E.histogram_fused_edge):
        assert flipped == 0, f"{wrong.__name__} cannot differ from numpy at n_bins = {n_bins}, yet {flipped} of {D} columns flipped"
        return
    with np.errstate(invalid="ignore"):
        want = R.js_columns(model, ref, n_bins)
        monkeypatch.setattr(R, "histogram_equal_width", wrong)
        got = R.js_columns(model, ref, n_bins)
    assert abs(got - want) > 1e-9, (f"{wrong.__name__} at n_bins = {n_bins}, D = {D}, seed {E.lattice_seed(n_bins, D)}: {flipped} of {D} "
                                    f"columns flipped, js_columns moved by {abs(got - want):.3e}; choose another seed")


@pytest.mark.parametrize("n_bins", E.LATTICE_BINS)
def test_widened_and_outside_columns(n_bins):
    model, ref = E.widened_columns(n_bins, 257, 11)
    assert ref.shape == (1, 257)
    for d in (0, 128, 256):
        c = ref[0, d]
        edges = np.linspace(c - 0.5, c + 0.5, n_bins + 1)
        assert np.isin(edges, model[:, d]).all()
        with np.errstate(invalid="ignore"):
            assert np.array_equal(R.histogram_equal_width(model[:, d], n_bins, c, c), _numpy_hist(model[:, d], n_bins, c, c))
    model, ref = E.outside_columns(n_bins, 257, 12)
    assert np.isfinite(model).all() and (model[:, 0] > ref[:, 0].max()).all() and (model[:, -1] < ref[:, -1].min()).all()
    for d in (0, 256):
        assert R.histogram_equal_width(model[:, d], n_bins, ref[:, d].min(), ref[:, d].max()).sum() == 0


def test_the_bars_are_exact():
    assert 3.0 == 2 * 1.7 - 0.4
    for bar in (3.0, 2 * 1.9 - 0.25, E.bonding_threshold(), 3.875, 3.8125):
        for d in (bar, E.below(bar)):
            assert np.sqrt(d * d) == d and np.sqrt((0.0 * 0.0 + d * d) + 0.0 * 0.0) == d
    assert 2 * 1.9 - 0.25 != 3.0 and E.below(E.bonding_threshold()) > 3.875


@pytest.mark.parametrize("L,i,j,k_exclusion", [(6, 1, 4, 0), (6, 1, 4, 2), (6, 1, 3, 1), (40, 38, 39, 0), (40, 10, 30, 0), (40, 10, 30, 7)])
def test_bar_chain_has_one_pair_at_the_bar(L, i, j, k_exclusion):
    bar = 3.0
    for dist, valid in ((bar, 1.0), (E.below(bar), 0.0)):
        ca = E.bar_chain(L, i, j, dist)
        d = R.pairwise_distance_ca(ca, 1)[0]
        at = E.pair_index(L, 1, i, j)
        assert d[at] == dist and (np.delete(d, at) > 3.79).all()                          # every other pair: a spacing or more
        assert R.validity(ca, k_exclusion=k_exclusion) == valid
        assert R.validity(ca, k_exclusion=j - i) == 1.0                                   # at offset k_exclusion: ignored
        assert R.validity(ca, k_exclusion=j - i - 1) == valid                             # at offset k_exclusion + 1: counted
    assert E.pair_index(40, 1, 38, 39) == 40 * 39 // 2 - 1 and E.pair_index(40, 1, 10, 30) >= 256


def test_bar_chain_other_bar_and_last_frame():
    bar = 2 * 1.9 - 0.25
    assert R.validity(E.bar_chain(6, 1, 4, bar), 1.9, 0.25) == 1.0 and R.validity(E.bar_chain(6, 1, 4, E.below(bar)), 1.9, 0.25) == 0.0
    assert R.validity(E.bar_chain(6, 1, 4, bar)) == 1.0 and R.validity(E.bar_chain(6, 1, 4, 3.2), 1.9, 0.25) == 0.0
    ca = E.bar_chain(6, 1, 4, E.below(3.0), 257, [256])
    assert R.validity(ca) == 1.0 - 1.0 / 257 and R.validity(ca[:256]) == 1.0
    assert R.validity(E.straight_chain(1)[None]) == 1.0 and R.validity(E.straight_chain(3)[None], k_exclusion=2) == 1.0


@pytest.mark.parametrize("L,bond", [(300, 0), (300, 255), (300, 256), (300, 298), (2, 0)])
def test_bonding_case_sits_on_the_threshold(L, bond):
    t = E.bonding_threshold()
    for length, want in ((t, 2.0 / 3.0), (E.below(t), 1.0)):
        model, ref = E.bonding_case(L, bond, length)
        adj = R.pairwise_adjacent(ref)
        assert adj.max() == 3.875 == adj[-1, -1] and (np.delete(adj.ravel(), adj.size - 1) == E.BOND).all()
        am = R.pairwise_adjacent(model)
        assert am[2, bond] == length and am[1, bond] == 3.8125 and (am[0] == E.BOND).all() and (np.delete(am[2], bond) == E.BOND).all()
        assert R.bonding_validity(model, ref) == want
        assert R.bonding_validity(model, ref[:2]) == 1.0 / 3.0                            # without the ref's last frame: 3.8125 breaks too


def test_pwd_inputs_round_differently_when_contracted():
    for L, k in E.PWD_CASES:
        if k >= L:
            continue
        ca = E.full_mantissa_coords(E.PWD_FRAMES, L, L)
        want, fused = R.pairwise_distance_ca(ca, k), E.pwd_contracted(ca, k)
        assert want.shape == fused.shape and (want != fused).any(), (L, k)
        assert np.abs(want - fused).max() <= 4 * np.spacing(want.max())


def test_long_ensembles_keep_everything_in_the_tail():
    n, t = E.N_LONG, E.TAIL_START
    assert n > 65536 + 64 and t >= 65600 and min(E.TAIL_CLASHES) >= t and max(E.TAIL_CLASHES) == n - 1
    ca = E.long_validity_ensemble()
    assert ca.shape == (n, 4, 3) and R.validity(ca[:t]) == 1.0 and R.validity(ca) == 1.0 - len(E.TAIL_CLASHES) / n
    assert R.validity(ca[:-1]) != R.validity(ca)
    model, ref = E.long_bonding_model(), E.long_bonding_ref()
    assert R.bonding_validity(model[:t], ref) == 1.0 and R.bonding_validity(model, ref) == (n - len(E.TAIL_CLASHES)) / n
    small = np.stack([E.bent_chain(4), E.bent_chain(4, 1, 3.8125)])
    assert R.bonding_validity(small, ref) == 1.0 and R.bonding_validity(small, ref[:-1]) == 0.5
    big, other = E.long_js_ensemble(1), E.short_js_ensemble(7)
    for cut in (big[:t], big[:-1]):                                                       # losing the tail, or frame n - 1 alone, shows
        assert abs(R.js_pwd(cut, other, 50, 1) - R.js_pwd(big, other, 50, 1)) > 1e-9
        assert abs(R.js_pwd(other, cut, 50, 1) - R.js_pwd(other, big, 50, 1)) > 1e-9
        assert abs(R.js_rg(cut, other) - R.js_rg(big, other)) > 1e-9
        assert abs(R.js_rg(other, cut) - R.js_rg(other, big)) > 1e-9

"""GPU tests of esmdiff_amd/csrc/metrics.hip alone, through the C ABI, at its histogram and launch edges, against oracle/metrics_ref.py
(pinned to the reference project's outputs by g9 / g9b).  The inputs are tests/metrics_edges_ref.py's; tests/test_metrics_edges_cpu.py
shows without a GPU that they bite (a fused or missing edge correction moves the value, each chain has exactly the stated pair at exactly
the stated distance, the long ensembles depend on their tail and on their last frame).
THE BARS are tests/test_metrics.py's: |err| <= 1e-12 on unrounded JS values, 1e-11 with kl; validity and bonding validity, ratios of
integer counts, EQUAL the oracle and the stated fraction; esmdiff_metrics_pwd equals the oracle bit for bit.  Every output starts as
garbage, and a refused call leaves it so.
Shapes: D and n of 1, 255, 256, 257 around the 256-thread block; n_bins of 1, 3, 7, 50; L of 1, 2; pair and bond indices on both sides of
256; 70 000 frames, more than the 65 536 one grid extent holds, with everything that matters from frame 65 600 on and in frame n - 1."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import metrics_ref as R
from tests import metrics_edges_ref as E

pytestmark = pytest.mark.gpu

TOL, TOL_KL = 1e-12, 1e-11
E_INVALID = -1
GARBAGE = -7.25


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _dev(x):
    import torch
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64)).cuda()


def _lib():
    from esmdiff_amd import _native as N
    return N.lib()


def _scalar(fn, *args):
    """An entry whose last two arguments are the output double and the stream -> (code, value); the value starts as GARBAGE."""
    out = ctypes.c_double(GARBAGE)
    code = fn(*args, ctypes.byref(out), None)
    return code, out.value


def _js_columns(model, ref, n_bins, wm=None, wr=None, kl=0, D=None):
    xm, xr, dwm, dwr = _dev(model), _dev(ref), _dev(wm), _dev(wr)
    return _scalar(_lib().esmdiff_metrics_js_columns, _p(xm), model.shape[0], _p(dwm), _p(xr), ref.shape[0], _p(dwr),
                   ref.shape[1] if D is None else D, n_bins, kl)


def _js_pwd(model, ref, n_bins, k, wm=None, wr=None, kl=0):
    xm, xr, dwm, dwr = _dev(model), _dev(ref), _dev(wm), _dev(wr)
    return _scalar(_lib().esmdiff_metrics_js_pwd, _p(xm), model.shape[0], _p(dwm), _p(xr), ref.shape[0], _p(dwr), ref.shape[1], n_bins, k, kl)


def _js_rg(model, ref, n_bins=50, wm=None, wr=None, kl=0):
    xm, xr, dwm, dwr = _dev(model), _dev(ref), _dev(wm), _dev(wr)
    return _scalar(_lib().esmdiff_metrics_js_rg, _p(xm), model.shape[0], _p(dwm), _p(xr), ref.shape[0], _p(dwr), ref.shape[1], n_bins, kl)


def _validity(ca, radius=1.7, overlap=0.4, k_exclusion=0):
    x = _dev(ca)
    return _scalar(_lib().esmdiff_metrics_validity, _p(x), ca.shape[0], ca.shape[1], radius, overlap, k_exclusion)


def _bonding(model, ref):
    xm, xr = _dev(model), _dev(ref)
    return _scalar(_lib().esmdiff_metrics_bonding_validity, _p(xm), model.shape[0], _p(xr), ref.shape[0], ref.shape[1])


def _pwd(ca, k):
    """-> (code, (n, D) array); the output starts as GARBAGE (one element when there is no pair)."""
    import torch
    n, L = ca.shape[:2]
    D = len(np.triu_indices(L, k=k)[0])
    x = _dev(ca)
    out = torch.full((n, max(D, 1)), GARBAGE, dtype=torch.float64, device="cuda")
    code = _lib().esmdiff_metrics_pwd(_p(x), n, L, k, _p(out), None)
    torch.cuda.synchronize()
    return code, out.cpu().numpy()


def _check_columns(model, ref, n_bins, wm=None, wr=None):
    with np.errstate(invalid="ignore"):
        for kl, tol in ((0, TOL), (1, TOL_KL)):
            want = R.js_columns(model, ref, n_bins, wm, wr, bool(kl))
            code, got = _js_columns(model, ref, n_bins, wm, wr, kl)
            assert code == 0 and np.isfinite(want) and abs(got - want) <= tol, (n_bins, ref.shape, kl, wm is not None, code, got, want)


# ---- 1. esmdiff_metrics_js_columns on the edge lattice ------------------------------------------------------------------------------
@pytest.mark.parametrize("D", E.LATTICE_DS)
@pytest.mark.parametrize("n_bins", E.LATTICE_BINS)
def test_js_columns_on_the_edge_lattice(n_bins, D):
    model, ref = E.edge_lattice_columns(n_bins, D, E.lattice_seed(n_bins, D))
    wm, wr = E.lattice_weights(model.shape[0], ref.shape[0], 5)
    _check_columns(model, ref, n_bins)
    _check_columns(model, ref, n_bins, wm, wr)
    _check_columns(model, ref, n_bins, wm, None)
    _check_columns(model, ref, n_bins, None, wr)


@pytest.mark.parametrize("n_bins", E.LATTICE_BINS)
def test_js_columns_single_frames_and_empty_columns(n_bins):
    model, ref = E.edge_lattice_columns(n_bins, 257, E.lattice_seed(n_bins, 257))
    for row in (0, model.shape[0] - 6, model.shape[0] - 1):          # n_model = 1: an in-range frame, an outside one, the NaN frame
        _check_columns(model[row:row + 1], ref, n_bins)
    model, ref = E.widened_columns(n_bins, 257, 11)                  # n_ref = 1: lo == hi in every column
    wm, _ = E.lattice_weights(model.shape[0], 1, 6)
    _check_columns(model, ref, n_bins)
    _check_columns(model, ref, n_bins, wm, np.array([0.75]))
    _check_columns(model[3:4], ref, n_bins)                          # one frame against one frame
    model, ref = E.outside_columns(n_bins, 257, 12)                  # columns 0 and 256: the pseudo count alone
    _check_columns(model, ref, n_bins)
    _check_columns(model[:, :1], ref[:, :1], n_bins)
    _check_columns(model[:, -1:], ref[:, -1:], n_bins)


def test_js_columns_refuses_empty_shapes():
    model, ref = E.edge_lattice_columns(7, 4, 1)
    for D, n_bins in ((0, 7), (-1, 7), (4, 0), (4, -3), (0, 0)):
        for kl in (0, 1):
            assert _js_columns(model, ref, n_bins, kl=kl, D=D) == (E_INVALID, GARBAGE), (D, n_bins, kl)
    assert _js_columns(model, ref, 7)[0] == 0


# ---- 2. esmdiff_metrics_pwd ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,k", E.PWD_CASES)
def test_pwd_is_bitwise_the_oracle(L, k):
    ca = E.full_mantissa_coords(E.PWD_FRAMES, L, L)
    code, got = _pwd(ca, k)
    if k >= L:                                                       # D = 0
        assert code == E_INVALID and (got == GARBAGE).all()
        return
    want = R.pairwise_distance_ca(ca, k)
    assert code == 0 and got.shape == want.shape and np.array_equal(got, want), (L, k, int((got != want).sum()))
    code, one = _pwd(ca[-1:], k)                                     # n = 1
    assert code == 0 and np.array_equal(one, want[-1:])


# ---- 3. esmdiff_metrics_js_rg -------------------------------------------------------------------------------------------------------
SIZES = (1, 255, 256, 257)


@functools.lru_cache(maxsize=None)
def _rg_ensembles(L):
    rng = np.random.default_rng(100 + L)
    steps = rng.normal(size=(L, 3)) + np.array([2.0, 0, 0])
    base = np.cumsum(E.SPACING * steps / np.linalg.norm(steps, axis=-1, keepdims=True), 0)
    ref = base[None] * (1 + 0.08 * rng.normal(size=(257, 1, 1))) + rng.normal(size=(257, L, 3)) * 0.3
    model = base[None] * (1.03 + 0.12 * rng.normal(size=(257, 1, 1))) + rng.normal(size=(257, L, 3)) * 0.5
    return model, ref


@pytest.mark.parametrize("L", (1, 2, 60))
def test_js_rg_around_the_block(L):
    model, ref = _rg_ensembles(L)
    for nm in SIZES:
        for nr in SIZES:
            want = R.js_rg(model[:nm], ref[:nr])
            code, got = _js_rg(model[:nm], ref[:nr])
            assert code == 0 and abs(got - want) <= TOL, (L, nm, nr, code, got, want)
    if L == 1:                                                       # every rg is 0: one widened range, one occupied bin
        assert (R.radius_of_gyration(ref) == 0).all() and _js_rg(model, ref) == (0, 0.0)


def test_js_rg_weights_and_kl():
    model, ref = _rg_ensembles(60)
    model, ref = model[:257], ref[:256]
    rng = np.random.default_rng(8)
    wm, wr = rng.uniform(0.5, 1.5, 257), rng.uniform(0.5, 1.5, 256)
    wm[::5] = 0.0
    for n_bins in (1, 20, 50):
        for kl, tol in ((0, TOL), (1, TOL_KL)):
            want = R.js_rg(model, ref, n_bins, wm, wr, bool(kl))
            code, got = _js_rg(model, ref, n_bins, wm, wr, kl)
            assert code == 0 and abs(got - want) <= tol, (n_bins, kl, code, got, want)


# ---- 4. esmdiff_metrics_validity at the bar -----------------------------------------------------------------------------------------
def _valid(ca, want, **kw):
    """The device equals the oracle and the stated value."""
    oracle = R.validity(ca, kw.get("radius", 1.7), kw.get("overlap", 0.4), kw.get("k_exclusion", 0))
    assert oracle == want and _validity(ca, **kw) == (0, want), (ca.shape, kw, want, oracle, _validity(ca, **kw))


@pytest.mark.parametrize("L,i,j", [(6, 1, 4), (6, 1, 2), (40, 38, 39), (40, 10, 30), (40, 0, 39)])
def test_validity_at_the_bar(L, i, j):
    at, just_below = E.bar_chain(L, i, j, 3.0), E.bar_chain(L, i, j, E.below(3.0))
    _valid(at, 1.0)                                                  # strict <: a pair AT the bar is no clash
    _valid(just_below, 0.0)
    _valid(just_below, 1.0, k_exclusion=j - i)                       # the pair's offset is k_exclusion: ignored
    if j - i > 1:
        _valid(just_below, 0.0, k_exclusion=j - i - 1)               # k_exclusion + 1: counted
        _valid(at, 1.0, k_exclusion=j - i - 1)


def test_validity_other_bar_frames_and_short_chains():
    bar = 2 * 1.9 - 0.25
    _valid(E.bar_chain(6, 1, 4, bar), 1.0, radius=1.9, overlap=0.25)
    _valid(E.bar_chain(6, 1, 4, E.below(bar)), 0.0, radius=1.9, overlap=0.25)
    _valid(E.bar_chain(6, 1, 4, 3.2), 0.0, radius=1.9, overlap=0.25)   # between the two bars
    _valid(E.bar_chain(6, 1, 4, 3.2), 1.0)
    for L, i, j in ((6, 1, 4), (40, 10, 30)):
        ca = E.bar_chain(L, i, j, E.below(3.0), 257, [256])          # only the last frame clashes
        _valid(ca, 1.0 - 1.0 / 257)
        _valid(ca[:256], 1.0)
        _valid(ca[256:], 0.0)                                        # n = 1
        _valid(E.bar_chain(L, i, j, 3.0, 257, [256]), 1.0)
    _valid(E.straight_chain(1)[None], 1.0)                           # L = 1: no pair
    _valid(np.zeros((3, 1, 3)), 1.0)
    _valid(E.bar_chain(3, 0, 2, 1.0), 0.0, k_exclusion=1)
    _valid(E.bar_chain(3, 0, 2, 1.0), 1.0, k_exclusion=2)            # k_exclusion + 1 >= L: no pair
    _valid(E.bar_chain(3, 0, 2, 1.0), 1.0, k_exclusion=7)


# ---- 5. esmdiff_metrics_bonding_validity at the threshold ---------------------------------------------------------------------------
@pytest.mark.parametrize("L,bond", [(300, 0), (300, 255), (300, 256), (300, 298), (2, 0)])
def test_bonding_validity_at_the_threshold(L, bond):
    t = E.bonding_threshold()
    for length, want in ((t, 2.0 / 3.0), (E.below(t), 1.0)):         # strict <: a bond AT max + 1e-6 is broken
        model, ref = E.bonding_case(L, bond, length)
        assert R.bonding_validity(model, ref) == want and _bonding(model, ref) == (0, want), (length, _bonding(model, ref))
        assert _bonding(model[2:], ref) == (0, 0.0 if length == t else 1.0)   # n_model = 1
    model, ref = E.bonding_case(L, bond, t)
    assert R.bonding_validity(model, ref[:2]) == 1.0 / 3.0 and _bonding(model, ref[:2]) == (0, 1.0 / 3.0)   # the last ref frame matters
    assert _bonding(ref, ref) == (0, 1.0)


def test_bonding_validity_refuses_one_atom():
    ca = np.zeros((3, 1, 3))
    assert _bonding(ca, ca) == (E_INVALID, GARBAGE)


# ---- 6. more frames than one grid extent --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _long_js():
    return E.long_js_ensemble(1), E.short_js_ensemble(7)


def test_long_validity_and_bonding_validity():
    n = E.N_LONG
    ca = E.long_validity_ensemble()
    _valid(ca, 1.0 - len(E.TAIL_CLASHES) / n)
    _valid(ca[:-1], 1.0 - (len(E.TAIL_CLASHES) - 1) / (n - 1))
    _valid(ca[:E.TAIL_START], 1.0)
    model, ref = E.long_bonding_model(), E.long_bonding_ref()
    want = (n - len(E.TAIL_CLASHES)) / n
    assert R.bonding_validity(model, ref) == want and _bonding(model, ref) == (0, want), _bonding(model, ref)
    small = np.stack([E.bent_chain(4), E.bent_chain(4, 1, 3.8125)])  # valid only if the ref's last frame was seen
    assert R.bonding_validity(small, ref) == 1.0 and _bonding(small, ref) == (0, 1.0), _bonding(small, ref)
    assert _bonding(small, ref[:-1]) == (0, 0.5)


def test_long_js_pwd_and_js_rg():
    big, other = _long_js()
    for model, ref in ((big, other), (other, big)):                  # the long ensemble as the model, then as the reference
        want = R.js_pwd(model, ref, 50, 1)
        code, got = _js_pwd(model, ref, 50, 1)
        assert code == 0 and abs(got - want) <= TOL, ("js_pwd", model.shape, code, got, want)
        want = R.js_rg(model, ref)
        code, got = _js_rg(model, ref)
        assert code == 0 and abs(got - want) <= TOL, ("js_rg", model.shape, code, got, want)


def test_long_pwd_is_bitwise_the_oracle():
    big, _ = _long_js()
    for k in (1, 3):
        want = R.pairwise_distance_ca(big, k)
        code, got = _pwd(big, k)
        assert code == 0, code
        assert np.array_equal(got[-1], want[-1]) and np.array_equal(got[E.TAIL_START:], want[E.TAIL_START:]), "the tail"
        assert np.array_equal(got, want)

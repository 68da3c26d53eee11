"""esmdiff_rmsd_prepare / esmdiff_rmsd_nearest (csrc/rmsd_nn.hip) through esmdiff_amd/pairs.py against tests/neighbours_ref.py, and the
model level of esmdiff_amd/neighbours.py.  Shapes come from the exported constants (N.RMSD_NN_TILE, N.RMSD_NN_RECT): a few hundred
frames at most.

The error bar of msd is neighbours_ref.bar: 16 (L_sel + 16) u (sum |a|^2 + sum |b|^2) / N about the origin; the reference is the direct
Kabsch deviation by numpy's SVD.  Exact claims (cross products, G, centroids on integer frames; counts, histograms, indices on inputs the
reference shows to be clear of the bar; bit-equality between runs, slot counts and placements) are asserted with ==."""
import numpy as np
import pytest

from tests import neighbours_ref as ref

pytestmark = pytest.mark.gpu


def _N():
    from esmdiff_amd import _native as N
    return N


def _dev(x, dtype=None):
    import torch
    t = torch.as_tensor(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).cuda().contiguous()


def _prep(X, sel=None):
    import torch
    from esmdiff_amd import pairs
    return pairs.rmsd_prepare(_dev(np.asarray(X, np.float64)), None if sel is None else _dev(np.asarray(sel, np.uint8)))


def _np(res):
    return {k: v.cpu().numpy() for k, v in res.items() if hasattr(v, "cpu")}


def _run(A, B=None, sel=None, **kw):
    from esmdiff_amd import pairs
    pa = _prep(A, sel)
    pb = None if B is None else _prep(B, sel)
    kw.setdefault("dense", ("msd", "cross"))
    return _np(pairs.rmsd_nearest(pa, pb, **kw)), pa, pb


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _same(r1, r2, keys=None):
    keys = sorted(r1) if keys is None else keys
    return [k for k in keys if not _bits(r1[k], r2[k])]


def _integer_frames(rng, n, L, sel):
    """Small integer coordinates whose centroid over the selection is an integer."""
    X = rng.integers(-20, 21, size=(n, L, 3)).astype(np.int64)
    idx = np.flatnonzero(sel)
    Nsel = len(idx)
    X[:, idx[-1]] += (-X[:, idx].sum(1)) % Nsel
    assert (X[:, idx].sum(1) % Nsel == 0).all()
    return X


def _selection(kind, L):
    sel = np.ones(L, bool)
    if kind == "first":
        sel[0] = False
    elif kind == "last":
        sel[-1] = False
    elif kind == "interior":
        sel[1:-1:2] = False
    return sel


def _sizes():
    N = _N()
    return [1, 15, 16, 17, N.RMSD_NN_TILE - 1, N.RMSD_NN_TILE + 1, N.RMSD_NN_RECT + 1]


def test_constants_match_the_reference():
    N = _N()
    assert N.RMSD_NN_RECT == ref.RECT and N.RMSD_NN_RECT % N.RMSD_NN_TILE == 0 and N.RMSD_NN_TILE % 16 == 0
    assert [N.rmsd_nn_padded(k) for k in (2, 3, 4, 5, 58, 67)] == [ref.padded(k) for k in (2, 3, 4, 5, 58, 67)] == [4, 4, 4, 8, 60, 68]


# (L, selection, index into the size list for n, for m): every L of the K tail and the padding, every selection kind, every size on both sides
EXACT = [(2, "all", 0, 3), (3, "all", 1, 6), (4, "all", 2, 4), (5, "all", 3, 0), (58, "all", 4, 2), (67, "all", 5, 1), (5, "all", 6, 5),
         (5, "first", 3, 5), (6, "last", 5, 3), (9, "interior", 1, 4), (67, "interior", 2, 6), (58, "first", 6, 0)]


@pytest.mark.parametrize("L,kind,ni,mi", EXACT)
def test_exact_layer_on_integer_frames(L, kind, ni, mi):
    """Integer frames with an integer centroid: cross, G and the centroids equal the int64 restatement; frames with use = 0 at a
    tile's first and last lane, holding NaN and 1e300, change no bit of anything else."""
    import torch
    from esmdiff_amd import pairs
    N = _N()
    n, m = _sizes()[ni], _sizes()[mi]
    sel = _selection(kind, L)
    rng = np.random.default_rng(100 * L + n + m)
    A, B = _integer_frames(rng, n, L, sel), _integer_frames(rng, m, L, sel)
    ca, ga, cb, gb, cross = ref.exact(A, B, sel)
    Af, Bf = A.astype(np.float64), B.astype(np.float64)
    res, pa, pb = _run(Af, Bf, None if kind == "all" else sel)
    for p, c, g in ((pa, ca, ga), (pb, cb, gb)):
        info = p["info"].cpu().numpy()
        assert (info[:, :3] == c).all() and (info[:, 3] == g).all() and (p["use"].cpu().numpy() == 1).all()
    assert (res["cross"] == cross).all()
    assert (res["row_pairs"] == m).all() and (res["col_pairs"] == n).all()

    # the unselected residues are never read: garbage there changes nothing
    if kind != "all":
        Ag = Af.copy()
        Ag[:, ~sel] = np.nan
        res_g, _, _ = _run(Ag, Bf, sel)
        assert not _same(res, res_g)

    # unused frames at a tile's first and last lane: prepare drops the NaN frame and the 1e300 frame (its G overflows) ...
    bad_a = sorted({0, min(n, N.RMSD_NN_TILE) - 1, n - 1})
    bad_b = sorted({0, min(m, 16) - 1, m - 1})
    Ax, Bx = Af.copy(), Bf.copy()
    for k, i in enumerate(bad_a):
        Ax[i, np.flatnonzero(sel)[0]] = np.nan if k % 2 == 0 else 1e300
    for k, j in enumerate(bad_b):
        Bx[j, np.flatnonzero(sel)[-1]] = 1e300 if k % 2 == 0 else np.nan
    s = None if kind == "all" else sel
    pax, pbx = _prep(Ax, s), _prep(Bx, s)
    ua, ub = np.ones(n, bool), np.ones(m, bool)
    ua[bad_a], ub[bad_b] = False, False
    assert (pax["use"].cpu().numpy() == ua).all() and (pbx["use"].cpu().numpy() == ub).all()
    clean = _np(pairs.rmsd_nearest(pax, pbx, cutoffs=(30.0,), bins=8, width=10.0, dense=("msd",)))
    # ... and nearest never reads an unused frame: garbage in its P row and info changes no bit of any output
    for p, bad in ((pax, bad_a), (pbx, bad_b)):
        for k, i in enumerate(bad):
            p["P"][i] = float("nan") if k % 2 else 1e300
            p["info"][i] = 1e300 if k % 2 else float("nan")
    dirty = _np(pairs.rmsd_nearest(pax, pbx, cutoffs=(30.0,), bins=8, width=10.0, dense=("msd",)))
    assert not _same(clean, dirty)
    assert np.isnan(dirty["row_rmsd"][bad_a]).all() and (dirty["row_index"][bad_a] == -1).all() and (dirty["row_pairs"][bad_a] == 0).all()
    assert (dirty["row_sum"][bad_a] == 0).all() and (dirty["row_count"][bad_a] == 0).all() and (dirty["col_count"][bad_b] == 0).all()
    used_a, used_b = int(ua.sum()), int(ub.sum())
    assert (dirty["row_pairs"][ua] == used_b).all() and (dirty["col_pairs"][ub] == used_a).all() and dirty["hist"].sum() == used_a * used_b
    if used_b == 0:
        assert np.isnan(dirty["row_rmsd"]).all() and (dirty["row_index"] == -1).all()
    # the used pairs' msd are the bits of the run without the unused frames' rows and columns in other places (purity)
    if used_a and used_b:
        sub, _, _ = _run(Af[ua], Bf[ub], s, dense=("msd",))
        assert _bits(sub["msd"], dirty["msd"][np.ix_(ua, ub)])


def _cases(kind, rng, L):
    """A (n, L, 3), B (m, L, 3) for the error bar."""
    if kind == "random":
        return ref.chains(rng, 19, L), ref.chains(rng, 35, L)
    if kind == "near":                                     # rotated, shifted copies with 1e-6 of noise: the cancellation bites
        base = ref.chains(rng, 18, L)
        B = np.stack([b @ ref.rotation(rng).T + rng.normal(size=3) * 5 + rng.normal(size=b.shape) * 1e-6 for b in base])
        return base, B
    if kind == "mirror":
        base = ref.chains(rng, 17, L)
        return base, np.stack([(b * np.array([1.0, 1.0, -1.0])) @ ref.rotation(rng).T for b in base])
    if kind == "collinear":
        t = np.arange(L, dtype=np.float64)[:, None] * 3.8
        d = rng.normal(size=(20, 1, 3))
        X = t[None] * d / np.linalg.norm(d, axis=2, keepdims=True) + rng.normal(size=(20, 1, 3)) * 10
        return X[:9], X[9:]
    if kind == "planar":
        X = np.stack([np.concatenate([ref.chain(rng, L)[:, :2], np.zeros((L, 1))], 1) @ ref.rotation(rng).T + rng.normal(size=3) * 10
                      for _ in range(20)])
        return X[:9], X[9:]
    raise AssertionError(kind)


@pytest.mark.parametrize("reflection", [False, True])
@pytest.mark.parametrize("kind", ["random", "near", "mirror", "collinear", "planar"])
@pytest.mark.parametrize("L", [5, 67, 300])
def test_msd_is_within_the_bar(kind, L, reflection):
    import torch
    from esmdiff_amd import pairs
    rng = np.random.default_rng(7 * L + len(kind))
    A, B = _cases(kind, rng, L)
    want, bars = ref.msd_direct(A, B, None, reflection), ref.bar(A, B)
    res, _, _ = _run(A, B, reflection=reflection, dense=("msd",))
    ratio = float((np.abs(res["msd"] - want) / bars).max())
    print(f"MEASURED rmsd_nn msd {kind} L={L} reflection={reflection}: largest |msd - ref| / bar = {ratio:.3e}")
    assert ratio <= 1.0, (kind, L, reflection, ratio)
    if kind == "mirror":                                   # the sigma rule: a mirror image fits exactly only when reflections are allowed
        d = np.diag(res["msd"])
        assert (d <= np.diag(bars)).all() if reflection else (d > 1e6 * np.diag(bars)).all()
    # esmdiff_superpose_pairs' rmsd^2: the same quantity in deviation form, whose own rounding (a rotation applied to L residues and a
    # sum of 3 L squares, all relative to sum |a|^2 + sum |b|^2 about the origin) is covered by one more bar
    old = pairs.superpose(_dev(A), _dev(B), None, None, reflection, ("rmsd",))["rmsd"].cpu().numpy() ** 2
    assert (np.abs(res["msd"] - old) <= 2 * bars).all(), float((np.abs(res["msd"] - old) / bars).max())


@pytest.fixture(scope="module")
def big():
    """One cross problem that spans two rectangles each way and partial tiles, with its CPU reference (shared, left unchanged)."""
    N = _N()
    rng = np.random.default_rng(11)
    n, m, L = N.RMSD_NN_RECT + N.RMSD_NN_TILE + 1, N.RMSD_NN_RECT + 17, 21
    A, B = ref.chains(rng, n, L), ref.chains(rng, m, L)
    # every frame of A gets a near copy in B and the other way round, so the minima are well below the typical distance
    for i in range(0, n, 3):
        B[(7 * i) % m] = A[i] @ ref.rotation(rng).T + rng.normal(size=A[i].shape) * (0.05 + 0.002 * i)
    want, bars = ref.msd_direct(A, B), ref.bar(A, B)
    ref.assert_separated(want, bars)
    return {"A": A, "B": B, "want": want, "bars": bars, "use_a": np.ones(n, bool), "use_b": np.ones(m, bool)}


def test_minima_and_indices(big):
    res, _, _ = _run(big["A"], big["B"], dense=("msd",))
    rmin, rarg, cmin, carg, _ = ref.nearest(big["want"], big["use_a"], big["use_b"])
    assert (res["row_index"] == rarg).all() and (res["col_index"] == carg).all()
    assert (np.abs(res["msd"] - big["want"]) <= big["bars"]).all()
    dmin_r, darg_r, dmin_c, darg_c, _ = ref.nearest(res["msd"], big["use_a"], big["use_b"])
    assert _bits(res["row_rmsd"], np.sqrt(dmin_r)) and _bits(res["col_rmsd"], np.sqrt(dmin_c))
    assert (res["row_index"] == darg_r).all() and (res["col_index"] == darg_c).all()


def test_sums_have_the_published_order(big):
    res, _, _ = _run(big["A"], big["B"], dense=("msd",))
    rmsd = np.sqrt(res["msd"])
    rows, cols = ref.fold_sums(rmsd, big["use_a"], big["use_b"])
    assert _bits(res["row_sum"], rows) and _bits(res["col_sum"], cols)
    n, m = rmsd.shape
    assert (np.abs(res["row_sum"] - rmsd.sum(1)) <= m * ref.U * rmsd.sum(1)).all()       # any order: (m - 1) u sum |x| to first order
    assert (np.abs(res["col_sum"] - rmsd.sum(0)) <= n * ref.U * rmsd.sum(0)).all()
    assert (res["row_pairs"] == m).all() and (res["col_pairs"] == n).all()


def test_slots_and_runs_change_no_bit(big):
    keys = None
    first, _, _ = _run(big["A"], big["B"], cutoffs=(1.0, 5.0), bins=16, width=2.0, slots=1)
    for slots in (None, 1, 3, 1000):
        again, _, _ = _run(big["A"], big["B"], cutoffs=(1.0, 5.0), bins=16, width=2.0, slots=slots)
        assert not _same(first, again, keys), slots
    self1, _, _ = _run(big["A"], None, cutoffs=(1.0, 5.0), bins=16, width=2.0, slots=1)
    for slots in (None, 2, 1000):
        again, _, _ = _run(big["A"], None, cutoffs=(1.0, 5.0), bins=16, width=2.0, slots=slots)
        assert not _same(self1, again), slots


def test_counts_and_histogram_equal_numpy(big):
    want, bars = big["want"], big["bars"]
    rmsd = np.sqrt(want)
    # marks moved off any reference value that is nearer than the bar (none is, on these inputs: the reference asserts it)
    cutoffs = (0.31, 2.03, 9.07, 14.9, 200.0)
    bins, width = 24, 1.3
    ref.assert_clear(want, bars, cutoffs)
    ref.assert_clear(want, bars, width * np.arange(1, bins))
    res, _, _ = _run(big["A"], big["B"], cutoffs=cutoffs, bins=bins, width=width, dense=())
    for t, c in enumerate(cutoffs):
        assert (res["row_count"][:, t] == (rmsd <= c).sum(1)).all() and (res["col_count"][:, t] == (rmsd <= c).sum(0)).all(), c
    hist = np.bincount(np.minimum(bins - 1, np.floor(rmsd / width).astype(np.int64)).reshape(-1), minlength=bins)
    assert (res["hist"] == hist).all()


def test_duplicates_lowest_index_wins_with_equal_bits():
    """Bit-identical frames of B in different blocks, tiles and rectangles: equal msd bits (purity), and the lowest index is the answer."""
    N = _N()
    rng = np.random.default_rng(5)
    n, m, L = 40, N.RMSD_NN_RECT + 40, 13
    A, B = ref.chains(rng, n, L), ref.chains(rng, m, L)
    places = [3, 16 + 3, N.RMSD_NN_TILE + 5, N.RMSD_NN_RECT + 2]
    for j in places:
        B[j] = A[7] + rng.normal(size=(1, 3)) if j == places[0] else B[places[0]]
    res, _, _ = _run(A, B, dense=("msd",))
    for j in places[1:]:
        assert _bits(res["msd"][:, j], res["msd"][:, places[0]])
    assert res["row_index"][7] == places[0]
    Bp = B.copy()                                          # without the first, the next one in index order
    Bp[places[0]] = ref.chain(rng, L) + 500.0
    resp, _, _ = _run(A, Bp, dense=("msd",))
    assert resp["row_index"][7] == places[1]
    # duplicates in A: the columns' minima
    A2 = np.concatenate([A, A[7:8], ref.chains(rng, N.RMSD_NN_RECT, L), A[7:8]])
    res2, _, _ = _run(A2, B[places[0]:places[0] + 1], dense=("msd",))
    assert res2["col_index"][0] == 7 and _bits(res2["msd"][7], res2["msd"][n]) and _bits(res2["msd"][7], res2["msd"][-1])


def test_permuting_b_permutes_the_columns(big):
    rng = np.random.default_rng(3)
    perm = rng.permutation(len(big["B"]))
    r0, _, _ = _run(big["A"], big["B"], cutoffs=(5.0,), dense=("msd",))
    r1, _, _ = _run(big["A"], big["B"][perm], cutoffs=(5.0,), dense=("msd",))
    assert _bits(r0["row_rmsd"], r1["row_rmsd"]) and (perm[r1["row_index"]] == r0["row_index"]).all()
    assert _bits(r0["msd"][:, perm], r1["msd"]) and _bits(r0["row_count"], r1["row_count"])
    assert _bits(r0["col_rmsd"][perm], r1["col_rmsd"]) and _bits(r0["col_index"][perm], r1["col_index"])
    assert _bits(r0["col_sum"][perm], r1["col_sum"]) and _bits(r0["col_count"][perm], r1["col_count"])


@pytest.mark.parametrize("which", [0, 1, 2, 3, 4])
def test_self_mode(which):
    """An ensemble against itself: the diagonal excluded, pairs = used - 1, each unordered pair once in the histogram, the dense msd
    symmetric, every row output the cross run's with the diagonal taken out."""
    N = _N()
    n = [1, 2, 17, N.RMSD_NN_TILE + 1, N.RMSD_NN_RECT + N.RMSD_NN_TILE + 3][which]
    rng = np.random.default_rng(40 + n)
    L = 11
    X = ref.chains(rng, n, L)
    for i in range(0, n // 2, 2):                          # near copies, so that cutoffs and minima have something to find
        X[n - 1 - i] = X[i] @ ref.rotation(rng).T + rng.normal(size=X[i].shape) * (0.1 + 0.01 * i)
    dropped = [n // 2] if n > 2 else []
    X[dropped] = np.nan
    use = np.ones(n, bool)
    use[dropped] = False
    used = int(use.sum())
    cutoffs, bins, width = (1.07, 8.3), 12, 2.9
    res, _, _ = _run(X, None, cutoffs=cutoffs, bins=bins, width=width)
    assert "col_rmsd" not in res
    Xc = np.where(use[:, None, None], X, 0.0)
    want, bars = ref.msd_direct(Xc, Xc), ref.bar(Xc, Xc)
    rmin, rarg, _, _, ok = ref.nearest(want, use, None)
    off = ok
    assert (np.abs(res["msd"] - want)[off] <= bars[off]).all()
    assert _bits(res["msd"], res["msd"].T) and (np.diag(res["msd"])[use] == 0).all() and np.isnan(res["msd"][~use]).all()
    assert _bits(res["cross"].reshape(n, n, 3, 3), res["cross"].reshape(n, n, 3, 3).transpose(1, 0, 3, 2))
    assert (res["row_pairs"] == np.where(use, used - 1, 0)).all()
    assert res["hist"].sum() == used * (used - 1) // 2
    if used > 2:
        ref.assert_separated(np.where(off, want, np.nan), bars[off].max())
    assert (res["row_index"] == rarg).all()
    dmin, darg, _, _, _ = ref.nearest(res["msd"], use, None)
    assert _bits(res["row_rmsd"], np.sqrt(dmin))
    rows, _ = ref.fold_sums(np.sqrt(np.where(off, res["msd"], 0.0)), use, None)
    assert _bits(res["row_sum"], rows)
    ref.assert_clear(np.where(off, want, np.nan), bars, cutoffs + tuple(width * np.arange(1, bins)))
    rm = np.sqrt(np.where(off, want, np.inf))
    for t, c in enumerate(cutoffs):
        assert (res["row_count"][:, t] == (rm <= c).sum(1)).all()
    iu = np.triu(off, 1)
    hist = np.bincount(np.minimum(bins - 1, np.floor(np.sqrt(want[iu]) / width).astype(np.int64)), minlength=bins)
    assert (res["hist"] == hist).all()


def test_error_returns_write_nothing():
    import ctypes
    import torch
    from esmdiff_amd import pairs
    N = _N()
    rng = np.random.default_rng(1)
    X = _dev(ref.chains(rng, 5, 6))
    P, info, use = torch.full((5, 3, 8), 7.0, device="cuda", dtype=torch.float64), torch.full((5, 4), 7.0, device="cuda", dtype=torch.float64), \
        torch.full((5,), 7, device="cuda", dtype=torch.uint8)
    sel = _dev(np.array([1, 0, 0, 0, 0, 0], np.uint8))
    p, st = pairs._p, pairs._stream()
    assert N.lib().esmdiff_rmsd_prepare(p(X), 5, 6, p(sel), 1, p(P), p(info), p(use), st) == -1
    torch.cuda.synchronize()
    assert (P == 7).all() and (info == 7).all() and (use == 7).all()
    with pytest.raises(RuntimeError, match="selected residues"):
        pairs.rmsd_prepare(X, sel)

    a = pairs.rmsd_prepare(X)
    out = torch.full((5,), 7.0, device="cuda", dtype=torch.float64)
    hist = torch.full((4,), 7, device="cuda", dtype=torch.int64)
    cut = (ctypes.c_double * 9)(*range(1, 10))
    size = N.rmsd_nn_scratch_bytes(5, 0, 1)
    scratch = torch.zeros(size // 8, device="cuda", dtype=torch.int64)
    null = ctypes.c_void_p(0)

    def call(T=0, bins=0, n_sel=6, bytes_=size):
        return N.lib().esmdiff_rmsd_nearest(p(a["P"]), p(a["info"]), p(a["use"]), 5, null, null, null, 0, n_sel, 0, cut, T, bins, 1.0,
                                            p(out), *[null] * 9, p(hist), null, null, p(scratch), bytes_, st)
    assert call(T=9) == -1 and call(bins=-1) == -1 and call(n_sel=1) == -1
    assert call(bytes_=size - 8) == -5 and call(bins=N.RMSD_NN_MAX_BINS + 1) == -5
    torch.cuda.synchronize()
    assert (out == 7).all() and (hist == 7).all()
    assert call(T=8, bins=4) == 0 and not (out == 7).any() and int(hist.sum()) == 10
    with pytest.raises(RuntimeError, match="cutoffs"):
        pairs.rmsd_nearest(a, cutoffs=tuple(range(9)))
    with pytest.raises(RuntimeError, match="scratch"):
        pairs.rmsd_nearest(a, scratch_bytes=size - 8)


# ---- the model level: esmdiff_amd/neighbours.py ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted():
    """K = 4 well-separated states (independent random chains: tens of Angstrom apart), an MD-like trajectory that visits all of them
    with 0.2 A of noise under random rigid motions, and samples around the first three only."""
    rng = np.random.default_rng(21)
    K, L, n_traj, n_samples = 4, 37, 301, 45
    states = ref.chains(rng, K, L)
    move = lambda x: x @ ref.rotation(rng).T + rng.normal(size=3) * 30
    label = rng.integers(0, K, size=n_traj)
    traj = np.stack([move(states[k] + rng.normal(size=(L, 3)) * 0.2) for k in label])
    slabel = rng.integers(0, K - 1, size=n_samples)
    samples = np.stack([move(states[k] + rng.normal(size=(L, 3)) * 0.2) for k in slabel])
    return {"states": states, "traj": traj, "label": label, "samples": samples, "slabel": slabel, "K": K}


def test_coverage_finds_the_uncovered_state(planted):
    from esmdiff_amd import neighbours
    cut = (0.05, 2.0)                                      # below the noise; between the noise (0.2 A a coordinate) and the separation
    c = neighbours.coverage(planted["samples"], planted["traj"], cut)
    missing = np.flatnonzero(planted["label"] == planted["K"] - 1)
    assert list(c["unrecalled"][1]) == list(missing) and len(missing) > 0
    assert c["recall"][1] == pytest.approx(1 - len(missing) / len(planted["traj"])) and c["precision"][1] == 1.0
    assert c["recall"][0] == 0.0 and c["precision"][0] == 0.0 and len(c["novel"]) == 0
    assert (planted["label"][c["nearest_frame"]] == planted["slabel"]).all()
    covered = planted["label"] != planted["K"] - 1
    assert (planted["slabel"][c["nearest_sample"][covered]] == planted["label"][covered]).all()
    share = np.array([(planted["label"] == k).mean() for k in planted["slabel"]])
    assert np.allclose(c["density"][:, 1], share, atol=1e-12)
    w = np.where(covered, 1.0, 0.0)
    assert neighbours.coverage(planted["samples"], planted["traj"], cut, weights=w)["recall"][1] == 1.0
    far = neighbours.coverage(planted["traj"], planted["samples"], cut)     # the other way round: the fourth state's frames are novel
    assert list(far["novel"]) == list(missing)


def test_memmap_in_chunks_gives_the_same_bits(planted, tmp_path):
    from esmdiff_amd import neighbours
    np.save(tmp_path / "traj.npy", planted["traj"])
    mm = np.load(tmp_path / "traj.npy", mmap_mode="r")
    kw = dict(cutoffs=(0.5, 2.0), hist_bins=20, hist_max=60.0)
    whole = neighbours.nearest(planted["samples"], planted["traj"], **kw)
    for chunk in (64, 300):
        parts = neighbours.nearest(planted["samples"], mm, chunk_frames=chunk, **kw)
        for k, v in vars(whole).items():
            w = getattr(parts, k)
            assert _bits(np.asarray(v), np.asarray(w)) if isinstance(v, np.ndarray) else v == w, (chunk, k)
    one = neighbours.nearest(mm, None, chunk_frames=50, **kw)
    two = neighbours.nearest([planted["traj"][:100], planted["traj"][100:]], None, **kw)
    assert all(_bits(getattr(one, k), getattr(two, k)) for k in ("rmsd_a", "index_a", "sum_a", "count_a", "hist")) and one.rmsd_b is None
    assert one.n_pairs == 301 * 300 // 2 == int(one.hist.sum())


def test_best_per_state_and_self_statistics(planted):
    from esmdiff_amd import ensemble, neighbours
    S, T = planted["samples"], planted["states"]
    rmsd, index = neighbours.best_per_state(S, T, reflection=True)
    sd = np.stack([ensemble.squared_deviation(S, np.broadcast_to(t, S.shape).copy()).mean(1) for t in T], 1)      # (n, K) msd, the reference's rule
    bars = ref.bar(S, T)
    assert (np.abs(rmsd ** 2 - sd.min(0)) <= 2 * bars.max()).all() and (index == sd.argmin(0)).all()
    # the mean pairwise RMSD and its histogram against the dense route
    dense = ensemble.pairwise_rmsd(S)
    iu = np.triu_indices(len(S), 1)
    assert neighbours.mean_pairwise_rmsd(S) == pytest.approx(dense[iu].mean(), rel=1e-9)
    hist, edges = neighbours.rmsd_distribution(S, 30, 60.0)
    assert hist.sum() == len(iu[0]) and (np.abs(hist - np.histogram(dense[iu], edges)[0]).sum() <= 2)
    js = neighbours.js_pairwise_rmsd({"target": planted["traj"][:120], "samples": S, "same": planted["traj"][:120]})
    assert js["target"] == 0.0 and js["same"] == 0.0 and 0.0 < js["samples"] < 1.0
    # a residue set, and frames that are not finite on it
    sel = np.ones(S.shape[1], bool)
    sel[[0, 5]] = False
    S2 = S.copy()
    S2[:, 5] = np.nan
    S2[3, 7] = np.nan
    nb = neighbours.nearest(S2, T, select=sel, cutoffs=(2.0,))
    assert list(np.flatnonzero(~nb.used_a)) == [3] and nb.index_a[3] == -1 and np.isnan(nb.rmsd_a[3]) and (nb.pairs_b == len(S) - 1).all()
    auto = neighbours.nearest(S2[4:], T)                   # default: the residues finite in both first frames
    assert list(np.flatnonzero(~auto.select)) == [5] and auto.used_a.all()


def test_coverage_report_block(planted, monkeypatch):
    from esmdiff_amd import analyze_ensemble
    S, T = planted["samples"], planted["states"]
    monkeypatch.setattr(analyze_ensemble, "load_ca", lambda *a, **k: (S, list(T[:2]), len(S), np.arange(len(S))))
    monkeypatch.setattr(analyze_ensemble, "_trajectory", lambda *a, **k: (planted["traj"], 100))
    block = analyze_ensemble.coverage_report("s.pdb", ["a.pdb", "b.pdb"], "t.npy", cutoffs=(0.05, 2.0))
    assert block["precision"] == [0.0, 1.0] and block["frames_used"] == 301 and block["samples_dropped"] == 0 and block["n_residues"] == 37
    assert (planted["slabel"][block["targets"]["nearest_sample"]] == [0, 1]).all() and (planted["label"][block["targets"]["nearest_frame"]] == [0, 1]).all()
    assert block["mean_pairwise_rmsd"]["samples"] > 1.0 and block["mean_pairwise_rmsd"]["trajectory"] > 1.0
    assert analyze_ensemble._jsonable(block)["recall"][1] == block["recall"][1]

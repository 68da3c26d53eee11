"""GPU tests of the kinetics layer (esmdiff_amd/csrc/lagged.hip through the C ABI and esmdiff_amd/pairs.py, esmdiff_amd/kinetics.py)
against the numpy restatement tests/kinetics_ref.py and, at model level, oracle/metrics_ref.tica_fit.  Every output starts as garbage.
THE BARS.  Integer operands: the five outputs of the moments entry EQUAL the int64 restatement.  Coordinates against features: the
coordinate form equals the feature form run on esmdiff_metrics_pwd's output bit for bit.  Means, residual sums and the projection:
bit-equal to the restatement's published order, and within 2 gamma_m mean|x| / 2 gamma_D sum |f - mean| |W|.  Moments of real operands:
|S_dev - S_ref| <= 2 gamma_m |a|^T |b| elementwise (any order of summation, with or without FMA).  Two calls are bit-identical, whatever
the number of scratch slots.  Model level, after asserting that the input is well posed (eigenvalue gaps >= 0.05, no eigenvalue of c00
within a factor 1.5 of epsilon): eigenvalues, timescales' inputs, projections and js_tica within 1e-6 of the oracle (the project's
device-vs-scipy figure for this quantity).
Shapes: D of 1, 15, 16, 17, 66 around the 16-wide MFMA block and the 64-wide tile (66: two tiles, the second one 2 wide); m of 1, 3, 4,
5 around the four frames of an instruction; m of FRAME_CHUNK - 1, FRAME_CHUNK + 1, 2 FRAME_CHUNK + 3 around the chunk; lag 1 and
FRAME_CHUNK + 2.  The caller's-stream contract is held in tests/test_gpu_stream_tica.py."""
import ctypes

import numpy as np
import pytest

from tests import kinetics_ref as R

pytestmark = pytest.mark.gpu

FC = R.FRAME_CHUNK
NAMES = ("S00", "S0t", "Stt", "r0", "rt")
E_INVALID = -1
GARBAGE = -7.25


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _dev(x):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64)).cuda()


def _shape(X, pwd_offset):
    return X.shape[1], (X.shape[1] if pwd_offset == 0 else R.n_features(X.shape[1], pwd_offset))


def _moments(X, lag, c, pwd_offset=0, slots=1, scratch_bytes=None, null=(), **over):
    """esmdiff_lagged_moments on numpy inputs -> (code, {name: array}); outputs and scratch start as garbage."""
    import torch
    from esmdiff_amd import _native as N
    n = X.shape[0]
    L_or_D, D = _shape(X, pwd_offset)
    D = max(D, 1)
    x, cd = _dev(X), _dev(c)
    out = {k: torch.full((D, D) if k[0] == "S" else (D,), GARBAGE, dtype=torch.float64, device="cuda") for k in NAMES}
    size = R.scratch_bytes(D, slots, True) if scratch_bytes is None else scratch_bytes
    scratch = torch.full((max(size, 8) // 8,), GARBAGE, dtype=torch.float64, device="cuda")
    arg = lambda k, t: None if k in null else t
    code = N.lib().esmdiff_lagged_moments(_p(arg("X", x)), over.get("n", n), over.get("L_or_D", L_or_D), pwd_offset, lag, _p(arg("center", cd)),
                                          *[_p(arg(k, out[k])) for k in NAMES], _p(arg("scratch", scratch)), size, None)
    torch.cuda.synchronize()
    return code, {k: v.cpu().numpy() for k, v in out.items()}


def _means(X, lag, pwd_offset=0, slots=1, scratch_bytes=None, **over):
    import torch
    from esmdiff_amd import _native as N
    L_or_D, D = _shape(X, pwd_offset)
    D = max(D, 1)
    x = _dev(X)
    m0, mt = (torch.full((D,), GARBAGE, dtype=torch.float64, device="cuda") for _ in range(2))
    size = R.scratch_bytes(D, slots, False) if scratch_bytes is None else scratch_bytes
    scratch = torch.full((max(size, 8) // 8,), GARBAGE, dtype=torch.float64, device="cuda")
    code = N.lib().esmdiff_lagged_means(_p(x), over.get("n", X.shape[0]), over.get("L_or_D", L_or_D), pwd_offset, lag, _p(m0), _p(mt), _p(scratch), size, None)
    torch.cuda.synchronize()
    return code, m0.cpu().numpy(), mt.cpu().numpy()


def _project(X, mean, W, pwd_offset=0, dim=None, **over):
    import torch
    from esmdiff_amd import _native as N
    L_or_D, D = _shape(X, pwd_offset)
    x, md, wd = _dev(X), _dev(mean), _dev(W)
    dim = W.shape[1] if dim is None else dim
    Y = torch.full((max(X.shape[0], 1), max(W.shape[1], 1)), GARBAGE, dtype=torch.float64, device="cuda")
    scratch = torch.full((max(D, 1),), GARBAGE, dtype=torch.float64, device="cuda")
    code = N.lib().esmdiff_lagged_project(_p(x), X.shape[0], over.get("L_or_D", L_or_D), pwd_offset, _p(md), _p(wd), dim, _p(Y), _p(scratch),
                                          max(D, 1) * 8, None)
    torch.cuda.synchronize()
    return code, Y.cpu().numpy()


def _integers(rng, n, D, lag):
    """Integer features in [-512, 512] in which feature 0 LEADS the last one by `lag` (an asymmetric S0t), and a centre in [-8, 8]."""
    F = rng.integers(-512, 513, size=(n, D)).astype(np.float64)
    if D > 1:
        F[lag:, D - 1] = F[:n - lag, 0]
    return F, rng.integers(-8, 9, size=D).astype(np.float64)


def _exact(F, lag, c, slots=1):
    code, got = _moments(F, lag, c, 0, slots)
    assert code == 0
    want = R.moments_int(F, lag, c)
    tag = f"n = {F.shape[0]}, D = {F.shape[1]}, lag = {lag}"
    assert max(np.abs(v).max() for v in want.values()) < 2 ** 53, tag
    for k in NAMES:
        assert np.array_equal(got[k], want[k].astype(np.float64)), f"{tag}: {k}"
    assert np.array_equal(got["S00"], got["S00"].T) and np.array_equal(got["Stt"], got["Stt"].T), tag
    return got


@pytest.mark.parametrize("D", [1, 15, 16, 17, 66])
def test_integer_moments_equal_int64_around_the_tile_and_the_instruction(D):
    rng = np.random.default_rng(100 + D)
    for m in (1, 3, 4, 5):
        for lag in (1, 3):
            F, c = _integers(rng, m + lag, D, lag)
            got = _exact(F, lag, c)
            if D > 1 and m > 1:
                assert not np.array_equal(got["S0t"], got["S0t"].T)      # both triangles are compared against an asymmetric matrix
    F, c = _integers(rng, 700, D, 7)
    got = _exact(F, 7, c, slots=2)
    if D > 1:
        # feature 0 leads the last one by the lag: S0t sees it above the diagonal and not below
        assert got["S0t"][0, D - 1] > 0.5 * got["S00"][0, 0] and abs(got["S0t"][D - 1, 0]) < 0.2 * got["S0t"][0, D - 1]


@pytest.mark.parametrize("m", [FC - 1, FC + 1, 2 * FC + 3])
@pytest.mark.parametrize("lag", [1, FC + 2])
def test_integer_moments_equal_int64_around_the_frame_chunk(m, lag):
    rng = np.random.default_rng(m + lag)
    F, c = _integers(rng, m + lag, 17, lag)
    one = _exact(F, lag, c, slots=1)
    many = _exact(F, lag, c, slots=5)                                       # more slots than chunks: the same rounds' sums
    for k in NAMES:
        assert np.array_equal(one[k], many[k]), k


@pytest.mark.parametrize("L", [2, 7, 12])
@pytest.mark.parametrize("k", [1, 3])
def test_the_coordinate_form_equals_the_feature_form_bit_for_bit(L, k):
    import torch
    from esmdiff_amd import metrics
    if k >= L:
        code, got = _moments(np.zeros((10, L, 3)), 2, np.zeros(1), k)
        assert code == E_INVALID and all(np.all(v == GARBAGE) for v in got.values())
        return
    rng = np.random.default_rng(L * 10 + k)
    n, lag = FC + 37, 5
    X = np.cumsum(rng.standard_normal((n, L, 3)) * 2.2, axis=1) + rng.standard_normal((n, 1, 3)) * 30.0
    F = metrics.pairwise_distance_ca(torch.as_tensor(X), k).cpu().numpy()
    assert np.array_equal(F, R.features(X, k)) and F.shape[1] == R.n_features(L, k)
    code_c, m0c, mtc = _means(X, lag, k)
    code_f, m0f, mtf = _means(F, lag, 0)
    assert code_c == 0 and code_f == 0 and np.array_equal(m0c, m0f) and np.array_equal(mtc, mtf)
    c = (m0f + mtf) / 2.0
    (code_c, mc), (code_f, mf) = _moments(X, lag, c, k), _moments(F, lag, c, 0)
    assert code_c == 0 and code_f == 0
    for name in NAMES:
        assert np.array_equal(mc[name], mf[name]), name
    W = rng.standard_normal((F.shape[1], 3))
    (code_c, yc), (code_f, yf) = _project(X, c, W, k), _project(F, c, W, 0)
    assert code_c == 0 and code_f == 0 and np.array_equal(yc, yf)


@pytest.fixture(scope="module")
def real():
    """One trajectory of real operands and its restated moments, shared by the tests below and never written."""
    n, L, lag = 2 * FC + 77, 12, 9
    X = R.trajectory(n, L, seed=3)
    m0, mt = R.means(X, lag, 1)
    c = (m0 + mt) / 2.0
    return {"X": X, "lag": lag, "m": n - lag, "mean0": m0, "meant": mt, "c": c, "ref": R.moments(X, lag, c, 1),
            "env": R.moments_envelope(X, lag, c, 1), "F": R.features(X, 1)}


def test_means_have_the_published_bits_and_hold_the_bound(real):
    code, m0, mt = _means(real["X"], real["lag"], 1, slots=2)
    assert code == 0
    m, F = real["m"], real["F"]
    bar0, bart = 2 * R.gamma(m) * np.abs(F[:m]).mean(0), 2 * R.gamma(m) * np.abs(F[real["lag"]:]).mean(0)
    ratio = max((np.abs(m0 - F[:m].mean(0)) / bar0).max(), (np.abs(mt - F[real["lag"]:].mean(0)) / bart).max())
    print(f"MEASURED lagged means: {ratio:.3g} of the bar 2 gamma_m mean|x| (m = {m}) against numpy's pairwise mean; "
          f"bit-equal to the published order: {np.array_equal(m0, real['mean0']) and np.array_equal(mt, real['meant'])}")
    assert ratio <= 1.0
    assert np.array_equal(m0, real["mean0"]) and np.array_equal(mt, real["meant"])


def test_real_moments_hold_the_any_order_bound_and_repeat(real):
    code, got = _moments(real["X"], real["lag"], real["c"], 1, slots=1)
    assert code == 0
    g = 2 * R.gamma(real["m"])
    worst = 0.0
    for k in ("S00", "S0t", "Stt"):
        ratio = (np.abs(got[k] - real["ref"][k]) / (g * real["env"][k])).max()
        worst = max(worst, ratio)
        assert ratio <= 1.0, (k, ratio)
    print(f"MEASURED lagged moments: {worst:.3g} of the bar 2 gamma_m |a|^T |b| (m = {real['m']}, gamma_m = {R.gamma(real['m']):.3g})")
    for k in ("r0", "rt"):
        assert np.array_equal(got[k], real["ref"][k]), k                     # the residual sums have a published order
        assert (np.abs(got[k] - real["ref"][k]) <= g * real["env"][k]).all()
    assert np.array_equal(got["S00"], got["S00"].T) and np.array_equal(got["Stt"], got["Stt"].T)
    again = _moments(real["X"], real["lag"], real["c"], 1, slots=1)[1]
    wide = _moments(real["X"], real["lag"], real["c"], 1, slots=3)[1]
    for k in NAMES:
        assert np.array_equal(got[k], again[k]) and np.array_equal(got[k], wide[k]), k


def test_projection_bits_bound_and_batch_independence(real):
    rng = np.random.default_rng(5)
    X, F = real["X"][:301], real["F"][:301]
    for dim in (1, 2, 16):
        W = rng.standard_normal((F.shape[1], dim))
        code, Y = _project(X, real["c"], W, 1)
        assert code == 0
        want = R.project(X, real["c"], W, 1)
        exact = (F - real["c"]) @ W
        ratio = (np.abs(Y - exact) / (2 * R.gamma(F.shape[1]) * R.project_envelope(X, real["c"], W, 1))).max()
        print(f"MEASURED lagged projection dim {dim}: {ratio:.3g} of the bar 2 gamma_D sum |f - mean| |W| (D = {F.shape[1]}); "
              f"bit-equal to the published tree: {np.array_equal(Y, want)}")
        assert ratio <= 1.0 and np.array_equal(Y, want)
        for t in (0, 150, 300):                                              # a frame alone has its row of the batch
            assert np.array_equal(_project(X[t:t + 1], real["c"], W, 1)[1][0], Y[t])
        assert np.array_equal(_project(X, real["c"], W, 1)[1], Y)


def test_limits_are_refused_and_nothing_is_written():
    X, c = np.ones((20, 5, 3)) * np.arange(5)[None, :, None], np.zeros(10)
    F = np.ones((20, 10))
    bad = [_moments(X, 0, c, 1), _moments(X, 20, c, 1), _moments(X, 25, c, 1), _moments(X, 2, c, 5), _moments(X, 2, c, -1),
           _moments(F, 2, c, 0, scratch_bytes=R.scratch_bytes(10, 1, True) - 8), _moments(F, 2, c, 0, null=("center",)),
           _moments(F, 2, c, 0, null=("scratch",)), _moments(F, 2, c, 0, null=("S0t",)),
           _moments(F, 2, c, 0, L_or_D=R.MAX_D + 1), _moments(X, 2, c, 1, L_or_D=R.MAX_L + 1)]
    for code, got in bad:
        assert code == E_INVALID and all(np.all(v == GARBAGE) for v in got.values())
    for code, m0, mt in (_means(X, 0, 1), _means(X, 20, 1), _means(F, 2, 0, scratch_bytes=R.scratch_bytes(10, 1, False) - 8),
                         _means(F, 2, 0, L_or_D=R.MAX_D + 1), _means(X, 2, 1, L_or_D=R.MAX_L + 1)):
        assert code == E_INVALID and np.all(m0 == GARBAGE) and np.all(mt == GARBAGE)
    for code, Y in (_project(F, c, np.ones((10, 17)), 0), _project(F, c, np.ones((10, 2)), 0, dim=0), _project(F, c, np.ones((10, 2)), 0, L_or_D=R.MAX_D + 1)):
        assert code == E_INVALID and np.all(Y == GARBAGE)
    code, got = _moments(np.ones((4, R.MAX_L, 3)) * np.arange(R.MAX_L)[None, :, None], 1, np.zeros(R.MAX_D), 127)      # the limits themselves pass
    assert code == 0 and abs(got["S00"][0, 0] - 3 * 3 * 127.0 ** 2) < 1e-6      # one pair, (0, 127), three times its squared distance


def test_non_finite_input_raises():
    from esmdiff_amd import kinetics
    X = R.trajectory(40, 6, seed=1)
    for bad in (np.nan, np.inf):
        Y = X.copy()
        Y[17, 2, 1] = bad
        with pytest.raises(ValueError, match="nan or inf"):
            kinetics.lagged_moments(Y, 3)
        with pytest.raises(ValueError, match="nan or inf"):
            kinetics.tica(X, 3).transform(Y)
    with pytest.raises(ValueError, match="more than lagtime"):
        kinetics.tica(X, 40)


# ---- model level ------------------------------------------------------------------------------------------------------------------
EPS = 1e-6


@pytest.fixture(scope="module", params=[(600, 12, 5), (300, 9, 3)], ids=lambda p: "x".join(map(str, p)))
def posed(request):
    """A generated trajectory, the oracle's fit of it, and the assertions that the input is well posed, on the oracle's own numbers."""
    from oracle import metrics_ref as O
    n, L, lag = request.param
    X = R.trajectory(n, L, seed=0)
    F = O.pairwise_distance_ca(X, 1)
    mean, comp, lam = O.tica_fit(F, lag, dim=4, epsilon=EPS)
    a, b = F[:-lag] - mean, F[lag:] - mean
    s = np.linalg.eigvalsh((a.T @ a + b.T @ b) / (2.0 * len(a)))
    al = np.abs(lam)
    assert al[0] - al[1] >= 0.05 and al[1] - al[2] >= 0.05, al
    assert not ((s > EPS / 1.5) & (s < EPS * 1.5)).any(), s[:3]
    return {"X": X, "F": F, "lag": lag, "mean": mean, "comp": comp, "lam": lam, "kept": int((s > EPS).sum())}


def test_tica_agrees_with_the_oracle(posed):
    from esmdiff_amd import kinetics
    X, lag = posed["X"], posed["lag"]
    model = kinetics.tica(X, lag, dim=2, epsilon=EPS)
    err = np.abs(model.eigenvalues - posed["lam"][:2]).max()
    want_ts = -lag / np.log(np.abs(posed["lam"][:2]))
    ts_bar = 1e-6 * lag / (np.abs(posed["lam"][:2]) * np.log(np.abs(posed["lam"][:2])) ** 2)      # 1e-6 in the eigenvalue, through -lag / ln
    ts_err = (np.abs(model.timescales - want_ts) / ts_bar).max()
    want = ((posed["F"] - posed["mean"]) @ posed["comp"][:, :2]) * posed["lam"][:2]
    got = model.transform(X)
    span = want.max(0) - want.min(0)
    sign = np.sign((got * want).sum(0))
    perr = (np.abs(got * sign - want) / span).max()
    print(f"MEASURED tica: |eigenvalue - oracle| {err:.3g}, timescales {ts_err:.3g} of that bar carried through -lag / ln, projection {perr:.3g} of its range (bar 1e-6)")
    assert model.n_kept == posed["kept"] and model.m == X.shape[0] - lag
    assert err <= 1e-6 and ts_err <= 1.0 and perr <= 1e-6
    assert np.array_equal(model.timescales, kinetics.timescales_from_eigenvalues(model.eigenvalues, lag))
    comp = model.components.cpu().numpy()
    assert (comp[np.abs(comp).argmax(0), np.arange(2)] > 0).all()             # the sign convention
    assert np.abs(model.mean.cpu().numpy() - posed["mean"]).max() <= 1e-12 * np.abs(posed["mean"]).max()
    ckv = model.cumulative_kinetic_variance
    assert np.all(np.diff(ckv) >= 0) and abs(ckv[-1] - 1.0) < 1e-12 and len(ckv) == model.n_kept
    its = kinetics.implied_timescales(X, [lag, 2 * lag], k=3)
    assert its.shape == (2, 3) and (np.abs(its[0, :2] - want_ts) <= ts_bar).all()


def test_js_tica_agrees_with_the_unfused_route_and_the_oracle(posed):
    from esmdiff_amd import kinetics, metrics
    from oracle import metrics_ref as O
    rng = np.random.default_rng(2)
    X, lag = posed["X"], posed["lag"]
    model_x = X[rng.integers(0, len(X), 150)] + 0.3 * rng.standard_normal((150,) + X.shape[1:])
    ens = {"target": X, "model": model_x}
    for weights in (None, {"model": rng.uniform(0.5, 1.5, 150), "target": rng.uniform(0.5, 1.5, len(X))}):
        got, tic = kinetics.js_tica(ens, lagtime=lag, weights=weights, rounded=False)
        old = metrics.js_tica(ens, lagtime=lag, weights=weights, rounded=False, return_tic=False)
        w = weights or {}
        ref = O.js_tica(model_x, X, lagtime=lag, w_model=w.get("model"), w_ref=w.get("target"))
        print(f"MEASURED js_tica: fused {got['model']:.9f}, unfused {old['model']:.9f}, oracle {ref:.9f}")
        assert got["target"] == 0.0 and abs(got["model"] - old["model"]) <= 1e-6 and abs(got["model"] - ref) <= 1e-6
        assert tic["model"].shape == (150, 2) and tic["target"].shape == (len(X), 2)
    plain = kinetics.js_tica(ens, lagtime=lag, rounded=False, return_tic=False)["model"]
    assert kinetics.js_tica(ens, lagtime=lag, return_tic=False)["model"] == float(np.around(plain, 4))


def test_vamp_form_agrees_with_numpy(posed):
    from esmdiff_amd import kinetics
    X, lag, F = posed["X"], posed["lag"], posed["F"]
    sv = R.koopman_singular_values(F, lag, EPS)
    model = kinetics.tica(X, lag, dim=3, epsilon=EPS, reversible=False)
    err = np.abs(model.eigenvalues - sv[:3]).max()
    score, want = kinetics.vamp2(X, lag, dim=3, epsilon=EPS), 1.0 + float((sv[:3] ** 2).sum())
    print(f"MEASURED vamp: |singular value - numpy| {err:.3g}, vamp2 {score:.9f} against {want:.9f}")
    assert err <= 1e-6 and abs(score - want) <= 1e-6 and abs(model.vamp2(3) - want) <= 1e-6
    assert abs(kinetics.vamp2(X, lag, epsilon=EPS) - (1.0 + float((sv ** 2).sum()))) <= 1e-6 * len(sv)


def test_a_list_of_trajectories_never_pairs_across_a_boundary():
    from esmdiff_amd import kinetics
    X, lag = R.trajectory(260, 7, seed=4), 6
    A, B = X[:100], X[100:]
    c = R.features(X, 1).mean(0)
    both = kinetics.lagged_moments([A, B], lag, center=c)
    a, b = kinetics.lagged_moments(A, lag, center=c), kinetics.lagged_moments(B, lag, center=c)
    whole = kinetics.lagged_moments(X, lag, center=c)
    assert both.m == a.m + b.m == 260 - 2 * lag and whole.m == 260 - lag
    for k in NAMES:
        assert bool((getattr(both, k) == getattr(a, k) + getattr(b, k)).all()), k
    assert not bool((both.S0t == whole.S0t).all())
    too_short = kinetics.lagged_moments([A, B, X[:lag]], lag, center=c)       # a trajectory without a pair adds nothing
    assert too_short.m == both.m and bool((too_short.S00 == both.S00).all())


def test_a_memmap_in_chunks_gives_the_same_model(tmp_path):
    from esmdiff_amd import kinetics
    n, L, lag = 700, 8, 4
    X = R.trajectory(n, L, seed=6)
    np.save(tmp_path / "traj.npy", X)
    mm = np.load(tmp_path / "traj.npy", mmap_mode="r")
    whole, parts = kinetics.lagged_moments(X, lag), kinetics.lagged_moments(mm, lag, chunk_frames=256)
    assert whole.m == parts.m == n - lag
    c = whole.center.cpu().numpy()
    env = R.moments_envelope(X, lag, c, 1)
    assert np.abs(parts.center.cpu().numpy() - c).max() <= 4 * R.gamma(n) * np.abs(R.features(X, 1)).mean(0).max()
    # the two centres differ by roundings, so the raw sums are compared after the correction to the estimator's mean: the covariances
    for got, want, e in zip(parts.covariances(), whole.covariances(), (env["S00"] + env["Stt"], env["S0t"] + env["S0t"].T)):
        bar = 4 * R.gamma(n) * e / (2.0 * (n - lag)) + 1e-13 * np.abs(want.cpu().numpy())
        assert (np.abs((got - want).cpu().numpy()) <= bar).all()
    m1, m2 = kinetics.fit(whole, 2), kinetics.fit(parts, 2)
    assert np.abs(m1.eigenvalues - m2.eigenvalues).max() <= 1e-9


def test_the_command_lines_block(tmp_path):
    import json
    from esmdiff_amd import analyze_ensemble, kinetics
    n, L, lag = 600, 12, 5
    X = R.trajectory(n, L, seed=0)
    np.save(tmp_path / "ref.npy", X)
    rng = np.random.default_rng(3)
    samples = X[rng.integers(0, n, 40)] + 0.2 * rng.standard_normal((40, L, 3))
    block = kinetics.report(np.load(tmp_path / "ref.npy", mmap_mode="r"), samples, X[[0, 300]], lagtime=lag, dim=2, lagtimes=[3, lag], chunk_frames=256)
    model = kinetics.tica(X, lag)
    assert np.abs(block["eigenvalues"] - model.eigenvalues).max() <= 1e-9 and block["n_kept"] == model.n_kept and block["pairs"] == n - lag
    assert np.array_equal(block["timescales"], kinetics.timescales_from_eigenvalues(block["eigenvalues"], lag))
    assert block["samples_tic"].shape == (40, 2) and block["targets_tic"].shape == (2, 2) and block["js_tic"].shape == (2,)
    assert np.abs(block["targets_tic"] - model.transform(X[[0, 300]])).max() <= 1e-9 and 0.0 < block["js_tica"] == float(np.mean(block["js_tic"])) < 1.0
    assert abs(block["vamp2"] - kinetics.vamp2(X, lag, 2)) <= 1e-9 and block["vamp2"] > 1.0
    its = block["implied_timescales"]
    assert its["lagtimes"] == [3, lag] and its["timescales"].shape == (2, 3) and abs(its["timescales"][1, 0] - block["timescales"][0]) <= 1e-6 * block["timescales"][0]
    F = block["free_energy"]["F"]
    assert F.shape == (50, 50) and len(block["free_energy"]["edges"]) == 2 and np.isnan(F).any()
    assert abs(np.exp(-F[~np.isnan(F)]).sum() - 1.0) < 1e-12                  # -ln p of a distribution over the trajectory's frames
    text = json.dumps(analyze_ensemble._jsonable({"tica": block}))
    assert "NaN" not in text and "Infinity" not in text and json.loads(text)["tica"]["lagtime"] == lag

"""GPU tests of the covariance layer (esmdiff_flex_transforms of csrc/flex.hip and the two entries of csrc/aligned.hip through the C
ABI and esmdiff_amd/pairs.py, esmdiff_amd/covariance.py) against the numpy restatement tests/aligned_ref.py.  Every output and the
scratch start as garbage.
THE BARS.  Integer operands (coordinates in [-512, 512], transforms from the 24 proper signed permutations with integer translations in
[-64, 64], an integer centre): S, r and count EQUAL the int64 restatement, S == S^T, every magnitude below 2^53.  Real operands: the
features are the restatement's bits, so r is bit-equal to the published order, and |S_dev - S_ref| <= 2 gamma_m |a|^T |a| elementwise
(any order of summation, with or without FMA inside the matrix unit); the coordinates lie 40 A from the origin, so a wrong centre or
a fused multiply-add in the transform would show.  The projection: bit-equal to the restatement's order.  Two calls are bit-identical,
whatever the number of scratch slots.  esmdiff_flex_transforms: rmsd bit-equal to esmdiff_flex_fit's, rot proper and orthonormal to
1e-12, rot a + tr within 1e-9 of esmdiff_flex_fit's moved structure.  Model level, after asserting that the input is well posed (the
gaps of the three leading eigenvalues at least 5 % of the first): covariance, modes, rmsf, dccm, rmwd and pca_w2 within 1e-9 of the
restatement on numpy-aligned frames (two Kabsch fits by different decompositions agree to 1e-12 A; the eigenvectors divide that by
gaps of order one).
Shapes, D = 3 L: L of 1, 5, 6, 21, 22, 43 (D of 3, 15, 18, 63, 66, 129) around the 16-wide MFMA block and the 64-wide tile (129: three
tiles, an off-diagonal pair two apart); frames of 1, 3, 4, 5 around the four of an instruction, 31 and 33 around the staged block, and
FRAME_CHUNK - 1, FRAME_CHUNK + 1, 2 FRAME_CHUNK + 3 around the chunk.  The caller's-stream contract is held in
tests/test_gpu_stream_transforms_aligned.py."""
import ctypes

import numpy as np
import pytest

from tests import aligned_ref as R
from tests import flex_ref as F

pytestmark = pytest.mark.gpu

FC = R.FRAME_CHUNK
E_INVALID, E_CAPACITY = -1, -5
GARBAGE = -7.25


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _dev(x, dtype=np.float64):
    import torch
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x, dtype=dtype)).cuda()


def _moments(X, T, use, c, slots=1, scratch_bytes=None, null=(), **over):
    """esmdiff_aligned_moments on numpy inputs -> (code, {S, r, count}); outputs and scratch start as garbage."""
    import torch
    from esmdiff_amd import _native as N
    n, L = X.shape[:2]
    D = 3 * L
    x, t, u, cd = _dev(X), _dev(T), _dev(use, np.uint8), _dev(c)
    out = {"S": torch.full((D, D), GARBAGE, dtype=torch.float64, device="cuda"), "r": torch.full((D,), GARBAGE, dtype=torch.float64, device="cuda"),
           "count": torch.full((1,), -77, dtype=torch.int64, device="cuda")}
    size = R.scratch_bytes(L, slots) if scratch_bytes is None else scratch_bytes
    scratch = torch.full((max(size, 8) // 8 + 1,), GARBAGE, dtype=torch.float64, device="cuda")
    arg = lambda k, v: None if k in null else v
    code = N.lib().esmdiff_aligned_moments(_p(arg("X", x)), over.get("n", n), over.get("L", L), _p(t), _p(u), _p(arg("center", cd)),
                                           _p(arg("S", out["S"])), _p(arg("r", out["r"])), _p(arg("count", out["count"])),
                                           _p(arg("scratch", scratch)), size, None)
    torch.cuda.synchronize()
    return code, {k: v.cpu().numpy() for k, v in out.items()}


def _untouched(got):
    return np.all(got["S"] == GARBAGE) and np.all(got["r"] == GARBAGE) and got["count"][0] == -77


def _project(X, T, mean, W, dim=None, **over):
    import torch
    from esmdiff_amd import _native as N
    n, L = X.shape[:2]
    x, t, md, wd = _dev(X), _dev(T), _dev(mean), _dev(W)
    dim = W.shape[1] if dim is None else dim
    Y = torch.full((n, max(W.shape[1], 1)), GARBAGE, dtype=torch.float64, device="cuda")
    code = N.lib().esmdiff_aligned_project(_p(x), n, over.get("L", L), _p(t), _p(md), _p(wd), dim, _p(Y), None)
    torch.cuda.synchronize()
    return code, Y.cpu().numpy()


def _integers(rng, n, L):
    """Integer coordinates in [-512, 512], transforms from the signed permutations with translations in [-64, 64], a centre in [-8, 8]."""
    X = rng.integers(-512, 513, size=(n, L, 3)).astype(np.float64)
    P = R.signed_permutations()
    T = np.concatenate([P[rng.integers(0, 24, n)].reshape(n, 9), rng.integers(-64, 65, size=(n, 3))], axis=1).astype(np.float64)
    return X, T, rng.integers(-8, 9, size=3 * L).astype(np.float64)


def _exact(X, T, use, c, slots=1):
    code, got = _moments(X, T, use, c, slots)
    assert code == 0
    on = np.ones(len(X), bool) if use is None else use.astype(bool)
    want = R.moments_int(np.where(on[:, None, None], X, 0.0), None if T is None else np.where(on[:, None], T, 0.0), use, c)
    tag = f"n = {X.shape[0]}, L = {X.shape[1]}, T {'given' if T is not None else 'null'}"
    assert max(int(np.abs(want[k]).max()) for k in ("S", "r")) < 2 ** 53, tag
    assert np.array_equal(got["S"], want["S"].astype(np.float64)), f"{tag}: S"
    assert np.array_equal(got["r"], want["r"].astype(np.float64)), f"{tag}: r"
    assert got["count"][0] == want["count"] and np.array_equal(got["S"], got["S"].T), tag
    return got


@pytest.mark.parametrize("L", [1, 5, 6, 21, 22, 43])
def test_integer_moments_equal_int64_around_the_tile_the_instruction_and_the_block(L):
    rng = np.random.default_rng(100 + L)
    for n in (1, 3, 4, 5, 31, 33):
        X, T, c = _integers(rng, n, L)
        got = _exact(X, T, None, c)
        _exact(X, None, None, c)
        if n > 1:
            assert np.abs(got["S"]).max() > 0 and got["count"][0] == n


@pytest.mark.parametrize("n", [FC - 1, FC + 1, 2 * FC + 3])
def test_integer_moments_equal_int64_around_the_frame_chunk(n):
    rng = np.random.default_rng(n)
    X, T, c = _integers(rng, n, 6)
    one = _exact(X, T, None, c, slots=1)
    many = _exact(X, T, None, c, slots=5)                                    # more slots than chunks: the same rounds' sums
    assert all(np.array_equal(one[k], many[k]) for k in one)
    _exact(X, None, None, c, slots=2)


@pytest.mark.parametrize("case", ["first", "last", "block", "all"])
def test_unused_frames_reach_no_sum(case):
    rng = np.random.default_rng(7)
    n, L = FC + 40, 6
    X, T, c = _integers(rng, n, L)
    use = np.ones(n, np.uint8)
    use[{"first": slice(0, 1), "last": slice(n - 1, n), "block": slice(32, 64), "all": slice(0, n)}[case]] = 0
    X[use == 0], T[use == 0] = np.nan, np.nan                                # what is not used is never read
    got = _exact(X, T, use, c)
    assert got["count"][0] == int(use.sum()) and np.isfinite(got["S"]).all() and np.isfinite(got["r"]).all()
    if case == "all":
        assert got["count"][0] == 0 and np.all(got["S"] == 0.0) and np.all(got["r"] == 0.0)
    _exact(X, None, use, c)


@pytest.fixture(scope="module")
def real():
    """Real operands and their restated moments, shared and never written: a chain 40 A from the origin with 0.5 A of noise, every frame
    moved by its own rigid motion, and the transforms that move it back.  The features then lie within a few A of a centre that is tens of
    A from the origin: a - c cancels most of f, and a wrong centre or a fused multiply-add in f shows at full size."""
    rng = np.random.default_rng(11)
    n, L = 2 * FC + 77, 22
    frames = np.cumsum(rng.standard_normal((1, L, 3)) * 2.2, axis=1) + 40.0 + rng.standard_normal((n, L, 3)) * 0.5
    rot = np.stack([F.E.random_rotation(rng) for _ in range(n)])
    shift = rng.standard_normal((n, 1, 3)) * 20.0
    X = np.einsum("ncd,nld->nlc", rot, frames) + shift
    back = rot.transpose(0, 2, 1)
    T = np.concatenate([back.reshape(n, 9), -np.einsum("ncd,nd->nc", back, shift[:, 0])], axis=1)
    use = (rng.random(n) < 0.9).astype(np.uint8)
    feat = R.features(X, T)
    c = feat[use.astype(bool)].mean(0) + 0.05 * rng.standard_normal(3 * L)
    return {"X": X, "T": T, "use": use, "c": c, "F": feat, "ref": R.moments(X, T, use, c), "env": R.moments_envelope(X, T, use, c)}


def test_real_moments_within_the_rounding_bound_and_r_in_the_published_order(real):
    code, got = _moments(real["X"], real["T"], real["use"], real["c"], slots=2)
    assert code == 0 and got["count"][0] == real["ref"]["count"] == int(real["use"].sum())
    m = real["ref"]["count"]
    err, bound = np.abs(got["S"] - real["ref"]["S"]), 2 * R.gamma(m) * real["env"]["S"]
    print(f"MEASURED aligned moments: max |S_dev - S_ref| / bound = {(err / bound).max():.3g}, m = {m}")
    assert (err <= bound).all() and np.array_equal(got["S"], got["S"].T)
    assert np.array_equal(got["r"], real["ref"]["r"])
    assert np.abs(real["c"]).min() > 20.0 and np.abs(real["F"] - real["c"]).max() < 4.0        # the centre far from the origin, the features near it
    assert np.sqrt((real["X"] ** 2).sum(-1)).mean() > 40.0                                     # and the coordinates far from it too
    # T = NULL on the same coordinates: the raw coordinate is the feature
    c0 = real["X"].reshape(len(real["X"]), -1).mean(0)
    code, raw = _moments(real["X"], None, None, c0)
    want, env = R.moments(real["X"], None, None, c0), R.moments_envelope(real["X"], None, None, c0)
    assert code == 0 and np.array_equal(raw["r"], want["r"]) and (np.abs(raw["S"] - want["S"]) <= 2 * R.gamma(len(real["X"])) * env["S"]).all()


def test_the_slot_count_changes_no_bit_and_two_calls_agree(real):
    runs = [_moments(real["X"], real["T"], real["use"], real["c"], slots=s) for s in (1, 5, 5)]
    assert all(code == 0 for code, _ in runs)
    for k in ("S", "r", "count"):
        assert np.array_equal(runs[0][1][k], runs[1][1][k]) and np.array_equal(runs[1][1][k], runs[2][1][k]), k


def _transforms(A, ma, ref, mref, null=()):
    import torch
    from esmdiff_amd import _native as N
    n, L = A.shape[:2]
    a, m, r, mr = _dev(A), _dev(ma, np.uint8), _dev(ref), _dev(mref, np.uint8)
    T = torch.full((n, 12), GARBAGE, dtype=torch.float64, device="cuda")
    rmsd = torch.full((n,), GARBAGE, dtype=torch.float64, device="cuda")
    ok = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    code = N.lib().esmdiff_flex_transforms(_p(a), n, L, _p(m), _p(r), _p(mr), _p(None if "T" in null else T), _p(None if "rmsd" in null else rmsd),
                                           _p(None if "ok" in null else ok), None)
    torch.cuda.synchronize()
    return code, T.cpu().numpy(), rmsd.cpu().numpy(), ok.cpu().numpy()


@pytest.mark.parametrize("L", [2, 7, 65])
@pytest.mark.parametrize("masked", [False, True])
def test_transforms_are_flex_fit_s_fit(L, masked):
    from esmdiff_amd import pairs
    rng = np.random.default_rng(L + 1000 * masked)
    n = 9
    A = F.rigid_moves(rng, np.cumsum(rng.standard_normal((n, L, 3)) * 2.2, axis=1))
    ref = A[0] + rng.standard_normal((L, 3)) * 0.3
    ma = mref = None
    if masked:
        ma, mref = (rng.random((n, L)) < 0.7).astype(np.uint8), (rng.random(L) < 0.8).astype(np.uint8)
        ma[:, :2], mref[:2] = 1, 1                                            # two common residues everywhere
    code, T, rmsd, ok = _transforms(A, ma, ref, mref)
    assert code == 0 and np.all(ok == 1)
    aligned, rmsd_fit = pairs.fit(_dev(A), _dev(ma, np.uint8), _dev(ref), _dev(mref, np.uint8))
    assert np.array_equal(rmsd, rmsd_fit.cpu().numpy())                       # the same statements: the same bits
    rot, tr = T[:, :9].reshape(n, 3, 3), T[:, 9:]
    assert (np.linalg.det(rot) > 0).all() and np.abs(rot @ rot.transpose(0, 2, 1) - np.eye(3)).max() < 1e-12
    assert np.abs(np.einsum("ncd,nld->nlc", rot, A) + tr[:, None] - aligned.cpu().numpy()).max() < 1e-9
    assert np.abs(R.features(A, T).reshape(n, L, 3) - aligned.cpu().numpy()).max() < 1e-9
    want_T, want_rmsd, good = R.transforms(A, np.ones((n, L), bool) if ma is None else ma.astype(bool), ref,
                                           np.ones(L, bool) if mref is None else mref.astype(bool))
    assert good.all() and np.abs(rmsd - want_rmsd).max() < 1e-9
    code, T2, rmsd2, _ = _transforms(A, ma, ref, mref, null=("rmsd",))
    assert code == 0 and np.array_equal(T2, T) and np.all(rmsd2 == GARBAGE)


def test_a_frame_with_one_common_residue_fails_alone():
    rng = np.random.default_rng(5)
    n, L = 6, 7
    A = F.rigid_moves(rng, np.cumsum(rng.standard_normal((n, L, 3)) * 2.2, axis=1))
    ma = np.ones((n, L), np.uint8)
    code, T, rmsd, ok = _transforms(A, ma, A[0], None)
    ma[3] = 0
    ma[3, 4] = 1
    A3 = A.copy()
    A3[3, :4] = np.nan                                                        # masked: never read into a sum
    code2, T2, rmsd2, ok2 = _transforms(A3, ma, A[0], None)
    assert code == 0 and code2 == 0 and np.all(ok == 1) and list(ok2) == [1, 1, 1, 0, 1, 1]
    assert np.isnan(T2[3]).all() and np.isnan(rmsd2[3])
    others = np.arange(n) != 3
    assert np.array_equal(T2[others], T[others]) and np.array_equal(rmsd2[others], rmsd[others])
    for null in (("T",), ("ok",)):
        code, Tn, rn, okn = _transforms(A, ma, A[0], None, null=null)
        assert code == E_INVALID and np.all(Tn == GARBAGE) and np.all(rn == GARBAGE) and np.all(okn == 9)
    code, Tn, _, okn = _transforms(A[:, :1], None, A[0, :1], None)            # L = 1: esmdiff_flex_fit's check
    assert code == E_INVALID and np.all(Tn == GARBAGE) and np.all(okn == 9)


@pytest.mark.parametrize("L", [1, 21, 22, 43])
@pytest.mark.parametrize("dim", [1, 16])
def test_projection_is_bit_equal_to_the_published_order(L, dim):
    rng = np.random.default_rng(L * 100 + dim)
    n = 70
    X = np.cumsum(rng.standard_normal((n, L, 3)) * 2.2, axis=1) + 40.0
    T = np.concatenate([np.stack([F.E.random_rotation(rng) for _ in range(n)]).reshape(n, 9), rng.standard_normal((n, 3)) * 20.0], axis=1)
    mean, W = R.features(X, T).mean(0), rng.standard_normal((3 * L, dim))
    code, Y = _project(X, T, mean, W)
    assert code == 0 and np.array_equal(Y, R.project(X, T, mean, W))
    code, alone = _project(X[37:38], T[37:38], mean, W)                       # a frame's row does not depend on the batch
    assert code == 0 and np.array_equal(alone[0], Y[37])
    code, raw = _project(X, None, mean, W)
    assert code == 0 and np.array_equal(raw, R.project(X, None, mean, W))


def test_refusals_touch_nothing():
    rng = np.random.default_rng(3)
    X, T, c = _integers(rng, 10, 4)
    for dim in (0, 17):
        code, Y = _project(X, T, c, np.zeros((12, 16)), dim=dim)
        assert code == E_INVALID and np.all(Y == GARBAGE)
    code, Y = _project(X, T, c, np.zeros((12, 2)), L=1281)
    assert code == E_CAPACITY and np.all(Y == GARBAGE)
    code, got = _moments(X, T, None, c, L=1281, scratch_bytes=R.scratch_bytes(4, 1))
    assert code == E_CAPACITY and _untouched(got)
    for null in ("S", "X", "center", "r", "count", "scratch"):
        code, got = _moments(X, T, None, c, null=(null,))
        assert code == E_INVALID and _untouched(got), null
    code, got = _moments(X, T, None, c, scratch_bytes=R.scratch_bytes(4, 1) - 1)
    assert code == E_INVALID and _untouched(got)
    for over in ({"n": 0}, {"L": 0}):
        code, got = _moments(X, T, None, c, **over)
        assert code == E_INVALID and _untouched(got), over


# ---- model level ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    """Two planted ensembles on one base chain (n = 300 and 200, L = 12; the second with ten times the noise), their numpy-aligned
    frames on the first one's frame 0, and the device's moments."""
    from esmdiff_amd import covariance
    A = F.planted(np.random.default_rng(7), 300, 12)
    B = F.planted(np.random.default_rng(7), 200, 12, noise=0.5)               # the same base and fields: the generator draws them first
    ref = A[0].copy()
    on = lambda X: np.ones(X.shape[:2], bool)
    Aa, Ba = F.fit(A, on(A), ref, np.ones(12, bool))[0], F.fit(B, on(B), ref, np.ones(12, bool))[0]
    return {"A": A, "B": B, "ref": ref, "Aa": Aa, "Ba": Ba, "mA": covariance.aligned_moments(A, ref, keep_transforms=True),
            "mB": covariance.aligned_moments(B, ref)}


def _check_model(mA, mB, Aa, Ba):
    from esmdiff_amd import covariance
    assert mA.count == len(Aa) and mA.n_dropped == 0 and mB.count == len(Ba)
    assert np.abs(mA.mean - Aa.mean(0)).max() < 1e-9 and np.abs(mA.covariance() - R.covariance(Aa)).max() < 1e-9
    lam, V = R.modes(Aa, 3)
    got_lam, got_V = mA.modes(3)
    assert np.abs(got_lam - lam).max() < 1e-9 and np.abs(got_V.reshape(3, -1) - V).max() < 1e-9
    assert np.abs(mA.rmsf() - R.rmsf(Aa)).max() < 1e-9 and np.abs(mA.dccm() - R.dccm(Aa)).max() < 1e-9
    assert np.abs(np.array(list(covariance.rmwd(mA, mB).values())) - np.array(R.rmwd(Aa, Ba))).max() < 1e-9
    assert abs(covariance.pca_w2(mA, mB, 2) - R.pca_w2(Aa, Ba, 2)) < 1e-9


def test_the_model_level_against_the_restatement_on_aligned_frames(model):
    from esmdiff_amd import covariance, flexibility
    lam = R.modes(model["Aa"], 4)[0]
    # well posed: the gaps among the three leading eigenvalues are at least 5 % of the first.  The third mode also needs a gap below it:
    # two Kabsch fits differ by 1e-12 A, the covariances by 1e-11 or less, and a mode moves by that over its gap: 1 % of the first
    # eigenvalue (0.6 A^2 here) leaves 1e-11, two orders inside the 1e-9 bar
    assert lam[0] - lam[1] >= 0.05 * lam[0] and lam[1] - lam[2] >= 0.05 * lam[0] and lam[2] - lam[3] >= 0.01 * lam[0], lam
    lamB = R.modes(model["Ba"], 3)[0]
    assert lam[0] - lam[1] >= 0.05 * lam[0] and lamB[0] - lamB[1] >= 0.05 * lamB[0]
    _check_model(model["mA"], model["mB"], model["Aa"], model["Ba"])
    mA = model["mA"]
    assert np.abs(mA.rmsd - F.fit(model["A"], np.ones((300, 12), bool), model["ref"], np.ones(12, bool))[1]).max() < 1e-9
    assert mA.transforms.shape == (300, 12) and np.abs(R.features(model["A"], mA.transforms).reshape(300, 12, 3) - model["Aa"]).max() < 1e-9
    assert np.abs(mA.rmsf() - flexibility.rmsf(model["A"], start=0, max_iter=1, tol=0.0)).max() < 1e-9
    lam3, V = R.modes(model["Aa"], 3)
    want = (model["Ba"] - model["Aa"].mean(0)).reshape(200, -1) @ V.T
    assert np.abs(mA.project(model["B"], 3) - want).max() < 1e-9
    assert abs(covariance.joint_pca_w2(mA, model["mB"], 2) - covariance.joint_pca_w2(model["mB"], mA, 2)) < 1e-9
    with pytest.raises(ValueError, match="same reference"):
        covariance.rmwd(mA, covariance.aligned_moments(model["B"], model["B"][0]))


def test_rigid_moves_change_nothing_beyond_the_bar(model):
    from esmdiff_amd import covariance
    rng = np.random.default_rng(8)
    mA = covariance.aligned_moments(F.rigid_moves(rng, model["A"]), model["ref"])
    mB = covariance.aligned_moments(F.rigid_moves(rng, model["B"]), model["ref"])
    _check_model(mA, mB, model["Aa"], model["Ba"])


def test_a_list_and_a_memmap_give_the_moments_of_the_concatenation(model, tmp_path):
    from esmdiff_amd import covariance
    A, ref, whole = model["A"], model["ref"], model["mA"]
    a = np.abs(model["Aa"].reshape(300, -1) - ref.reshape(-1))
    bound_S, bound_r = 2 * R.gamma(300) * (a.T @ a), 2 * R.gamma(300) * a.sum(0)    # each side is within gamma_m of the exact sums
    np.save(tmp_path / "traj.npy", A)
    for other in (covariance.aligned_moments([A[:130], A[130:]], ref),
                  covariance.aligned_moments(np.load(tmp_path / "traj.npy", mmap_mode="r"), ref, chunk_frames=64)):
        assert other.count == 300 and other.n_dropped == 0 and np.array_equal(other.rmsd, whole.rmsd)
        assert (np.abs((other.S - whole.S).cpu().numpy()) <= bound_S).all() and (np.abs((other.r - whole.r).cpu().numpy()) <= bound_r).all()


def test_dropped_frames_and_the_residue_set(model):
    from esmdiff_amd import covariance
    A, ref = model["A"].copy(), model["ref"].copy()
    ref[5] = np.nan                                                           # the set: the 11 residues valid in ref
    A[10, 3] = np.nan                                                         # a residue of the set unresolved: the frame is dropped
    A[20, 5] = np.nan                                                         # not in the set: the frame stays
    m = covariance.aligned_moments(A, ref)
    keep = np.delete(np.arange(12), 5)
    assert np.array_equal(m.residues, keep) and m.count == 299 and m.n_dropped == 1 and m.S.shape == (33, 33)
    rest = np.delete(A, 10, axis=0)[:, keep]
    Xa = F.fit(rest, np.ones(rest.shape[:2], bool), ref[keep], np.ones(11, bool))[0]
    assert np.abs(m.covariance() - R.covariance(Xa)).max() < 1e-9 and np.abs(m.mean - Xa.mean(0)).max() < 1e-9
    assert np.isfinite(m.rmsd).all() and np.isnan(m.project(A, 2)[10]).all() and np.isfinite(m.project(A, 2)[20]).all()

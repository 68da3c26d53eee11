"""GPU tests of the superposition layer (esmdiff_amd/csrc/superpose.hip through esmdiff_amd/ensemble.py and the C ABI): the Kabsch
side against the reference's own outputs (tests/golden/g13_superposition.npz), both kernels against their float64 restatement
(tests/ensemble_ref.py, itself held to g13 by tests/test_ensemble_cpu.py), determinism, and the reference's call shapes.
No network engine is built anywhere in this file.  [TMSCORE-RECALL]: the TM search is compared with its restatement, not with the
TMscore program (parity unpinned)."""
import json

import numpy as np
import pytest

from tests import ensemble_ref as E

pytestmark = pytest.mark.gpu

PLAIN, MIRROR, MASKED, PLANAR, TWO = range(5)
ZERO_RMSD = 1e-11          # a noise-free copy aligns to rounding only (tests/test_ensemble_cpu.py states the reasoning)


@pytest.fixture(scope="module")
def ens():
    from esmdiff_amd import ensemble
    return ensemble


@pytest.fixture(scope="module")
def g13(golden_dir):
    return np.load(golden_dir / "g13_superposition.npz")


def _orthogonal(R, det=None):
    np.testing.assert_allclose(R @ np.swapaxes(R, -1, -2), np.broadcast_to(np.eye(3), R.shape), atol=1e-12)
    if det is not None:
        np.testing.assert_allclose(np.linalg.det(R), det, atol=1e-12)


# ---- 1. against g13 -------------------------------------------------------------------------------------------------------
def test_squared_deviation_and_pairwise_rmsd_against_g13(ens, g13):
    for c, kind in enumerate(g13["kind"]):
        src, tgt = g13[f"src_{c}"], g13[f"tgt_{c}"]
        noise_free = g13["noise"][c] == 0
        want_proper = np.sqrt(np.nanmean(g13[f"scipy_dist_{c}"] ** 2))
        if kind != MASKED:       # the reference's call shape (it cannot take NaN): numpy in, numpy out
            sd = ens.squared_deviation(src[None], tgt[None])
            rmsd = ens.squared_deviation(src[None], tgt[None], reduction="rmsd")
            assert isinstance(sd, np.ndarray) and sd.shape == (1, len(src)) and rmsd.shape == (1,)
            np.testing.assert_allclose(sd[0], g13[f"sd_{c}"], rtol=0, atol=1e-9, err_msg=str(c))
            if noise_free:
                assert rmsd[0] < ZERO_RMSD and g13[f"rmsd_{c}"] < ZERO_RMSD
            else:
                np.testing.assert_allclose(rmsd[0], g13[f"rmsd_{c}"], rtol=1e-9, err_msg=str(c))
        # all-pairs entry, both rules; NaN coordinates are the mask
        for reflection, want in ((True, float(g13[f"rmsd_{c}"])), (False, want_proper)):
            if kind == MASKED and not reflection:
                continue             # scipy's number there is get_structures' own-mask centring: aligned_deviation below
            got = ens.pairwise_rmsd(src, tgt, reflection=reflection)
            assert got.shape == (1, 1)
            if noise_free and (reflection or kind != MIRROR):
                assert got[0, 0] < ZERO_RMSD, (c, reflection, got)
            else:
                np.testing.assert_allclose(got[0, 0], want, rtol=1e-9, err_msg=f"{c} {reflection}")
            R, t = ens.superposition(src, tgt, reflection=reflection)
            _orthogonal(R[0, 0], det=None if reflection else 1.0)
            if kind in (PLAIN, MIRROR) or (kind == MASKED and reflection):      # R is unique only off the degenerate cases
                np.testing.assert_allclose(R[0, 0], g13[f"R_{c}"] if reflection else g13[f"scipy_rot_{c}"].T, atol=1e-9, err_msg=str(c))
                if reflection:
                    np.testing.assert_allclose(t[0, 0], g13[f"t_{c}"], atol=1e-7, err_msg=str(c))
        # the distances apo_analysis takes after get_structures, the masked pair (different residues missing) included
        dev = ens.aligned_deviation(src, tgt)
        np.testing.assert_allclose(dev[0, 0] ** 2, g13[f"scipy_dist_{c}"] ** 2, rtol=0, atol=1e-9, equal_nan=True, err_msg=str(c))
    # the mirror image separates the two rules
    c = int(np.flatnonzero(g13["kind"] == MIRROR)[0])
    src, tgt = g13[f"src_{c}"], g13[f"tgt_{c}"]
    assert ens.pairwise_rmsd(src, tgt, reflection=True)[0, 0] < ZERO_RMSD
    assert ens.pairwise_rmsd(src, tgt, reflection=False)[0, 0] > 1.0
    assert np.linalg.det(ens.superposition(src, tgt, reflection=True)[0][0, 0]) < 0


# ---- 2. shapes that cross the kernel's boundaries -------------------------------------------------------------------------
def _masks(rng, n, L):
    m = rng.random((n, L)) > 0.2
    m[:, :2] = True                 # at least two valid residues everywhere ...
    m[0] = False
    m[0, L - 1] = True              # ... except row 0: one valid residue, every pair with it must be NaN
    return m


@pytest.mark.parametrize("L", [2, 3, 5, 63, 64, 65, 130])
def test_superpose_shapes_against_the_restatement(ens, L):
    from esmdiff_amd import _native as N
    import ctypes
    import torch
    rng = np.random.default_rng(1000 + L)
    for n, m in ((1, 1), (2, 3), (7, None)):
        A = E.ensemble(rng, n, L)
        B = None if m is None else E.ensemble(rng, m, L)
        for masked in (False, True):
            ma = _masks(rng, n, L) if masked else None
            mb = None if (B is None or not masked) else _masks(rng, m, L)[::-1].copy()     # its one-residue row is the last
            for reflection in (False, True):
                want_rmsd, want_sd, want_R, want_t = E.superpose_pairs(A, B, ma, mb, reflection)
                # one launch with every output, through the C ABI
                Ad, Bd = torch.as_tensor(A).cuda(), None if B is None else torch.as_tensor(B).cuda()
                mad = None if ma is None else torch.as_tensor(ma).to(torch.uint8).cuda()
                mbd = None if mb is None else torch.as_tensor(mb).to(torch.uint8).cuda()
                mm = n if m is None else m
                out = {k: torch.full(s, 7.0, dtype=torch.float64, device="cuda")
                       for k, s in (("rmsd", (n, mm)), ("sd", (n, mm, L)), ("R", (n, mm, 3, 3)), ("t", (n, mm, 3)))}
                p = lambda x: ctypes.c_void_p(0 if x is None else x.data_ptr())    # noqa: E731
                code = N.lib().esmdiff_superpose_pairs(p(Ad), n, p(Bd), mm, L, p(mad), p(mbd), int(reflection), p(out["rmsd"]),
                                                       p(out["sd"]), p(out["R"]), p(out["t"]), None)
                assert code == 0
                rmsd, sd, R, t = (out[k].cpu().numpy() for k in ("rmsd", "sd", "R", "t"))
                tag = f"L={L} n={n} m={m} masked={masked} reflection={reflection}"
                assert np.array_equal(np.isnan(rmsd), np.isnan(want_rmsd)), tag
                assert np.array_equal(np.isnan(sd), np.isnan(want_sd)), tag
                if masked:
                    assert np.isnan(rmsd[0]).all() and np.isnan(R[0]).all() and np.isnan(t[0]).all() and np.isnan(sd[0]).all(), tag
                np.testing.assert_allclose(rmsd, want_rmsd, rtol=1e-9, atol=ZERO_RMSD, equal_nan=True, err_msg=tag)
                np.testing.assert_allclose(sd, want_sd, rtol=0, atol=1e-9, equal_nan=True, err_msg=tag)
                ok = ~np.isnan(rmsd)
                _orthogonal(R[ok], det=None if reflection else 1.0)
                if L >= 63:                                   # enough residues everywhere for a unique rotation
                    np.testing.assert_allclose(R[ok], want_R[ok], atol=1e-9, err_msg=tag)
                    np.testing.assert_allclose(t[ok], want_t[ok], atol=1e-7, err_msg=tag)
                # the Python entry gives the same bits as the raw launch
                assert np.array_equal(ens.pairwise_rmsd(A, B, ma, mb, reflection=reflection), rmsd, equal_nan=True), tag


def test_long_pair_and_the_length_limit(ens):
    """L = 1026 (BASELINE configs[3]) through both kernels; beyond the TM kernel's LDS limit the error comes back as RuntimeError."""
    from esmdiff_amd import _native as N
    rng = np.random.default_rng(1026)
    A = E.ensemble(rng, 2, 1026, noise=2.0)
    want = E.superpose_pair(A[0], A[1], allow_reflection=False)
    got = ens.pairwise_rmsd(A[:1], A[1:])
    np.testing.assert_allclose(got[0, 0], want[0], rtol=1e-9)
    np.testing.assert_allclose(ens.aligned_deviation(A[:1], A[1:])[0, 0] ** 2, want[1], rtol=0, atol=1e-9)
    tm, R, t = ens.tm_matrix(A[:1], A[1:], return_transform=True)
    assert tm[0, 0] >= E.tm_at_kabsch(A[0], A[1]) - 1e-12 and tm[0, 0] <= 1.0
    np.testing.assert_allclose(E.tm_at(A[0], A[1], R[0, 0], t[0, 0]), tm[0, 0], rtol=0, atol=1e-9)   # the returned fit scores what it says
    moved = A[0] @ E.random_rotation(rng).T + 5.0
    assert abs(ens.tm_score(A[0], moved) - 1.0) < 1e-12
    # the limit itself works, one residue more is refused; the RMSD kernel reads global memory and has no limit
    big = E.ensemble(rng, 2, N.TM_MAX_L + 1, noise=2.0)
    with pytest.raises(RuntimeError, match="beyond the kernel's limit"):
        ens.tm_matrix(big)
    np.testing.assert_allclose(ens.pairwise_rmsd(big[:1], big[1:])[0, 0], E.superpose_pair(big[0], big[1])[0], rtol=1e-9)


# ---- 3. TM-score against the restatement ----------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [5, 16, 64, 65, 130])
def test_tm_matrix_against_the_restatement(ens, L):
    rng = np.random.default_rng(2000 + L)
    A = E.ensemble(rng, 6, L, noise=2.0)
    A[5] = A[0] @ E.random_rotation(rng).T + rng.normal(size=3) * 20          # a rigid copy of sample 0
    got = ens.tm_matrix(A)
    want = E.tm_matrix(A)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-9)
    assert abs(got[0, 5] - 1.0) < 1e-12 and abs(got[5, 0] - 1.0) < 1e-12 and np.abs(np.diag(got) - 1.0).max() < 1e-12
    for i in range(6):
        for j in range(6):
            assert got[i, j] >= E.tm_at_kabsch(A[i], A[j]) - 1e-12, (i, j)


def test_tm_masks_normalise_by_the_native(ens):
    rng = np.random.default_rng(2065)
    A, B = E.ensemble(rng, 2, 65, noise=2.0), E.ensemble(rng, 3, 65, noise=2.0)
    ma, mb = _masks(rng, 2, 65), _masks(rng, 3, 65)[::-1].copy()
    got = ens.tm_matrix(A, B, ma, mb)
    want = E.tm_matrix(A, B, ma, mb)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got[0]).all() and np.isnan(got[:, 2]).all()
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-9, equal_nan=True)
    # NaN coordinates are a mask too
    An = A.copy()
    An[~ma] = np.nan
    assert np.array_equal(ens.tm_matrix(An, B, None, mb), got, equal_nan=True)


def test_tm_finds_the_rigid_core(ens):
    """60 % of the residues moved rigidly and exactly, the rest thrown 30-50 A away: TM >= 0.6 needs the fragment search — the global
    Kabsch superposition (the search's first seed alone) stays far below."""
    a, b = E.core_case(np.random.default_rng(7))
    tm, R, t = ens.tm_matrix(a, b, return_transform=True)
    assert tm[0, 0] >= 0.6 - 1e-9
    assert E.tm_at_kabsch(a, b) < 0.5
    np.testing.assert_allclose(a[:60] @ R[0, 0].T + t[0, 0], b[:60], atol=1e-6)      # the returned fit is the core's
    np.testing.assert_allclose(tm[0, 0], E.tm_pair(a, b)[0], rtol=0, atol=1e-9)


# ---- 4. determinism and composition ---------------------------------------------------------------------------------------
def test_bit_identical_runs_and_launch_independence(ens):
    rng = np.random.default_rng(4)
    A = E.ensemble(rng, 4, 65, noise=2.0)
    ma = _masks(rng, 4, 65)
    ma[0] = True
    tm1, tm2 = ens.tm_matrix(A, mask_models=ma), ens.tm_matrix(A, mask_models=ma)
    assert np.array_equal(tm1, tm2)
    from esmdiff_amd import pairs
    args = pairs.pair_args(A, None, ma, None)
    out1 = pairs.superpose(*args, False, ("rmsd", "sd", "R", "t"))
    out2 = pairs.superpose(*args, False, ("rmsd", "sd", "R", "t"))
    for k in out1:
        assert np.array_equal(out1[k].cpu().numpy(), out2[k].cpu().numpy(), equal_nan=True), k
    tm, rmsd = ens.tm_matrix(A), ens.pairwise_rmsd(A)
    for i in range(4):
        for j in range(4):
            assert tm[i, j] == ens.tm_score(A[i], A[j]), (i, j)                     # bit for bit
            assert rmsd[i, j] == ens.pairwise_rmsd(A[i], A[j])[0, 0], (i, j)


# ---- 5. the reference's call shapes ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(5)
    S = E.ensemble(rng, 12, 40, noise=2.0)
    t1, t2 = ((S[k] + rng.normal(size=(40, 3))) @ E.random_rotation(rng).T + rng.normal(size=3) * 20 for k in (0, 1))
    return S, t1, t2


def test_tm_ensemble_functions(ens, small):
    S, t1, t2 = small
    tm_to = {k: np.array([E.tm_pair(s, t)[0] for s in S]) for k, t in (("t1", t1), ("t2", t2))}
    np.testing.assert_allclose(ens.tm_ensemble(S, t1, t2), 0.5 * tm_to["t1"].max() + 0.5 * tm_to["t2"].max(), rtol=0, atol=1e-9)
    best_tm, best_rmsd = ens.tm_n_ensemble(S, np.stack([t1, t2]))
    assert isinstance(best_tm, list) and isinstance(best_rmsd, list) and len(best_tm) == len(best_rmsd) == 2
    np.testing.assert_allclose(best_tm, [tm_to["t1"].max(), tm_to["t2"].max()], rtol=0, atol=1e-9)
    want_rmsd = [min(E.superpose_pair(s, t)[0] for s in S) for t in (t1, t2)]
    np.testing.assert_allclose(best_rmsd, want_rmsd, rtol=1e-9)
    pair = [E.tm_pair(S[i], S[j])[0] for i in range(12) for j in range(i + 1, 12)]
    np.testing.assert_allclose(ens.tm_diversity(S), np.mean(pair), rtol=0, atol=1e-9)
    # the down-sampling draws from the generator argument, not from numpy's global state
    sub = np.random.default_rng(3).choice(12, 5, replace=False)
    got = ens.tm_n_ensemble(S, np.stack([t1, t2]), max_n_model=5, rng=3)
    np.testing.assert_allclose(got[0], [tm_to["t1"][sub].max(), tm_to["t2"][sub].max()], rtol=0, atol=1e-9)
    assert got == ens.tm_n_ensemble(S, np.stack([t1, t2]), max_n_model=5, rng=np.random.default_rng(3))


def test_apo_report(ens, small):
    S, t1, t2 = small
    t1, t2 = t1.copy(), t2.copy()
    t1[[0, 1, 20]] = np.nan                   # unresolved residues, different ones in the two states
    t2[[20, 38, 39]] = np.nan
    m1, m2 = ~np.isnan(t1[:, 0]), ~np.isnan(t2[:, 0])
    rep = ens.apo_report(S, t1, t2)
    assert set(rep) == {"tm1max", "tm2max", "tm_ens", "ensvar", "tmpair", "rmsd", "rmsf"}
    tm1 = max(E.tm_pair(t1, s, m1, None)[0] for s in S)           # tmscore(state, sample): the sample normalises
    tm2 = max(E.tm_pair(t2, s, m2, None)[0] for s in S)
    np.testing.assert_allclose([rep["tm1max"], rep["tm2max"], rep["tm_ens"]], [tm1, tm2, (tm1 + tm2) / 2], rtol=0, atol=1e-9)
    ensvar = np.mean([E.tm_pair(S[k], S[j])[0] for j in range(12) for k in range(j + 1, 12)])
    np.testing.assert_allclose(rep["ensvar"], ensvar, rtol=0, atol=1e-9)
    tmpair = (E.tm_pair(t1, t2, m1, m2)[0] + E.tm_pair(t2, t1, m2, m1)[0]) / 2
    np.testing.assert_allclose(rep["tmpair"], tmpair, rtol=0, atol=1e-9)
    np.testing.assert_allclose(rep["rmsd"] ** 2, E.aligned_deviation_pair(t1, t2, m1, m2) ** 2, rtol=0, atol=1e-9, equal_nan=True)
    dev = np.stack([E.aligned_deviation_pair(S[j], S[k]) for j in range(12) for k in range(j + 1, 12)])
    np.testing.assert_allclose(rep["rmsf"] ** 2, np.mean(dev ** 2, 0), rtol=0, atol=1e-9)
    # explicit masks say the same as NaN coordinates
    rep2 = ens.apo_report(S, np.nan_to_num(t1), np.nan_to_num(t2), mask1=m1, mask2=m2)
    for k in ("tm1max", "tm2max", "tmpair"):
        assert rep2[k] == rep[k], k


def test_cli_writes_both_reports(ens, small, tmp_path):
    from esmdiff_amd import analyze_ensemble, pdbio
    S, t1, t2 = small

    def write(path, ca):
        bb = np.stack([ca + np.array([-0.5, 1.2, 0.3]), ca, ca + np.array([1.1, 0.9, -0.4])], axis=1)       # N, CA, C
        pdbio.write_backbone_pdb(path, "A" * len(ca), bb)

    files = []
    for i, s in enumerate(S):
        files.append(tmp_path / f"s_{i}.pdb")
        write(files[-1], s)
    pdbio.merge_pdbfiles(files, tmp_path / "target7.pdb", verbose=False)
    write(tmp_path / "a.pdb", t1)
    write(tmp_path / "b.pdb", t2)
    loaded = pdbio.load_coords(tmp_path / "target7.pdb", max_n_model=None, verbose=False)
    assert loaded.shape == (12, 40, 3)
    la, lb = (pdbio.load_coords(tmp_path / f, max_n_model=None, verbose=False)[0] for f in ("a.pdb", "b.pdb"))
    # two targets: the apo / holo row
    out = analyze_ensemble.main(["--samples", str(tmp_path / "target7.pdb"), "--targets", str(tmp_path / "a.pdb"), str(tmp_path / "b.pdb"),
                                 "--output", str(tmp_path / "apo")])
    assert out == tmp_path / "apo" / "target7.ensemble.json"
    rep, want = json.loads(out.read_text()), ens.apo_report(loaded, la, lb)
    assert set(rep) == {"tm1max", "tm2max", "tm_ens", "ensvar", "tmpair", "rmsd", "rmsf"}
    for k in ("tm1max", "tm2max", "tm_ens", "ensvar", "tmpair"):
        assert rep[k] == want[k], k
    assert np.array_equal(np.array(rep["rmsd"]), want["rmsd"]) and np.array_equal(np.array(rep["rmsf"]), want["rmsf"])
    assert len(rep["rmsd"]) == len(rep["rmsf"]) == 40
    # paths are accepted where arrays are
    assert ens.tm_diversity(tmp_path / "target7.pdb") == ens.tm_diversity(loaded)
    # K targets: the BPTI-style lists and the three csv columns
    out = analyze_ensemble.main(["--samples", str(tmp_path / "target7.pdb"), "--targets", str(tmp_path / "a.pdb"), str(tmp_path / "b.pdb"),
                                 str(tmp_path / "s_3.pdb"), "--output", str(tmp_path / "bpti"), "--max_models", "100"])
    rep = json.loads(out.read_text())
    assert set(rep) == {"best_tm", "best_rmsd", "TM-ens", "RMSD-ens", "TM-div"}
    assert len(rep["best_tm"]) == len(rep["best_rmsd"]) == 3
    assert abs(rep["best_tm"][2] - 1.0) < 1e-12 and rep["best_rmsd"][2] < ZERO_RMSD          # sample 3 is its own best match
    assert rep["TM-ens"] == np.mean(rep["best_tm"]) and rep["RMSD-ens"] == np.mean(rep["best_rmsd"])
    assert rep["TM-div"] == ens.tm_diversity(loaded)

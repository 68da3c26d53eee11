"""GPU tests of the contact layer (esmdiff_amd/csrc/contacts.hip through the C ABI, esmdiff_amd/pairs.py, esmdiff_amd/contacts.py and the
command line) against the numpy float64 restatement tests/contacts_ref.py (itself held to hand-worked cases and to the reference's own
idp_metrics numbers by tests/test_contacts_cpu.py).  Integer outputs are compared exactly, the two sums of the maps bit for bit; q_soft
to 1e-12 absolute (tests/test_metrics.py's TOL: the device's exp is not numpy's).  No network engine is built."""
import ctypes
import json
from pathlib import Path

import numpy as np
import pytest

from tests import contacts_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-12
GOLDEN = Path(__file__).parent / "golden"


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _dev(x, dt):
    import torch
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x, dtype=dt)).cuda()


def _map(X, mask=None, cutoff=R.CUTOFF, min_sep=R.MIN_SEP, sums=True, n=None, L=None, scratch_bytes=None):
    """esmdiff_contact_map on numpy inputs -> (code, valid, count, sum_d, sum_d2).  The outputs start as -7 and the scratch as 0xff
    bytes (NaN and -1): the caller zeroes nothing."""
    import torch
    from esmdiff_amd import _native as N
    x, mk = _dev(X, np.float64), _dev(mask, np.uint8)
    n = X.shape[0] if n is None else n
    L = X.shape[1] if L is None else L
    side = min(max(L, 1), X.shape[1])
    valid, count = (torch.full((side, side), -7, dtype=torch.int32, device="cuda") for _ in range(2))
    sum_d, sum_d2 = (torch.full((side, side), -7.0, dtype=torch.float64, device="cuda") for _ in range(2)) if sums else (None, None)
    size = R.scratch_bytes(n, L) if n >= 1 and 2 <= L <= R.MAX_L else 0
    size = size if scratch_bytes is None else scratch_bytes
    scratch = torch.full((max(size, 8),), 255, dtype=torch.uint8, device="cuda")
    code = N.lib().esmdiff_contact_map(_p(x), n, L, _p(mk), cutoff, min_sep, _p(valid), _p(count), _p(sum_d), _p(sum_d2),
                                       _p(scratch) if size else None, size, None)
    torch.cuda.synchronize()
    return (code, *[None if t is None else t.cpu().numpy() for t in (valid, count, sum_d, sum_d2)])


def _same_map(got, want, tag, sums=True):
    assert got[0] == 0, tag
    for name, g, w in zip(("valid", "count"), got[1:3], want[:2]):
        assert g.dtype == np.int32 and np.array_equal(g, w), f"{tag}: {name}"
    for name, g, w in zip(("sum_d", "sum_d2"), got[3:], want[2:]):
        if sums:
            assert g.dtype == np.float64 and np.array_equal(g.view(np.int64), w.view(np.int64)), f"{tag}: {name} differs in its bits"
        else:
            assert g is None
    for g in got[1:]:
        if g is not None:
            assert np.array_equal(g, g.T), f"{tag}: not symmetric"


def _ensemble(seed, n, L):
    rng = np.random.default_rng(seed)
    return R.ensemble(rng, n, R.chain(rng, L)), rng


# ---- 1. contact maps ------------------------------------------------------------------------------------------------------------------
# frames: one chunk (1, 16), both sides of the first chunk boundary (17: 16 + 1), three chunks with a ragged one (33, 40)
@pytest.mark.parametrize("L", [2, 5, 63, 64, 65, 128, 129])
def test_contact_map_equals_the_restatement(L):
    """64 is the tile edge: L = 63, 64 are one tile, 65 and 128 two tiles a side, 129 three (mirrored tiles, a ragged last tile)."""
    for n in (1, 16, 17, 33, 40):
        X, rng = _ensemble(100 * L + n, n, L)
        mask = rng.random((n, L)) > 0.25
        holes = X.copy()
        holes[rng.random((n, L)) < 0.2] = np.nan
        assert R.chunks(n, L) == {1: 1, 16: 1, 17: 2, 33: 3, 40: 3}[n]
        for min_sep in (1, 3):
            if L >= 63:
                _, count, _, _ = R.contact_map(X, None, R.CUTOFF, min_sep)
                assert 0 < count.sum() and (count[np.triu_indices(L, min_sep)] == 0).any(), "contacts and non-contacts"
            for tag, x, mk in (("plain", X, None), ("mask", X, mask), ("nan", holes, None), ("nan + mask", holes, mask)):
                want = R.contact_map(x, mk, R.CUTOFF, min_sep)
                _same_map(_map(x, mk, R.CUTOFF, min_sep), want, f"L={L} n={n} sep={min_sep} {tag}")
            idx = np.arange(L)
            near = np.abs(idx[:, None] - idx[None, :]) < min_sep
            for g in _map(X, None, R.CUTOFF, min_sep)[1:]:
                assert not g[near].any()
        _same_map(_map(X, mask, sums=False), R.contact_map(X, mask), f"L={L} n={n} without sums", sums=False)


@pytest.mark.parametrize("L", [5, 65])
def test_contact_map_with_the_most_chunks(L):
    """4089 frames: 256 chunks of 16, the last one of 9; 4100: chunks of 17, 242 of them, the last of 3."""
    assert (R.chunks(4089, L), R.chunk_frames(4089, L)) == (256, 16) and (R.chunks(4100, L), R.chunk_frames(4100, L)) == (242, 17)
    for n in (4089, 4100):
        X, rng = _ensemble(n + L, n, L)
        mask = rng.random((n, L)) > 0.1
        first = _map(X, mask, R.CUTOFF, 1)
        _same_map(first, R.contact_map(X, mask, R.CUTOFF, 1), f"L={L} n={n}")
        for g, f in zip(_map(X, mask, R.CUTOFF, 1), first):     # a second run is bit-identical
            assert np.array_equal(g, f, equal_nan=True)


def test_contact_map_where_the_tiles_cap_the_chunks():
    """L = 450: 8 tiles a side, 36 pair tiles, at most 28 chunks; 40 frames are 3 chunks of 16, 16 and 8 (the fold across many tiles)."""
    X, rng = _ensemble(450, 40, 450)
    assert R.chunks(40, 450) == 3 and R.pair_tiles(450) == 36
    mask = rng.random((40, 450)) > 0.1
    _same_map(_map(X, mask), R.contact_map(X, mask), "L=450")


def test_contact_map_boundary_and_errors():
    from esmdiff_amd import pairs
    import torch
    X = np.array([[[0.0, 0, 0], [3.0, 4.0, 0]]])
    assert _map(X, None, 5.0, 1)[2][0, 1] == 0 and _map(X, None, np.nextafter(5.0, 6.0), 1)[2][0, 1] == 1
    near = np.array([[[0.0, 0, 0], [np.nextafter(5.0, 0.0), 0, 0]]])
    assert _map(near, None, 5.0, 1)[2][0, 1] == 1
    Y, _ = _ensemble(3, 40, 12)
    assert _map(Y, n=0)[0] == -1 and _map(Y, L=1)[0] == -1 and _map(Y, min_sep=0)[0] == -1 and _map(Y, cutoff=float("nan"))[0] == -1
    assert _map(Y, L=R.MAX_L + 1)[0] == -5                      # refused before anything is launched or read
    assert _map(Y, scratch_bytes=R.scratch_bytes(40, 12) - 8)[0] == -5
    y = torch.as_tensor(Y).cuda()
    with pytest.raises(RuntimeError, match="min_sep = 0"):
        pairs.contact_map(y, None, 8.0, 0)
    with pytest.raises(RuntimeError, match=f"limit \\({R.MAX_L} residues\\)"):
        pairs.contact_map(torch.zeros((1, R.MAX_L + 1, 3), dtype=torch.float64, device="cuda"), None, 8.0, 3)
    valid, count, sum_d, sum_d2 = pairs.contact_map(y, None, 8.0, 3, sums=False)
    assert sum_d is None and sum_d2 is None and np.array_equal(count.cpu().numpy(), R.contact_map(Y)[1])


# ---- 2. the reference's numbers ---------------------------------------------------------------------------------------------------------
def test_contact_error_reproduces_the_reference_and_idp_metrics():
    from esmdiff_amd import contacts
    from esmdiff_amd import metrics as M
    G, GC = np.load(GOLDEN / "g9_metrics.npz"), np.load(GOLDEN / "g9c_ensemble_helpers.npz")
    keys = [str(k) for k in G["keys"]]
    ens = {k: G["ca_" + k] for k in keys}
    for tag, k in (("", 3), ("_k1", 1)):
        got = contacts.contact_error(dict(ens), pwd_offset=k)
        idp = M.idp_metrics(dict(ens), pwd_offset=k)
        for nm, d, other in zip(("mse_contact", "mae_contact", "mse_pwd", "mae_pwd"), got, (idp[2], idp[5], idp[0], idp[3])):
            mine = [d[key] for key in keys]
            print(nm, tag, mine, GC[f"idp_{nm}{tag}"].tolist(), [other[key] for key in keys])
            assert np.allclose(mine, GC[f"idp_{nm}{tag}"], rtol=1e-11, atol=1e-13), (nm, tag)
            assert np.allclose(mine, [other[key] for key in keys], rtol=1e-11, atol=1e-13), (nm, tag)
            assert d["target"] == 0.0


# ---- 3. native contacts ---------------------------------------------------------------------------------------------------------------
def _native(A, B, maskA=None, maskB=None, cutoff=R.CUTOFF, min_sep=R.MIN_SEP, lam=R.LAMBDA, beta=R.BETA, per_residue=True, soft=True,
            n=None, m=None, L=None):
    """esmdiff_native_contacts on numpy inputs -> (code, kept, total, kept_res, total_res, q_soft); the outputs start as -7."""
    import torch
    from esmdiff_amd import _native as N
    a, b, ma, mb = _dev(A, np.float64), _dev(B, np.float64), _dev(maskA, np.uint8), _dev(maskB, np.uint8)
    n = A.shape[0] if n is None else n
    m = (A if B is None else B).shape[0] if m is None else m
    L = A.shape[1] if L is None else L
    rows, cols, width = max(n, 1), max(m, 1), min(max(L, 1), A.shape[1])
    kept = torch.full((rows, cols), -7, dtype=torch.int32, device="cuda")
    total = torch.full((cols,), -7, dtype=torch.int32, device="cuda")
    kept_res = torch.full((rows, cols, width), -7, dtype=torch.int32, device="cuda") if per_residue else None
    total_res = torch.full((cols, width), -7, dtype=torch.int32, device="cuda") if per_residue else None
    q_soft = torch.full((rows, cols), -7.0, dtype=torch.float64, device="cuda") if soft else None
    code = N.lib().esmdiff_native_contacts(_p(a), n, _p(b), m, L, _p(ma), _p(mb), cutoff, min_sep, lam, beta, _p(kept), _p(total),
                                           _p(kept_res), _p(total_res), _p(q_soft), None)
    torch.cuda.synchronize()
    return (code, *[None if t is None else t.cpu().numpy() for t in (kept, total, kept_res, total_res, q_soft)])


def _same_native(got, want, tag):
    assert got[0] == 0, tag
    for name, g, w in zip(("kept", "total", "kept_res", "total_res"), got[1:5], want[:4]):
        if g is not None:
            assert g.dtype == np.int32 and g.shape == w.shape and np.array_equal(g, w), f"{tag}: {name}"
    if got[3] is not None:
        assert np.array_equal(got[3].sum(-1), got[1]) and np.array_equal(got[4].sum(-1), got[2]), f"{tag}: per-residue sums"
    if got[5] is not None:
        err = float(np.abs(got[5] - want[4]).max())
        print(tag, "q_soft max", float(want[4].max()), "err", err)
        assert err <= TOL, f"{tag}: q_soft off by {err}"


@pytest.mark.parametrize("L", [2, 5, 63, 64, 65, 129])
def test_native_contacts_equal_the_restatement(L):
    """8 models are one tile: n = 7, 8, 9, 17 are below, on and above it (a ragged second tile, three tiles); m on both sides as well."""
    for n, m in ((1, 1), (3, 9), (7, 2), (8, 1), (9, 2), (17, 1)):
        rng = np.random.default_rng(1000 * L + 10 * n + m)
        base = R.chain(rng, L)
        A, B = R.ensemble(rng, n, base, 0.2, 2.5), R.ensemble(rng, m, base, 0.0, 1.0)
        if L >= 63:
            kept, total, _, _, _ = R.native_contacts(A, B)
            assert total.min() > 0 and 0 < kept.sum() < np.broadcast_to(total, kept.shape).sum(), "contacts kept and contacts lost"
        masks = [(None, None), (rng.random((n, L)) > 0.2, None), (None, rng.random((m, L)) > 0.2),
                 (rng.random((n, L)) > 0.2, rng.random((m, L)) > 0.2)]
        for ma, mb in masks:
            for min_sep in (1, 3):
                tag = f"L={L} n={n} m={m} masks={ma is not None},{mb is not None} sep={min_sep}"
                want = R.native_contacts(A, B, ma, mb, min_sep=min_sep)
                _same_native(_native(A, B, ma, mb, min_sep=min_sep), want, tag)
        # the other template (no q_soft: rows split over workgroups) and NULL per-residue outputs
        got = _native(A, B, masks[3][0], masks[3][1], per_residue=False, soft=False)
        assert got[3] is None and got[4] is None and got[5] is None
        _same_native(got, R.native_contacts(A, B, masks[3][0], masks[3][1]), f"L={L} n={n} m={m} counts only")


def test_native_contacts_self_masked_coordinates_and_two_runs():
    rng = np.random.default_rng(7)
    A = R.ensemble(rng, 5, R.chain(rng, 65))
    ma = rng.random((5, 65)) > 0.25
    want = R.native_contacts(A, None, ma)
    holes = A.copy()
    holes[~ma] = np.nan                                          # NaN under the mask changes nothing
    first = _native(holes, None, ma)
    _same_native(first, want, "B == NULL")
    second = _native(holes, holes, ma, ma)
    for g, f in zip(second, first):                              # bit-identical, q_soft included
        assert np.array_equal(g, f)
    full = _native(A, None)
    assert np.array_equal(np.diag(full[1]), full[2])             # Q(native, native) = 1 hard ...
    assert np.all(np.diag(full[5]) < full[2]) and np.all(np.diag(full[5]) > 0.9 * full[2])      # ... and below 1 soft


def test_native_contacts_boundaries_and_other_parameters():
    native = np.array([[[0.0, 0, 0], [3.0, 4.0, 0]]])
    assert _native(native, native, cutoff=5.0, min_sep=1)[2].tolist() == [0]
    assert _native(native, native, cutoff=np.nextafter(5.0, 6.0), min_sep=1)[2].tolist() == [2]
    models = np.stack([R.line([0, 5.0]), R.line([0, np.nextafter(5.0, 0.0)]), R.line([0, np.nextafter(5.0, 6.0)])])
    got = _native(models, native, cutoff=6.0, min_sep=1, lam=1.0)
    assert got[0] == 0 and got[2].tolist() == [2] and got[1][:, 0].tolist() == [0, 2, 0]
    _same_native(got, R.native_contacts(models, native, cutoff=6.0, min_sep=1, lam=1.0), "lam = 1")
    # the hand-worked case of the CPU tests
    got = _native(R.line([0, 4, 9, 18])[None], R.line([0, 4, 8, 12])[None], min_sep=1)
    assert got[2].tolist() == [6] and got[4].tolist() == [[1, 2, 2, 1]] and got[1].tolist() == [[2]] and got[3].tolist() == [[[1, 1, 0, 0]]]
    rng = np.random.default_rng(11)
    base = R.chain(rng, 70)
    A, B = R.ensemble(rng, 4, base), R.ensemble(rng, 2, base, 0.0, 0.5)
    for kw in ({"cutoff": 10.0, "lam": 1.8, "beta": 2.0}, {"cutoff": 6.5, "lam": 1.0, "beta": 50.0, "min_sep": 4}):
        _same_native(_native(A, B, **kw), R.native_contacts(A, B, **kw), str(kw))


def test_native_contacts_errors_surface_as_the_binding_texts():
    import torch
    from esmdiff_amd import pairs
    rng = np.random.default_rng(9)
    A, B = R.ensemble(rng, 2, R.chain(rng, 12)), R.ensemble(rng, 3, R.chain(rng, 12))
    assert _native(A, B, n=0)[0] == -1 and _native(A, B, m=0)[0] == -1 and _native(A, B, L=1)[0] == -1
    assert _native(A, B, min_sep=0)[0] == -1 and _native(A, B, lam=float("nan"))[0] == -1
    assert _native(A, B, L=R.MAX_L + 1)[0] == -5                 # refused before anything is launched or read
    a, b = torch.as_tensor(A).cuda(), torch.as_tensor(B).cuda()
    with pytest.raises(RuntimeError, match="esmdiff_native_contacts: invalid argument.*min_sep = 0"):
        pairs.native_contacts(a, b, None, None, 8.0, 0, 1.2, 5.0)
    big = torch.zeros((1, R.MAX_L + 1, 3), dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match=f"esmdiff_native_contacts: L = {R.MAX_L + 1} is beyond the kernel's limit"):
        pairs.native_contacts(big, None, None, None, 8.0, 3, 1.2, 5.0)
    kept, total, kept_res, total_res, q_soft = pairs.native_contacts(a, b, None, None, 8.0, 3, 1.2, 5.0, soft=False)
    assert kept_res is None and total_res is None and q_soft is None
    assert np.array_equal(kept.cpu().numpy(), R.native_contacts(A, B)[0])


# ---- 4. the Python layer --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(2025)
    base = R.chain(rng, 30)
    S, K = R.ensemble(rng, 9, base, 0.1, 2.0), R.ensemble(rng, 3, base, 0.0, 0.5)
    K[2, 4] = np.nan                                             # an unresolved native residue
    S[1, 7] = np.nan                                             # and an unresolved sample residue
    return S, K


def test_host_contact_map_and_native_contacts(data):
    from esmdiff_amd import contacts
    S, K = data
    m = contacts.contact_map(S)
    valid, count, sum_d, sum_d2 = R.contact_map(S)
    assert np.array_equal(m.valid, valid) and np.array_equal(m.count, count) and m.valid[7, 20] == 8 and m.n_frames == 9
    assert np.array_equal(m.sum_d, sum_d) and np.array_equal(m.sum_d2, sum_d2)
    freq, mean = R.frequency(valid, count), R.per_frame(valid, sum_d)
    assert np.array_equal(m.frequency(), freq, equal_nan=True) and np.isnan(m.frequency()[0, 1]) and np.nanmax(freq) == 1.0
    assert np.array_equal(m.mean_distance(), mean, equal_nan=True)
    assert np.array_equal(m.log_probability(), np.log(freq + 0.01), equal_nan=True)
    var = R.per_frame(valid, sum_d2) - mean ** 2
    assert np.allclose(m.std_distance(), np.sqrt(np.maximum(var, 0)), rtol=0, atol=1e-15, equal_nan=True)
    mask = np.random.default_rng(1).random((9, 30)) > 0.3
    want = R.contact_map(S, mask, 10.0, 2)
    got = contacts.contact_map(S, cutoff=10.0, min_separation=2, mask=mask)
    assert np.array_equal(got.count, want[1]) and np.array_equal(got.sum_d2, want[3])

    mk = ~np.isnan(K).any(-1)
    ms = ~np.isnan(S).any(-1)
    hard, soft, res = R.q(S, K, ms, mk)
    nc = contacts.native_contacts(S, K, per_residue=True)
    assert nc.q.shape == (9, 3) and nc.q_residue.shape == (9, 3, 30)
    assert np.array_equal(nc.q, hard) and np.array_equal(np.isnan(nc.q_residue), np.isnan(res)) and np.isnan(res[:, 2, 4]).all()
    assert np.nanmax(np.abs(nc.q_residue - res)) == 0 and np.max(np.abs(nc.q_soft - soft)) <= TOL
    assert contacts.native_contacts(S, K).q_residue is None
    hard18 = R.q(S, K, ms, mk, cutoff=9.0, min_sep=4, lam=1.8, beta=3.0)
    nc18 = contacts.native_contacts(S, K, cutoff=9.0, min_separation=4, lam=1.8, beta=3.0)
    assert np.array_equal(nc18.q, hard18[0]) and np.max(np.abs(nc18.q_soft - hard18[1])) <= TOL
    best, q_ens = contacts.q_ensemble(S, K)
    assert np.array_equal(best, hard.max(0)) and q_ens == float(np.mean(hard.max(0)))
    far = R.line([0, 20, 40, 60])
    none = contacts.native_contacts(far, far)
    assert np.isnan(none.q[0, 0]) and np.isnan(none.q_soft[0, 0]) and none.total.tolist() == [0]
    assert np.isnan(contacts.q_ensemble(far, far)[1])


def _two_states():
    """State 1: a straight rod with 3.5 A steps — its contacts below 8 A with |a - b| >= 2 are the pairs (a, a + 2), 7 A apart.  State 2: a
    hairpin with 4 A steps, residues 0 .. 5 out along x, 6 .. 11 back at y = 6: residues a <= 5 and b >= 6 are
    sqrt(16 (11 - a - b)^2 + 36) apart — 6 A, 7.2 A or at least 10 A — and two residues of one arm 4 |a - b| >= 8 A."""
    rod = R.line(3.5 * np.arange(12))
    hairpin = np.array([[4.0 * k, 0, 0] if k <= 5 else [4.0 * (11 - k), 6.0, 0] for k in range(12)])
    in_1 = {(a, a + 2) for a in range(10)}
    in_2 = {(a, b) for a in range(6) for b in range(6, 12) if abs(a + b - 11) <= 1 and b - a >= 2}
    return rod, hairpin, in_1, in_2


def test_contact_switches_on_two_constructed_states():
    from esmdiff_amd import contacts
    rod, hairpin, in_1, in_2 = _two_states()
    assert (4, 6) in in_1 & in_2 and (5, 7) in in_1 & in_2 and len(in_2) == 15
    S = np.stack([rod, rod, hairpin, rod])
    got = contacts.contact_switches(S, rod, hairpin, min_separation=2)
    assert {tuple(g["pair"]) for g in got if g["state"] == 1} == in_1 - in_2
    assert {tuple(g["pair"]) for g in got if g["state"] == 2} == in_2 - in_1
    assert all(g["frequency"] == (0.75 if g["state"] == 1 else 0.25) for g in got) and len(got) == 8 + 13
    assert [(g["pair"][0], g["pair"][1], g["state"], g["frequency"]) for g in got] == R.contact_switches(S, rod, hairpin, min_sep=2)
    # an unresolved target residue takes its pairs out; samples without the pair give None
    broken = hairpin.copy()
    broken[3] = np.nan
    got = contacts.contact_switches(S, rod, broken, min_separation=2)
    assert not [g for g in got if 3 in g["pair"]] and len(got) == 8 + 13 - 2 - 3
    holes = S.copy()
    holes[:, 0] = np.nan
    got = contacts.contact_switches(holes, rod, hairpin, min_separation=2)
    assert all((g["frequency"] is None) == (0 in g["pair"]) for g in got)


def test_internal_scaling_and_flory_exponent():
    from esmdiff_amd import contacts
    rod = R.line(4.0 * np.arange(20))
    shifted = np.stack([rod, rod + 3.0, rod[:, [1, 0, 2]]])       # the rod along x, moved, and along y
    sc = contacts.internal_scaling(shifted)
    assert np.array_equal(sc.separation, np.arange(1, 20)) and np.array_equal(sc.rms_distance, 4.0 * np.arange(1, 20))
    assert abs(contacts.flory_exponent(sc) - 1.0) <= 1e-12 and abs(contacts.flory_exponent(sc, fit_range=(3, 12)) - 1.0) <= 1e-12
    rng = np.random.default_rng(4)
    S = R.ensemble(rng, 20, R.chain(rng, 40))
    mask = rng.random((20, 40)) > 0.2
    mask[:, 0] = False                                           # the separation L - 1 has no resolved pair
    sep, rms = R.internal_scaling(S, mask)
    got = contacts.internal_scaling(S, mask)
    assert np.isnan(rms[-1]) and np.array_equal(got.rms_distance, rms, equal_nan=True)
    nu = contacts.flory_exponent(got)
    x, y = np.log(sep[:-1]), np.log(rms[:-1])
    assert abs(nu - np.polyfit(x, y, 1)[0]) <= 1e-12 and 0.2 < nu < 0.8       # a noisy random walk: below one half


# ---- 5. the command line ----------------------------------------------------------------------------------------------------------------
def test_command_line(tmp_path):
    from esmdiff_amd import analyze_ensemble, contacts, pdbio
    rng = np.random.default_rng(31)
    states = [R.chain(rng, 24) for _ in range(2)]

    def write(path, ca):
        bb = np.stack([ca + np.array([-0.5, 1.2, 0.3]), ca, ca + np.array([1.1, 0.9, -0.4])], axis=1)
        pdbio.write_backbone_pdb(path, "A" * len(ca), bb)

    files = []
    for i, k in enumerate((0, 1, 0, 1, 1, 0)):
        files.append(tmp_path / f"s_{i}.pdb")
        write(files[-1], states[k] + rng.normal(size=(24, 3)) * 0.3)
    samples_path = tmp_path / "t7.pdb"
    pdbio.merge_pdbfiles(files, samples_path, verbose=False)
    targets = []
    for k in range(2):
        targets.append(tmp_path / f"state_{k}.pdb")
        write(targets[-1], states[k])
    S = pdbio.load_coords(samples_path, max_n_model=None, verbose=False).astype(np.float64)
    K = np.stack([pdbio.load_coords(t, max_n_model=None, verbose=False)[0] for t in targets]).astype(np.float64)

    common = ["--samples", str(samples_path), "--targets", *map(str, targets)]
    with_flag = analyze_ensemble.main(common + ["--output", str(tmp_path / "a"), "--contacts", "--contact_cutoff", "9.0",
                                                "--contact_min_sep", "2"])
    without = analyze_ensemble.main(common + ["--output", str(tmp_path / "b")])
    doc = json.loads(with_flag.read_text())
    block = doc.pop("contacts")
    assert "contacts" not in json.loads(without.read_text())
    assert json.dumps(doc, indent=1) + "\n" == without.read_text()          # the rest is byte for byte the run without the flag

    assert (block["cutoff"], block["min_separation"], block["lam"], block["beta"]) == (9.0, 2, 1.2, 5.0)
    valid, count, sum_d, _ = R.contact_map(S, None, 9.0, 2)
    a, b = np.nonzero(np.triu(count > 0, 1))
    assert [c[:2] for c in block["contacts"]] == [[int(i), int(j)] for i, j in zip(a, b)] and len(a) > 20
    assert [c[2] for c in block["contacts"]] == (count[a, b] / valid[a, b]).tolist()
    assert [c[3] for c in block["contacts"]] == (sum_d[a, b] / valid[a, b]).tolist()
    sep, rms = R.internal_scaling(S)
    assert block["scaling"]["separation"] == sep.tolist() and block["scaling"]["rms_distance"] == rms.tolist()
    assert block["flory_exponent"] == contacts.flory_exponent(contacts.Scaling(sep, rms))
    hard, soft, _ = R.q(S, K, cutoff=9.0, min_sep=2)
    total = R.native_contacts(S, K, cutoff=9.0, min_sep=2)[1]
    for k in range(2):
        t = block["targets"][k]
        assert t["n_contacts"] == total[k] // 2 and t["q"] == hard[:, k].tolist() and np.max(np.abs(np.array(t["q_soft"]) - soft[:, k])) <= TOL
        assert t["q_mean"] == float(np.mean(hard[:, k])) and t["q_best"] == hard[:, k].max() and t["best_model"] == int(hard[:, k].argmax())
    assert block["q_ens"] == float(np.mean(hard.max(0)))
    want = R.contact_switches(S, K[0], K[1], 9.0, 2)
    assert [(g["pair"][0], g["pair"][1], g["state"], g["frequency"]) for g in block["contact_switches"]] == want and len(want) > 5

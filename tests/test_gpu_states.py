"""The three entries of csrc/msm.hip and esmdiff_amd/states.py on the device against tests/states_ref.py: integer operands EQUAL the
int64 restatement, real operands are bit-equal to the published-order restatement and within the any-order rounding bound of plain
numpy sums; every padded dimension, the centre-tile and chunk boundaries, ties, NaN and inf, scratch slots and refusals; the transition
counts on both sides of the LDS / global switch; and the model level (Lloyd loop, kmeans++, TICA -> k-means -> MSM on two wells)."""
import ctypes

import numpy as np
import pytest

from tests import states_ref as R

pytestmark = pytest.mark.gpu

TILE, CHUNK = R.CENTRE_TILE, R.FRAME_CHUNK
KS = [1, 2, 63, 64, 65, TILE - 1, TILE + 1, 2 * TILE + 3]
NS = [1, 63, 64, 65, CHUNK - 1, CHUNK + 1, 2 * CHUNK + 3]


def dev(a, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda") if dtype is None else torch.as_tensor(np.ascontiguousarray(a).astype(dtype), device="cuda")


def bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def run(Y, C, slots=None):
    """-> what the two entries give for (Y, C), as numpy: labels, dist2 of the assignment; labels, counts, sums, inertia of the step."""
    from esmdiff_amd import pairs
    labels, dist2 = pairs.kmeans_assign(dev(Y, np.float64), dev(C, np.float64))
    res = pairs.kmeans_step(dev(Y, np.float64), dev(C, np.float64), slots=slots)
    return (labels.cpu().numpy(), dist2.cpu().numpy()), (res["labels"].cpu().numpy(), res["counts"].cpu().numpy(), res["sums"].cpu().numpy(),
                                                         float(res["inertia"][0]))


def check_case(n, k, d, seed):
    rng = np.random.default_rng(seed)
    # integer operands: everything EQUALS the int64 restatement
    Yi, Ci = rng.integers(-512, 513, size=(n, d)), rng.integers(-512, 513, size=(k, d))
    (la, d2), (ls, counts, sums, inertia) = run(Yi, Ci)
    li, d2i = R.assign_int(Yi, Ci)
    _, ci, si, ii = R.step_int(Yi, Ci)
    assert np.array_equal(la, li) and np.array_equal(ls, li) and la.dtype == np.int32
    assert np.array_equal(d2, d2i.astype(np.float64)) and np.array_equal(counts, ci) and counts.dtype == np.int64
    assert np.array_equal(sums, si.astype(np.float64)) and inertia == float(ii)
    # real operands: bit-equal to the published order, and within the any-order bound of plain numpy
    Y, C = rng.standard_normal((n, d)) * 3.0, rng.standard_normal((k, d)) * 3.0
    (la, d2), (ls, counts, sums, inertia) = run(Y, C)
    lr, d2r = R.assign(Y, C)
    _, cr, sr, ir = R.step(Y, C)
    assert np.array_equal(la, lr) and np.array_equal(ls, lr) and np.array_equal(counts, cr)
    assert bits(d2, d2r) and bits(sums, sr) and bits(inertia, ir)
    plain = ((Y - C[lr]) ** 2).sum(1)                                                 # numpy's own order
    assert (np.abs(d2 - plain) <= 2.0 * R.gamma(d) * plain).all()
    for j in range(k):
        mine = Y[lr == j]
        if len(mine):
            assert (np.abs(sums[j] - mine.sum(0)) <= 2.0 * R.gamma(len(mine)) * np.abs(mine).sum(0)).all()
        else:
            assert bits(sums[j], np.zeros(d))                                         # an empty cluster: +0.0
    assert abs(inertia - plain.sum()) <= 2.0 * R.gamma(n) * plain.sum() + 2.0 * R.gamma(d) * plain.sum()


@pytest.mark.parametrize("d", [1, 2, 3, 5, 16])
@pytest.mark.parametrize("k", KS)
def test_centres_and_dimensions(k, d):
    """Every padded dimension (1, 2, 4, 8, 16) against every k around the wave and the centre tile, three chunks of frames."""
    check_case(2 * CHUNK + 3, k, d, seed=1000 * k + d)


@pytest.mark.parametrize("kd", [(65, 3), (TILE + 1, 16)], ids=lambda p: "x".join(map(str, p)))
@pytest.mark.parametrize("n", NS)
def test_frame_counts(n, kd):
    check_case(n, kd[0], kd[1], seed=n)


def test_ties_go_to_the_lower_index():
    k = TILE + 2
    C = np.zeros((k, 2))
    C[:, 0] = 4.0 * np.arange(k)
    C[k - 1] = C[5]                                                                   # a duplicate of centre 5, in the second tile
    pairs_of = np.arange(TILE + 1)                                                    # j and j + 1 for j <= TILE: 127 | 128 straddles the tile boundary
    Y = np.concatenate([np.stack([4.0 * pairs_of + 2.0, np.zeros(len(pairs_of))], 1),           # exactly midway: both distances are 4
                        np.stack([4.0 * 5 + np.array([-1.0, 0.0, 1.0]), np.array([1.0, 0.0, -1.0])], 1)])     # nearest to centre 5 and its copy
    (la, d2), (ls, counts, sums, inertia) = run(Y, C)
    want = np.concatenate([pairs_of, [5, 5, 5]]).astype(np.int32)
    assert np.array_equal(la, want) and np.array_equal(ls, want) and la[TILE - 1] == TILE - 1 and la[TILE] == TILE
    assert np.array_equal(d2[:len(pairs_of)], np.full(len(pairs_of), 4.0)) and np.array_equal(d2[-3:], [2.0, 0.0, 2.0])
    assert counts[k - 1] == 0 and bits(sums[k - 1], np.zeros(2)) and counts[5] == 4
    lr, cr, sr, ir = R.step(Y, C)
    assert np.array_equal(counts, cr) and bits(sums, sr) and bits(inertia, ir)


def test_nan_and_inf():
    rng = np.random.default_rng(5)
    n, k, d = CHUNK + 40, 70, 3
    Y, C = rng.standard_normal((n, d)), rng.standard_normal((k, d))
    bad = [0, 7, 63, 64, CHUNK - 1, CHUNK, n - 1]
    for i, t in enumerate(bad):
        Y[t, i % d] = [np.nan, np.inf, -np.inf][i % 3]
    (la, d2), (ls, counts, sums, inertia) = run(Y, C)
    lr, cr, sr, ir = R.step(Y, C)
    assert (la[bad] == -1).all() and np.isnan(d2[bad]).all() and (np.delete(la, bad) >= 0).all() and np.isfinite(np.delete(d2, bad)).all()
    assert np.array_equal(la, lr) and np.array_equal(ls, lr) and bits(d2, R.assign(Y, C)[1])
    assert counts.sum() == n - len(bad) and np.array_equal(counts, cr) and bits(sums, sr) and bits(inertia, ir) and np.isfinite(sums).all()
    clean = np.delete(Y, bad, axis=0)                                                 # the frame is absent from every sum
    assert (np.abs(sums.sum(0) - clean.sum(0)) <= 2.0 * R.gamma(len(clean)) * np.abs(clean).sum(0)).all()
    # one centre non-finite: never chosen, the others as without it
    Y = rng.standard_normal((300, d))
    for value in (np.nan, np.inf, -np.inf):
        C2 = C.copy()
        near = R.assign(Y, C)[0]
        victim = int(np.bincount(near, minlength=k).argmax())
        C2[victim, 1] = value
        (la, d2), (ls, counts, sums, inertia) = run(Y, C2)
        assert not (la == victim).any() and counts[victim] == 0 and (la >= 0).all() and np.array_equal(la, R.assign(Y, C2)[0])
        keep = near != victim
        assert np.array_equal(la[keep], near[keep])
    # every centre non-finite: every label -1, nothing summed
    (la, d2), (ls, counts, sums, inertia) = run(Y, np.full((k, d), np.nan))
    assert (la == -1).all() and (ls == -1).all() and np.isnan(d2).all() and counts.sum() == 0 and bits(sums, np.zeros((k, d))) and bits(inertia, 0.0)


def test_slots_change_no_bit():
    import torch
    from esmdiff_amd import pairs
    rng = np.random.default_rng(9)
    Y, C = dev(rng.standard_normal((3 * CHUNK + 17, 5))), dev(rng.standard_normal((40, 5)))
    ref = pairs.kmeans_step(Y, C)
    for slots in (1, 2, 3, 4, 9, None):
        got = pairs.kmeans_step(Y, C, slots=slots)
        assert all(torch.equal(ref[key].view(torch.uint8), got[key].view(torch.uint8)) for key in ref), slots
    no_labels = pairs.kmeans_step(Y, C, labels=False)
    assert "labels" not in no_labels and torch.equal(no_labels["sums"].view(torch.uint8), ref["sums"].view(torch.uint8))
    assert torch.equal(pairs.kmeans_assign(Y, C, dist2=False)[0], ref["labels"]) and pairs.kmeans_assign(Y, C, dist2=False)[1] is None
    empty = pairs.kmeans_step(Y[:0].contiguous(), C)                                  # n = 0: the sums of nothing
    assert int(empty["counts"].sum()) == 0 and bits(empty["sums"].cpu().numpy(), np.zeros((40, 5))) and float(empty["inertia"][0]) == 0.0
    assert pairs.kmeans_assign(Y[:0].contiguous(), C)[0].shape == (0,)


def test_refusals_write_nothing():
    import torch
    from esmdiff_amd import _native as N
    from esmdiff_amd.pairs import _p, _stream
    L = N.lib()
    null = ctypes.c_void_p(0)

    def garbage(shape, dtype):
        return torch.full(shape, -77, dtype=dtype, device="cuda")

    def step(n, d, k, scratch_bytes, scratch_null=False):
        Y, C = torch.zeros((n, d), dtype=torch.float64, device="cuda"), torch.zeros((k, d), dtype=torch.float64, device="cuda")
        outs = [garbage((n,), torch.int32), garbage((k,), torch.int64), garbage((k, d), torch.float64), garbage((1,), torch.float64)]
        scratch = garbage((max(scratch_bytes // 8, 1),), torch.int64)
        code = L.esmdiff_kmeans_step(_p(Y), n, d, _p(C), k, _p(outs[0]), _p(outs[1]), _p(outs[2]), _p(outs[3]), null if scratch_null else _p(scratch),
                                     scratch_bytes, _stream())
        torch.cuda.synchronize()
        return code, all(bool((o == -77).all()) for o in outs + [scratch])

    def assign(n, d, k):
        Y, C = torch.zeros((n, d), dtype=torch.float64, device="cuda"), torch.zeros((k, d), dtype=torch.float64, device="cuda")
        outs = [garbage((n,), torch.int32), garbage((n,), torch.float64)]
        code = L.esmdiff_kmeans_assign(_p(Y), n, d, _p(C), k, _p(outs[0]), _p(outs[1]), _stream())
        torch.cuda.synchronize()
        return code, all(bool((o == -77).all()) for o in outs)

    one = N.kmeans_slot_bytes(10, 3)
    assert step(50, 3, 10, one - 8) == (-5, True) and step(50, 3, 10, 0) == (-5, True)          # a short scratch: ESMDIFF_E_CAPACITY
    assert step(50, 3, 10, one, scratch_null=True) == (-1, True)                                  # a NULL scratch: ESMDIFF_E_INVALID
    assert step(4, 17, 2, N.kmeans_slot_bytes(2, 17)) == (-5, True) and assign(4, 17, 2) == (-5, True)
    assert step(4, 2, 4097, N.kmeans_slot_bytes(4097, 2)) == (-5, True) and assign(4, 2, 4097) == (-5, True)
    assert step(50, 3, 10, one)[0] == 0 and assign(50, 3, 10)[0] == 0                              # and the same calls within the limits run
    Y = torch.zeros((4, 2), dtype=torch.float64, device="cuda")
    lab = garbage((4,), torch.int32)
    assert L.esmdiff_kmeans_assign(_p(Y), 4, 2, null, 1, _p(lab), null, _stream()) == -1 and bool((lab == -77).all())
    assert L.esmdiff_kmeans_assign(_p(Y), -1, 2, _p(Y), 1, _p(lab), null, _stream()) == -1
    # the transition counts: a label equal to k is found before anything is written
    labels = torch.as_tensor(np.array([0, 1, 2, 1, 0, 3], np.int32), device="cuda")
    counts, scratch = garbage((3, 3), torch.int64), torch.zeros(1, dtype=torch.int64, device="cuda")
    assert L.esmdiff_transition_counts(_p(labels), 6, 3, 1, _p(counts), _p(scratch), 8, _stream()) == -1 and bool((counts == -77).all())
    assert L.esmdiff_transition_counts(_p(labels), 6, 3, 0, _p(counts), _p(scratch), 8, _stream()) == -1
    assert L.esmdiff_transition_counts(_p(labels), 6, 3, 1, _p(counts), null, 8, _stream()) == -1
    assert L.esmdiff_transition_counts(_p(labels), 6, 3, 1, _p(counts), _p(scratch), 4, _stream()) == -5
    assert L.esmdiff_transition_counts(_p(labels), 6, 4097, 1, _p(counts), _p(scratch), 8, _stream()) == -5 and bool((counts == -77).all())
    assert L.esmdiff_transition_counts(_p(labels), 6, 4, 1, _p(garbage((4, 4), torch.int64)), _p(scratch), 8, _stream()) == 0
    from esmdiff_amd import pairs
    with pytest.raises(RuntimeError, match="label >= k"):
        pairs.transition_counts(labels, 3, 1)


@pytest.mark.parametrize("k", [1, 2, R.TRANSITION_LDS_MAX_K, R.TRANSITION_LDS_MAX_K + 1])
def test_transition_counts(k):
    """Both sides of the LDS / global switch; one pair, no pair, a lag beyond a workgroup's chunk; labels that hold -1."""
    from esmdiff_amd import pairs
    rng = np.random.default_rng(k)
    n = R.TRANSITION_FRAME_CHUNK + 300
    labels = rng.integers(0, k, size=n).astype(np.int32)
    labels[rng.random(n) < 0.05] = -1
    labels[[0, n - 1]] = k - 1
    held = dev(labels)
    for lag in (1, 7, R.TRANSITION_FRAME_CHUNK + 2, n - 1, n, n + 5):
        got = pairs.transition_counts(held, k, lag).cpu().numpy()
        want = R.transition_counts(labels, k, lag)
        valid = int(((labels[:max(n - lag, 0)] >= 0) & (labels[lag:] >= 0)).sum()) if lag < n else 0
        assert got.dtype == np.int64 and np.array_equal(got, want) and got.sum() == valid, lag
        if lag >= n:
            assert got.sum() == 0
        if lag == n - 1:
            assert got.sum() == 1 and got[k - 1, k - 1] == 1
    clean = rng.integers(0, k, size=500).astype(np.int32)
    assert np.array_equal(pairs.transition_counts(dev(clean), k, 3).cpu().numpy(), R.transition_counts(clean, k, 3))
    assert pairs.transition_counts(dev(clean[:0]), k, 3).sum() == 0


def test_kmeans_equals_the_restated_lloyd_loop():
    from esmdiff_amd import states
    Y, init = R.blob_problem()                                                        # well posed: tests/test_states_cpu.py
    centres, labels, counts, inertia, updates, converged = R.lloyd(Y, init)
    model = states.kmeans(Y, len(init), init=init)
    assert np.array_equal(model.labels, labels) and bits(model.centres, centres) and np.array_equal(model.counts, counts)
    assert bits(model.inertia, inertia) and model.n_iter == updates and model.converged == converged and converged
    assert np.array_equal(model.assign(Y), labels) and np.array_equal(model.assign(Y[:77]), labels[:77])
    short = states.kmeans(Y, len(init), init=init, n_iter=1)
    c1, l1, n1, i1, u1, v1 = R.lloyd(Y, init, n_iter=1)
    assert short.n_iter == 1 and not short.converged and bits(short.centres, c1) and np.array_equal(short.labels, l1) and bits(short.inertia, i1)
    halves = states.kmeans([Y[:1000], Y[1000:]], len(init), init=init)               # a list of trajectories: taken together
    assert bits(halves.centres, centres) and np.array_equal(halves.labels, labels)
    # an empty cluster keeps its centre: a centre far from every frame
    far = np.concatenate([init, [[1e3, 1e3, 1e3]]])
    model = states.kmeans(Y, len(far), init=far)
    cf, lf, nf, _, _, _ = R.lloyd(Y, far)
    assert model.counts[-1] == 0 and bits(model.centres[-1], far[-1]) and bits(model.centres, cf) and np.array_equal(model.labels, lf)


def test_kmeans_plus_plus_is_reproducible():
    from esmdiff_amd import states
    Y, _, owner = R.blobs(3000, 6, 2, seed=4)
    a, b = states.kmeans(Y, 6, seed=11), states.kmeans(Y, 6, seed=11)
    assert bits(a.centres, b.centres) and np.array_equal(a.labels, b.labels) and bits(a.inertia, b.inertia) and a.n_iter == b.n_iter
    assert a.converged and a.counts.sum() == len(Y) and np.array_equal(a.counts, np.bincount(a.labels, minlength=6))
    u = states.kmeans(Y, 6, init="uniform")
    assert u.converged and u.counts.sum() == len(Y)
    with pytest.raises(ValueError):
        states.kmeans(Y[:3], 6)
    with pytest.raises(ValueError, match="nan or inf"):
        states.kmeans(np.array([[0.0, np.nan], [1.0, 1.0]]), 1)


def test_two_wells_through_tica_kmeans_and_msm():
    from esmdiff_amd import kinetics, states
    lag, k = 5, 8
    X, wells = R.two_wells(6000, 4, seed=0, hop=0.01)
    tica = kinetics.tica(X, lag, dim=1, features=True)
    Y = tica.transform(X)
    km = states.kmeans(Y, k, seed=0)
    assert np.array_equal(states.discretize(tica, X, km), km.labels)
    counts = states.transition_counts(km.labels, lag, k)
    assert np.array_equal(counts, R.transition_counts(km.labels, k, lag)) and counts.sum() == len(X) - lag
    split = states.transition_counts([km.labels[:2500], km.labels[2500:]], lag, k)    # a list: no pair crosses the boundary
    assert np.array_equal(split, R.transition_counts(km.labels[:2500], k, lag) + R.transition_counts(km.labels[2500:], k, lag))
    model = states.msm(km.labels, lag, k=k)
    assert len(model.active_set) == k and model.converged and np.array_equal(model.counts, counts)
    want = R.slowest_timescale(km.labels, k, lag)
    truth = -1.0 / np.log(1.0 - 2.0 * 0.01)
    print(f"MEASURED two wells: slowest timescale {model.timescales[0]:.6f} frames, restated {want:.6f}, the jump process's {truth:.1f}")
    assert abs(model.timescales[0] - want) <= 1e-9 * want
    assert 0.5 * truth < model.timescales[0] < 2.0 * truth and abs(model.eigenvalues[2]) < 0.5 < model.eigenvalues[1]
    sets = model.metastable(2)
    side = np.array([np.round(wells[km.labels == s].mean()) for s in model.active_set]).astype(int)
    purity = np.array([(wells[km.labels == s] == side[i]).mean() for i, s in enumerate(model.active_set)])
    assert purity.min() > 0.99 and set(side) == {0, 1}
    assert len(set(sets.assignment[side == 0])) == 1 and len(set(sets.assignment[side == 1])) == 1 and sets.assignment[side == 0][0] != sets.assignment[side == 1][0]
    assert abs(sets.weights.sum() - 1.0) <= 1e-12 and sets.weights.min() > 0.2
    table = states.msm_timescales(km.labels, [lag, 2 * lag], n=2, k=k)
    assert table.shape == (2, 2) and abs(table[0, 0] - model.timescales[0]) <= 1e-9 * want and np.isfinite(table[:, 0]).all()
    res = states.compare_populations(km.labels, model, sets)                          # the trajectory against its own model
    assert res["outside"] == 0.0 and res["js"] < 0.1 and np.abs(res["populations"]["samples"] - res["populations"]["msm"]).max() < 0.1


def test_the_command_line_block():
    """states.report on a small synthetic chain: every key of the "msm" block, consistent with one another and writable as JSON."""
    import json
    from esmdiff_amd import states
    from esmdiff_amd.analyze_ensemble import _jsonable
    from tests import kinetics_ref as K
    traj = K.trajectory(1500, 6, seed=2)
    samples, targets = traj[::50].copy(), traj[:2].copy()
    block = states.report(traj, samples, targets, lagtime=5, dim=2, states=6, msm_lagtime=3, metastable=2, seed=1)
    whole = states.report(traj, samples, targets, lagtime=5, dim=2, states=6, msm_lagtime=3, metastable=2, seed=1, chunk_frames=400)
    assert block["states"] == 6 and block["lagtime"] == 3 and block["tica_lagtime"] == 5 and block["frames"] == 1500 and block["seed"] == 1
    assert block["count_total"] == 1500 - 3 and 2 <= block["active_states"] <= 6 and len(block["active_set"]) == block["active_states"]
    assert block["centres"].shape == (6, 2) and block["inertia"] > 0 and block["kmeans_iterations"] >= 1
    pi = block["stationary_distribution"]
    assert len(pi) == block["active_states"] and abs(pi.sum() - 1.0) <= 1e-12 and (pi > 0).all()
    assert abs(block["eigenvalues"][0] - 1.0) <= 1e-10 and len(block["timescales"]) == len(block["eigenvalues"]) - 1
    assert block["sample_labels"].shape == (30,) and block["target_labels"].shape == (2,) and block["sample_labels"].max() < 6
    sets = block["metastable"]
    assert len(sets) == 2 and abs(sum(s["weight"] for s in sets) - 1.0) <= 1e-12 and all(len(s["mean_tic"]) == 2 for s in sets)
    assert sorted(np.concatenate([s["states"] for s in sets]).tolist()) == block["active_set"].tolist()
    cmp = block["compare_populations"]
    assert 0.0 <= cmp["outside"] <= 1.0 and cmp["n_samples"] == 30 and abs(cmp["populations"]["msm"].sum() - 1.0) <= 1e-12
    # the trajectory in pieces of 400 pairs: another order of the moments' sums, so equal only up to rounding in the coordinates
    assert whole["frames"] == 1500 and whole["count_total"] == block["count_total"] and whole["sample_labels"].shape == (30,)
    assert abs(whole["eigenvalues"][0] - 1.0) <= 1e-10 and abs(whole["stationary_distribution"].sum() - 1.0) <= 1e-12
    text = json.dumps({k: _jsonable(v) for k, v in block.items()})
    assert json.loads(text)["states"] == 6

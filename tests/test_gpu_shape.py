"""GPU tests of the shape layer (esmdiff_amd/csrc/shape.hip through the C ABI, esmdiff_amd/shape.py and the command line) against the
numpy float64 restatement tests/shape_ref.py (itself held to hand-worked cases by tests/test_shape_cpu.py).  Every output starts as a
sentinel.
  count, hist, dmax    exactly equal on every input: d and d / width are the same IEEE operations on both sides
  centroid, tensor sums, sum_inv_d, ree    bit for bit, the restatement following the published orders
  Debye                |device - restatement| <= 1e-13 E for every (frame, q), E the envelope sum f^2 + 2 sum |f_a f_b| min(1, 1 / (q d)).
                       The restatement (math.fsum of numpy's terms) is within 2e-16 E of a long-double evaluation; the device differs
                       from it in its sin (a few ulp) and in the order of summation (depth x 2^-53): 1e-13, about 450 ulp of E, leaves two
                       orders of magnitude.  The worst ratio is printed (MEASURED debye) and recorded in EXPERIMENTS.md.
Shapes: L = 1, 2, 3, 63, 64, 65, 130 (one wave up to 128, eight beyond) and 1 026; 4 096 with one frame and two q (integers, dmax and the
Debye bar only) and 4 097 refused; n = 0, 1, 17, 300 at L = 12 (eight frames a workgroup, the last one partly filled); Q = 1, 8, 9, 51
around the chunk of 8 and 1 025 refused; bins = 1 and 100."""
import ctypes
import json
from pathlib import Path

import numpy as np
import pytest

from tests import shape_ref as R

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = np.load(ROOT / "tests" / "golden" / "g9_metrics.npz")
SENTINEL_I, SENTINEL_F = -7, 1.0e30
E_INVALID, E_CAPACITY = -1, -5
BAR = 1e-13


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _dev(x, dt):
    import torch
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x, dtype=dt)).cuda()


def _frames(X, mask=None, width=None, bins=0, n=None, L=None, null=(), cells=None):
    """esmdiff_shape_frames on numpy inputs -> (code, count, desc, hist); the outputs start as sentinels.  width None: hist is NULL."""
    import torch
    from esmdiff_amd import _native as N
    x, mk = _dev(X, np.float64), _dev(mask, np.uint8)
    rows = max(X.shape[0], 1)
    out = {"count": torch.full((rows,), SENTINEL_I, dtype=torch.int32, device="cuda"),
           "desc": torch.full((rows, 12), SENTINEL_F, dtype=torch.float64, device="cuda"),
           "hist": None if width is None else torch.full((max(bins, 1) + 1 if cells is None else cells,), SENTINEL_I, dtype=torch.int64, device="cuda")}
    arg = {k: None if k in null else v for k, v in out.items()}
    code = N.lib().esmdiff_shape_frames(_p(None if "X" in null else x), X.shape[0] if n is None else n, X.shape[1] if L is None else L, _p(mk),
                                        _p(arg["count"]), _p(arg["desc"]), _p(arg["hist"]), 0.0 if width is None else float(width), bins, None)
    torch.cuda.synchronize()
    return (code, *[None if t is None else t.cpu().numpy() for t in out.values()])


def _debye(X, q, ff=None, mask=None, n=None, L=None, Q=None, null=()):
    """esmdiff_debye_frames on numpy inputs -> (code, intensity); the output starts as a sentinel."""
    import torch
    from esmdiff_amd import _native as N
    x, mk, qd, fd = _dev(X, np.float64), _dev(mask, np.uint8), _dev(q, np.float64), _dev(ff, np.float64)
    out = torch.full((max(X.shape[0], 1), len(q)), SENTINEL_F, dtype=torch.float64, device="cuda")
    code = N.lib().esmdiff_debye_frames(_p(None if "X" in null else x), X.shape[0] if n is None else n, X.shape[1] if L is None else L, _p(mk),
                                        _p(None if "q" in null else qd), len(q) if Q is None else Q, _p(fd),
                                        _p(None if "intensity" in null else out), None)
    torch.cuda.synchronize()
    return code, out.cpu().numpy()


def _bits(a):
    """The bytes of a float64 array as integers, every NaN as one value."""
    a = np.ascontiguousarray(a, np.float64)
    return np.where(np.isnan(a), np.int64(-1), a.view(np.int64))


def _spoil(rng, X, k):
    """The mask patterns, one per frame in turn (frame s gets pattern (k + s) % 5): untouched; a masked residue; a NaN coordinate and
    the first and the last residue masked; every residue masked; one valid residue."""
    n, L = X.shape[:2]
    mask = np.ones((n, L), bool)
    for s in range(n):
        kind = (k + s) % 5
        if kind == 1:
            mask[s, rng.integers(0, L)] = False
        elif kind == 2:
            X[s, rng.integers(0, L), rng.integers(0, 3)] = np.nan
            mask[s, 0] = mask[s, -1] = False
        elif kind == 3:
            mask[s] = False
        elif kind == 4:
            mask[s] = False
            mask[s, rng.integers(0, L)] = True
    return X, (None if mask.all() else mask)


def _q(Q):
    return np.linspace(0.0, 0.5, Q) if Q > 1 else np.array([0.3])


@pytest.fixture(scope="module")
def cases():
    """[(tag, X, mask, bins, width, q, reference frames, reference debye)], each reference computed once."""
    rng = np.random.default_rng(20261020)
    shapes = [(L, 5, (1, 8, 9, 51)[k % 4], (1, 100)[k % 2]) for k, L in enumerate((1, 2, 3, 63, 64, 65, 130))]
    shapes += [(1026, 2, 2, 100), (12, 1, 9, 100), (12, 17, 8, 1), (12, 300, 9, 100)]
    out = []
    for k, (L, n, Q, bins) in enumerate(shapes):
        X = R.chains(rng, n, L)
        if k % 3 == 0:
            X[0, L // 2] = X[0, 0]                                      # two coincident atoms in the first frame: d = 0, 1 / d = +inf, s(0) = 1
        X, mask = _spoil(rng, X, 0 if n < 5 else k)
        width = (1.0, 0.37)[k % 2] if bins > 1 else 7.3
        q = _q(Q)
        out.append((f"L={L} n={n} Q={Q} bins={bins}", X, mask, bins, width, q, R.frames(X, mask, width, bins), R.debye(X, q, None, mask)))
    return out


def _check_frames(got, want, tag, sums=True):
    code, count, desc, hist = got
    assert code == 0, tag
    assert np.array_equal(count, want[0]), f"{tag}: count"
    if want[2] is not None:
        assert np.array_equal(hist, want[2]), f"{tag}: hist"
    assert np.array_equal(desc[:, 10], want[1][:, 10]), f"{tag}: dmax"
    assert not np.any(desc == SENTINEL_F) and not np.any(count == SENTINEL_I), f"{tag}: an element was not written"
    if sums:
        for name, cols in (("centroid", slice(0, 3)), ("tensor sums", slice(3, 9)), ("sum_inv_d", slice(9, 10)), ("ree", slice(11, 12))):
            assert np.array_equal(_bits(desc[:, cols]), _bits(want[1][:, cols])), f"{tag}: {name}"


# ---- 1. esmdiff_shape_frames ----------------------------------------------------------------------------------------------------------
def test_frames_equal_the_restatement(cases):
    pairs_seen = 0
    for tag, X, mask, bins, width, _, want, _ in cases:
        got = _frames(X, mask, width, bins)
        _check_frames(got, want, tag)
        assert got[3].sum() == (want[0] * (want[0] - 1) // 2).sum(), tag
        pairs_seen += int(got[3].sum())
        alone = _frames(X, mask)                                         # without the histogram: the same descriptors
        assert alone[3] is None and np.array_equal(_bits(alone[2]), _bits(got[2])) and np.array_equal(alone[1], got[1]), tag
        again = _frames(X, mask, width, bins)                            # two runs
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got[1:], again[1:])), tag
    assert pairs_seen > 1_000_000
    seen = np.concatenate([c[6][0] for c in cases])
    assert (seen == 0).any() and (seen == 1).any()                       # a frame with nothing, a frame with one residue


def test_a_frame_does_not_see_its_batch(cases):
    for tag, X, mask, _, _, q, _, _ in cases:
        if X.shape[0] < 5:
            continue
        batch, scat = _frames(X, mask), _debye(X, q, None, mask)
        for s in (0, 2, X.shape[0] - 1):
            mk = None if mask is None else mask[s:s + 1]
            alone, one = _frames(X[s:s + 1], mk), _debye(X[s:s + 1], q, None, mk)
            assert alone[1][0] == batch[1][s] and alone[2][0].tobytes() == batch[2][s].tobytes(), (tag, s)
            assert one[1][0].tobytes() == scat[1][s].tobytes(), (tag, s)


def test_garbage_in_masked_residues_changes_nothing(cases):
    rng = np.random.default_rng(5)
    tag, X, _, bins, width, q = next(c for c in cases if c[1].shape[:2] == (5, 130))[:6]
    X = np.nan_to_num(X, nan=1.0)
    mask = rng.random(X.shape[:2]) > 0.2
    dirty = X.copy()
    dirty[~mask] = rng.choice([np.nan, np.inf, -np.inf, 1e300, 0.0], size=dirty[~mask].shape)
    a, b = _frames(X, mask, width, bins), _frames(dirty, mask, width, bins)
    assert a[0] == b[0] == 0 and all(u.tobytes() == v.tobytes() for u, v in zip(a[1:], b[1:]))
    assert _debye(X, q, None, mask)[1].tobytes() == _debye(dirty, q, None, mask)[1].tobytes()


# ---- 2. esmdiff_debye_frames ----------------------------------------------------------------------------------------------------------
def _worst(got, want, tag):
    code, I = got
    ref, env = want
    assert code == 0 and not np.any(I == SENTINEL_F) and np.isfinite(I).all(), tag
    ratio = np.where(env > 0, np.abs(I - ref) / np.where(env > 0, env, 1.0), np.abs(I - ref))
    return float(ratio.max(initial=0.0))


def test_debye_within_the_bar(cases):
    worst = 0.0
    for tag, X, mask, _, _, q, frames_ref, want in cases:
        got = _debye(X, q, None, mask)
        w = _worst(got, want, tag)
        print(f"MEASURED debye {tag}: worst |device - restatement| / E = {w:.3e}")
        worst = max(worst, w)
        assert w <= BAR, f"{tag}: {w} of the envelope"
        if q[0] == 0.0:                                                  # every term is 1.0
            assert np.array_equal(got[1][:, 0], (frames_ref[0] * frames_ref[0]).astype(np.float64)), f"{tag}: I(0) is N^2"
        assert _debye(X, q, None, mask)[1].tobytes() == got[1].tobytes(), f"{tag}: two runs"
    print(f"MEASURED debye worst ratio over the cases: {worst:.3e} (bar {BAR:g})")


def test_the_same_q_gives_the_same_bits_in_any_array(cases):
    for tag, X, mask, _, _, _, _, _ in cases:
        if X.shape[1] not in (12, 65, 130) or X.shape[0] > 17:
            continue
        q = _q(51)
        full = _debye(X, q, None, mask)[1]
        for k in (0, 7, 8, 23, 48, 50):
            assert _debye(X, q[k:k + 1], None, mask)[1][:, 0].tobytes() == full[:, k].tobytes(), (tag, k)
        shifted = _debye(X, q[3:12], None, mask)[1]                      # other chunk positions, Q = 9
        assert shifted.tobytes() == np.ascontiguousarray(full[:, 3:12]).tobytes(), tag


def test_form_factors(cases):
    from esmdiff_amd import shape
    rng = np.random.default_rng(11)
    for tag, X, mask, _, _, q, _, _ in cases:
        L = X.shape[1]
        if L not in (3, 12, 64, 130) or X.shape[0] > 17:
            continue
        ones = _debye(X, q, np.ones((L, len(q))), mask)
        assert ones[0] == 0 and ones[1].tobytes() == _debye(X, q, None, mask)[1].tobytes(), f"{tag}: ff of ones against NULL"
        ff = shape.sphere_form_factor(q[None, :] * rng.uniform(1.5, 3.5, (L, 1)), 1.0) * rng.choice([1.0, -0.5, 2.0], (L, 1))
        w = _worst(_debye(X, q, ff, mask), R.debye(X, q, ff, mask), tag)
        print(f"MEASURED debye with form factors {tag}: worst ratio {w:.3e}")
        assert w <= BAR, f"{tag}: {w} of the envelope with form factors"


def test_coincident_atoms_give_finite_values():
    X = np.zeros((2, 5, 3))
    X[1, :, 0] = [0.0, 0.0, 3.8, 3.8, 7.6]
    q = _q(9)
    code, I = _debye(X, q)
    ref, env = R.debye(X, q)
    assert code == 0 and np.isfinite(I).all() and np.array_equal(I[0], np.full(9, 25.0)) and (np.abs(I - ref) <= BAR * env).all()
    got = _frames(X, None, 1.0, 10)
    _check_frames(got, R.frames(X, None, 1.0, 10), "coincident")
    assert np.isinf(got[2][:, 9]).all() and got[3][0] == 12             # 1 / 0 is +inf, by the header; ten pairs at d = 0 and two more


# ---- 3. the limits ---------------------------------------------------------------------------------------------------------------------
def test_the_longest_chain():
    rng = np.random.default_rng(4096)
    X = R.chain(rng, 4096)[None]
    X[0, 1234] = np.nan
    q = np.array([0.0, 0.5])
    want = R.frames(X, None, 2.0, 100, sums=False)
    _check_frames(_frames(X, None, 2.0, 100), want, "L=4096", sums=False)
    w = _worst(_debye(X, q), R.debye(X, q), "L=4096")
    print(f"MEASURED debye L=4096 n=1 Q=2: worst ratio {w:.3e}")
    assert w <= BAR


def test_capacity_and_invalid_calls_touch_nothing():
    X = R.chains(np.random.default_rng(1), 3, 12)
    q = _q(9)
    clean = lambda got: all(np.all(a == (SENTINEL_F if a.dtype == np.float64 else SENTINEL_I)) for a in got[1:] if a is not None)
    long = np.zeros((1, 4097, 3))
    got = _frames(long, None, 1.0, 10)
    assert got[0] == E_CAPACITY and clean(got)
    got = _debye(long, q)
    assert got[0] == E_CAPACITY and clean(got)
    got = _debye(X, np.linspace(0.0, 0.5, 1025))
    assert got[0] == E_CAPACITY and clean(got)
    assert _debye(X, np.linspace(0.0, 0.5, 1024))[0] == 0
    got = _frames(X, None, 1.0, 4097, cells=16)
    assert got[0] == E_CAPACITY and clean(got)
    for kw in ({"n": -1}, {"L": 0}, {"null": ("X",)}, {"null": ("count",)}, {"null": ("desc",)}, {"bins": 0}, {"bins": -4}, {"width": 0.0},
               {"width": -1.0}, {"width": np.nan}, {"width": np.inf}):
        got = _frames(X, **{"width": 1.0, "bins": 10, **kw})
        assert got[0] == E_INVALID and clean(got), kw
    for kw in ({"n": -1}, {"L": 0}, {"Q": 0}, {"null": ("X",)}, {"null": ("q",)}, {"null": ("intensity",)}):
        got = _debye(X, q, **kw)
        assert got[0] == E_INVALID and clean(got), kw
    got = _frames(X, None, 1.0, 10, n=0)                                # no frame: the histogram is zeroed, nothing else is touched
    assert got[0] == 0 and clean(got[:3]) and not got[3].any()
    got = _debye(X, q, n=0)
    assert got[0] == 0 and clean(got)
    assert _frames(X, None, None, -5)[0] == 0                           # without hist, width and bins are ignored


# ---- 4. the Python layer and the command line -----------------------------------------------------------------------------------------
def test_python_layer(cases):
    from esmdiff_amd import shape
    d = shape.frames(GOLDEN["ca_target"])
    assert np.abs(d.rg / GOLDEN["rg_target"] - 1.0).max() <= 1e-12
    for tag, X, mask, _, _, _, want, _ in cases:
        if X.shape[1] > 130 or X.shape[0] > 17:
            continue
        d, ref = shape.frames(X, mask), R.derived(want[0], want[1])
        assert np.array_equal(d.count, want[0]) and np.array_equal(_bits(d.centroid), _bits(want[1][:, :3])), tag
        for name, w in ref.items():
            g = getattr(d, name)
            assert np.array_equal(np.isnan(g), np.isnan(w)), f"{tag}: NaN pattern of {name}"
            ok = np.isfinite(w)
            assert np.array_equal(np.isinf(g), np.isinf(w)) and (np.abs(g[ok] - w[ok]) <= 1e-12 * np.maximum(1.0, np.abs(w[ok]))).all(), f"{tag}: {name}"
        assert set(d.summary()) == set(shape.QUANTITIES)
    X = np.nan_to_num(cases[6][1], nan=0.5)                             # (5, 130, 3)
    mask = np.ones(X.shape[:2], bool)
    mask[1, 3:9] = False
    N = mask.sum(1)
    for bins, r_max in ((100, None), (1, None), (40, 20.0)):
        pr = shape.distance_distribution(X, r_max, bins, mask)
        assert pr["counts"].sum() + pr["overflow"] == (N * (N - 1) // 2).sum() and (pr["overflow"] == 0) == (r_max is None)
        assert pr["width"] == pr["r_max"] / bins and len(pr["edges"]) == bins + 1 and abs((pr["p"] * pr["width"]).sum() - 1.0) < 1e-12
    assert pr["r_max"] == 20.0 and np.array_equal(pr["counts"], R.frames(X, mask, 0.5, 40)[2][:40])
    top = shape.frames(X, mask).dmax.max()
    assert shape.distance_distribution(X, None, 10, mask)["r_max"] == np.ceil(top)
    q = _q(9)
    I = shape.debye(X, q, mask=mask)
    ref, env = R.debye(X, q, None, mask)
    assert (np.abs(I - ref) <= BAR * env).all()
    prof = shape.saxs_profile(X, q)
    full = shape.debye(X, q)
    assert np.array_equal(prof["intensity"], full.sum(0) / 5.0) and prof["i0"] == 130.0 ** 2 and prof["normalised"][0] == 1.0
    w = np.array([1.0, 0.0, 0.0, 3.0, 0.0])
    assert np.allclose(shape.saxs_profile(X, q[1:], weights=w)["intensity"], (full[0, 1:] + 3.0 * full[3, 1:]) / 4.0, rtol=1e-14)
    assert shape.saxs_profile(X, q[1:])["i0"] == 130.0 ** 2
    for bad in ([-0.1, 0.2], [0.1, np.nan], [np.inf], []):
        with pytest.raises(ValueError, match="non-negative"):
            shape.debye(X, bad)
    with pytest.raises(RuntimeError, match="L = 4097"):
        shape.frames(np.zeros((1, 4097, 3)))
    # a compact chain: the Guinier radius of the point-scatterer profile is the coordinate Rg (the mean of Rg^2 over frames, to O(q^4))
    fine = np.linspace(0.0, 0.02, 21)
    fit = shape.guinier_rg(fine, shape.saxs_profile(X, fine)["intensity"])
    rms = np.sqrt(np.mean(shape.frames(X).rg ** 2))
    assert abs(fit["rg"] / rms - 1.0) < 0.02 and abs(fit["i0"] / 130.0 ** 2 - 1.0) < 1e-2
    # js_shape: 0 against itself; the conventions of js_rg on the quantity they share
    from esmdiff_amd import metrics
    a, b = GOLDEN["ca_target"], GOLDEN["ca_model_a"]
    same = shape.js_shape({"target": a, "same": a})
    assert set(same) == {"rg", "ree", "rh", "asphericity"} and all(v == {"same": 0.0, "target": 0.0} for v in same.values())
    js = shape.js_shape({"target": a, "model": b}, quantities=("rg", "dmax"))
    assert abs(js["rg"]["model"] - metrics.js_rg({"target": a, "model": b})["model"]) <= 1e-4 and 0.0 < js["dmax"]["model"] <= 1.0   # one unit of the rounding


def test_command_line(tmp_path):
    from esmdiff_amd import analyze_ensemble, pdbio, shape
    g = np.load(ROOT / "tests" / "golden" / "g14_backbones.npz")
    xyz, seq = g["bpti_xyz"], str(g["bpti_seq"])
    rng = np.random.default_rng(11)
    centred = xyz[:, :3] - xyz[:, 1].mean(0)
    files = []
    for i, sigma in enumerate((0.0, 0.05, 0.1, 0.2, 0.3, 0.1)):
        files.append(tmp_path / f"s_{i}.pdb")
        pdbio.write_backbone_pdb(files[-1], seq, centred + sigma * rng.normal(size=centred.shape))
    pdbio.merge_pdbfiles(files[:4], tmp_path / "ens.pdb", verbose=False)
    ca = pdbio.load_coords(tmp_path / "ens.pdb", max_n_model=None, verbose=False).astype(np.float64)
    q_exp = np.linspace(0.01, 0.4, 25)
    i_exp = 3.0 * shape.debye(ca[2], q_exp)[0]
    lines = ["# q I sigma"] + [f"{a:.6f} {b:.9e} {0.02 * b:.9e}" for a, b in zip(q_exp, i_exp)]
    (tmp_path / "saxs.dat").write_text("\n".join(lines) + "\n")

    args = ["--samples", str(tmp_path / "ens.pdb"), "--targets", str(files[4]), str(files[5])]
    plain = analyze_ensemble.main(args + ["--output", str(tmp_path / "plain")])
    full = json.loads(analyze_ensemble.main(args + ["--output", str(tmp_path / "shape"), "--shape", "--pr_bins", "50", "--saxs"]).read_text())
    assert "shape" not in json.loads(plain.read_text()) and "saxs" not in json.loads(plain.read_text())
    rest = {k: v for k, v in full.items() if k not in ("shape", "saxs")}
    assert json.dumps(rest, indent=1) + "\n" == plain.read_text()        # the other keys: the same bytes
    block, d = full["shape"], shape.frames(ca)
    assert block["pr_bins"] == 50 and len(block["pr"]["counts"]) == 50 and sum(block["pr"]["counts"]) == 4 * 58 * 57 // 2 and block["pr"]["overflow"] == 0
    for k in shape.QUANTITIES:
        assert np.array_equal(np.array(block["samples"][k], float), getattr(d, k)) and block["summary"][k]["n"] == 4, k
    assert block["samples"]["count"] == [58] * 4 and len(block["targets"]) == 2 and block["targets"][0]["count"] == 58
    assert abs(block["targets"][1]["rg"] - shape.frames(pdbio.load_coords(files[5], max_n_model=None, verbose=False)).rg[0]) < 1e-12
    assert block["js_shape"]["n_targets"] == 2 and set(block["js_shape"]) == {"n_targets", "rg", "ree", "rh", "asphericity"}
    sx = full["saxs"]
    assert len(sx["q"]) == 51 and sx["q"][-1] == 0.5 and sx["i0"] == 58.0 ** 2 and sx["normalised"][0] == 1.0 and "chi2_mean" not in sx
    assert abs(sx["guinier"]["rg"] / sx["rg_coordinates_rms"] - 1.0) < 0.1 and len(sx["kratky"]["y"]) == 51
    data = json.loads(analyze_ensemble.main(args + ["--output", str(tmp_path / "data"), "--saxs_data", str(tmp_path / "saxs.dat")]).read_text())
    sx = data["saxs"]
    assert "shape" not in data and np.allclose(sx["q"], q_exp, rtol=0, atol=1e-6) and len(sx["chi2_samples"]["chi2"]) == 4
    assert sx["chi2_samples"]["best_model"] == 2 and sx["chi2_samples"]["chi2"][2] < 1e-6 and abs(sx["chi2_samples"]["scale"][2] - 3.0) < 1e-5
    assert sx["chi2_mean"]["chi2"] >= 0.0 and sx["chi2_mean"]["scale"] > 0.0


# ---- 5. the caller's stream ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clock():
    from tests.stream_order import Clock
    return Clock()


@pytest.mark.parametrize("name", ["shape_frames", "shape_frames_hist", "debye_frames", "debye_frames_ff"])
def test_entries_work_on_the_callers_stream(clock, name):
    """On a delayed non-blocking stream against the null stream: bit-equal outputs, and the call has synchronised the stream."""
    import torch
    from esmdiff_amd import pairs
    from tests.stream_order import run_both
    n, L, Q = 6, 40, 9
    gen = lambda seed: torch.Generator().manual_seed(seed)
    chain = lambda k: torch.cumsum(torch.randn(n, L, 3, generator=gen(1 + k), dtype=torch.float64) * 2.2, 1)
    qs = lambda k: torch.linspace(0.0, 0.5 - 0.1 * k, Q, dtype=torch.float64)
    ffs = lambda k: 1.0 + torch.rand(L, Q, generator=gen(5 + k), dtype=torch.float64)
    mk, call = {
        "shape_frames": (lambda k: [chain(k)], lambda b: pairs.shape_frames(b[0], None)[:2]),
        "shape_frames_hist": (lambda k: [chain(k)], lambda b: pairs.shape_frames(b[0], None, 0.5, 100)),
        "debye_frames": (lambda k: [chain(k), qs(k)], lambda b: pairs.debye_frames(b[0], None, b[1])),
        "debye_frames_ff": (lambda k: [chain(k), qs(k), ffs(k)], lambda b: pairs.debye_frames(b[0], None, b[1], b[2])),
    }[name]
    fresh, stale = [t.cuda() for t in mk(0)], [t.cuda() for t in mk(1)]
    rep = run_both(clock, name, lambda: fresh, lambda: stale, call)
    print(f"MEASURED stream order {rep.name}: host return {rep.host_ms:.3f} ms, delay {rep.delay_ms:.0f} ms, "
          f"busy_on_return {rep.busy_on_return}, mismatches {rep.mismatches}")
    assert rep.ok, (rep.name, rep.mismatches)
    assert rep.busy_on_return is False, (rep.name, "the entry synchronises its stream")

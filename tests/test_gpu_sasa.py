"""GPU tests of the accessibility layer (esmdiff_amd/csrc/sasa.hip through the C ABI, esmdiff_amd/accessibility.py and the command line)
against the numpy float64 restatement tests/sasa_ref.py (itself held to hand-worked cases by tests/test_sasa_cpu.py).  Every output starts
as a sentinel.  THE BAR: every integer output — count, sum_count, valid, exposed, exposed_count, present_count and the three co-occurrence
maps — is exactly equal to the restatement on every input, the restatement having no cull and no early exit; the areas derived in Python
from those integers equal the restatement's bit for bit; two runs are identical.
Shapes: 1, 2, 63, 64, 65, 129 atoms a frame (around the chunk of 64 candidates), 256 and 260 (a frame to a wave up to 256 atoms, to eight
beyond), 4 096 with one frame at P = 8 and 4 097 refused; A = 1, 3 and 4; P = 1, 63, 64, 65, 96, 1 024 and 1 025 refused; n = 0, 1, 17,
300 at L = 12 (eight frames a workgroup, the last one partly filled).  Co-occurrence: every n of 0, 1, 63, 64, 65, 129, 1 000 with every
L of 1, 2, 63, 64, 65, 130.  The caller's-stream contract of the two entries is held in tests/test_gpu_stream_sasa.py, which says why it is
a module of its own."""
import ctypes
import json
from pathlib import Path

import numpy as np
import pytest

from tests import sasa_ref as R

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
BACKBONES = np.load(ROOT / "tests" / "golden" / "g14_backbones.npz")
NAMES = ("count", "sum_count", "valid", "exposed", "exposed_count", "present_count")
SENTINEL = {"count": -7, "sum_count": -7, "valid": -7, "exposed": 77, "exposed_count": -7, "present_count": -7}
E_INVALID, E_CAPACITY = -1, -5
BACKBONE_R = np.add(R.DEFAULT_RADII, 1.4)


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _dev(x, dt):
    import torch
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x, dtype=dt)).cuda()


def _sasa(X, mask, radii, points, threshold=0.2, null=(), **over):
    """esmdiff_sasa_frames on numpy inputs -> (code, {name: array}); every output starts as its sentinel, the names in `null` are NULL."""
    import torch
    from esmdiff_amd import _native as N
    n, L, A = X.shape[:3]
    rows = max(n, 1)
    x, mk, rd, ud = _dev(X, np.float64), _dev(mask, np.uint8), _dev(radii, np.float64), _dev(points, np.float64)
    shapes = {"count": ((rows, L, A), torch.int32), "sum_count": ((L, A), torch.int64), "valid": ((L, A), torch.int32),
              "exposed": ((rows, L), torch.uint8), "exposed_count": ((L,), torch.int32), "present_count": ((L,), torch.int32)}
    out = {k: torch.full(s, SENTINEL[k], dtype=dt, device="cuda") for k, (s, dt) in shapes.items()}
    arg = lambda k, t: None if k in null else t
    code = N.lib().esmdiff_sasa_frames(_p(arg("X", x)), over.get("n", n), over.get("L", L), over.get("A", A), _p(mk), _p(arg("radii", rd)),
                                       _p(arg("points", ud)), over.get("P", len(points)), float(threshold), *[_p(arg(k, out[k])) for k in NAMES], None)
    torch.cuda.synchronize()
    return code, {k: v.cpu().numpy() for k, v in out.items()}


def _untouched(got, names=NAMES):
    return all(np.all(got[k] == SENTINEL[k]) for k in names)


def _equal(got, want, tag, n):
    code, out = got
    assert code == 0, tag
    for k in NAMES:
        g = out[k][:n] if k in ("count", "exposed") else out[k]
        assert g.dtype == want[k].dtype and np.array_equal(g, want[k]), f"{tag}: {k}"


def _spoil(rng, X, k):
    """The five mask patterns of tests/test_gpu_shape.py, one per frame in turn (frame s gets pattern (k + s) % 5): untouched; a masked
    residue; a NaN coordinate of one atom and the first and the last residue masked; every residue masked; one valid residue."""
    n, L, A = X.shape[:3]
    mask = np.ones((n, L), bool)
    for s in range(n):
        kind = (k + s) % 5
        if kind == 1:
            mask[s, rng.integers(0, L)] = False
        elif kind == 2:
            X[s, rng.integers(0, L), rng.integers(0, A), rng.integers(0, 3)] = np.nan
            mask[s, 0] = mask[s, -1] = False
        elif kind == 3:
            mask[s] = False
        elif kind == 4:
            mask[s] = False
            mask[s, rng.integers(0, L)] = True
    return X, (None if mask.all() else mask)


def _coils(rng, n, L, A):
    return np.stack([R.coil(rng, L, A) for _ in range(n)])


def _radii(L, A):
    return np.tile(BACKBONE_R if A == 4 else BACKBONE_R[:A] if A == 3 else [3.27], (L, 1)).astype(np.float64)


@pytest.fixture(scope="module")
def cases():
    """[(tag, X, mask, radii, points, threshold, reference)], each reference computed once."""
    rng = np.random.default_rng(20261021)
    out = []

    def add(tag, X, mask, radii, P, threshold=0.2):
        u = R.sphere_points(P)
        out.append((f"{tag} n={X.shape[0]} L={X.shape[1]} A={X.shape[2]} P={P}", X, mask, radii, u, threshold, R.frames(X, mask, radii, u, threshold)))

    for k, (atoms, P) in enumerate(zip((1, 2, 63, 64, 65, 129), (96, 1, 63, 64, 65, 96))):      # around the chunk of 64 candidates
        X, mask = _spoil(rng, _coils(rng, 5, atoms, 1), k)
        add("coil", X, mask, _radii(atoms, 1), P, (0.2, 0.5)[k % 2])
    for n, P in ((1, 1024), (17, 96), (300, 65)):                                               # eight frames a workgroup
        X, mask = _spoil(rng, _coils(rng, n, 12, 4), n)
        add("coil", X, mask, _radii(12, 4), P)
    X, mask = _spoil(rng, _coils(rng, 10, 21, 3), 1)
    add("coil", X, mask, _radii(21, 3), 96)
    X, mask = _spoil(rng, _coils(rng, 9, 64, 4), 2)                                            # 256 atoms: the last size a wave takes alone
    add("coil", X, mask, _radii(64, 4), 96)
    X, mask = _spoil(rng, _coils(rng, 3, 65, 4), 0)                                            # 260 atoms: eight waves a frame
    add("radii along the chain", X, mask, BACKBONE_R[None, :] * rng.uniform(0.6, 1.5, (65, 1)) + rng.uniform(0.0, 0.3, (65, 4)), 96, 0.3)
    add("helix", R.helix(30)[None], None, _radii(30, 4), 96)
    add("bpti", BACKBONES["bpti_xyz"][None], None, _radii(58, 4), 96)
    lattice = np.stack(np.meshgrid(*[np.arange(3.0)] * 3, indexing="ij"), -1).reshape(1, 27, 1, 3)
    add("lattice", lattice, None, np.array([0.5, 1.0, 1.5] * 9)[:, None], 96, 0.1)             # atoms touch exactly at d = R_i + R_j
    add("lattice of one radius", lattice + 0.3, None, np.full((27, 1), 1.0), 96, 0.1)
    add("coincident", np.tile([1.3, -2.7, 0.9], (2, 10, 4, 1)), None, np.full((10, 4), 3.27), 96)
    add("coincident", np.tile([11.3, -22.7, 30.9], (1, 65, 1, 1)), None, np.full((65, 1), 3.27), 65)
    X = _coils(rng, 2, 100, 1)
    X[:, 50] = X.mean(1)
    big = _radii(100, 1)
    big[50] = 1000.0
    add("one atom swallows the rest", X, None, big, 96)
    return out


# ---- 1. esmdiff_sasa_frames ------------------------------------------------------------------------------------------------------------
def test_frames_equal_the_restatement(cases):
    tests_made = 0
    for tag, X, mask, radii, u, thr, want in cases:
        got = _sasa(X, mask, radii, u, thr)
        _equal(got, want, tag, X.shape[0])
        assert not any(np.any(got[1][k] == SENTINEL[k]) for k in NAMES), f"{tag}: an element was not written"
        again = _sasa(X, mask, radii, u, thr)
        assert all(got[1][k].tobytes() == again[1][k].tobytes() for k in NAMES), f"{tag}: two runs"
        tests_made += int((want["count"] >= 0).sum()) * len(u)
    assert tests_made > 500_000                                          # the fixture is not a handful of points
    flags = np.concatenate([c[6]["exposed"].ravel() for c in cases])
    counts = np.concatenate([c[6]["count"].ravel() for c in cases])
    assert all((flags == v).any() for v in (0, 1, 2)) and (counts == -1).any() and (counts == 0).any()
    swallowed = cases[-1][6]["count"][:, :, 0]
    assert (swallowed[:, 50] == 96).all() and (np.delete(swallowed, 50, axis=1) == 0).all()    # the walk stops early on every other atom
    tag, coincident = cases[-3][0], cases[-3][6]["count"]
    assert 0 < coincident.min() == coincident.max() < 96, tag                                   # rounding decides, and decides alike


def test_areas_from_the_integers_equal_the_restatement(cases):
    from esmdiff_amd import accessibility as acc
    for tag, X, mask, radii, u, thr, want in cases:
        if X.shape[0] > 17:
            continue
        count = _sasa(X, mask, radii, u, thr)[1]["count"][:X.shape[0]]
        a = acc.Accessibility(count, radii, len(u), 1.4)
        for got, ref in zip((a.atom_area(), a.residue_area(), a.relative(), a.total()), R.areas(want["count"], radii, len(u))):
            assert got.tobytes() == ref.tobytes(), tag
        assert np.array_equal(a.exposed(thr), want["exposed"]), tag


def test_the_largest_frame():
    rng = np.random.default_rng(4096)
    X = R.coil(rng, 1024, 4)[None]
    X[0, 700, 2, 1] = np.nan
    u = R.sphere_points(8)
    _equal(_sasa(X, None, _radii(1024, 4), u), R.frames(X, None, _radii(1024, 4), u), "4096 atoms", 1)


def test_a_frame_does_not_see_its_batch(cases):
    for tag, X, mask, radii, u, thr, want in cases:
        if X.shape[0] < 5 or X.shape[0] > 17:
            continue
        for s in (0, 2, X.shape[0] - 1):
            alone = _sasa(X[s:s + 1], None if mask is None else mask[s:s + 1], radii, u, thr)[1]
            assert np.array_equal(alone["count"][0], want["count"][s]) and np.array_equal(alone["exposed"][0], want["exposed"][s]), (tag, s)


def test_garbage_in_masked_residues_is_never_read():
    rng = np.random.default_rng(5)
    X = _coils(rng, 6, 40, 4)
    mask = rng.random((6, 40)) > 0.25
    u, radii = R.sphere_points(96), _radii(40, 4)
    want = R.frames(X, mask, radii, u)
    for junk in (1e300, np.inf, -np.inf, np.nan):
        dirty = X.copy()
        dirty[~mask] = junk
        _equal(_sasa(dirty, mask, radii, u), want, f"masked coordinates set to {junk}", 6)
    dirty = X.copy()
    dirty[~mask] = rng.choice([np.nan, np.inf, 1e300, 0.0], size=dirty[~mask].shape)
    _equal(_sasa(dirty, mask, radii, u), want, "masked coordinates of every kind", 6)


def test_each_output_may_be_null(cases):
    tag, X, mask, radii, u, thr, want = next(c for c in cases if c[1].shape[:3] == (17, 12, 4))
    for name in NAMES:
        code, out = _sasa(X, mask, radii, u, thr, null=(name,))
        assert code == 0 and _untouched(out, (name,)), name
        for k in NAMES:
            if k != name:
                g = out[k][:17] if k in ("count", "exposed") else out[k]
                assert np.array_equal(g, want[k]), (name, k)
    code, out = _sasa(X, mask, radii, u, thr, null=NAMES)
    assert code == 0 and _untouched(out)


def test_capacity_and_invalid_calls_touch_nothing():
    rng = np.random.default_rng(1)
    X, u = _coils(rng, 3, 12, 4), R.sphere_points(96)
    radii = _radii(12, 4)
    got = _sasa(np.zeros((1, 4097, 1, 3)), None, np.ones((4097, 1)), u)
    assert got[0] == E_CAPACITY and _untouched(got[1])
    got = _sasa(np.zeros((1, 1025, 4, 3)), None, np.ones((1025, 4)), u)
    assert got[0] == E_CAPACITY and _untouched(got[1])
    got = _sasa(X, None, radii, np.zeros((1025, 3)))
    assert got[0] == E_CAPACITY and _untouched(got[1])
    for kw in ({"n": -1}, {"L": 0}, {"A": 2}, {"A": 0}, {"A": 5}, {"P": 0}, {"null": ("X",)}, {"null": ("radii",)}, {"null": ("points",)},
               {"threshold": np.nan}):
        got = _sasa(X, None, radii, u, **kw)
        assert got[0] == E_INVALID and _untouched(got[1]), kw
    assert _sasa(X, None, radii, u, np.nan, null=("exposed", "exposed_count", "present_count"))[0] == 0     # nobody reads the threshold
    code, out = _sasa(X, None, radii, u, n=0)                            # no frame: the ensemble outputs are zeroed, nothing else is touched
    assert code == 0 and _untouched(out, ("count", "exposed")) and not any(out[k].any() for k in ("sum_count", "valid", "exposed_count", "present_count"))


# ---- 2. esmdiff_cooccurrence -----------------------------------------------------------------------------------------------------------
def _cooccurrence(flags, null=(), short=0, **over):
    import torch
    from esmdiff_amd import _native as N
    n, L = flags.shape
    f = torch.as_tensor(np.ascontiguousarray(flags if n else np.zeros((1, L), np.uint8))).cuda()
    out = torch.full((3, L, L), -7, dtype=torch.int32, device="cuda")
    size = N.coocc_scratch_bytes(n, L)
    scratch = torch.full((max(size // 8, 1),), -1, dtype=torch.int64, device="cuda")                # need not be zeroed
    code = N.lib().esmdiff_cooccurrence(_p(None if "flags" in null else f), over.get("n", n), over.get("L", L), _p(None if "out" in null else out),
                                        _p(None if "scratch" in null else scratch), size - short, None)
    torch.cuda.synchronize()
    return code, out.cpu().numpy()


@pytest.mark.parametrize("L", [1, 2, 63, 64, 65, 130])
def test_cooccurrence_equals_the_restatement(L):
    rng = np.random.default_rng(L)
    for n in (0, 1, 63, 64, 65, 129, 1000):
        flags = rng.choice(np.array([0, 1, 2], np.uint8), size=(n, L), p=[0.5, 0.4, 0.1])
        if L > 1:
            flags[:, L // 2] = 2                                         # a residue that is never defined
        code, out = _cooccurrence(flags)
        want = R.cooccurrence(flags)
        assert code == 0 and out.dtype == want.dtype and np.array_equal(out, want), (n, L)
        assert _cooccurrence(flags)[1].tobytes() == out.tobytes(), (n, L)
        if L > 1 and n:
            assert not out[:, L // 2].any() and not out[:, :, L // 2].any() and out[0].trace() == (flags < 2).sum()


def test_cooccurrence_takes_any_other_value_as_undefined_and_checks_its_arguments():
    rng = np.random.default_rng(9)
    flags = rng.choice(np.array([0, 1, 2, 3, 255], np.uint8), size=(100, 7))
    assert np.array_equal(_cooccurrence(flags)[1], R.cooccurrence(np.where(flags > 1, 2, flags)))
    clean = lambda got: np.all(got[1] == -7)
    for kw in ({"n": -1}, {"L": 0}, {"null": ("flags",)}, {"null": ("out",)}, {"null": ("scratch",)}):
        got = _cooccurrence(flags, **kw)
        assert got[0] == E_INVALID and clean(got), kw
    got = _cooccurrence(flags, short=8)
    assert got[0] == E_CAPACITY and clean(got)
    got = _cooccurrence(flags, n=0, null=("scratch",))                  # no frame needs no scratch
    assert got[0] == 0 and not got[1].any()


# ---- 3. the Python layer and the command line ------------------------------------------------------------------------------------------
def test_python_layer(cases):
    from esmdiff_amd import accessibility as acc
    rng = np.random.default_rng(3)
    bpti = BACKBONES["bpti_xyz"]
    # A = 4, A = 3 (O inferred, the last residue's absent) and A = 1 (the caller's radius)
    full = acc.sasa(bpti)
    assert np.array_equal(full.counts, next(c for c in cases if c[0].startswith("bpti"))[6]["count"]) and full.points == 96
    three = acc.sasa(bpti[:, :3], points=64)
    X4 = acc.atom_array(bpti[:, :3])
    want = R.frames(X4, None, _radii(58, 4), R.sphere_points(64))
    assert np.array_equal(three.counts, want["count"]) and (three.counts[0, -1, 3] == -1) and (three.counts[0, :-1] >= 0).all()
    ca = np.stack([bpti[:, 1], bpti[:, 1] + 0.5 * rng.normal(size=(58, 3))])
    one = acc.sasa(ca, radii=2.5, probe=1.0, points=63)
    assert np.array_equal(one.counts, R.frames(ca[:, :, None, :], None, np.full((58, 1), 3.5), R.sphere_points(63))["count"])
    with pytest.raises(ValueError, match="no default radius"):
        acc.sasa(ca)
    with pytest.raises(RuntimeError, match="1025 x 4 atoms"):
        acc.sasa(np.zeros((1, 1025, 4, 3)))
    for got, ref in zip((full.atom_area(), full.residue_area(), full.relative(), full.total()), R.areas(full.counts, full.radii, 96)):
        assert got.tobytes() == ref.tobytes()
    assert 3000.0 < full.total()[0] < 12000.0 and 0.0 < np.nanmin(full.relative()) and np.nanmax(full.relative()) < 1.0

    # the fused reduction: no (n, L, A) array, the same integers
    tag, X, mask, radii, u, thr, want = next(c for c in cases if c[1].shape[:3] == (300, 12, 4))
    e = acc.exposure(X, thr, mask=mask, points=len(u), joint=True)
    assert e.n == 300 and all(np.array_equal(getattr(e, k), want[k]) for k in ("sum_count", "valid", "exposed_count", "present_count"))
    assert np.array_equal(e.joint(), R.cooccurrence(want["exposed"])) and np.array_equal(e.joint()[0].diagonal(), want["present_count"])
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.array_equal(e.frequency(), want["exposed_count"] / want["present_count"], equal_nan=True)
        mean = R.atom_area(radii, want["sum_count"] / want["valid"], len(u))
    assert np.array_equal(e.mean_atom_area(), np.where(want["valid"] > 0, mean, np.nan), equal_nan=True)
    assert np.array_equal(e.mean_residue_area(), R.residue_sum(np.where(want["valid"] > 0, mean, 0.0)))
    per_frame = acc.sasa(X, points=len(u), mask=mask)                     # the mean of the frames' areas, from the (n, L, A) counts
    assert np.array_equal(per_frame.counts, want["count"])
    assert np.allclose(e.mean_atom_area(), np.nanmean(per_frame.atom_area(), axis=0), rtol=1e-12, equal_nan=True)
    mi = e.mutual_information()
    assert mi.shape == (12, 12) and np.array_equal(mi, mi.T) and (mi >= 0).all() and (mi <= np.log(2.0) + 1e-12).all()
    with pytest.raises(AssertionError, match="joint=True"):
        acc.exposure(X[:3], points=8).joint()

    # ensembles against each other
    other = acc.exposure(X + 0.3 * rng.normal(size=X.shape), thr, mask=mask, points=len(u), joint=True)
    assert acc.exposed_jaccard(e, e) == 1.0 and 0.0 <= acc.exposed_jaccard(e, other) <= 1.0
    fa, fb = e.frequency() > 0.5, other.frequency() > 0.5
    assert acc.exposed_jaccard(e, other) == (fa & fb).sum() / (fa | fb).sum()
    assert acc.exposure_mi_correlation(e, e)["spearman"] == pytest.approx(1.0) and abs(acc.exposure_mi_correlation(e, other)["spearman"]) <= 1.0
    assert acc.js_sasa({"target": X[:50], "same": X[:50], "other": X[50:120] * 1.3}, points=24) == \
        {"same": 0.0, "other": acc.js_sasa({"target": X[:50], "other": X[50:120] * 1.3}, points=24)["other"], "target": 0.0}
    t1, t2 = bpti, BACKBONES["bpti_xyz"] * np.array([1.0, 1.0, 1.6])      # stretched along z: some residues open up
    sw = acc.exposure_switches(np.stack([t1, t2, t2]), t1, t2)
    e1, e2 = acc.sasa(t1).exposed()[0], acc.sasa(t2).exposed()[0]
    assert [s["residue"] for s in sw] == np.nonzero((e1 != e2) & (e1 != 2) & (e2 != 2))[0].tolist() and len(sw) > 0
    assert all(s["exposed"] == [bool(e1[s["residue"]]), bool(e2[s["residue"]])] and s["frequency"] in (1.0 / 3.0, 2.0 / 3.0) for s in sw)


def test_command_line(tmp_path):
    from esmdiff_amd import accessibility as acc
    from esmdiff_amd import analyze_ensemble, pdbio
    xyz, seq = BACKBONES["bpti_xyz"], str(BACKBONES["bpti_seq"])
    rng = np.random.default_rng(11)
    centred = xyz[:, :3] - xyz[:, 1].mean(0)
    files = []
    for i, sigma in enumerate((0.0, 0.05, 0.1, 0.2, 0.3, 0.1)):
        files.append(tmp_path / f"s_{i}.pdb")
        pdbio.write_backbone_pdb(files[-1], seq, centred + sigma * rng.normal(size=centred.shape))
    pdbio.merge_pdbfiles(files[:4], tmp_path / "ens.pdb", verbose=False)
    args = ["--samples", str(tmp_path / "ens.pdb"), "--targets", str(files[4]), str(files[5])]
    plain = analyze_ensemble.main(args + ["--output", str(tmp_path / "plain")])
    full = json.loads(analyze_ensemble.main(args + ["--output", str(tmp_path / "sasa"), "--sasa", "--sasa_points", "64", "--sasa_threshold", "0.1"]).read_text())
    block = full.pop("sasa")
    assert json.dumps(full, indent=1) + "\n" == plain.read_text()        # the other keys: the same bytes
    assert (block["points"], block["probe"], block["threshold"], block["radii"]) == (64, 1.4, 0.1, list(acc.DEFAULT_RADII)) and "unpinned" in block["parity"]
    backbones = pdbio.load_coords(tmp_path / "ens.pdb", max_n_model=None, ca_only=False, verbose=False)
    e, a = acc.exposure(backbones, 0.1, points=64), acc.sasa(backbones, points=64)
    assert np.array_equal(np.array(block["exposed_frequency"]), e.frequency()) and np.array_equal(np.array(block["residue_area"]), e.mean_residue_area())
    assert np.array_equal(np.array(block["relative"]), e.mean_relative()) and np.array_equal(np.array(block["total_area"]), a.total())
    assert block["summary"]["n"] == 4 and len(block["targets"]) == 2 and len(block["targets"][0]["relative"]) == 58
    t0 = acc.sasa(pdbio.load_coords(files[4], max_n_model=None, ca_only=False, verbose=False), points=64)
    assert block["targets"][0]["total_area"] == float(t0.total()[0]) and 0.0 <= block["targets"][0]["exposed_jaccard"] <= 1.0
    assert block["targets"][0]["exposed"] == [bool(v) for v in t0.exposed(0.1)[0] == 1]
    assert isinstance(block["exposure_switches"], list)

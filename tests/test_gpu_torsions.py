"""GPU tests of the torsion layer (esmdiff_amd/csrc/torsions.hip through the C ABI, esmdiff_amd/torsions.py and the command line)
against the numpy float64 restatement tests/torsions_ref.py (itself held to prescribed torsions and hand-worked cases by
tests/test_torsions_cpu.py).  Every output starts as a sentinel.
  angles          within 1e-12 rad: the arguments of atan2 are bit-equal by construction, the two atan2 differ by a few ulp of pi
  bond lengths    bit-equal;  the NaN pattern identical
  counts          exact;  hist exact against the host binning of the device's own angles on every input, and against the restatement
                  on the edge-free inputs (chains built from (phi, psi) at the centres of 5-degree cells +- 0.4 widths: 0.5 degrees
                  from every edge of 1, 36 and 72 bins; the test asserts 1e-6 degrees on the restatement's angles before it compares)
  sums            bit-equal to the restatement following the published order
Shapes: L = 1, 2, 3 (fewer residues than a torsion needs), 63, 64, 65, 130 around the wave width and past one workgroup of 256 threads,
5000 (no limit on L; with 210 frames the one shape here whose chunks hold more than 16 frames); n = 15, 16, 17, 33 on either side
of the chunk boundaries at F = 16 (one, one, two and three chunks)."""
import ctypes
import json
from pathlib import Path

import numpy as np
import pytest

from tests import torsions_ref as R

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = np.load(ROOT / "tests" / "golden" / "g14_backbones.npz")
SENTINEL_I, SENTINEL_F = -7, 1.0e30
E_INVALID, E_CAPACITY = -1, -5


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _dev(x, dt):
    import torch
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x, dtype=dt)).cuda()


def _torsions(X, mask=None, brk=R.BREAK, geometry=True, n=None, L=None, atoms=None, null=()):
    """esmdiff_backbone_torsions on numpy inputs -> (code, phi, psi, omega, geom); the outputs start as sentinels."""
    import torch
    from esmdiff_amd import _native as N
    x, mk = _dev(X, np.float64), _dev(mask, np.uint8)
    rows, width = max(X.shape[0], 1), X.shape[1]
    out = {k: torch.full((rows, width), SENTINEL_F, dtype=torch.float64, device="cuda") for k in ("phi", "psi", "omega")}
    out["geom"] = torch.full((rows, width, 6), SENTINEL_F, dtype=torch.float64, device="cuda") if geometry else None
    arg = {k: None if k in null else v for k, v in out.items()}
    code = N.lib().esmdiff_backbone_torsions(_p(None if "X" in null else x), X.shape[0] if n is None else n, width if L is None else L,
                                             X.shape[2] if atoms is None else atoms, _p(mk), float(brk), _p(arg["phi"]), _p(arg["psi"]),
                                             _p(arg["omega"]), _p(arg["geom"]), None)
    torch.cuda.synchronize()
    return (code, *[None if t is None else t.cpu().numpy() for t in out.values()])


def _rama(X, bins, mask=None, brk=R.BREAK, sums=True, scratch_bytes=None, n=None, L=None, atoms=None, null=()):
    """esmdiff_ramachandran on numpy inputs -> (code, hist, counts, sums); the outputs start as sentinels, the scratch as NaN."""
    import torch
    from esmdiff_amd import _native as N
    x, mk = _dev(X, np.float64), _dev(mask, np.uint8)
    nn, width = X.shape[:2]
    cells = max(min(bins, 80), 1)
    out = {"hist": torch.full((width, cells, cells), SENTINEL_I, dtype=torch.int32, device="cuda"),
           "counts": torch.full((width, 5), SENTINEL_I, dtype=torch.int32, device="cuda"),
           "sums": torch.full((width, 6), SENTINEL_F, dtype=torch.float64, device="cuda") if sums else None}
    size = N.rama_scratch_bytes(nn, width) if scratch_bytes is None else scratch_bytes
    scratch = torch.full((size // 8,), float("nan"), dtype=torch.float64, device="cuda") if size else None
    arg = {k: None if k in null else v for k, v in out.items()}
    code = N.lib().esmdiff_ramachandran(_p(None if "X" in null else x), nn if n is None else n, width if L is None else L,
                                        X.shape[2] if atoms is None else atoms, _p(mk), float(brk), bins, _p(arg["hist"]),
                                        _p(arg["counts"]), _p(arg["sums"]), _p(scratch), size, None)
    torch.cuda.synchronize()
    return (code, *[None if t is None else t.cpu().numpy() for t in out.values()])


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _rotate_tail(x, i):
    """Turn everything after N of residue i + 1 by 180 degrees about the axis C_i -> N_{i+1}: the peptide i -> i + 1 becomes cis, every
    other torsion, length and angle stays."""
    origin = x[i + 1, 0].copy()
    axis = origin - x[i, 2]
    axis /= np.linalg.norm(axis)
    flat = x.reshape(-1, 3)
    first = (i + 1) * x.shape[1] + 1                                 # CA of residue i + 1
    v = flat[first:] - origin
    flat[first:] = origin + 2.0 * np.outer(v @ axis, axis) - v       # a half turn: v -> 2 (v . a) a - v


def _break_after(x, i, length=3.0):
    """Move residues i + 1 .. along C_i -> N_{i+1} until that bond is `length` long."""
    d = x[i + 1, 0] - x[i, 2]
    x[i + 1:] += d / np.linalg.norm(d) * (length - np.linalg.norm(d))


def _spoil(rng, X, k):
    """The mask patterns, one per structure in turn (structure s gets pattern (k + s) % 5): untouched; a masked residue; a NaN atom;
    a chain break at 3.0 Angstrom and a cis peptide; the first and the last residue masked."""
    n, L = X.shape[:2]
    mask = np.ones((n, L), bool)
    for s in range(n):
        kind = (k + s) % 5
        if kind == 1:
            mask[s, rng.integers(0, L)] = False
        elif kind == 2:
            X[s, rng.integers(0, L), rng.integers(0, 3), rng.integers(0, 3)] = np.nan
        elif kind == 3 and L >= 4:
            _break_after(X[s], rng.integers(0, L - 1))
            _rotate_tail(X[s], rng.integers(0, L - 1))
        elif kind == 4:
            mask[s, 0] = mask[s, -1] = False
    return X, (None if mask.all() else mask)


def _edge_free(X, mask, bins):
    """The condition of the exact histogram comparison, on the restatement's angles: none within 1e-6 degrees of a bin edge."""
    phi, psi, _ = R.torsions(X, mask)
    a = np.concatenate([phi[np.isfinite(phi)], psi[np.isfinite(psi)]]) * R.DEG
    if a.size == 0:
        return True
    t = (a + 180.0) / (360.0 / bins)
    return bool((np.abs(t - np.round(t)) * (360.0 / bins)).min() > 1e-6)


@pytest.fixture(scope="module")
def cases():
    """[(tag, X, mask)] for entry 1: every L with n = 1, 2, 7 in turn, atoms 3 and 4 in turn, every mask pattern."""
    rng = np.random.default_rng(20261020)
    out, k = [], 0
    for L in (1, 2, 3, 63, 64, 65, 130):
        for n in (1, 2, 7):
            atoms = 3 + k % 2
            X, _ = R.chains(rng, n, L, atoms, bins=72)
            X, mask = _spoil(rng, X, k)
            out.append((f"L={L} n={n} atoms={atoms} k={k}", X, mask))
            k += 1
    return out


@pytest.fixture(scope="module")
def mixed():
    """33 frames of 65 residues: helix, strand, and per frame in turn a cis peptide, a break, a masked residue, a NaN atom."""
    rng = np.random.default_rng(7)
    pp = np.array([(-57.0, -47.0)] * 30 + [(-120.0, 130.0)] * 35)
    X = np.stack([R.nerf([tuple(a) for a in pp + rng.uniform(-2.0, 2.0, pp.shape)]) for _ in range(33)])
    mask = np.ones((33, 65), bool)
    for s in range(33):
        if s % 4 == 0:
            _rotate_tail(X[s], 10 + s % 7)
        if s % 4 == 1:
            _break_after(X[s], 40)
        if s % 4 == 2:
            mask[s, 20 + s % 5] = False
        if s % 8 == 3:
            X[s, 50, 1, 2] = np.nan
    return np.ascontiguousarray(X), mask


@pytest.fixture(scope="module")
def long_chains():
    """210 noisy copies of a chain of 5000 residues: cap = 13 chunks, F = 17 frames each."""
    rng = np.random.default_rng(8)
    base = R.chains(rng, 1, 5000, 3, bins=72)[0][0]
    X = base[None] + 0.02 * rng.normal(size=(210,) + base.shape)
    X[3, 2500, 1, 0] = np.nan
    return X


def _check_entry1(got, want, tag):
    assert got[0] == 0, tag
    for name, g, w in zip(("phi", "psi", "omega"), got[1:4], want[:3]):
        assert np.array_equal(np.isnan(g), np.isnan(w)), f"{tag}: NaN pattern of {name}"
        ok = ~np.isnan(w)
        worst = np.abs(g[ok] - w[ok]).max(initial=0.0)
        assert worst <= 1e-12, f"{tag}: {name} off by {worst}"
    g, w = got[4], want[3]
    assert np.array_equal(np.isnan(g), np.isnan(w)), f"{tag}: NaN pattern of geom"
    assert np.array_equal(_bits(np.nan_to_num(g[:, :, :3])), _bits(np.nan_to_num(w[:, :, :3]))), f"{tag}: bond lengths"
    ok = ~np.isnan(w[:, :, 3:])
    assert np.abs(g[:, :, 3:][ok] - w[:, :, 3:][ok]).max(initial=0.0) <= 1e-12, f"{tag}: bond angles"


# ---- 1. esmdiff_backbone_torsions ------------------------------------------------------------------------------------------------------
def test_torsions_equal_the_restatement(cases):
    seen = 0
    for tag, X, mask in cases:
        got = _torsions(X, mask)
        _check_entry1(got, R.torsions(X, mask, geometry=True), tag)
        assert not np.any(got[1] == SENTINEL_F) and not np.any(got[4] == SENTINEL_F), tag      # every element is written
        seen += int(np.isfinite(got[1]).sum())
        alone = _torsions(X, mask, geometry=False)
        assert alone[4] is None and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(alone[1:4], got[1:4])), tag
    assert seen > 1500


def test_break_distance_is_an_argument(cases):
    tag, X, mask = next(c for c in cases if c[1].shape[:2] == (7, 65))
    for brk in (1.0, 1.329, 3.0, np.nextafter(3.0, 4.0)):
        _check_entry1(_torsions(X, mask, brk), R.torsions(X, mask, brk, geometry=True), f"{tag} break {brk}")
    defined = [int(np.isfinite(_torsions(X, mask, brk)[3]).sum()) for brk in (2.5, 2.9, 3.1)]
    assert defined[0] == defined[1] < defined[2]                     # the structures broken at 3.0 Angstrom link again
    assert np.isnan(_torsions(X, mask, 1.0)[1]).all()


def test_garbage_in_masked_residues_changes_nothing(cases):
    rng = np.random.default_rng(5)
    tag, X, _ = next(c for c in cases if c[1].shape[:2] == (7, 130))
    X = np.nan_to_num(X, nan=1.0)
    mask = rng.random(X.shape[:2]) > 0.2
    clean = _torsions(X, mask)
    dirty = X.copy()
    dirty[~mask] = rng.choice([np.nan, np.inf, -np.inf, 1e300, 0.0], size=dirty[~mask].shape)
    for a, b in zip(clean[1:], _torsions(dirty, mask)[1:]):
        assert np.array_equal(_bits(a), _bits(b))
    r1, r2 = _rama(X, 36, mask), _rama(dirty, 36, mask)
    assert r1[0] == r2[0] == 0 and all(np.array_equal(_bits(a) if a.dtype == np.float64 else a, _bits(b) if b.dtype == np.float64 else b)
                                       for a, b in zip(r1[1:], r2[1:]))


def test_a_structure_does_not_see_its_batch(cases):
    for tag, X, mask in cases:
        if X.shape[0] != 7:
            continue
        batch = _torsions(X, mask)
        for s in (0, 3, 6):
            alone = _torsions(X[s:s + 1], None if mask is None else mask[s:s + 1])
            assert all(np.array_equal(_bits(a[0]), _bits(b[s])) for a, b in zip(alone[1:], batch[1:])), (tag, s)


def test_no_length_limit(long_chains):
    X = long_chains[:2]
    _check_entry1(_torsions(X), R.torsions(X, geometry=True), "L=5000")


def test_invalid_calls_touch_nothing_and_an_empty_batch_succeeds(cases):
    X = cases[-1][1]
    untouched = lambda got: all(np.all(a == (SENTINEL_I if a.dtype == np.int32 else SENTINEL_F)) for a in got[1:] if a is not None)
    for kw in ({"n": -1}, {"L": 0}, {"atoms": 2}, {"atoms": 5}, {"brk": 0.0}, {"brk": -2.5}, {"brk": np.inf}, {"brk": np.nan},
               {"null": ("X",)}, {"null": ("phi",)}, {"null": ("omega",)}):
        got = _torsions(X, **kw)
        assert got[0] == E_INVALID and untouched(got), kw
    got = _torsions(X, n=0)
    assert got[0] == 0 and untouched(got)
    for kw in ({"n": -1}, {"L": 0}, {"atoms": 2}, {"brk": 0.0}, {"brk": np.nan}, {"null": ("X",)}, {"null": ("hist",)}, {"null": ("counts",)}):
        got = _rama(X, 36, **kw)
        assert got[0] == E_INVALID and untouched(got), kw
    for bins, code in ((0, E_INVALID), (-3, E_INVALID), (73, E_CAPACITY), (80, E_CAPACITY)):
        got = _rama(X, bins)
        assert got[0] == code and untouched(got), bins
    got = _rama(X, 36, n=0)                                           # no frame: every output is zero
    assert got[0] == 0 and not got[1].any() and not got[2].any() and not got[3].any()


# ---- 2. esmdiff_ramachandran ------------------------------------------------------------------------------------------------------------
def _check_entry2(X, mask, bins, tag, want=None, sums=True, edge_free=True):
    got = _rama(X, bins, mask, sums=sums)
    assert got[0] == 0, tag
    want = R.ramachandran(X, bins, mask, sums=sums) if want is None else want
    assert np.array_equal(got[2], want[1]), f"{tag}: counts"
    dev = _torsions(X, mask, geometry=False)
    assert np.array_equal(got[1], R.histogram(dev[1], dev[2], bins)), f"{tag}: hist against the device's own angles"
    assert got[1].sum() == want[1][:, 2].sum()
    if edge_free:
        assert _edge_free(X, mask, bins), f"{tag}: an angle within 1e-6 degrees of an edge"
        assert np.array_equal(got[1], want[0]), f"{tag}: hist against the restatement"
    if sums:
        assert np.array_equal(_bits(got[3]), _bits(want[2])), f"{tag}: sums"
    else:
        assert got[3] is None
    return got


@pytest.mark.parametrize("L", [1, 2, 65, 130])
def test_maps_equal_the_restatement_at_the_chunk_boundaries(L):
    from esmdiff_amd import _native as N
    rng = np.random.default_rng(100 + L)
    X33, _ = R.chains(rng, 33, L, 3 + L % 2, bins=72)
    X33, mask33 = _spoil(rng, X33, L)
    F = N.rama_chunk_frames(33, L)
    assert F == 16
    for k, n in enumerate((F - 1, F, F + 1, 2 * F + 1)):
        X, mask = X33[:n], None if mask33 is None else mask33[:n]
        assert N.rama_chunks(n, L) == (1, 1, 2, 3)[k] and N.rama_chunk_frames(n, L) == F
        bins = (36, 72, 1, 36)[k]
        got = _check_entry2(X, mask, bins, f"L={L} n={n} bins={bins}")
        _check_entry2(X, mask, bins, f"L={L} n={n} bins={bins} no sums", sums=False)
        if k < 2:                                                        # one chunk: the scratch is not looked at
            again = _rama(X, bins, mask, scratch_bytes=0)
            assert again[0] == 0 and np.array_equal(_bits(again[3]), _bits(got[3])) and np.array_equal(again[1], got[1])
        else:                                                            # several: a scratch one byte short is refused, nothing is written
            need = N.rama_scratch_bytes(n, L)
            assert need == N.rama_chunks(n, L) * L * 48
            short = _rama(X, bins, mask, scratch_bytes=need - 8)
            assert short[0] == E_CAPACITY and np.all(short[1] == SENTINEL_I) and np.all(short[3] == SENTINEL_F)
            assert _rama(X, bins, mask, sums=False, scratch_bytes=0)[0] == 0          # without sums no scratch is needed


def test_mixed_ensemble_and_two_runs(mixed):
    X, mask = mixed
    want = R.ramachandran(X, 36, mask)
    assert want[1][:, 4].sum() == 9 and 0 < want[1][40, 3] < 33 and want[1][22, 2] < 33            # cis, the break, a masked residue
    a = _check_entry2(X, mask, 36, "mixed", want)
    b = _rama(X, 36, mask)
    for u, v in zip(a[1:], b[1:]):
        assert u.tobytes() == v.tobytes()
    _check_entry2(X, mask, 72, "mixed 72", edge_free=False)
    _check_entry2(X, mask, 1, "mixed 1", edge_free=False)


def test_chunks_longer_than_sixteen_frames(long_chains):
    from esmdiff_amd import _native as N
    X = long_chains
    assert N.rama_chunk_frames(210, 5000) == 17 and N.rama_chunks(210, 5000) == 13
    _check_entry2(X, None, 36, "210 x 5000", edge_free=False)


# ---- 3. the Python layer and the command line ------------------------------------------------------------------------------------------
def test_python_layer_and_command_line(tmp_path):
    from scipy.spatial.distance import jensenshannon
    from esmdiff_amd import analyze_ensemble, pdbio
    from esmdiff_amd import torsions as T
    xyz, seq = GOLDEN["bpti_xyz"], str(GOLDEN["bpti_seq"])
    t = T.torsions(xyz, geometry=True)
    ref = R.torsions(xyz[None], geometry=True)
    assert t.phi.shape == (1, 58) and t.present.all() and np.nanmax(np.abs(t.phi - ref[0] * R.DEG)) < 1e-10
    assert np.array_equal(_bits(np.nan_to_num(t.bond_lengths)), _bits(np.nan_to_num(ref[3][:, :, :3])))
    assert np.array_equal(np.isnan(t.psi), np.isnan(ref[1])) and np.isnan(t.phi[0, 0]) and np.isnan(t.psi[0, -1])
    rad = T.torsions(xyz, degrees=False)
    assert np.nanmax(np.abs(rad.omega - ref[2])) <= 1e-12 and np.array_equal(rad.cis(), np.abs(ref[2]) < np.pi / 2)
    rng = np.random.default_rng(11)
    centred = xyz[:, :3] - xyz[:, 1].mean(0)
    files = []
    for i, sigma in enumerate((0.0, 0.05, 0.1, 0.2, 0.3, 0.1)):
        files.append(tmp_path / f"s_{i}.pdb")
        pdbio.write_backbone_pdb(files[-1], seq, centred + sigma * rng.normal(size=centred.shape))
    pdbio.merge_pdbfiles(files[:4], tmp_path / "ens.pdb", verbose=False)
    bb = pdbio.load_coords(tmp_path / "ens.pdb", max_n_model=None, ca_only=False, verbose=False).astype(np.float64)
    m = T.ramachandran(tmp_path / "ens.pdb")
    want = R.ramachandran(bb, 36)
    dev = T.torsions(tmp_path / "ens.pdb", degrees=False)
    assert m.n_frames == 4 and m.bins == 36 and np.array_equal(m.counts, want[1]) and np.array_equal(_bits(m.sums), _bits(want[2]))
    assert np.array_equal(m.hist, R.histogram(dev.phi, dev.psi, 36))
    masked = T.ramachandran(bb, mask=np.arange(58) != 20)
    assert masked.counts[20].tolist() == [0] * 5 and masked.counts[19, 1] == 0 and masked.counts[21, 0] == 0
    assert np.isnan(masked.density()[20]).all() and np.isnan(masked.entropy()[20]) and np.isnan(masked.circular_mean()[20]).all()
    assert np.allclose(m.density().sum((1, 2))[1:-1], 1.0) and (m.circular_variance()[1:-1] >= -1e-15).all()
    assert abs(m.circular_mean()[5, 2]) > 150.0 and m.cis_fraction()[:-1].max() == 0.0

    # js_ramachandran: 0 against itself, scipy's value from the same histograms against a shifted ensemble
    helix = np.stack([R.nerf([(-57.0 + d, -47.0 - d)] * 12)[:, :3] for d in (-6.0, -2.0, 2.0, 6.0)])
    shifted = np.stack([R.nerf([(-67.0 + d, -37.0 - d)] * 12)[:, :3] for d in (-6.0, -2.0, 2.0, 6.0)])
    assert T.js_ramachandran({"target": helix, "same": helix}) == {"same": 0.0, "target": 0.0}
    res, rows = T.js_ramachandran({"target": helix, "shifted": shifted}, rounded=False, per_residue=True)
    ha, hb = T.ramachandran(shifted).hist, T.ramachandran(helix).hist
    js = [jensenshannon(ha[i].ravel() + 1e-6, hb[i].ravel() + 1e-6) for i in range(1, 11)]
    assert np.abs(rows["shifted"][1:11] - js).max() < 1e-15 and np.isnan(rows["shifted"][[0, 11]]).all()
    assert abs(res["shifted"] - np.mean(js)) < 1e-15 and res["shifted"] > 0.1 and res["target"] == 0.0
    assert T.js_ramachandran({"target": helix, "shifted": shifted})["shifted"] == round(res["shifted"], 4)
    # an all-alpha chain is 1 in alpha; the strand is beta; agreement and switches
    hm = T.ramachandran(helix)
    assert np.array_equal(hm.region_propensity()[1:11], np.tile([1.0, 0, 0, 0, 0], (10, 1))) and np.isnan(hm.region_propensity()[0]).all()
    strand = R.nerf([(-120.0, 130.0)] * 12)[:, :3]
    assert T.region_string(T.torsions(strand))[0] == "-" + "B" * 10 + "-" and T.region_string(T.torsions(helix))[0] == "-" + "A" * 10 + "-"
    agree = T.torsion_agreement(helix, helix[1], tolerance=5.0)          # phi and psi are 4, 0, 4 and 8 degrees from the target's
    assert agree["share"].tolist() == [1.0, 1.0, 1.0, 0.0] and agree["best_model"] == 0 and agree["share_mean"] == 0.75
    assert agree["per_residue"][1:11].tolist() == [0.75] * 10 and np.isnan(agree["per_residue"][0])
    assert T.torsion_agreement(helix, helix[1], tolerance=3.0)["share"].tolist() == [0.0, 1.0, 0.0, 0.0]
    assert T.torsion_agreement(helix, strand)["share_best"] == 0.0
    sw = T.region_switches(helix, helix[0], strand)
    assert [s["residue"] for s in sw] == list(range(1, 11)) and sw[0] == {"residue": 1, "regions": ["alpha", "beta"], "share": [1.0, 0.0]}
    geo = T.geometry_summary(helix)
    assert abs(geo["n_ca"]["mean"] - 1.458) < 1e-9 and abs(geo["c_n_ca"]["max"] - 121.7) < 1e-9 and geo["c_n"]["n"] == 44
    assert geo["cis_fraction"] == 0.0 and geo["outliers"].tolist() == [0] * 4 and geo["share_without_outliers"] == 1.0
    with pytest.raises(RuntimeError, match="bins = 73"):
        T.ramachandran(helix, bins=73)

    args = ["--samples", str(tmp_path / "ens.pdb"), "--targets", str(files[4]), str(files[5])]
    plain = analyze_ensemble.main(args + ["--output", str(tmp_path / "plain")])
    full = json.loads(analyze_ensemble.main(args + ["--output", str(tmp_path / "tors"), "--torsions", "--rama_bins", "36"]).read_text())
    assert "torsions" not in json.loads(plain.read_text())
    assert json.dumps({k: v for k, v in full.items() if k != "torsions"}, indent=1) + "\n" == plain.read_text()   # the other keys: the same bytes
    block = full["torsions"]
    assert block["bins"] == 36 and block["break_distance"] == 2.5 and block["n_frames"] == 4 and block["counts"] == want[1].tolist()
    assert np.array_equal(np.array(block["region_propensity"], float), m.region_propensity(), equal_nan=True)
    assert np.array_equal(np.array(block["circular_mean"], float), m.circular_mean(), equal_nan=True)
    assert len(block["targets"]) == 2 and len(block["targets"][0]["regions"]) == 58 and len(block["targets"][0]["agreement"]["share"]) == 4
    assert block["js_ramachandran"]["n_targets"] == 2 and 0.0 < block["js_ramachandran"]["mean"] < 1.0
    assert set(block["geometry"]) >= set(T.QUANTITIES) and "region_switches" in block and len(block["entropy"]) == 58

"""GPU tests of the secondary-structure layer (esmdiff_amd/csrc/dssp.hip through the C ABI, esmdiff_amd/secondary.py and the two
command lines) against the numpy float64 restatement tests/dssp_ref.py (itself held to pinned strings and to a second restatement by
tests/test_dssp_cpu.py).  Every output starts as a sentinel and every comparison is exact: codes, acceptors and counts with
np.array_equal, the energies on their bit patterns.  No tolerance anywhere.
Shapes: L = 1 .. 7 (below the shortest helix or bridge), 63, 64, 65, 130 around the wave width (a wave's lanes take acceptors 64 at a
time), 1096 (a chain of about 1 100 residues), and 2048 / 2049 / 2165 on either side of the hbond kernel's one staging boundary
(DSSP_TILE = 2048 acceptors in LDS at a time; at 2165 hydrogen bonds cross residue 2048 in both directions)."""
import ctypes
import json
from pathlib import Path

import numpy as np
import pytest

from tests import dssp_ref as R

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = np.load(ROOT / "tests" / "golden" / "g14_backbones.npz")
SENTINEL_I, SENTINEL_B, SENTINEL_E = -7, 0xEE, 1.0e30
NOISE = (0.0, 0.1, 0.3, 0.6, 1.0)
TILE = 2048                                  # csrc/dssp.hip: DSSP_TILE


def _chain(name):
    seq = str(GOLDEN[f"{name}_seq"])
    return GOLDEN[f"{name}_xyz"], np.array([c == "P" for c in seq], np.uint8)


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _call(X, mask=None, no_donor=None, n=None, L=None, want_counts=True, null=()):
    """esmdiff_dssp on numpy inputs -> (code, ss, counts, acceptor, energy); the outputs start as sentinels."""
    import torch
    from esmdiff_amd import _native as N
    dev = lambda x, dt: None if x is None else torch.as_tensor(np.ascontiguousarray(x, dtype=dt)).cuda()
    x, mk, nd = dev(X, np.float64), dev(mask, np.uint8), dev(no_donor, np.uint8)
    rows, width = max(X.shape[0], 1), X.shape[1]
    n = X.shape[0] if n is None else n
    L = X.shape[1] if L is None else L
    out = {"ss": torch.full((rows, width), SENTINEL_B, dtype=torch.uint8, device="cuda"),
           "counts": torch.full((width, 8), SENTINEL_I, dtype=torch.int32, device="cuda") if want_counts else None,
           "acceptor": torch.full((rows, width, 2), SENTINEL_I, dtype=torch.int32, device="cuda"),
           "energy": torch.full((rows, width, 2), SENTINEL_E, dtype=torch.float64, device="cuda")}
    arg = {k: None if k in null else v for k, v in out.items()}
    code = N.lib().esmdiff_dssp(_p(None if "X" in null else x), n, L, _p(mk), _p(nd), _p(arg["ss"]), _p(arg["counts"]),
                                _p(arg["acceptor"]), _p(arg["energy"]), None)
    torch.cuda.synchronize()
    return (code, *[None if t is None else t.cpu().numpy() for t in out.values()])


def _exact(got, want, tag):
    assert got[0] == 0, tag
    for name, g, w in zip(("ss", "counts", "acceptor"), got[1:4], want[:3]):
        if g is not None:
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), f"{tag}: {name}"
    assert got[4].shape == want[3].shape and np.array_equal(got[4].view(np.int64), want[3].view(np.int64)), f"{tag}: energy"


def _untouched(got):
    return (np.all(got[1] == SENTINEL_B) and np.all(got[2] == SENTINEL_I) and np.all(got[3] == SENTINEL_I) and np.all(got[4] == SENTINEL_E))


def _case(rng, base, no_donor, n, k):
    """A batch of n noisy copies (structure s at NOISE[(k + s) % 5]); every second case masked (20 % off), every third with NaN atoms
    (an absent residue, a missing O in the chain, a missing last O — what the inferred O leaves), every second with proline flags."""
    L = len(base)
    X = np.stack([base + NOISE[(k + s) % 5] * rng.normal(size=base.shape) for s in range(n)])
    mask = (rng.random((n, L)) > 0.2) if k % 2 else None
    if k % 3 == 0:
        X[:, -1, 3] = np.nan
        if L > 4:
            X[0, L // 2, rng.integers(0, 3)] = np.nan
            X[-1, L // 3, 3] = np.nan
    return X, mask, (no_donor if k % 4 < 2 else None)


@pytest.fixture(scope="module")
def cases():
    """[(tag, X, mask, no_donor, reference outputs with details)], computed once."""
    rng = np.random.default_rng(20261019)
    out, k = [], 0
    sources = {"1fmf_A": _chain("1fmf_A"), "1c54_A": _chain("1c54_A")}
    for L in (1, 2, 3, 4, 5, 6, 7, 63, 64, 65, 130):
        for name, (xyz, nd) in sources.items():
            if L > len(xyz):
                continue
            lo = (k * 11) % (len(xyz) - L + 1)
            out.append((f"{name}[{lo}:{lo + L}] case {k}", *_case(rng, xyz[lo:lo + L], nd[lo:lo + L], (1, 3, 9)[k % 3], k)))
            k += 1
    for name in ("1fmf_A", "1c54_A", "bpti"):                    # the whole chains, nine copies: every noise level, the two highest twice
        xyz, nd = _chain(name)
        out.append((f"{name} x 9", *_case(rng, xyz, nd, 9, 5 if name == "bpti" else 7)))
    for name, pp in (("alpha", [R.ALPHA] * 16), ("3-10", [R.HELIX310] * 16), ("pi", [R.PI] * 16), ("beta", [R.BETA] * 16), ("mixed", R.MIXED)):
        x = R.nerf(pp)
        out.append((f"synthetic {name}", x[None], None, None))
        out.append((f"synthetic {name} x 3 noisy", *_case(rng, x, None, 3, 1)))
    z = R.nerf([R.ALPHA] * 16)                                   # a hand-placed pair 0.3 A apart: the energy floor
    z[5, 3] = z[9, 0] + np.array([0.3, 0.0, 0.0])
    out.append(("hand-placed close pair", z[None], None, None))
    return [(tag, X, mask, nd, R.dssp(X, mask, nd, details=True)) for tag, X, mask, nd in out]


# ---- 1. shapes and census --------------------------------------------------------------------------------------------------------
def test_census_of_the_input_set(cases):
    """What the inputs exercise, asserted on the restatement's own outputs."""
    codes, par, anti, most, clamped = set(), 0, 0, 0, 0
    lengths, batches = set(), set()
    for tag, X, mask, nd, ref in cases:
        codes |= set(ref[0].reshape(-1).tolist())
        lengths.add(X.shape[1])
        batches.add(X.shape[0])
        for info in ref[4]:
            par, anti = par + info["parallel"], anti + info["antiparallel"]
            most, clamped = max(most, int(info["candidates"].max(initial=0))), clamped + info["clamped"]
    assert codes == set(range(8)), sorted(codes)
    assert par > 0 and anti > 0
    assert most >= 3, "no donor with three acceptors under -0.5: the two-best rule drops nothing"
    assert clamped >= 1, "the -9.9 floor never fires"
    assert lengths >= {1, 2, 3, 4, 5, 6, 7, 63, 64, 65, 130} and batches >= {1, 3, 9}


def test_outputs_equal_the_restatement(cases):
    for tag, X, mask, nd, ref in cases:
        _exact(_call(X, mask, nd), ref, tag)


def test_counts_may_be_null(cases):
    tag, X, mask, nd, ref = next(c for c in cases if c[0] == "synthetic mixed x 3 noisy")
    got = _call(X, mask, nd, want_counts=False)
    assert got[2] is None
    _exact(got, ref, tag)


# ---- 2. chain breaks, long chains, invalid calls -----------------------------------------------------------------------------------
def test_chain_break():
    xyz, nd = _chain("bpti")
    two = np.concatenate([xyz, xyz + 100.0])
    ref = R.dssp(two, no_donor=np.tile(nd, 2))
    got = _call(two[None], None, np.tile(nd, 2))
    _exact(got, ref, "two copies of bpti")
    one = R.string(R.dssp(xyz, no_donor=nd)[0][0])
    assert R.string(got[1][0]) == one + one                      # no hydrogen bond, turn, bridge or bend spans the break
    assert np.all(got[3][0, 58] == -1) and np.all((got[3][0, 58:] >= 58) | (got[3][0, 58:] == -1)) and np.all(got[3][0, :58] < 58)


@pytest.fixture(scope="module")
def long_chain():
    """16 copies of 1fmf.A side by side without the first 27 residues, 0.3 A noise: 2165 residues.  Residue 2048 is residue 20 of the
    last copy, between its first two strands, which pair in the parallel sheet."""
    xyz, nd = _chain("1fmf_A")
    rng = np.random.default_rng(7)
    big = np.concatenate([xyz + np.array([0.0, 0.0, 60.0 * k]) for k in range(16)])[27:]
    return big + 0.3 * rng.normal(size=big.shape), np.tile(nd, 16)[27:]


@pytest.mark.parametrize("L", [1096, TILE, TILE + 1, 2165])
def test_long_chains(long_chain, L):
    big, nd = long_chain
    X = big[None, :L]
    ref = R.dssp(X, None, nd[:L])
    if L == len(big):                                            # a condition on the inputs: hydrogen bonds cross the staging boundary both ways
        acc = ref[2][0]
        assert np.any((acc[TILE:] >= 0) & (acc[TILE:] < TILE)) and np.any(acc[:TILE] >= TILE)
        assert R.E in ref[0][0, TILE - 20:TILE] and R.E in ref[0][0, TILE:TILE + 20]
    _exact(_call(X, None, nd[:L]), ref, f"L = {L}")


def test_invalid_calls_touch_nothing_and_an_empty_batch_zeroes_the_counts():
    from esmdiff_amd import _native as N
    x = R.nerf([R.ALPHA] * 8)[None]
    for kw in ({"L": N.DSSP_MAX_L + 1}, {"L": 0}, {"n": -1}, {"null": ("ss",)}, {"null": ("acceptor",)}, {"null": ("energy",)},
               {"null": ("X",)}):
        got = _call(x, **kw)
        assert got[0] == -1 and _untouched(got), kw              # ESMDIFF_E_INVALID
    got = _call(x, n=0)
    assert got[0] == 0 and np.all(got[2] == 0)
    assert np.all(got[1] == SENTINEL_B) and np.all(got[3] == SENTINEL_I) and np.all(got[4] == SENTINEL_E)


# ---- 3. masked residues --------------------------------------------------------------------------------------------------------------
def test_garbage_in_masked_residues_changes_nothing():
    xyz, nd = _chain("1c54_A")
    rng = np.random.default_rng(3)
    X = xyz[None] + 0.3 * rng.normal(size=(3,) + xyz.shape)
    mask = rng.random((3, 96)) > 0.2
    clean = _call(X, mask, nd)
    _exact(clean, R.dssp(X, mask, nd), "clean")
    for garbage in (1e300, np.nan, -1e300, 0.0):
        Y = X.copy()
        Y[~mask] = garbage
        got = _call(Y, mask, nd)
        for a, b in zip(got[1:4], clean[1:4]):
            assert np.array_equal(a, b), garbage
        assert np.array_equal(got[4].view(np.int64), clean[4].view(np.int64)), garbage
    assert np.all(clean[1][~mask] == 0) and np.array_equal(clean[2].sum(1), mask.sum(0))


# ---- 4. determinism -----------------------------------------------------------------------------------------------------------------
def test_two_runs_are_identical_and_a_structure_does_not_see_its_batch(cases):
    tag, X, mask, nd, ref = next(c for c in cases if c[0] == "1fmf_A x 9")
    first, again = _call(X, mask, nd), _call(X, mask, nd)
    for a, b in zip(first[1:4], again[1:4]):
        assert np.array_equal(a, b)
    assert np.array_equal(first[4].view(np.int64), again[4].view(np.int64))
    for s in (0, 4, 8):
        alone = _call(X[s:s + 1], None if mask is None else mask[s:s + 1], nd)
        assert np.array_equal(alone[1][0], first[1][s]) and np.array_equal(alone[3][0], first[3][s])
        assert np.array_equal(alone[4][0].view(np.int64), first[4][s].view(np.int64))


# ---- 5. end to end -----------------------------------------------------------------------------------------------------------------
def test_python_layer_and_command_lines(tmp_path):
    from esmdiff_amd import analyze_ensemble, pdbio, secondary, secondary_structure
    xyz, nd = _chain("bpti")
    seq = str(GOLDEN["bpti_seq"])
    rng = np.random.default_rng(11)
    centred = xyz[:, :3] - xyz[:, 1].mean(0)
    files = []
    for i, sigma in enumerate((0.0, 0.1, 0.3, 0.6, 1.0, 0.3)):
        files.append(tmp_path / f"s_{i}.pdb")
        pdbio.write_backbone_pdb(files[-1], seq, centred + sigma * rng.normal(size=centred.shape))
    pdbio.merge_pdbfiles(files[:4], tmp_path / "ens.pdb", verbose=False)

    def restated(path):
        bb = pdbio.load_coords(path, max_n_model=None, ca_only=False, verbose=False).astype(np.float64)
        return R.dssp(np.concatenate([bb, secondary.infer_oxygen(bb)[:, :, None]], axis=2), None, nd)

    ref = restated(tmp_path / "ens.pdb")
    ss = secondary.dssp(tmp_path / "ens.pdb", seq)
    assert np.array_equal(ss.codes, ref[0]) and np.array_equal(ss.counts, ref[1]) and np.array_equal(ss.acceptor, ref[2])
    assert np.array_equal(ss.energy.view(np.int64), ref[3].view(np.int64)) and ss.present.all() and np.all(ss.n_present == 4)
    assert ss.strings == [R.string(r) for r in ref[0]]
    targets = [restated(f) for f in files[4:]]
    agree = secondary.ss_agreement(ss, secondary.dssp(files[4], seq))
    want_q3 = (R.reduce3(ref[0]) == R.reduce3(targets[0][0])).mean(1)
    assert np.array_equal(agree["q3"], want_q3) and agree["q3_best"] == want_q3.max() and agree["best_model"] == int(want_q3.argmax())
    masked = secondary.dssp(tmp_path / "ens.pdb", seq, mask=np.arange(58) != 20)
    assert np.all(masked.codes[:, 20] == 0) and masked.n_present[20] == 0 and np.isnan(masked.propensity()[20]).all()

    args = ["--samples", str(tmp_path / "ens.pdb"), "--targets", str(files[4]), str(files[5])]
    plain = analyze_ensemble.main(args + ["--output", str(tmp_path / "plain")])
    full = json.loads(analyze_ensemble.main(args + ["--output", str(tmp_path / "dssp"), "--dssp"]).read_text())
    assert "dssp" not in json.loads(plain.read_text())
    assert json.dumps({k: v for k, v in full.items() if k != "dssp"}, indent=1) + "\n" == plain.read_text()   # the other keys: the same bytes
    block = full["dssp"]
    assert block["legend"] == R.LEGEND and block["strings"] == [R.string(r) for r in ref[0]]
    assert block["counts"] == ref[1].tolist() and [t["string"] for t in block["targets"]] == [R.string(t[0][0]) for t in targets]
    assert block["targets"][0]["agreement"]["q3"] == want_q3.tolist()
    assert np.array_equal(np.array(block["propensity"]), ss.propensity()) and block["content"] == ss.content()
    r1, r2 = R.reduce3(targets[0][0][0]), R.reduce3(targets[1][0][0])
    assert [s["residue"] for s in block["switch_residues"]] == np.nonzero(r1 != r2)[0].tolist()

    path = secondary_structure.main(["--samples", str(tmp_path / "ens.pdb"), "--output", str(tmp_path / "cli")])
    alone = json.loads(path.read_text())
    assert path.name == "ens.dssp.json" and set(alone) == {"legend", "reduced_legend", "strings", "counts", "propensity", "content"}
    assert {k: block[k] for k in alone} == alone
    assert (tmp_path / "cli" / "ens.ss").read_text().split() == block["strings"]
    two = json.loads(secondary_structure.main(["--samples", str(tmp_path / "ens.pdb"), "--output", str(tmp_path / "cli2"),
                                               "--max_models", "2"]).read_text())
    keep = np.sort(np.random.default_rng(0).choice(4, 2, replace=False))
    assert two["strings"] == [block["strings"][i] for i in keep]

"""CPU tests of the secondary-structure layer: the two numpy restatements of tests/dssp_ref.py (the reference of
tests/test_gpu_dssp.py) against the strings pinned for three crystal structures and the synthetic helices, and against each other on
noisy inputs; the C ABI's declaration; and what needs no device in esmdiff_amd/secondary.py."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import dssp_ref as R

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = np.load(ROOT / "tests" / "golden" / "g14_backbones.npz")

PINS = {
    "bpti": ("--TTTSS-----SSS--EEEEEEEGGGTEEEEEEE-SSS--SS-BS-HHHHHHHH---", None),
    "1fmf_A": ("----EEEEEEBTT----HHHHHHHHHHHHTT-EEEE-BSSB-HHHHHHHHHHHT-SEEEEEE-SSBHHHHHTTHHHHHHHTT-TT-EEEEEES-BSS---HHHHHHHHHHTT-SEEE-TT--"
               "HHHHHHHHHHHHT--", (20, 1)),
    "1c54_A": ("----EEEGGGS-HHHHHHHHHHHTT---SSTTTTEE---TT--S----TTSEEEEE---TT-SS--S-EEEEESSSS-EEEESSTTS--EEEETT-", (3, 13)),
}


def _chain(name):
    seq = str(GOLDEN[f"{name}_seq"])
    return GOLDEN[f"{name}_xyz"], np.array([c == "P" for c in seq], np.uint8)


def _same(a, b):
    """ss, counts, acceptor exactly, the energies bit for bit."""
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
            and np.array_equal(a[3].view(np.int64), b[3].view(np.int64)))


@pytest.mark.parametrize("name", sorted(PINS))
def test_pinned_strings_of_the_crystal_structures(name):
    xyz, no_donor = _chain(name)
    want, bridges = PINS[name]
    assert len(want) == len(xyz)
    out = R.dssp(xyz, no_donor=no_donor, details=True)
    assert R.string(out[0][0]) == want
    if bridges:
        assert (out[4][0]["parallel"], out[4][0]["antiparallel"]) == bridges
    loops = R.dssp_loops(xyz, no_donor=no_donor)
    assert R.string(loops[0][0]) == want and _same(out, loops)
    assert out[1].sum(1).tolist() == [1] * len(xyz) and out[2].dtype == np.int32 and out[0].dtype == np.uint8


def test_bpti_shows_the_known_fold():
    s = PINS["bpti"][0]
    assert s[17:24] == "EEEEEEE" and s[28:35] == "EEEEEEE" and s[44] == "B" and s[47:55] == "HHHHHHHH"


@pytest.mark.parametrize("phi_psi,want", [(R.ALPHA, "-HHHHHHHHHHHHHH-"), (R.HELIX310, "-GGGGGGGGGGGGGG-"), (R.PI, "-IIIIIIIIIIIIII-"),
                                          (R.BETA, "-" * 16)])
def test_pinned_strings_of_the_synthetic_chains(phi_psi, want):
    x = R.nerf([phi_psi] * 16)
    out, loops = R.dssp(x), R.dssp_loops(x)
    assert R.string(out[0][0]) == want and _same(out, loops)


def test_pinned_string_of_the_mixed_chain():
    x = R.nerf(R.MIXED)
    out = R.dssp(x)
    assert R.string(out[0][0]) == "-HHHHHHHHHS-----GGGGGGGGIIIIIIIII-" and _same(out, R.dssp_loops(x))


def test_nerf_geometry():
    x = R.nerf(R.MIXED)
    d = lambda a, b: np.linalg.norm(a - b, axis=-1)
    np.testing.assert_allclose(d(x[:, 0], x[:, 1]), 1.458, atol=1e-12)
    np.testing.assert_allclose(d(x[:, 1], x[:, 2]), 1.525, atol=1e-12)
    np.testing.assert_allclose(d(x[:-1, 2], x[1:, 0]), 1.329, atol=1e-12)
    np.testing.assert_allclose(d(x[:, 2], x[:, 3]), 1.231, atol=1e-12)


def test_the_inferred_oxygen_moves_three_residues_of_bpti():
    from esmdiff_amd import secondary
    xyz, no_donor = _chain("bpti")
    inferred = np.concatenate([xyz[:, :3], secondary.infer_oxygen(xyz)[:, None]], axis=1)
    got = R.string(R.dssp(inferred, no_donor=no_donor)[0][0])
    want = PINS["bpti"][0]
    assert [i for i in range(58) if got[i] != want[i]] == [24, 25, 26] and got[24:27] == "TTT" and want[24:27] == "GGG"
    rmsd = np.sqrt(np.mean(np.sum((inferred[:-1, 3] - xyz[:-1, 3]) ** 2, -1)))
    assert 0.05 < rmsd < 0.2


def test_the_two_restatements_agree_on_noisy_inputs():
    rng = np.random.default_rng(20261019)
    seen = set()
    for name, lo, hi in (("1fmf_A", 0, 70), ("1c54_A", 20, 96), ("bpti", 0, 58)):
        xyz, no_donor = _chain(name)
        for sigma in (0.3, 1.0):
            X = xyz[None, lo:hi] + sigma * rng.normal(size=(2, hi - lo, 4, 3))
            mask = rng.random((2, hi - lo)) > 0.2
            X[0, 7, 1] = np.nan                                  # a missing CA: absent
            X[1, 9, 3] = np.nan                                  # a missing O: present, accepts nothing, residue 10 donates nothing
            X[1, -1, 3] = np.nan
            for m in (None, mask):
                a, b = R.dssp(X, m, no_donor[lo:hi]), R.dssp_loops(X, m, no_donor[lo:hi])
                assert _same(a, b)
                seen |= set(a[0].reshape(-1).tolist())
                assert np.all(a[0][0, 7] == 0) and a[1][7].sum() <= 1
                if m is not None:
                    assert np.all(a[0][~m] == 0) and np.array_equal(a[1].sum(1), (m & np.isfinite(X[:, :, :3]).all((2, 3))).sum(0))
    assert seen >= {R.LOOP, R.S, R.T, R.G, R.B, R.E, R.H}


def test_edge_rules():
    x = R.nerf([R.ALPHA] * 16)
    acceptor, energy = R.dssp(x)[2][0], R.dssp(x)[3][0]
    assert acceptor[4:, 0].tolist() == list(range(12)) and np.all(acceptor[:4] == -1) and np.all(energy[:4] == 0.0)
    assert np.all(energy[4:, 0] < -0.5) and np.all(energy[:, 0] <= energy[:, 1])
    # a proline at 8 donates nothing: turn_4(4) is gone, the helix 5..8 + 3 loses the stretches that needed it
    nd = np.zeros(16, np.uint8)
    nd[8] = 1
    assert np.all(R.dssp(x, no_donor=nd)[2][0, 8] == -1)
    # a break: residues 8.. moved 100 A away; no hydrogen bond, turn or helix spans it
    y = x.copy()
    y[8:] += 100.0
    acc2 = R.dssp(y)[2][0]
    assert np.all(acc2[8] == -1) and np.all((acc2[8:] >= 8) | (acc2[8:] == -1)) and np.all(acc2[:8] < 8)
    # two atoms closer than 0.5 A: the pair's energy is the floor
    z = x.copy()
    z[5, 3] = z[9, 0] + np.array([0.3, 0.0, 0.0])
    info = R.dssp(z, details=True)
    assert info[4][0]["clamped"] >= 1 and info[3][0, 9, 0] == -9.9 and info[2][0, 9, 0] == 5
    assert _same(info[:4], R.dssp_loops(z))
    for L in range(1, 8):
        assert _same(R.dssp(x[:L]), R.dssp_loops(x[:L]))


def test_long_chains_take_well_under_a_second():
    import time
    xyz, _ = _chain("1fmf_A")
    big = np.concatenate([xyz + np.array([0.0, 0.0, 60.0 * k]) for k in range(8)])
    t0 = time.perf_counter()
    ss = R.dssp(big)[0]
    assert time.perf_counter() - t0 < 1.0 and len(big) == 1096
    assert R.string(ss[0, :137])[1:-1] == PINS["1fmf_A"][0][1:-1]          # the copies are separate chains, each with its own states


def test_header_declares_the_entry_and_the_binding_lists_it():
    from esmdiff_amd import _native as N
    header = (ROOT / "include" / "esmdiff_hip.h").read_text()
    decl = re.search(r"int\s+esmdiff_dssp\s*\(([^;]*)\)\s*;", header)
    assert decl, "include/esmdiff_hip.h does not declare esmdiff_dssp"
    args = [" ".join(a.split()) for a in decl.group(1).split(",")]
    assert args == ["const double* X", "int32_t n", "int32_t L", "const uint8_t* mask", "const uint8_t* no_donor", "uint8_t* ss",
                    "int32_t* counts", "int32_t* acceptor", "double* energy", "void* stream"]
    assert "esmdiff_dssp" in N.EXPORTS
    assert re.search(r"#define\s+ESMDIFF_ABI_VERSION\s+8\b", header)
    assert int(re.search(r"#define\s+ESMDIFF_DSSP_MAX_L\s+(\d+)", header).group(1)) == N.DSSP_MAX_L == 4096
    from esmdiff_amd import build
    assert build.UNITS["dssp"] == ["-ffp-contract=off"] and (build.CSRC / "dssp.hip").is_file()


def test_three_state_reduction_and_propensity():
    from esmdiff_amd import secondary as S
    assert S.LEGEND == R.LEGEND and "".join(S.REDUCED_LEGEND[c] for c in S.reduce_codes(np.arange(8))) == "CCCHHEEH"
    assert np.array_equal(S.reduce_codes(np.arange(8)), R.reduce3(np.arange(8)))
    codes = np.array([[R.H, R.H, R.E, R.LOOP, R.T], [R.G, R.S, R.B, R.LOOP, R.H], [R.I, R.E, R.E, R.LOOP, R.H], [R.H, R.T, R.LOOP, R.LOOP, R.E]])
    present = np.ones((4, 5), bool)
    present[:, 3] = False
    present[3, 4] = False
    ss = S.SecondaryStructure.from_codes(codes, present)
    assert ss.strings == ["HHE-T", "GSB-H", "IEE-H", "HT---"] and ss.n_present.tolist() == [4, 4, 4, 0, 3]
    assert ss.counts[0].tolist() == [0, 0, 0, 1, 1, 0, 0, 2] and ss.counts[3].sum() == 0
    p = ss.propensity()
    assert p[0].tolist() == [1.0, 0.0, 0.0] and p[1].tolist() == [0.25, 0.25, 0.5] and p[2].tolist() == [0.0, 0.75, 0.25]
    assert np.isnan(p[3]).all() and p[4].tolist() == [2 / 3, 0.0, 1 / 3]
    assert ss.propensity(reduced=False).shape == (5, 8) and ss.propensity(reduced=False)[0, R.H] == 0.5
    assert ss.content() == {"helix": 7 / 15, "strand": 4 / 15, "coil": 4 / 15}
    assert ss.reduced().tolist()[0] == [0, 0, 1, 2, 2]


def test_q3_and_switch_residues():
    from esmdiff_amd import secondary as S
    target = S.SecondaryStructure.from_codes([R.H, R.H, R.E, R.E, R.LOOP, R.LOOP], [1, 1, 1, 1, 1, 0])
    other = S.SecondaryStructure.from_codes([R.H, R.LOOP, R.E, R.H, R.LOOP, R.LOOP])
    samples = S.SecondaryStructure.from_codes([[R.G, R.H, R.B, R.T, R.S, R.H], [R.H, R.T, R.T, R.E, R.H, R.LOOP], [R.LOOP] * 6],
                                              [[1] * 6, [1, 1, 1, 1, 0, 1], [0] * 6])
    a = S.ss_agreement(samples, target)
    assert a["q3"][:2].tolist() == [4 / 5, 2 / 4] and np.isnan(a["q3"][2])
    assert a["q3_mean"] == (4 / 5 + 2 / 4) / 2 and a["q3_best"] == 4 / 5 and a["best_model"] == 0
    assert a["per_residue"][:5].tolist() == [1.0, 0.5, 0.5, 0.5, 1.0] and np.isnan(a["per_residue"][5])
    sw = S.switch_residues(samples, target, other)
    assert sw == [{"residue": 1, "classes": ["H", "C"], "share": [0.5, 0.5]}, {"residue": 3, "classes": ["E", "H"], "share": [0.5, 0.0]}]
    block = S.report(samples, [target, other])
    assert set(block) == {"legend", "reduced_legend", "strings", "counts", "propensity", "content", "targets", "switch_residues"}
    assert [t["string"] for t in block["targets"]] == ["HHEE--", "H-EH--"] and "switch_residues" not in S.report(samples, [target])
    assert set(S.report(samples)) == {"legend", "reduced_legend", "strings", "counts", "propensity", "content"}


def test_float64_oxygen_placement_equals_the_float32_one():
    from esmdiff_amd import pdbio, secondary
    xyz, _ = _chain("1c54_A")
    got = secondary.infer_oxygen(xyz)
    want = pdbio.infer_oxygen(xyz)
    assert want.dtype == np.float32 and got.dtype == np.float64 and np.isnan(got[-1]).all()
    assert np.array_equal(got[:-1].astype(np.float32), want[:-1])
    batch = np.stack([xyz[:, :3], xyz[::-1, :3]])
    both = secondary.infer_oxygen(batch)
    assert np.array_equal(both[0], got, equal_nan=True) and np.array_equal(both[1].astype(np.float32), pdbio.infer_oxygen(xyz[::-1]), equal_nan=True)
    bb = secondary.backbone_array(xyz[:, :3].astype(np.float32))
    assert bb.shape == (1, 96, 4, 3) and bb.dtype == np.float64 and np.isnan(bb[0, -1, 3]).all()
    assert secondary.backbone_array(xyz).shape == (1, 96, 4, 3) and np.array_equal(secondary.backbone_array(xyz)[0], xyz)
    assert np.isnan(secondary.infer_oxygen(xyz[:1])).all()
    with pytest.raises(AssertionError, match="backbones should be"):
        secondary.backbone_array(xyz[:, 1])


def test_parsers_know_dssp():
    from esmdiff_amd import analyze_ensemble, secondary_structure
    a = analyze_ensemble.parser().parse_args(["--samples", "x.pdb", "--targets", "a.pdb", "--output", "o", "--dssp"])
    assert a.dssp is True and analyze_ensemble.parser().parse_args(["--samples", "x.pdb", "--targets", "a.pdb", "--output", "o"]).dssp is False
    assert "--dssp" in analyze_ensemble.__doc__ and "DSSP-RECALL" in analyze_ensemble.__doc__
    b = secondary_structure.parser().parse_args(["--samples", "x.pdb", "--output", "o", "--max_models", "5"])
    assert (b.samples, b.output, b.max_models, b.seed) == ("x.pdb", "o", 5, 0)
    import inspect
    assert list(inspect.signature(analyze_ensemble.analyze).parameters)[-1] == "dssp"


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_dssp_has_no_cpu_fallback():
    from esmdiff_amd import secondary
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        secondary.dssp(R.nerf([R.ALPHA] * 8))

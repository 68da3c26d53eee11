"""CPU tests of the contact layer: the numpy restatement tests/contacts_ref.py (the reference of tests/test_gpu_contacts.py) against
hand-worked cases, the definitions' edge rules and the reference's own idp_metrics numbers (tests/golden/g9c_ensemble_helpers.npz), the
C ABI's declarations, and what needs no device in the Python surface."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import contacts_ref as R

ROOT = Path(__file__).resolve().parent.parent
BELOW_5 = np.nextafter(5.0, 0.0)


def test_contact_map_hand_worked():
    """Three frames of four CA atoms on a line, cutoff 8, min_sep 1.  Frame 0: x = 0, 4, 8, 12; frame 1: x = 0, 6, 12, 18; frame 2:
    x = 0, 2, 4, 6.  Pair (0, 1): d = 4, 6, 2 -> 3 contacts, sum 12, squares 56.  Pair (0, 2): d = 8, 12, 4 -> 1 contact (8 is not
    below 8), sum 24, squares 224.  Pair (0, 3): d = 12, 18, 6 -> 1, sum 36, squares 504."""
    X = np.stack([R.line([0, 4, 8, 12]), R.line([0, 6, 12, 18]), R.line([0, 2, 4, 6])])
    valid, count, sum_d, sum_d2 = R.contact_map(X, None, 8.0, 1)
    assert valid.tolist() == [[0, 3, 3, 3], [3, 0, 3, 3], [3, 3, 0, 3], [3, 3, 3, 0]]
    assert count[0].tolist() == [0, 3, 1, 1] and count[1].tolist() == [3, 0, 3, 1]
    assert sum_d[0].tolist() == [0.0, 12.0, 24.0, 36.0] and sum_d2[0].tolist() == [0.0, 56.0, 224.0, 504.0]
    for m in (valid, count, sum_d, sum_d2):
        assert np.array_equal(m, m.T)
    # min_separation: the pairs closer in sequence are 0 in every map
    v3, c3, s3, q3 = R.contact_map(X, None, 8.0, 3)
    keep = np.abs(np.subtract.outer(np.arange(4), np.arange(4))) >= 3
    assert np.array_equal(v3, valid * keep) and np.array_equal(c3, count * keep) and np.array_equal(s3, sum_d * keep)
    assert c3[0, 3] == 1 and v3.sum() == 6
    # a masked residue and a NaN coordinate leave the frame's pairs alike
    mask = np.ones((3, 4), bool)
    mask[1, 2] = False
    holes = X.copy()
    holes[1, 2] = np.nan
    got = R.contact_map(X, mask, 8.0, 1)
    assert got[0][0, 2] == 2 and got[1][1, 2] == 2 and got[2][0, 2] == 12.0 and got[3][0, 2] == 80.0 and got[0][0, 1] == 3
    for g, h in zip(got, R.contact_map(holes, None, 8.0, 1)):
        assert np.array_equal(g, h)
    assert np.isnan(R.frequency(v3, c3)[0, 1]) and R.frequency(valid, count)[0, 2] == 1 / 3


def test_contact_is_strict_at_the_cutoff():
    """(0, 0, 0) and (3, 4, 0): the distance is exactly 5.0, not below a cutoff of 5.0; (3, 4, 0) scaled to the next float below is."""
    X = np.array([[[0.0, 0, 0], [3.0, 4.0, 0]]])
    assert R.distances(X[0])[0, 1] == 5.0
    assert R.contact_map(X, None, 5.0, 1)[1][0, 1] == 0
    assert R.contact_map(X, None, np.nextafter(5.0, 6.0), 1)[1][0, 1] == 1
    near = np.array([[[0.0, 0, 0], [BELOW_5, 0, 0]]])
    assert R.contact_map(near, None, 5.0, 1)[1][0, 1] == 1


def test_chunked_order_is_the_one_that_is_stated():
    """40 frames of L = 5 are 3 chunks of 16, 16 and 8: the sums are the chunk sums added in order, each a running sum of its frames."""
    rng = np.random.default_rng(0)
    X = R.ensemble(rng, 40, R.chain(rng, 5))
    assert R.chunk_frames(40, 5) == 16 and R.chunks(40, 5) == 3
    d = np.stack([R.distances(x) for x in X])
    want = np.zeros((5, 5))
    for c in range(3):
        part = np.zeros((5, 5))
        for f in range(16 * c, min(40, 16 * c + 16)):
            part = part + d[f]
        want = part if c == 0 else want + part
    np.fill_diagonal(want, 0.0)
    assert np.array_equal(R.contact_map(X, None, 8.0, 1)[2], want)


def test_native_contacts_hand_worked():
    """Native at x = 0, 4, 8, 12, cutoff 8, min_sep 1: the contacts are the neighbours (d0 = 4), 6 ordered pairs, total_res = 1, 2, 2, 1.
    Model at x = 0, 4, 9, 18 with lam = 1.2: neighbour distances 4, 5, 9 against 4.8 -> only (0, 1) is kept, both ways."""
    native, model = R.line([0, 4, 8, 12])[None], R.line([0, 4, 9, 18])[None]
    kept, total, kept_res, total_res, q_soft = R.native_contacts(model, native, min_sep=1)
    assert total.tolist() == [6] and total_res.tolist() == [[1, 2, 2, 1]]
    assert kept.tolist() == [[2]] and kept_res.tolist() == [[[1, 1, 0, 0]]]
    want = 2 * sum(1.0 / (1.0 + np.exp(5.0 * (d - 4.8))) for d in (4.0, 5.0, 9.0))
    assert abs(q_soft[0, 0] - want) < 1e-15
    # min_separation 2: the native's pairs (a, a + 2) are 8 A apart, not below 8 -> no contact, Q is NaN
    kept, total, _, total_res, _ = R.native_contacts(model, native, min_sep=2)
    assert total.tolist() == [0] and kept.tolist() == [[0]]
    hard, soft, res = R.q(model, native, min_sep=2)
    assert np.isnan(hard).all() and np.isnan(soft).all() and np.isnan(res).all()
    # ... and with a cutoff of 9 they are: 4 more ordered pairs
    assert R.native_contacts(model, native, cutoff=9.0, min_sep=2)[1].tolist() == [4]
    assert R.native_contacts(model, native, cutoff=9.0, min_sep=1)[3].tolist() == [[2, 3, 3, 2]]     # 4 A and 8 A neighbours


def test_native_contacts_are_strict():
    """d0 = 5.0 exactly is no native contact at cutoff 5.0; with lam = 1.0 a model distance equal to d0 is not kept, the next float
    below it is."""
    native = np.array([[[0.0, 0, 0], [3.0, 4.0, 0]]])
    assert R.native_contacts(native, native, cutoff=5.0, min_sep=1)[1].tolist() == [0]
    assert R.native_contacts(native, native, cutoff=np.nextafter(5.0, 6.0), min_sep=1)[1].tolist() == [2]
    models = np.stack([R.line([0, 5.0]), R.line([0, BELOW_5]), R.line([0, np.nextafter(5.0, 6.0)])])
    kept, total, _, _, _ = R.native_contacts(models, native, cutoff=6.0, min_sep=1, lam=1.0)
    assert total.tolist() == [2] and kept[:, 0].tolist() == [0, 2, 0]


def test_masked_native_residue_leaves_the_contact_set():
    rng = np.random.default_rng(1)
    native, model = R.chain(rng, 14), R.chain(rng, 14)
    mask = np.ones((1, 14), bool)
    mask[0, 5] = False
    full = R.native_contacts(model[None], native[None], min_sep=1)
    kept, total, kept_res, total_res, q_soft = R.native_contacts(model[None], native[None], maskB=mask, min_sep=1)
    with_5 = R.distances(native)[5] < 8.0
    with_5[5] = False
    assert with_5.sum() >= 2 and total_res[0, 5] == 0 and kept_res[0, 0, 5] == 0
    assert np.array_equal(total_res[0], (full[3][0] - with_5) * (np.arange(14) != 5)) and total[0] == full[1][0] - 2 * with_5.sum()
    native_nan = native.copy()
    native_nan[5] = np.nan                                       # a masked coordinate is never looked at
    again = R.native_contacts(model[None], native_nan[None], maskB=mask, min_sep=1)
    assert np.array_equal(again[2], kept_res) and np.array_equal(again[4], q_soft)


def test_masked_model_residue_keeps_nothing_but_stays_in_total():
    rng = np.random.default_rng(2)
    native = R.chain(rng, 14)
    full = R.native_contacts(native[None], native[None], min_sep=1)
    mask = np.ones((1, 14), bool)
    mask[0, 3] = False
    kept, total, kept_res, total_res, q_soft = R.native_contacts(native[None], native[None], maskA=mask, min_sep=1)
    with_3 = R.distances(native)[3] < 8.0
    with_3[3] = False
    assert np.array_equal(total_res, full[3]) and total[0] == full[1][0]
    assert kept_res[0, 0, 3] == 0 and kept[0, 0] == full[0][0, 0] - 2 * with_3.sum()
    assert np.array_equal(kept_res[0, 0], (full[2][0, 0] - with_3) * (np.arange(14) != 3))
    assert q_soft[0, 0] < full[4][0, 0]


def test_q_of_a_native_against_itself():
    rng = np.random.default_rng(3)
    X = np.stack([R.chain(rng, 40) for _ in range(3)])
    hard, soft, res = R.q(X)
    assert np.array_equal(np.diag(hard), np.ones(3)) and np.all(np.diag(soft) < 1.0) and np.all(np.diag(soft) > 0.9)
    assert np.all(hard[~np.eye(3, dtype=bool)] < 1.0)
    ok = ~np.isnan(res[0, 0])
    assert ok.sum() > 30 and np.all(res[0, 0][ok] == 1.0)
    far = R.line([0, 20, 40, 60])[None]                          # no pair within 8 A
    hard, soft, res = R.q(far, far)
    assert np.isnan(hard[0, 0]) and np.isnan(soft[0, 0]) and np.isnan(res).all()


# ---- the reference's own numbers ------------------------------------------------------------------------------------------------------
G = np.load(ROOT / "tests" / "golden" / "g9_metrics.npz")
GC = np.load(ROOT / "tests" / "golden" / "g9c_ensemble_helpers.npz")
KEYS = [str(k) for k in G["keys"]]
ENS = {k: G["ca_" + k] for k in KEYS}


def test_maps_reproduce_the_reference_idp_metrics():
    """eval_utils.idp_metrics' contact and distance numbers (recorded from the reference's own code) from the (L, L) maps, at the
    tolerance tests/test_metrics.py holds the numpy restatement of idp_metrics to."""
    for tag, k in (("", 3), ("_k1", 1)):
        got = R.contact_error(dict(ENS), pwd_offset=k)
        for nm, d in zip(("mse_contact", "mae_contact", "mse_pwd", "mae_pwd"), got):
            want = GC[f"idp_{nm}{tag}"]
            assert np.allclose([d[key] for key in KEYS], want, rtol=1e-12, atol=1e-14), (nm, tag, [d[key] for key in KEYS], want)
            assert d["target"] == 0.0
    # the fixture is not degenerate: some pairs are in contact in some frames and not in all, and no distance sits on the cutoff
    valid, count, _, _ = R.contact_map(ENS["target"], None, 8.0, 3)
    iu = np.triu_indices(24, 3)
    assert len(iu[0]) == 231 and 5 <= ((count[iu] > 0) & (count[iu] < valid[iu])).sum() <= 7
    assert min(np.abs(R.distances(x)[iu] - 8.0).min() for x in ENS["target"]) > 2.5e-3


# ---- declarations ---------------------------------------------------------------------------------------------------------------------
def _macros(tmp_path):
    """The header's function-like macros as C functions: a few lines of C that include the header, compiled by the host compiler."""
    import ctypes
    import shutil
    import subprocess
    cc = next((c for c in (shutil.which("cc"), shutil.which("gcc"), shutil.which("clang"), "/opt/rocm/llvm/bin/clang",
                           "/opt/rocm/lib/llvm/bin/clang") if c and Path(c).exists()), None)
    assert cc, "no host C compiler"
    src = tmp_path / "contact_macros.c"
    src.write_text('#include "esmdiff_hip.h"\n'
                   "int64_t chunks(int64_t n, int64_t L) { return ESMDIFF_CONTACT_CHUNKS(n, L); }\n"
                   "int64_t frames(int64_t n, int64_t L) { return ESMDIFF_CONTACT_CHUNK_FRAMES(n, L); }\n"
                   "int64_t scratch(int64_t n, int64_t L) { return ESMDIFF_CONTACT_SCRATCH_BYTES(n, L); }\n")
    subprocess.run([cc, "-shared", "-fPIC", "-O1", f"-I{ROOT / 'include'}", str(src), "-o", str(tmp_path / "contact_macros.so")], check=True)
    lib = ctypes.CDLL(str(tmp_path / "contact_macros.so"))
    for fn in (lib.chunks, lib.frames, lib.scratch):
        fn.argtypes, fn.restype = [ctypes.c_int64, ctypes.c_int64], ctypes.c_int64
    return lib.chunks, lib.frames, lib.scratch


def test_header_declares_both_entries_and_the_binding_mirrors_the_macros(tmp_path):
    from esmdiff_amd import _native as N
    from esmdiff_amd import build
    header = (ROOT / "include" / "esmdiff_hip.h").read_text()
    decl = re.search(r"int\s+esmdiff_contact_map\s*\(([^;]*)\)\s*;", header)
    assert decl, "include/esmdiff_hip.h does not declare esmdiff_contact_map"
    args = [a.strip() for a in decl.group(1).split(",")]
    assert len(args) == 13 and args[0] == "const double* X" and args[-1] == "void* stream"
    assert [a for a in args if a.startswith("int32_t*")] == ["int32_t* valid", "int32_t* count"]
    assert [a for a in args if a.startswith("double*")] == ["double* sum_d", "double* sum_d2"]
    decl = re.search(r"int\s+esmdiff_native_contacts\s*\(([^;]*)\)\s*;", header)
    assert decl, "include/esmdiff_hip.h does not declare esmdiff_native_contacts"
    args = [a.strip() for a in decl.group(1).split(",")]
    assert len(args) == 17 and args[0] == "const double* A" and args[-1] == "void* stream"
    assert [a for a in args if a.startswith("int32_t*")] == ["int32_t* kept", "int32_t* total", "int32_t* kept_res", "int32_t* total_res"]
    assert "double* q_soft" in args
    assert "esmdiff_contact_map" in N.EXPORTS and "esmdiff_native_contacts" in N.EXPORTS
    assert re.search(r"#define\s+ESMDIFF_ABI_VERSION\s+8\b", header)
    limit = int(re.search(r"#define\s+ESMDIFF_CONTACT_MAX_L\s+(\d+)", header).group(1))
    assert limit >= 4096 and limit == N.CONTACT_MAX_L == R.MAX_L
    assert int(re.search(r"#define\s+ESMDIFF_CONTACT_MAX_CHUNKS\s+(\d+)", header).group(1)) == N.CONTACT_MAX_CHUNKS == R.MAX_CHUNKS
    assert int(re.search(r"#define\s+ESMDIFF_CONTACT_TILE\s+(\d+)", header).group(1)) == N.CONTACT_TILE == R.TILE
    chunks, frames, scratch = _macros(tmp_path)
    seen = set()
    for L in (2, 5, 58, 63, 64, 65, 128, 129, 256, 448, 449, 1000, 1984, 1985, 4096):
        for n in (1, 15, 16, 17, 32, 33, 100, 1008, 1009, 4080, 4081, 4096, 4097, 5000, 100000):
            c = chunks(n, L)
            assert c == N.contact_chunks(n, L) == R.chunks(n, L), (n, L)
            assert frames(n, L) == N.contact_chunk_frames(n, L) == R.chunk_frames(n, L), (n, L)
            assert scratch(n, L) == N.contact_scratch_bytes(n, L) == R.scratch_bytes(n, L), (n, L)
            assert 1 <= c <= 256 and (c - 1) * frames(n, L) < n <= c * frames(n, L)       # no chunk is empty
            assert (scratch(n, L) == 0) == (c == 1)
            seen.add(c)
    assert {1, 2, 3, 64, 256} <= seen and chunks(100000, 58) == 256 and chunks(100000, 1985) == 1 and chunks(100000, 1984) == 2
    assert "-ffp-contract=off" in build.UNITS["contacts"]
    assert (ROOT / "esmdiff_amd" / "csrc" / "contacts.hip").is_file()


def test_parser_knows_contacts():
    from esmdiff_amd import analyze_ensemble
    a = analyze_ensemble.parser().parse_args(["--samples", "x.pdb", "--targets", "t.pdb", "--output", "o", "--contacts",
                                              "--contact_cutoff", "7.5", "--contact_min_sep", "4"])
    assert a.contacts is True and a.contact_cutoff == 7.5 and a.contact_min_sep == 4
    a = analyze_ensemble.parser().parse_args(["--samples", "x.pdb", "--targets", "t.pdb", "--output", "o"])
    assert a.contacts is False and a.contact_cutoff == 8.0 and a.contact_min_sep == 3
    assert "--contacts" in analyze_ensemble.__doc__


def test_flory_exponent_is_plain_numpy():
    from esmdiff_amd import contacts
    s = np.arange(1, 40)
    for nu in (0.5, 0.6, 1.0):
        assert abs(contacts.flory_exponent(contacts.Scaling(s, 3.8 * s ** nu)) - nu) < 1e-12
    bent = np.where(s < 10, 3.8 * s, 3.8 * 10 ** 0.5 * s ** 0.5)
    assert abs(contacts.flory_exponent(contacts.Scaling(s, bent), fit_range=(10, 39)) - 0.5) < 1e-12
    assert abs(contacts.flory_exponent(contacts.Scaling(s, bent), fit_range=(1, 9)) - 1.0) < 1e-12
    assert np.isnan(contacts.flory_exponent(contacts.Scaling(s, np.full(39, np.nan))))


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_contacts_have_no_cpu_fallback():
    from esmdiff_amd import contacts
    x = np.zeros((2, 5, 3))
    for call in (lambda: contacts.contact_map(x), lambda: contacts.contact_error({"target": x, "m": x}),
                 lambda: contacts.native_contacts(x, x), lambda: contacts.q_ensemble(x, x),
                 lambda: contacts.contact_switches(x, x[0], x[1]), lambda: contacts.internal_scaling(x),
                 lambda: contacts.report(x, x)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()

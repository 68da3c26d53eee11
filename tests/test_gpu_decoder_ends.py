"""The kernels that turn the structure decoder's and the structure encoder's outputs into what a user reads, one at a time
(run with -m gpu on an MI355X): backbone coordinates, pLDDT, the pair features, PAE / TM rows / pTM, the encoder's nearest
neighbours, neighbourhood gather and nearest code, and the chunk loop of the pairwise head over a batch.

References, inputs and bars are tests/decoder_ends_ref.py (float64 statements written from oracle/decoder_ref.py and
oracle/encoder_ref.py; each bar 4 x what a float32 evaluation of the same formula needs over these very inputs);
tests/test_decoder_ends_cpu.py checks them without a GPU.  Where a result is determined exactly (pair features, neighbours on
a lattice, integer codes, gathers, the same sample in another chunk) the comparison is torch.equal.

Every kernel's own needed_coef is printed as a MEASURED line and written to parity_decoder_ends.json, in the directory where
tests/test_gpu_strict.py keeps parity_strict.json.
"""
import json

import pytest
import torch

from tests import decoder_ends_ref as dr
from tests.test_gpu_strict import _OUT as _STRICT_OUT

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
_OUT = _STRICT_OUT.with_name("parity_decoder_ends.json")        # the suite's one directory of measured figures


def _record(key, val):
    try:
        _OUT.parent.mkdir(exist_ok=True)
        cur = json.loads(_OUT.read_text()) if _OUT.exists() else {}
        cur[key] = val
        _OUT.write_text(json.dumps(cur, indent=1, sort_keys=True))
    except OSError:
        pass
    print("MEASURED", key, json.dumps(val))


def _padded(v: torch.Tensor, ld: int) -> torch.Tensor:
    """v (M, n) inside rows of ld floats on the device; the padding holds values that would show if they were read."""
    buf = torch.full((v.shape[0], ld), 1e30, dtype=F32)
    buf[:, :v.shape[1]] = v
    return buf.cuda()


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ld", [23, 128])
@pytest.mark.parametrize("M", dr.BACKBONE_M)
def test_dim6_to_backbone_vs_float64(M, ld):
    from esmdiff_amd.engine import dim6_to_backbone
    need = {"coords": 0.0, "bonds": 0.0}
    ideal = torch.tensor(dr.IDEAL_BONDS, dtype=F64)
    worst = []
    for seed in (0, 1):
        v = dr.backbone_case(M, seed)
        ref, unit = dr.backbone_formula(v, 10.0, F64), dr.backbone_unit(v, 10.0)
        got = dim6_to_backbone(_padded(v, ld), 10.0).cpu()
        assert got.shape == (M, 3, 3) and bool(torch.isfinite(got).all())
        bl = dr.bond_lengths(got)
        need["coords"] = max(need["coords"], dr.needed_coef(got, ref, F32, unit))
        need["bonds"] = max(need["bonds"], dr.needed_coef(bl, ideal.expand_as(bl), F32, unit[:, 0]))
        r = dr.ratio(got, ref, F32, dr.BACKBONE_COEF * unit)
        rb = dr.ratio(bl, ideal.expand_as(bl), F32, dr.BACKBONE_COEF * unit[:, 0])
        worst.append((seed, float(r.max()), int(r.amax((1, 2)).argmax()), float(rb.max())))
    _record(f"dim6_to_backbone[M={M},ld={ld}]", need)
    for seed, rmax, row, rbmax in worst:
        assert rmax <= 1.0, (seed, rmax, row)
        assert rbmax <= 1.0, (seed, rbmax)                                      # |N - CA| = 1.4592, |C - CA| = 1.5251


def test_dim6_to_backbone_degenerate_rows_stay_finite():
    """x = 0, y = 0, both, y parallel / antiparallel to x: the frame is ill-conditioned there, so these rows are compared
    with nothing; they must not produce Inf / NaN, their CA is still trans, and they sit in a tensor of their own."""
    from esmdiff_amd.engine import dim6_to_backbone
    v = dr.backbone_degenerate_rows()
    got = dim6_to_backbone(_padded(v, 23), 10.0).cpu()
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got[:, 1], v[:, :3] * 10.0)


@pytest.mark.parametrize("ld", [50, 64])
@pytest.mark.parametrize("M", dr.BACKBONE_M)
def test_plddt_mean_vs_float64(M, ld):
    from esmdiff_amd.engine import plddt_mean
    cases = []
    for seed in (0, 1):
        p = dr.plddt_case(M, seed)
        cases.append((seed, dr.plddt_formula(p, F64), plddt_mean(_padded(p, ld), dr.PLDDT_BINS).cpu()))
    _record(f"plddt_mean[M={M},ld={ld}]", max(dr.needed_coef(got, ref, F32, dr.F32_EPS) for _, ref, got in cases))
    for seed, ref, got in cases:
        assert float(dr.ratio(got, ref, F32, dr.PLDDT_COEF * dr.F32_EPS).max()) <= 1.0, seed
        if M >= dr.PLDDT_SPECIAL:
            s = M - dr.PLDDT_SPECIAL
            centres = (torch.arange(50, dtype=F64) + 0.5) / 50
            # one bin at +90, the rest at -90: that bin's centre; all-equal logits: 0.5
            assert float(dr.ratio(got[s:s + 50], centres, F32, dr.PLDDT_COEF * dr.F32_EPS).max()) <= 1.0
            assert float(dr.ratio(got[s + 50:], torch.full((4,), 0.5, dtype=F64), F32, dr.PLDDT_COEF * dr.F32_EPS).max()) <= 1.0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("nb,L", dr.PAIR_SHAPES)
def test_pair_features_bit_for_bit(nb, L, dtype):
    """Feature (i, j) = [q_j * k_i | q_j - k_i]: one float32 operation per element, rounded once to the build's type, so the
    bits are determined.  Random data: a transposed pair or a shifted sample cannot pass."""
    from esmdiff_amd.engine import pair_features
    qk = torch.randn(nb, L, 128, generator=torch.Generator().manual_seed(nb * 100 + L)).to(dtype)
    got = pair_features(qk.cuda()).cpu()
    want = dr.pair_features_expected(qk)
    assert got.dtype == dtype and got.shape == (nb, L, L, 128)
    view = torch.int16 if dtype == torch.bfloat16 else torch.int32
    assert torch.equal(got.view(view), want.view(view))


# ---------------------------------------------------------------------------------------------------------------
def test_pae_tm_bin_sweep():
    """Pair (i, j) puts all its probability into bin (i L + j) % 64: PAE(i, j) is that bin's centre (all 64, the special
    last one included, and each through the 16-lanes-per-pair mapping), TM row i the mean of 1 / (1 + (c / d0)^2)."""
    from esmdiff_amd.engine import pae_tm
    lg, tk, bins = dr.pae_sweep_case()
    ref = dr.pae_tm_formula(lg, tk, F64)
    tm, pae, ptm = (t.cpu() for t in pae_tm(lg.cuda(), tk.cuda()))
    centres = dr.pae_centres(F64)
    err = (pae.double() - centres[bins][None]).abs()
    _record("pae_tm_sweep", {"pae_abs_err": float(err.max()), "tm_rows": dr.needed_coef(tm, ref[1], F32, dr.F32_EPS)})
    assert float(err.max()) <= dr.SWEEP_PAE_ABS, (float(err.max()), int(bins.flatten()[err[0].flatten().argmax()]))
    assert float(dr.ratio(tm, ref[1], F32, dr.TM_COEF * dr.F32_EPS).max()) <= 1.0
    assert torch.equal(ptm, tm.max(-1).values)


@pytest.mark.parametrize("scale", dr.PAE_SCALES)
@pytest.mark.parametrize("L,counts", dr.PAE_CASES)
def test_pae_tm_vs_float64(L, counts, scale):
    from esmdiff_amd.engine import pae_tm
    lg, tk = dr.pae_case(L, counts, scale)
    ref_pae, ref_tm, ref_ptm = dr.pae_tm_formula(lg, tk, F64)
    lgd, tkd = lg.cuda(), tk.cuda()
    tm, pae, ptm = (t.cpu() for t in pae_tm(lgd, tkd))
    aa = tk < dr.MASK_ID
    sq = aa[:, :, None] & aa[:, None, :]
    _record(f"pae_tm[L={L},valid={list(counts)},x{scale:g}]",
            {"pae": dr.needed_coef(pae, ref_pae, F32, dr.PAE_UNIT), "tm_rows": dr.needed_coef(tm, ref_tm, F32, dr.F32_EPS),
             "ptm": dr.needed_coef(ptm, ref_ptm, F32, dr.F32_EPS)})
    assert float(dr.ratio(pae, ref_pae, F32, dr.PAE_COEF * dr.PAE_UNIT).max()) <= 1.0
    if bool((~sq).any()):                                                     # masked pairs: the mean of the centres
        mean_c = dr.pae_centres(F64).mean().expand(int((~sq).sum()))
        assert float(dr.ratio(pae[~sq], mean_c, F32, dr.PAE_COEF * dr.PAE_UNIT).max()) <= 1.0
    assert float(dr.ratio(tm, ref_tm, F32, dr.TM_COEF * dr.F32_EPS).max()) <= 1.0
    assert bool((tm[~aa] == 0).all())                                         # special-token rows: exactly 0
    assert float(dr.ratio(ptm, ref_ptm, F32, dr.TM_COEF * dr.F32_EPS).max()) <= 1.0
    assert torch.equal(ptm, tm.max(-1).values)                                # pTM is the maximum of the rows it returns
    for b, n in enumerate(counts):
        if n == 0:
            assert float(ptm[b]) == 0.0
    # without a PAE matrix: the same pTM and TM rows, bit for bit
    tm2, none, ptm2 = pae_tm(lgd, tkd, want_pae=False)
    assert none is None and torch.equal(ptm2.cpu(), ptm) and torch.equal(tm2.cpu(), tm)


# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lattice_edges():
    """(L, pattern) -> (ca, has, oracle neighbours float64), computed once and left unchanged."""
    from oracle.encoder_ref import knn_edges
    out = {}
    for L in dr.KNN_L:
        for pat in dr.KNN_PATTERNS:
            ca, has = dr.knn_lattice_case(L, pat)
            out[(L, pat)] = (ca, has, knn_edges(ca.double(), has, dr.KNN))
    return out


@pytest.mark.parametrize("pattern", dr.KNN_PATTERNS)
@pytest.mark.parametrize("L", dr.KNN_L)
def test_encoder_knn_on_a_lattice_is_the_oracles(lattice_edges, L, pattern):
    """Exact keys with ties everywhere (tests/decoder_ends_ref.py: lattice_fold): the lowest index among equals.  The narrow
    folds and the all-unknown sample tie keys of different threads only (the reduction's rule); the "wide" folds at
    L = 300 also tie residues j and j + 256 among one residue's 16 nearest, two keys of one thread (the scan's rule;
    tests/test_decoder_ends_cpu.py asserts the fixture holds such pairs)."""
    from esmdiff_amd.engine import encoder_knn
    ca, has, want = lattice_edges[(L, pattern)]
    got = encoder_knn(ca.cuda(), has.cuda(), dr.KNN).cpu().long()
    assert got.shape == (2, L, min(dr.KNN, L))
    assert torch.equal(got, want), (got != want).nonzero()[:4].tolist()
    if pattern == "known+none":                                               # nothing known: i, i - 1, i + 1, i - 2, ...
        assert torch.equal(got[1], dr.all_unknown_order(L, min(dr.KNN, L)))


@pytest.mark.parametrize("L", [64, 300])
def test_encoder_knn_on_a_lattice_scaled_by_3_8_differs_only_at_near_ties(L):
    """The same folds at the real CA - CA distance: 3.8 n is rounded, equal lattice distances become keys a few ulp apart,
    and no exact order exists to demand (tests/test_decoder_ends_cpu.py); every difference from the float64 oracle must still
    be between two candidates whose float64 keys agree to 2^-22.  Near ties abound here, so the share is reported, not capped."""
    from esmdiff_amd.engine import encoder_knn
    from oracle.encoder_ref import knn_edges
    for pattern in dr.KNN_PATTERNS:
        ca, has = dr.knn_lattice_case(L, pattern, scale=3.8)
        want = knn_edges(ca.double(), has, dr.KNN)
        got = encoder_knn(ca.cuda(), has.cuda(), dr.KNN).cpu()
        share, far = dr.knn_unexplained(got, want, dr.knn_keys64(ca, has))
        _record(f"encoder_knn_lattice_3.8[L={L},{pattern}]", {"differing_share": share, "not_near_ties": far})
        assert far == 0


def test_encoder_knn_random_coordinates_vs_float64():
    from esmdiff_amd.engine import encoder_knn
    from oracle.encoder_ref import knn_edges
    ca, has = dr.knn_random_case()
    want = knn_edges(ca.double(), has, dr.KNN)
    got = encoder_knn(ca.cuda(), has.cuda(), dr.KNN).cpu()
    share, far = dr.knn_unexplained(got, want, dr.knn_keys64(ca, has))
    _record("encoder_knn_random", {"differing_share": share, "not_near_ties": far})
    assert far == 0 and share <= 0.01


@pytest.mark.parametrize("pattern", dr.KNN_PATTERNS)
@pytest.mark.parametrize("L", dr.KNN_L)
def test_encoder_neighbourhood_bit_for_bit(lattice_edges, L, pattern):
    from esmdiff_amd.engine import encoder_neighbourhood
    ca, has, edges = lattice_edges[(L, pattern)]
    D, bins = 256, 32
    g = torch.Generator().manual_seed(L)
    table = torch.randn(2 * bins + 2, D, generator=g)
    rot, trans = torch.randn(2, L, 3, 3, generator=g), torch.randn(2, L, 3, generator=g)
    if L == 300 and pattern == "known+none":                                   # the clamp at +-bins is reached on both sides
        off = edges[0] - edges[0][:, :1]
        assert int(off.min()) < -bins and int(off.max()) > bins
    want = dr.neighbourhood_expected(edges, table, rot, trans, has, bins)
    got = encoder_neighbourhood(edges.int().cuda(), table.cuda(), rot, trans, has, bins)
    for name, a, b in zip(("x", "nrot", "ntrans", "nmask"), got, want):
        assert torch.equal(a.cpu(), b), name


@pytest.mark.parametrize("n_codes", dr.CODE_N)
@pytest.mark.parametrize("R", dr.CODE_R)
def test_encoder_nearest_code_integer_ties(R, n_codes):
    """Exact distances; every other row sits on a duplicated code row (tests/decoder_ends_ref.py: duplicate_pairs): the lower
    index wins within a thread's stride and across threads; rows without a frame give MASK."""
    from esmdiff_amd.engine import encoder_nearest_code
    z, code, has, pairs = dr.code_integer_case(R, n_codes)
    want = dr.nearest_code_formula(z, code, has, F64)
    got = encoder_nearest_code(z.cuda(), code.cuda(), has.cuda()).cpu()
    assert torch.equal(got, want), (got != want).nonzero().flatten()[:4].tolist()
    assert bool((got[~has] == dr.MASK_ID).all())


def test_encoder_nearest_code_random_vs_float64():
    from esmdiff_amd.engine import encoder_nearest_code
    z, code, has = dr.code_random_case()
    got = encoder_nearest_code(z.cuda(), code.cuda(), has.cuda()).cpu()
    share, far = dr.code_unexplained(got, z, code, has)
    _record("encoder_nearest_code_random", {"differing_share": share, "not_near_ties": far})
    assert far == 0 and share <= 0.01


# ---------------------------------------------------------------------------------------------------------------
def _decoder(precision, max_batch, max_len):
    from esmdiff_amd.config import TINY_DECODER
    from esmdiff_amd.engine import StructureDecoder
    from esmdiff_amd.weights import random_init_decoder_state_dict
    sd = random_init_decoder_state_dict(TINY_DECODER, seed=2)
    assert "pairwise_classification_head.linear2.weight" in sd
    return StructureDecoder(TINY_DECODER, sd, max_batch=max_batch, max_len=max_len, precision=precision)


def _tokens(B, L, seed):
    g = torch.Generator().manual_seed(seed)
    tok = torch.randint(0, 4096, (B, L), generator=g)
    tok[:, 0], tok[:, -1] = dr.BOS, dr.EOS
    tok[0, L // 2] = dr.MASK_ID
    return tok


def _pair_row_bytes(precision):
    """What esmdiff_hip_test.h states of esmdiff_decoder_set_pair_chunk_bytes: features + hidden + 64 f32 logits per pair row."""
    return 256 * (4 if precision == "f32" else 2) + 256


@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_pairwise_chunk_loop_is_bit_identical_to_one_chunk(precision):
    """B = 5 samples decoded in one chunk (the default budget), in chunks of 2, 2, 1 and one by one.  Every kernel of the
    pairwise head is local to its pair row and the GEMMs' rows do not depend on M (tests/test_gpu_gemm_dispatch.py), so pTM
    and PAE must not change by a bit: a difference is a wrong per-chunk offset."""
    B, L = 5, 33
    dec = _decoder(precision, B, L)
    tok = _tokens(B, L, 11)
    try:
        base = [t.cpu() for t in dec.decode(tok, return_ptm=True, return_pae=True)]
        assert float(base[1].min()) > 0 and len({float(v) for v in base[1]}) == B      # five different samples
        for cb in (2, 1):
            dec.set_pair_chunk_bytes(cb * L * L * _pair_row_bytes(precision))
            got = [t.cpu() for t in dec.decode(tok, return_ptm=True, return_pae=True)]
            assert torch.equal(got[1], base[1]), (cb, "ptm")
            assert torch.equal(got[2], base[2]), (cb, "pae", (got[2] != base[2]).nonzero()[:3].tolist())
            assert torch.equal(got[0], base[0])
            only_ptm = dec.decode(tok, return_ptm=True)[1].cpu()                   # pae = NULL in the chunk loop
            assert torch.equal(only_ptm, base[1]), (cb, "ptm without pae")
        dec.set_pair_chunk_bytes(0)                                                # the default again
        got = [t.cpu() for t in dec.decode(tok, return_ptm=True, return_pae=True)]
        assert torch.equal(got[1], base[1]) and torch.equal(got[2], base[2])
        with pytest.raises(RuntimeError):
            dec.set_pair_chunk_bytes(-1)
    finally:
        dec.close()


@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_pairwise_workspace_reallocation(precision):
    """L = 20, then 40 (the pair-row workspace grows), then 20 again (it stays): the first and third results are the same
    bits, the second is a fresh decoder's."""
    dec, fresh = _decoder(precision, 2, 40), _decoder(precision, 2, 40)
    t20, t40 = _tokens(2, 20, 5), _tokens(2, 40, 6)
    try:
        a = [t.cpu() for t in dec.decode(t20, return_ptm=True, return_pae=True)]
        b = [t.cpu() for t in dec.decode(t40, return_ptm=True, return_pae=True)]
        c = [t.cpu() for t in dec.decode(t20, return_ptm=True, return_pae=True)]
        f = [t.cpu() for t in fresh.decode(t40, return_ptm=True, return_pae=True)]
        for x, y in zip(a, c):
            assert torch.equal(x, y)
        for x, y in zip(b, f):
            assert torch.equal(x, y)
        assert b[2].shape == (2, 40, 40) and float(b[1].min()) > 0
    finally:
        dec.close()
        fresh.close()


def test_set_pair_chunk_bytes_refuses_other_engines():
    from esmdiff_amd import _native as N
    from esmdiff_amd.config import TINY
    from esmdiff_amd.engine import Engine
    from esmdiff_amd.weights import random_init_state_dict
    eng = Engine(TINY, random_init_state_dict(TINY, seed=0), max_batch=1, max_len=16)
    try:
        assert N.lib().esmdiff_decoder_set_pair_chunk_bytes(eng._h, 1 << 20) == -1
    finally:
        eng.close()

"""The references, inputs and bars of tests/test_gpu_decoder_ends.py (tests/decoder_ends_ref.py), checked without a GPU:
the float64 statements agree with the oracle's own functions, every bar lets the float32 evaluation of the same formula
through with the factor 4 it was derived with, every bar stops the planted errors, and the reference alone satisfies every
equality the GPU test demands (float32 and float64 give the same neighbours / codes on the exact fixtures).  Also: the new
test entry points refuse bad arguments without touching a device."""
import ctypes

import pytest
import torch
import torch.nn as nn

from oracle import decoder_ref as od
from oracle.encoder_ref import knn_edges
from tests import decoder_ends_ref as dr

F64, F32 = torch.float64, torch.float32
SEEDS = (0, 1)


def _passes(r) -> bool:
    return bool(torch.isfinite(r).all()) and float(r.max()) <= 1.0


# ---------------------------------------------------------------------------------------------------------------
# the bars and where they come from
@pytest.fixture(scope="module")
def pae_refs():
    """(L, counts, scale) -> (logits, tokens, float64 (pae, tm_rows, ptm)): computed once."""
    out = {}
    for L, counts in dr.PAE_CASES:
        for sc in dr.PAE_SCALES:
            lg, tk = dr.pae_case(L, counts, sc)
            out[(L, counts, sc)] = (lg, tk, dr.pae_tm_formula(lg, tk, F64))
    return out


def test_backbone_and_plddt_bars_hold_four_times_the_float32_evaluation():
    need = {"backbone": 0.0, "bond": 0.0, "plddt": 0.0}
    ideal = torch.tensor(dr.IDEAL_BONDS, dtype=F64)
    for M in dr.BACKBONE_M:
        for seed in SEEDS:
            v = dr.backbone_case(M, seed)
            got, ref, unit = dr.backbone_formula(v, 10.0, F32), dr.backbone_formula(v, 10.0, F64), dr.backbone_unit(v, 10.0)
            need["backbone"] = max(need["backbone"], dr.needed_coef(got, ref, F32, unit))
            bl = dr.bond_lengths(got)
            need["bond"] = max(need["bond"], dr.needed_coef(bl, ideal.expand_as(bl), F32, unit[:, 0]))
            # the reference has the ideal bonds (up to the 1e-12 under Gram-Schmidt's square roots: 1e-3 of the smallest unit)
            assert float((dr.bond_lengths(ref) - ideal).abs().max()) < 1e-2 * float(unit.min())
            p = dr.plddt_case(M, seed)
            need["plddt"] = max(need["plddt"], dr.needed_coef(dr.plddt_formula(p, F32), dr.plddt_formula(p, F64), F32, dr.F32_EPS))
    print("MEASURED float32 needed_coef", need)
    assert need["backbone"] <= dr.BACKBONE_COEF / 4 and need["bond"] <= dr.BACKBONE_COEF / 4
    assert need["plddt"] <= dr.PLDDT_COEF / 4
    # ... and the bars are no looser than that rule makes them (a figure within 2 x of a power of two may land on either side)
    assert dr.BACKBONE_COEF <= 2 * dr.pow2_bar(need["backbone"]) and dr.PLDDT_COEF <= 2 * dr.pow2_bar(need["plddt"])


def test_pae_and_tm_bars_hold_four_times_the_float32_evaluation(pae_refs):
    need = {"pae": 0.0, "tm": 0.0, "ptm": 0.0}
    for lg, tk, ref in pae_refs.values():
        got = dr.pae_tm_formula(lg, tk, F32)
        need["pae"] = max(need["pae"], dr.needed_coef(got[0], ref[0], F32, dr.PAE_UNIT))
        need["tm"] = max(need["tm"], dr.needed_coef(got[1], ref[1], F32, dr.F32_EPS))
        need["ptm"] = max(need["ptm"], dr.needed_coef(got[2], ref[2], F32, dr.F32_EPS))
    lg, tk, bins = dr.pae_sweep_case()
    got, ref = dr.pae_tm_formula(lg, tk, F32), dr.pae_tm_formula(lg, tk, F64)
    need["sweep_tm"] = dr.needed_coef(got[1], ref[1], F32, dr.F32_EPS)
    print("MEASURED float32 needed_coef", need)
    assert need["pae"] <= dr.PAE_COEF / 4 and max(need["tm"], need["ptm"], need["sweep_tm"]) <= dr.TM_COEF / 4
    assert dr.PAE_COEF <= 2 * dr.pow2_bar(need["pae"]) and dr.TM_COEF <= 2 * dr.pow2_bar(need["tm"])
    # the bin sweep: the reference is the bin's centre itself, and float32 is within 2 ulp of 31.5 of it
    centres = dr.pae_centres(F64)
    assert torch.equal(ref[0], centres[bins][None].expand_as(ref[0]))
    assert float((got[0].double() - ref[0]).abs().max()) <= dr.SWEEP_PAE_ABS
    assert set(bins.flatten().tolist()) == set(range(64))                       # every centre is pinned
    n = dr.SWEEP_L
    assert n < 19                                                              # ... with d0 at its clamp
    d0 = 1.24 * (19 - 15) ** (1 / 3) - 1.8
    want = (1 / (1 + (centres[bins] / d0) ** 2)).mean(-1)
    assert float((ref[1] - want[None]).abs().max()) < 1e-12


# ---------------------------------------------------------------------------------------------------------------
# the float64 statements against the oracle's own functions
class _Const(nn.Module):
    def __init__(self, v):
        super().__init__()
        self.v = v

    def forward(self, x):
        return self.v


def test_backbone_statement_is_the_oracle_heads_tail():
    v = dr.backbone_case(257, 0)
    head = od.Dim6RotStructureHeadRef(8, trans_scale=10.0).double()
    head.proj = _Const(v.double())                                            # the tail, fed the 23-vectors
    with torch.no_grad():
        want = head(torch.zeros(257, 8, dtype=F64))
    ref = dr.backbone_formula(v, 10.0, F64)
    # the oracle forms -x as trans - (x + trans): 2^-53 |trans| on a unit vector, times the 1.6 A of the ideal atoms
    assert float((ref - want).abs().max()) < 1e-12
    head32 = od.Dim6RotStructureHeadRef(8, trans_scale=10.0)
    head32.proj = _Const(v)
    with torch.no_grad():
        want32 = head32(torch.zeros(257, 8))
    # in float32 that round trip costs the oracle 2^-24 |trans| per axis component: inside the unit, outside the bar's 4 x
    assert float(dr.ratio(want32, ref, F32, 4 * dr.BACKBONE_COEF * dr.backbone_unit(v, 10.0)).max()) <= 1.0


def test_plddt_statement_is_the_oracle_mixture_mean():
    p = dr.plddt_case(257, 0)
    centres = (torch.arange(50, dtype=F32) + 0.5) / 50                         # oracle.decoder_ref, StructureTokenDecoderRef.forward
    want = (p.softmax(-1) * centres).sum(-1)
    ref = dr.plddt_formula(p, F64)
    assert _passes(dr.ratio(want, ref, F32, dr.PLDDT_COEF * dr.F32_EPS))
    s = 257 - dr.PLDDT_SPECIAL
    assert float((ref[s:s + 50] - (torch.arange(50, dtype=F64) + 0.5) / 50).abs().max()) < 1e-15    # one-hot rows: the centres
    assert float((ref[s + 50:] - 0.5).abs().max()) < 1e-15                                              # all-equal rows: 0.5


def test_pae_and_tm_statements_are_the_oracle_functions(pae_refs):
    assert float((dr.pae_centres(F64) - od.pae_bins().double()).abs().max()) < 31.75 * 2.0 ** -23
    for (L, counts, sc), (lg, tk, ref) in pae_refs.items():
        aa = tk < dr.MASK_ID
        pae = od.compute_predicted_aligned_error(lg, aa)
        ptm = od.compute_tm(lg, aa)
        assert _passes(dr.ratio(pae, ref[0], F32, dr.PAE_COEF * dr.PAE_UNIT)), (L, counts, sc)
        assert _passes(dr.ratio(ptm, ref[2], F32, dr.TM_COEF * dr.F32_EPS)), (L, counts, sc)
        # what the GPU test asserts of the kernel holds of the reference: masked pairs at the mean centre, special rows and
        # samples without a valid token at 0
        sq = aa[:, :, None] & aa[:, None, :]
        assert float((ref[0][~sq] - dr.pae_centres(F64).mean()).abs().max() if (~sq).any() else 0.0) < 1e-12
        assert float(ref[1][~aa].abs().max()) == 0.0
        for b, n in enumerate(counts):
            assert (float(ref[2][b]) == 0.0) == (n == 0)


def test_pair_feature_statement_is_the_oracle_heads_input():
    qk = torch.randn(2, 7, 128, generator=torch.Generator().manual_seed(1))
    head = od.PairwisePredictionHeadRef(128)
    with torch.no_grad():
        head.downproject.weight.copy_(torch.eye(128))
    seen = []
    head.linear1.register_forward_pre_hook(lambda m, a: seen.append(a[0]))
    with torch.no_grad():
        head(qk)
    assert torch.equal(seen[0], dr.pair_features_expected(qk))
    # bfloat16: one float32 operation on the bf16 operands, rounded once; feature (i, j) is q_j with k_i
    q16 = qk.bfloat16()
    X = dr.pair_features_expected(q16)
    assert X.dtype == torch.bfloat16 and X[1, 2, 5, 3] == (q16[1, 5, 3].float() * q16[1, 2, 64 + 3].float()).bfloat16()
    assert X[1, 2, 5, 64 + 3] == (q16[1, 5, 3].float() - q16[1, 2, 64 + 3].float()).bfloat16()


def test_neighbourhood_statement_is_the_oracle_gather():
    ca, has = dr.knn_lattice_case(64, "gaps+known")
    edges = knn_edges(ca, has, dr.KNN)
    g = torch.Generator().manual_seed(2)
    table, rot, trans = torch.randn(66, 8, generator=g), torch.randn(2, 64, 3, 3, generator=g), torch.randn(2, 64, 3, generator=g)
    x, nrot, ntrans, nmask = dr.neighbourhood_expected(edges, table, rot, trans, has, 32)
    emb = nn.Embedding(66, 8)
    with torch.no_grad():
        emb.weight.copy_(table)
        diff = (edges - edges[..., :1]).clamp(-32, 32) + 33                    # oracle.encoder_ref, StructureTokenEncoderRef.forward
        assert torch.equal(x, emb(diff))
    b, i, e = 0, 40, 7
    j = int(edges[b, i, e])
    assert torch.equal(nrot[b, i, e], rot[b, j]) and torch.equal(ntrans[b, i, e], trans[b, j]) and int(nmask[b, i, e]) == int(has[b, j])


# ---------------------------------------------------------------------------------------------------------------
# planted errors
def test_backbone_bar_rejects_a_flipped_axis_and_e2_cannot_reach_the_output():
    v = dr.backbone_case(257, 0)
    ref, unit = dr.backbone_formula(v, 10.0, F64), dr.backbone_unit(v, 10.0)
    # e2 with the opposite sign: the ideal N, CA, C all have z = 0 (oracle.decoder_ref.BB_COORDINATES), so e2 is multiplied
    # by zero and no comparison of backbone atoms can see its sign.  Stated here so that nobody counts on it.
    assert all(row[2] == 0.0 for row in od.BB_COORDINATES)
    assert torch.equal(dr.backbone_formula(v, 10.0, F64, e2_sign=-1.0), ref)
    # what can go wrong in the frame and be seen: e1 with the opposite sign (N mirrored through the x axis) ...
    bad = dr.backbone_formula(v, 10.0, F64, e1_sign=-1.0)
    r = dr.ratio(bad.float(), ref, F32, dr.BACKBONE_COEF * unit)
    assert not _passes(r) and _passes(r[:, 1:])                               # only N moves, and its bond length does not:
    assert float((dr.bond_lengths(bad) - dr.bond_lengths(ref)).abs().max()) < 1e-9
    # ... trans scaled twice, x and y swapped, the 1e-5 missing from the normalisation of a short axis
    twice = ref + (v[:, None, 0:3].double() * 10.0) * 9.0
    assert not _passes(dr.ratio(twice.float(), ref, F32, dr.BACKBONE_COEF * unit))
    sw = v.clone()
    sw[:, 3:6], sw[:, 6:9] = v[:, 6:9], v[:, 3:6]
    assert not _passes(dr.ratio(dr.backbone_formula(sw, 10.0, F64).float(), ref, F32, dr.BACKBONE_COEF * unit))


def test_plddt_bar_rejects_centres_at_the_bin_edges():
    for M in (1, 257):
        p = dr.plddt_case(M, 0)
        ref = dr.plddt_formula(p, F64)
        bad = dr.plddt_formula(p, F64, centre_offset=0.0)                       # i / n instead of (i + 0.5) / n
        assert not _passes(dr.ratio(bad.float(), ref, F32, dr.PLDDT_COEF * dr.F32_EPS))
        assert _passes(dr.ratio(ref.float(), ref, F32, dr.PLDDT_COEF * dr.F32_EPS))


def _pae_ratios(got, ref):
    return (dr.ratio(got[0].float(), ref[0], F32, dr.PAE_COEF * dr.PAE_UNIT), dr.ratio(got[1].float(), ref[1], F32, dr.TM_COEF * dr.F32_EPS),
            dr.ratio(got[2].float(), ref[2], F32, dr.TM_COEF * dr.F32_EPS))


def test_pae_and_tm_bars_reject_the_planted_errors(pae_refs):
    lg, tk, ref = pae_refs[(33, (18, 19), 1.0)]
    assert all(_passes(r) for r in _pae_ratios(ref, ref))
    # the last bin centre half a step off: PAE moves everywhere; the TM rows and pTM where d0 is large enough for a pair
    # 31.75 A off to count (255 valid tokens: d0 = 5.9, the last bin weighs 0.03; at 18 tokens 3e-5)
    bad = dr.pae_tm_formula(lg, tk, F64, last_shift_steps=-0.5)
    assert not _passes(_pae_ratios(bad, ref)[0])
    lg2, tk2, ref2 = pae_refs[(258, (255,), 1.0)]
    assert not any(_passes(r) for r in _pae_ratios(dr.pae_tm_formula(lg2, tk2, F64, last_shift_steps=-0.5), ref2))
    # d0 without the clamp at 19: only the sample with 18 valid tokens can tell, in its TM rows and pTM
    bad = dr.pae_tm_formula(lg, tk, F64, clamp=False)
    r = _pae_ratios(bad, ref)
    assert _passes(r[0]) and not _passes(r[1][0]) and _passes(r[1][1]) and not _passes(r[2][:1]) and _passes(r[2][1:])
    # TM averaged over L instead of over the valid count
    r = _pae_ratios(dr.pae_tm_formula(lg, tk, F64, mean_over_L=True), ref)
    assert _passes(r[0]) and not _passes(r[1]) and not _passes(r[2])
    # a masked pair left unmasked: valid row 1 with the special token at L // 2
    aa = tk < dr.MASK_ID
    i = int(aa[0].nonzero()[0])
    assert not bool(aa[0, 33 // 2])
    r = _pae_ratios(dr.pae_tm_formula(lg, tk, F64, unmask=(0, i, 33 // 2)), ref)
    assert not _passes(r[0]) and float(r[0][0, i, 33 // 2]) > 1 and _passes(r[0][1])
    # the same plants on the bin sweep (17 valid tokens: below the clamp)
    lg, tk, bins = dr.pae_sweep_case()
    ref = dr.pae_tm_formula(lg, tk, F64)
    bad = dr.pae_tm_formula(lg, tk, F64, last_shift_steps=0.5)
    assert float((bad[0] - ref[0]).abs().max()) > dr.SWEEP_PAE_ABS
    bad = dr.pae_tm_formula(lg, tk, F64, clamp=False)
    assert not _passes(_pae_ratios(bad, ref)[1])


# ---------------------------------------------------------------------------------------------------------------
# the exact comparisons of the GPU test hold of the reference alone
@pytest.mark.parametrize("pattern", dr.KNN_PATTERNS)
def test_lattice_knn_is_the_same_in_float32_and_float64(pattern):
    for L in dr.KNN_L:
        ca, has = dr.knn_lattice_case(L, pattern)
        e32, e64 = knn_edges(ca, has, dr.KNN), knn_edges(ca.double(), has, dr.KNN)
        assert torch.equal(e32, e64), L
        assert e32.shape == (2, L, min(dr.KNN, L)) and torch.equal(e32[..., 0], torch.arange(L).expand(2, L))
        # the keys of this file are the oracle's: a stable sort of them gives the same neighbours
        assert torch.equal(dr.knn_keys64(ca, has).sort(dim=-1, stable=True)[1][..., :dr.KNN], e64)
        if pattern == "known+none":
            assert torch.equal(e64[1], dr.all_unknown_order(L, min(dr.KNN, L)))
        elif pattern == "gaps+known":
            assert not bool(has[0, L - 1]) and (L < 3 or not bool(has[0, L // 3]))


def test_lattice_fixture_has_ties_and_offsets_beyond_the_clamp():
    ca, has = dr.knn_lattice_case(300, "known+none")
    k = dr.knn_keys64(ca, has)[0]
    srt = k.sort(dim=-1)[0][:, :dr.KNN]
    assert float((srt[:, 1:] == srt[:, :-1]).double().mean()) > 0.5             # ties abound among the 16 nearest
    e = knn_edges(ca.double(), has, dr.KNN)[0]
    off = e - e[:, :1]
    assert int(off.min()) < -32 and int(off.max()) > 32
    # the walk is self-avoiding and connected
    pts = {tuple(p) for p in (ca[0] / dr.LATTICE_SCALE).round().int().tolist()}
    assert len(pts) == 300 and float((ca[0, 1:] - ca[0, :-1]).norm(dim=-1).sub(dr.LATTICE_SCALE).abs().max()) == 0.0


def test_wide_lattice_fixture_ties_two_keys_of_one_kernel_thread():
    """The kernel's tie rule is written twice: in a thread's scan over keys j, j + 256, ... and in the reduction across
    threads.  Only a tie between residues 256 apart, both among a residue's 16 nearest, reaches the first; the narrow folds
    (contacts at most 49 apart) and the all-unknown sample (i +- 8) have none, the wide folds at L = 300 do."""
    for pattern, expect in (("known+none", False), ("gaps+known", False), ("wide", True)):
        ca, has = dr.knn_lattice_case(300, pattern)
        e, k = knn_edges(ca.double(), has, dr.KNN), dr.knn_keys64(ca, has)
        for b in (0, 1):
            pairs = dr.tied_pairs_one_block_apart(e[b], k[b])
            assert bool(pairs) == expect, (pattern, b, pairs[:3])
            # ... and the oracle lists the lower index of such a pair first
            assert all(e[b, i].tolist().index(j) < e[b, i].tolist().index(j + dr.KNN_BLOCK) for i, j in pairs)


def test_a_lattice_scaled_by_3_8_would_not_be_exact():
    """Why LATTICE_SCALE is 3.75: with 3.8 equal lattice distances are unequal float32 numbers a few ulp apart, and float32
    and float64 evaluations of the oracle already order them differently, so no kernel could be held to either."""
    ca, has = dr.knn_lattice_case(64, "known+none", scale=3.8)
    assert not torch.equal(knn_edges(ca, has, dr.KNN), knn_edges(ca.double(), has, dr.KNN))
    # what can be held at 3.8 (and the GPU test holds): differences only between keys that agree to 2^-22 in float64
    for L in (64, 300):
        for pattern in dr.KNN_PATTERNS:
            ca, has = dr.knn_lattice_case(L, pattern, scale=3.8)
            share, far = dr.knn_unexplained(knn_edges(ca, has, dr.KNN), knn_edges(ca.double(), has, dr.KNN), dr.knn_keys64(ca, has))
            assert far == 0 and share > 0, (L, pattern)


def test_random_knn_differs_from_float64_only_at_near_ties():
    ca, has = dr.knn_random_case()
    e64 = knn_edges(ca.double(), has, dr.KNN)
    share, far = dr.knn_unexplained(knn_edges(ca, has, dr.KNN), e64, dr.knn_keys64(ca, has))
    print("MEASURED float32 knn vs float64: differing share", share)
    assert far == 0 and share <= 0.01
    swapped = e64.clone()
    swapped[0, 5, 3], swapped[0, 5, 9] = e64[0, 5, 9], e64[0, 5, 3]          # two neighbours out of order: not a near tie
    assert dr.knn_unexplained(swapped, e64, dr.knn_keys64(ca, has))[1] == 2


@pytest.mark.parametrize("n_codes", dr.CODE_N)
def test_integer_codebook_argmin_is_the_same_in_float32_and_float64(n_codes):
    for R in dr.CODE_R:
        z, code, has, pairs = dr.code_integer_case(R, n_codes)
        t32, t64 = dr.nearest_code_formula(z, code, has, F32), dr.nearest_code_formula(z, code, has, F64)
        assert torch.equal(t32, t64)
        assert torch.equal(dr.code_d2(z, code, F32).double(), dr.code_d2(z, code, F64))      # exact sums
        assert bool((t64[~has] == dr.MASK_ID).all())
        low = {b: a for a, b in pairs}
        assert not any(int(t) in low for t in t64[has])                        # never the upper copy of a duplicated row
        if pairs:
            assert int(t64[0]) == pairs[0][0] and float(dr.code_d2(z[:1], code, F64)[0, pairs[0][1]]) == 0.0
    if n_codes > 256:                                                          # duplicates on both sides of a multiple of 256
        assert any(a // 256 != b // 256 for a, b in pairs) and any((b - a) % 256 == 0 for a, b in pairs)
        assert any(a % 256 > b % 256 for a, b in pairs) and any(a % 256 < b % 256 for a, b in pairs)


def test_random_codebook_differs_from_float64_only_at_near_ties():
    z, code, has = dr.code_random_case()
    t32 = dr.nearest_code_formula(z, code, has, F32)
    share, far = dr.code_unexplained(t32, z, code, has)
    print("MEASURED float32 nearest code vs float64: differing share", share)
    assert far == 0 and share <= 0.01
    # the sum of squared differences is the oracle's |z|^2 - 2 z.e + |e|^2
    zz, ee = z.double(), code.double()
    d2 = (zz ** 2).sum(-1, keepdim=True) - 2 * zz @ ee.t() + (ee ** 2).sum(-1)[None]
    assert torch.equal(d2.argmin(-1), dr.nearest_code_formula(z, code, has, F64))
    wrong = dr.nearest_code_formula(z, code, has, F64)
    wrong[3] = (wrong[3] + 1) % 4096
    assert dr.code_unexplained(wrong, z, code, has)[1] == 1


# ---------------------------------------------------------------------------------------------------------------
def test_decoder_end_entry_points_refuse_bad_arguments_before_touching_a_device():
    from esmdiff_amd import _native as N
    lib = N.lib()
    fake = 4096                                                                # never dereferenced: refused first
    assert lib.esmdiff_dim6_to_backbone(None, 23, fake, 4, 10.0, None) == -1
    assert lib.esmdiff_dim6_to_backbone(fake, 23, None, 4, 10.0, None) == -1
    assert lib.esmdiff_dim6_to_backbone(fake, 23, fake, 0, 10.0, None) == -1
    assert lib.esmdiff_dim6_to_backbone(fake, 8, fake, 4, 10.0, None) == -1
    assert lib.esmdiff_plddt_mean(None, 50, 50, fake, 4, None) == -1
    assert lib.esmdiff_plddt_mean(fake, 49, 50, fake, 4, None) == -1
    assert lib.esmdiff_plddt_mean(fake, 50, 0, fake, 4, None) == -1
    assert lib.esmdiff_plddt_mean(fake, 50, 50, fake, -1, None) == -1
    for dtype, nb, L in ((1, 1, 4), (3, 1, 4), (-1, 1, 4), (0, 0, 4), (2, 1, 0), (0, 3, 30000)):
        assert lib.esmdiff_pair_features(fake, dtype, fake, nb, L, None) == -1, (dtype, nb, L)
    assert lib.esmdiff_pair_features(None, 0, fake, 1, 4, None) == -1
    assert lib.esmdiff_pair_features(fake, 1, fake, 1, 4, None) == -1 and "f16" in lib.esmdiff_last_error(None).decode()
    for bad in (dict(logits=None), dict(tokens=None), dict(tm=None), dict(ptm=None), dict(nb=0), dict(L=0), dict(max_bin=0.0),
                dict(nb=3, L=30000)):
        a = dict(logits=fake, tokens=fake, tm=fake, pae=None, ptm=fake, nb=1, L=4, max_bin=31.0)
        a.update(bad)
        assert lib.esmdiff_pae_tm(a["logits"], a["tokens"], a["tm"], a["pae"], a["ptm"], a["nb"], a["L"], a["max_bin"], None) == -1, bad
    assert lib.esmdiff_decoder_set_pair_chunk_bytes(None, 1 << 20) == -1
    assert lib.esmdiff_encoder_knn(None, fake, 1, 4, 16, fake, None) == -1
    for B, L, knn in ((0, 4, 16), (1, 0, 16), (1, 4, 0), (1, 8193, 16)):
        assert lib.esmdiff_encoder_knn(fake, fake, B, L, knn, fake, None) == -1, (B, L, knn)
    assert "8192" in lib.esmdiff_encoder_last_error(None).decode()
    nb = lambda **kw: lib.esmdiff_encoder_neighbourhood(  # noqa: E731
        kw.get("edges", fake), fake, fake, fake, fake, kw.get("B", 1), kw.get("L", 8), kw.get("K", 4), kw.get("D", 16),
        kw.get("bins", 32), kw.get("x", fake), fake, fake, fake, None)
    for bad in (dict(edges=None), dict(x=None), dict(B=0), dict(L=0), dict(K=0), dict(K=9), dict(D=0), dict(D=6), dict(bins=0)):
        assert nb(**bad) == -1, bad
    assert lib.esmdiff_encoder_nearest_code(None, fake, fake, 1, 16, 128, fake, None) == -1
    for R, n, d in ((0, 16, 128), (1, 0, 128), (1, 16, 0), (1, 16, 8193)):
        assert lib.esmdiff_encoder_nearest_code(fake, fake, fake, R, n, d, fake, None) == -1, (R, n, d)

"""What a create does to a state dict, and the input stage, one launcher at a time and then whole (tests/loader_ref.py holds the
references; tests/test_loader_cpu.py shows that the comparators reject planted errors).

A bfloat16 checkpoint reaches the ESMDIFF_BF16 branch of every conversion kernel (csrc/convert.hip: to_bf16 / to_f32 /
interleave_swiglu; csrc/gemm_split.hip: weight_absmax / split_weight with the FFN-up interleave; csrc/attention_split.hip:
rownorm_max).  No other test creates anything from a bfloat16 tensor, and a whole-forward bar of 0.03 on the logits cannot see a
row kernel of the input stage (csrc/embed.hip, the 16-bit-input LayerNorm of csrc/norm.hip) go subtly wrong.

Conversions, the interleave, the split, embed and gather are determined bit for bit: their asserts are equality of the integer
views (lr.all_same_bits: a NaN matches any NaN).  Three results carry float32 arithmetic: the row-norm maximum and the sigma MLP
under bars derived from their operation counts, the LayerNorm under tests/rowwise_ref.py's bar; each prints the measured ratio."""
import ctypes

import pytest
import torch

from tests import loader_ref as lr
from tests import rowwise_ref as rr

pytestmark = pytest.mark.gpu

NAME = {torch.bfloat16: "bf16", torch.float16: "f16", torch.float32: "f32"}
SRC = (torch.float32, torch.bfloat16)
MASK = 4096


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4096 * 256 + 1])
@pytest.mark.parametrize("src", SRC, ids=lambda d: NAME[d])
def test_convert_weight_bit_for_bit(src, n):
    """to_bf16_kernel (bf16 and f16 builds) and to_f32_kernel from a float32 and from a bfloat16 source, bit for bit against
    torch: round to nearest even into bfloat16 (overflow to inf), clamp to +-65504 then round into float16, exact into float32.
    The float32 source walks lr.f32_pool() (ties, neighbours of ties, the saturation edge, f16 subnormal ties, signed zeros,
    denormals, NaNs, 4 000 normals), the bfloat16 source all 65 536 patterns; n = 4096 x 256 + 1 is the first size at which the
    grid-stride loop takes a second trip.  The element after dst[n - 1] is never written.

    NaN weights: a NaN source gives a NaN in every destination type.  This test found the f16 build turning every NaN, quiet or
    signalling, into +-65504 on an MI355X (0 of 2 072 float32 NaNs and 0 of 4 064 bfloat16 NaNs kept: the clamp's v_med3_f32
    answers a NaN operand with a bound), while the bfloat16 and float32 destinations kept all of them; convert.hip's cv_f2bf now
    passes a NaN around the clamp.  +-inf saturating to +-65504 in float16 is the contract and is asserted here.
    float32 denormals (the only inputs where a signed zero is accepted beside torch's value): the MI355X gives torch's value, 0
    of 2 590 denormal inputs flushed in any destination type."""
    from esmdiff_amd.engine import convert_weight
    x = lr.tile_pool(lr.f32_pool() if src == torch.float32 else lr.bf16_pool(), n)
    den = lr.is_f32_denormal(x) if src == torch.float32 else None
    xd = x.cuda()
    for dst in (torch.bfloat16, torch.float16, torch.float32):
        out = torch.full((n + 8,), 7.0, dtype=dst, device="cuda")
        convert_weight(xd, dst, out=out)
        got, want = out[:n].cpu(), lr.convert_ref(x, dst)
        nan_in = torch.isnan(x.float())
        kept = int(torch.isnan(got.float())[nan_in].sum())
        flushed = int(((lr.bits(got) != lr.bits(want)) & den).sum()) if den is not None else 0
        print(f"MEASURED convert {NAME[src]} -> {NAME[dst]} n={n}: NaN kept {kept} of {int(nan_in.sum())}; "
              f"denormal inputs flushed {flushed} of {int(den.sum()) if den is not None else 0}")
        bad = (~lr.same_bits(got, want, den)).nonzero().flatten()[:4].tolist()
        assert lr.all_same_bits(got, want, den), (NAME[dst], [(hex(int(lr.bits(x)[i]) & 0xffffffff), float(got[i]), float(want[i])) for i in bad])
        assert bool((out[n:] == 7.0).all()), NAME[dst]


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,K", [(32, 64), (64, 320), (96, 512)])
def test_interleave_swiglu_bit_for_bit(H, K):
    """interleave_swiglu_kernel, both builds, from both source dtypes: dst rows in blocks of 32, [gate 32t..32t+31 | up
    32t..32t+31], each element converted as convert_weight converts it.  K = 64 leaves three quarters of the block idle, 320 is
    one full trip of 256 threads plus a partial one, 512 two full trips; H = 96: an odd number of block pairs."""
    from esmdiff_amd.engine import interleave_swiglu
    g = torch.Generator().manual_seed(H + K)
    w = 0.05 * torch.randn(2 * H, K, generator=g)
    w[5, 3], w[H + 7, K - 1] = 7.0e4, -7.0e4                                   # beyond float16: saturates in the f16 build
    for src in SRC:
        ws = w.to(src)
        for dst in (torch.bfloat16, torch.float16):
            got = interleave_swiglu(ws.cuda(), dst).cpu()
            want = lr.interleave_ref(ws, dst)
            bad = (~lr.same_bits(got, want)).any(-1).nonzero().flatten()[:4].tolist()
            assert lr.all_same_bits(got, want), (NAME[src], NAME[dst], "rows", bad)


def test_interleave_swiglu_refuses_h_not_a_multiple_of_32():
    from esmdiff_amd import _native as N
    lib = N.lib()
    src = torch.ones(2 * 48, 64, device="cuda")
    out = torch.full((2 * 48, 64), 7.0, dtype=torch.bfloat16, device="cuda")
    for H, K, sdt, kind in ((48, 64, 0, 0), (16, 64, 0, 1), (0, 64, 0, 0), (32, 0, 0, 0), (32, 64, 2, 0), (32, 64, 0, 2)):
        assert lib.esmdiff_interleave_swiglu(src.data_ptr(), sdt, out.data_ptr(), kind, H, K, None) == -1, (H, K, sdt, kind)
    torch.cuda.synchronize()
    assert bool((out.float() == 7.0).all())


# ---------------------------------------------------------------------------------------------------------------
def _just_below(v: float, dtype) -> float:
    """The largest number of `dtype` below the power of two v."""
    b = lr.bits(torch.tensor([v], dtype=dtype)) - 1
    return float(b.view(dtype)[0])


def _weight_matrix(kind, N, K, src, seed):
    """[N, K] of dtype `src`: N(0, 0.05) clamped to +-0.1, then by kind: "pow2" one element exactly 2^-3 (the matrix maximum),
    "below" that element just below 2^-3 in `src`'s own format, "neg" the maximum magnitude carried by a negative element, "zero"
    all zeros, "nan" one NaN among ordinary values."""
    g = torch.Generator().manual_seed(seed)
    w = (0.05 * torch.randn(N, K, generator=g)).clamp(-0.1, 0.1).to(src)
    r, c = N - 3, K - 5
    if kind == "pow2":
        w[r, c] = 2.0 ** -3
    elif kind == "below":
        w[r, c] = _just_below(2.0 ** -3, src)
    elif kind == "neg":
        w[r, c] = -0.3
    elif kind == "zero":
        w.zero_()
    elif kind == "nan":
        w[r, c] = float("nan")
    else:
        assert kind == "random"
    return w


@pytest.mark.parametrize("N,n_pad,K", [(256, 256, 128), (300, 512, 384), (128, 256, 128)])
@pytest.mark.parametrize("src", SRC, ids=lambda d: NAME[d])
def test_split_weight_bit_for_bit(src, N, n_pad, K):
    """weight_absmax_kernel + split_weight_kernel from both source dtypes, with and without the FFN-up row interleave, bit for
    bit (w3 and 2^-k) against lr.split_weight_ref: maximum exactly a power of two / just below one (the scale's exponent
    changes between the two), a negative maximum, an all-zero matrix (finite 2^-k, an all-zero w3), one NaN element (the scale
    ignores it; its three planes are NaN).  Rows N .. n_pad - 1 come back zero."""
    from esmdiff_amd.engine import split_weight_from
    for kind in ("random", "pow2", "below", "neg", "zero", "nan"):
        w = _weight_matrix(kind, N, K, src, seed=N + K)
        for ih in (0, N // 2):
            if ih and ih % 32:
                continue
            got, inv = split_weight_from(w.cuda(), interleave_h=ih, n_pad=n_pad)
            want, want_inv = lr.split_weight_ref(w, n_pad, ih)
            assert inv == want_inv and inv > 0, (kind, ih, inv, want_inv)
            got = got.cpu()
            bad = (~lr.same_bits(got, want)).any(-1).nonzero().flatten()[:4].tolist()
            assert lr.all_same_bits(got, want), (kind, ih, "rows", bad)
            assert bool((lr.bits(got[N:]) == 0).all())
    # the two scale cases really differ by one exponent
    assert lr.weight_scale_exponent(_weight_matrix("below", N, K, src, 1)) == lr.weight_scale_exponent(_weight_matrix("pow2", N, K, src, 1)) + 1


def test_split_weight_of_a_converted_weight_and_the_f32_entry():
    """f32 -> bf16 on the device, then split from bfloat16, equals the split of w.bfloat16().float() handed over as float32;
    esmdiff_split_weight (the float32 entry kept for the GEMM tests) is the new entry with ESMDIFF_F32 and no interleave; a bad
    interleave_h is refused and touches nothing."""
    from esmdiff_amd import _native as N
    from esmdiff_amd.engine import convert_weight, split_weight, split_weight_from
    w = _weight_matrix("random", 256, 384, torch.float32, seed=9)
    w16 = convert_weight(w.cuda(), torch.bfloat16)
    assert lr.all_same_bits(w16.cpu(), w.bfloat16())
    for ih in (0, 128):
        a, ia = split_weight_from(w16, interleave_h=ih)
        b, ib = split_weight_from(w.bfloat16().float().cuda(), interleave_h=ih)
        assert ia == ib and torch.equal(lr.bits(a), lr.bits(b)), ih
    a, ia = split_weight(w.cuda())
    b, ib = split_weight_from(w.cuda())
    assert ia == ib and torch.equal(lr.bits(a), lr.bits(b))
    lib = N.lib()
    out = torch.full((256, 3 * 384), 7.0, dtype=torch.float16, device="cuda")
    inv = ctypes.c_float(5.0)
    wd = w.cuda()
    for ih in (100, 64, -128, 96):
        assert lib.esmdiff_split_weight_from(wd.data_ptr(), 0, out.data_ptr(), 256, 256, 384, ih, ctypes.byref(inv)) == -1, ih
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and inv.value == 5.0


@pytest.mark.parametrize("r0,rows,K", [(0, 1, 64), (128, 5, 320), (512, 256, 256)])
def test_weight_rownorm_max_vs_float64(r0, rows, K):
    """rownorm_max_kernel over rows r0 .. r0 + rows - 1 (the rows around them carry 10x larger norms: a wrong range shows)
    against float64 under lr.rownorm_bar = (K / 64 + 8) 2^-24 relative + one ulp; a bfloat16 source gives the bits of its
    float32 image.  Measured on an MI355X: ratio to the bar 0.003 - 0.046; every error within the one ulp, so the coefficient
    needed of the relative term is 0.00 (9 - 13 allowed)."""
    from esmdiff_amd.engine import weight_rownorm_max
    g = torch.Generator().manual_seed(r0 + rows + K)
    w = torch.randn(r0 + rows + 4, K, generator=g) * (1 + torch.rand(r0 + rows + 4, 1, generator=g))
    w[:r0] *= 10
    w[r0 + rows:] *= 10
    for src in SRC:
        ws = w.to(src)
        got = weight_rownorm_max(ws.cuda(), r0, rows)
        ref = lr.rownorm_max_ref(ws, r0, rows)
        bar = lr.rownorm_bar(ref, K)
        ulp = bar - (K / 64 + 8) * lr.F32_EPS * ref
        need = max(0.0, abs(got - ref) - ulp) / (lr.F32_EPS * ref)
        print(f"MEASURED rownorm_max r0={r0} rows={rows} K={K} {NAME[src]}: ratio {abs(got - ref) / bar:.3f}, coef needed {need:.2f} "
              f"of {K / 64 + 8:.0f}")
        assert abs(got - ref) <= bar, (NAME[src], got, ref, bar)
        if src == torch.bfloat16:
            assert got == weight_rownorm_max(ws.float().cuda(), r0, rows)


# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tables():
    """E_seq [64, D], E_struct [4101, D], c [D] per width, made once."""
    made = {}

    def get(D):
        if D not in made:
            g = torch.Generator().manual_seed(D)
            made[D] = tuple(t.cuda() for t in (torch.randn(64, D, generator=g), torch.randn(4101, D, generator=g),
                                               torch.randn(D, generator=g)))
        return made[D]
    return get


# (seq, xtok) of the rows a forward over valid ids never feeds: the forcing from the sequence track over an ordinary structure
# id, -1 -> MASK, the structure clamp on both sides, the sequence clamp on both sides (-3 clamps to BOS and forces)
EDGE_ROWS = [(0, 17), (1, 17), (2, 17), (31, 17), (7, -1), (7, -7), (7, 4096), (7, 5000), (-3, 17), (64, 17)]


def _embed_ids(B, L, seed, first_edge=0):
    g = torch.Generator().manual_seed(seed)
    seq = torch.randint(4, 24, (B * L,), generator=g)
    xtok = torch.randint(0, 4096, (B * L,), generator=g)
    for i, (s, t) in enumerate(EDGE_ROWS[first_edge:first_edge + B * L]):
        seq[i], xtok[i] = s, t
    return seq.view(B, L), xtok.view(B, L)


@pytest.mark.parametrize("D", [256, 1536, 2048])
@pytest.mark.parametrize("B,L", [(1, 1), (3, 5)])
def test_embed_rows_bit_for_bit(tables, B, L, D):
    """embed_kernel bit for bit against ((E_seq[s] + E_struct[t']) + c) + cond in torch float32: D = 256 is one partial trip of
    the 1024-column loop, 1536 one full and one partial, 2048 two full; no cond, one cond vector for all samples (stride 0), one
    per sample (stride D, all different).  The first ten rows are EDGE_ROWS; at (1, 1) each of them is its own launch."""
    from esmdiff_amd.engine import embed_rows
    e_seq, e_struct, cvec = tables(D)
    cond = torch.randn(B, D, generator=torch.Generator().manual_seed(B + D))
    host = [t.cpu() for t in (e_seq, e_struct, cvec)]
    for first in (range(len(EDGE_ROWS) + 1) if B * L == 1 else (0,)):
        seq, xtok = _embed_ids(B, L, seed=D + first, first_edge=first)
        for c, stride in ((None, 0), (cond[1 % B:1 % B + 1].contiguous(), 0), (cond, D)):
            got = embed_rows(seq.cuda(), xtok.cuda(), e_seq, e_struct, cvec, None if c is None else c.cuda(), stride).cpu()
            want = lr.embed_ref(seq, xtok, *host, c, stride)
            bad = (~lr.same_bits(got, want)).any(-1).nonzero()[:4].tolist()
            assert lr.all_same_bits(got, want), (first, c is None, stride, "rows", bad)


def test_gather_table_rows_bit_for_bit():
    """gather_rows_kernel: out = table[tok], ids below 0 and at n_rows clamped into the table; D = 4 (one lane), 768 (the tiny
    decoder's width), 2048 (two trips)."""
    from esmdiff_amd.engine import gather_table_rows
    for D in (4, 768, 2048):
        table = torch.randn(37, D, generator=torch.Generator().manual_seed(D))
        tok = torch.tensor([0, 36, -1, 37, 5, -9, 1000, 5, 12], dtype=torch.int64)
        got = gather_table_rows(tok.cuda(), table.cuda()).cpu()
        assert lr.all_same_bits(got, lr.gather_ref(tok, table)), D


@pytest.mark.parametrize("n_sigma", [1, 3])
@pytest.mark.parametrize("D", [6, 512, 1536])
def test_sigma_mlp_vs_float64(D, n_sigma):
    """gemv_kernel<true> + gemv_kernel<false> (the time-conditioning MLP) against float64.  Bars from the operation count
    (lr.sigma_mlp_ref): (K / 64 + 8) 2^-24 (sum |w x| + |b|) per dot product, 1.1 of the first layer's bar plus 6 x 2^-24 |silu|
    through the activation, the hidden vector's bar through |W2|; the second layer also alone, from the kernel's own hidden
    vector.  D = 6: the last block's waves 2 and 3 have no output (the n >= N guard).  Measured on an MI355X: hidden ratio
    0.015 - 0.045 (coefficient needed 0.00 - 0.14 of the 12 allowed), cond ratio 0.001 - 0.007, second layer alone 0.011 - 0.137
    (coefficient needed 1.11 of 8.1 at D = 6, 0.32 - 0.41 of 16 / 32 at D = 512 / 1536)."""
    from esmdiff_amd.engine import sigma_mlp
    F = 256
    g = torch.Generator().manual_seed(D + n_sigma)
    x = 2 * torch.rand(n_sigma, F, generator=g) - 1                              # a sinusoid embedding lives in [-1, 1]
    w1, b1 = torch.randn(D, F, generator=g) / 16, 0.1 * torch.randn(D, generator=g)
    w2, b2 = torch.randn(D, D, generator=g) / D ** 0.5, 0.1 * torch.randn(D, generator=g)
    hidden, cond = (t.cpu() for t in sigma_mlp(*(t.cuda() for t in (x, w1, b1, w2, b2))))
    ref = lr.sigma_mlp_ref(x, w1, b1, w2, b2)
    rh = lr.bar_ratio(hidden, ref["hidden"], ref["hidden_bar"])
    rc = lr.bar_ratio(cond, ref["cond"], ref["cond_bar"])
    r2, u2 = lr.second_layer_ref(hidden, w2, b2)
    ra = lr.bar_ratio(cond, r2, lr.dot_coef(D) * u2)
    over = ((hidden.double() - ref["hidden"]).abs() - lr.SILU_COEF * lr.F32_EPS * ref["hidden"].abs()).clamp(min=0)
    need1 = float((over / (lr.SILU_SLOPE * ref["unit1"])).max())
    need2 = float(((cond.double() - r2).abs() / u2).max())
    print(f"MEASURED sigma_mlp D={D} n_sigma={n_sigma}: hidden ratio {float(rh.max()):.3f} (coef needed {need1:.2f} of {lr.dot_coef(F):.0f}), "
          f"cond ratio {float(rc.max()):.3f}, second layer alone {float(ra.max()):.3f} (coef needed {need2:.2f} of {lr.dot_coef(D):.1f})")
    assert lr.passes(rh), float(rh.max())
    assert lr.passes(ra), float(ra.max())
    assert lr.passes(rc), float(rc.max())


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [128, 512, 768, 1536, 2048])
def test_layernorm_16in_vs_float64(D):
    """layernorm_kernel<NV, IN_BF16 = true> in the bf16 and the f16 build (the head's LayerNorm after GELU, the pLDDT and
    pairwise heads' LayerNorms) on M = 1, 5, 1027 rows with and without the bias, the last row low-variance, under the bar of
    test_add_layernorm_vs_float64 (rr.ratio with rr.LN_COEF: the arithmetic is the same).  Measured on an MI355X: ratio
    0.995 - 0.998 in both builds (the output rounding dominates), coefficient needed 0.00 - 0.65 of the 4 allowed."""
    from esmdiff_amd.engine import layernorm_16in
    worst = {}
    for M in (1, 5, 1027):
        for dtype in (torch.bfloat16, torch.float16):
            x16, w, b = lr.ln16_case(M, D, dtype, seed=D + M)
            xd, wd, bd = x16.cuda(), w.cuda(), b.cuda()
            for bias in (bd, None):
                y = layernorm_16in(xd, wd, bias)
                ref, unit = rr.add_ln_ref64(xd.float(), wd, bias)
                r = float(rr.ratio(y, ref, dtype, rr.LN_COEF * unit).max())
                wst = worst.setdefault(NAME[dtype], [0.0, 0.0])
                wst[0], wst[1] = max(wst[0], r), max(wst[1], rr.needed_coef(y, ref, dtype, unit))
                assert r <= 1.0, (M, NAME[dtype], bias is None, r)
    print(f"MEASURED layernorm_16in D={D} " + " ".join(f"{k}: ratio {v[0]:.3f} coef {v[1]:.2f}" for k, v in worst.items()))


def test_layernorm_16in_refuses_bad_widths():
    from esmdiff_amd import _native as N
    lib = N.lib()
    x = torch.full((4, 2304), 3.0, dtype=torch.bfloat16, device="cuda")
    w = torch.ones(2304, device="cuda")
    y = torch.full((4, 2304), 7.0, dtype=torch.bfloat16, device="cuda")
    for dtype, M, D in ((0, 4, 130), (1, 4, 130), (0, 4, 2052), (1, 4, 2304), (0, 4, 0), (0, 0, 256), (2, 4, 256), (0, 4, -4)):
        assert lib.esmdiff_layernorm_16in(dtype, x.data_ptr(), w.data_ptr(), None, y.data_ptr(), M, D, None) == -1, (dtype, M, D)
    torch.cuda.synchronize()
    assert bool((y.float() == 7.0).all())


# ---------------------------------------------------------------------------------------------------------------
# Whole creates from a bfloat16 checkpoint: an object made from {k: v.bfloat16()} must return the bits of one made from
# {k: v.bfloat16().float()} — the loader's ESMDIFF_BF16 branches against its ESMDIFF_F32 ones on the same values.
def _bf16(sd):
    return {k: (v.bfloat16() if v.is_floating_point() else v) for k, v in sd.items()}


def _bf16_image(sd):
    return {k: (v.bfloat16().float() if v.is_floating_point() else v) for k, v in sd.items()}


def _forward_inputs(B, L):
    g = torch.Generator().manual_seed(L)
    seq = torch.cat([torch.tensor([0]), torch.randint(4, 24, (L - 2,), generator=g), torch.tensor([2])])[None].repeat(B, 1)
    x = torch.full((B, L), MASK, dtype=torch.int64)
    x[:, 5:20] = torch.randint(0, 4096, (B, 15), generator=g)
    return x, seq


SHAPES = [(2, 60), (5, 258)]


def _logits(eng):
    from esmdiff_amd.schedule import ddpm_schedule
    tf = ddpm_schedule(25).t_freq[6]
    out = []
    for B, L in SHAPES:
        x, seq = _forward_inputs(B, L)
        out.append(eng.forward_logits(x.cuda(), seq.cuda(), tf).cpu())
    return out


@pytest.fixture(scope="module")
def tiny_sd():
    from esmdiff_amd.config import TINY
    from esmdiff_amd.weights import random_init_state_dict
    return random_init_state_dict(TINY, seed=1)


@pytest.fixture(scope="module")
def f32_logits(tiny_sd):
    """The float32 engine made from the float32 image of the bfloat16 dict: the reference of the odd-dict tests."""
    from esmdiff_amd.config import TINY
    from esmdiff_amd.engine import Engine
    eng = Engine(TINY, _bf16_image(tiny_sd), max_batch=5, max_len=258, precision="f32")
    out = _logits(eng)
    eng.close()
    return out


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(lr.bits(a.float()), lr.bits(b.float()))


@pytest.mark.parametrize("precision,head", [("bf16", None), ("f16", None), ("f32", None), ("f32_split", None), ("bf16", "f32")])
def test_engine_from_a_bf16_state_dict_equals_its_f32_image(tiny_sd, precision, head):
    """forward_logits at (2, 60) and (5, 258) — the small-batch and the regular path — bit for bit in every precision, and the
    attention scales an f32_split create picks per layer from the row norms of the qkv weight."""
    from esmdiff_amd.config import TINY
    from esmdiff_amd.engine import Engine
    res = []
    for sd in (_bf16(tiny_sd), _bf16_image(tiny_sd)):
        eng = Engine(TINY, sd, max_batch=5, max_len=258, precision=precision, head_precision=head)
        res.append((_logits(eng), [eng.attention_scales(i) for i in range(TINY.n_layers)] if precision == "f32_split" else None))
        eng.close()
    (a, sa), (b, sb) = res
    assert sa == sb
    for (B, L), la, lb in zip(SHAPES, a, b):
        assert bool(torch.isfinite(la).all()) and float(la.float().std()) > 0.1, (B, L)
        assert _same(la, lb), (precision, head, B, L, float((la.float() - lb.float()).abs().max()))


def test_engine_from_mixed_odd_dtype_and_strided_state_dicts(tiny_sd, f32_logits):
    """Against the float32 engine of the float32 image: every second tensor bfloat16; tensors as float16 (where that holds the
    value exactly) or float64 (the host's .float() branch); 2-D tensors as non-contiguous views."""
    from esmdiff_amd.config import TINY
    from esmdiff_amd.engine import Engine
    img = _bf16_image(tiny_sd)
    mixed = {k: (v.bfloat16() if i % 2 else v) for i, (k, v) in enumerate(img.items())}
    odd = {k: (v.half() if torch.equal(v.half().float(), v) else v.double()) for k, v in img.items()}
    assert {v.dtype for v in odd.values()} == {torch.float16, torch.float64}
    strided = {k: (v.t().contiguous().t() if v.dim() == 2 else v) for k, v in img.items()}
    assert any(not v.is_contiguous() for v in strided.values())
    for name, sd in (("mixed", mixed), ("f16 / f64", odd), ("strided", strided)):
        eng = Engine(TINY, sd, max_batch=5, max_len=258, precision="f32")
        got = _logits(eng)
        eng.close()
        for (B, L), la, lb in zip(SHAPES, got, f32_logits):
            assert _same(la, lb), (name, B, L, float((la.float() - lb.float()).abs().max()))


def test_bf16_engine_from_a_bf16_state_dict_vs_oracle(tiny_sd):
    """The pair of engines above tied to the reference network: the bf16 engine made from the bfloat16 dict against
    oracle.esm3_ref on the float32 image, at the bars of test_forward_logits_vs_oracle.  Measured on an MI355X: max 0.0098,
    mean 0.00157."""
    from esmdiff_amd.config import TINY
    from esmdiff_amd.engine import Engine
    from esmdiff_amd.schedule import ddpm_schedule
    from oracle.esm3_ref import build_from_state_dict
    net, emb = build_from_state_dict(TINY, _bf16_image(tiny_sd))
    eng = Engine(TINY, _bf16(tiny_sd), max_batch=2, max_len=60)
    B, L = 2, 60
    x, seq = _forward_inputs(B, L)
    sch = ddpm_schedule(25)
    with torch.no_grad():
        cond = torch.tile(emb(sch.sigma_t[6] * torch.ones(B))[:, None, :], (1, L, 1))
        ref = net(structure_tokens=x, sequence_tokens=seq, auxiliary_embeddings=cond).structure_logits
    got = eng.forward_logits(x.cuda(), seq.cuda(), sch.t_freq[6]).float().cpu()
    eng.close()
    err = (got - ref).abs()
    cos = torch.nn.functional.cosine_similarity(got.flatten(), ref.flatten(), dim=0)
    print(f"MEASURED bf16 engine from a bf16 dict vs oracle: max {float(err.max()):.4f} mean {float(err.mean()):.5f} cos {float(cos):.6f}")
    assert float(cos) > 0.9999, float(cos)
    assert float(err.max()) < 0.03 and float(err.mean()) < 4.5e-3, (float(err.max()), float(err.mean()))
    assert float((got.argmax(-1) == ref.argmax(-1)).float().mean()) > 0.96


@pytest.mark.parametrize("precision", ["bf16", "f32", "f32_split"])
def test_decoder_from_a_bf16_state_dict_equals_its_f32_image(precision):
    """Backbone, pLDDT, pTM and PAE of a (2, 33) decode, bit for bit in every precision the decoder accepts."""
    from esmdiff_amd.config import TINY_DECODER
    from esmdiff_amd.engine import StructureDecoder
    from esmdiff_amd.weights import random_init_decoder_state_dict
    sd = random_init_decoder_state_dict(TINY_DECODER, seed=2)
    B, L = 2, 33
    g = torch.Generator().manual_seed(33)
    tok = torch.randint(0, 4096, (B, L), generator=g)
    tok[:, 0], tok[:, -1] = 4098, 4097
    res = []
    for d in (_bf16(sd), _bf16_image(sd)):
        dec = StructureDecoder(TINY_DECODER, d, max_batch=B, max_len=L, precision=precision)
        res.append([t.cpu() for t in dec.decode(tok.cuda(), return_plddt=True, return_ptm=True, return_pae=True)])
        dec.close()
    for name, a, b in zip(("coords", "plddt", "ptm", "pae"), *res):
        assert bool(torch.isfinite(a).all()), name
        assert _same(a, b), (precision, name, float((a - b).abs().max()))


@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_encoder_from_a_bf16_state_dict_equals_its_f32_image(precision):
    """The tokens of a (2, 33) encode, equal in both precisions the encoder accepts."""
    from esmdiff_amd.config import TINY_ENCODER
    from esmdiff_amd.engine import StructureEncoder
    from esmdiff_amd.weights import random_init_encoder_state_dict
    sd = random_init_encoder_state_dict(TINY_ENCODER, seed=6)
    B, L = 2, 33
    g = torch.Generator().manual_seed(33)
    ca = torch.cumsum(torch.randn(B, L, 3, generator=g) * 2.2, 1)
    xyz = torch.stack([ca + torch.randn(B, L, 3, generator=g) * 0.8, ca, ca + torch.randn(B, L, 3, generator=g) * 0.8], 2)
    xyz[0, 5:8] = float("inf")
    res = []
    for d in (_bf16(sd), _bf16_image(sd)):
        enc = StructureEncoder(TINY_ENCODER, d, precision=precision)
        res.append(enc.encode(xyz).cpu())
        enc.close()
    assert torch.equal(res[0], res[1]), (precision, int((res[0] != res[1]).sum()))
    assert len(set(res[0][res[0] != MASK].tolist())) > 8                          # tokens, not one constant

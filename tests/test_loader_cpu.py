"""The references and comparators of tests/test_gpu_loader.py (tests/loader_ref.py) on the CPU: each reference gives the values
its contract names, each comparator passes the reference itself and rejects the planted error a kernel of that kind could
carry without a whole-forward bar noticing.  Also: the new test entries refuse bad arguments without touching a device."""
import ctypes
import struct

import pytest
import torch

from tests import loader_ref as lr
from tests import rowwise_ref as rr


def _f32(bits_):
    return lr.from_bits([bits_], torch.float32)


def _b16(t):
    return int(lr.bits(t)[0]) & 0xffff


# ---------------------------------------------------------------------------------------------------------------
def test_conversion_references_give_the_quoted_values():
    bf = lambda b: _b16(lr.convert_ref(_f32(b), torch.bfloat16))
    assert bf(0x3f808000) == 0x3f80 and bf(0x3f818000) == 0x3f82                  # ties to even
    assert bf(0x3f807fff) == 0x3f80 and bf(0x3f808001) == 0x3f81
    assert bf(0x3f817fff) == 0x3f81 and bf(0x3f818001) == 0x3f82
    assert bf(0x7f7fffff) == 0x7f80 and bf(0xff7fffff) == 0xff80                  # overflow to inf
    h = lambda v: float(lr.convert_ref(v if isinstance(v, torch.Tensor) else torch.tensor([v], dtype=torch.float32), torch.float16)[0])
    assert h(_f32(0x7f7fffff)) == 65504.0 and h(float("inf")) == 65504.0 and h(float("-inf")) == -65504.0
    assert h(65504.0) == 65504.0 and h(65519.9) == 65504.0 and h(65520.0) == 65504.0
    assert h(2.0 ** -25) == 0.0 and h(3 * 2.0 ** -26) == 2.0 ** -24 and h(3 * 2.0 ** -25) == 2.0 ** -23
    assert _b16(lr.convert_ref(torch.tensor([-0.0]), torch.float16)) == 0x8000
    for dst in (torch.bfloat16, torch.float16, torch.float32):
        assert bool(torch.isnan(lr.convert_ref(torch.tensor([float("nan")]), dst)).all())
    pats = lr.f32_patterns()
    for v, want in ((65504.0, 0x477fe000), (65519.9, 0x477fefe6), (65520.0, 0x477ff000), (2.0 ** -25, 0x33000000),
                    (3 * 2.0 ** -26, 0x33400000), (3 * 2.0 ** -25, 0x33c00000), (2.0 ** -14, 0x38800000)):
        assert struct.unpack("<I", struct.pack("<f", v))[0] == want and want in pats, v
    # bf16 -> f32 is exact; bf16 -> bf16 the identity, on every pattern
    pool = lr.bf16_pool()
    assert pool.numel() == 65536 and len(set(lr.bits(pool).tolist())) == 65536
    assert lr.all_same_bits(lr.convert_ref(pool, torch.bfloat16), pool)
    assert lr.all_same_bits(lr.convert_ref(lr.convert_ref(pool, torch.float32), torch.bfloat16), pool)
    den = lr.is_f32_denormal(lr.from_bits([0x00000001, 0x007fffff, 0x00800000, 0, 0x80000001], torch.float32))
    assert den.tolist() == [True, True, False, False, True]


def test_conversion_comparator_rejects_truncation_and_missing_saturation():
    pool = lr.f32_pool()
    want = lr.convert_ref(pool, torch.bfloat16)
    assert lr.all_same_bits(want.clone(), want)
    trunc = lr.convert_truncating_bf16(pool)
    assert not lr.all_same_bits(trunc, want)
    tie = lr.from_bits([0x3f818000], torch.float32)                               # the tie with an odd kept bit alone tells
    assert not lr.all_same_bits(lr.convert_truncating_bf16(tie), lr.convert_ref(tie, torch.bfloat16))
    even = lr.from_bits([0x3f808000], torch.float32)                              # (the even one truncates to the right answer)
    assert lr.all_same_bits(lr.convert_truncating_bf16(even), lr.convert_ref(even, torch.bfloat16))
    want16 = lr.convert_ref(pool, torch.float16)
    assert lr.all_same_bits(want16.clone(), want16)
    assert not lr.all_same_bits(pool.half(), want16)                              # unsaturated: 65520 and inf become inf
    big = torch.tensor([65520.0])
    assert not lr.all_same_bits(big.half(), lr.convert_ref(big, torch.float16))
    # a NaN matches any NaN and nothing else; a NaN turned into a finite bound is rejected
    nan = lr.from_bits([0x7fc00000, 0x7f800001], torch.float32)
    assert lr.all_same_bits(lr.from_bits([0x7e01, 0xfe00], torch.float16), lr.convert_ref(nan, torch.float16))
    assert not lr.all_same_bits(torch.tensor([-65504.0, 65504.0]).half(), lr.convert_ref(nan, torch.float16))
    # the denormal allowance: a zero of the right sign, on denormal inputs only
    den = lr.from_bits([0x00400000, 0x80400000, 0x3f800000], torch.float32)
    w = lr.convert_ref(den, torch.bfloat16)
    mask = lr.is_f32_denormal(den)
    assert lr.all_same_bits(torch.tensor([0.0, -0.0, 1.0]).bfloat16(), w, mask)
    assert not lr.all_same_bits(torch.tensor([-0.0, -0.0, 1.0]).bfloat16(), w, mask)      # wrong sign
    assert not lr.all_same_bits(torch.tensor([0.0, -0.0, 0.0]).bfloat16(), w, mask)       # a normal input flushed
    assert not lr.all_same_bits(torch.tensor([0.0, -0.0, 1.0]).bfloat16(), w)             # no allowance without the mask


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,K", [(32, 64), (64, 320), (96, 512)])
def test_interleave_reference_and_its_comparator(H, K):
    w = torch.randn(2 * H, K, generator=torch.Generator().manual_seed(H))
    out = lr.interleave_rows(w)
    for rho in range(2 * H):                                                       # the sentence, row by row
        t, up, j = rho // 64, (rho // 32) % 2, rho % 32
        assert torch.equal(out[rho], w[(H if up else 0) + 32 * t + j]), rho
    for dst in (torch.bfloat16, torch.float16):
        want = lr.interleave_ref(w, dst)
        assert lr.all_same_bits(lr.interleave_ref(w.bfloat16(), dst), lr.interleave_ref(w.bfloat16().float(), dst))
        assert not lr.all_same_bits(lr.interleave_ref(w, dst, swap_blocks=(0, 1)), want)   # gate and up of one hidden block
        if H > 32:
            assert not lr.all_same_bits(lr.interleave_ref(w, dst, swap_blocks=(1, 3)), want)   # two up blocks


def test_split_weight_reference_and_its_comparator():
    g = torch.Generator().manual_seed(3)
    N, n_pad, K = 300, 512, 128
    w = (0.05 * torch.randn(N, K, generator=g)).clamp(-0.1, 0.1)
    for amax, k in ((2.0 ** -3, 17), (2.0 ** -3 * (1 - 2.0 ** -24), 18), (1.0, 14), (3.0e4, 0), (2.0 ** 14, 0)):
        w[7, 5] = amax
        assert lr.weight_scale_exponent(w) == k, amax
        w3, inv = lr.split_weight_ref(w, n_pad)
        hi = w3[:N, K:2 * K].float()
        assert inv == 2.0 ** -k and 2.0 ** 14 <= float(hi.abs().max()) <= 2.0 ** 15
        assert torch.equal(w3[:N, K:2 * K], w3[:N, 2 * K:]) and bool((w3[N:] == 0).all())
        # hi + lo restores w 2^k to 2^-22 relative (or f16's subnormal spacing)
        a = w.double() * 2.0 ** k
        assert bool(((hi.double() + w3[:N, :K].double() - a).abs() <= rr.split_bar(a)).all())
    assert lr.weight_scale_exponent(torch.zeros(4, 4)) == 14 - (20 - 127)
    z3, zinv = lr.split_weight_ref(torch.zeros(256, 128), 256)
    assert bool((z3 == 0).all()) and zinv == 2.0 ** (20 - 127 - 14) and zinv > 0
    wn = w.clone()
    wn[11, 3] = float("nan")
    assert lr.weight_scale_exponent(wn) == lr.weight_scale_exponent(w)             # the scale ignores the NaN
    n3, _ = lr.split_weight_ref(wn, n_pad)
    assert int(torch.isnan(n3).sum()) == 3 and lr.all_same_bits(n3.clone(), n3)
    want, _ = lr.split_weight_ref(w, n_pad)
    swapped, _ = lr.split_weight_ref(w, n_pad, exchange=True)
    assert not lr.all_same_bits(swapped, want)                                     # hi and lo exchanged
    wi = 0.05 * torch.randn(128, K, generator=g)
    plain, _ = lr.split_weight_ref(wi, 256)
    inter, _ = lr.split_weight_ref(wi, 256, interleave_h=64)
    assert not lr.all_same_bits(plain, inter)
    assert lr.all_same_bits(inter, lr.split_weight_ref(lr.interleave_rows(wi), 256)[0])


def test_rownorm_bar():
    w = torch.randn(64, 320, generator=torch.Generator().manual_seed(4))
    ref = lr.rownorm_max_ref(w, 8, 40)
    f32 = float(w[8:48].pow(2).sum(-1).sqrt().max())                               # torch float32 sits inside the bar
    assert abs(f32 - ref) <= lr.rownorm_bar(ref, 320)
    assert abs(ref * (1 + 16 * rr.F32_EPS) - ref) > lr.rownorm_bar(ref, 320)       # (320 / 64 + 8 = 13) + 1 ulp (<= 2) < 16
    assert abs(lr.rownorm_max_ref(w, 8, 39) - ref) > lr.rownorm_bar(ref, 320) or int(w[8:48].pow(2).sum(-1).argmax()) != 39


# ---------------------------------------------------------------------------------------------------------------
def _embed_case(B, L, D, seed):
    g = torch.Generator().manual_seed(seed)
    e_seq, e_struct = torch.randn(64, D, generator=g), torch.randn(4101, D, generator=g)
    cvec, cond = torch.randn(D, generator=g), torch.randn(B, D, generator=g)
    seq = torch.randint(4, 24, (B, L), generator=g)
    xtok = torch.randint(0, 4096, (B, L), generator=g)
    return seq, xtok, e_seq, e_struct, cvec, cond


def test_embed_reference_rules_and_its_comparator():
    B, L, D = 3, 5, 256
    seq, xtok, e_seq, e_struct, cvec, cond = _embed_case(B, L, D, 5)
    s, t = lr.embed_ids(torch.tensor([[0, 1, 2, 31, 7, 7, 7, 7, 7, -3, 64]]), torch.tensor([[5, 5, 5, 5, -1, -7, 4096, 5000, 4100, 9, 9]]))
    assert s.tolist() == [[0, 1, 2, 31, 7, 7, 7, 7, 7, 0, 63]]
    assert t.tolist() == [[4098, 4099, 4097, 4100, 4096, 0, 4096, 4100, 4100, 4098, 9]]
    want = lr.embed_ref(seq, xtok, e_seq, e_struct, cvec, cond, D)
    for b in range(B):
        for l in range(L):
            assert torch.equal(want[b, l], ((e_seq[seq[b, l]] + e_struct[xtok[b, l]]) + cvec) + cond[b])
    assert torch.equal(lr.embed_ref(seq, xtok, e_seq, e_struct, cvec, None, 0), (e_seq[seq] + e_struct[xtok]) + cvec)
    assert torch.equal(lr.embed_ref(seq, xtok, e_seq, e_struct, cvec, cond, 0), (e_seq[seq] + e_struct[xtok] + cvec) + cond[0])
    assert lr.all_same_bits(want.clone(), want)
    assert not lr.all_same_bits(lr.embed_ref(seq, xtok, e_seq, e_struct, cvec, cond, D, cond_by_row_mod_b=True), want)
    # at (B, L) = (1, 1) the two indexings coincide: the planted error needs B > 1 and L > 1 to show
    one = _embed_case(1, 1, D, 6)
    assert lr.all_same_bits(lr.embed_ref(*one, D, cond_by_row_mod_b=True), lr.embed_ref(*one, D))
    table = torch.randn(9, 8)
    assert torch.equal(lr.gather_ref(torch.tensor([-1, 0, 8, 9]), table), table[[0, 0, 8, 8]])


@pytest.mark.parametrize("D", [6, 512])
def test_sigma_mlp_bar_passes_float32_and_rejects_four_bars(D):
    g = torch.Generator().manual_seed(D)
    F, n = 256, 3
    x = torch.randn(n, F, generator=g)
    w1, b1 = torch.randn(D, F, generator=g) / 16, 0.1 * torch.randn(D, generator=g)
    w2, b2 = torch.randn(D, D, generator=g) / D ** 0.5, 0.1 * torch.randn(D, generator=g)
    ref = lr.sigma_mlp_ref(x, w1, b1, w2, b2)
    hid32 = torch.nn.functional.silu(x @ w1.T + b1)
    cond32 = hid32 @ w2.T + b2
    assert lr.passes(lr.bar_ratio(hid32, ref["hidden"], ref["hidden_bar"]))
    assert lr.passes(lr.bar_ratio(cond32, ref["cond"], ref["cond_bar"]))
    r2, u2 = lr.second_layer_ref(hid32, w2, b2)
    assert lr.passes(lr.bar_ratio(cond32, r2, lr.dot_coef(D) * u2))
    for key in ("hidden", "cond"):
        bad = ref[key].clone()
        bad[1, D // 2] += 4 * ref[key + "_bar"][1, D // 2]
        r = lr.bar_ratio(bad, ref[key], ref[key + "_bar"])
        assert not lr.passes(r) and int((r > 1).sum()) == 1
    assert lr.dot_coef(256) == 12 and lr.dot_coef(1536) == 32


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_ln16_bar_passes_the_rounded_reference_and_rejects_eps(dtype):
    x16, w, b = lr.ln16_case(5, 768, dtype, 7)
    ref, _ = rr.add_ln_ref64(x16.float(), w, b)
    assert lr.passes(lr.ln16_ratio(ref.to(dtype), x16, w, b))
    eps6, _ = rr.add_ln_ref64(x16.float(), w, b, eps=1e-6)
    r = lr.ln16_ratio(eps6.to(dtype), x16, w, b)
    assert not lr.passes(r[-1:]) and lr.passes(r[:-1])                             # only the low-variance row can tell
    nob, _ = rr.add_ln_ref64(x16.float(), w, None)
    assert not lr.passes(lr.ln16_ratio(nob.to(dtype), x16, w, b))                  # a dropped bias


# ---------------------------------------------------------------------------------------------------------------
def test_loader_entry_points_refuse_bad_arguments_before_touching_a_device():
    from esmdiff_amd import _native as N
    lib = N.lib()
    fake = 4096                                                                    # never dereferenced: refused first
    inv = ctypes.c_float(0)
    for bad in ((None, 0, fake, 0, 4), (fake, 0, None, 0, 4), (fake, 2, fake, 0, 4), (fake, -1, fake, 0, 4), (fake, 0, fake, 3, 4),
                (fake, 0, fake, -1, 4), (fake, 0, fake, 0, 0), (fake, 0, fake, 0, -5)):
        assert lib.esmdiff_convert_weight(*bad, None) == -1, bad
    for bad in ((None, 0, fake, 0, 32, 64), (fake, 0, None, 0, 32, 64), (fake, 2, fake, 0, 32, 64), (fake, 0, fake, 2, 32, 64),
                (fake, 0, fake, 0, 48, 64), (fake, 0, fake, 0, 0, 64), (fake, 0, fake, 0, 32, 0), (fake, 0, fake, 0, -32, 64)):
        assert lib.esmdiff_interleave_swiglu(*bad, None) == -1, bad
    assert "32" in lib.esmdiff_last_error(None).decode()
    for bad in ((None, 0, fake, 256, 256, 128, 0), (fake, 0, None, 256, 256, 128, 0), (fake, 2, fake, 256, 256, 128, 0),
                (fake, 0, fake, 0, 256, 128, 0), (fake, 0, fake, 300, 256, 128, 0), (fake, 0, fake, 256, 300, 128, 0),
                (fake, 0, fake, 256, 256, 100, 0), (fake, 1, fake, 256, 256, 128, 100), (fake, 1, fake, 256, 256, 128, 64),
                (fake, 0, fake, 256, 256, 128, -128), (fake, 0, fake, 200, 256, 128, 100)):
        assert lib.esmdiff_split_weight_from(*bad, ctypes.byref(inv)) == -1, bad
    assert lib.esmdiff_split_weight_from(fake, 0, fake, 256, 256, 128, 0, None) == -1
    assert lib.esmdiff_split_weight(None, fake, 256, 256, 128, ctypes.byref(inv)) == -1
    for bad in ((None, 0, 0, 4, 64), (fake, 2, 0, 4, 64), (fake, 0, -1, 4, 64), (fake, 0, 0, 0, 64), (fake, 0, 0, 4, 0)):
        assert lib.esmdiff_weight_rownorm_max(*bad, ctypes.byref(inv)) == -1, bad
    assert lib.esmdiff_weight_rownorm_max(fake, 0, 0, 4, 64, None) == -1

    def embed(**kw):
        a = dict(seq=fake, xtok=fake, e_seq=fake, e_struct=fake, cvec=fake, cond=None, cs=0, out=fake, B=1, L=2, D=256)
        a.update(kw)
        return lib.esmdiff_embed_rows(a["seq"], a["xtok"], a["e_seq"], a["e_struct"], a["cvec"], a["cond"], a["cs"], a["out"], a["B"],
                                      a["L"], a["D"], None)
    for bad in ({"seq": None}, {"xtok": None}, {"e_seq": None}, {"e_struct": None}, {"cvec": None}, {"out": None}, {"B": 0}, {"L": 0},
                {"D": 0}, {"D": 258}, {"cs": -4}, {"cs": 6}, {"B": 65536, "L": 65536}):
        assert embed(**bad) == -1, bad
    for bad in ((None, fake, fake, 4, 8, 9), (fake, None, fake, 4, 8, 9), (fake, fake, None, 4, 8, 9), (fake, fake, fake, 0, 8, 9),
                (fake, fake, fake, 4, 6, 9), (fake, fake, fake, 4, 0, 9), (fake, fake, fake, 4, 8, 0)):
        assert lib.esmdiff_gather_table_rows(*bad, None) == -1, bad
    ok = [fake] * 7 + [256, 512, 1]
    for i in range(7):
        assert lib.esmdiff_sigma_mlp(*[None if j == i else v for j, v in enumerate(ok)], None) == -1, i
    for F, D, n in ((0, 512, 1), (256, 0, 1), (256, 512, 0), (256, 512, 65536)):
        assert lib.esmdiff_sigma_mlp(*([fake] * 7), F, D, n, None) == -1, (F, D, n)
    for bad in ((2, fake, fake, None, fake, 4, 256), (-1, fake, fake, None, fake, 4, 256), (0, None, fake, None, fake, 4, 256),
                (0, fake, None, None, fake, 4, 256), (0, fake, fake, None, None, 4, 256), (0, fake, fake, None, fake, 0, 256),
                (0, fake, fake, None, fake, 4, 0), (1, fake, fake, None, fake, 4, 130), (1, fake, fake, None, fake, 4, 2052)):
        assert lib.esmdiff_layernorm_16in(*bad, None) == -1, bad
    assert "2048" in lib.esmdiff_last_error(None).decode()

"""The comparator of tests/test_gpu_attention16.py (tests/rowwise_ref.py: attention16_*) must let the 16-bit attention kernel's own
arithmetic through and stop the errors a flash-style kernel with a lazy rescale can carry.  The arithmetic: attention16_emulate,
the tile loop of csrc/attention_kernel.inc in torch (float32 scores, 64-key tiles, one raise decision per wave of 32 queries,
16-bit P, float32 O and l), on every case the GPU test runs; ATT16_COEF is re-derived here from its figures.  The errors: O or l
left at the old scale on a raise, the last key dropped, the clamped key of a partial tail counted.  Unit-size rows, the only
regime the attention tests had before, cannot see the first: that is asserted too.  Last: esmdiff_attention_16_parts refuses bad
arguments without touching a device."""
import ctypes
import math

import pytest
import torch

from tests import rowwise_ref as rr

DTYPES = [torch.bfloat16, torch.float16]
RESCALE_KINDS = ("gain4", "gain8", "stairs_up", "stairs_up7", "one_key", "last_key", "lone_query")


def _pow2_ceil(v: float) -> float:
    return 2.0 ** math.ceil(math.log2(v))


def _case(kind, B, L, H, dtype, lens=None):
    q, k, v = rr.attention_case(kind, B, L, H, seed=L, lens=lens)
    ops = rr.attention16_operands(q, k, v, dtype)
    ref, unit = rr.attention16_ref64(*ops, B, L, H, dtype, lens=lens)
    return ops, ref, unit


def _flat_ok(got, qkv16, B, L, H, dtype) -> bool:
    """got [B*L, H*64] against the float64 mean of the V rows of its sample: OUT_EPS |mean| + ATT16_FLAT_ABS max|v|."""
    v = qkv16[:, 2 * H * 64:].double().view(B, L, H * 64)
    mean = v.mean(1, keepdim=True)
    bar = rr.OUT_EPS[dtype] * mean.abs() + rr.ATT16_FLAT_ABS * v.abs().amax()
    return bool(((got.double().view(B, L, H * 64) - mean).abs() <= bar).all())


@pytest.fixture(scope="module")
def emulated():
    """Per dtype: the largest needed_coef of the unplanted emulation per kind over every launch of the GPU test, and where."""
    out = {}
    for dtype in DTYPES:
        worst = {}
        lens = list(rr.ATT16_RAGGED_LENS)
        runs = [(B, H, L, kinds, None) for B, H, L, kinds in rr.attention16_runs()]
        runs.append((len(lens), rr.ATT16_RAGGED_H, max(lens), rr.ATT16_RAGGED_KINDS, lens))
        for B, H, L, kinds, ln in runs:
            for kind in kinds:
                ops, ref, unit = _case(kind, B, L, H, dtype, ln)
                got = rr.attention16_emulate(*ops, B, L, H, dtype, lens=ln)
                assert bool(torch.isfinite(got.float()).all()), (dtype, kind, B, H, L)
                r = float(rr.ratio(got, ref, dtype, rr.ATT16_COEF_BUILD[dtype] * unit).max())
                assert r <= 1.0, (dtype, kind, B, H, L, ln is not None, r)
                if kind == "flat":
                    assert _flat_ok(got, ops[2], B, L, H, dtype), (dtype, B, H, L)
                need = rr.needed_coef(got, ref, dtype, unit)
                if need >= worst.get(kind, (0.0,))[0]:
                    worst[kind] = (need, B, H, L, ln is not None)
        out[dtype] = worst
    return out


def test_the_emulation_passes_every_case_and_sets_the_coefficient(emulated):
    """The unplanted emulation is within each build's bar in every kind, at every (B, H, L) of the GPU test and in its ragged
    batch (asserted while the fixture runs), needs at most a quarter of ATT16_COEF, and ATT16_COEF is 4 x its largest need
    rounded up to a power of two.  The bf16 build's own coefficient follows the same rule from the bf16 figures."""
    top = {}
    for dtype, worst in emulated.items():
        for kind, w in sorted(worst.items()):
            print(f"MEASURED attention16 emulation {str(dtype)[6:]} {kind}: coef {w[0]:.2f} at B H L = {w[1:4]}{' ragged' if w[4] else ''}")
        top[dtype] = max(w[0] for w in worst.values())
    need = max(top.values())
    print(f"MEASURED attention16 emulation: bf16 {top[torch.bfloat16]:.2f}, f16 {top[torch.float16]:.2f}; 4x -> {_pow2_ceil(4 * need):g}")
    assert need <= rr.ATT16_COEF / 4 and _pow2_ceil(4 * need) == rr.ATT16_COEF, (need, rr.ATT16_COEF)
    for dtype in DTYPES:
        assert top[dtype] <= rr.ATT16_COEF_BUILD[dtype] <= rr.ATT16_COEF
        assert rr.ATT16_COEF_BUILD[dtype] <= _pow2_ceil(4 * top[dtype]), (dtype, top[dtype])   # not wider than the rule gives it
    assert rr.ATT16_COEF_BUILD[torch.float16] == rr.ATT16_COEF


def test_the_cases_reach_the_regimes_their_names_promise():
    """What the emulation's own counters say at L = 258, B H = 16 (4 tiles and a HALF tail after each wave's first): unit rows never
    raise the maximum again; neither do the falling staircases; the 7-nat rising staircase raises it at every tile; the 5-nat one
    lags (P above 2^7, never above 2^8) and raises at about every second tile; gains of 4 and 8 raise it at most tiles; one
    aligned query per wave is enough to raise it for all 32 (lone_query)."""
    B, H, L = 2, 8, 258
    st = {}
    for kind in rr.ATT16_KINDS:
        ops, _, _ = _case(kind, B, L, H, torch.bfloat16)
        st[kind] = {}
        rr.attention16_emulate(*ops, B, L, H, torch.bfloat16, stats=st[kind])
    frac = {k: s["raises"] / s["tiles"] for k, s in st.items()}
    for kind in ("unit", "stairs_down", "stairs_down7", "first_key", "flat"):
        assert frac[kind] == 0, (kind, frac[kind])
    assert frac["stairs_up7"] == 1
    assert 0.4 <= frac["stairs_up"] <= 0.6 and 2.0 ** 7 < st["stairs_up"]["pmax"] <= 2.0 ** rr.ATT16_THR
    assert frac["gain4"] > 0.5 and frac["gain8"] > 0.5 and frac["lone_query"] > 0.75
    assert frac["one_key"] == 0.25 and frac["last_key"] == 0.25             # at the heavy key's tile alone: tile 2, the tail
    assert all(s["pmax"] <= 2.0 ** rr.ATT16_THR for s in st.values())
    # without the aligned queries the same keys raise the maximum less than a quarter as often: the lone lane trips its wave
    q, k, v = rr.attention_case("lone_query", B, L, H, seed=L)
    q0, _, _ = rr.attention_case("unit", B, L, H, seed=L)
    s0 = {}
    rr.attention16_emulate(*rr.attention16_operands(q0, k, v, torch.bfloat16), B, L, H, torch.bfloat16, stats=s0)
    assert s0["raises"] < 0.25 * st["lone_query"]["raises"], (s0, st["lone_query"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_unit_rows_cannot_see_a_missing_rescale(dtype):
    """Why this file exists: on N(0, 1) rows no tile's maximum exceeds the first tile's by 8 log2 units, the maximum is raised once
    and a kernel that never rescales O (or l) computes the very same bits: the plant passes at every L and (B, H)."""
    for L in rr.ATT16_LS:
        for B, H in rr.ATT_BH:
            ops, ref, unit = _case("unit", B, L, H, dtype)
            good = rr.attention16_emulate(*ops, B, L, H, dtype)
            for plant in ("no_o_rescale", "no_l_rescale"):
                st = {}
                bad = rr.attention16_emulate(*ops, B, L, H, dtype, plant=plant, stats=st)
                assert st.get("raises", 0) == 0 and torch.equal(bad.view(torch.int16), good.view(torch.int16)), (plant, L, B, H)
                assert float(rr.ratio(bad, ref, dtype, rr.ATT16_COEF_BUILD[dtype] * unit).max()) <= 1.0, (plant, L, B, H)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_bar_rejects_a_missing_rescale_in_the_sharp_regimes(dtype):
    """no_o_rescale and no_l_rescale are rejected, under the wider ATT16_COEF, in every kind built for them wherever a tile after
    the first raises the maximum: at L = 129 and 258 (3 and 5 tiles, both HALF tails) in all seven kinds, and at L = 65 (HALF
    tail) and 97 (MASKED tail) in the kinds that raise it in the second tile by construction — there the 5-nat staircase is
    still one step (7.2 log2 units) under the threshold, and one_key's key 2L/3 lies in tile 0.  B H = 1 and 16."""
    for plant in ("no_o_rescale", "no_l_rescale"):
        worst = {}
        for L in (65, 97, 129, 258):
            for kind in (RESCALE_KINDS if L > 128 else ("stairs_up7", "last_key", "lone_query")):
                for B, H in ((1, 1), (2, 8)):
                    ops, ref, unit = _case(kind, B, L, H, dtype)
                    bad = rr.attention16_emulate(*ops, B, L, H, dtype, plant=plant)
                    r = float(rr.ratio(bad, ref, dtype, rr.ATT16_COEF * unit).max())
                    worst[kind] = min(worst.get(kind, r), r)
                    assert r > 1.0, (plant, kind, L, B, H, r)
        print(f"MEASURED attention16 {plant} {str(dtype)[6:]}: smallest worst ratio per kind " +
              ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_bar_rejects_a_dropped_last_key_and_a_tail_key_counted_twice(dtype):
    """drop_last_key in unit, gain4, stairs_up7 and last_key at every L of the GPU test from 31 up (B H = 16); tail_key_twice at
    L = 33, 65, 97 and 258 (tails of 1, 1, 33 and 2 keys) on unit rows through the bar and on flat rows through the mean of V,
    which needs no reference."""
    B, H = 2, 8
    for L in rr.ATT16_LS[1:]:
        for kind in ("unit", "gain4", "stairs_up7", "last_key"):
            ops, ref, unit = _case(kind, B, L, H, dtype)
            bad = rr.attention16_emulate(*ops, B, L, H, dtype, plant="drop_last_key")
            assert float(rr.ratio(bad, ref, dtype, rr.ATT16_COEF * unit).max()) > 1.0, (kind, L)
    for L in (33, 65, 97, 258):
        for B, H in ((1, 1), (2, 8)):
            ops, ref, unit = _case("unit", B, L, H, dtype)
            bad = rr.attention16_emulate(*ops, B, L, H, dtype, plant="tail_key_twice")
            assert float(rr.ratio(bad, ref, dtype, rr.ATT16_COEF * unit).max()) > 1.0, ("unit", L, B, H)
            ops, _, _ = _case("flat", B, L, H, dtype)
            assert _flat_ok(rr.attention16_emulate(*ops, B, L, H, dtype), ops[2], B, L, H, dtype), (L, B, H)
            assert not _flat_ok(rr.attention16_emulate(*ops, B, L, H, dtype, plant="tail_key_twice"), ops[2], B, L, H, dtype), (L, B, H)


def test_ragged_reference_and_emulation_are_each_sample_at_its_own_length():
    """With lens, reference, unit and emulation are those of every sample alone; padded rows are (0, 0) and +0; last_key's heavy
    key is the sample's own last valid one."""
    lens = list(rr.ATT16_RAGGED_LENS)
    B, L, H, dtype = len(lens), max(lens), rr.ATT16_RAGGED_H, torch.bfloat16
    ops, ref, unit = _case("last_key", B, L, H, dtype, lens)
    got = rr.attention16_emulate(*ops, B, L, H, dtype, lens=lens)
    for b, n in enumerate(lens):
        rows = slice(b * L, b * L + n)
        solo = tuple(t[rows] for t in ops)
        r1, u1 = rr.attention16_ref64(*solo, 1, n, H, dtype)
        assert torch.equal(ref[rows], r1) and torch.equal(unit[rows], u1)
        assert torch.equal(got[rows].view(torch.int16), rr.attention16_emulate(*solo, 1, n, H, dtype).view(torch.int16))
        pad = slice(b * L + n, (b + 1) * L)
        assert bool((ref[pad] == 0).all()) and bool((unit[pad] == 0).all()) and bool((got[pad].view(torch.int16) == 0).all())
        q = (ops[0][rows].double() / rr.QSCALE).view(n, H, 64).transpose(0, 1)
        k = ops[1][rows].double().view(n, H, 64).transpose(0, 1)
        p = torch.softmax(q @ k.transpose(-1, -2) / 8, -1)
        assert float(p[..., n - 1].min()) > 0.9, (n, float(p[..., n - 1].min()))


def test_attention_16_parts_refuses_bad_arguments_before_touching_a_device():
    """Every argument of esmdiff_attention_16_parts is validated before the first HIP call, so this runs without a GPU."""
    from esmdiff_amd import _native as N
    lib = N.lib()
    fake = 4096                                                               # never dereferenced: refused first

    def att(**kw):
        a = dict(dtype=0, q=fake, k=fake, qkv=fake, ctx=fake, lens=None, B=2, L=8, H=4)
        a.update(kw)
        return lib.esmdiff_attention_16_parts(a["dtype"], a["q"], a["k"], a["qkv"], a["ctx"], a["lens"], a["B"], a["L"], a["H"], None)
    i32x2 = ctypes.c_int32 * 2
    for bad in ({"q": None}, {"k": None}, {"qkv": None}, {"ctx": None}, {"dtype": 2}, {"dtype": -1}, {"B": 0}, {"B": -1}, {"L": 0},
                {"L": -3}, {"H": 0}, {"H": -1}, {"H": 33}, {"lens": i32x2(8, 0)}, {"lens": i32x2(9, 8)}, {"lens": i32x2(8, -3)},
                {"dtype": 1, "lens": i32x2(0, 1)}):
        assert att(**bad) == -1, bad
    assert "lens[0]" in lib.esmdiff_last_error(None).decode()

"""The comparators of tests/test_gpu_rowwise.py (tests/rowwise_ref.py) must let the right answer through and stop wrong
ones: the float64 reference rounded to each build's output type passes, the same with a planted error fails.  The plants
are the defects a row kernel can carry without a whole-network test noticing.  Also: the new test entry points refuse bad
arguments without touching a device."""
import ctypes

import pytest
import torch

from tests import rowwise_ref as rr

BUILDS = (torch.bfloat16, torch.float16, torch.float32)


def _passes(r) -> bool:
    return bool(torch.isfinite(r).all()) and float(r.max()) <= 1.0


# ---------------------------------------------------------------------------------------------------------------
B, L, VH = 2, 65, 4                         # L % 4 == 1: the last key opens a 4-key trip of its own


@pytest.fixture(scope="module")
def geom_case():
    frames = rr.chain_frames(B, L, ["all", "gaps"], seed=2)
    P = torch.randn(B, L, 15 * VH, generator=torch.Generator().manual_seed(2))
    g = torch.Generator().manual_seed(3)
    scales = {"init": (0.5 * torch.randn(VH, generator=g), 0.5 * torch.randn(VH, generator=g)),
              "sharp": (0.5 * torch.randn(VH, generator=g), 6 + 2 * torch.rand(VH, generator=g)),
              "flat": (-10 + 0.1 * torch.randn(VH, generator=g), -10 + 0.1 * torch.randn(VH, generator=g))}
    return frames, P, scales


def _geom(geom_case, dtype, kind, **plant):
    frames, P, scales = geom_case
    P16 = P.to(dtype)
    ref, unit = rr.geom_ref64(P16, *frames, *scales[kind])
    bad, _ = rr.geom_ref64(P16, *frames, *scales[kind], **plant) if plant else (ref, None)
    return ref, unit, bad


@pytest.mark.parametrize("dtype", BUILDS)
@pytest.mark.parametrize("kind", ["init", "sharp", "flat"])
def test_geom_bar_passes_the_rounded_reference(geom_case, dtype, kind):
    ref, unit, _ = _geom(geom_case, dtype, kind)
    assert _passes(rr.geom_ratio(ref.to(dtype), ref, unit, dtype))


@pytest.mark.parametrize("dtype", BUILDS)
def test_geom_bar_rejects_a_dropped_rotation_product_in_lanes_48_to_63(geom_case, dtype):
    """The r06 defect's shape: queries 48 - 63 of one (sample, head) wrong; here q_rot loses R[0][1] * v[1]."""
    frames, P, _ = geom_case
    rot = frames[0].double()
    P16 = P.to(dtype)

    def plant(parts, heads):
        if 2 in heads:
            h = heads.index(2)
            parts[0][1, h, 48:64, 0] -= rot[1, 48:64, 0, 1] * P16[1, 48:64, 3 * 2 + 1].double()
    ref, unit, bad = _geom(geom_case, dtype, "init", plant=plant)
    r = rr.geom_ratio(bad.to(dtype), ref, unit, dtype)
    assert not _passes(r)
    assert float(r[1, 48:64, 2].max()) > 1 and float(r[0].max()) <= 1          # and it is found where it was planted


@pytest.mark.parametrize("dtype", BUILDS)
def test_geom_bar_rejects_a_dropped_last_key_under_the_sharp_scale(geom_case, dtype):
    frames = geom_case[0]
    km = frames[2].clone()
    km[:, L - 1] = False
    ref, unit, bad = _geom(geom_case, dtype, "sharp", key_mask=km)
    assert not _passes(rr.geom_ratio(bad.to(dtype), ref, unit, dtype))


@pytest.mark.parametrize("dtype", BUILDS)
@pytest.mark.parametrize("kind", ["init", "flat"])
def test_geom_bar_rejects_a_frameless_key_counted_as_framed(geom_case, dtype, kind):
    frames = geom_case[0]
    km = frames[2].clone()
    j = int((~km[1]).nonzero()[1])                                             # a frameless key inside the Inf run
    km[1, j] = True
    ref, unit, bad = _geom(geom_case, dtype, kind, key_mask=km)
    assert not _passes(rr.geom_ratio(bad.to(dtype), ref, unit, dtype))


@pytest.mark.parametrize("dtype", BUILDS)
def test_geom_bar_rejects_swapped_samples(geom_case, dtype):
    ref, unit, _ = _geom(geom_case, dtype, "init")
    assert not _passes(rr.geom_ratio(ref.flip(0).to(dtype), ref, unit, dtype))


# ---------------------------------------------------------------------------------------------------------------
H, BQ, LQ = 12, 2, 9                        # D = 768: ends in a half 512-column slab


@pytest.fixture(scope="module")
def qk_case():
    D = H * 64
    g = torch.Generator().manual_seed(4)
    x = torch.randn(BQ * LQ, 3 * D, generator=g)
    x[3, :4] = 500.0                                                          # outlier channels
    x[-1, :2 * D] = 3 + 3e-3 * torch.randn(2 * D, generator=g)                # a low-variance row
    return x, 1 + 0.3 * torch.randn(D, generator=g), 1 + 0.3 * torch.randn(D, generator=g)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_qk_rope_bar_passes_the_rounded_reference_and_rejects_plants(qk_case, dtype):
    x, qw, kw = qk_case
    qkv = x.to(dtype)
    (qr, qu), (kr, ku) = rr.qk_rope_ref64(qkv, qw, kw, BQ, LQ, H)
    for ref, unit in ((qr, qu), (kr, ku)):
        assert _passes(rr.ratio(ref.to(dtype), ref, dtype, rr.QK_COEF * unit))
    # a wrong rotate-half partner in one head: column offset +-16 instead of +-32
    (pq, _), (pk, _) = rr.qk_rope_ref64(qkv, qw, kw, BQ, LQ, H, partner=torch.arange(64) ^ 16, plant_head=5)
    for bad, ref, unit in ((pq, qr, qu), (pk, kr, ku)):
        r = rr.ratio(bad.to(dtype), ref, dtype, rr.QK_COEF * unit)
        assert not _passes(r) and _passes(r.view(-1, H, 64)[:, [h for h in range(H) if h != 5]])
    # eps = 1e-6 instead of 1e-5: caught on the low-variance row
    (eq, _), (ek, _) = rr.qk_rope_ref64(qkv, qw, kw, BQ, LQ, H, eps=1e-6)
    for bad, ref, unit in ((eq, qr, qu), (ek, kr, ku)):
        assert not _passes(rr.ratio(bad.to(dtype)[-1:], ref[-1:], dtype, rr.QK_COEF * unit[-1:]))


def test_rope_tables_match_the_engine_recipe():
    """inv_freq = 1.0f / powf(10000.0f, (float)(2i) / 64.0f) at engine create: the float32 values the reference uses."""
    inv = rr.rope_inv_freq()
    assert inv.dtype == torch.float32 and float(inv[0]) == 1.0
    assert torch.equal(inv, (1.0 / torch.pow(torch.tensor(10000.0), torch.arange(0, 64, 2, dtype=torch.float32) / 64)))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_add_ln_bar_passes_the_rounded_reference_and_rejects_plants(dtype):
    M, D = 5, 768
    g = torch.Generator().manual_seed(6)
    x = torch.randn(M, D, generator=g) * 3
    x[-1] = 5 + 2e-3 * torch.randn(D, generator=g)                            # a low-variance row
    d1 = torch.randn(M, D, generator=g).to(dtype)
    d2 = (0.5 * torch.randn(M, D, generator=g)).to(dtype)
    d1[-1] = (1e-3 * torch.randn(D, generator=g)).to(dtype)
    d2[-1] = (1e-3 * torch.randn(D, generator=g)).to(dtype)
    w, b = 1 + 0.3 * torch.randn(D, generator=g), 0.2 * torch.randn(D, generator=g)
    v = (x + d1.float()) + d2.float()
    ref, unit = rr.add_ln_ref64(v, w, b)
    assert _passes(rr.ratio(ref.to(dtype), ref, dtype, rr.LN_COEF * unit))
    twice, _ = rr.add_ln_ref64(v + d2.float(), w, b)                          # delta2 added twice
    assert not _passes(rr.ratio(twice.to(dtype), ref, dtype, rr.LN_COEF * unit))
    eps6, _ = rr.add_ln_ref64(v, w, b, eps=1e-6)                              # eps 1e-6 instead of 1e-5
    r = rr.ratio(eps6.to(dtype), ref, dtype, rr.LN_COEF * unit)
    assert not _passes(r[-1:]) and _passes(r[:-1])                            # only the low-variance row can tell


def test_add_ln_bar_and_f16_subnormal_outputs():
    """Why the LayerNorm cases keep their gains at or above rr.LN_MIN_GAIN: without a bias an f16 output under 2^-14 is subnormal
    and rounds by up to 2^-25, which the bar's relative output term does not describe.  With a gain of 0.0036 in one column (what
    1 + 0.3 randn gives at seed 1792) the float64 reference rounded to f16 — the best any f16 kernel can do — misses the bar; with
    the gains of rr.ln_gains it passes, as does bfloat16 with either."""
    M, D = 1027, 1792
    g = torch.Generator().manual_seed(D)
    w = 1 + 0.3 * torch.randn(D, generator=g)
    assert 0.003 < float(w.abs().min()) < 0.004
    x = torch.randn(M, D, generator=g) * 3 + torch.randn(M, 1, generator=g)
    ref, unit = rr.add_ln_ref64(x, w, None)
    r = rr.ratio(ref.half(), ref, torch.float16, rr.LN_COEF * unit)
    assert not _passes(r) and float(ref.reshape(-1)[int(r.argmax())].abs()) < 2.0 ** -14
    assert _passes(rr.ratio(ref.bfloat16(), ref, torch.bfloat16, rr.LN_COEF * unit))
    wk = rr.ln_gains(D, torch.Generator().manual_seed(D))
    assert float(wk.abs().min()) == rr.LN_MIN_GAIN and torch.equal(wk[w.abs() >= rr.LN_MIN_GAIN], w[w.abs() >= rr.LN_MIN_GAIN])
    ref, unit = rr.add_ln_ref64(x, wk, None)
    assert _passes(rr.ratio(ref.half(), ref, torch.float16, rr.LN_COEF * unit))
    _, rstd, vmax = rr.ln64(x, wk)
    assert float((rstd * vmax).min()) * rr.LN_MIN_GAIN >= 1 / 8                # the condition the floor was derived from


# ---------------------------------------------------------------------------------------------------------------
def test_new_entry_points_refuse_bad_arguments_before_touching_a_device():
    """esmdiff_geom_attention / esmdiff_add_layernorm validate everything before their first HIP call, so these run
    without a GPU."""
    from esmdiff_amd import _native as N
    lib = N.lib()
    w = (ctypes.c_float * 4)()
    fake = 4096                                                               # never dereferenced: refused first

    def geom(**kw):
        a = dict(P=fake, dtype=0, rot=fake, trans=fake, has=fake, out=fake, B=1, L=8, VH=4)
        a.update(kw)
        return lib.esmdiff_geom_attention(a["P"], a["dtype"], a["rot"], a["trans"], a["has"], w, w, a["out"], a["B"],
                                          a["L"], a["VH"], None)
    for bad in ({"P": None}, {"rot": None}, {"trans": None}, {"has": None}, {"out": None}, {"dtype": 3}, {"dtype": -1},
                {"B": 0}, {"L": 0}, {"VH": 0}, {"B": -1}, {"L": 3201}):
        assert geom(**bad) == -1, bad
    assert "3200" in lib.esmdiff_last_error(None).decode()
    assert lib.esmdiff_geom_attention(fake, 0, fake, fake, fake, None, w, fake, 1, 8, 4, None) == -1
    for dtype, M, D in ((0, 4, 0), (1, 4, 0), (0, 4, -256), (2, 4, 256), (0, 0, 256)):
        assert lib.esmdiff_add_layernorm(dtype, fake, None, None, 1, fake, None, fake, M, D, None) == -1, (dtype, M, D)
    assert lib.esmdiff_qk_norm_rope(None, fake, fake, fake, fake, fake, 1, 1, 8, None) == -1
    assert lib.esmdiff_attention_f16(None, fake, fake, fake, fake, 1, 1, None) == -1

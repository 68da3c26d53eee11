"""The row kernels between the GEMMs, one at a time, against float64 statements of the same op (tests/rowwise_ref.py):
block 0's geometric attention in its bf16, f16 and f32 builds (csrc/geom.hip), q/k LayerNorm + rotary in the bf16 and f16
builds and attention in the f16 build (csrc/norm.hip, csrc/attention.hip), and the fused residual add + LayerNorm in both
16-bit builds (csrc/norm.hip).  Whole-network parity cannot see these kernels go subtly wrong: a planted error in a few
geometric (sample, head) pairs moves the logits by less than the forward's bf16 bar.

The references are computed on the device in float64 from the exact 16-bit (or f32) inputs the kernel received.  Every
bar is per element (or per (sample, query, head)): OUT_EPS |ref| for the output rounding plus coef x an arithmetic unit
(rowwise_ref.py); each assert states the largest ratio to the bar measured on an MI355X.  tests/test_rowwise_bars_cpu.py
shows that these comparators reject planted errors.
"""
import math

import pytest
import torch

from tests import rowwise_ref as rr

pytestmark = pytest.mark.gpu

BUILDS = (torch.bfloat16, torch.float16, torch.float32)
NAME = {torch.bfloat16: "bf16", torch.float16: "f16", torch.float32: "f32"}


def _scales(kind: str, VH: int, g: torch.Generator):
    """Raw per-head (rotation, distance) scales: "init" N(0, 0.5) as random init; "sharp" a raw distance scale of 6 - 8
    (nearest keys dominate, the lazy rescale runs); "big" raw > 20 (softplus's threshold branch); "flat" raw ~ -10
    (near-uniform attention)."""
    n = lambda: torch.randn(VH, generator=g)
    if kind == "init":
        return 0.5 * n(), 0.5 * n()
    if kind == "sharp":
        return 0.5 * n(), 6 + 2 * torch.rand(VH, generator=g)
    if kind == "big":
        return 20.5 + 3 * torch.rand(VH, generator=g), 20.5 + 3 * torch.rand(VH, generator=g)
    assert kind == "flat"
    return -10 + 0.1 * n(), -10 + 0.1 * n()


def _P(B, L, VH, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, L, 15 * VH, generator=g).cuda()


def _check_geom(out, P16, frames, raw, dtype, what):
    rot, trans, has = frames
    ref, unit = rr.geom_ref64(P16, rot, trans, has, *raw)
    assert out.dtype == dtype and out.shape == ref.shape
    # frameless rows (and every row of a sample without frames) are exact zeros: +0.0, bit for bit
    bits = out.view(torch.int16 if dtype != torch.float32 else torch.int32)
    assert bool((bits[~has.cuda()] == 0).all()), what
    r = rr.geom_ratio(out, ref, unit, dtype)
    assert torch.isfinite(r).all(), what
    return float(r.max()), rr.needed_coef(out, ref, dtype, unit[:, None, :].repeat_interleave(3, -1))


GEOM_CASES = [  # (L, B, VH): every L, both B, both VH; one long chain
    (1, 1, 128), (2, 3, 256), (3, 3, 128), (5, 1, 256), (63, 3, 128), (64, 1, 256), (65, 3, 256), (129, 3, 128),
    (258, 1, 256), (1026, 3, 128)]


@pytest.mark.parametrize("L,B,VH", GEOM_CASES)
def test_geom_attention_vs_float64(L, B, VH):
    """geom_attention_kernel, bf16 / f16 / f32 builds, against oracle.geom_ref.geom_attention_core in float64: all-framed,
    NaN BOS / EOS plus an Inf run (different per sample), a sample without frames; four scale regimes."""
    from esmdiff_amd.engine import geom_attention
    patterns = ["all", "gaps", "none"][:B] if B > 1 else [["all", "gaps"][L % 2]]
    if B == 3 and L % 2:
        patterns = ["gaps", "all", "gaps2"]                      # odd L at B = 3: two different masks, every sample framed
    frames = rr.chain_frames(B, L, patterns, seed=L)
    P = _P(B, L, VH, seed=L + VH)
    g = torch.Generator().manual_seed(7 * L + B)
    worst = {}
    for kind in ("init", "sharp", "big", "flat"):
        raw = _scales(kind, VH, g)
        for dtype in BUILDS:
            P16 = P.to(dtype)
            out = geom_attention(P16, *frames, *raw)
            r, need = _check_geom(out, P16, frames, raw, dtype, (kind, NAME[dtype]))
            w = worst.setdefault(NAME[dtype], [0.0, 0.0])
            w[0], w[1] = max(w[0], r), max(w[1], need)
            # bf16 / f16: the output rounding dominates, measured ratio 0.87 - 0.99 over the cases (bounded by construction);
            # f32: measured ratio 0.70 at L = 2 (coef 1.4 of the unit needed, 2 allowed), 0.09 - 0.13 from L = 63 on
            assert r <= 1.0, (kind, NAME[dtype], r, need)
    print(f"MEASURED geom L={L} B={B} VH={VH} " + " ".join(f"{k}: ratio {v[0]:.3f} coef {v[1]:.2f}" for k, v in worst.items()))


def test_geom_attention_self_only_key_is_its_own_value():
    """A query whose only framed key is itself attends to itself alone: its output is its own value vector (rotated into
    the global frame and back), analytically; every other row of that sample is zero."""
    from esmdiff_amd.engine import geom_attention
    B, L, VH = 2, 65, 128
    frames = rr.chain_frames(B, L, ["self", "gaps"], seed=5)
    P = _P(B, L, VH, seed=5)
    g = torch.Generator().manual_seed(5)
    for kind in ("init", "sharp", "big"):
        raw = _scales(kind, VH, g)
        for dtype in BUILDS:
            P16 = P.to(dtype)
            out = geom_attention(P16, *frames, *raw)
            r, _ = _check_geom(out, P16, frames, raw, dtype, (kind, NAME[dtype]))
            assert r <= 1.0, (kind, NAME[dtype], r)
            value = P16[0, L // 2, 6 * VH:9 * VH].double().view(VH, 3)
            got = out[0, L // 2].double().view(VH, 3)
            # R^T (R v) in f32: a few 2^-24 of |v| plus the frame's own departure from orthonormality, then the output rounding
            R = frames[0][0, L // 2].double()
            orth = float((R.T @ R - torch.eye(3, dtype=torch.float64)).abs().sum())
            bar = rr.OUT_EPS[dtype] * value.abs() + (8 * rr.F32_EPS + orth) * value.norm(dim=-1, keepdim=True).cuda()
            assert bool(((got - value).abs() <= bar).all()), (kind, NAME[dtype], float((got - value).abs().max()))
            others = torch.cat([out[0, :L // 2], out[0, L // 2 + 1:]])
            assert bool((others == 0).all())


def test_geom_attention_longest_chain_and_refusal():
    """L = 3200 is the longest chain the kernel's 150 KB LDS request holds (12 floats per key); L = 3201 is refused
    before anything is launched, as are bad arguments."""
    import ctypes

    from esmdiff_amd import _native as N
    from esmdiff_amd.engine import geom_attention
    B, L, VH = 1, 3200, 4
    frames = rr.chain_frames(B, L, ["gaps"], seed=3)
    P = _P(B, L, VH, seed=3)
    g = torch.Generator().manual_seed(3)
    for kind in ("init", "sharp"):
        raw = _scales(kind, VH, g)
        for dtype in BUILDS:
            P16 = P.to(dtype)
            out = geom_attention(P16, *frames, *raw)
            r, need = _check_geom(out, P16, frames, raw, dtype, (kind, NAME[dtype]))
            assert r <= 1.0, (kind, NAME[dtype], r, need)
            print(f"MEASURED geom L=3200 {kind} {NAME[dtype]}: ratio {r:.3f} coef {need:.2f}")
    sentinel = torch.full((1, 3201, 3 * VH), 7.0, device="cuda")
    with pytest.raises(RuntimeError, match="3200"):
        geom_attention(torch.zeros(1, 3201, 15 * VH, device="cuda"), *rr.chain_frames(1, 3201, ["all"], seed=1),
                       torch.zeros(VH), torch.zeros(VH))
    lib = N.lib()
    w = (ctypes.c_float * VH)()
    rot, trans, has = (t.cuda().contiguous() for t in frames)
    has = has.to(torch.uint8)
    args = lambda **kw: [kw.get("P", P.data_ptr()), kw.get("dtype", 2), rot.data_ptr(), trans.data_ptr(), has.data_ptr(), w, w,
                         kw.get("out", sentinel.data_ptr()), kw.get("B", 1), kw.get("L", L), kw.get("VH", VH), None]
    for bad in ({"P": None}, {"out": None}, {"dtype": 3}, {"dtype": -1}, {"B": 0}, {"L": 0}, {"VH": 0}, {"L": -5}, {"L": 3201}):
        assert lib.esmdiff_geom_attention(*args(**bad)) == -1, bad
    torch.cuda.synchronize()
    assert bool((sentinel == 7.0).all())                          # nothing was launched into it


def test_geom_attention_kernel_invariances():
    """On the kernel alone: a global rotation plus a 1e3 A translation of every frame leaves the outputs unchanged within the
    f32 cancellation bound; each sample launched alone equals its row of the batched launch bit for bit; two launches are
    bit-identical."""
    from esmdiff_amd.engine import geom_attention
    B, L, VH = 3, 129, 128
    rot, trans, has = rr.chain_frames(B, L, ["gaps", "all", "gaps2"], seed=9)
    Q = torch.linalg.qr(torch.randn(3, 3, generator=torch.Generator().manual_seed(9), dtype=torch.float64))[0]
    Q = Q * torch.sign(torch.linalg.det(Q))
    rot2 = (Q @ rot.double()).float()
    trans2 = (trans.double() @ Q.T + torch.tensor([1e3, -1e3, 0.5e3], dtype=torch.float64)).float()
    P = _P(B, L, VH, seed=9)
    g = torch.Generator().manual_seed(9)
    for kind in ("init", "sharp"):
        raw = _scales(kind, VH, g)
        for dtype in BUILDS:
            P16 = P.to(dtype)
            out = geom_attention(P16, rot, trans, has, *raw)
            assert torch.equal(out, geom_attention(P16, rot, trans, has, *raw))
            for b in range(B):
                one = geom_attention(P16[b:b + 1].contiguous(), rot[b:b + 1], trans[b:b + 1], has[b:b + 1], *raw)
                assert torch.equal(one[0], out[b]), b
            moved = geom_attention(P16, rot2, trans2, has, *raw)
            _, unit = rr.geom_ref64(P16, rot2, trans2, has, *raw)        # its smax carries the 1e3 A coordinates
            # both outputs are rounded: one output ulp (2 x half) apart at most, plus the arithmetic of both runs
            eps = rr.OUT_EPS[dtype]
            d = (moved.double() - out.double()).abs().view(B, L, VH, 3)
            bar = 2 * eps * out.double().abs().view(B, L, VH, 3) + 2 * rr.GEOM_COEF * unit[:, None, :, None]
            r = float(torch.where(d == 0, torch.zeros_like(d), d / bar).max())
            print(f"MEASURED geom invariance {kind} {NAME[dtype]}: ratio {r:.3f}")
            assert r <= 1.0, (kind, NAME[dtype], r)


# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engines():
    from esmdiff_amd.config import TINY
    from esmdiff_amd.engine import Engine
    from esmdiff_amd.weights import random_init_state_dict
    sd = random_init_state_dict(TINY, seed=1)
    e = {torch.bfloat16: Engine(TINY, sd, max_batch=3, max_len=1026),
         torch.float16: Engine(TINY, sd, max_batch=3, max_len=1026, precision="f16")}
    yield e
    for v in e.values():
        v.close()


def _qkv(M, D, seed, dtype, outliers=True):
    """q, k, v rows ~ N(0, 1) + a row offset; a few rows carry +-500 outlier channels (trained_like_state_dict's
    activations have them), one row is low-variance (std 3e-3 around 3: eps = 1e-5 matters there)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, 3 * D, generator=g) + torch.randn(M, 1, generator=g)
    if outliers and M > 2:
        for r in range(0, M, max(1, M // 7)):
            ch = torch.randint(0, 2 * D, (4,), generator=g)
            x[r, ch] = 500.0 * torch.sign(torch.randn(4, generator=g))
        x[M - 1, :2 * D] = 3 + 3e-3 * torch.randn(2 * D, generator=g)
    return x.to(dtype).cuda()


QK_CASES = [(8, 1, 1026), (12, 3, 65), (20, 2, 129), (24, 3, 258)]   # D = 512, 768, 1280 (half slabs), 1536


@pytest.mark.parametrize("H,B,L", QK_CASES)
def test_qk_norm_rope_vs_float64(engines, H, B, L):
    """qk_norm_rope_kernel, bf16 and f16 builds: full-width LayerNorm of q and k, rotary of the float32 angle l * inv_freq
    (positions up to 1025), q pre-scaled by log2(e)/8, against float64."""
    D = H * 64
    g = torch.Generator().manual_seed(H)
    qw, kw = (1 + 0.3 * torch.randn(D, generator=g)).cuda(), (1 + 0.3 * torch.randn(D, generator=g)).cuda()
    for dtype, eng in engines.items():
        qkv = _qkv(B * L, D, seed=H + L, dtype=dtype)
        q, k = eng.qk_norm_rope(qkv, qw, kw, B, L, H)
        (qr, qu), (kr, ku) = rr.qk_rope_ref64(qkv, qw, kw, B, L, H)
        rs = []
        for got, ref, unit in ((q, qr, qu), (k, kr, ku)):
            r = rr.ratio(got, ref, dtype, rr.QK_COEF * unit)
            rs.append((float(r.max()), rr.needed_coef(got, ref, dtype, unit)))
            # output rounding dominates: measured ratio 0.993 - 0.996; coef needed 0.08 - 0.76 of the 4 allowed
            assert float(r.max()) <= 1.0, (NAME[dtype], float(r.max()))
        print(f"MEASURED qk_norm_rope D={D} B={B} L={L} {NAME[dtype]}: q {rs[0][0]:.3f} / {rs[0][1]:.2f}, "
              f"k {rs[1][0]:.3f} / {rs[1][1]:.2f}")


ATT_SHAPES = [(2, 60), (1, 258), (3, 130), (2, 129), (2, 257), (2, 259), (1, 64), (1, 65), (2, 33), (2, 128), (1, 256),
              (1, 192), (2, 32), (1, 31), (1, 1), (1, 1026)]


def test_attention_f16_vs_float64(engines):
    """attention_kernel_occ{3,4} in the f16 build (the certified engine's fast path), with the f16 q/k norm + rotary, at the
    shapes of test_attention_block and the 1026-token chain, against float64 per (token, head, channel)."""
    from esmdiff_amd.config import TINY
    eng = engines[torch.float16]
    D, H = TINY.d_model, TINY.n_heads
    g = torch.Generator().manual_seed(4)
    qw, kw = (1 + 0.3 * torch.randn(D, generator=g)).cuda(), (1 + 0.3 * torch.randn(D, generator=g)).cuda()
    worst = (0.0, 0.0)
    for B, L in ATT_SHAPES:
        qkv = _qkv(B * L, D, seed=B * 1000 + L, dtype=torch.float16, outliers=False)
        got = eng.attention(qkv, qw, kw, B, L)
        ref, unit = rr.attention_ref64(qkv, qw, kw, B, L, H, torch.float16)
        r = rr.ratio(got, ref, torch.float16, rr.ATT_COEF * unit)
        worst = (max(worst[0], float(r.max())), max(worst[1], rr.needed_coef(got, ref, torch.float16, unit)))
        # 16-bit q, k, P operands: coef 0.36 of the unit needed over all shapes, 1 allowed (~3x measured)
        assert float(r.max()) <= 1.0, (B, L, float(r.max()))
    with pytest.raises(RuntimeError, match="f16"):
        engines[torch.bfloat16]._chk(engines[torch.bfloat16]._lib.esmdiff_attention_f16(
            engines[torch.bfloat16]._h, qkv.data_ptr(), qw.data_ptr(), kw.data_ptr(), got.data_ptr(), 1, 1, None))
    print(f"MEASURED attention f16: ratio {worst[0]:.3f} coef {worst[1]:.2f}")


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [256, 512, 768, 1280, 1536, 2048])
def test_add_layernorm_vs_float64(D):
    """add_layernorm_kernel, bf16 and f16 builds: v = (x + delta) + delta2 with either delta absent, x written back bit-equal
    to torch float32 when write_x (untouched otherwise), y against float64 LayerNorm of v (a low-variance row included)."""
    from esmdiff_amd.engine import add_layernorm
    g = torch.Generator().manual_seed(D)
    w, b = (1 + 0.3 * torch.randn(D, generator=g)).cuda(), (0.2 * torch.randn(D, generator=g)).cuda()
    worst = {}
    for M in (1, 3, 4, 5, 1027):
        x0 = (torch.randn(M, D, generator=g) * 3 + torch.randn(M, 1, generator=g)).cuda()
        d1, d2 = torch.randn(M, D, generator=g).cuda(), (0.5 * torch.randn(M, D, generator=g)).cuda()
        if M >= 3:
            x0[M - 1] = 5 + 2e-3 * torch.randn(D, generator=g).cuda()
            d1[M - 1] *= 1e-3
            d2[M - 1] *= 1e-3
        for dtype in (torch.bfloat16, torch.float16):
            for delta in (None, d1.to(dtype)):
                for delta2 in (None, d2.to(dtype)):
                    v = x0.clone()
                    if delta is not None:
                        v = v + delta.float()
                    if delta2 is not None:
                        v = v + delta2.float()
                    for write_x in (0, 1):
                        for bias in (b, None):
                            x = x0.clone()
                            y = add_layernorm(dtype, x, delta, delta2, write_x, w, bias)
                            assert torch.equal(x, v if write_x else x0), (M, NAME[dtype], write_x)
                            ref, unit = rr.add_ln_ref64(v, w, bias)
                            r = float(rr.ratio(y, ref, dtype, rr.LN_COEF * unit).max())
                            wst = worst.setdefault(NAME[dtype], [0.0, 0.0])
                            wst[0], wst[1] = max(wst[0], r), max(wst[1], rr.needed_coef(y, ref, dtype, unit))
                            # output rounding dominates: measured ratio 0.996 - 0.998; coef 1.1 - 3.6 needed, 4 allowed
                            assert r <= 1.0, (M, NAME[dtype], delta is None, delta2 is None, write_x, r)
    print(f"MEASURED add_layernorm D={D} " + " ".join(f"{k}: ratio {v[0]:.3f} coef {v[1]:.2f}" for k, v in worst.items()))


def test_add_layernorm_refuses_bad_shapes():
    """D <= 0 (the launcher once sent D = 0 to its 2048-wide case), D % 256 != 0, D > 2048 and unknown builds are refused
    before any launch."""
    from esmdiff_amd import _native as N
    lib = N.lib()
    x = torch.full((4, 256), 3.0, device="cuda")
    w = torch.ones(256, device="cuda")
    y = torch.full((4, 256), 7.0, dtype=torch.bfloat16, device="cuda")
    for dtype, M, D in ((0, 4, 0), (1, 4, 0), (0, 4, -256), (0, 4, 128), (0, 1, 2304), (2, 4, 256), (0, 0, 256)):
        assert lib.esmdiff_add_layernorm(dtype, x.data_ptr(), None, None, 1, w.data_ptr(), None, y.data_ptr(), M, D,
                                         None) == -1, (dtype, M, D)
    assert lib.esmdiff_add_layernorm(0, None, None, None, 1, w.data_ptr(), None, y.data_ptr(), 4, 256, None) == -1
    torch.cuda.synchronize()
    assert bool((y.float() == 7.0).all()) and bool((x == 3.0).all())

"""The row kernels between the GEMMs of the float32-grade engines (F32: csrc/strict.hip; F32_SPLIT: csrc/gemm_split.hip,
csrc/attention_split.hip), one launcher at a time through the entries of include/esmdiff_hip_test.h, against float64 statements
of the same op (tests/rowwise_ref.py).  The certified sampler and every "ids equal the float32 chain" claim treat these engines
as exact, and whole forwards cannot see one of these kernels lose half its operand bits: the bars here are in the kernels' own
rounding units (coef x unit, nothing for the float32 output), so they can.  tests/test_f32_rows_bars_cpu.py shows that the same
comparators pass a torch float32 evaluation and reject planted defects; each test prints the worst ratio measured on an MI355X.
TINY engines only, for the rotary tables and the create-time scale rule."""
import math

import pytest
import torch

from tests import rowwise_ref as rr

pytestmark = pytest.mark.gpu
F32 = torch.float32
MAX_LEN = 258


def _big_gain_state_dict():
    """TINY weights whose q/k LayerNorm gains reach 50 and whose ln1 gain, bias and value-projection rows are large: what the
    create-time scale rule has to survive."""
    from esmdiff_amd.config import TINY
    from esmdiff_amd.weights import random_init_state_dict
    sd = random_init_state_dict(TINY, seed=11)
    g = torch.Generator().manual_seed(12)
    D = TINY.d_model
    for i in range(TINY.n_layers):
        b = f"net.transformer.blocks.{i}.attn."
        for nm, top in (("q_ln.weight", 50.0), ("k_ln.weight", 35.0 + 15.0 * i)):
            w = 4 + 4 * torch.rand(D, generator=g)
            w[int(torch.randint(0, D, (1,), generator=g))] = top
            sd[b + nm] = w * torch.sign(torch.randn(D, generator=g))
        sd[b + "layernorm_qkv.0.weight"] = 3 * (1 + 0.3 * torch.randn(D, generator=g)) * (1 + i)
        sd[b + "layernorm_qkv.0.bias"] = 2.0 * torch.randn(D, generator=g)
        sd[b + "layernorm_qkv.1.weight"][2 * D:] *= 5.0 * (1 + 3 * i)
    return sd


@pytest.fixture(scope="module")
def engines():
    from esmdiff_amd.config import TINY
    from esmdiff_amd.engine import Engine
    sd = _big_gain_state_dict()
    e = {p: Engine(TINY, sd, max_batch=2, max_len=MAX_LEN, precision=p) for p in ("f32", "f32_split")}
    yield TINY, sd, e
    for v in e.values():
        v.close()


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [256, 320, 1028, 1280, 1536, 2048])
def test_layernorm_f32_rows_vs_float64(D):
    """layernorm_f32_kernel and layernorm_split_kernel (FULL at D % 256 == 0, else the column-tested form; NV 1 .. 8; GELU_IN; a
    bf16 / f16 delta; y32 on and off) at M = 1, 5, 130 (a partial last workgroup of 4 rows), gains 1 and 30, with and without
    bias, on unit, low-variance, 1e4-scale, spike and all-zero rows: y32 within LN_COEF of float64; the split row reproduces
    y32 to the derived split bound with the exact power-of-two rs, equal hi planes, max |hi| in [2^14, 2^15] and a zero split
    with finite rs on an all-zero row."""
    from esmdiff_amd.engine import layernorm_f32rows
    worst = {"f32": 0.0, "split y32": 0.0, "split value": 0.0}
    for M in (1, 5, 130):
        for gain in (1.0, 30.0):
            x, w, b, delta, kinds = (t.cuda() for t in rr.ln_case(M, D, seed=D + M, gain=gain, first_kind=D % 5))
            for bias in (b, None):
                ref, unit = rr.ln_rows_ref64(x, w, bias)
                y = layernorm_f32rows(x, w, bias, split=False)
                worst["f32"] = max(worst["f32"], rr.needed_coef(y, ref, F32, unit))
                assert float(rr.ratio(y, ref, F32, rr.LN_COEF * unit).max()) <= 1.0, ("f32", M, gain, bias is None)
                for gelu_in in (False, True):
                    for d16 in (None, delta.to(torch.bfloat16), delta.to(torch.float16)):
                        what = (M, gain, bias is None, gelu_in, None if d16 is None else d16.dtype)
                        ref, unit = rr.ln_rows_ref64(x, w, bias, gelu_in=gelu_in, delta=d16)
                        a3, rs, y32 = layernorm_f32rows(x, w, bias, split=True, gelu_in=gelu_in, delta=d16)
                        worst["split y32"] = max(worst["split y32"], rr.needed_coef(y32, ref, F32, unit))
                        assert float(rr.ratio(y32, ref, F32, rr.LN_COEF * unit).max()) <= 1.0, what
                        rep = rr.split_rows_report(a3, rs, y32)
                        worst["split value"] = max(worst["split value"], float(rep["value"].max()))
                        assert rr.split_rows_ok(rep), (what, rr.split_rows_explain(rep, a3, rs, y32))
                        if bias is None and d16 is None:                     # an all-zero row: finite rs, a zero split
                            z = kinds == rr.LN_ZERO
                            assert bool((a3[z].float() == 0).all()) and bool(torch.isfinite(rs[z]).all()) and bool((rs[z] > 0).all())
                        # without y32 the same row is written: the f32 copy is a store more, not another computation
                        b3, brs, none = layernorm_f32rows(x, w, bias, split=True, gelu_in=gelu_in, delta=d16, want_y32=False)
                        assert none is None and torch.equal(b3.view(torch.int16), a3.view(torch.int16)) and torch.equal(brs, rs), what
    # measured on an MI355X: f32 coef 1.23 - 2.20 and split y32 coef 1.77 - 2.20 of the 4 allowed; split value 0.55 - 1.00 of its bound
    print(f"MEASURED layernorm f32 rows D={D}: " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))


def test_layernorm_f32_rows_refuses_bad_widths():
    """D = 2052 (above the 8 register slabs) and D % 4 != 0 are refused by both kernels before anything is launched."""
    from esmdiff_amd.engine import layernorm_f32rows
    for D in (2052, 258, 1030):
        x, w = torch.ones(4, D, device="cuda"), torch.ones(D, device="cuda")
        for split in (False, True):
            with pytest.raises(RuntimeError, match="2048"):
                layernorm_f32rows(x, w, None, split=split)


# ---------------------------------------------------------------------------------------------------------------
def _qkv32(M, D, seed):
    """q, k, v rows ~ N(0, 1) + a row offset, +-500 outlier channels in a few rows, the last row low-variance."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, 3 * D, generator=g) + torch.randn(M, 1, generator=g)
    if M > 2:
        for r in range(0, M, max(1, M // 7)):
            ch = torch.randint(0, 2 * D, (4,), generator=g)
            x[r, ch] = 500.0 * torch.sign(torch.randn(4, generator=g))
        x[M - 1, :2 * D] = 3 + 3e-3 * torch.randn(2 * D, generator=g)
    return x.cuda()


@pytest.mark.parametrize("H", [1, 4, 5, 24, 32])
def test_qk_norm_rope_f32_vs_float64(engines, H):
    """qk_norm_rope_f32_kernel and qk_norm_rope_split_kernel (FULL at H % 4 == 0) at L = 1, 2 and max_len = 258 (the last
    table position), B = 2: the f32 rows against the unscaled reference; [hi | lo] at scales 1, 2^6, 2^13 (times log2(e)/8 on q)
    against the scaled one, plus the split bound; hi to nearest, everything finite."""
    _, _, engs = engines
    D, B = H * 64, 2
    g = torch.Generator().manual_seed(H)
    w0 = [(1 + 0.3 * torch.randn(D, generator=g)).cuda() for _ in range(2)]
    qs32 = float(torch.tensor(rr.QSCALE, dtype=F32))
    worst = {"f32": 0.0, "split": 0.0}
    for L in (1, 2, MAX_LEN):
        qkv = _qkv32(B * L, D, seed=H + L)
        qw, kw = 6 * w0[0], 6 * w0[1]
        got = engs["f32"].qk_norm_rope_f32(qkv, qw, kw, B, L, H)
        for x, (ref, unit) in zip(got, rr.qk_rope_f32_ref64(qkv, qw, kw, B, L, H)):
            worst["f32"] = max(worst["f32"], rr.needed_coef(x, ref, F32, unit))
            assert float(rr.ratio(x, ref, F32, rr.QK_COEF * unit).max()) <= 1.0, ("f32", L)
        for scale, gain in rr.QK_SPLIT_GAIN.items():
            qw, kw = gain * w0[0], gain * w0[1]
            got = engs["f32_split"].qk_norm_rope_f32(qkv, qw, kw, B, L, H, split=True, q_scale=qs32 * scale, k_scale=scale)
            refs = rr.qk_rope_f32_ref64(qkv, qw, kw, B, L, H, q_scale=qs32 * scale, k_scale=scale)
            for x2, (ref, unit) in zip(got, refs):
                assert bool(torch.isfinite(x2.float()).all()) and float(x2.float().abs().max()) < 2.0 ** 15, (scale, L)
                hi, lo, _ = rr.split_planes(x2, D, planes=2)
                assert bool((lo.abs() <= rr.half_ulp_f16(hi)).all()), (scale, L)
                r = rr.ratio(hi + lo, ref, F32, rr.QK_COEF * unit + rr.split_bar(ref))
                worst["split"] = max(worst["split"], float(r.max()))
                assert float(r.max()) <= 1.0, (scale, L, float(r.max()))
    # measured: f32 coef 1.24 - 1.57 of 4; split ratio 0.30 - 0.35
    print(f"MEASURED qk_norm_rope f32 rows D={D}: f32 coef {worst['f32']:.2f} of {rr.QK_COEF:g}, split ratio {worst['split']:.3f}")


def test_qk_spike_row_stays_finite_under_the_engines_own_scale(engines):
    """One column at 1e3, the rest 0, under the largest q / k gain (50): the normalised spike reaches sqrt(D - 1) x 50; with the
    scale the engine chose at create the split row stays finite, |hi| < 2^15, and within the bar."""
    cfg, sd, engs = engines
    eng = engs["f32_split"]
    D, H = cfg.d_model, cfg.n_heads
    for layer in range(cfg.n_layers):
        qw = sd[f"net.transformer.blocks.{layer}.attn.q_ln.weight"].cuda()
        kw = sd[f"net.transformer.blocks.{layer}.attn.k_ln.weight"].cuda()
        att_qk, _ = eng.attention_scales(layer)
        qkv = torch.zeros(2, 3 * D).cuda()
        qkv[0, int(qw.abs().argmax())] = 1e3
        qkv[0, D + int(kw.abs().argmax())] = 1e3
        qkv[1, int(qw.abs().argmax())] = -1e3
        qkv[1, D + int(kw.abs().argmax())] = -1e3
        qs = float(torch.tensor(rr.QSCALE, dtype=F32)) * att_qk
        got = eng.qk_norm_rope_f32(qkv, qw, kw, 1, 2, H, split=True, q_scale=qs, k_scale=att_qk)
        refs = rr.qk_rope_f32_ref64(qkv, qw, kw, 1, 2, H, q_scale=qs, k_scale=att_qk)
        worst = []
        for x2, (ref, unit) in zip(got, refs):
            assert bool(torch.isfinite(x2.float()).all()) and float(x2[:, :D].float().abs().max()) < 2.0 ** 15
            hi, lo, _ = rr.split_planes(x2, D, planes=2)
            worst.append(float(rr.ratio(hi + lo, ref, F32, rr.QK_COEF * unit + rr.split_bar(ref)).max()))
            assert worst[-1] <= 1.0, (layer, worst)
        assert float(got[1][:, :D].float().abs().max()) > 2.0 ** 12             # the k spike really uses the range
        print(f"MEASURED qk spike layer {layer}: att_qk {att_qk:g}, max |hi| q {float(got[0][:, :D].float().abs().max()):.0f} "
              f"k {float(got[1][:, :D].float().abs().max()):.0f} of 32768, ratio q {worst[0]:.3f} k {worst[1]:.3f}")


def test_attention_scale_rule_cannot_overflow(engines):
    """engine create's att_qk / att_v: powers of two with att_qk sqrt(2 (D - 1)) wmax <= 30000 and att_v (sqrt(D) gmax + |b|_2)
    max_row |W_v|_2 <= 30000, the bounds computed from the state dict in float64; and not smaller than needed (above a quarter
    of the room)."""
    cfg, sd, engs = engines
    D = cfg.d_model
    for layer in range(cfg.n_layers):
        b = f"net.transformer.blocks.{layer}.attn."
        att_qk, att_v = engs["f32_split"].attention_scales(layer)
        wmax = max(float(sd[b + "q_ln.weight"].double().abs().max()), float(sd[b + "k_ln.weight"].double().abs().max()))
        gmax = float(sd[b + "layernorm_qkv.0.weight"].double().abs().max())
        b2 = float(sd[b + "layernorm_qkv.0.bias"].double().norm())
        rn = float(sd[b + "layernorm_qkv.1.weight"][2 * D:].double().norm(dim=1).max())
        qk_bound, v_bound = math.sqrt(2 * (D - 1)) * wmax, (math.sqrt(D) * gmax + b2) * rn
        assert rr.is_pow2(att_qk) and rr.is_pow2(att_v), (att_qk, att_v)
        assert att_qk * qk_bound <= 30000 and att_v * v_bound <= 30000, (layer, att_qk * qk_bound, att_v * v_bound)
        assert att_qk * qk_bound > 30000 / 4 and att_v * v_bound > 30000 / 4, (layer, att_qk * qk_bound, att_v * v_bound)
        assert wmax >= 49.9                                                  # the gains really reach 50
        print(f"MEASURED scale rule layer {layer}: att_qk {att_qk:g} x {qk_bound:.0f} = {att_qk * qk_bound:.0f}, "
              f"att_v {att_v:g} x {v_bound:.0f} = {att_v * v_bound:.0f}")
    with pytest.raises(RuntimeError, match="F32_SPLIT"):
        engs["f32"].attention_scales(0)
    with pytest.raises(RuntimeError, match="layer"):
        engs["f32_split"].attention_scales(cfg.n_layers)


def test_engine_entries_refuse_bad_arguments(engines):
    """esmdiff_qk_norm_rope_f32 and esmdiff_get_attention_scales need an engine, so their refusals run here: a split flag other
    than 0 / 1, H outside 1 .. 32, B or L not positive, L above max_len, scales that are zero, negative, infinite or NaN, null
    pointers; nothing is written."""
    import ctypes
    cfg, _, engs = engines
    eng = engs["f32_split"]
    H, D = cfg.n_heads, cfg.d_model
    qkv, w = torch.ones(2, 3 * D).cuda(), torch.ones(D).cuda()
    q, k = torch.full((2, 2 * D), 7.0, dtype=torch.float16).cuda(), torch.full((2, 2 * D), 7.0, dtype=torch.float16).cuda()

    def call(**kw):
        a = dict(qkv=qkv.data_ptr(), qw=w.data_ptr(), kw=w.data_ptr(), split=1, qs=1.0, ks=1.0, q=q.data_ptr(), k=k.data_ptr(),
                 B=1, L=2, H=H)
        a.update(kw)
        return eng._lib.esmdiff_qk_norm_rope_f32(eng._h, a["qkv"], a["qw"], a["kw"], a["split"], a["qs"], a["ks"], a["q"],
                                                 a["k"], a["B"], a["L"], a["H"], None)
    inf, nan = float("inf"), float("nan")
    for bad in ({"qkv": None}, {"qw": None}, {"kw": None}, {"q": None}, {"k": None}, {"split": 2}, {"split": -1}, {"H": 0},
                {"H": 33}, {"H": -1}, {"B": 0}, {"L": 0}, {"B": -1}, {"L": MAX_LEN + 1}, {"qs": 0.0}, {"ks": 0.0}, {"qs": -1.0},
                {"ks": -2.0}, {"qs": inf}, {"ks": inf}, {"qs": nan}, {"ks": nan}):
        assert call(**bad) == -1, bad
    assert "finite and positive" in eng._lib.esmdiff_last_error(eng._h).decode()
    torch.cuda.synchronize()
    assert bool((q == 7.0).all()) and bool((k == 7.0).all())                  # nothing was launched
    qf, kf = torch.empty(2, D).cuda(), torch.empty(2, D).cuda()
    assert call() == 0 and call(split=0, qs=nan, ks=-1.0, q=qf.data_ptr(), k=kf.data_ptr()) == 0   # the f32 form ignores the scales
    assert bool(torch.isfinite(qf).all()) and bool(torch.isfinite(kf).all())
    f = ctypes.c_float(0)
    get = eng._lib.esmdiff_get_attention_scales
    assert get(eng._h, 0, None, ctypes.byref(f)) == -1 and get(eng._h, 0, ctypes.byref(f), None) == -1
    assert get(eng._h, -1, ctypes.byref(f), ctypes.byref(f)) == -1 and get(eng._h, cfg.n_layers, ctypes.byref(f), ctypes.byref(f)) == -1
    assert get(engs["f32"]._h, 0, ctypes.byref(f), ctypes.byref(f)) == -1


def test_v_split_vs_its_bound():
    """v_split_kernel: [hi | lo] of the V third times the scale, to the split bound, hi to nearest (D = 320, 512, 2048; scales 1, 2^11)."""
    from esmdiff_amd.engine import v_split
    worst = 0.0
    for M, D in ((1, 320), (5, 2048), (130, 512)):
        qkv = _qkv32(M, D, seed=M + D)
        for scale in (1.0, 2.0 ** 11):
            v2 = v_split(qkv, scale)
            hi, lo, _ = rr.split_planes(v2, D, planes=2)
            a = qkv[:, 2 * D:].double() * scale
            assert bool(torch.isfinite(v2.float()).all()) and bool((lo.abs() <= rr.half_ulp_f16(hi)).all())
            worst = max(worst, float(((hi + lo - a).abs() / rr.split_bar(a)).max()))
            assert bool(((hi + lo - a).abs() <= rr.split_bar(a)).all()), (M, D, scale)
            assert torch.equal(v2.view(torch.int16), rr.split_operand(qkv[:, 2 * D:], scale).view(torch.int16))
    print(f"MEASURED v_split: {worst:.2f} of the split bound, bit-equal to the float32 restatement")


# ---------------------------------------------------------------------------------------------------------------
QS32 = float(torch.tensor(rr.QSCALE, dtype=F32))


def _split_ops(q, k, v, sq, sv):
    return rr.split_operand(q, QS32 * sq), rr.split_operand(k, sq), rr.split_operand(v, sv)


def _split_ref(q2, k2, v2, sq, sv, B, L, H):
    """The float64 reference of the split kernel from (hi + lo) / scale of its own operands; q carries log2(e)/8 exactly."""
    return rr.attention32_ref64(rr.split_operand_value(q2, sq) * rr.LN2_8, rr.split_operand_value(k2, sq),
                                rr.split_operand_value(v2, sv), B, L, H)


def _lens_for(B, L):
    return {1: [max(1, L - 1)], 2: [max(1, L // 3), L], 3: [L, (L + 1) // 2, 1]}[B]


@pytest.mark.parametrize("L", rr.ATT_LS)
def test_attention_f32_parts_vs_float64(L):
    """attention_f32_kernel and attention_split_kernel (scales 1 and 2^8 / 2^12) on the same inputs under the same bar,
    ATT32_COEF x 2^-24 (1 + |q| kmax / 8) sum_k p_k |v_k|, at B H = 1, 9, 16: unit-size rows, q/k gains 4 and 8, staircases that
    rescale at every 64-key tile / never after the first, one key with all the mass.  Every case again with lens: padded context
    rows exactly 0, valid rows bit-equal to a solo launch at that length and within the bar, 50 x garbage in the padded operand rows."""
    from esmdiff_amd.engine import attention_f32_parts
    worst = {"f32": 0.0, "split": 0.0, "split scaled": 0.0}
    for B, H in rr.ATT_BH:
        D = H * 64
        for kind in rr.ATT_KINDS:
            q, k, v = (t.cuda() for t in rr.attention_case(kind, B, L, H, seed=L))
            ref, unit = rr.attention32_ref64(q, k, v, B, L, H)
            qkv = torch.cat([q, k, v], 1).contiguous()
            got = attention_f32_parts(q, k, qkv, B, L, H)
            worst["f32"] = max(worst["f32"], rr.needed_coef(got, ref, F32, unit))
            assert float(rr.ratio(got, ref, F32, rr.ATT32_COEF * unit).max()) <= 1.0, ("f32", B, H, kind)
            runs = {"f32": (q, k, qkv, {})}
            for name, sq, sv in (("split", 1.0, 1.0), ("split scaled", 2.0 ** 8, 2.0 ** 12)):
                q2, k2, v2 = _split_ops(q, k, v, sq, sv)
                assert all(bool(torch.isfinite(t.float()).all()) for t in (q2, k2, v2))
                sref, sunit = _split_ref(q2, k2, v2, sq, sv, B, L, H)
                kw = dict(qk_scale_product=sq * sq, v_scale=sv)
                got = attention_f32_parts(q2, k2, v2, B, L, H, **kw)
                worst[name] = max(worst[name], rr.needed_coef(got, sref, F32, sunit))
                assert float(rr.ratio(got, sref, F32, rr.ATT32_COEF * sunit).max()) <= 1.0, (name, B, H, kind)
                runs[name] = (q2, k2, v2, kw)
            lens = _lens_for(B, L)                                           # ragged launches of the same three kernels
            g = torch.Generator().manual_seed(L + B)
            for name, (qq, kk, vv, kw) in runs.items():
                qq, kk, vv = qq.clone(), kk.clone(), vv.clone()
                for b, n in enumerate(lens):                                 # 50 x garbage in the padded operand rows (finite in f16)
                    for t in (qq, kk, vv):
                        amp = 50.0 * float(t[b * L:b * L + n].float().abs().mean())
                        t[b * L + n:(b + 1) * L] = (amp * torch.randn(L - n, t.shape[1], generator=g)).clamp(-6e4, 6e4).to(t.dtype).cuda()
                got = attention_f32_parts(qq, kk, vv, B, L, H, lengths=lens, **kw).view(B, L, D)
                for b, n in enumerate(lens):
                    solo = attention_f32_parts(*(t[b * L:b * L + n].contiguous() for t in (qq, kk, vv)), 1, n, H, **kw)
                    assert torch.equal(got[b, :n].contiguous().view(torch.int32), solo.view(torch.int32)), (name, B, H, kind, n)
                    assert bool((got[b, n:] == 0).all()), (name, B, H, kind, n)
                    if name == "f32":
                        sref, sunit = rr.attention32_ref64(qq[b * L:b * L + n], kk[b * L:b * L + n], vv[b * L:b * L + n, 2 * D:], 1, n, H)
                    else:
                        sq, sv = math.sqrt(kw["qk_scale_product"]), kw["v_scale"]
                        sref, sunit = _split_ref(qq[b * L:b * L + n], kk[b * L:b * L + n], vv[b * L:b * L + n], sq, sv, 1, n, H)
                    assert float(rr.ratio(solo, sref, F32, rr.ATT32_COEF * sunit).max()) <= 1.0, (name, "ragged", B, H, kind, n)
    # measured: coef <= 1.8 up to L = 129; at L = 258 f32 2.31, split 2.68, split scaled 3.24 of 32 (float32 torch: 5.92)
    print(f"MEASURED attention f32 parts L={L}: " + ", ".join(f"{k} coef {v:.2f}" for k, v in worst.items()) + f" of {rr.ATT32_COEF:g}")


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,FH", [(1, 4), (5, 4), (1, 512), (5, 512), (1, 4096), (5, 4096)])
def test_swiglu_f32_vs_float64(M, FH):
    """swiglu_f32_kernel: silu(g) u within SWIGLU_COEF ulp of |mid| + 2^-24 |u|, gates at -100, -20, 0, 20, 100 included."""
    from esmdiff_amd.engine import swiglu_f32
    gu = rr.swiglu_case(M, FH, seed=FH + M).cuda()
    ref, unit, floor = rr.swiglu_ref64(gu)
    got = swiglu_f32(gu)
    need = rr.swiglu_needed_coef(got, ref, unit, floor)
    # measured: coef 0.44 - 2.39
    print(f"MEASURED swiglu_f32 M={M} FH={FH}: coef {need:.2f} of {rr.SWIGLU_COEF:g}")
    assert bool(torch.isfinite(got).all())
    assert bool(((got.double() - ref).abs() <= rr.SWIGLU_COEF * unit + floor).all()), need


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K,S", [(300, 1536, 1536, 3), (300, 1536, 4096, 4), (1, 256, 768, 3)])
def test_gemm_split_k_and_its_reduce(M, N, K, S):
    """launch_gemm256w4_splitk + splitk_reduce_resid_kernel: x + ((p0 + p1) + ...) rs / div, bit-equal to the float32
    restatement from the slice planes the launch left; the pair within test_gemm_split_vs_float64's 1e-6 sum|a w|."""
    from esmdiff_amd.engine import gemm_split_k, split_rows, split_weight
    g = torch.Generator().manual_seed(M + N + K)
    A = torch.randn(M, K, generator=g) * (10.0 ** torch.randint(-2, 3, (M, 1), generator=g).float())
    A[:, ::7] *= 1e-3
    W = (torch.rand(N, K, generator=g) * 2 - 1) / K ** 0.5
    x0 = torch.randn(M, N, generator=g)
    div = 1.1547005
    a3, rs = split_rows(A.cuda())
    w3, inv = split_weight(W.cuda())
    x = x0.clone().cuda()
    parts = gemm_split_k(a3, rs, w3, inv, x, S, div=div)
    p = parts[:, :M].cpu()
    acc = p[0]
    for s in range(1, S):
        acc = acc + p[s]
    want = x0 + (acc * rs.cpu()[:, None]) / torch.tensor(div, dtype=F32)      # float32 on the host: IEEE division
    assert torch.equal(x.cpu().view(torch.int32), want.view(torch.int32)), float((x.cpu() - want).abs().max())
    ref = A.double() @ W.double().T
    mag = A.double().abs() @ W.double().abs().T
    rel = float((((acc * rs.cpu()[:, None]).double() - ref).abs() / mag).max())
    print(f"MEASURED gemm_split_k {M}x{N}x{K} S={S}: max err / sum|a w| {rel:.2e}")
    assert rel < 1e-6, rel                                                   # measured 4.7e-8 - 1.2e-7
    assert bool(((x.cpu().double() - (x0.double() + ref / div)).abs() <= 1e-6 * mag + 2.0 ** -23 * x0.double().abs() + 1e-6).all())


def test_gemm_split_k_refuses_what_the_launcher_refuses():
    from esmdiff_amd.engine import gemm_split_k
    for M, N, K, S in ((4, 256, 768, 1), (4, 128, 768, 3), (4, 256, 768, 5), (4, 256, 128, 2), (4, 256, 256, 3), (4, 256, 1536, 7)):
        a3 = torch.zeros(M, 3 * K, dtype=torch.float16, device="cuda")
        w3 = torch.zeros(N, 3 * K, dtype=torch.float16, device="cuda")
        x = torch.full((M, N), 7.0, device="cuda")
        with pytest.raises(RuntimeError, match="gemm_split_k"):
            gemm_split_k(a3, None, w3, 1.0, x, S)
        assert bool((x == 7.0).all())

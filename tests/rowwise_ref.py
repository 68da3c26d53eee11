"""Float64 references and error-model comparators of the row kernels that run between the GEMMs: block 0's geometric
attention (csrc/geom.hip), q/k LayerNorm + rotary and the fused residual add + LayerNorm (csrc/norm.hip), attention
(csrc/attention.hip).  tests/test_gpu_rowwise.py compares the kernels through them; tests/test_rowwise_bars_cpu.py shows
that the same comparators pass the float64 reference rounded to each build's type and reject planted errors.
The second half holds the same for the row kernels of the float32-grade engines (csrc/strict.hip, csrc/gemm_split.hip,
csrc/attention_split.hip): tests/test_gpu_f32_rows.py and tests/test_f32_rows_bars_cpu.py; and, after the float32-grade attention, for the 16-bit
attention kernel on operands handed to it (attention16_*: cases for its lazy rescale, reference, an emulation of its tile loop):
tests/test_gpu_attention16.py and tests/test_attention16_bars_cpu.py.

Every bar has the form  |got - ref| <= OUT_EPS[type] * |ref| + coef * unit : the first term is the output rounding of the
build (round to nearest: half an ulp, at most 2^-8 |x| for bfloat16, 2^-11 |x| for IEEE half, nothing for float32), the
second the arithmetic inside the kernel, in a unit that scales with the magnitudes it works on.  `ratio` returns the
left side over the right side per element; a kernel passes when every ratio is <= 1.
"""
from __future__ import annotations

import math

import torch

from esmdiff_amd.geometry import build_affine3d_from_coordinates
from oracle.geom_ref import geom_attend, geom_rotate_parts

OUT_EPS = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 0.0}
F32_EPS = 2.0 ** -24
LN_EPS = 1e-5
LOG2E = 1.4426950408889634


def ratio(got: torch.Tensor, ref: torch.Tensor, dtype: torch.dtype, abs_bar: torch.Tensor) -> torch.Tensor:
    """|got - ref| / (OUT_EPS[dtype] |ref| + abs_bar), float64, elementwise (abs_bar broadcasts)."""
    ref = ref.double()
    err = (got.double() - ref).abs()
    return torch.where(err == 0, torch.zeros_like(err), err / (OUT_EPS[dtype] * ref.abs() + abs_bar))


def needed_coef(got, ref, dtype, unit) -> float:
    """The smallest coef for which `ratio(got, ref, dtype, coef * unit)` stays <= 1: what the arithmetic term of a bar
    has to cover once the output rounding is paid (for the measured values written beside the asserts)."""
    ref = ref.double()
    over = ((got.double() - ref).abs() - OUT_EPS[dtype] * ref.abs()).clamp(min=0)
    return float(torch.where(over == 0, torch.zeros_like(over), over / unit).max())


# ---------------------------------------------------------------------------------------------------------------
# geometric attention.  Arithmetic error of the f32 walk over the keys: a logit of magnitude |s| carries ~|s| 2^-24, which
# moves an output by at most that times the spread of the value vectors; the running sums over L keys add ~sqrt(L) 2^-24
# of the largest value.  unit(b, h) = 2^-24 vmax (smax + sqrt(L)), vmax = largest value norm among the framed keys,
# smax = bound on |logit| from the largest rotated q, k and the largest distance between framed points.
GEOM_COEF = 2.0


def softplus64(raw) -> torch.Tensor:
    raw = torch.as_tensor(raw, dtype=torch.float64)
    return torch.where(raw > 20, raw, torch.log1p(torch.exp(raw)))


def geom_ref64(P: torch.Tensor, rot, trans, mask, raw_rot, raw_dist, *, key_mask=None, plant=None,
               max_bytes: float = 4e8):
    """P (B, L, 15 VH) exactly as the kernel received it -> (ref float64 (B, L, 3 VH), unit float64 (B, VH)).
    raw_rot / raw_dist: the RAW per-head scales.  Computed on P's device, chunked over heads.  plant(parts, heads) may
    modify the rotated parts in place (tests of the comparator only)."""
    B, L, C = P.shape
    VH = C // 15
    dev = P.device
    p = P.double()
    rot, trans = rot.to(dev, torch.float64), trans.to(dev, torch.float64)
    mask = mask.to(dev, torch.bool)
    km = mask if key_mask is None else key_mask.to(dev, torch.bool)
    w_rot, w_dist = softplus64(raw_rot).to(dev), softplus64(raw_dist).to(dev)
    ref = torch.empty(B, L, 3 * VH, dtype=torch.float64, device=dev)
    unit = torch.zeros(B, VH, dtype=torch.float64, device=dev)
    nh = max(1, min(VH, int(max_bytes // (B * L * L * 3 * 8 * 2))))
    kmf = km[:, None, :]                                                   # (B, 1, L)
    for h0 in range(0, VH, nh):
        heads = list(range(h0, min(VH, h0 + nh)))
        parts = list(geom_rotate_parts(p, rot, trans, heads))
        if plant is not None:
            plant(parts, heads)
        q_rot, k_rot, value, q_dist, k_dist = parts
        ref[..., 3 * h0:3 * heads[-1] + 3] = geom_attend(q_rot, k_rot, value, q_dist, k_dist, rot, mask, w_rot[heads],
                                                        w_dist[heads], key_mask=km)
        nrm = lambda t: t.norm(dim=-1).masked_fill(~kmf, 0).amax(-1)       # (B, h) over framed residues
        vmax, rmax = nrm(value), nrm(q_rot) * nrm(k_rot)
        cmax = torch.maximum(nrm(q_dist), nrm(k_dist))
        smax = (w_rot[heads] * rmax + w_dist[heads] * 2 * cmax) / math.sqrt(3)
        unit[:, h0:heads[-1] + 1] = F32_EPS * vmax * (smax + math.sqrt(L))
    return ref, unit


def chain_frames(B: int, L: int, patterns, seed: int):
    """Frames of a 3.8 A random-walk CA chain (N, C 1.46 / 1.52 A off CA in random directions) through
    esmdiff_amd.geometry.build_affine3d_from_coordinates.  patterns[b]: "all" framed; "gaps": NaN at BOS and EOS and an
    Inf run (the inpainting marker) at L/3 .. L/3 + L/4; "gaps2": the same with the run at L/2 ..; "none": no frames;
    "self": only residue L // 2 framed (its only framed key is itself)."""
    g = torch.Generator().manual_seed(seed)

    def unit_vec():
        u = torch.randn(B, L, 3, generator=g, dtype=torch.float64)
        return u / u.norm(dim=-1, keepdim=True)
    ca = torch.cumsum(3.8 * unit_vec(), 1)
    xyz = torch.stack([ca + 1.46 * unit_vec(), ca, ca + 1.52 * unit_vec()], 2).float()
    for b, pat in enumerate(patterns):
        if pat in ("gaps", "gaps2"):
            xyz[b, 0] = xyz[b, -1] = float("nan")
            s0 = L // 3 if pat == "gaps" else L // 2
            xyz[b, s0:s0 + max(1, L // 4)] = float("inf")
        elif pat == "none":
            xyz[b] = float("nan")
        elif pat == "self":
            keep = xyz[b, L // 2].clone()
            xyz[b] = float("inf")
            xyz[b, L // 2] = keep
        else:
            assert pat == "all", pat
    return build_affine3d_from_coordinates(xyz)


def geom_ratio(got, ref, unit, dtype, coef: float = GEOM_COEF) -> torch.Tensor:
    """Per (sample, query, head): the largest ratio of its 3 components."""
    B, L, C = ref.shape
    r = ratio(got.reshape(B, L, C // 3, 3), ref.reshape(B, L, C // 3, 3), dtype, coef * unit[:, None, :, None])
    return r.amax(-1)


# ---------------------------------------------------------------------------------------------------------------
# q/k LayerNorm + rotary.  The kernel's rotary tables hold cos / sin of the float32 angle (float)l * inv_freq, inv_freq =
# 1.0f / powf(10000, 2i / 64) (engine create); the reference takes the same float32 angle and evaluates it in float64.
# Arithmetic error: the f32 statistics move n = LN(x) w by ~2^-24 (|n| + rstd |w| max|x|) per element (the mean carries
# ~2^-24 max|x|, which a low-variance row multiplies by a large rstd), and rotary adds the partner's share:
# unit = 2^-24 (|n| + |n'| + rstd (|w| + |w'|) max|x|) times the q scale.
QK_COEF = 4.0
QSCALE = 0.125 * LOG2E


def rope_inv_freq() -> torch.Tensor:
    i = torch.arange(32, dtype=torch.float64)
    p = (10000.0 ** (2 * i / 64).float().double()).float()                # powf(10000, (float)(2i) / 64), rounded
    return torch.tensor(1.0, dtype=torch.float32) / p


def rope_tables(L: int, device) -> tuple:
    ang = torch.arange(L, dtype=torch.float32)[:, None] * rope_inv_freq()[None]   # float32 product, as at create
    ang = ang.double().to(device)
    return torch.cos(ang), torch.sin(ang)                                  # (L, 32)


def rotate_half(x: torch.Tensor, partner=None) -> torch.Tensor:
    """x (..., H, 64) -> [-x2, x1] per head (partner: a permutation of 0..63 that replaces the half swap, for plants)."""
    if partner is None:
        return torch.cat([-x[..., 32:], x[..., :32]], -1)
    sign = torch.cat([-torch.ones(32), torch.ones(32)]).to(x.device, x.dtype)
    return x[..., partner] * sign


def ln64(x: torch.Tensor, w, b=None, eps: float = LN_EPS):
    """float64 LayerNorm over the last dim -> (n * w + b, rstd (..., 1), max |x| (..., 1))."""
    x = x.double()
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    rstd = 1.0 / torch.sqrt((d * d).mean(-1, keepdim=True) + eps)
    y = d * rstd * w.double()
    if b is not None:
        y = y + b.double()
    return y, rstd, x.abs().amax(-1, keepdim=True)


def qk_rope_ref64(qkv: torch.Tensor, q_w, k_w, B: int, L: int, H: int, *, eps: float = LN_EPS, partner=None,
                  plant_head=None):
    """qkv [B*L, 3 H 64] exactly as the kernel received it -> ((q_ref, q_unit), (k_ref, k_unit)), float64 [B*L, H*64];
    q_ref carries the kernel's log2(e)/8 pre-scale.  partner / plant_head: a wrong rotate-half permutation in one head
    (tests of the comparator only)."""
    D = H * 64
    cos, sin = rope_tables(L, qkv.device)
    cos = torch.cat([cos, cos], -1).repeat(B, 1)[:, None, :]               # (B*L, 1, 64)
    sin = torch.cat([sin, sin], -1).repeat(B, 1)[:, None, :]
    out = []
    for which, w in ((0, q_w), (1, k_w)):
        x = qkv[:, which * D:(which + 1) * D].double()
        n, rstd, xmax = ln64(x, w.to(qkv.device), eps=eps)
        nh = n.view(-1, H, 64)
        rh = rotate_half(nh)
        if plant_head is not None:
            rh[:, plant_head] = rotate_half(nh[:, plant_head], partner)
        r = nh * cos + rh * sin
        wa = w.to(qkv.device).double().abs().view(H, 64)
        unit = nh.abs() + rotate_half(nh).abs() + rstd[:, :, None] * (wa + rotate_half(wa).abs()) * xmax[:, :, None]
        scale = QSCALE if which == 0 else 1.0
        out.append(((r * scale).reshape(-1, D), (F32_EPS * scale * unit).reshape(-1, D)))
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------
# attention (16-bit q, k, P and v operands, f32 accumulation): a relative operand error e on q and k moves a logit
# s = q.k / 8 by ~e |q| |k| / 8 and the 16-bit P by e, independently per key, so an output moves by about
# e (1 + |q| kmax / 8) sqrt(sum_k p_k^2 v_k^2): unit(b, h, query, channel) = OUT_EPS x that, in the 16-bit type's rounding.
ATT_COEF = 1.0


def attention_ref64(qkv: torch.Tensor, q_w, k_w, B: int, L: int, H: int, dtype: torch.dtype):
    """softmax(q k^T / 8) v per head in float64 from the 16-bit qkv the kernel received -> (ref, unit) [B*L, H*64]."""
    D = H * 64
    (q, _), (k, _) = qk_rope_ref64(qkv, q_w, k_w, B, L, H)
    q = (q / LOG2E).view(B, L, H, 64).transpose(1, 2)                       # natural-base logits: q / 8 . k
    k = k.view(B, L, H, 64).transpose(1, 2)
    v = qkv[:, 2 * D:].double().view(B, L, H, 64).transpose(1, 2)
    p = torch.softmax(q @ k.transpose(-1, -2), -1)
    ref = (p @ v).transpose(1, 2).reshape(B * L, D)
    qn = (q * 8).norm(dim=-1, keepdim=True)                                 # (B, H, L, 1)
    kmax = k.norm(dim=-1).amax(-1)[..., None, None]
    unit = OUT_EPS[dtype] * (1 + qn * kmax / 8) * torch.sqrt((p * p) @ (v * v))
    return ref, unit.transpose(1, 2).reshape(B * L, D)


# ---------------------------------------------------------------------------------------------------------------
# residual add + LayerNorm: v = (x + delta) + delta2 in float32 is exact arithmetic the kernel must match bit for bit;
# y = LayerNorm(v) w + b from f32 statistics: unit = 2^-24 (|y| + |n w| + rstd |w| max|v|).
LN_COEF = 4.0


# The bar's output term OUT_EPS |ref| describes a rounding to nearest only inside the normal range of the type.  Below 2^-14 an f16
# output is subnormal and rounds with half a spacing of 2^-25 whatever its size; without a bias y = n w crosses zero, so such outputs
# occur in every large case.  The arithmetic term covers them where LN_COEF 2^-24 rstd |w| max|v| >= 2^-25, i.e. rstd |w| max|v| >=
# 1/8.  A row of D >= 256 unit-variance values has rstd max|v| >= 2.6 (its largest value lies that many deviations out), so gains of
# at least 1 / 16 keep every f16 case inside the bar's model; below that the float64 reference itself, rounded to f16, misses the
# bar (tests/test_rowwise_bars_cpu.py: 8.6 x at |w| = 0.0036).  bfloat16 has float32's exponent range: no such floor.
LN_MIN_GAIN = 1.0 / 16


def ln_gains(D: int, g: torch.Generator) -> torch.Tensor:
    """w = 1 + 0.3 randn with |w| kept at or above LN_MIN_GAIN (sign kept)."""
    w = 1 + 0.3 * torch.randn(D, generator=g)
    return torch.where(w.abs() < LN_MIN_GAIN, torch.copysign(torch.tensor(LN_MIN_GAIN), w), w)


def add_ln_ref64(v32: torch.Tensor, w, b, *, eps: float = LN_EPS):
    """v32: the float32 sum (x + delta) + delta2 -> (ref float64, unit float64)."""
    y, rstd, vmax = ln64(v32, w, b, eps=eps)
    nw, _, _ = ln64(v32, w, None, eps=eps)
    return y, F32_EPS * (y.abs() + nw.abs() + rstd * w.double().abs() * vmax)


# ===============================================================================================================
# The float32-grade row kernels of F32 / F32_SPLIT engines (csrc/strict.hip, csrc/gemm_split.hip, csrc/attention_split.hip):
# tests/test_gpu_f32_rows.py compares them through what follows, tests/test_f32_rows_bars_cpu.py shows that the same
# comparators pass the float64 reference rounded to float32 and a torch float32 evaluation, and reject planted defects.
# OUT_EPS[float32] = 0: every bar below is coef x an arithmetic unit alone.

def gelu64(x: torch.Tensor, tanh: bool = False) -> torch.Tensor:
    """Exact (erf) GELU in float64; tanh: the approximation the kernels must NOT compute (plants only)."""
    x = x.double()
    if tanh:
        return 0.5 * x * (1 + torch.tanh(math.sqrt(2 / math.pi) * (x + 0.044715 * x ** 3)))
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2)))


def ln_rows_ref64(x32: torch.Tensor, w, b, *, gelu_in: bool = False, delta=None, eps: float = LN_EPS, tanh_gelu: bool = False,
                  delta_times: int = 1):
    """layernorm_f32_kernel / layernorm_split_kernel: LayerNorm of x (+ delta: the float32 sum x + float(delta) is exact
    arithmetic, the reference starts from it), or of the exact-erf GELU of x -> (ref, unit) float64 under LN_COEF.  With
    gelu_in the unit gains 4 x 2^-24 rstd |w| max|gelu(x)| for the f32 erff.  tanh_gelu / delta_times: plants."""
    v = x32
    for _ in range(delta_times if delta is not None else 0):
        v = v + delta.float()
    if not gelu_in:
        return add_ln_ref64(v, w, b, eps=eps)
    g = gelu64(v, tanh_gelu)
    ref, unit = add_ln_ref64(g, w, b, eps=eps)
    _, rstd, _ = ln64(gelu64(v), w, None, eps=eps)
    return ref, unit + 4 * F32_EPS * rstd * w.double().abs() * gelu64(v).abs().amax(-1, keepdim=True)


LN_ROW_KINDS = ("unit", "low_variance", "scale_1e4", "spike", "zero")
LN_LOW_VARIANCE, LN_ZERO = 1, 4                                             # indices into LN_ROW_KINDS


def ln_case(M: int, D: int, seed: int, gain: float, first_kind: int = 0):
    """(x f32 [M, D], w, b, delta f32 [M, D], kinds [M]): row r is of kind LN_ROW_KINDS[(first_kind + r) % 5] — unit normal;
    low variance (5 + 2e-3 randn: eps = 1e-5 matters, the mean's rounding is multiplied by a large rstd); scale 1e4; a single
    1e3 spike over 1e-2 noise; all zero (row_scale's clamp: finite rs, a zero split when there is no bias).  w = gain (1 + 0.3
    randn), b = 0.2 gain randn; delta (a 16-bit branch output, to be rounded by the caller) is 1e-3 of the row's own spread on
    the low-variance row so that the row stays one."""
    g = torch.Generator().manual_seed(seed)
    kinds = (first_kind + torch.arange(M)) % 5
    x = torch.randn(M, D, generator=g)
    delta = torch.randn(M, D, generator=g)
    for r in range(M):
        kd = int(kinds[r])
        if kd == 1:
            x[r] = 5 + 2e-3 * x[r]
            delta[r] *= 2e-6
        elif kd == 2:
            x[r] *= 1e4
        elif kd == 3:
            x[r] *= 1e-2
            x[r, (7 * r + 3) % D] = 1e3
        elif kd == 4:
            x[r] = 0
    w = gain * (1 + 0.3 * torch.randn(D, generator=g))
    b = 0.2 * gain * torch.randn(D, generator=g)
    return x, w, b, delta, kinds


# ---- split rows (gemm_split.hip: row_scale / split4; attention_split.hip: split_pair).  a = y s with s a power of two; hi =
# f16(a) to nearest, lo = f16(a - hi): |a - hi| <= 2^-11 |a| (half an ulp of 11 bits), lo rounds that to 11 bits again or,
# below f16's normal range, to the subnormal spacing 2^-24: |hi + lo - a| <= max(2^-22 |a|, 2^-25).  Derived, not measured.
SPLIT_REL, SPLIT_ABS = 2.0 ** -22, 2.0 ** -25


def split_bar(a: torch.Tensor) -> torch.Tensor:
    return torch.clamp(SPLIT_REL * a.double().abs(), min=SPLIT_ABS)


def split_emulate(y32: torch.Tensor, s: torch.Tensor, *, toward_zero: bool = False):
    """What split4 computes from the f32 values y32 and the power-of-two scale s (broadcast): (hi, lo) float16.
    toward_zero: hi truncated instead of rounded to nearest (a plant)."""
    a = y32.float() * s.float()
    hi = a.half()
    if toward_zero:
        up = hi.float().abs() > a.abs()                                     # rounded away from zero: step one f16 back
        bits = hi.view(torch.int16) - up.to(torch.int16)                   # sign-magnitude: the magnitude's predecessor
        hi = bits.view(torch.float16)
    lo = (a - hi.float()).half()
    return hi, lo


def row_scale_ref(y32: torch.Tensor) -> torch.Tensor:
    """row_scale's rs = 1 / s per row of y32 (f32 [M, D]): 2^(e - 14), e the exponent of the row maximum clamped as the kernel
    clamps it (biased 20 .. 250), so that the maximum lands in [2^14, 2^15).  float32 [M]."""
    amax = y32.float().abs().amax(-1)
    eb = ((amax.view(torch.int32) >> 23) & 0xff).clamp(20, 250)
    return ((eb - 14) << 23).to(torch.int32).view(torch.float32)


def split_planes(a3: torch.Tensor, D: int, planes: int = 3):
    """a3 f16 [M, planes D] -> (hi, lo) float64 and, for the GEMM's [hi | lo | hi] rows, the third plane (else None)."""
    hi, lo = a3[:, :D], a3[:, D:2 * D]
    return hi.double(), lo.double(), (a3[:, 2 * D:3 * D] if planes == 3 else None)


def half_ulp_f16(hi: torch.Tensor) -> torch.Tensor:
    """Half the spacing of float16 at hi (float64 values of f16 numbers): 2^(e - 11) for |hi| in [2^e, 2^(e+1)), 2^-25 below 2^-14."""
    _, e = torch.frexp(hi)                                                   # |hi| = m 2^e, m in [0.5, 1)
    # 2^(e - 12) from its exponent bits: exact on every device (a device pow / ldexp may miss a power of two by an ulp)
    half = ((e.to(torch.int64) - 12 + 1023).clamp(min=1) << 52).view(torch.float64)
    return torch.where(hi == 0, torch.full_like(hi, 2.0 ** -25), torch.clamp(half, min=2.0 ** -25))


def split_rows_report(a3: torch.Tensor, rs: torch.Tensor, y32: torch.Tensor) -> dict:
    """Every property of a split row [hi | lo | hi] + rs against the f32 row y32 it was made from, located per row:
      value   [M, D] |hi + lo - y / rs| over split_bar (<= 1 passes)
      rs_ok   [M]    rs is exactly row_scale's power of two for this row (finite, also on an all-zero row)
      planes  [M]    plane 2 equals plane 0 bit for bit
      range   [M]    max |hi| in [2^14, 2^15] (closed: a maximum that rounds up to 32768 passes); all-zero rows: a zero split
      nearest [M]    |lo| <= half an ulp of hi: hi was rounded to nearest, not toward zero (then |lo| reaches a whole ulp)
      finite  [M]    """
    D = y32.shape[-1]
    hi, lo, hi2 = split_planes(a3, D)
    a = y32.double() / rs.double()[:, None]
    err = (hi + lo - a).abs()
    value = torch.where(err == 0, torch.zeros_like(err), err / split_bar(a))
    want = row_scale_ref(y32).to(rs.device)
    hmax = hi.abs().amax(-1)
    zero_row = y32.abs().amax(-1) == 0
    rng = torch.where(zero_row, (a3.float().abs().amax(-1) == 0), (hmax >= 2.0 ** 14) & (hmax <= 2.0 ** 15))
    return {"value": value, "rs_ok": (rs == want) & torch.isfinite(rs) & (rs > 0),
            "planes": (a3[:, :D].view(torch.int16) == hi2.view(torch.int16)).all(-1), "range": rng,
            "nearest": (lo.abs() <= half_ulp_f16(hi)).all(-1),
            "finite": torch.isfinite(a3.float()).all(-1) & torch.isfinite(value).all(-1)}


def split_rows_ok(rep: dict) -> bool:
    return bool((rep["value"] <= 1).all() and rep["rs_ok"].all() and rep["planes"].all() and rep["range"].all()
                and rep["nearest"].all() and rep["finite"].all())


def split_rows_explain(rep: dict, a3: torch.Tensor, rs: torch.Tensor, y32: torch.Tensor) -> str:
    """What failed in a split_rows_report and the numbers of the first offending element, for an assert's message."""
    D = y32.shape[-1]
    hi, lo, _ = split_planes(a3, D)
    out = []
    for key, v in rep.items():
        bad = (v > 1) if key == "value" else ~v
        if not bool(bad.any()):
            continue
        r = int(bad.reshape(bad.shape[0], -1).any(-1).nonzero()[0])
        el = (lo[r].abs() > half_ulp_f16(hi[r])) if key == "nearest" else (rep["value"][r] > 1)
        c = int(el.nonzero()[0]) if bool(el.any()) else int(y32[r].abs().argmax())
        out.append(f"{key}: row {r} col {c} y {float(y32[r, c])!r} rs {float(rs[r])!r} hi {float(hi[r, c])!r} lo {float(lo[r, c])!r} "
                   f"value ratio {float(rep['value'][r, c]):.3f} max|hi| {float(hi[r].abs().max())!r}")
    return "; ".join(out)


def is_pow2(v: float) -> bool:
    return v > 0 and math.isfinite(v) and math.frexp(v)[0] == 0.5


# ---- q/k LayerNorm + rotary of the float32-grade engines: qk_rope_ref64 with its q scale replaced by the kernel's own
# The q/k LayerNorm gain the tests pair with each split scale: |row| <= sqrt(D - 1) max|w| scale must stay inside f16 (the rule
# the engine picks its scale by): gains of 6 up to 2^6 (45 x 12 x 64 = 35 000 at D = 2048), 0.05 at 2^13 (45 x 0.1 x 8192 = 37 000).
QK_SPLIT_GAIN = {1.0: 6.0, 2.0 ** 6: 6.0, 2.0 ** 13: 0.05}


def qk_rope_f32_ref64(qkv, q_w, k_w, B, L, H, *, q_scale: float = 1.0, k_scale: float = 1.0, **plant):
    """((q_ref, q_unit), (k_ref, k_unit)) for qk_norm_rope_f32_kernel (no scale) / qk_norm_rope_split_kernel (the rotated rows
    times q_scale / k_scale: reference and unit carry the same factor).  Bar: QK_COEF x unit, plus split_bar(ref) for the
    split form's hi + lo."""
    (q, qu), (k, ku) = qk_rope_ref64(qkv, q_w, k_w, B, L, H, **plant)
    return (q * (q_scale / QSCALE), qu * (q_scale / QSCALE)), (k * k_scale, ku * k_scale)


# ---- attention in float32 grade (attention_f32_kernel: fmaf chains; attention_split_kernel: split operands, exact products,
# f32 accumulation).  A logit s = q.k / 8 carries ~2^-24 |q| |k| / 8 of accumulation error, which moves p_k by that
# relative amount; exp, the running sums and the final division add ~2^-24 each:
# unit(b, h, query, channel) = 2^-24 (1 + |q| kmax / 8) sum_k p_k |v_k|.
# ATT32_COEF = 4 x the largest needed_coef of a plain torch float32 evaluation of the same formula on the test's own inputs
# (attention_cases below), rounded up to a power of two.  Measured on the CPU (tests/test_f32_rows_bars_cpu.py, EXPERIMENTS.md):
# float32 torch needs 1.29 (unit), 2.47 / 2.18 (gains 4 / 8), 1.74 (one_key), 1.16 (falling staircase) and 5.92 on the rising
# staircase at L = 258 (q and k
# nearly parallel with |q| |k| / 8 = 20: every partial sum of the 64-term dot product rounds in the same direction)
# -> 4 x 5.92 = 23.7 -> 32.
ATT32_COEF = 32.0


def attention32_ref64(q, k, v, B: int, L: int, H: int, *, drop_last_key: bool = False):
    """softmax(q k^T / 8) v per head in float64 from q, k, v [B*L, H*64] as the kernel was handed them -> (ref, unit)."""
    D = H * 64
    q, k, v = (t.double().view(B, L, H, 64).transpose(1, 2) for t in (q, k, v))
    s = q @ k.transpose(-1, -2) / 8
    if drop_last_key:
        s[..., -1] = -float("inf")
    p = torch.softmax(s, -1)
    ref = (p @ v).transpose(1, 2).reshape(B * L, D)
    qn = q.norm(dim=-1, keepdim=True)
    kmax = k.norm(dim=-1).amax(-1)[..., None, None]
    unit = F32_EPS * (1 + qn * kmax / 8) * (p @ v.abs())
    return ref, unit.transpose(1, 2).reshape(B * L, D)


def attention32_torch(q, k, v, B: int, L: int, H: int) -> torch.Tensor:
    """The same formula evaluated by torch in float32 (what ATT32_COEF is calibrated on)."""
    q, k, v = (t.float().view(B, L, H, 64).transpose(1, 2) for t in (q, k, v))
    p = torch.softmax(q @ k.transpose(-1, -2) / 8, -1)
    return (p @ v).transpose(1, 2).reshape(B * L, H * 64)


LN2_8 = 8 * math.log(2.0)                                                   # 1 / (log2(e) / 8)


def split_operand(x32: torch.Tensor, scale: float) -> torch.Tensor:
    """[hi | lo] float16 rows of x32 * scale (float32 product), as qk_norm_rope_split / v_split hand them to the attention."""
    hi, lo = split_emulate(x32, torch.tensor(scale, dtype=torch.float32, device=x32.device))
    return torch.cat([hi, lo], -1).contiguous()


def split_operand_value(x2: torch.Tensor, scale: float) -> torch.Tensor:
    """(hi + lo) / scale in float64: the operand the split attention really multiplies (its rounding is not charged twice)."""
    D = x2.shape[-1] // 2
    return (x2[:, :D].double() + x2[:, D:].double()) / scale


ATT_KINDS = ("unit", "gain4", "gain8", "stairs_up", "stairs_down", "one_key")
# ... and what the 16-bit kernel gets on top (attention16_* below): its lazy-rescale threshold is 8 log2 units, not 4
ATT16_KINDS = ATT_KINDS + ("stairs_up7", "stairs_down7", "last_key", "first_key", "lone_query", "flat")
# L: one stage (<= 64), the HALF tail (tail <= 32), the masked tail, exact tiles, 1 to 4 waves of 32 queries, several query blocks
ATT_LS = (1, 31, 32, 33, 64, 65, 96, 97, 128, 129, 258)
ATT_BH = ((1, 1), (3, 3), (2, 8))                                           # B H = 1, 9 (XCD slots left empty), 16


def attention_case(kind: str, B: int, L: int, H: int, seed: int, lens=None):
    """q, k, v float32 [B*L, H*64] (CPU).  unit / gain4 / gain8: N(0, 1) rows times 1 / 4 / 8 on q and k (trained q/k LayerNorm
    gains).  stairs_up / stairs_down: the best logit rises / falls by 5 nats (7.2 log2 units, above the split kernel's lazy-rescale
    threshold of 4) from one 64-key tile to the next: a rescale at every tile, or never after the first.  one_key: key 2L/3
    carries all the mass, every other p is below 2^-13 (the lo part of P is subnormal).
    The kinds ATT16_KINDS adds, for the 16-bit kernel and its threshold of 8 (under which the 5-nat staircase lags: P reaches 2^7.2
    and the maximum is raised at every second tile): stairs_up7 / stairs_down7: the staircase with 7 nats (10.1 log2 units) per
    tile.  last_key / first_key: one_key with the heavy key at L - 1 (the sample's own last valid key, lens[b] - 1, when lens is
    given) / at 0.  lone_query: the keys of stairs_up7 under unit-size queries, except query 32 w + (5 + 7 w) % 32 of every wave
    w of 32 queries, which is aligned with the staircase: one lane decides for its wave.  flat: q = 0, every output is the mean
    of the V rows."""
    g = torch.Generator().manual_seed(seed)
    shape = (B, L, H, 64)
    q, k, v = (torch.randn(shape, generator=g) for _ in range(3))
    if kind.startswith("gain"):
        q, k = q * float(kind[4:]), k * float(kind[4:])
    elif kind == "flat":
        q = torch.zeros(shape)
    elif kind != "unit":
        u = torch.randn(B, 1, H, 64, generator=g)
        u = u / u.norm(dim=-1, keepdim=True)
        if kind == "lone_query":
            for q0 in range(0, L, 32):
                i = q0 + (5 + 7 * (q0 // 32)) % 32
                if i < L:
                    q[:, i] = 8 * u[:, 0] + 0.3 * q[:, i]
        else:
            q = 8 * u + 0.3 * q                                              # q . k / 8 = (u . k) + noise
        if kind in ("one_key", "last_key", "first_key"):
            k = 0.3 * k
            for b in range(B):
                n = L if lens is None else int(lens[b])
                at = {"one_key": (2 * n) // 3, "last_key": n - 1, "first_key": 0}[kind]
                k[b, at] = 12 * u[b, 0] + 0.3 * k[b, at]
        else:
            step = {"stairs_up": 5.0, "stairs_down": -5.0, "stairs_up7": 7.0, "stairs_down7": -7.0, "lone_query": 7.0}[kind]
            tile = (torch.arange(L) // 64).float()[None, :, None, None]
            k = 0.3 * k + step * tile * u
    return tuple(t.reshape(B * L, H * 64).contiguous() for t in (q, k, v))


# ---- the 16-bit attention kernel alone (csrc/attention.hip, attention_kernel.inc; esmdiff_attention_16_parts): its operands are
# handed to it, so q and k carry no rounding of their own and the float64 reference starts from the very 16-bit values.
# What is left: P = exp2(s - m) is rounded to the 16-bit type before P . V, independently per key: OUT_EPS sqrt(sum_k p_k^2 v_k^2);
# and the float32 score arithmetic, as for the float32-grade kernels above: 2^-24 (1 + |q| kmax / 8) sum_k p_k |v_k|.
#   unit = OUT_EPS[dtype] sqrt((p p) @ (v v)) + 2^-24 (1 + |q| kmax / 8) (p @ |v|);   bar = OUT_EPS |ref| + ATT16_COEF unit
# ATT16_COEF = 4 x the largest needed_coef of attention16_emulate (the kernel's own arithmetic on the CPU, no plant) over every
# case tests/test_gpu_attention16.py runs (attention16_runs, the ragged batch included), rounded up to a power of two.  Measured
# on the CPU (tests/test_attention16_bars_cpu.py, EXPERIMENTS.md): the bf16 emulation needs 1.97 (stairs_down7 at B H L = 2 8 97; 1.71
# on unit rows), the f16 one 1.77 on the staircases and unit rows but 12.50 on one_key at B H L = 3 3 32 (9.67 gain4, 7.38
# last_key, 6.79 first_key): one key holds all the mass, so in the channels where its v is near 0 the output and the other
# keys' P (~1e-5) lie below f16's normal range 2^-14, where the spacing is 2^-24 whatever the value and the unit's relative 2^-11
# no longer describes a rounding.  4 x 12.50 = 50 -> 64.
# ATT16_COEF_BUILD: the same rule on each build's own figures (bf16: 4 x 1.97 = 7.9 -> 8), so that the wide subnormal range of
# f16 does not loosen the bar of the default bf16 engine eightfold.  The tests assert the build's bar, which implies ATT16_COEF's.
# The kernels themselves, measured on an MI355X (tests/test_gpu_attention16.py): bf16 1.97, f16 12.50, at the same cases — the
# emulation's figures to the third digit up to L = 129, within 0.03 of them at L = 258 and 1026.
ATT16_COEF = 64.0
ATT16_COEF_BUILD = {torch.bfloat16: 8.0, torch.float16: 64.0}
ATT16_THR = 8.0                                                             # attention_kernel.inc: THR, log2 units
ATT16_LS = ATT_LS
ATT16_LONG = ((1, 1, 1026), ("stairs_up7", "stairs_up", "gain8"))           # one long chain: 17 tiles, 33 waves
ATT16_RAGGED_LENS = (3, 33, 64, 65, 97, 129, 258)
ATT16_RAGGED_H = 3
ATT16_RAGGED_KINDS = ("gain8", "stairs_up7", "last_key")
# the flat check needs no softmax reference: l = the number of keys and every P = 1 are exact, O is a float32 sum of L 16-bit values
# (about 2^-24 of a partial sum ~ sqrt(L) sigma per addition: ~2^-24 sigma after the division by L) times a rounded 1 / L:
# OUT_EPS |mean| + 4 x 2^-24 max|v|
ATT16_FLAT_ABS = 4 * F32_EPS


def attention16_runs():
    """(B, H, L, kinds) of every plain launch of tests/test_gpu_attention16.py::test_attention16_parts_vs_float64."""
    for L in ATT16_LS:
        for B, H in ATT_BH + (((1, 24),) if L == 258 else ()):
            yield B, H, L, ATT16_KINDS
    (B, H, L), kinds = ATT16_LONG
    yield B, H, L, kinds


def attention16_operands(q, k, v, dtype: torch.dtype):
    """What the kernel is handed, from a case's float32 q, k, v: q times log2(e)/8 (a float32 product, as qk_norm_rope forms
    it) and k rounded to dtype; qkv [*, 3 D] with v rounded in its last third and NaN in the q and k thirds, which the kernel
    must not read."""
    qs = torch.tensor(QSCALE, dtype=torch.float32, device=q.device)
    q16, k16, v16 = (q.float() * qs).to(dtype), k.to(dtype), v.to(dtype)
    nan = torch.full_like(v16, float("nan"))
    return q16.contiguous(), k16.contiguous(), torch.cat([nan, nan, v16], 1).contiguous()


def _per_sample(fn, tensors, B, L, H, lens, out_dtype):
    """fn(sample's rows ..., n) at each sample's own length; rows from lens[b] on stay +0."""
    outs = None
    for b, n in enumerate(lens):
        res = fn(*(t[b * L:b * L + int(n)] for t in tensors), int(n))
        res = res if isinstance(res, tuple) else (res,)
        if outs is None:
            outs = tuple(torch.zeros(B * L, H * 64, dtype=out_dtype, device=r.device) for r in res)
        for o, r in zip(outs, res):
            o[b * L:b * L + int(n)] = r
    return outs if len(outs) > 1 else outs[0]


def attention16_ref64(q16, k16, qkv16, B: int, L: int, H: int, dtype: torch.dtype, lens=None):
    """softmax(q k^T / 8) v per head in float64 from the 16-bit operands the kernel was handed (q16 / (log2(e)/8) is q) ->
    (ref, unit) [B*L, H*64] on the operands' device.  lens: every sample at its own length, (0, 0) on its padded rows."""
    D = H * 64
    if lens is not None:
        return _per_sample(lambda a, b, c, n: attention16_ref64(a, b, c, 1, n, H, dtype), (q16, k16, qkv16), B, L, H, lens,
                           torch.float64)
    q = (q16.double() / QSCALE).view(B, L, H, 64).transpose(1, 2)
    k = k16.double().view(B, L, H, 64).transpose(1, 2)
    v = qkv16[:, 2 * D:].double().view(B, L, H, 64).transpose(1, 2)
    p = torch.softmax(q @ k.transpose(-1, -2) / 8, -1)
    ref = (p @ v).transpose(1, 2).reshape(B * L, D)
    qn = q.norm(dim=-1, keepdim=True)
    kmax = k.norm(dim=-1).amax(-1)[..., None, None]
    unit = OUT_EPS[dtype] * torch.sqrt((p * p) @ (v * v)) + F32_EPS * (1 + qn * kmax / 8) * (p @ v.abs())
    return ref, unit.transpose(1, 2).reshape(B * L, D)


ATT16_PLANTS = ("no_o_rescale", "no_l_rescale", "drop_last_key", "tail_key_twice")


def attention16_emulate(q16, k16, qkv16, B: int, L: int, H: int, dtype: torch.dtype, lens=None, *, thr: float = ATT16_THR,
                        plant=None, stats=None):
    """attention_kernel.inc's arithmetic in torch: float32 scores of the 16-bit operands (base 2: q16 carries log2(e)/8), keys in
    tiles of 64 (a last tile of at most 32 valid keys computes 32; keys past the end are the clamped row L - 1 at a score of
    -1e30), per wave of 32 queries one decision to raise the running maxima — when any of its queries' tile maximum exceeds its
    running maximum by more than thr — with O and l of every query of the wave rescaled by exp2(m_old - m_new); P = exp2(s - m)
    summed unrounded into l and rounded to dtype for P . V, float32 O, then O * (1 / l) rounded to dtype -> [B*L, H*64] dtype.
    stats (a dict): "tiles" and "raises" count the (head, wave, tile) steps after each wave's first tile and the raises among
    them; "pmax" the largest P.  plant (tests of the comparator only): no_o_rescale / no_l_rescale: O / l keeps its old scale
    on a raise after tile 0; drop_last_key: key L - 1 is masked; tail_key_twice: the first clamped key of a partial last tile
    (a copy of key L - 1) is not masked."""
    assert plant is None or plant in ATT16_PLANTS, plant
    D = H * 64
    if lens is not None:
        return _per_sample(lambda a, b, c, n: attention16_emulate(a, b, c, 1, n, H, dtype, thr=thr, plant=plant, stats=stats),
                           (q16, k16, qkv16), B, L, H, lens, dtype)
    f32 = torch.float32
    q, k, v = (t.float().view(B, L, H, 64).transpose(1, 2) for t in (q16, k16, qkv16[:, 2 * D:]))   # (B, H, L, 64)
    out = torch.empty(B, H, L, 64, dtype=dtype, device=q.device)
    nkt = (L + 63) // 64
    tail = L - (nkt - 1) * 64
    for q0 in range(0, L, 32):
        qw = q[:, :, q0:q0 + 32]
        nq = qw.shape[2]
        m = torch.full((B, H, nq), -1e30, dtype=f32, device=q.device)
        l = torch.zeros(B, H, nq, dtype=f32, device=q.device)
        o = torch.zeros(B, H, nq, 64, dtype=f32, device=q.device)
        for kt in range(nkt):
            last = kt == nkt - 1
            idx = kt * 64 + torch.arange(32 if last and tail <= 32 else 64, device=q.device)
            valid = idx < (L + 1 if plant == "tail_key_twice" and last else L)
            if plant == "drop_last_key":
                valid = valid & (idx != L - 1)
            src = idx.clamp(max=L - 1)
            s = qw @ k[:, :, src].transpose(-1, -2)
            s = torch.where(valid, s, torch.full_like(s, -1e30))
            mx = s.amax(-1)
            up = ((mx - m) > thr).any(-1, keepdim=True)                      # wave-wide: (B, H, 1)
            m_new = torch.maximum(m, mx)
            alpha = torch.exp2(m - m_new)
            m = torch.where(up, m_new, m)
            if not (plant == "no_l_rescale" and kt > 0):
                l = torch.where(up, l * alpha, l)
            if not (plant == "no_o_rescale" and kt > 0):
                o = torch.where(up[..., None], o * alpha[..., None], o)
            p = torch.exp2(s - m[..., None])
            l = l + p.sum(-1)
            o = o + p.to(dtype).float() @ v[:, :, src]
            if stats is not None:
                stats["pmax"] = max(stats.get("pmax", 0.0), float(p.max()))
                if kt > 0:
                    stats["tiles"] = stats.get("tiles", 0) + up.numel()
                    stats["raises"] = stats.get("raises", 0) + int(up.sum())
        out[:, :, q0:q0 + nq] = (o * (1.0 / l)[..., None]).to(dtype)
    return out.transpose(1, 2).reshape(B * L, D)


# ---- SwiGLU of the F32 engine (swiglu_f32_kernel): mid = silu(g) u = g / (1 + exp(-g)) u.  exp, the add, the division and the
# product round once each: a few 2^-24 of |mid|; where exp(-g) overflows float32 (g < -88.7) the kernel gives 0 for a true
# |silu(g)| < 2^-122: covered by 2^-24 |u|.  bar = SWIGLU_COEF 2^-24 |mid| + 2^-24 |u|.
# SWIGLU_COEF = 4 x the largest needed coefficient of torch's float32 silu(g) * u on swiglu_case's rows, rounded up to a power
# of two.  Measured on the CPU: 2.39 -> 4 x 2.39 = 9.6 -> 16.
SWIGLU_COEF = 16.0
SWIGLU_G = (-100.0, -20.0, 0.0, 20.0, 100.0)


def swiglu_case(M: int, FH: int, seed: int) -> torch.Tensor:
    """gu float32 [M, 2 FH] = [gate | up]: gates N(0, 3), the first columns of every row at -100, -20, 0, 20, 100 (as far as
    FH reaches); ups N(0, 1) over three decades."""
    g = torch.Generator().manual_seed(seed)
    gate = 3 * torch.randn(M, FH, generator=g)
    n = min(FH, len(SWIGLU_G))
    gate[:, :n] = torch.tensor(SWIGLU_G[:n])
    up = torch.randn(M, FH, generator=g) * 10 ** torch.randint(-1, 2, (M, FH), generator=g).float()
    return torch.cat([gate, up], 1).contiguous()


def swiglu_ref64(gu: torch.Tensor):
    """-> (ref, unit = 2^-24 |ref|, floor = 2^-24 |u|) float64; bar = SWIGLU_COEF unit + floor."""
    FH = gu.shape[1] // 2
    g, u = gu[:, :FH].double(), gu[:, FH:].double()
    ref = g * torch.sigmoid(g) * u
    return ref, F32_EPS * ref.abs(), F32_EPS * u.abs()


def swiglu_needed_coef(got, ref, unit, floor) -> float:
    over = ((got.double() - ref).abs() - floor).clamp(min=0)
    return float(torch.where(over == 0, torch.zeros_like(over), over / unit).max())

"""Float64 references and error-model comparators of the row kernels that run between the GEMMs: block 0's geometric
attention (csrc/geom.hip), q/k LayerNorm + rotary and the fused residual add + LayerNorm (csrc/norm.hip), attention
(csrc/attention.hip).  tests/test_gpu_rowwise.py compares the kernels through them; tests/test_rowwise_bars_cpu.py shows
that the same comparators pass the float64 reference rounded to each build's type and reject planted errors.

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


def add_ln_ref64(v32: torch.Tensor, w, b, *, eps: float = LN_EPS):
    """v32: the float32 sum (x + delta) + delta2 -> (ref float64, unit float64)."""
    y, rstd, vmax = ln64(v32, w, b, eps=eps)
    nw, _, _ = ln64(v32, w, None, eps=eps)
    return y, F32_EPS * (y.abs() + nw.abs() + rstd * w.double().abs() * vmax)

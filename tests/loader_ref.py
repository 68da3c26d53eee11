"""Plain torch / float64 statements of what a create does to each tensor of a state dict (csrc/convert.hip, the weight half of
csrc/gemm_split.hip and csrc/attention_split.hip) and of the input stage (csrc/embed.hip, the 16-bit-input LayerNorm of
csrc/norm.hip), written from the documented contracts, with the comparators tests/test_gpu_loader.py applies to the kernels.
tests/test_loader_cpu.py shows that each comparator passes its own reference and rejects a planted error.

Everything a conversion, the interleave, the split and the input stage produce is determined bit for bit, so their comparator is
equality of the integer views (`same_bits`: a NaN matches any NaN, nothing else is forgiven).  Three results carry float32
arithmetic and get a derived bar instead: the row-norm maximum, the sigma MLP, the LayerNorm (tests/rowwise_ref.py's)."""
from __future__ import annotations

import math

import torch

from esmdiff_amd import constants as C
from tests import rowwise_ref as rr

F32_EPS = rr.F32_EPS
F16_MAX = 65504.0
INT_VIEW = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32}


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(INT_VIEW[t.dtype])


def from_bits(patterns, dtype: torch.dtype) -> torch.Tensor:
    """Unsigned bit patterns (ints) -> a tensor of `dtype` that holds exactly them."""
    n = 16 if dtype != torch.float32 else 32
    v = torch.tensor([p - (1 << n) if p >= (1 << (n - 1)) else p for p in patterns], dtype=INT_VIEW[dtype])
    return v.view(dtype)


def same_bits(got: torch.Tensor, want: torch.Tensor, signed_zero_ok: torch.Tensor | None = None) -> torch.Tensor:
    """Elementwise: the bits are equal, or both are NaN (the payload of a NaN is not part of any contract here).
    signed_zero_ok (bool, the inputs that are float32 denormals): there, a zero of the reference's sign passes too — a device
    may flush a float32 denormal on its way through an arithmetic instruction."""
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    ok = (bits(got) == bits(want)) | (torch.isnan(got) & torch.isnan(want))
    if signed_zero_ok is not None:
        ok = ok | (signed_zero_ok & (got == 0) & (torch.signbit(got) == torch.signbit(want)))
    return ok


def all_same_bits(got, want, signed_zero_ok=None) -> bool:
    """The bit-for-bit assert: torch.equal on the integer views once the positions where the reference is NaN (and the result
    must be) and the allowed flushed denormals are set aside."""
    ok = same_bits(got, want, signed_zero_ok)
    exact = bits(got) == bits(want)
    forgiven = ok & ~exact
    return bool(ok.all()) and torch.equal(bits(got).masked_fill(forgiven, 0), bits(want).masked_fill(forgiven, 0))


# ---- conversions ------------------------------------------------------------------------------------------------------------
def convert_ref(x: torch.Tensor, dst: torch.dtype) -> torch.Tensor:
    """float32 / bfloat16 -> bfloat16: round to nearest even, overflow to inf; -> float16: clamp to +-65504 then round to nearest
    even (inf saturates, NaN stays NaN); -> float32: exact."""
    if dst == torch.bfloat16:
        return x.float().bfloat16()
    if dst == torch.float16:
        return x.float().clamp(-F16_MAX, F16_MAX).half()
    assert dst == torch.float32
    return x.float()


def is_f32_denormal(x: torch.Tensor) -> torch.Tensor:
    """Non-zero with a zero float32 exponent field (every bfloat16 denormal is one too)."""
    a = x.float().abs()
    return (a > 0) & (a < 2.0 ** -126)


def convert_truncating_bf16(x: torch.Tensor) -> torch.Tensor:
    """A plant: the low 16 bits dropped instead of rounded."""
    return (x.float().view(torch.int32) >> 16).to(torch.int16).view(torch.bfloat16)


def f32_patterns() -> list:
    """The float32 bit patterns the conversion tests always include (both signs where a sign exists)."""
    p = [0x3f808000, 0x3f818000,                       # bf16 ties: kept bit even (-> 0x3f80), odd (-> 0x3f82)
         0x3f807fff, 0x3f817fff, 0x3f808001, 0x3f818001,  # one bit below / above those ties
         0x7f7fffff,                                   # the largest float32: bf16 inf, f16 65504
         0x477fe000, 0x477fefe6, 0x477ff000,           # 65504, 65519.9, 65520 (the first float32 that rounds to f16 inf)
         0x7f800000,                                   # inf
         0x33000000, 0x33400000, 0x33c00000,           # 2^-25 (f16 tie 0 | 2^-24 -> 0), 3 2^-26 (-> 2^-24), 3 2^-25 (tie -> 2^-23)
         0x00000000,                                   # 0
         0x00000001, 0x00008000, 0x00018000, 0x00400000, 0x007fffff,  # float32 denormals (two of them bf16 ties)
         0x00800000,                                   # the smallest normal
         0x38800000, 0x387fffff, 0x38000000,           # 2^-14 (smallest normal f16), the float32 below it, 2^-15 (f16 subnormal)
         0x7fc00000, 0x7f800001, 0x7fffffff, 0x7f808000]  # quiet NaN, signalling NaNs (the last one: payload in the bits bf16 drops)
    return p + [q | 0x80000000 for q in p]


def f32_pool(seed: int = 0) -> torch.Tensor:
    """f32_patterns() + 2 000 normals times 0.02 (weights) + 2 000 times 300 (beyond bf16's integers, inside f16)."""
    g = torch.Generator().manual_seed(seed)
    return torch.cat([from_bits(f32_patterns(), torch.float32), 0.02 * torch.randn(2000, generator=g),
                      300.0 * torch.randn(2000, generator=g)])


def bf16_pool() -> torch.Tensor:
    """All 65 536 bfloat16 patterns."""
    return (torch.arange(65536, dtype=torch.int32) - 32768).to(torch.int16).view(torch.bfloat16)


def tile_pool(pool: torch.Tensor, n: int) -> torch.Tensor:
    """n elements that walk the pool from a start that depends on n; the whole pool once n reaches its length."""
    return pool[(torch.arange(n) + (n % 7) * 3) % pool.numel()].contiguous()


# ---- FFN-up interleave ------------------------------------------------------------------------------------------------------
def interleave_rows(w: torch.Tensor, swap_blocks=None) -> torch.Tensor:
    """w [2H, K] = [gate rows 0..H-1 | up rows H..2H-1] -> rows in blocks of 32: [gate 32t..32t+31 | up 32t..32t+31] for t = 0,
    1, ...  swap_blocks (i, j): a plant, two 32-row blocks of the result exchanged."""
    H2, K = w.shape
    H = H2 // 2
    assert H2 == 2 * H and H % 32 == 0
    gate, up = w[:H].reshape(H // 32, 32, K), w[H:].reshape(H // 32, 32, K)
    blocks = torch.stack([gate, up], 1).reshape(2 * H // 32, 32, K).clone()
    if swap_blocks is not None:
        i, j = swap_blocks
        blocks[[i, j]] = blocks[[j, i]]
    return blocks.reshape(H2, K)


def interleave_ref(w: torch.Tensor, dst: torch.dtype, swap_blocks=None) -> torch.Tensor:
    return convert_ref(interleave_rows(w, swap_blocks), dst)


# ---- split weight -----------------------------------------------------------------------------------------------------------
def weight_scale_exponent(w: torch.Tensor) -> int:
    """k of split_weight: 2^k maps the largest finite-or-infinite |w| (NaNs ignored) into [2^14, 2^15).  The float32 exponent
    field of that maximum is clamped to 20 .. 250 first, so an all-zero (or all-denormal) matrix gets the k of 2^-107 and an
    infinite one the k of 2^123: 2^k and 2^-k are always normal float32 numbers."""
    a = w.float().abs().flatten()
    a = a[~torch.isnan(a)]
    amax = float(a.max()) if a.numel() else 0.0
    if math.isinf(amax):
        field = 255
    elif amax < 2.0 ** -126:
        field = 0
    else:
        field = math.frexp(amax)[1] - 1 + 127                                 # amax in [2^e, 2^(e+1)): field = e + 127
    e = min(max(field, 20), 250) - 127
    return 14 - e


def split_weight_ref(w: torch.Tensor, n_pad: int, interleave_h: int = 0, exchange: bool = False):
    """(w3 float16 [n_pad, 3K] = [lo | hi | hi] of a = w 2^k in float32, hi = half(a), lo = half(a - float(hi)), rows N .. n_pad-1
    zero; 2^-k as a float).  interleave_h = N / 2: rows permuted as interleave_rows.  exchange: a plant, hi and lo swapped."""
    N, K = w.shape
    w32 = w.float()
    k = weight_scale_exponent(w32)
    if interleave_h:
        assert N == 2 * interleave_h
        w32 = interleave_rows(w32)
    a = w32 * torch.tensor(2.0 ** k, dtype=torch.float32)
    hi = a.half()
    lo = (a - hi.float()).half()
    if exchange:
        hi, lo = lo, hi
    w3 = torch.zeros(n_pad, 3 * K, dtype=torch.float16)
    w3[:N] = torch.cat([lo, hi, hi], 1)
    return w3, 2.0 ** -k


# ---- row-norm maximum -------------------------------------------------------------------------------------------------------
def rownorm_max_ref(w: torch.Tensor, r0: int, rows: int) -> float:
    return float(w[r0:r0 + rows].double().pow(2).sum(-1).sqrt().max())


def rownorm_bar(ref: float, K: int) -> float:
    """(K / 64 + 8) 2^-24 |ref| + one float32 ulp of ref: a lane adds K / 64 squares one after the other, six butterfly levels and
    the squares' own roundings make up the 8; the square root rounds once (and halves the sum's relative error: not claimed)."""
    ulp = 2.0 ** (math.frexp(ref)[1] - 1 - 23) if ref > 0 else 2.0 ** -149
    return (K / 64 + 8) * F32_EPS * abs(ref) + ulp


# ---- embed ------------------------------------------------------------------------------------------------------------------
FORCED = ((C.SEQUENCE_BOS_TOKEN, C.STRUCTURE_BOS_TOKEN), (C.SEQUENCE_PAD_TOKEN, C.STRUCTURE_PAD_TOKEN),
          (C.SEQUENCE_EOS_TOKEN, C.STRUCTURE_EOS_TOKEN), (C.SEQUENCE_CHAINBREAK_TOKEN, C.STRUCTURE_CHAINBREAK_TOKEN))


def embed_ids(seq: torch.Tensor, xtok: torch.Tensor):
    """(s, t'): the table rows the input stage reads.  s = seq clamped into the 64-row sequence table; t' = xtok with -1 read
    as MASK, clamped into the 4101-row structure table, then BOS / PAD / EOS / chainbreak wherever s is the sequence track's."""
    s = seq.clamp(0, 63)
    t = torch.where(xtok == -1, torch.full_like(xtok, C.STRUCTURE_MASK_TOKEN), xtok).clamp(0, C.STRUCTURE_VOCAB - 1)
    for sid, tid in FORCED:
        t = torch.where(s == sid, torch.full_like(t, tid), t)
    return s, t


def embed_ref(seq, xtok, e_seq, e_struct, cvec, cond, cond_stride: int, cond_by_row_mod_b: bool = False) -> torch.Tensor:
    """((E_seq[s] + E_struct[t']) + c) + cond in float32, in that order -> [B, L, D].  cond: None, or a flat float32 buffer whose
    vector for sample b starts at b cond_stride (stride 0: one vector for all).  cond_by_row_mod_b: a plant, the vector of
    sample (row mod B) instead of (row div L)."""
    B, L = seq.shape
    D = cvec.numel()
    s, t = embed_ids(seq, xtok)
    v = (e_seq.float()[s] + e_struct.float()[t]) + cvec.float()
    if cond is not None:
        flat = cond.float().flatten()
        per_sample = torch.stack([flat[b * cond_stride:b * cond_stride + D] for b in range(B)])      # [B, D]
        row = torch.arange(B * L)
        which = (row % B) if cond_by_row_mod_b else (row // L)
        v = v + per_sample[which].view(B, L, D)
    return v


def gather_ref(tok: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    return table[tok.clamp(0, table.shape[0] - 1)]


# ---- sigma MLP --------------------------------------------------------------------------------------------------------------
SILU_SLOPE = 1.1                                                              # sup |silu'| = 1.0998
SILU_COEF = 6.0


def dot_coef(K: int) -> float:
    """The coefficient of one wave-per-output dot product of length K: K / 64 serial additions per lane, six butterfly levels,
    the bias, the product rounding: K / 64 + 8."""
    return K / 64 + 8


def sigma_mlp_ref(t_freq, w1, b1, w2, b2):
    """Float64 sigma MLP and its bars, all [n_sigma, D]: hidden = silu(W1 x + b1), cond = W2 hidden + b2.
      unit1 = 2^-24 (sum |w1 x| + |b1|): bar on the first pre-activation = dot_coef(F) unit1; silu passes at most 1.1 of it on and
              adds 6 x 2^-24 |silu| (expf, the add, the division): hidden_bar = 1.1 dot_coef(F) unit1 + 6 x 2^-24 |hidden|
      unit2 = 2^-24 (sum |w2 hidden| + |b2|): cond_bar = dot_coef(D) unit2 + |W2| hidden_bar."""
    x, w1, b1, w2, b2 = (t.double() for t in (t_freq, w1, b1, w2, b2))
    pre = x @ w1.T + b1
    hidden = pre * torch.sigmoid(pre)
    unit1 = F32_EPS * (x.abs() @ w1.abs().T + b1.abs())
    hidden_bar = SILU_SLOPE * dot_coef(w1.shape[1]) * unit1 + SILU_COEF * F32_EPS * hidden.abs()
    cond = hidden @ w2.T + b2
    unit2 = F32_EPS * (hidden.abs() @ w2.abs().T + b2.abs())
    cond_bar = dot_coef(w2.shape[1]) * unit2 + hidden_bar @ w2.abs().T
    return {"hidden": hidden, "hidden_bar": hidden_bar, "unit1": unit1, "cond": cond, "cond_bar": cond_bar, "unit2": unit2}


def second_layer_ref(hidden_got, w2, b2):
    """The second layer alone, from the hidden vector the kernel itself produced: (ref, unit2) float64; bar dot_coef(D) unit2."""
    h, w2, b2 = hidden_got.double(), w2.double(), b2.double()
    return h @ w2.T + b2, F32_EPS * (h.abs() @ w2.abs().T + b2.abs())


def bar_ratio(got, ref, bar) -> torch.Tensor:
    """|got - ref| / bar elementwise in float64 (0 where the error is 0); passes when finite and <= 1 everywhere."""
    err = (got.double() - ref.double()).abs()
    return torch.where(err == 0, torch.zeros_like(err), err / bar)


def passes(r: torch.Tensor) -> bool:
    return bool(torch.isfinite(r).all()) and float(r.max()) <= 1.0


# ---- 16-bit-input LayerNorm -------------------------------------------------------------------------------------------------
def ln16_case(M: int, D: int, dtype: torch.dtype, seed: int):
    """x16 [M, D] of `dtype` (N(0, 3) plus a row offset; the last row low-variance: 0.5 + 2^-8 {-1, 0, 1}, which both 16-bit
    types hold exactly — variance 1e-5, where eps = 1e-5 matters), w, b float32."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, D, generator=g) * 3 + torch.randn(M, 1, generator=g)
    x[M - 1] = 0.5 + 2.0 ** -8 * torch.randint(-1, 2, (D,), generator=g).float()
    return x.to(dtype), 1 + 0.3 * torch.randn(D, generator=g), 0.2 * torch.randn(D, generator=g)


def ln16_ratio(y16, x16, w, b) -> torch.Tensor:
    """rowwise_ref's LayerNorm bar on the exact 16-bit input: OUT_EPS |ref| + LN_COEF unit."""
    ref, unit = rr.add_ln_ref64(x16.float(), w, b)
    return rr.ratio(y16, ref, x16.dtype, rr.LN_COEF * unit)

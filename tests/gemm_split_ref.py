"""Pure torch helpers of tests/test_gpu_gemm_split_tiles.py and tests/test_gemm_split_cases_cpu.py: the split-f16 256x256 GEMM
(csrc/gemm256w4_split.hip) seen as what it is to the kernel, a plain f16 GEMM over one walk of K' = 3K columns with an f32
accumulator, out = rs[m] * w_inv * (A16 . W16^T).  Nothing here calls the library under test.

Exact operands.  A16 [M, 3K] and W16 [N, 3K] are independent integers in [-3, 3], dense and different in all three K segments (a
K-tile or K slice read from the wrong place changes the result; with real hi / lo / hi planes a wrong hi segment would not); rs is
a power of two per row, 2^-3 .. 2^3, w_inv a power of two.  Every product and partial sum is an integer of magnitude <= 9 * 3K
(110 592 at K = 4096) < 2^24 in any order or slicing, every scale is exact, so STORE, STORE + integer bias and RESID_DIV with a
power-of-two div and an integer x0 are exact and compared with torch.equal.

The bar of the fused SwiGLU (launcher code 4), mid = gt * rcp(1 + exp2(gt * -log2 e)) * up in float32, against ref = g sigmoid(g) u
in float64:

    bar = COEF(g) * 2^-24 * |ref| + 2^-24 * |u|,      COEF(g) = SWIGLU4_C0 + SWIGLU4_C1 * |g| * log2(e) * (1 - sigmoid(g))

C0 covers the roundings every element has (the scale products, exp2, the add, rcp, two products).  The C1 term is the derived cost
of rounding the argument g * -log2 e before exp2: an argument of magnitude |g| log2 e carries up to 2^-24 |g| log2 e of absolute
error (the product's rounding, and the float32 constant's own), exp2 turns it into that relative error of e^-g, and
d ln sigmoid / d ln e^-g = -(1 - sigmoid(g)): it matters only on the negative side, where swiglu_f32_kernel's expf(-g) has no such
term (SWIGLU_COEF = 16 of tests/rowwise_ref.py does not transfer).  The floor 2^-24 |u| covers exp2 overflowing to inf below
g ~ -88.7, where the kernel gives 0 for a true |silu(g)| < 2^-121.

Measured on the CPU with swiglu4_emulation (every step in float32) on the gate / up grids of swiglu_shapes(256), the way
SWIGLU_COEF was made (swiglu_needed: without the floor, gates in [-80, 0) for c1): c0 = the largest |err| / (2^-24 |ref|) over gates
> 0, c1 = the largest (|err| / (2^-24 |ref|) - c0) / (|g| log2 e (1 - sigmoid g)) over gates < 0; 4 x each, rounded up to a power of
two:

    c0 measured 2.76 (1.60, 2.47, 2.63, 2.76 on the four grids)  -> 4 x 2.76 = 11.0 -> SWIGLU4_C0 = 16
    c1 measured 0.83 (0.80, 0.81, 0.80, 0.83)                    -> 4 x 0.83 = 3.3  -> SWIGLU4_C1 = 4

What the measurement also showed: WITH the floor the second term never binds.  |g| log2 e (1 - sigmoid g) * |g sigmoid(g)| <= 0.64
for every g (its maximum, near |g| = 2.4), so the derived cost is at most 0.64 * 2^-24 |u| per unit of c1, below the floor the bar
already carries for the overflow; measured with the floor subtracted, the emulation needs c1 = 0.  The term is kept as derived (it is
what holds the emulation where the floor is left out: the CPU file asserts that the flat coefficient alone does not), and the bar is
no looser for it than 2^-24 (16 |ref| + 3.6 |u|).

tests/test_gemm_split_cases_cpu.py re-derives both figures; the GPU test prints what the device needed."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

BM = BN = 256                       # the tile of csrc/gemm256w4_common.h
GROUP_M = 8
F32_EPS = 2.0 ** -24
LOG2E = 1.4426950408889634
SWIGLU4_C0 = 16.0
SWIGLU4_C1 = 4.0
DIV_ENGINE = 1.1547005              # the engine's residue scaling factor, as test_gemm_split_k_and_its_reduce uses it


# ---- shapes -------------------------------------------------------------------------------------------------------------------
def grid_cap(cus: int) -> int:
    """persistent_grid(): one workgroup per CU, the CU count rounded down to a multiple of 8, at least 8."""
    return cus // 8 * 8 if cus >= 8 else 8


def grid(tiles: int, cus: int) -> int:
    return min(tiles, grid_cap(cus))


def tiles_n_for_rounds(tiles_m: int, rounds: int, cus: int) -> int:
    """The smallest tiles_n with tiles_m * tiles_n > rounds * grid: some workgroup then runs rounds + 1 tiles."""
    return rounds * grid_cap(cus) // tiles_m + 1


def tiles_n_ragged(tiles_m: int, rounds: int, cus: int) -> int:
    """The next tiles_n above tiles_n_for_rounds whose tile count is no multiple of 8 (rr != 0 in tile_origin)."""
    tn = tiles_n_for_rounds(tiles_m, rounds, cus) + 1
    while tiles_m * tn % 8 == 0:
        tn += 1
    return tn


def tile_origin(vt: int, tiles_m: int, tiles_n: int):
    """The raster of csrc/gemm256w4_tile.inc restated: virtual tile -> (tile row, tile column)."""
    n_tiles = tiles_m * tiles_n
    xcd, qq, rr = vt & 7, n_tiles >> 3, n_tiles & 7
    lin = (xcd * (qq + 1) if xcd < rr else rr * (qq + 1) + (xcd - rr) * qq) + (vt >> 3)
    per_group = GROUP_M * tiles_n
    grp, in_grp = divmod(lin, per_group)
    gsz = min(GROUP_M, tiles_m - grp * GROUP_M)
    return grp * GROUP_M + in_grp % gsz, in_grp // gsz


# ---- exact cases --------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    M: int
    N: int
    K: int
    A16: torch.Tensor               # f16 [M, 3K], integers in [-3, 3]
    W16: torch.Tensor               # f16 [N, 3K]
    rs: torch.Tensor                # f32 [M], powers of two 2^-3 .. 2^3
    bias: torch.Tensor              # f32 [N], integers in [-8, 8]
    w_inv: float
    seed: int

    def x0(self, device="cpu") -> torch.Tensor:
        """f32 [M, N] integers in [-8, 8] (its own stream: the operands do not depend on whether it was drawn)."""
        g = torch.Generator(device=device).manual_seed(self.seed + 1)
        return torch.randint(-8, 9, (self.M, self.N), generator=g, device=device).float()


def case_seed(M: int, N: int, K: int) -> int:
    return (1000003 * M + 1009 * N + K) % (2 ** 31 - 1)


def make_case(M: int, N: int, K: int, w_inv: float = 0.25, rs_row0: Optional[float] = None) -> Case:
    """Operands on the host (the CPU file checks the same tensors the GPU file runs)."""
    seed = case_seed(M, N, K)
    g = torch.Generator().manual_seed(seed)
    A16 = torch.randint(-3, 4, (M, 3 * K), generator=g).to(torch.float16)
    W16 = torch.randint(-3, 4, (N, 3 * K), generator=g).to(torch.float16)
    rs = 2.0 ** torch.randint(-3, 4, (M,), generator=g).float()
    if rs_row0 is not None:
        rs[0] = rs_row0
    bias = torch.randint(-8, 9, (N,), generator=g).float()
    return Case(M, N, K, A16, W16, rs, bias, w_inv, seed)


def exactness_margin(A16: torch.Tensor, W16: torch.Tensor) -> float:
    """(|A16| . |W16|^T).max(): below 2^24 every partial sum of the product is an exact float32 integer."""
    return float((A16.double().abs() @ W16.double().abs().t()).max())


def assert_exact_inputs(A16: torch.Tensor, W16: torch.Tensor) -> None:
    big = exactness_margin(A16, W16)
    assert big < 2 ** 24, f"inputs: (|A16| . |W16|^T).max() = {big} must stay below 2^24"


def as_f32_exact(x64: torch.Tensor, what: str) -> torch.Tensor:
    """A float64 reference that must be a float32 number as it stands (a condition on the inputs, not a tolerance)."""
    x32 = x64.float()
    assert bool((x32.double() == x64).all()), f"inputs: {what} is not exact in float32"
    return x32


# ---- the row layout launcher code 4 expects -----------------------------------------------------------------------------------
def interleave_swiglu(Wg: torch.Tensor, Wu: torch.Tensor) -> torch.Tensor:
    """gate [FH, K'], up [FH, K'] -> W [2 FH, K'] in blocks of 64 rows: [gate 32t .. 32t+31 | up 32t .. 32t+31]."""
    FH, K = Wg.shape
    assert Wu.shape == Wg.shape and FH % 32 == 0
    return torch.stack([Wg.view(FH // 32, 32, K), Wu.view(FH // 32, 32, K)], 1).reshape(2 * FH, K).contiguous()


def deinterleave_swiglu(W: torch.Tensor):
    """The inverse: W [2 FH, K'] -> (gate [FH, K'], up [FH, K'])."""
    N, K = W.shape
    assert N % 64 == 0
    b = W.view(N // 64, 2, 32, K)
    return b[:, 0].reshape(N // 2, K).contiguous(), b[:, 1].reshape(N // 2, K).contiguous()


def deinterleave_columns(P: torch.Tensor):
    """The product of an interleaved W, [M, 2 FH] -> (gate [M, FH], up [M, FH])."""
    M, N = P.shape
    b = P.view(M, N // 64, 2, 32)
    return b[:, :, 0].reshape(M, N // 2), b[:, :, 1].reshape(M, N // 2)


# ---- fused SwiGLU: cases, reference, bar, float32 emulation ---------------------------------------------------------------------
def make_swiglu_case(M: int, N: int, K: int) -> Case:
    """w_inv = 1 and rs[0] = 1: row 0's gates are the integer sums themselves (standard deviation 16 sqrt(3K) ~ 78 at K = 128), so
    that M = 1 already spans [-100, 100]; rows with rs = 2^-3 fill in the range where the sigmoid moves.  One gate weight row
    (logical gate row 5 = interleaved row 5) is zero, so that every row of A has a gate that is exactly 0."""
    c = make_case(M, N, K, w_inv=1.0, rs_row0=1.0)
    c.W16[5] = 0
    return c


def swiglu_ref64(g: torch.Tensor, u: torch.Tensor):
    """float64 gate, up -> (ref = g sigmoid(g) u, the t of COEF(g) = c0 + c1 t, floor = 2^-24 |u|)."""
    sig = torch.sigmoid(g)
    # 1 - sigmoid(g) = sigmoid(-g): no cancellation on the positive side
    return g * sig * u, g.abs() * LOG2E * torch.sigmoid(-g), F32_EPS * u.abs()


def swiglu_bar(ref, t, floor, c0=SWIGLU4_C0, c1=SWIGLU4_C1):
    return (c0 + c1 * t) * F32_EPS * ref.abs() + floor


def swiglu4_emulation(g32: torch.Tensor, u32: torch.Tensor) -> torch.Tensor:
    """The kernel's expression with every step in float32 (torch on the host: IEEE division for the hardware's rcp)."""
    assert g32.dtype == u32.dtype == torch.float32
    e = torch.exp2(g32 * torch.tensor(-1.4426950408889634, dtype=torch.float32))
    return g32 * (torch.tensor(1.0, dtype=torch.float32) / (1.0 + e)) * u32


SWIGLU4_MEASURE_G_MIN = -80.0       # below it 1 / (1 + e^-g) < 2^-115 nears float32's subnormals; the floor's domain anyway


def swiglu_needed(got: torch.Tensor, g: torch.Tensor, u: torch.Tensor):
    """-> (c0 needed, c1 needed), both WITHOUT the floor (it would hide the second): c0 = the largest |got - ref| / (2^-24 |ref|)
    over gates >= 0, c1 = the largest excess over that c0 per unit of t over gates in [SWIGLU4_MEASURE_G_MIN, 0)."""
    ref, t, _ = swiglu_ref64(g, u)
    live = ref != 0
    need = torch.where(live, (got.double() - ref).abs() / (F32_EPS * ref.abs()).clamp(min=1e-300), torch.zeros_like(ref))
    pos = live & (g > 0)
    c0 = float(need[pos].max()) if bool(pos.any()) else 0.0
    neg = live & (g < 0) & (g >= SWIGLU4_MEASURE_G_MIN)
    c1 = float(((need[neg] - c0).clamp(min=0) / t[neg]).max()) if bool(neg.any()) else 0.0
    return c0, c1


def swiglu_needed_total(got, g, u) -> float:
    """The largest (|got - ref| - floor) / (COEF(g) 2^-24 |ref|): <= 1 inside the bar."""
    ref, t, floor = swiglu_ref64(g, u)
    over = ((got.double() - ref).abs() - floor).clamp(min=0)
    return float(torch.where(over == 0, torch.zeros_like(over), over / ((SWIGLU4_C0 + SWIGLU4_C1 * t) * F32_EPS * ref.abs())).max())


def swiglu_gates_ups(c: Case):
    """float64 (gate, up) [M, N / 2] of a SwiGLU case whose W16 rows are interleaved."""
    P = (c.A16.double() @ c.W16.double().t()) * (c.rs.double()[:, None] * c.w_inv)
    return deinterleave_columns(P)


def assert_gate_span(g: torch.Tensor) -> None:
    assert float(g.min()) < -88.7 and float(g.max()) > 20 and bool((g == 0).any()), (float(g.min()), float(g.max()))
    assert float(g.min()) <= -100 and float(g.max()) >= 100, (float(g.min()), float(g.max()))


# ---- the cases of the GPU file (shapes that depend on the device come from its CU count) ---------------------------------------
SHORT_K = (128, 256, 384)                       # 6, 12, 18 K-tiles of the 3K walk: 1, 4, 7 steady iterations
SHORT_N = (256, 768)
SHORT_M = (1, 127, 128, 129, 255, 256, 257)     # the wave-row boundary at 128 and the tile boundary at 256
RASTER = ((4, 3), (9, 3), (3, 3))               # (tiles_m, tiles_n): < GROUP_M; a last group of one tile row; 9 tiles, rr = 1
KSLICE_SK = ((2, 256), (3, 384), (3, 512), (3, 640))      # (S, K): slices of 6, 6, 8, 10 K-tiles (kslice_tiles)
KSLICE_M = (1, 257, 300)
KSLICE_N = (256, 768)
HANDOFF_RAGGED_ROWS = 100                       # the last tile row of the hand-off cases holds 256 - 100 rows


def kslice_tiles(S: int, K: int) -> int:
    return 3 * K // S // 64


def handoff_shapes(cus: int):
    """(M, N, K, tag) of groups 3 and 4: 17 tile rows and just over one round of tiles, the same with a tile count that is no
    multiple of 8, 33 tile rows and just over two rounds, and that at K = 256."""
    m1, m2 = 17 * BM - HANDOFF_RAGGED_ROWS, 33 * BM - HANDOFF_RAGGED_ROWS
    return {
        "one_round": (m1, BN * tiles_n_for_rounds(17, 1, cus), 128),
        "one_round_rr": (m1, BN * tiles_n_ragged(17, 1, cus), 128),
        "two_rounds": (m2, BN * tiles_n_for_rounds(33, 2, cus), 128),
        "two_rounds_k256": (m2, BN * tiles_n_for_rounds(33, 2, cus), 256),
    }


def kslice_handoff_shape(cus: int):
    """(S, M, N, K): S = 4 slices of five tile rows, 20 virtual tile rows (groups of 8 straddle the slice boundaries at 5, 10, 15);
    16 tile columns (320 virtual tiles, what a 256-CU device needs), more on a larger device."""
    return 4, 5 * BM - HANDOFF_RAGGED_ROWS, BN * max(16, tiles_n_for_rounds(20, 1, cus)), 512


def swiglu_shapes(cus: int):
    m1, n1, k1 = handoff_shapes(cus)["one_round"]
    return [(1, 512, 128), (129, 512, 128), (257, 512, 128), (m1, n1, k1)]


def all_exact_shapes(cus: int):
    """Every (M, N, K) the GPU file runs with exact operands on a device of `cus` CUs."""
    out = [(M, N, K) for K in SHORT_K for N in SHORT_N for M in SHORT_M]
    out += [(tm * BM - 3, tn * BN, 128) for tm, tn in RASTER]
    out += list(handoff_shapes(cus).values())
    out += [(M, N, K) for _, K in KSLICE_SK for N in KSLICE_N for M in KSLICE_M]
    S, M, N, K = kslice_handoff_shape(cus)
    out.append((M, N, K))
    return out

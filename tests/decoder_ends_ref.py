"""What the ends of the structure decoder and the glue kernels of the structure encoder must compute, stated once, with the
inputs and the bars of tests/test_gpu_decoder_ends.py.  tests/test_decoder_ends_cpu.py shows on the CPU that these statements
agree with oracle/decoder_ref.py and oracle/encoder_ref.py, that the bars let a float32 evaluation through and that they stop
planted errors.

Every formula below is written from the oracle (never from the kernels) and takes the dtype it is evaluated in: float64 is
the reference; float32 is the plain torch evaluation of the same formula whose own error sets each bar.  Where the oracle
casts to float32 (`_pae_probs`) the float64 evaluation simply does not.

Bars have the shape of tests/rowwise_ref.py: |got - ref| <= COEF * unit.  The outputs are float32, so there is no output
rounding term; every unit is a magnitude the kernel works on:
    backbone   2^-24 (|trans| + 2) per residue (trans after scaling; the ideal atoms lie within 1.6 A of the origin)
    pLDDT      2^-24                TM rows, pTM   2^-24                PAE   2^-24 * 31.5
Each COEF is 4 x the needed_coef of the float32 evaluation over the very inputs of the GPU test, rounded up to a power of
two; the factor 4 pays for another summation order and, in the PAE / TM kernel, for the hardware exp.  The float32 figures
stand beside the constants; tests/test_decoder_ends_cpu.py re-measures them and holds them to COEF / 4.
"""
from __future__ import annotations

import math

import torch

from oracle.decoder_ref import BB_COORDINATES, MAX_PAE_BIN
from tests.rowwise_ref import F32_EPS, needed_coef, ratio  # noqa: F401  (re-exported for the two test files)

F32 = torch.float32
MASK_ID = 4096                       # ids >= 4096 are special tokens
BOS, EOS, PAD = 4098, 4097, 4099

# float32 evaluation on the CPU over the GPU test's inputs needs (tests/test_decoder_ends_cpu.py prints them):
BACKBONE_COEF = 8.0                  # 1.70 over BACKBONE_M x seeds (0, 1); the bond lengths under the same bar need 0.87
PLDDT_COEF = 16.0                    # 3.45 over BACKBONE_M x seeds (0, 1)
PAE_COEF = 32.0                      # 4.67 over PAE_CASES x PAE_SCALES
TM_COEF = 8.0                        # 1.08 for the TM rows over PAE_CASES x PAE_SCALES (pTM 0.66, the bin sweep's rows 0.40)
PAE_UNIT = F32_EPS * 31.5
SWEEP_PAE_ABS = 2 * 2.0 ** -19       # 2 ulp of 31.5 (the ulp of [16, 32) in float32 is 2^-19)


def pow2_bar(measured: float) -> float:
    """4 x measured, rounded up to a power of two: how a COEF above follows from its float32 figure."""
    return 2.0 ** math.ceil(math.log2(4 * measured))


# ---------------------------------------------------------------------------------------------------------------
# Dim6RotStructureHead's tail (oracle.decoder_ref.Dim6RotStructureHeadRef.forward after self.proj)
def backbone_formula(v: torch.Tensor, trans_scale: float, dtype, *, e1_sign: float = 1.0, e2_sign: float = 1.0) -> torch.Tensor:
    """v (M, >= 9): [trans 3 | x 3 | y 3 | ...] -> N, CA, C (M, 3, 3).  The oracle forms the frame from the points
    x + trans, trans, y + trans; their differences are -x and y, which is what is written here (in exact arithmetic the
    same thing, in float32 without the round trip through trans).  e1_sign / e2_sign = -1 plant that axis reversed."""
    v = v.to(dtype)
    trans = v[:, 0:3] * trans_scale
    ax = v[:, 3:6] / (v[:, 3:6].norm(dim=-1, keepdim=True) + 1e-5)
    ay = v[:, 6:9] / (v[:, 6:9].norm(dim=-1, keepdim=True) + 1e-5)
    e0 = -ax
    e0 = e0 / torch.sqrt((e0 ** 2).sum(-1, keepdim=True) + 1e-12)            # oracle.geom_ref.graham_schmidt
    e1 = ay - e0 * (e0 * ay).sum(-1, keepdim=True)
    e1 = e1 / torch.sqrt((e1 ** 2).sum(-1, keepdim=True) + 1e-12)
    e2 = e2_sign * torch.cross(e0, e1, dim=-1)
    rot = torch.stack([e0, e1_sign * e1, e2], dim=-1)                                  # columns e0, e1, e2
    bb = torch.tensor(BB_COORDINATES, dtype=dtype)
    return torch.einsum("mij,aj->mai", rot, bb) + trans[:, None, :]


def backbone_unit(v: torch.Tensor, trans_scale: float) -> torch.Tensor:
    """(M, 1, 1): 2^-24 (|trans| + 2)."""
    return (F32_EPS * ((v[:, 0:3].double() * trans_scale).norm(dim=-1) + 2.0))[:, None, None]


IDEAL_BONDS = tuple(float(torch.tensor(BB_COORDINATES[a], dtype=torch.float64).norm()) for a in (0, 2))   # 1.4592, 1.5251


def bond_lengths(bb: torch.Tensor) -> torch.Tensor:
    """(M, 3, 3) -> (M, 2) float64: |N - CA|, |C - CA|."""
    bb = bb.double()
    return torch.stack([(bb[:, 0] - bb[:, 1]).norm(dim=-1), (bb[:, 2] - bb[:, 1]).norm(dim=-1)], -1)


BACKBONE_M = (1, 255, 256, 257, 700)


def backbone_case(M: int, seed: int = 0) -> torch.Tensor:
    """(M, 23) float32: trans uniform in +-30 (before scaling), the rest standard normal."""
    g = torch.Generator().manual_seed(1000 * seed + M)
    v = torch.randn(M, 23, generator=g)
    v[:, :3] = (torch.rand(M, 3, generator=g) * 2 - 1) * 30
    return v


def backbone_degenerate_rows() -> torch.Tensor:
    """Rows whose frame is ill-conditioned: x = 0, y = 0, both 0, y parallel and antiparallel to x.  Finite output only."""
    g = torch.Generator().manual_seed(5)
    v = torch.randn(5, 23, generator=g)
    v[0, 3:6] = 0
    v[1, 6:9] = 0
    v[2, 3:9] = 0
    v[3, 6:9] = 2.5 * v[3, 3:6]
    v[4, 6:9] = -0.5 * v[4, 3:6]
    return v


# ---------------------------------------------------------------------------------------------------------------
# pLDDT (oracle.decoder_ref.StructureTokenDecoderRef.forward: CategoricalMixture(bins = n, start = 0, end = 1).mean())
def plddt_formula(logits: torch.Tensor, dtype, *, centre_offset: float = 0.5) -> torch.Tensor:
    logits = logits.to(dtype)
    n = logits.shape[-1]
    centres = (torch.arange(n, dtype=dtype) + centre_offset) / n
    return (logits.softmax(-1) * centres).sum(-1)


PLDDT_BINS = 50
PLDDT_SPECIAL = PLDDT_BINS + 4        # one-hot rows, then all-equal rows


def plddt_case(M: int, seed: int = 0) -> torch.Tensor:
    """(M, 50) float32: random logits, even rows x 1 and odd rows x 30; from M >= 54 the LAST 54 rows are one bin at +90
    and the rest at -90 (once per bin: the result is that bin's centre) and four all-equal rows (the result is 0.5)."""
    g = torch.Generator().manual_seed(2000 * seed + M)
    v = torch.randn(M, PLDDT_BINS, generator=g)
    v[1::2] *= 30
    if M >= PLDDT_SPECIAL:
        s = M - PLDDT_SPECIAL
        v[s:s + PLDDT_BINS] = -90.0
        v[s:s + PLDDT_BINS][torch.arange(PLDDT_BINS), torch.arange(PLDDT_BINS)] = 90.0
        for r, c in enumerate((0.0, 7.5, -90.0, 90.0)):
            v[s + PLDDT_BINS + r] = c
    return v


# ---------------------------------------------------------------------------------------------------------------
# PAE / pTM (oracle.decoder_ref.pae_bins, compute_predicted_aligned_error, compute_tm)
def pae_centres(dtype, max_bin: float = MAX_PAE_BIN, num_bins: int = 64, *, last_shift_steps: float = 0.0) -> torch.Tensor:
    """linspace(0, max_bin, num_bins - 1) + step / 2 and one more centre a step further (last_shift_steps plants an error
    of that many steps on the last one)."""
    step = max_bin / (num_bins - 2)
    c = torch.linspace(0, max_bin, num_bins - 1, dtype=dtype) + step / 2
    return torch.cat([c, (c[-1] + step + last_shift_steps * step)[None]])


def pae_tm_formula(logits: torch.Tensor, tokens: torch.Tensor, dtype, max_bin: float = MAX_PAE_BIN, *,
                   last_shift_steps: float = 0.0, clamp: bool = True, mean_over_L: bool = False, unmask=None):
    """logits (B, L, L, bins), tokens (B, L) -> (pae (B, L, L), tm_rows (B, L), ptm (B,)).  The keyword arguments plant the
    errors tests/test_decoder_ends_cpu.py wants the bars to stop; unmask = (b, i, j) leaves that masked pair unmasked."""
    B, L = tokens.shape
    aa = tokens < MASK_ID
    square = aa[:, :, None] & aa[:, None, :]
    keep = square.clone()
    if unmask is not None:
        keep[unmask] = True
    # a masked pair: every bin at the same (lowest) value -> uniform probabilities
    probs = logits.to(dtype).masked_fill(~keep[..., None], torch.finfo(dtype).min).softmax(-1)
    centres = pae_centres(dtype, max_bin, logits.shape[-1], last_shift_steps=last_shift_steps)
    pae = (probs * centres).sum(-1)
    n = aa.sum(-1, keepdim=True)
    d0 = 1.24 * ((n.clamp_min(19) if clamp else n) - 15).to(dtype) ** (1.0 / 3.0) - 1.8          # (B, 1)
    f_d = 1.0 / (1.0 + (centres[None] / d0) ** 2)                                                 # (B, bins)
    tm = (probs * f_d[:, None, None, :]).sum(-1)
    sq = square.to(dtype)
    den = torch.full_like(sq.sum(-1), float(L)) if mean_over_L else sq.sum(-1)
    tm_rows = (sq * tm).sum(-1) / (1e-10 + den)
    return pae, tm_rows, tm_rows.max(-1).values


def tokens_with_valid(L: int, n_valid: int, g: torch.Generator) -> torch.Tensor:
    """(L,) int64: BOS and EOS at the ends, one MASK at L // 2, n_valid structure ids at random inner positions, PAD on
    the rest.  L == 1: the one token is valid or BOS."""
    if L == 1:
        return torch.tensor([int(torch.randint(0, MASK_ID, (1,), generator=g)) if n_valid else BOS])
    tok = torch.full((L,), PAD, dtype=torch.int64)
    tok[0], tok[-1] = BOS, EOS
    inner = [p for p in range(1, L - 1) if not (L >= 4 and p == L // 2)]
    if L >= 4:
        tok[L // 2] = MASK_ID
    assert n_valid <= len(inner), (L, n_valid)
    order = torch.randperm(len(inner), generator=g)[:n_valid]
    for o in order.tolist():
        tok[inner[o]] = int(torch.randint(0, MASK_ID, (1,), generator=g))
    return tok


# (L, valid tokens per sample): 0, 1, 18, 19, 20 and more: both sides of the clamp of d0 at 19
PAE_CASES = ((1, (0, 1)), (10, (7, 0)), (15, (12, 1)), (16, (13, 1)), (17, (14, 0)), (33, (18, 19)), (33, (20, 30)),
             (258, (255,)))
PAE_SCALES = (1.0, 10.0)


def pae_case(L: int, counts, scale: float):
    """-> logits (nb, L, L, 64) float32 = randn * scale, tokens (nb, L)."""
    g = torch.Generator().manual_seed(L * 131 + sum(counts) * 7 + int(scale))
    tokens = torch.stack([tokens_with_valid(L, n, g) for n in counts])
    assert [int(v) for v in (tokens < MASK_ID).sum(-1)] == list(counts)
    return torch.randn(len(counts), L, L, 64, generator=g) * scale, tokens


SWEEP_L, SWEEP_NB = 17, 2


def pae_sweep_case():
    """Every token valid; pair (i, j) has logit 0 in bin (i L + j) % 64 and -200 elsewhere: the softmax is that bin alone
    (exp(-200) is 0 next to 1 in float32 and 1e-87 in float64)."""
    L, nb = SWEEP_L, SWEEP_NB
    bins = (torch.arange(L)[:, None] * L + torch.arange(L)[None]) % 64
    logits = torch.full((nb, L, L, 64), -200.0)
    logits.scatter_(-1, bins[None, :, :, None].expand(nb, L, L, 1), 0.0)
    g = torch.Generator().manual_seed(17)
    return logits, torch.randint(0, MASK_ID, (nb, L), generator=g), bins


# ---------------------------------------------------------------------------------------------------------------
# pair features (oracle.decoder_ref.PairwisePredictionHeadRef.forward): exact in one operation per element
PAIR_SHAPES = ((1, 1), (2, 7), (3, 16), (2, 33))


def pair_features_expected(qk: torch.Tensor) -> torch.Tensor:
    """qk (nb, L, 128) bfloat16 or float32 -> (nb, L, L, 128): feature (i, j) = [q_j * k_i | q_j - k_i], each the float32
    result of one multiply or subtract rounded once to qk's type: the only value a correct kernel can produce."""
    q, k = qk.float().chunk(2, dim=-1)
    prod = q[:, None, :, :] * k[:, :, None, :]
    diff = q[:, None, :, :] - k[:, :, None, :]
    return torch.cat([prod, diff], dim=-1).to(qk.dtype)


# ---------------------------------------------------------------------------------------------------------------
# kNN fixtures (the operation itself is oracle.encoder_ref.knn_edges)
KNN_L = (1, 9, 16, 17, 64, 257, 300)
KNN = 16
LATTICE_SCALE = 3.75      # the CA - CA distance of 3.8 A rounded to a binary fraction: see lattice_fold


def lattice_fold(L: int, w: int = 5, scale: float = LATTICE_SCALE) -> torch.Tensor:
    """(L, 3) float32: a self-avoiding walk on Z^3 folded into a w x w column, times `scale`.  Each layer is a boustrophedon
    over the w x w grid and every other layer runs backwards, so the walk is connected and a residue touches residues up to
    2 w^2 - 1 places away in sequence (49 for w = 5: beyond the relative-position clamp at 32, on both sides).
    With scale = 3.75 (= 15 / 4) every coordinate, difference, square and sum of squares is an integer multiple of 1 / 16
    below 2^24 / 16: exact in float32 whatever the order of operations or their fusion, so equal lattice distances are equal
    keys.  (3.8 is not a binary fraction: 3.8 n rounds differently for different n and equal lattice distances come out
    a few ulp apart; tests/test_decoder_ends_cpu.py shows float32 and float64 then order them differently.)"""
    cell = []
    for r in range(w):
        cols = range(w) if r % 2 == 0 else range(w - 1, -1, -1)
        cell += [(c, r) for c in cols]
    pts = []
    for n in range(L):
        k, m = divmod(n, w * w)
        x, y = cell[m if k % 2 == 0 else w * w - 1 - m]
        pts.append((x, y, k))
    return torch.tensor(pts, dtype=torch.float32) * scale


KNN_PATTERNS = ("known+none", "gaps+known", "wide")
KNN_BLOCK = 256          # a kernel thread's keys lie this far apart: a tie between residues j and j + 256 is a tie inside one thread


def knn_lattice_case(L: int, pattern: str, scale: float = LATTICE_SCALE):
    """-> ca (2, L, 3) float32 with zeros where unknown (as StructureEncoder.encode passes it), has (2, L) bool.
    "known+none": sample 0 all known (w = 5), sample 1 all unknown.  "gaps+known": sample 0 with a run of unknown residues
    from L // 3 on and an unknown last residue, sample 1 all known on a 4 x 4 column.  "wide": all known on 12 x 12 and
    13 x 13 columns, where layers are 144 / 169 residues and a residue touches residues up to 287 / 337 places away: at
    L = 300 residues j and j + 256 are equidistant neighbours of a third (tied_pairs_one_block_apart)."""
    ws = (12, 13) if pattern == "wide" else (5, 4)
    ca = torch.stack([lattice_fold(L, w, scale) for w in ws])
    has = torch.ones(2, L, dtype=torch.bool)
    if pattern == "known+none":
        has[1] = False
    elif pattern == "gaps+known":
        has[0, L // 3:L // 3 + max(1, L // 5)] = False
        has[0, L - 1] = False
    else:
        assert pattern == "wide", pattern
    return torch.where(has[..., None], ca, torch.zeros_like(ca)), has


def tied_pairs_one_block_apart(edges: torch.Tensor, keys: torch.Tensor):
    """edges (L, K) neighbours, keys (L, L) -> [(i, j)]: residues j and j + KNN_BLOCK both among i's neighbours with equal
    keys."""
    out = []
    for i, row in enumerate(edges.tolist()):
        s = set(row)
        out += [(i, j) for j in row if j + KNN_BLOCK in s and float(keys[i, j]) == float(keys[i, j + KNN_BLOCK])]
    return out


def knn_random_case(L: int = 300, seed: int = 3):
    """A random-walk chain with steps of 3.8 A +- 3 % (equal steps would tie residues i - 1 and i + 1 at every i), all
    known but a run in sample 1."""
    g = torch.Generator().manual_seed(seed)
    u = torch.randn(2, L, 3, generator=g)
    step = 3.8 * (1 + 0.03 * torch.randn(2, L, 1, generator=g))
    ca = torch.cumsum(step * u / u.norm(dim=-1, keepdim=True), 1)
    has = torch.ones(2, L, dtype=torch.bool)
    has[1, 40:60] = False
    return torch.where(has[..., None], ca, torch.zeros_like(ca)), has


def knn_keys64(ca: torch.Tensor, has: torch.Tensor) -> torch.Tensor:
    """The float64 sort keys of oracle.encoder_ref.knn_edges, (B, L, L): distance where both residues are known, sequence
    distance x 100 + 1e6 elsewhere."""
    L = ca.shape[1]
    ca = torch.where(has[..., None], ca.double(), torch.zeros_like(ca, dtype=torch.float64))
    both = has[:, :, None] & has[:, None, :]
    ar = torch.arange(L)
    seq = (ar[:, None] - ar[None, :]).abs().double() * 1e2 + 1e6
    return torch.where(both, (ca[:, :, None] - ca[:, None, :]).norm(dim=-1), seq[None])


KNN_NEAR_TIE = 2.0 ** -22


def knn_unexplained(got: torch.Tensor, ref: torch.Tensor, keys: torch.Tensor):
    """-> (share of positions where got != ref, number of those where the two candidates' float64 keys differ by
    KNN_NEAR_TIE relative or more: the differences no rounding explains)."""
    got, ref = got.long(), ref.long()
    kg, kr = keys.gather(-1, got), keys.gather(-1, ref)
    diff = got != ref
    far = diff & ((kg - kr).abs() >= KNN_NEAR_TIE * torch.maximum(kg, kr))
    return float(diff.double().mean()), int(far.sum())


def all_unknown_order(L: int, K: int) -> torch.Tensor:
    """(L, K): residue i's neighbours when nothing is known: i, then by sequence distance, the lower index first."""
    rows = []
    for i in range(L):
        cand = sorted(range(L), key=lambda j: (abs(i - j), j))
        rows.append(cand[:K])
    return torch.tensor(rows)


# ---------------------------------------------------------------------------------------------------------------
# neighbourhood (oracle.encoder_ref.StructureTokenEncoderRef.forward: the gathers after knn_edges)
def neighbourhood_expected(edges: torch.Tensor, table: torch.Tensor, rot, trans, has, bins: int):
    B = edges.shape[0]
    edges = edges.long()
    bi = torch.arange(B)[:, None, None]
    diff = (edges - edges[..., :1]).clamp(-bins, bins) + bins + 1
    return table[diff], rot[bi, edges], trans[bi, edges], has[bi, edges].to(torch.uint8)


# ---------------------------------------------------------------------------------------------------------------
# nearest code (oracle.encoder_ref.StructureTokenEncoderRef.forward: argmin of the squared distance, MASK without a frame)
CODE_N = (1, 255, 256, 300, 4096)
CODE_R = (1, 5, 70)
CODE_D = 128
CODE_NEAR_TIE = 2.0 ** -20


def code_d2(z: torch.Tensor, code: torch.Tensor, dtype) -> torch.Tensor:
    """(R, n_codes) squared distances, as a sum of squared differences."""
    z, code = z.to(dtype), code.to(dtype)
    return torch.stack([((zr[None] - code) ** 2).sum(-1) for zr in z])


def nearest_code_formula(z, code, has, dtype) -> torch.Tensor:
    return code_d2(z, code, dtype).argmin(-1).masked_fill(~has, MASK_ID)     # argmin: the first of equal minima


def duplicate_pairs(n_codes: int):
    """Index pairs (a < b) that will hold the same code row, on both sides of a multiple of 256, in one thread's stride
    (b - a a multiple of 256) and across threads in both orders of (a % 256, b % 256)."""
    cand = [(0, n_codes - 1), (3, 200), (201, 253), (255, 256), (4, 260), (250, 261), (100, 3940), (511, 512), (700, 1444),
            (2047, 4094)]
    pairs = [(a, b) for a, b in cand if a < b < n_codes]
    assert len({i for p in pairs for i in p}) == 2 * len(pairs)              # no index in two pairs
    return pairs


def code_integer_case(R: int, n_codes: int):
    """Integer z and codes in [-8, 8]: every squared distance is an integer below 2^15, exact in float32 in any order.
    Even rows sit exactly on a duplicated code row (distance 0 twice: the lower index must win), odd rows are free; every
    third row has no frame."""
    g = torch.Generator().manual_seed(R * 10007 + n_codes)
    code = torch.randint(-8, 9, (n_codes, CODE_D), generator=g).float()
    z = torch.randint(-8, 9, (R, CODE_D), generator=g).float()
    pairs = duplicate_pairs(n_codes)
    for a, b in pairs:
        code[b] = code[a]
    for r in range(0, R, 2):
        if pairs:
            z[r] = code[pairs[(r // 2) % len(pairs)][0]]
    has = torch.ones(R, dtype=torch.bool)
    has[2::3] = False
    return z, code, has, pairs


def code_random_case(R: int = 70, n_codes: int = 4096, seed: int = 9):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(R, CODE_D, generator=g), torch.randn(n_codes, CODE_D, generator=g), torch.ones(R, dtype=torch.bool)


def code_unexplained(got: torch.Tensor, z, code, has):
    """-> (share of rows where got differs from the float64 argmin, number of those where the float64 distance of got's code
    exceeds the best by CODE_NEAR_TIE of the best or more)."""
    d2 = code_d2(z, code, torch.float64)
    ref = d2.argmin(-1)
    best = d2.gather(-1, ref[:, None])[:, 0]
    mine = d2.gather(-1, got.long().clamp(max=code.shape[0] - 1)[:, None])[:, 0]
    diff = (got.long() != ref) & has
    far = diff & ((mine - best) >= CODE_NEAR_TIE * best)
    return float(diff.double().mean()), int(far.sum())

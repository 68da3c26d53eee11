"""The needed-rows and sub-batch bookkeeping kernels, each alone through its entry of include/esmdiff_hip_test.h, bit for bit
against tests/needed_rows_ref.py: mask_row_list_kernel, gather_rows16_kernel, copy_masked_logits_kernel, the mapped ddpm step,
move_token_rows_kernel, samples_with_mask_kernel, rows_identical_kernel (csrc/sampler.hip) and add_layernorm_rows_kernel
(csrc/norm.hip).  These decide which rows the last block and the head run on and which logits row the sampler then reads; the
end-to-end comparisons of tests/test_gpu_needed_rows.py reach their edges only by accident.

Every output buffer is filled with a sentinel and carries guard rows behind its end; whole buffers are compared, so what a kernel is
not documented to write must still hold the sentinel.  Float and 16-bit buffers are compared through integer views."""
import ctypes

import numpy as np
import pytest
import torch

from tests import needed_rows_ref as nr
from tests import rowwise_ref as rr

pytestmark = pytest.mark.gpu

MASK, V = nr.MASK, 4101
GUARD = 64
NAME = {torch.bfloat16: "bf16", torch.float16: "f16"}


def _unmasked(n, rng):
    return np.array(nr.UNMASKED_IDS, dtype=np.int64)[rng.integers(0, len(nr.UNMASKED_IDS), n)]


def _lib():
    from esmdiff_amd import _native as N
    return N.lib()


# ---------------------------------------------------------------------------------------------------------------
# mask_row_list_kernel: one workgroup of 1024 threads per part, a count pass and a prefix pass in tiles of 1024 rows
ROW_LIST_SHAPES = ((1, 1, 1), (1, 63, 1), (1, 64, 1), (1, 65, 1), (1, 1023, 1), (1, 1024, 1), (1, 1025, 1), (3, 700, 1),
                   (9, 258, 2), (7, 33, 3), (5, 130, 4), (4, 40, 4))


def _row_list_patterns(B, L, n_parts, rng):
    """(name, bool [B L]): where MASK sits.  The 7/8 patterns put every part at its own edge (exactly floor(7 rows / 8) masked rows,
    and one more); the single-mask patterns exist once per part that has such a row."""
    n = B * L
    parts = nr.part_rows(B, L, n_parts)
    yield "none", np.zeros(n, bool)
    yield "all", np.ones(n, bool)
    for extra in (0, 1):
        m = np.zeros(n, bool)
        for t0, rows in parts:
            m[t0 + rng.permutation(rows)[:7 * rows // 8 + extra]] = True
        yield f"seven_eighths+{extra}", m
    for pi, (t0, rows) in enumerate(parts):
        for name, r in (("first", 0), ("last", rows - 1), ("row1023", 1023), ("row1024", 1024)):
            if r < rows:
                m = np.zeros(n, bool)
                m[t0 + r] = True
                yield f"{name}_of_part{pi}", m
    m = np.zeros(n, bool)
    m[0::2] = True
    yield "every_second", m
    yield "random", rng.random(n) < 0.5
    m = np.zeros(n, bool)
    for t0, rows in parts:
        last = (rows - 1) // 1024 * 1024
        m[t0 + last:t0 + rows] = rng.random(rows - last) < 0.5
    yield "last_tile_only", m


@pytest.mark.parametrize("B,L,n_parts", ROW_LIST_SHAPES)
def test_mask_row_list(B, L, n_parts):
    """list, map and count of every part, and nothing else written: the 64-lane ballot edge (L 63 / 64 / 65), the 1024-row tile
    edge of the prefix (1023 / 1024 / 1025, masks at rows 1023 and 1024, masks in the last tile only, three tiles at (3, 700)),
    uneven B pi / np cuts (4 + 5, 2 + 2 + 3, 1 + 1 + 1 + 2), the count * 8 == rows * 7 edge of the compact rule on both sides, and
    unmasked ids that are MASK's neighbours or MASK in their low 32 bits."""
    from esmdiff_amd.engine import mask_row_list
    rng = np.random.default_rng(B * 10000 + L * 10 + n_parts)
    n = B * L
    seen = set()
    for name, m in _row_list_patterns(B, L, n_parts, rng):
        ids = _unmasked(n, rng)
        ids[m] = MASK
        before = (np.full(n + GUARD, -7, np.int32), np.full(n + GUARD, -9, np.int32), np.full(n_parts + GUARD, -11, np.int32))
        dev = [torch.from_numpy(a).cuda() for a in before]
        mask_row_list(torch.from_numpy(ids).view(B, L).cuda(), n_parts, *dev)
        msg = nr.check_row_list([t.cpu().numpy() for t in dev], ids, B, L, n_parts, before)
        assert not msg, (B, L, n_parts, name, msg)
        seen.add(name.split("_of_")[0])
    t0, rows = nr.part_rows(B, L, n_parts)[0]
    assert nr.compact(7 * rows // 8, rows) and not nr.compact(7 * rows // 8 + 1, rows)      # the two patterns straddle the rule
    assert ("row1024" in seen) == (max(r for _, r in nr.part_rows(B, L, n_parts)) > 1024)


def test_mask_row_list_refusals():
    """np > B, np = 0, L = 0, B = 0 and null pointers return ESMDIFF_E_INVALID and write nothing."""
    lib = _lib()
    x = torch.full((4, 8), MASK, dtype=torch.int64, device="cuda")
    lst, mp, cnt = (torch.full((40,), s, dtype=torch.int32, device="cuda") for s in (-7, -9, -11))
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for B, L, n_parts in ((4, 8, 5), (4, 8, 0), (4, 0, 1), (0, 8, 1), (4, 8, -1)):
        assert lib.esmdiff_mask_row_list(p(x), B, L, n_parts, p(lst), p(mp), p(cnt), None) == -1, (B, L, n_parts)
    for args in ((None, p(lst), p(mp), p(cnt)), (p(x), None, p(mp), p(cnt)), (p(x), p(lst), None, p(cnt)), (p(x), p(lst), p(mp), None)):
        assert lib.esmdiff_mask_row_list(args[0], 4, 8, 2, *args[1:], None) == -1
    torch.cuda.synchronize()
    assert bool((lst == -7).all()) and bool((mp == -9).all()) and bool((cnt == -11).all())


# ---------------------------------------------------------------------------------------------------------------
# gather_rows16_kernel: one wave per row, 16 bytes per lane and trip
@pytest.mark.parametrize("D", (8, 504, 512, 520, 1536, 2048))
def test_gather_rows16(D):
    """1, 63, 64, 65, 192 and 256 sixteen-byte chunks per row (the 64-lane trip edge), 1 .. 1027 rows (the 4-rows-per-workgroup
    edge), ascending, descending and repeating lists, random 16-bit patterns (NaNs of either type among them)."""
    from esmdiff_amd.engine import gather_rows16
    rng = np.random.default_rng(D)
    for n in (1, 3, 4, 5, 1027):
        S = 2 * n + 3
        src = rng.integers(-2 ** 15, 2 ** 15, (S, D), dtype=np.int16)
        asc = np.sort(rng.permutation(S)[:n]).astype(np.int32)
        lists = {"ascending": asc, "descending": asc[::-1].copy(), "repeats": rng.integers(0, min(S, 3), n).astype(np.int32)}
        dsrc = torch.from_numpy(src).cuda()
        for name, rows in lists.items():
            before = np.full((n + 2, D), 0x5a5a, dtype=np.int16)
            dst = torch.from_numpy(before).cuda()
            gather_rows16(dsrc.view(torch.bfloat16), torch.from_numpy(rows).cuda(), dst.view(torch.bfloat16))
            msg = nr.check_gather_rows(dst.cpu().numpy(), src, rows, before)
            assert not msg, (n, D, name, msg)
            assert np.array_equal(dsrc.cpu().numpy(), src)


def test_gather_rows16_refusals():
    lib = _lib()
    src = torch.zeros(4, 16, dtype=torch.int16, device="cuda")
    dst = torch.full((4, 16), 0x5a5a, dtype=torch.int16, device="cuda")
    rows = torch.zeros(4, dtype=torch.int32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for n, D in ((4, 12), (4, 0), (4, -8), (0, 16), (-1, 16)):
        assert lib.esmdiff_gather_rows16(p(src), p(rows), p(dst), n, D, None) == -1, (n, D)
    for args in ((None, p(rows), p(dst)), (p(src), None, p(dst)), (p(src), p(rows), None)):
        assert lib.esmdiff_gather_rows16(*args, 4, 16, None) == -1
    torch.cuda.synchronize()
    assert bool((dst == 0x5a5a).all())


# ---------------------------------------------------------------------------------------------------------------
# add_layernorm_rows_kernel<NV>: add_layernorm_kernel on compact rows gathered from the full-size residual stream
LN_WIDTHS = tuple(range(256, 2049, 256))
# the widths at which y equals add_layernorm_kernel's bit for bit (the product relies on it at 1536: a compact tail must give the
# logits of the plain one)
LN_BITWISE_WIDTHS = LN_WIDTHS
Y_SENTINEL = 0x7fc1          # a NaN in bf16, a NaN in f16


@pytest.mark.parametrize("D", LN_WIDTHS)
def test_add_layernorm_rows(D):
    """Both builds, every instantiation (NV = D / 256 = 1 .. 8), M compact rows gathered from a buffer of 2 M + 3:
    (a) x_out = (x[rows] + delta[rows]) + delta2 bit-equal to torch float32, (b) y within the LayerNorm bar of
    tests/rowwise_ref.py against float64, (c) y bit-equal to add_layernorm_kernel of the same build on the gathered inputs,
    (d) the full-size x and delta unchanged, and guard rows of x_out and y untouched.  Gains 1 + 0.3 randn kept at |w| >= 1 / 16
    (rr.ln_gains): with the raw draw of this seed, |w| = 0.0078 in one column at D = 1024 and 0.0036 at D = 1792, the f16 build's
    subnormal outputs of that column sat at 1.65 x and 4.59 x the bar on an MI355X (M = 1027, no bias) — in both LayerNorm kernels,
    bit for bit, and exactly where the float64 reference rounded to f16 sits: the format's spacing, not a kernel (EXPERIMENTS.md
    "Row bookkeeping", tests/test_rowwise_bars_cpu.py)."""
    from esmdiff_amd.engine import add_layernorm, add_layernorm_rows
    g = torch.Generator().manual_seed(D)
    w, b = rr.ln_gains(D, g).cuda(), (0.2 * torch.randn(D, generator=g)).cuda()
    worst, differ = {}, {}
    for M in (1, 3, 4, 5, 1027):
        F = 2 * M + 3
        lists = {"ascending": torch.randperm(F, generator=g)[:M].sort().values}
        if M == 5:
            lists["repeats"] = torch.tensor([6, 6, 2, 12, 2])
        for lname, rows in lists.items():
            x0 = (torch.randn(F, D, generator=g) * 3 + torch.randn(F, 1, generator=g)).cuda()
            d1, d2 = torch.randn(F, D, generator=g).cuda(), (0.5 * torch.randn(M, D, generator=g)).cuda()
            if M >= 3:                                    # one low-variance row: eps matters, rstd is large
                x0[rows[M - 1]] = 5 + 2e-3 * torch.randn(D, generator=g).cuda()
                d1[rows[M - 1]] *= 1e-3
                d2[M - 1] *= 1e-3
            rows_dev = rows.to(torch.int32).cuda()
            for dtype in (torch.bfloat16, torch.float16):
                for delta in (None, d1.to(dtype)):
                    for delta2 in (None, d2.to(dtype)):
                        v = x0[rows_dev.long()]
                        if delta is not None:
                            v = v + delta[rows_dev.long()].float()
                        if delta2 is not None:
                            v = v + delta2.float()
                        for bias in (b, None):
                            x = x0.clone()
                            dl = None if delta is None else delta.clone()
                            x_out = torch.full((M + 2, D), -12345.0, device="cuda")
                            y = torch.full((M + 2, D), Y_SENTINEL, dtype=torch.int16, device="cuda").view(dtype)
                            add_layernorm_rows(dtype, x, dl, rows_dev, delta2, x_out, w, bias, y)
                            case = (M, lname, NAME[dtype], delta is None, delta2 is None, bias is None)
                            assert torch.equal(x_out[:M].view(torch.int32), v.view(torch.int32)), case              # (a)
                            assert bool((x_out[M:] == -12345.0).all()), case
                            assert bool((y[M:].view(torch.int16) == Y_SENTINEL).all()), case
                            assert torch.equal(x, x0) and (dl is None or torch.equal(dl.view(torch.int16), delta.view(torch.int16))), case   # (d)
                            ref, unit = rr.add_ln_ref64(v, w, bias)
                            r = float(rr.ratio(y[:M], ref, dtype, rr.LN_COEF * unit).max())
                            wst = worst.setdefault(NAME[dtype], [0.0, 0.0])
                            wst[0], wst[1] = max(wst[0], r), max(wst[1], rr.needed_coef(y[:M], ref, dtype, unit))
                            assert r <= 1.0, (case, r)                                                               # (b)
                            plain = add_layernorm(dtype, x0[rows_dev.long()].contiguous(),
                                                  None if delta is None else delta[rows_dev.long()].contiguous(), delta2, True, w, bias)
                            ne = y[:M].view(torch.int16) != plain.view(torch.int16)
                            if bool(ne.any()):
                                dd = differ.setdefault(NAME[dtype], [0, 0.0, case])
                                dd[0] += int(ne.sum())
                                dd[1] = max(dd[1], float((y[:M].double() - plain.double()).abs().max()))
    print(f"MEASURED add_layernorm_rows D={D} " + " ".join(f"{k}: ratio {v[0]:.3f} coef {v[1]:.2f}" for k, v in worst.items()) +
          " | elements that differ from add_layernorm: " + (" ".join(f"{k}: {v[0]} (max |diff| {v[1]:.3g}, first at {v[2]})"
                                                                     for k, v in differ.items()) or "none"))
    if D in LN_BITWISE_WIDTHS:
        assert not differ, differ                                                                                    # (c)


def test_add_layernorm_rows_refusals():
    """(e) rows or x_out null, D = 128, 2304 and 0, M = 0, an unknown build and null x / w / y are refused with nothing written."""
    lib = _lib()
    x = torch.full((8, 256), 3.0, device="cuda")
    w = torch.ones(256, device="cuda")
    rows = torch.arange(4, dtype=torch.int32, device="cuda")
    x_out = torch.full((4, 256), -12345.0, device="cuda")
    y = torch.full((4, 256), 7.0, dtype=torch.bfloat16, device="cuda")
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())

    def call(dtype=0, x_=x, rows_=rows, x_out_=x_out, w_=w, y_=y, M=4, D=256):
        return lib.esmdiff_add_layernorm_rows(dtype, p(x_), None, p(rows_), None, p(x_out_), p(w_), None, p(y_), M, D, None)
    assert call(rows_=None) == -1 and call(x_out_=None) == -1
    assert call(x_=None) == -1 and call(w_=None) == -1 and call(y_=None) == -1
    for D in (128, 2304, 0, -256):
        assert call(D=D) == -1 and call(dtype=1, D=D) == -1, D
    assert call(M=0) == -1 and call(dtype=2) == -1
    torch.cuda.synchronize()
    assert bool((x_out == -12345.0).all()) and bool((y.float() == 7.0).all()) and bool((x == 3.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((x_out == 3.0).all())


# ---------------------------------------------------------------------------------------------------------------
# copy_masked_logits_kernel: one workgroup of 256 threads per row
@pytest.mark.parametrize("V_", (1, 255, 256, 257, 4101))
def test_copy_masked_logits(V_):
    """The 256-thread trip edge of the column loop, equal and different row strides, with and without a map.  x (7 samples of 6,
    cut 3 + 4): part 0 half masked, so its logits sit compact at the head of the part; part 1 all masked, mapped to itself.  Logits
    are random bits (NaN patterns included); unmasked rows of out, columns V .. ld_out - 1 of masked rows and the guard rows keep
    the sentinel."""
    from esmdiff_amd.engine import copy_masked_logits
    B, L, n_parts = 7, 6, 2
    rng = np.random.default_rng(V_)
    n = B * L
    ids = _unmasked(n, rng)
    t1 = nr.part_rows(B, L, n_parts)[1][0]
    ids[:t1][rng.permutation(t1)[:t1 // 2]] = MASK
    ids[t1:] = MASK
    _, row_map, count = nr.row_list_ref(ids, B, L, n_parts, sentinel=(-1, n, -1))     # unmasked rows point at a decoy row of zeros
    assert nr.compact(count[0], t1) and not nr.compact(count[1], n - t1)
    for ld, ld_out in ((4104, 4104), (4104, 4352)):
        logits = rng.integers(-2 ** 31, 2 ** 31, (n + 1, ld), dtype=np.int64).astype(np.int32)
        logits[n] = 0
        logits[:n, :4] = (0x7fc00000, 0x7f800001, -1, -(2 ** 31))                      # quiet NaN, signalling NaN, NaN, -0
        dl = torch.from_numpy(logits).cuda().view(torch.float32)
        dx = torch.from_numpy(ids).cuda()
        for mp in (None, row_map):
            before = np.full((n + 2, ld_out), 0x7fc12345, dtype=np.int32)
            out = torch.from_numpy(before).cuda()
            copy_masked_logits(dx, dl, None if mp is None else torch.from_numpy(mp).cuda(), out.view(torch.float32), V_)
            msg = nr.check_masked_copy(out.cpu().numpy(), ids, logits, mp, V_, before)
            assert not msg, (V_, ld, ld_out, mp is None, msg)


def test_copy_masked_logits_refusals():
    lib = _lib()
    x = torch.full((4,), MASK, dtype=torch.int64, device="cuda")
    lg = torch.zeros(4, 16, device="cuda")
    out = torch.full((4, 16), -5.0, device="cuda")
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    for args in ((None, lg, out), (x, None, out), (x, lg, None)):
        assert lib.esmdiff_copy_masked_logits(p(args[0]), p(args[1]), 16, None, p(args[2]), 16, 8, 4, None) == -1
    for ld, ld_out, V_, rows in ((7, 16, 8, 4), (16, 7, 8, 4), (16, 16, 0, 4), (16, 16, 8, 0)):
        assert lib.esmdiff_copy_masked_logits(p(x), p(lg), ld, None, p(out), ld_out, V_, rows, None) == -1
    torch.cuda.synchronize()
    assert bool((out == -5.0).all())


# ---------------------------------------------------------------------------------------------------------------
# ddpm_step_kernel<PER, false, false, MAPPED = true>: the logits of row r are row row_map[p(r)] of a buffer that holds the masked
# rows only
@pytest.fixture(scope="module")
def plain_step():
    """The plain esmdiff_ddpm_step, held bit-exact to the C oracle by tests/test_gpu_kernels.py: the expected ids."""
    from esmdiff_amd.config import TINY
    from esmdiff_amd.engine import Engine
    from esmdiff_amd.weights import random_init_state_dict
    eng = Engine(TINY, random_init_state_dict(TINY, seed=1), max_batch=2, max_len=16)
    yield eng.ddpm_step
    eng.close()


OFFSET = 2 ** 32 + 5          # a Philox sample index above 32 bits


def _mapped_buffer(full, ids, row_map, n_rows, expected, ld):
    """(buffer [n_rows, ld], the map with its unwritten entries pointed at a decoy row): the masked rows of `full` stored where the
    map says, every other row a decoy with one huge logit at a column that no expected id takes."""
    masked = np.flatnonzero(ids == MASK)
    taken = set(np.unique(expected).tolist()) | {MASK}
    decoy_col = next(c for c in range(4096) if c not in taken)
    buf = torch.zeros(n_rows, ld)
    buf[:, decoy_col] = 1e4
    real = row_map[masked]
    assert len(set(real.tolist())) == len(masked) and real.min() >= 0 and real.max() < n_rows
    buf[torch.from_numpy(real.astype(np.int64))] = full.reshape(-1, ld)[torch.from_numpy(masked)]
    decoy_rows = sorted(set(range(n_rows)) - set(real.tolist()))
    assert decoy_rows, "the case leaves no decoy row"
    mp = row_map.copy()
    mp[mp < 0] = decoy_rows[0]
    return buf.cuda(), torch.from_numpy(mp).cuda(), decoy_col


@pytest.mark.parametrize("B,L,n_parts", [(3, 258, 1), (9, 40, 2)])
def test_ddpm_step_mapped(plain_step, B, L, n_parts):
    """logits_period = 0: the update and the final pass, row strides 4104 and 4352, sample indices above 2^32.  (3, 258): every
    second row masked, one compact part.  (9, 40) cut 4 + 5: the first part half masked and compact, the second all masked and
    mapped to itself.  All B L rows of the buffer exist, so a wrong index reads a decoy row and draws the decoy column."""
    from esmdiff_amd.engine import ddpm_step_mapped
    rng = np.random.default_rng(B * L)
    g = torch.Generator().manual_seed(B * L)
    n = B * L
    ids = rng.integers(0, 4096, n).astype(np.int64)
    if n_parts == 1:
        ids[0::2] = MASK
    else:
        t1 = nr.part_rows(B, L, n_parts)[1][0]
        ids[:t1][rng.random(t1) < 0.5] = MASK
        ids[t1:] = MASK
    _, row_map, count = nr.row_list_ref(ids, B, L, n_parts)
    assert nr.compact(count[0], nr.part_rows(B, L, n_parts)[0][1])
    x0 = torch.from_numpy(ids).view(B, L).cuda()
    for ld in (4104, 4352):
        full = torch.randn(B, L, ld, generator=g) * 3
        for final in (False, True):
            mc = (0.0, 0.0) if final else (0.5, 0.05)        # nine in ten masked rows are drawn
            want = plain_step(x0.clone(), full.cuda(), *mc, final=final, seed=77, sample_offset=OFFSET, step=3).cpu()
            buf, mp, decoy_col = _mapped_buffer(full, ids, row_map, n, want.numpy(), ld)
            got = ddpm_step_mapped(x0.clone(), buf, V, *mc, final=final, seed=77, sample_offset=OFFSET, step=3, rows_map=mp).cpu()
            assert torch.equal(got, want), (B, L, ld, final, int((got != want).sum()), int((got == decoy_col).sum()))
            assert not bool((want == MASK).all()) and torch.equal(want.reshape(-1)[ids != MASK], torch.from_numpy(ids[ids != MASK]))


@pytest.mark.parametrize("B,Bf,n_parts", [(6, 2, 1), (6, 2, 2), (5, 2, 1), (5, 2, 2)])
def test_ddpm_step_mapped_shared_step0(plain_step, B, Bf, n_parts):
    """row_map together with logits_period = Bf, what a shared step 0 with a compact tail runs: every sample holds the same tokens,
    the forward ran on Bf samples, and sample b reads row_map[(b % Bf) L + l].  Expected: the plain step on the logits tiled b % Bf
    (B = 5: an uneven last period).  Also logits_period without a map."""
    from esmdiff_amd.engine import ddpm_step_mapped
    L = 33
    rng = np.random.default_rng(B * 10 + n_parts)
    g = torch.Generator().manual_seed(B * 10 + n_parts)
    row = rng.integers(0, 4096, L).astype(np.int64)
    row[rng.permutation(L)[:L // 2]] = MASK
    ids = np.tile(row, B)
    _, row_map, count = nr.row_list_ref(ids[:Bf * L], Bf, L, n_parts)
    assert all(nr.compact(c, r) for c, (_, r) in zip(count, nr.part_rows(Bf, L, n_parts)))
    x0 = torch.from_numpy(ids).view(B, L).cuda()
    for ld in (4104, 4352):
        full = torch.randn(Bf, L, ld, generator=g) * 3
        tiled = full[[b % Bf for b in range(B)]].contiguous()
        for final in (False, True):
            mc = (0.0, 0.0) if final else (0.5, 0.05)        # nine in ten masked rows are drawn
            want = plain_step(x0.clone(), tiled.cuda(), *mc, final=final, seed=9, sample_offset=OFFSET, step=0).cpu()
            buf, mp, decoy_col = _mapped_buffer(full, ids[:Bf * L], row_map, B * L, want.numpy(), ld)
            got = ddpm_step_mapped(x0.clone(), buf, V, *mc, final=final, seed=9, sample_offset=OFFSET, step=0, logits_period=Bf,
                                   rows_map=mp).cpu()
            assert torch.equal(got, want), (B, Bf, ld, final, int((got != want).sum()), int((got == decoy_col).sum()))
            if not final:                                # different noise per sample: the samples do not all draw the same ids
                assert not torch.equal(want[0], want[Bf])
            plain = torch.zeros(B * L, ld)
            plain[:, decoy_col] = 1e4
            plain[:Bf * L] = full.reshape(-1, ld)
            got = ddpm_step_mapped(x0.clone(), plain.cuda(), V, *mc, final=final, seed=9, sample_offset=OFFSET, step=0,
                                   logits_period=Bf).cpu()
            assert torch.equal(got, want), (B, Bf, ld, final, "no map")


def test_ddpm_step_mapped_refusals():
    lib = _lib()
    from esmdiff_amd import _native as N
    x = torch.full((2, 4), MASK, dtype=torch.int64, device="cuda")
    lg = torch.zeros(8, 4104, device="cuda")
    rng = N.Rng(1, 0)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())

    def call(x_=x, lg_=lg, ld=4104, V_=V, final=0, rng_=ctypes.byref(rng), B=2, L=4, period=0):
        return lib.esmdiff_ddpm_step_mapped(p(x_), p(lg_), ld, V_, 0.5, 0.46, final, rng_, 0, B, L, period, None, None)
    assert call(x_=None) == -1 and call(lg_=None) == -1 and call(rng_=None) == -1
    assert call(ld=4100) == -1 and call(V_=4096) == -1 and call(V_=5121, ld=5128) == -1
    assert call(B=0) == -1 and call(L=0) == -1 and call(period=-1) == -1
    torch.cuda.synchronize()
    assert bool((x == MASK).all())
    assert call(final=1, rng_=None) == 0              # the final pass draws nothing
    torch.cuda.synchronize()
    assert bool((x == 0).all())                       # all-zero logits: the lowest index wins


# ---------------------------------------------------------------------------------------------------------------
# move_token_rows_kernel
@pytest.mark.parametrize("gather", (1, 0))
def test_move_token_rows(gather):
    """Gather and scatter of n rows of L int64 (values above 2^32), one thread per element: L = 1, 7, 258, n = 1, 3, 24.  Every
    row of the destination that is not named keeps its sentinel, the guard rows too."""
    from esmdiff_amd.engine import move_token_rows
    rng = np.random.default_rng(gather)
    for n in (1, 3, 24):
        for L in (1, 7, 258):
            S = n + 4                                    # rows of the side that idx points into
            src = rng.integers(0, 2 ** 40, (S if gather else n, L), dtype=np.int64)
            idx = (rng.integers(0, S, n) if gather else rng.permutation(S)[:n]).astype(np.int32)
            before = np.full(((n if gather else S) + 2, L), -3, dtype=np.int64)
            dst = torch.from_numpy(before).cuda()
            move_token_rows(torch.from_numpy(src).cuda(), dst, torch.from_numpy(idx).cuda(), n, bool(gather))
            msg = nr.check_move_rows(dst.cpu().numpy(), src, idx, n, bool(gather), before)
            assert not msg, (gather, n, L, msg)


def test_move_token_rows_live_samples_only():
    """The final-skip sub-batch ran n_run = 24 samples of which n_live = 5 go back: a scatter of 5 rows leaves the other 19 rows
    of the caller's batch, and the guard rows, at their sentinel.  n = 0 moves nothing."""
    from esmdiff_amd.engine import move_token_rows
    rng = np.random.default_rng(5)
    n_run, n_live, L = 24, 5, 258
    src = rng.integers(0, 2 ** 40, (n_run, L), dtype=np.int64)
    idx = rng.permutation(n_run).astype(np.int32)
    before = np.full((n_run + 2, L), -3, dtype=np.int64)
    for n in (n_live, 0):
        dst = torch.from_numpy(before).cuda()
        move_token_rows(torch.from_numpy(src).cuda(), dst, torch.from_numpy(idx).cuda(), n, False)
        got = dst.cpu().numpy()
        msg = nr.check_move_rows(got, src, idx, n, False, before)
        assert not msg, (n, msg)
        assert int((got != -3).any(axis=1).sum()) == n
    lib = _lib()
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    s, i = torch.from_numpy(src).cuda(), torch.from_numpy(idx).cuda()
    dst = torch.from_numpy(before).cuda()
    for args in ((None, dst, i), (s, None, i), (s, dst, None)):
        assert lib.esmdiff_move_token_rows(p(args[0]), p(args[1]), p(args[2]), 3, L, 0, None) == -1
    for n, L_, ga in ((-1, L, 0), (3, 0, 0), (3, L, 2)):
        assert lib.esmdiff_move_token_rows(p(s), p(dst), p(i), n, L_, ga, None) == -1
    torch.cuda.synchronize()
    assert bool((dst == -3).all())


# ---------------------------------------------------------------------------------------------------------------
# samples_with_mask_kernel: one wave per sample
@pytest.mark.parametrize("L", (1, 63, 64, 65, 258))
def test_samples_with_mask(L):
    """A single MASK at position 0, at 64 (the second trip of the wave) and at L - 1 of one sample, and none at all with MASK's
    neighbours and MASK-in-32-bits present: has is 1 for that sample alone, and the guard entries keep the sentinel."""
    from esmdiff_amd.engine import samples_with_mask
    rng = np.random.default_rng(L)
    for B in (1, 5, 24):
        for pos in (0, 64, L - 1, None):
            if pos is not None and pos >= L:
                continue
            for b in sorted({0, B // 2, B - 1}):
                x = _unmasked(B * L, rng).reshape(B, L)
                x[:, 0], x[:, -1] = 4095, 4097
                if L > 2:
                    x[:, 1] = 4096 + 2 ** 32
                if pos is not None:
                    x[b, pos] = MASK
                before = np.full(B + GUARD, -5, dtype=np.int32)
                has = torch.from_numpy(before).cuda()
                samples_with_mask(torch.from_numpy(x).cuda(), has)
                msg = nr.check_any_mask(has.cpu().numpy(), x, before)
                assert not msg, (B, L, pos, b, msg)
    lib = _lib()
    x = torch.full((2, 4), MASK, dtype=torch.int64, device="cuda")
    has = torch.full((2,), -5, dtype=torch.int32, device="cuda")
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    for args in ((None, 2, 4, has), (x, 2, 4, None), (x, 0, 4, has), (x, 2, 0, has)):
        assert lib.esmdiff_samples_with_mask(p(args[0]), args[1], args[2], p(args[3]), None) == -1
    torch.cuda.synchronize()
    assert bool((has == -5).all())


# ---------------------------------------------------------------------------------------------------------------
# rows_identical_kernel
def test_rows_identical():
    """B = 1 and identical rows give non-zero; one differing element, in seq only at the last position of the last row, in x only
    at the first position of row 1, or in the upper 32 bits alone, gives 0.  The flag's neighbours are not written."""
    from esmdiff_amd.engine import rows_identical
    rng = np.random.default_rng(1)

    def run(seq, x):
        flag = torch.full((1 + GUARD,), 12345, dtype=torch.int32, device="cuda")
        rows_identical(torch.from_numpy(seq).cuda(), torch.from_numpy(x).cuda(), flag)
        f = flag.cpu().numpy()
        assert (f[1:] == 12345).all()
        msg = nr.check_rows_identical(f[0], seq, x)
        assert not msg, (seq.shape, msg)
        return int(f[0])

    for L in (1, 258):
        row_s, row_x = rng.integers(0, 32, (1, L)).astype(np.int64), _unmasked(L, rng)[None] + 2 ** 34
        assert run(row_s, row_x) != 0                                        # B = 1
        for B in (2, 24):
            seq, x = np.tile(row_s, (B, 1)), np.tile(row_x, (B, 1))
            assert run(seq, x) != 0
            s2 = seq.copy()
            s2[B - 1, L - 1] += 1
            assert run(s2, x) == 0
            x2 = x.copy()
            x2[1, 0] += 1
            assert run(seq, x2) == 0
            x2 = x.copy()
            x2[B - 1, L // 2] += 2 ** 32
            assert run(seq, x2) == 0
            s2 = seq.copy()
            s2[B // 2, 0] += 2 ** 32
            assert run(s2, x) == 0
    lib = _lib()
    a = torch.zeros(2, 4, dtype=torch.int64, device="cuda")
    flag = torch.full((1,), 12345, dtype=torch.int32, device="cuda")
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    for args in ((None, a, 2, 4, flag), (a, None, 2, 4, flag), (a, a, 2, 4, None), (a, a, 0, 4, flag), (a, a, 2, 0, flag)):
        assert lib.esmdiff_rows_identical(p(args[0]), p(args[1]), args[2], args[3], p(args[4]), None) == -1
    torch.cuda.synchronize()
    assert int(flag[0]) == 12345

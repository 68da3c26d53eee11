"""tests/needed_rows_ref.py against cases written out by hand, and its checkers against planted mutants: an index kernel that
restarts its prefix at a tile or a wave, applies the 7/8 rule with < instead of <=, numbers its list from the batch instead of
from the part, writes the map on unmasked rows, compares ids in 32 bits, or scatters its padding samples must not pass."""
import numpy as np
import pytest

from tests import needed_rows_ref as nr

M = nr.MASK
HI = 4096 + 2 ** 32          # MASK in its low 32 bits


def test_parts_are_cut_as_the_forward_cuts_them():
    assert nr.part_rows(7, 3, 3) == [(0, 6), (6, 6), (12, 9)]                  # 2 + 2 + 3 samples
    assert nr.part_rows(5, 2, 4) == [(0, 2), (2, 2), (4, 2), (6, 4)]           # 1 + 1 + 1 + 2
    assert nr.part_rows(9, 258, 2) == [(0, 4 * 258), (4 * 258, 5 * 258)]
    assert nr.part_rows(4, 40, 4) == [(0, 40), (40, 40), (80, 40), (120, 40)]
    assert nr.part_rows(1, 1025, 1) == [(0, 1025)]


def test_row_list_by_hand_7_3_3():
    x = [M, 0, M, 4095, 4097, M,                 # part 0: rows 0, 2, 5 of 6 -> compact
         M, M, M, M, M, M,                       # part 1: 6 of 6 -> plain
         4099, M, HI, M, M, 0, 0, 0, M]          # part 2: rows 1, 3, 4, 8 of 9 -> compact; HI is not MASK
    lst, mp, cnt = nr.row_list_ref(np.array(x, dtype=np.int64), 7, 3, 3)
    assert cnt.tolist() == [3, 6, 4]
    assert lst.tolist() == [0, 2, 5, -1, -1, -1,  0, 1, 2, 3, 4, 5,  1, 3, 4, 8, -1, -1, -1, -1, -1]
    assert mp.tolist() == [0, -1, 1, -1, -1, 2,  6, 7, 8, 9, 10, 11,  -1, 12, -1, 13, 14, -1, -1, -1, 15]
    assert all(a.dtype == np.int32 for a in (lst, mp, cnt))


def test_row_list_by_hand_5_4():
    x = np.array([[M, 0], [0, 0], [0, M], [M, M], [0, M]], dtype=np.int64)       # parts of 1, 1, 1 and 2 samples
    lst, mp, cnt = nr.row_list_ref(x, 5, 2, 4, sentinel=(-7, -9, -11))
    assert cnt.tolist() == [1, 0, 1, 3]
    assert lst.tolist() == [0, -7,  -7, -7,  1, -7,  0, 1, 3, -7]
    assert mp.tolist() == [0, -9,  -9, -9,  -9, 4,  6, 7, -9, 8]               # row 5 is entry 0 of part 2; 3 of 4 rows: 24 <= 28, compact


@pytest.mark.parametrize("rows,n,squeezed", [(64, 56, True), (64, 57, False), (63, 55, True), (63, 56, False)])
def test_seven_eighths_edge(rows, n, squeezed):
    """count * 8 <= rows * 7 with equality at 56 of 64 (448 = 448); 55 of 63 is 440 <= 441, 56 of 63 is 448 > 441."""
    assert nr.compact(n, rows) == squeezed
    x = np.zeros(rows, dtype=np.int64)
    x[rows - n:] = M                                                             # the LAST n rows, so that a compact map differs
    lst, mp, cnt = nr.row_list_ref(x, 1, rows, 1)
    assert cnt.tolist() == [n]
    assert lst[:n].tolist() == list(range(rows - n, rows)) and (lst[n:] == -1).all()
    assert (mp[:rows - n] == -1).all()
    assert mp[rows - n:].tolist() == (list(range(n)) if squeezed else list(range(rows - n, rows)))


def test_before_and_guards_are_kept():
    x = np.array([0, M, 0, M], dtype=np.int64)
    before = (np.full(7, -7, np.int32), np.full(6, -9, np.int32), np.full(3, -11, np.int32))
    lst, mp, cnt = nr.row_list_ref(x, 2, 2, 2, before=before)
    assert lst.tolist() == [1, -7, 1, -7, -7, -7, -7] and mp.tolist() == [-9, 0, -9, 2, -9, -9] and cnt.tolist() == [1, 1, -11]
    assert before[0].tolist() == [-7] * 7                                        # the caller's arrays are not written


# ---- mutants of the row list ----
def mutant_row_list(x, B, L, n_parts, kind, before):
    """mask_row_list_kernel's structure — tiles of 1024 rows, waves of 64 — with one planted defect."""
    ids = [int(v) for v in np.asarray(x).reshape(-1)]
    lst, mp, cnt = (np.array(a, copy=True) for a in before)
    is_mask = (lambda v: (v & 0xffffffff) == M) if kind == "id32" else (lambda v: v == M)
    for pi, (t0, rows) in enumerate(nr.part_rows(B, L, n_parts)):
        count = sum(is_mask(ids[t0 + r]) for r in range(rows))
        cnt[pi] = count
        squeeze = count * 8 < rows * 7 if kind == "strict_less" else count * 8 <= rows * 7
        i = 0
        for r in range(rows):
            if (kind == "tile_restart" and r % 1024 == 0) or (kind == "wave_restart" and r % 64 == 0):
                i = 0
            if is_mask(ids[t0 + r]):
                lst[t0 + i] = r + (t0 if kind == "batch_relative" else 0)
                mp[t0 + r] = t0 + (i if squeeze else r)
                i += 1
            elif kind == "map_unmasked":
                mp[t0 + r] = t0 + r
    return lst, mp, cnt


def _case(B, L, n_parts, fill):
    x = np.zeros(B * L, dtype=np.int64)
    fill(x)
    before = (np.full(B * L + 8, -7, np.int32), np.full(B * L + 8, -9, np.int32), np.full(n_parts + 4, -11, np.int32))
    return x, B, L, n_parts, before


def _set(sl, v=M):
    def fill(x):
        x[sl] = v
    return fill


MUTANT_CASES = {
    # kind: the smallest case that shows it
    "tile_restart": _case(1, 1025, 1, _set(slice(1023, 1025))),                  # rows 1023 and 1024: the second is entry 1, not 0
    "wave_restart": _case(1, 65, 1, _set(slice(63, 65))),
    "strict_less": _case(1, 64, 1, _set(slice(8, 64))),                          # 56 of 64: compact by <=, plain by <
    "batch_relative": _case(7, 3, 3, _set(slice(7, 9))),                         # masks in part 1 only
    "map_unmasked": _case(2, 4, 1, _set(slice(1, 2))),
    "id32": _case(1, 5, 1, _set(slice(2, 3), HI)),
}


@pytest.mark.parametrize("kind", sorted(MUTANT_CASES))
def test_row_list_checker_rejects(kind):
    x, B, L, n_parts, before = MUTANT_CASES[kind]
    good = nr.row_list_ref(x, B, L, n_parts, before=before)
    assert nr.check_row_list(good, x, B, L, n_parts, before) == ""
    msg = nr.check_row_list(mutant_row_list(x, B, L, n_parts, kind, before), x, B, L, n_parts, before)
    assert msg, kind
    # without its defect the same code is the reference
    assert nr.check_row_list(mutant_row_list(x, B, L, n_parts, None, before), x, B, L, n_parts, before) == ""


def test_row_list_checker_names_the_element():
    x, B, L, n_parts, before = MUTANT_CASES["tile_restart"]
    msg = nr.check_row_list(mutant_row_list(x, B, L, n_parts, "tile_restart", before), x, B, L, n_parts, before)
    assert msg.startswith("list[0] (part 0, offset 0 of 1025 rows, 2 masked): got 1024, expected 1023"), msg
    x, B, L, n_parts, before = MUTANT_CASES["strict_less"]
    msg = nr.check_row_list(mutant_row_list(x, B, L, n_parts, "strict_less", before), x, B, L, n_parts, before)
    assert msg.startswith("map[8] (part 0, offset 8 of 64 rows, 56 masked): got 8, expected 0"), msg
    good = list(nr.row_list_ref(x, B, L, n_parts, before=before))
    good[0][70] = 3                                                               # a write behind the end
    assert "guard" in nr.check_row_list(good, x, B, L, n_parts, before)
    good[2][0] += 1
    assert nr.check_row_list(good, x, B, L, n_parts, before).startswith("count[0]")


def test_mutants_pass_where_their_defect_does_not_show():
    """Why the GPU cases single the edges out: on a half-masked part of 40 rows every mutant but two is right."""
    x, B, L, n_parts, before = _case(4, 40, 4, _set(slice(0, None, 2)))
    for kind in ("tile_restart", "wave_restart", "strict_less", "id32"):
        assert nr.check_row_list(mutant_row_list(x, B, L, n_parts, kind, before), x, B, L, n_parts, before) == "", kind


# ---- the other references and checkers ----
def test_gather_and_checker():
    src = np.arange(5 * 8, dtype=np.int16).reshape(5, 8)
    before = np.full((4, 8), 0x5a5a, dtype=np.int16)
    rows = [3, 0, 3]
    want = nr.gather_rows_ref(src, rows, before)
    assert want.tolist() == [src[3].tolist(), src[0].tolist(), src[3].tolist(), [0x5a5a] * 8]
    assert nr.check_gather_rows(want, src, rows, before) == ""
    bad = want.copy()
    bad[1] = src[1]                                                               # row i instead of rows[i]
    assert nr.check_gather_rows(bad, src, rows, before).startswith("dst[1, 0] (source row 0): got 8, expected 0")
    bad = want.copy()
    bad[3, 7] = 0
    assert "guard" in nr.check_gather_rows(bad, src, rows, before)


def test_move_rows_and_scatter_of_padding():
    """The final-skip sub-batch: n_run = 4 samples ran, n_live = 2 of them go back; a scatter of all 4 overwrites two complete
    samples of the caller's batch."""
    src = (np.arange(4 * 3, dtype=np.int64).reshape(4, 3) + 2 ** 33)
    idx = np.array([5, 2, 0, 1], dtype=np.int32)
    before = np.full((7, 3), -3, dtype=np.int64)
    want = nr.move_rows_ref(src, idx, 2, False, before)
    assert want[5].tolist() == src[0].tolist() and want[2].tolist() == src[1].tolist()
    assert (np.delete(want, [5, 2], axis=0) == -3).all()
    assert nr.check_move_rows(want, src, idx, 2, False, before) == ""
    padded = nr.move_rows_ref(src, idx, 4, False, before)                         # the mutant: the padding samples move too
    assert nr.check_move_rows(padded, src, idx, 2, False, before).startswith("dst[0, 0]: got 8589934598, expected -3")
    g = nr.move_rows_ref(want, idx, 2, True, np.full((3, 3), -3, dtype=np.int64))
    assert g.tolist() == [src[0].tolist(), src[1].tolist(), [-3] * 3]
    low = want.astype(np.int32).astype(np.int64)                                  # rows moved through 32 bits
    assert nr.check_move_rows(low, src, idx, 2, False, before)
    assert nr.move_rows_ref(src, idx, 0, False, before).tolist() == before.tolist()


def test_any_mask_and_checker():
    x = np.array([[0, 4095, 4097], [HI, 0, 0], [0, 0, M]], dtype=np.int64)
    before = np.full(5, -5, dtype=np.int32)
    want = nr.any_mask_ref(x, before)
    assert want.tolist() == [0, 0, 1, -5, -5]
    assert nr.check_any_mask(want, x, before) == ""
    in32 = want.copy()
    in32[1] = 1                                                                   # an id compared in 32 bits
    assert nr.check_any_mask(in32, x, before).startswith("has[1]: got 1, expected 0")
    last_missed = want.copy()
    last_missed[2] = 0
    assert nr.check_any_mask(last_missed, x, before)


def test_rows_identical_and_checker():
    seq = np.tile(np.array([[0, 5, 2]], dtype=np.int64), (3, 1))
    x = np.tile(np.array([[M, 7, HI]], dtype=np.int64), (3, 1))
    assert nr.rows_identical_ref(seq, x) and nr.rows_identical_ref(seq[:1], x[:1])
    assert nr.check_rows_identical(-1, seq, x) == "" and nr.check_rows_identical(0, seq, x)
    for arr, at, v in ((seq, (2, 2), 3), (x, (1, 0), 0), (x, (2, 2), M)):         # the last: equal in the low 32 bits
        a = arr.copy()
        a[at] = v
        s2, x2 = (a, x) if arr is seq else (seq, a)
        assert not nr.rows_identical_ref(s2, x2)
        assert nr.check_rows_identical(0, s2, x2) == ""
        assert nr.check_rows_identical(-1, s2, x2) == "flag -1, expected 0"       # what a 32-bit compare answers for the last


def test_masked_copy_and_checker():
    x = np.array([M, 0, M, HI], dtype=np.int64)
    logits = np.arange(4 * 6, dtype=np.int32).reshape(4, 6)
    before = np.full((5, 8), -2, dtype=np.int32)
    row_map = np.array([0, -9, 1, -9], dtype=np.int32)
    want = nr.masked_copy_ref(x, logits, row_map, 5, before)
    assert want[0].tolist() == [0, 1, 2, 3, 4, -2, -2, -2] and want[2].tolist() == [6, 7, 8, 9, 10, -2, -2, -2]
    assert (want[[1, 3, 4]] == -2).all()
    assert nr.masked_copy_ref(x, logits, None, 5, before)[2, :5].tolist() == [12, 13, 14, 15, 16]
    assert nr.check_masked_copy(want, x, logits, row_map, 5, before) == ""
    pad = want.copy()
    pad[0, 5] = 5                                                                 # a copy of ld columns instead of V
    assert nr.check_masked_copy(pad, x, logits, row_map, 5, before).startswith("out[0, 5] (masked row, padding column)")
    unmapped = nr.masked_copy_ref(x, logits, None, 5, before)
    assert nr.check_masked_copy(unmapped, x, logits, row_map, 5, before).startswith("out[2, 0] (masked row, column below V)")
    in32 = want.copy()
    in32[3, :5] = logits[0, :5]                                                   # row 3 taken for MASK
    assert nr.check_masked_copy(in32, x, logits, row_map, 5, before).startswith("out[3, 0] (unmasked row")

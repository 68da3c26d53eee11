"""Plain statements of the needed-rows and sub-batch bookkeeping kernels (csrc/sampler.hip: mask_row_list, gather_rows16,
copy_masked_logits, move_token_rows, samples_with_mask, rows_identical), written as loops over rows in Python integers, and a
checker for each that names the first wrong element.  tests/test_gpu_row_bookkeeping.py holds the kernels to them bit for bit;
tests/test_needed_rows_ref_cpu.py holds them to hand-written cases and shows that the checkers reject planted mutants.

Every reference starts from a copy of the output buffer as it was before the call (`before`: sentinels, guard rows included) and
writes only what the kernel is documented to write, so that comparing whole buffers also checks what must be left alone.
Arrays are numpy; 16-bit and float data come in as integer views (bits are compared, NaN patterns included).
"""
from __future__ import annotations

import numpy as np

MASK = 4096
# ids an unmasked row may hold: both neighbours of MASK, the pad id, and a value equal to MASK in its low 32 bits
UNMASKED_IDS = (0, 4095, 4097, 4099, 4096 + 2 ** 32)


def part_rows(B: int, L: int, n_parts: int):
    """[(t0, rows)] of the n_parts sub-batches: part pi holds samples [B pi // n_parts, B (pi + 1) // n_parts)."""
    assert 1 <= n_parts <= B and L >= 1
    out = []
    for pi in range(n_parts):
        t0 = (B * pi // n_parts) * L
        out.append((t0, (B * (pi + 1) // n_parts) * L - t0))
    return out


def compact(count: int, rows: int) -> bool:
    """The rule host and device apply to the same count: a part runs compacted when at most 7/8 of its rows hold MASK."""
    return count * 8 <= rows * 7


def row_list_ref(x, B: int, L: int, n_parts: int, before=None, sentinel=(-1, -1, -1)):
    """(list, map, count) of mask_row_list_kernel for x (B L ids, any shape).  before: (list, map, count) as they were (copied),
    else fresh arrays of B L / B L / n_parts entries filled with `sentinel`."""
    ids = [int(v) for v in np.asarray(x).reshape(-1)]
    assert len(ids) == B * L
    if before is None:
        lst, mp, cnt = (np.full(n, s, dtype=np.int32) for n, s in zip((B * L, B * L, n_parts), sentinel))
    else:
        lst, mp, cnt = (np.array(a, dtype=np.int32, copy=True) for a in before)
    for pi, (t0, rows) in enumerate(part_rows(B, L, n_parts)):
        masked = []
        for r in range(rows):
            if ids[t0 + r] == MASK:
                masked.append(r)
        cnt[pi] = len(masked)
        squeeze = compact(len(masked), rows)
        for i, r in enumerate(masked):
            lst[t0 + i] = r
            mp[t0 + r] = t0 + (i if squeeze else r)
    return lst, mp, cnt


def gather_rows_ref(src, rows, before):
    """dst [i, :] = src [rows[i], :] for every i; the other rows of `before` stay."""
    dst = np.array(before, copy=True)
    for i, r in enumerate(rows):
        dst[i, :] = src[int(r), :]
    return dst


def move_rows_ref(src, idx, n: int, gather: bool, before):
    """n rows: dst [i] = src [idx[i]] (gather) or dst [idx[i]] = src [i] (scatter); the other rows of `before` stay."""
    dst = np.array(before, copy=True)
    for i in range(n):
        if gather:
            dst[i, :] = src[int(idx[i]), :]
        else:
            dst[int(idx[i]), :] = src[i, :]
    return dst


def any_mask_ref(x, before):
    """has [b] = 1 if row b of x [B, L] holds MASK, else 0; the entries of `before` past B stay."""
    has = np.array(before, copy=True)
    for b in range(x.shape[0]):
        has[b] = 0
        for v in x[b]:
            if int(v) == MASK:
                has[b] = 1
    return has


def rows_identical_ref(seq, x) -> bool:
    """Every row of seq and of x equals row 0 of the same array, as 64-bit integers."""
    for b in range(1, x.shape[0]):
        for l in range(x.shape[1]):
            if int(seq[b, l]) != int(seq[0, l]) or int(x[b, l]) != int(x[0, l]):
                return False
    return True


def masked_copy_ref(x, logits, row_map, V: int, before):
    """out [row, :V] = logits [row_map[row] (or row), :V] on the rows of x (flat) that hold MASK; the rest of `before` stays."""
    out = np.array(before, copy=True)
    for row, v in enumerate(np.asarray(x).reshape(-1)):
        if int(v) == MASK:
            out[row, :V] = logits[int(row_map[row]) if row_map is not None else row, :V]
    return out


# ---- checkers: "" when got is right, else what is wrong at the first wrong element ----
def first_difference(got, want, what: str, describe=None) -> str:
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return f"{what}: shape {got.shape}, expected {want.shape}"
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    if bad.size == 0:
        return ""
    at = tuple(int(i) for i in np.unravel_index(int(bad[0]), want.shape))
    where = describe(at) if describe else ""
    return f"{what}{list(at)}{where}: got {got[at].item()!r}, expected {want[at].item()!r} ({bad.size} wrong elements)"


def check_row_list(got, x, B: int, L: int, n_parts: int, before) -> str:
    """got / before: (list, map, count) after / before the call, guard entries included."""
    want = row_list_ref(x, B, L, n_parts, before=before)
    parts = part_rows(B, L, n_parts)

    def describe(at):
        for pi, (t0, rows) in enumerate(parts):
            if t0 <= at[0] < t0 + rows:
                return f" (part {pi}, offset {at[0] - t0} of {rows} rows, {int(want[2][pi])} masked)"
        return " (guard)"
    for name, g, w in zip(("count", "list", "map"), (got[2], got[0], got[1]), (want[2], want[0], want[1])):
        msg = first_difference(g, w, name, None if name == "count" else describe)
        if msg:
            return msg
    return ""


def check_gather_rows(got, src, rows, before) -> str:
    return first_difference(got, gather_rows_ref(src, rows, before), "dst", lambda at: f" (source row {int(rows[at[0]])})" if at[0] < len(rows) else " (guard)")


def check_move_rows(got, src, idx, n: int, gather: bool, before) -> str:
    return first_difference(got, move_rows_ref(src, idx, n, gather, before), "dst")


def check_any_mask(got, x, before) -> str:
    return first_difference(got, any_mask_ref(x, before), "has")


def check_rows_identical(flag: int, seq, x) -> str:
    want = rows_identical_ref(seq, x)
    return "" if (int(flag) != 0) == want else f"flag {int(flag)}, expected {'non-zero' if want else '0'}"


def check_masked_copy(got, x, logits, row_map, V: int, before) -> str:
    ids = np.asarray(x).reshape(-1)

    def describe(at):
        if at[0] >= ids.size:
            return " (guard)"
        return f" ({'masked' if int(ids[at[0]]) == MASK else 'unmasked'} row, {'column below V' if at[1] < V else 'padding column'})"
    return first_difference(got, masked_copy_ref(x, logits, row_map, V, before), "out", describe)

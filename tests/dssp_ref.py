"""TEST INFRASTRUCTURE — NumPy float64 restatements of the secondary-structure assignment of esmdiff_amd/csrc/dssp.hip (Kabsch &
Sander 1983), and the NeRF builder of the synthetic chains.  Integer outputs and energies; the device is held to
them exactly.

  X (n, L, 4, 3)   N, CA, C, O;  mask (n, L) or None;  no_donor (L,) or None (proline: its N carries no H)
  a distance       sqrt((dx dx + dy dy) + dz dz), each operation rounded once (no FMA), numpy's correctly rounded sqrt and division
  present[i]       mask[i] and N, CA, C finite
  brk[0] = 1;  brk[j] = 0 iff present[j-1], present[j] and |C[j-1] - N[j]| <= 2.5;  a..b contiguous: brk[k] == 0 for k in a+1 .. b
  accept[i]        present[i] and O[i] finite
  donate[j]        brk[j] == 0, accept[j-1], not no_donor[j];  H[j] = N[j] + (C[j-1] - O[j-1]) / |C[j-1] - O[j-1]|
  E(i, j)          donor j, acceptor i, i != j, i != j-1, |CA[i] - CA[j]| < 9:
                   27.888 * (((1/|O[i]-N[j]| + 1/|C[i]-H[j]|) - 1/|O[i]-H[j]|) - 1/|C[i]-N[j]|);  any of the four distances < 0.5: -9.9;
                   else an E below -9.9 becomes -9.9
  acceptor[j][0..1], energy[j][0..1]   the two candidates of lowest E among those with E < -0.5, ties to the smaller i, slot 0 the
                   lower; an empty slot holds -1 and 0.0.  hb(i, j) iff i is in acceptor[j]
  turns, bridges, ladders, the passes (a) .. (g)   as DESIGN.md §3.22 states them
  codes            0 '-', 1 S, 2 T, 3 I, 4 G, 5 B, 6 E, 7 H;  counts[l, c] = #structures with residue l present and code c

`dssp` works on whole L x L arrays; `dssp_loops` is a second restatement of the same text in plain loops, one pair at a time."""
from __future__ import annotations

import numpy as np

LEGEND = "-STIGBEH"
LOOP, S, T, I, G, B, E, H = range(8)
COS70 = 0.3420201433256687
CA_CUT, E_CUT, E_MIN, D_MIN, Q = 9.0, -0.5, -9.9, 0.5, 27.888
BREAK = 2.5


def string(codes) -> str:
    return "".join(LEGEND[c] for c in codes)


def _dist(a, b):
    d = a - b
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    return np.sqrt((dx * dx + dy * dy) + dz * dz)


# ---- the vectorised restatement ---------------------------------------------------------------------------------------------------
def _flags(x, mask, no_donor):
    """-> present, brk, accept, donate (bool (L,)), Hpos (L, 3) (rows of non-donors are never read)."""
    L = x.shape[0]
    N, CA, C, O = x[:, 0], x[:, 1], x[:, 2], x[:, 3]
    present = np.isfinite(x[:, :3]).all((1, 2))
    if mask is not None:
        present &= np.asarray(mask).astype(bool)
    brk = np.ones(L, bool)
    accept = present & np.isfinite(O).all(1)
    Hpos = np.full((L, 3), np.nan)
    if L > 1:
        brk[1:] = ~(present[:-1] & present[1:] & (_dist(C[:-1], N[1:]) <= BREAK))
        co = C[:-1] - O[:-1]
        Hpos[1:] = N[1:] + co / _dist(C[:-1], O[:-1])[:, None]
    donate = ~brk
    donate[1:] &= accept[:-1]
    if no_donor is not None:
        donate &= ~np.asarray(no_donor).astype(bool)
    return present, brk, accept, donate, Hpos


def _energies(x, accept, donate, Hpos):
    """-> E (L, L) indexed [i, j] (acceptor, donor): the energy of a candidate pair, +inf where the pair is none or E >= -0.5."""
    L = x.shape[0]
    N, CA, C, O = x[:, 0], x[:, 1], x[:, 2], x[:, 3]
    idx = np.arange(L)
    pair = accept[:, None] & donate[None, :] & (idx[:, None] != idx[None, :]) & (idx[:, None] != idx[None, :] - 1)
    pair &= _dist(CA[:, None], CA[None, :]) < CA_CUT
    i, j = np.nonzero(pair)
    don, dch, doh, dcn = _dist(O[i], N[j]), _dist(C[i], Hpos[j]), _dist(O[i], Hpos[j]), _dist(C[i], N[j])
    e = Q * (((1.0 / don + 1.0 / dch) - 1.0 / doh) - 1.0 / dcn)
    e = np.where(e < E_MIN, E_MIN, e)
    e = np.where((don < D_MIN) | (dch < D_MIN) | (doh < D_MIN) | (dcn < D_MIN), E_MIN, e)
    out = np.full((L, L), np.inf)
    ok = e < E_CUT
    out[i[ok], j[ok]] = e[ok]
    return out


def _two_best(Em):
    L = Em.shape[0]
    acceptor, energy = np.full((L, 2), -1, np.int32), np.zeros((L, 2))
    Em = Em.copy()
    cols = np.arange(L)
    for s in range(2):
        best = Em.argmin(0)                                      # the first of equal minima: the smaller i
        e = Em[best, cols]
        found = np.isfinite(e)
        acceptor[found, s], energy[found, s] = best[found], e[found]
        Em[best, cols] = np.inf
    return acceptor, energy


def _shift(M, di, dj):
    """out[i, j] = M[i + di, j + dj], False outside."""
    L = M.shape[0]
    out = np.zeros_like(M)
    si, sj = slice(max(0, -di), L - max(0, di)), slice(max(0, -dj), L - max(0, dj))
    ti, tj = slice(max(0, di), L - max(0, -di)), slice(max(0, dj), L - max(0, -dj))
    out[si, sj] = M[ti, tj]
    return out


def _bridges(acceptor, brk):
    """-> parallel, antiparallel bool (L, L)."""
    L = len(brk)
    hb = np.zeros((L, L), bool)
    for s in range(2):
        j = np.nonzero(acceptor[:, s] >= 0)[0]
        hb[acceptor[j, s], j] = True
    ok = np.zeros(L, bool)
    if L >= 3:
        ok[1:-1] = ~brk[1:-1] & ~brk[2:]
    idx = np.arange(L)
    valid = ok[:, None] & ok[None, :] & (np.abs(idx[:, None] - idx[None, :]) >= 3)
    hbT = hb.T
    par = (_shift(hb, -1, 0) & _shift(hbT, 1, 0)) | (_shift(hbT, 0, -1) & _shift(hb, 0, 1))
    anti = (hb & hbT) | (_shift(hb, -1, 1) & _shift(hbT, 1, -1))
    return par & valid, anti & valid


def _contig(brk, span):
    """c[i] = i + span < L and brk[k] == 0 for k in i+1 .. i+span."""
    L = len(brk)
    c = np.zeros(L, bool)
    if L > span:
        cb = np.cumsum(brk)
        c[:L - span] = cb[span:] == cb[:L - span]
    return c


def _assign(x, present, brk, acceptor):
    L = len(brk)
    ss = np.zeros(L, np.uint8)
    par, anti = _bridges(acceptor, brk)
    ladder = (par & (_shift(par, -1, -1) | _shift(par, 1, 1))) | (anti & (_shift(anti, -1, 1) | _shift(anti, 1, -1)))
    ss[(par | anti).any(1)] = B
    ss[ladder.any(1)] = E
    turn = {}
    for n in (3, 4, 5):
        t = np.zeros(L, bool)
        if L > n:
            a = acceptor[n:]
            t[:L - n] = (a[:, 0] == np.arange(L - n)) | (a[:, 1] == np.arange(L - n))
        turn[n] = t & _contig(brk, n)
    for n, code in ((4, H), (3, G), (5, I)):
        start = np.zeros(L, bool)
        start[1:] = turn[n][:-1] & turn[n][1:]
        if code != H:                                            # only where the whole stretch is still loop
            free = ss == LOOP
            whole = np.zeros(L, bool)
            if L >= n:
                whole[:L - n + 1] = np.all([free[k:L - n + 1 + k] for k in range(n)], axis=0)
            start &= whole
        for k in range(n):
            at = np.nonzero(start)[0] + k                        # i + n < L: in range
            ss[at] = code
    for n in (3, 4, 5):
        for k in range(1, n):
            at = np.nonzero(turn[n])[0] + k
            at = at[ss[at] == LOOP]
            ss[at] = T
    if L >= 5:
        CA = x[:, 1]
        mid = np.arange(2, L - 2)
        mid = mid[(ss[mid] == LOOP) & (_contig(brk, 4)[mid - 2])]
        u, v = CA[mid] - CA[mid - 2], CA[mid + 2] - CA[mid]
        with np.errstate(invalid="ignore", divide="ignore"):
            c = ((u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) + u[:, 2] * v[:, 2]) / np.sqrt(
                ((u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2]) * ((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]))
        ss[mid[c < COS70]] = S
    ss[~present] = LOOP
    return ss, par, anti


def dssp(X, mask=None, no_donor=None, details: bool = False):
    """X (n, L, 4, 3) or (L, 4, 3) -> ss u8 (n, L), counts i32 (L, 8), acceptor i32 (n, L, 2), energy f64 (n, L, 2); details: also a
    list of per-structure dicts {"parallel", "antiparallel": the numbers of bridges (unordered pairs), "candidates": per donor the
    number of acceptors with E < -0.5, "clamped": the number of candidate pairs at -9.9}."""
    X = np.asarray(X, np.float64)
    if X.ndim == 3:
        X = X[None]
    n, L = X.shape[:2]
    assert X.shape[2:] == (4, 3)
    mask = None if mask is None else np.asarray(mask).reshape(n, L)
    ss, acceptor, energy = np.zeros((n, L), np.uint8), np.zeros((n, L, 2), np.int32), np.zeros((n, L, 2))
    counts, info = np.zeros((L, 8), np.int32), []
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for k in range(n):
            x = X[k]
            present, brk, accept, donate, Hpos = _flags(x, None if mask is None else mask[k], no_donor)
            x = np.where(present[:, None, None], x, np.nan)      # a masked residue's coordinates are never looked at
            Em = _energies(x, accept, donate, Hpos)
            acceptor[k], energy[k] = _two_best(Em)
            ss[k], par, anti = _assign(x, present, brk, acceptor[k])
            counts[np.nonzero(present)[0], ss[k][present]] += 1
            if details:
                info.append({"parallel": int(np.triu(par).sum()), "antiparallel": int(np.triu(anti).sum()),
                             "candidates": np.isfinite(Em).sum(0), "clamped": int((Em == E_MIN).sum())})
    return (ss, counts, acceptor, energy, info) if details else (ss, counts, acceptor, energy)


# ---- the second restatement: plain loops ---------------------------------------------------------------------------------------------
def _d(a, b):
    dx, dy, dz = a[0] - b[0], a[1] - b[1], a[2] - b[2]
    return np.sqrt((dx * dx + dy * dy) + dz * dz)


def _one_loops(x, mask, no_donor):
    L = x.shape[0]
    N, CA, C, O = x[:, 0], x[:, 1], x[:, 2], x[:, 3]
    present = [bool((mask is None or mask[i]) and np.isfinite(x[i, :3]).all()) for i in range(L)]
    brk = [True] + [not (present[j - 1] and present[j] and _d(C[j - 1], N[j]) <= BREAK) for j in range(1, L)]
    accept = [present[i] and bool(np.isfinite(O[i]).all()) for i in range(L)]

    def contiguous(a, b):
        return all(not brk[k] for k in range(a + 1, b + 1))

    acceptor, energy = np.full((L, 2), -1, np.int32), np.zeros((L, 2))
    for j in range(1, L):
        if brk[j] or not accept[j - 1] or (no_donor is not None and no_donor[j]):
            continue
        Hj = N[j] + (C[j - 1] - O[j - 1]) / _d(C[j - 1], O[j - 1])
        found = []
        for i in range(L):
            if not accept[i] or i == j or i == j - 1 or not _d(CA[i], CA[j]) < CA_CUT:
                continue
            ds = (_d(O[i], N[j]), _d(C[i], Hj), _d(O[i], Hj), _d(C[i], N[j]))
            if any(d < D_MIN for d in ds):
                e = E_MIN
            else:
                e = Q * (((1.0 / ds[0] + 1.0 / ds[1]) - 1.0 / ds[2]) - 1.0 / ds[3])
                if e < E_MIN:
                    e = E_MIN
            if e < E_CUT:
                found.append((e, i))
        for s, (e, i) in enumerate(sorted(found)[:2]):
            acceptor[j, s], energy[j, s] = i, e

    def hb(i, j):
        return 0 <= i < L and 0 <= j < L and i in (acceptor[j, 0], acceptor[j, 1])

    def inner(i):
        return 1 <= i <= L - 2 and contiguous(i - 1, i + 1)

    def parallel(i, j):
        return inner(i) and inner(j) and abs(i - j) >= 3 and ((hb(i - 1, j) and hb(j, i + 1)) or (hb(j - 1, i) and hb(i, j + 1)))

    def antiparallel(i, j):
        return inner(i) and inner(j) and abs(i - j) >= 3 and ((hb(i, j) and hb(j, i)) or (hb(i - 1, j + 1) and hb(j - 1, i + 1)))

    def turn(n, i):
        return 0 <= i and i + n < L and hb(i, i + n) and contiguous(i, i + n)

    ss = [LOOP] * L
    for i in range(L):                                           # (a)
        for j in range(L):
            if parallel(i, j):
                ss[i] = max(ss[i], B)
                if parallel(i - 1, j - 1) or parallel(i + 1, j + 1):
                    ss[i] = E
            if antiparallel(i, j):
                ss[i] = max(ss[i], B)
                if antiparallel(i - 1, j + 1) or antiparallel(i + 1, j - 1):
                    ss[i] = E
    for i in range(1, L):                                        # (b)
        if turn(4, i - 1) and turn(4, i):
            ss[i:i + 4] = [H] * 4
    for n, code in ((3, G), (5, I)):                             # (c), (d)
        before = list(ss)
        for i in range(1, L):
            if turn(n, i - 1) and turn(n, i) and all(before[k] == LOOP for k in range(i, i + n)):
                ss[i:i + n] = [code] * n
    for n in (3, 4, 5):                                          # (e)
        for i in range(L):
            if turn(n, i):
                for k in range(i + 1, i + n):
                    if ss[k] == LOOP:
                        ss[k] = T
    for i in range(2, L - 2):                                    # (f)
        if ss[i] == LOOP and contiguous(i - 2, i + 2):
            u, v = CA[i] - CA[i - 2], CA[i + 2] - CA[i]
            c = ((u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]) / np.sqrt(
                ((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]) * ((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]))
            if c < COS70:
                ss[i] = S
    for i in range(L):                                           # (g)
        if not present[i]:
            ss[i] = LOOP
    return np.array(ss, np.uint8), np.array(present), acceptor, energy


def dssp_loops(X, mask=None, no_donor=None):
    """The same outputs as `dssp`, one pair at a time (O(L^2) Python steps per structure: for short chains)."""
    X = np.asarray(X, np.float64)
    if X.ndim == 3:
        X = X[None]
    n, L = X.shape[:2]
    mask = None if mask is None else np.asarray(mask).reshape(n, L)
    ss, acceptor, energy = np.zeros((n, L), np.uint8), np.zeros((n, L, 2), np.int32), np.zeros((n, L, 2))
    counts = np.zeros((L, 8), np.int32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for k in range(n):
            ss[k], present, acceptor[k], energy[k] = _one_loops(X[k], None if mask is None else mask[k], no_donor)
            for l in range(L):
                if present[l]:
                    counts[l, ss[k, l]] += 1
    return ss, counts, acceptor, energy


def reduce3(codes) -> np.ndarray:
    """Eight codes -> 0 helix (H, G, I), 1 strand (E, B), 2 coil."""
    return np.array([2, 2, 2, 0, 0, 1, 1, 0], np.uint8)[np.asarray(codes)]


# ---- synthetic chains (NeRF) ---------------------------------------------------------------------------------------------------------
def _place(a, b, c, bond, angle, torsion):
    """The point d with |c d| = bond, angle b-c-d and dihedral a-b-c-d (degrees)."""
    angle, torsion = np.deg2rad(angle), np.deg2rad(torsion)
    bc = c - b
    bc /= np.linalg.norm(bc)
    nrm = np.cross(b - a, bc)
    nrm /= np.linalg.norm(nrm)
    m = np.cross(nrm, bc)
    d2 = np.array([-bond * np.cos(angle), bond * np.sin(angle) * np.cos(torsion), bond * np.sin(angle) * np.sin(torsion)])
    return c + d2[0] * bc + d2[1] * m + d2[2] * nrm


def nerf(phi_psi) -> np.ndarray:
    """[(phi, psi)] in degrees -> (L, 4, 3) N, CA, C, O: ideal bond lengths and angles, omega = 180; O at 1.231 A from C, CA-C-O
    120.5 degrees, dihedral N-CA-C-O = psi + 180."""
    phi_psi = list(phi_psi)
    L = len(phi_psi)
    x = np.zeros((L, 4, 3))
    x[0, 0] = (0.0, 0.0, 0.0)
    x[0, 1] = (1.458, 0.0, 0.0)
    ang = np.deg2rad(111.0)
    x[0, 2] = x[0, 1] + 1.525 * np.array([-np.cos(ang), np.sin(ang), 0.0])
    for i in range(L):
        psi = phi_psi[i][1]
        x[i, 3] = _place(x[i, 0], x[i, 1], x[i, 2], 1.231, 120.5, psi + 180.0)
        if i + 1 < L:
            x[i + 1, 0] = _place(x[i, 0], x[i, 1], x[i, 2], 1.329, 116.2, psi)
            x[i + 1, 1] = _place(x[i, 1], x[i, 2], x[i + 1, 0], 1.458, 121.7, 180.0)
            x[i + 1, 2] = _place(x[i, 2], x[i + 1, 0], x[i + 1, 1], 1.525, 111.0, phi_psi[i + 1][0])
    return x


ALPHA, HELIX310, PI, BETA = (-57.0, -47.0), (-49.0, -26.0), (-57.0, -70.0), (-120.0, 130.0)
MIXED = [ALPHA] * 10 + [BETA] * 6 + [HELIX310] * 8 + [PI] * 10

"""esmdiff_rmsd_prepare and esmdiff_rmsd_nearest (csrc/rmsd_nn.hip) restated in plain numpy float64 (a helper, no test).

  prepare          the centroid, G and the centred, compacted, zero-padded copy in the PUBLISHED ORDER of the kernel: lane l of 64 adds the
                   selected residues among l, l + 64, ... in increasing order from +0.0, then s_l = s_l + s_{l ^ d} for d = 32, 16, 8, 4,
                   2, 1; the centroid is that sum / N; G the same walk and tree over ((dx dx + dy dy) + dz dz), d = x - c.
  exact            the same quantities and the cross products H_ij = sum_l a_il b_jl^T in int64, for integer frames whose centroid is an integer.
  msd_direct       the reference of the error bar: direct Kabsch by numpy.linalg.svd with the determinant rule, DEVIATION form
                   (sum |R a - b|^2 / N with the rotation applied), no Gram identity anywhere.
  bar              16 (L_sel + 16) u (sum |a|^2 + sum |b|^2) / N with the sums about the ORIGIN (centring error is covered), u = 2^-53:
                   gamma_L on each of the nine inner products and on G, Weyl |ds_k| <= |dH|_F, 3 gamma_L sqrt(G_a G_b) <= 1.5 gamma_L
                   (G_a + G_b), three singular values, counted twice.
  gaps             per row and per column, second-best minus best msd; index tests assert gap > 2 bar for every row and column.
  fold_sums        row / column sums of sqrt(msd) in the PUBLISHED ORDER: the pairs are cut into rectangles of RECT frames a side; within
                   a rectangle a row's pairs are added in increasing j from +0.0 (a column's in increasing i), and a frame's rectangle
                   partials are added in increasing rectangle number from +0.0 (self mode: the rectangle that holds the frame itself
                   gives two partials, j < i then j > i).  Pairs with an unused frame are skipped.
  assert_clear     cutoffs and bin edges lie farther than the bar from every reference value.
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -53
RECT = 128           # ESMDIFF_RMSD_NN_RECT (tests assert it against esmdiff_amd._native)


def padded(n_sel: int) -> int:
    return (n_sel + 3) // 4 * 4


def _tree(s):
    """s (..., 64) -> the xor tree's value (every lane ends with the same bits; lane 0 is returned)."""
    idx = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        s = s + s[..., idx ^ d]
    return s[..., 0]


def _lane_sums(v, sel):
    """v (n, L) -> (n, 64): lane l's running sum over the selected residues among l, l + 64, ... from +0.0."""
    n, L = v.shape
    s = np.zeros((n, 64))
    for base in range(0, L, 64):
        for lane in range(min(64, L - base)):
            if sel[base + lane]:
                s[:, lane] = s[:, lane] + v[:, base + lane]
    return s


def prepare(X, sel=None):
    """X (n, L, 3), sel bool (L,) or None -> dict(P (n, 3, K), info (n, 4), use u8 (n,), n_sel), the kernel's bits."""
    X = np.asarray(X, np.float64)
    n, L = X.shape[:2]
    sel = np.ones(L, bool) if sel is None else np.asarray(sel, bool)
    N, K = int(sel.sum()), padded(int(sel.sum()))
    use = np.isfinite(X[:, sel]).all((1, 2))
    Xs = np.where(use[:, None, None], X, 0.0)
    with np.errstate(all="ignore"):
        c = np.stack([_tree(_lane_sums(Xs[:, :, k], sel)) / float(N) for k in range(3)], 1)
        d = Xs - c[:, None, :]
        G = _tree(_lane_sums((d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2], sel))
    use &= np.isfinite(G)
    P = np.zeros((n, 3, K))
    P[:, :, :N] = np.transpose(d[:, sel], (0, 2, 1))
    P[~use] = 0.0
    info = np.concatenate([c, G[:, None]], 1)
    info[~use] = 0.0
    return {"P": P, "info": info, "use": use.astype(np.uint8), "n_sel": N}


def exact(A, B, sel=None):
    """Integer frames whose selected centroid is an integer -> centroids (n, 3), G (n,) of A, and cross (n, m, 9), all int64."""
    A, B = np.asarray(A), np.asarray(B)
    sel = np.ones(A.shape[1], bool) if sel is None else np.asarray(sel, bool)
    N = int(sel.sum())
    out = []
    for X in (A, B):
        Xi = X[:, sel].astype(np.int64)
        s = Xi.sum(1)
        assert (s % N == 0).all(), "the centroid of every frame should be an integer"
        c = s // N
        out.append((c, Xi - c[:, None, :]))
    (ca, a), (cb, b) = out
    cross = np.einsum("ilr,jlc->ijrc", a, b).reshape(len(A), len(B), 9)
    return ca, (a * a).sum((1, 2)), cb, (b * b).sum((1, 2)), cross


def msd_direct(A, B, sel=None, reflection=False):
    """(n, m) mean squared deviation after the least-squares fit, by SVD with the determinant rule, deviation form."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    sel = np.ones(A.shape[1], bool) if sel is None else np.asarray(sel, bool)
    a, b = A[:, sel], B[:, sel]
    a, b = a - a.mean(1, keepdims=True), b - b.mean(1, keepdims=True)
    H = np.einsum("ilr,jlc->ijrc", a, b)
    Um, S, Vt = np.linalg.svd(H)
    if not reflection:
        flip = np.linalg.det(Um) * np.linalg.det(Vt) < 0
        Vt = Vt.copy()
        Vt[flip, 2, :] *= -1.0
    R = np.einsum("ijrk,ijkc->ijrc", Um, Vt)               # a R ~ b (row vectors)
    out = np.empty(H.shape[:2])
    for i in range(len(a)):
        moved = np.einsum("lr,jrc->jlc", a[i], R[i])
        out[i] = ((moved - b) ** 2).sum((1, 2)) / a.shape[1]
    return out


def bar(A, B, sel=None):
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    sel = np.ones(A.shape[1], bool) if sel is None else np.asarray(sel, bool)
    N = int(sel.sum())
    na, nb = (A[:, sel] ** 2).sum((1, 2)), (B[:, sel] ** 2).sum((1, 2))
    return 16.0 * (N + 16) * U * (na[:, None] + nb[None, :]) / N


def gaps(msd):
    """msd (n, m) with NaN / inf where there is no pair -> (row gap (n,), col gap (m,)): second best minus best (inf with one pair)."""
    v = np.where(np.isnan(msd), np.inf, msd)
    def gap(w):
        if w.shape[1] < 2:
            return np.full(w.shape[0], np.inf)
        s = np.sort(w, 1)
        with np.errstate(invalid="ignore"):
            return np.where(np.isfinite(s[:, 1]), s[:, 1] - s[:, 0], np.inf)
    return gap(v), gap(v.T)


def assert_separated(msd_ref, bars):
    """Every row and column: best and second-best reference msd differ by more than twice the (largest) bar."""
    rg, cg = gaps(msd_ref)
    b = float(np.nanmax(bars))
    assert (rg > 2 * b).all() and (cg > 2 * b).all(), (rg.min(), cg.min(), b)


def assert_clear(msd_ref, bars, marks):
    """marks (rmsd units: cutoffs, bin edges) are farther than the bar from every reference value, compared as msd."""
    v = msd_ref[np.isfinite(msd_ref)]
    b = np.broadcast_to(bars, msd_ref.shape)[np.isfinite(msd_ref)]
    for mark in np.asarray(marks, np.float64).reshape(-1):
        assert (np.abs(v - mark * mark) > b).all(), (mark, float(np.abs(v - mark * mark).min()))


def _seq(values):
    s = 0.0
    for v in values:
        s = s + v
    return s


def fold_sums(rmsd, use_a, use_b=None):
    """rmsd (n, m) the per-pair values whose bits are to be summed (use_b None: self mode, rmsd (n, n) symmetric, pairs i != j) ->
    (row sums (n,), col sums (m,) or None) in the published order."""
    rmsd = np.asarray(rmsd, np.float64)
    n, m = rmsd.shape
    self_mode = use_b is None
    ub = use_a if self_mode else use_b

    def side(mat, u_own, u_other):
        out = np.zeros(mat.shape[0])
        for i in range(mat.shape[0]):
            if not u_own[i]:
                continue
            total = 0.0
            for b0 in range(0, mat.shape[1], RECT):
                js = [j for j in range(b0, min(b0 + RECT, mat.shape[1])) if u_other[j] and not (self_mode and j == i)]
                groups = [[j for j in js if j < i], [j for j in js if j > i]] if self_mode and b0 <= i < b0 + RECT else [js]
                for g in groups:
                    if g:
                        total = total + _seq(mat[i, g])
            out[i] = total
        return out

    rows = side(rmsd, use_a, ub)
    return rows, (None if self_mode else side(rmsd.T, ub, use_a))


def nearest(msd, use_a, use_b=None):
    """Reference minima on a dense msd: (row min msd, row argmin, col min, col argmin), NaN / -1 without a pair; lowest index on ties."""
    msd = np.asarray(msd, np.float64)
    self_mode = use_b is None
    ub = use_a if self_mode else use_b
    ok = np.asarray(use_a, bool)[:, None] & np.asarray(ub, bool)[None, :]
    if self_mode:
        ok &= ~np.eye(len(msd), dtype=bool)
    v = np.where(ok, msd, np.inf)
    def best(w, has):
        arg = np.where(has, w.argmin(1), -1)
        return np.where(has, w.min(1), np.nan), arg.astype(np.int32)
    r = best(v, ok.any(1))
    c = best(v.T, ok.any(0))
    return r[0], r[1], c[0], c[1], ok


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def chain(rng, L):
    steps = rng.normal(size=(L, 3))
    steps *= 3.8 / np.linalg.norm(steps, axis=1, keepdims=True)
    return np.cumsum(steps, 0)


def chains(rng, n, L, shift=20.0):
    """n independent random chains, each moved by a random offset: no two are close, every gap is many orders above the bar."""
    return np.stack([chain(rng, L) + rng.normal(size=3) * shift for _ in range(n)])


def rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q *= np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] *= -1
    return q

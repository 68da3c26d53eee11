"""The samplers' draws as random variables: what the reference specifies, in float64, and the statistics that hold a set of ids to it.
Used by tests/test_sampler_distribution_cpu.py on the C oracle (N = 16 384 draws) and by tests/test_gpu_sampler_distribution.py on
the kernels (N = 2^20); problems and seeds are shared by import, and a seed is admissible only if the oracle passes with it.

  ddpm update (model.py:527-533, 602-603)  q_v = softmax(z + mask column at -1e6)_v (mc_t - mc_s), q_MASK = mc_s, normalised
  gibbs step (esm sample_logits order)     sort descending, keep the prefix whose cumulative probability is <= top_p (always the
                                           top-1), then drop ids >= 4096 and invalid_ids; softmax(kept / T), or the arg-max at T = 0
  q_xt (model.py:494-512)                  each position masked with probability move_chance, independently
  gibbs strategy "random"                  a uniform k-subset of the eligible positions

Bars (the issue's): every p-value >= 1e-4, every |z| <= 4.5.
"""
from __future__ import annotations

import ctypes

import numpy as np
from scipy import stats

from oracle import c_oracle

MASK, V, NVALID = 4096, 4101, 4096
P_BAR, Z_BAR = 1e-4, 4.5
LD = 4104

# (logit scale, mc_t, mc_s); the final pass is its own case (deterministic)
DDPM_PROBLEMS = [(2.0, 0.5, 0.3), (4.0, 0.999, 0.95904), (1.0, 0.04, 1e-5), (6.0, 0.7, 0.0)]
DDPM_SEED, DDPM_OFFSET, DDPM_STEP, DDPM_L = 11, 5, 7, 64
# name -> (logit scale, temperature, top_p, head width, heavy special id, invalid ids)
GIBBS_PROBLEMS = {
    "T1.4 p0.9": (2.0, 1.4, 0.9, 4101, False, ()),
    "T0.7 p0.5": (3.0, 0.7, 0.5, 4101, False, ()),
    "T1 p1": (1.0, 1.0, 1.0, 4101, False, ()),
    "T1.4 p0.9 stock head": (2.0, 1.4, 0.9, 4096, False, ()),
    "heavy special id": (2.0, 1.0, 0.9, 4101, True, ()),
    "invalid ids": (2.0, 1.0, 0.9, 4101, False, tuple(range(0, 4096, 3))),
    "T0": (2.0, 0.0, 0.9, 4101, False, ()),
}
GIBBS_SEED, GIBBS_OFFSET, GIBBS_STEP, GIBBS_L = 3, 9, 2, 258
QXT_CHANCES = [0.02, 0.5, 0.98]
QXT_SEED = 21
RANDOM_SEED, RANDOM_L, RANDOM_K, RANDOM_PROMPTS = 13, 34, 5, 4096


def logit_row(scale: float, seed: int = 0, heavy_special: bool = False) -> np.ndarray:
    """One row of LD float32 logits, N(0, scale^2); heavy_special: id 4099 (a special id) made the row's largest by 1."""
    z = (np.random.RandomState(1000 + seed).standard_normal(LD) * scale).astype(np.float32)
    if heavy_special:
        z[4099] = z[:V].max() + np.float32(1.0)
    return z


def _softmax(z):
    e = np.exp(z - z.max())
    return e / e.sum()


def ddpm_probs(z, mc_t, mc_s) -> np.ndarray:
    """q [V] of one masked row; mc_t, mc_s as the float32 values the kernel is handed."""
    zz = np.asarray(z[:V], dtype=np.float64).copy()
    zz[MASK] += -1e6
    mt, ms = float(np.float32(mc_t)), float(np.float32(mc_s))
    q = _softmax(zz) * (mt - ms)
    q[MASK] = ms
    return q / q.sum()


def ddpm_final_id(z) -> int:
    zz = np.asarray(z[:V], dtype=np.float64).copy()
    zz[MASK] += -1e6
    return int(zz.argmax())


def gibbs_kept(z, vocab, top_p, invalid_ids=()):
    """(kept ids ascending, margin): esm's nucleus over the whole row of `vocab` logits, then the specials and invalid_ids removed.
    margin = how far the cumulative probability on either side of the cut is from top_p (the kernel sums in float32: a margin above
    1e-5 keeps its cut where float64 puts it)."""
    zz = np.asarray(z[:vocab], dtype=np.float64)
    p = _softmax(zz)
    order = np.argsort(-zz, kind="stable")
    cum = np.cumsum(p[order])
    n = max(1, int((cum <= top_p).sum())) if top_p < 1.0 else vocab
    margin = min(abs(cum[n - 1] - top_p), abs(cum[min(n, vocab - 1)] - top_p)) if top_p < 1.0 else 1.0
    kept = order[:n]
    kept = kept[kept < NVALID]
    if len(invalid_ids):
        kept = kept[~np.isin(kept, np.asarray(invalid_ids))]
    return np.sort(kept), float(margin)


def cut_has_no_tie(z, vocab, top_p) -> bool:
    """No two equal logits within 1e-3 of the nucleus cut (the kernel keeps or drops a tie group whole; esm's sort splits it)."""
    if top_p >= 1.0:
        return True
    zz = np.asarray(z[:vocab], dtype=np.float64)
    p = _softmax(zz)
    order = np.argsort(-zz, kind="stable")
    n = max(1, int((np.cumsum(p[order]) <= top_p).sum()))
    cut = zz[order[n - 1]]
    near = np.sort(zz[np.abs(zz - cut) <= 1e-3])
    return bool((np.diff(near) > 0).all())


def gibbs_probs(z, vocab, temperature, top_p, invalid_ids=()) -> np.ndarray:
    """p [4096] of the id one masked row draws."""
    kept, _ = gibbs_kept(z, vocab, top_p, invalid_ids)
    zz = np.asarray(z[:NVALID], dtype=np.float64)
    p = np.zeros(NVALID)
    if kept.size == 0:                 # nothing valid in the nucleus: the best valid id (csrc/gibbs.hip)
        ok = np.ones(NVALID, dtype=bool)
        ok[list(invalid_ids)] = False
        p[int(np.where(ok, zz, -np.inf).argmax())] = 1.0
    elif temperature == 0.0:
        p[kept[zz[kept].argmax()]] = 1.0
    else:
        p[kept] = _softmax(zz[kept] / float(np.float32(temperature)))
    return p


# ---- statistics -------------------------------------------------------------------------------------------------------------------
def chi_square(ids, probs, min_expected: float = 20.0):
    """(chi2, dof, p) of ids against probs: cells of expectation < min_expected are pooled into one, which joins the smallest other
    cell if it is still below; cells of expectation 0 are no cells (a caller asserts that nothing was drawn there)."""
    ids = np.asarray(ids).reshape(-1)
    n = ids.size
    counts = np.bincount(ids, minlength=probs.size).astype(np.float64)
    expect = probs * n
    assert counts[expect == 0].sum() == 0, "ids of probability 0 were drawn"
    big = expect >= min_expected
    o, e = list(counts[big]), list(expect[big])
    small = (~big) & (expect > 0)
    if small.any():
        so, se = counts[small].sum(), expect[small].sum()
        if se >= min_expected or not e:
            o.append(so), e.append(se)
        else:
            j = int(np.argmin(e))
            o[j] += so
            e[j] += se
    o, e = np.asarray(o), np.asarray(e)
    assert abs(o.sum() - n) < 0.5 and abs(e.sum() - n) < 1e-6 * n and (e > 0).all()
    if o.size < 2:
        return 0.0, 0, 1.0
    c = float(((o - e) ** 2 / e).sum())
    return c, o.size - 1, float(stats.chi2.sf(c, o.size - 1))


def coincidence_z(a, b, probs) -> float:
    """z of the number of equal entries of two id arrays drawn independently from probs: (#equal - m S) / sqrt(m S (1 - S)), S = sum q^2."""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    m, s = a.size, float((np.asarray(probs, dtype=np.float64) ** 2).sum())
    return float((int((a == b).sum()) - m * s) / np.sqrt(m * s * (1 - s)))


def binomial_z(k, n, p) -> float:
    return float((k - n * p) / np.sqrt(n * p * (1 - p)))


def neighbour_pairs(ids, axis):
    """(a, b) = entries 0, 2, 4, ... and 1, 3, 5, ... along `axis`: disjoint pairs of neighbours, so the pairs are independent."""
    ids = np.asarray(ids)
    n = ids.shape[axis] // 2 * 2
    sl = lambda s: tuple(s if d == axis else slice(None) for d in range(ids.ndim))
    return ids[sl(slice(0, n, 2))], ids[sl(slice(1, n, 2))]


def subset_pair_probability(n: int, k: int) -> float:
    """P(two given positions are both chosen or both left) for a uniform k-subset of n: the hypergeometric value."""
    both = k * (k - 1) / (n * (n - 1))
    neither = (n - k) * (n - k - 1) / (n * (n - 1))
    return both + neither


# ---- the C oracle on one shared logit row (row stride 0: every row reads the same logits) -----------------------------------------
def oracle_ddpm(z, B, L, mc_t, mc_s, seed, sample_offset, step, final=False) -> np.ndarray:
    x = np.full((B, L), MASK, dtype=np.int64)
    row = np.ascontiguousarray(z, dtype=np.float32)
    c_oracle.lib().oracle_ddpm_step(x.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), row.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                    0, V, np.float32(mc_t), np.float32(mc_s), int(final), None, int(seed), int(sample_offset),
                                    int(step), B, L)
    return x


def gibbs_tokens(B, L):
    """(x, seq): every interior position masked, BOS / EOS at the ends."""
    x = np.full((B, L), MASK, dtype=np.int64)
    x[:, 0], x[:, -1] = 4098, 4097
    seq = np.full((B, L), 5, dtype=np.int64)
    seq[:, 0], seq[:, -1] = 0, 2
    return x, seq


def oracle_gibbs(z, B, L, vocab, temperature, top_p, invalid_ids, seed, sample_offset, step, k=None, strategy="entropy") -> np.ndarray:
    """x after one step with n_unmask = k (default L: every masked position takes its draw)."""
    x, seq = gibbs_tokens(B, L)
    row = np.ascontiguousarray(z, dtype=np.float32)
    nu = np.full(B, L if k is None else k, dtype=np.int32)
    mask = np.zeros(128, dtype=np.uint32)
    for v in invalid_ids:
        mask[v >> 5] |= np.uint32(1 << (v & 31))
    i64p, f32p, i32p = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)
    c_oracle.lib().oracle_gibbs_step(x.ctypes.data_as(i64p), seq.ctypes.data_as(i64p), row.ctypes.data_as(f32p), 0, int(vocab),
                                     np.float32(temperature), np.float32(top_p), nu.ctypes.data_as(i32p), None, int(seed),
                                     int(sample_offset), int(step), B, L, None, None, 1 if strategy == "random" else 0,
                                     mask.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)) if len(invalid_ids) else None)
    return x


def oracle_q_xt(B, L, move_chance, seed, sample_index, draw, lengths=None) -> np.ndarray:
    """moved [B, L] bool: u < move_chance, u the Philox uniform of column 4104 (csrc/score.hip), l < lengths[b]."""
    mc = np.float32(move_chance)
    out = np.zeros((B, L), dtype=bool)
    for b in range(B):
        n = L if lengths is None else int(lengths[b])
        for l in range(n):
            out[b, l] = c_oracle.philox_uniforms(seed, int(sample_index[b]), int(draw[b]), l, vocab=4105)[4104] < mc
    return out

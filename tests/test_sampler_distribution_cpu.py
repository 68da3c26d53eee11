"""The C oracle's draws in distribution, at N = 16 384: the CPU twin of tests/test_gpu_sampler_distribution.py (same problems, same
seeds, same statistics, by import from tests/sampler_dist_ref.py).  A seed is admissible for the device test only if the oracle
passes here with it.  The planted cases show that each statistic fails when it should."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import sampler_dist_ref as D

B_DDPM = 16384 // D.DDPM_L             # 256 samples of 64 positions
B_GIBBS = 64                           # 64 prompts of 256 masked positions
N_QXT = (256, 64)
CPU_PROMPTS = 512                      # of RANDOM_PROMPTS: 16 384 rows, what the host affords

VARIANTS = {"sample + 2^32": dict(sample_offset=D.DDPM_OFFSET + 2 ** 32), "step + 1": dict(step=D.DDPM_STEP + 1),
            "seed + 1": dict(seed=D.DDPM_SEED + 1), "seed high word + 1": dict(seed=D.DDPM_SEED + 2 ** 32)}


def _ddpm(i, **over):
    scale, mc_t, mc_s = D.DDPM_PROBLEMS[i]
    kw = dict(seed=D.DDPM_SEED, sample_offset=D.DDPM_OFFSET, step=D.DDPM_STEP)
    kw.update(over)
    return D.oracle_ddpm(D.logit_row(scale, i), B_DDPM, D.DDPM_L, mc_t, mc_s, **kw)


def _gibbs(name):
    scale, T, top_p, vocab, heavy, invalid = D.GIBBS_PROBLEMS[name]
    return D.oracle_gibbs(D.logit_row(scale, 50, heavy), B_GIBBS, D.GIBBS_L, vocab, T, top_p, invalid, D.GIBBS_SEED, D.GIBBS_OFFSET,
                          D.GIBBS_STEP)


@pytest.fixture(scope="module")
def draws():
    """Every oracle run of this file, once, on a few threads (the oracle holds no state; ctypes releases the GIL)."""
    jobs = {("ddpm", i): (_ddpm, (i,), {}) for i in range(len(D.DDPM_PROBLEMS))}
    jobs.update({("ddpm0", k): (_ddpm, (0,), v) for k, v in VARIANTS.items()})
    jobs.update({("gibbs", n): (_gibbs, (n,), {}) for n in D.GIBBS_PROBLEMS})
    jobs[("random",)] = (D.oracle_gibbs, (D.logit_row(1.0, 60), CPU_PROMPTS, D.RANDOM_L, 4101, 1.0, 1.0, (), D.RANDOM_SEED, 0, 1),
                         dict(k=D.RANDOM_K, strategy="random"))
    D.c_oracle.lib()                   # built and loaded before the threads ask for it
    with ThreadPoolExecutor(max_workers=8) as ex:
        futures = {k: ex.submit(f, *a, **kw) for k, (f, a, kw) in jobs.items()}
        return {k: f.result() for k, f in futures.items()}


@pytest.mark.parametrize("i", range(len(D.DDPM_PROBLEMS)))
def test_ddpm_goodness_of_fit(draws, i):
    scale, mc_t, mc_s = D.DDPM_PROBLEMS[i]
    q = D.ddpm_probs(D.logit_row(scale, i), mc_t, mc_s)
    x = draws[("ddpm", i)]
    c, dof, p = D.chi_square(x, q)
    zm = D.binomial_z(int((x == D.MASK).sum()), x.size, q[D.MASK]) if q[D.MASK] > 0 else 0.0
    zl, zb = D.coincidence_z(*D.neighbour_pairs(x, 1), q), D.coincidence_z(*D.neighbour_pairs(x, 0), q)
    print(f"MEASURED sampler distribution oracle ddpm {D.DDPM_PROBLEMS[i]} N={x.size}: chi2 {c:.1f} / {dof} p {p:.3g}; MASK fraction z "
          f"{zm:.2f}; coincidence z l|l+1 {zl:.2f}, sample|sample+1 {zb:.2f}")
    assert p >= D.P_BAR and abs(zm) <= D.Z_BAR and abs(zl) <= D.Z_BAR and abs(zb) <= D.Z_BAR
    if q[D.MASK] == 0:
        assert not (x == D.MASK).any()


def test_ddpm_final_pass_is_the_arg_max():
    for i, (scale, _, _) in enumerate(D.DDPM_PROBLEMS):
        z = D.logit_row(scale, i)
        x = D.oracle_ddpm(z, 2, D.DDPM_L, 0.0, 0.0, D.DDPM_SEED, D.DDPM_OFFSET, D.DDPM_STEP, final=True)
        assert (x == D.ddpm_final_id(z)).all()


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_ddpm_independence_between_counters(draws, variant):
    scale, mc_t, mc_s = D.DDPM_PROBLEMS[0]
    q = D.ddpm_probs(D.logit_row(scale, 0), mc_t, mc_s)
    z = D.coincidence_z(draws[("ddpm", 0)], draws[("ddpm0", variant)], q)
    c, dof, p = D.chi_square(draws[("ddpm0", variant)], q)
    print(f"MEASURED sampler distribution oracle ddpm independence {variant}: coincidence z {z:.2f}; chi2 p {p:.3g}")
    assert abs(z) <= D.Z_BAR and p >= D.P_BAR


@pytest.mark.parametrize("name", list(D.GIBBS_PROBLEMS))
def test_gibbs_goodness_of_fit(draws, name):
    scale, T, top_p, vocab, heavy, invalid = D.GIBBS_PROBLEMS[name]
    z = D.logit_row(scale, 50, heavy)
    assert D.cut_has_no_tie(z, vocab, top_p)
    kept, margin = D.gibbs_kept(z, vocab, top_p, invalid)
    assert margin > 1e-5 and kept.size > 1
    if heavy:
        assert int(np.argmax(z[:vocab])) == 4099 and kept.size < D.gibbs_kept(D.logit_row(scale, 50), vocab, top_p)[0].size
    p = D.gibbs_probs(z, vocab, T, top_p, invalid)
    x = draws[("gibbs", name)]
    assert (x[:, 0] == 4098).all() and (x[:, -1] == 4097).all()
    ids = x[:, 1:-1]
    assert np.isin(ids, kept).all()                       # nothing outside the kept set, specials and invalid ids included
    if T == 0.0:
        assert (ids == kept[np.argmax(z[kept])]).all()
        return
    c, dof, pv = D.chi_square(ids, p)
    zl = D.coincidence_z(*D.neighbour_pairs(ids, 1), p)
    print(f"MEASURED sampler distribution oracle gibbs {name} N={ids.size}: kept {kept.size}, chi2 {c:.1f} / {dof} p {pv:.3g}; "
          f"coincidence z l|l+1 {zl:.2f}")
    assert pv >= D.P_BAR and abs(zl) <= D.Z_BAR


@pytest.mark.parametrize("chance", D.QXT_CHANCES)
def test_q_xt_masks_with_the_stated_probability(chance):
    B, L = N_QXT
    lengths = [L - (b % 7) for b in range(B)]
    moved = D.oracle_q_xt(B, L, chance, D.QXT_SEED, list(range(100, 100 + B)), [b % 3 for b in range(B)], lengths)
    valid = np.arange(L)[None] < np.asarray(lengths)[:, None]
    assert not moved[~valid].any()
    n = int(valid.sum())
    zf = D.binomial_z(int(moved.sum()), n, float(np.float32(chance)))
    full = moved[:, :L - 6]                               # columns every sample holds
    zc = D.coincidence_z(*D.neighbour_pairs(full.astype(np.int64), 1), [chance, 1 - chance])
    print(f"MEASURED sampler distribution oracle q_xt {chance} N={n}: masked fraction z {zf:.2f}; coincidence z l|l+1 {zc:.2f}")
    assert abs(zf) <= D.Z_BAR and abs(zc) <= D.Z_BAR


def random_subset_statistics(x):
    """(every prompt unmasks exactly k, chi2 p of the positions' counts, coincidence z between positions i and i + 1)."""
    chosen = x[:, 1:-1] != D.MASK
    n = chosen.shape[1]
    exact = bool((chosen.sum(1) == D.RANDOM_K).all())
    counts = chosen.sum(0)
    c, dof, p = D.chi_square(np.repeat(np.arange(n), counts), np.full(n, 1.0 / n))
    s = D.subset_pair_probability(n, D.RANDOM_K)
    a, b = D.neighbour_pairs(chosen, 1)
    m = a.size
    z = float((int((a == b).sum()) - m * s) / np.sqrt(m * s * (1 - s)))
    return exact, p, z


def test_gibbs_random_strategy_picks_a_uniform_subset(draws):
    exact, p, z = random_subset_statistics(draws[("random",)])
    print(f"MEASURED sampler distribution oracle gibbs random {CPU_PROMPTS} prompts: positions chi2 p {p:.3g}; coincidence z i|i+1 {z:.2f}")
    assert exact and p >= D.P_BAR and abs(z) <= D.Z_BAR


# ---- planted: each statistic fails when it should ---------------------------------------------------------------------------------
def test_planted_wrong_expectation_fails_chi_square():
    """Draws from the true probabilities (numpy's generator, N = 2^20) against the expectation with T off by 5 % and with mc_s off by
    2 %: p < 1e-8, and the MASK fraction's z leaves the bar; against the true expectation they pass."""
    rs = np.random.RandomState(1)
    n = 1 << 20
    scale, T, top_p, vocab, heavy, invalid = D.GIBBS_PROBLEMS["T1.4 p0.9"]
    z = D.logit_row(scale, 50)
    p = D.gibbs_probs(z, vocab, T, top_p)
    ids = rs.choice(p.size, size=n, p=p)
    assert D.chi_square(ids, p)[2] >= D.P_BAR
    wrong = D.gibbs_probs(z, vocab, T * 1.05, top_p)
    assert D.chi_square(ids, wrong)[2] < 1e-8
    scale, mc_t, mc_s = D.DDPM_PROBLEMS[0]
    z = D.logit_row(scale, 0)
    q = D.ddpm_probs(z, mc_t, mc_s)
    ids = rs.choice(q.size, size=n, p=q)
    assert D.chi_square(ids, q)[2] >= D.P_BAR
    wrong = D.ddpm_probs(z, mc_t, mc_s * 1.02)
    assert D.chi_square(ids, wrong)[2] < 1e-8
    assert abs(D.binomial_z(int((ids == D.MASK).sum()), n, wrong[D.MASK])) > D.Z_BAR
    assert abs(D.binomial_z(int((ids == D.MASK).sum()), n, q[D.MASK])) <= D.Z_BAR


def test_planted_shared_uniforms_fail_the_coincidence_test(draws):
    """The same (seed, sample, step) requested twice shares every uniform: |z| > 10.  So does a second draw from the same uniforms
    at a slightly different distribution (mc_s moved): most ids coincide."""
    scale, mc_t, mc_s = D.DDPM_PROBLEMS[0]
    q = D.ddpm_probs(D.logit_row(scale, 0), mc_t, mc_s)
    again = _ddpm(0)
    assert abs(D.coincidence_z(draws[("ddpm", 0)], again, q)) > 10
    shifted = D.oracle_ddpm(D.logit_row(scale, 0), B_DDPM, D.DDPM_L, mc_t, mc_s * 0.9, D.DDPM_SEED, D.DDPM_OFFSET, D.DDPM_STEP)
    assert abs(D.coincidence_z(draws[("ddpm", 0)], shifted, q)) > 10
    # and a position that copies its neighbour fails the test between positions
    x = draws[("ddpm", 0)].copy()
    x[:, 1::8] = x[:, 0::8]
    assert abs(D.coincidence_z(*D.neighbour_pairs(x, 1), q)) > 10

"""The kernels' draws as random variables (csrc/sampler.hip, csrc/gibbs.hip, csrc/score.hip), at the power only the device affords:
N = 2^20 ids per ddpm problem against the float64 probabilities of tests/sampler_dist_ref.py, coincidence tests between draws that
differ in exactly one Philox counter, the masked fraction of q_xt and the subsets of the gibbs "random" strategy.

The bit-exact tests hold the kernels to an oracle that shares their math header and their counter layout, so a flaw in either is the
same on both sides; a distribution has no such blind spot.  Problems, seeds and statistics are tests/test_sampler_distribution_cpu.py's
(the C oracle passes with these seeds at N = 16 384).  Bars: every p >= 1e-4, every |z| <= 4.5; the planted cases must fail."""
import numpy as np
import pytest
import torch

from tests import sampler_dist_ref as D
from tests.test_sampler_distribution_cpu import VARIANTS, random_subset_statistics

pytestmark = pytest.mark.gpu

N_DDPM = 1 << 20
B_DDPM = N_DDPM // D.DDPM_L            # 16 384 samples of 64 positions, one logit row handed once (logits_period = 1)
B_ENG, L_ENG = 64, D.GIBBS_L


def _engine(vocab):
    from esmdiff_amd.config import ModelConfig
    from esmdiff_amd.engine import Engine
    from esmdiff_amd.weights import random_init_state_dict
    if vocab == 4101:
        cfg = ModelConfig(d_model=512, n_heads=8, v_heads=128, n_layers=1)
        sd = random_init_state_dict(cfg, seed=2)
    else:                              # the stock-ESM3 head: 4096-way, no sigma embedder
        cfg = ModelConfig(d_model=512, n_heads=8, v_heads=128, n_layers=1, n_structure_heads=4096, time_conditioning=False)
        sd = {k: v for k, v in random_init_state_dict(cfg, seed=2).items() if not k.startswith("sigma_embedder.")}
    assert cfg.n_structure_heads == vocab
    return Engine(cfg, sd, max_batch=B_ENG, max_len=L_ENG)


@pytest.fixture(scope="module")
def engines():
    made = {}

    def get(vocab):
        if vocab not in made:
            made[vocab] = _engine(vocab)
        return made[vocab]
    yield get
    for e in made.values():
        e.close()


def _ddpm_device(i, B=B_DDPM, final=False, **over):
    """ids [B, 64] of ddpm problem i through esmdiff_ddpm_step_mapped: every row MASK, one logit row repeated over the 64 positions."""
    from esmdiff_amd.engine import ddpm_step_mapped
    scale, mc_t, mc_s = D.DDPM_PROBLEMS[i]
    kw = dict(seed=D.DDPM_SEED, sample_offset=D.DDPM_OFFSET, step=D.DDPM_STEP)
    kw.update(over)
    logits = torch.from_numpy(D.logit_row(scale, i)).cuda()[None].repeat(D.DDPM_L, 1).contiguous()
    x = torch.full((B, D.DDPM_L), D.MASK, dtype=torch.int64, device="cuda")
    return ddpm_step_mapped(x, logits, D.V, mc_t, mc_s, final=final, logits_period=1, **kw).cpu().numpy()


@pytest.fixture(scope="module")
def ddpm0():
    """Problem 0's 2^20 ids, shared by the independence and planted tests."""
    return _ddpm_device(0)


@pytest.mark.parametrize("i", range(len(D.DDPM_PROBLEMS)))
def test_ddpm_goodness_of_fit(ddpm0, i):
    scale, mc_t, mc_s = D.DDPM_PROBLEMS[i]
    q = D.ddpm_probs(D.logit_row(scale, i), mc_t, mc_s)
    x = ddpm0 if i == 0 else _ddpm_device(i)
    c, dof, p = D.chi_square(x, q)
    zm = D.binomial_z(int((x == D.MASK).sum()), x.size, q[D.MASK]) if q[D.MASK] > 0 else 0.0
    zl, zb = D.coincidence_z(*D.neighbour_pairs(x, 1), q), D.coincidence_z(*D.neighbour_pairs(x, 0), q)
    print(f"MEASURED sampler distribution device ddpm {D.DDPM_PROBLEMS[i]} N={x.size}: chi2 {c:.1f} / {dof} p {p:.3g}; MASK fraction z "
          f"{zm:.2f}; coincidence z l|l+1 {zl:.2f}, sample|sample+1 {zb:.2f}")
    assert p >= D.P_BAR and abs(zm) <= D.Z_BAR and abs(zl) <= D.Z_BAR and abs(zb) <= D.Z_BAR
    if q[D.MASK] == 0:
        assert not (x == D.MASK).any()


def test_ddpm_ids_equal_the_oracle_at_equal_n(ddpm0):
    """The two files hold the same thing: the device's first 256 samples of problem 0 are the oracle's 16 384 ids of the CPU twin."""
    scale, mc_t, mc_s = D.DDPM_PROBLEMS[0]
    want = D.oracle_ddpm(D.logit_row(scale, 0), 256, D.DDPM_L, mc_t, mc_s, D.DDPM_SEED, D.DDPM_OFFSET, D.DDPM_STEP)
    assert np.array_equal(ddpm0[:256], want)


def test_ddpm_final_pass_is_the_arg_max():
    for i, (scale, _, _) in enumerate(D.DDPM_PROBLEMS):
        x = _ddpm_device(i, B=64, final=True)
        assert (x == D.ddpm_final_id(D.logit_row(scale, i))).all()


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_ddpm_independence_between_counters(ddpm0, variant):
    """Draws that differ in exactly one counter (l | l + 1 and sample | sample + 1 are in the goodness-of-fit test)."""
    scale, mc_t, mc_s = D.DDPM_PROBLEMS[0]
    q = D.ddpm_probs(D.logit_row(scale, 0), mc_t, mc_s)
    other = _ddpm_device(0, **VARIANTS[variant])
    z = D.coincidence_z(ddpm0, other, q)
    c, dof, p = D.chi_square(other, q)
    print(f"MEASURED sampler distribution device ddpm independence {variant} N={other.size}: coincidence z {z:.2f}; chi2 p {p:.3g}")
    assert abs(z) <= D.Z_BAR and p >= D.P_BAR


def test_ddpm_step_rows_with_per_sample_parameters(engines):
    """esmdiff_ddpm_step_rows: 2048 samples of 64 positions, even samples at problem 0's move chances and odd ones at problem 2's,
    each with its own sample index and step; each half against its own probabilities (N = 2^16 each)."""
    eng = engines(4101)
    B, L = 2048, D.DDPM_L
    z = D.logit_row(D.DDPM_PROBLEMS[0][0], 0)
    groups = [D.DDPM_PROBLEMS[0][1:], D.DDPM_PROBLEMS[2][1:]]
    index = [10 ** 6 + 3 * b for b in range(B)]
    params = eng.sample_step_params(index, [groups[b % 2][0] for b in range(B)], [groups[b % 2][1] for b in range(B)],
                                    [5 + b % 2 for b in range(B)], [0] * B)
    logits = torch.from_numpy(z).cuda()[None, None].repeat(B, L, 1).contiguous()
    x = torch.full((B, L), D.MASK, dtype=torch.int64, device="cuda")
    ids = eng.ddpm_step_rows(x, logits, params, seed=D.DDPM_SEED).cpu().numpy()
    del logits
    for g, (mc_t, mc_s) in enumerate(groups):
        q = D.ddpm_probs(z, mc_t, mc_s)
        part = ids[g::2]
        c, dof, p = D.chi_square(part, q)
        zm = D.binomial_z(int((part == D.MASK).sum()), part.size, q[D.MASK])
        zl = D.coincidence_z(*D.neighbour_pairs(part, 1), q)
        print(f"MEASURED sampler distribution device ddpm_step_rows ({mc_t}, {mc_s}) N={part.size}: chi2 {c:.1f} / {dof} p {p:.3g}; MASK "
              f"fraction z {zm:.2f}; coincidence z l|l+1 {zl:.2f}")
        assert p >= D.P_BAR and abs(zm) <= D.Z_BAR and abs(zl) <= D.Z_BAR


# ---- gibbs ------------------------------------------------------------------------------------------------------------------------
def _gibbs_device(eng, name, calls=1):
    """ids [calls * 64, 256] of the interior positions: every one masked, n_unmask = L, `calls` steps at advancing sample offsets."""
    scale, T, top_p, vocab, heavy, invalid = D.GIBBS_PROBLEMS[name]
    z = D.logit_row(scale, 50, heavy)
    x0, seq = D.gibbs_tokens(B_ENG, D.GIBBS_L)
    logits = torch.from_numpy(z).cuda()[None, None].repeat(B_ENG, D.GIBBS_L, 1).contiguous()
    seq_d, nu = torch.from_numpy(seq).cuda(), torch.full((B_ENG,), D.GIBBS_L, dtype=torch.int32)
    out = []
    eng.set_gibbs_options(invalid_ids=invalid)
    try:
        for c in range(calls):
            x = torch.from_numpy(x0).cuda()
            out.append(eng.gibbs_step(x, seq_d, logits, T, top_p, nu, seed=D.GIBBS_SEED, sample_offset=D.GIBBS_OFFSET + B_ENG * c,
                                      step=D.GIBBS_STEP))
        x = torch.cat(out).cpu().numpy()
    finally:
        eng.set_gibbs_options()
    assert (x[:, 0] == 4098).all() and (x[:, -1] == 4097).all()
    return x[:, 1:-1]


@pytest.mark.parametrize("name", list(D.GIBBS_PROBLEMS))
def test_gibbs_goodness_of_fit(engines, name):
    scale, T, top_p, vocab, heavy, invalid = D.GIBBS_PROBLEMS[name]
    z = D.logit_row(scale, 50, heavy)
    assert D.cut_has_no_tie(z, vocab, top_p)
    kept, margin = D.gibbs_kept(z, vocab, top_p, invalid)
    assert margin > 1e-5
    p = D.gibbs_probs(z, vocab, T, top_p, invalid)
    ids = _gibbs_device(engines(vocab), name)
    assert np.isin(ids, kept).all()                       # nothing outside the kept set
    if T == 0.0:
        assert (ids == kept[np.argmax(z[kept])]).all()
        return
    c, dof, pv = D.chi_square(ids, p)
    zl = D.coincidence_z(*D.neighbour_pairs(ids, 1), p)
    print(f"MEASURED sampler distribution device gibbs {name} N={ids.size}: kept {kept.size}, chi2 {c:.1f} / {dof} p {pv:.3g}; "
          f"coincidence z l|l+1 {zl:.2f}")
    assert pv >= D.P_BAR and abs(zl) <= D.Z_BAR


def test_gibbs_at_full_power_and_planted_temperature(engines):
    """N = 2^20 ids of "T1.4 p0.9" (64 steps at advancing sample offsets: 16 384 ids cannot tell a temperature off by 5 %): the
    float64 probabilities pass, the same probabilities at 1.05 T give p < 1e-8."""
    name = "T1.4 p0.9"
    scale, T, top_p, vocab, heavy, invalid = D.GIBBS_PROBLEMS[name]
    z = D.logit_row(scale, 50)
    ids = _gibbs_device(engines(vocab), name, calls=64)
    assert ids.size == 1 << 20
    c, dof, pv = D.chi_square(ids, D.gibbs_probs(z, vocab, T, top_p))
    zb = D.coincidence_z(*D.neighbour_pairs(ids, 0), D.gibbs_probs(z, vocab, T, top_p))
    wrong = D.chi_square(ids, D.gibbs_probs(z, vocab, T * 1.05, top_p))[2]
    print(f"MEASURED sampler distribution device gibbs {name} N={ids.size}: chi2 {c:.1f} / {dof} p {pv:.3g}; coincidence z "
          f"sample|sample+1 {zb:.2f}; planted 1.05 T p {wrong:.3g}")
    assert pv >= D.P_BAR and abs(zb) <= D.Z_BAR
    assert wrong < 1e-8


def test_gibbs_random_strategy_picks_a_uniform_subset(engines):
    """4096 prompts of L = 34 (32 eligible positions), k = 5, in 64 steps of 64 prompts."""
    eng = engines(4101)
    L, k = D.RANDOM_L, D.RANDOM_K
    x0, seq = D.gibbs_tokens(B_ENG, L)
    logits = torch.from_numpy(D.logit_row(1.0, 60)).cuda()[None, None].repeat(B_ENG, L, 1).contiguous()
    seq_d, nu = torch.from_numpy(seq).cuda(), torch.full((B_ENG,), k, dtype=torch.int32)
    out = []
    eng.set_gibbs_options(strategy="random")
    try:
        for c in range(D.RANDOM_PROMPTS // B_ENG):
            out.append(eng.gibbs_step(torch.from_numpy(x0).cuda(), seq_d, logits, 1.0, 1.0, nu, seed=D.RANDOM_SEED,
                                      sample_offset=B_ENG * c, step=1))
        x = torch.cat(out).cpu().numpy()
    finally:
        eng.set_gibbs_options()
    exact, p, z = random_subset_statistics(x)
    print(f"MEASURED sampler distribution device gibbs random {x.shape[0]} prompts: positions chi2 p {p:.3g}; coincidence z i|i+1 {z:.2f}")
    assert exact and p >= D.P_BAR and abs(z) <= D.Z_BAR
    # the first 512 prompts are the CPU twin's
    want = D.oracle_gibbs(D.logit_row(1.0, 60), 64, L, 4101, 1.0, 1.0, (), D.RANDOM_SEED, 0, 1, k=k, strategy="random")
    assert np.array_equal(x[:64], want)


# ---- q_xt -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chance", D.QXT_CHANCES)
def test_q_xt_masks_with_the_stated_probability(engines, chance):
    """2^20 positions in 64 calls of (64, 256); then one call with lengths: no padded position is ever masked."""
    eng = engines(4101)
    B, L = B_ENG, 256
    x0 = torch.randint(0, 4096, (B, L), generator=torch.Generator().manual_seed(1)).cuda()
    out = []
    for c in range((1 << 20) // (B * L)):
        xt, _ = eng.q_xt(x0, [chance] * B, seed=D.QXT_SEED, sample_index=list(range(100 + B * c, 100 + B * (c + 1))),
                         draw=[b % 3 for b in range(B)])
        out.append(xt)
    xt = torch.cat(out)
    assert bool(((xt == D.MASK) | (xt == x0.repeat(len(out), 1))).all())
    moved = (xt == D.MASK).cpu().numpy()
    zf = D.binomial_z(int(moved.sum()), moved.size, float(np.float32(chance)))
    zc = D.coincidence_z(*D.neighbour_pairs(moved.astype(np.int64), 1), [chance, 1 - chance])
    zb = D.coincidence_z(*D.neighbour_pairs(moved.astype(np.int64), 0), [chance, 1 - chance])
    print(f"MEASURED sampler distribution device q_xt {chance} N={moved.size}: masked fraction z {zf:.2f}; coincidence z l|l+1 {zc:.2f}, "
          f"sample|sample+1 {zb:.2f}")
    assert abs(zf) <= D.Z_BAR and abs(zc) <= D.Z_BAR and abs(zb) <= D.Z_BAR
    # the CPU twin's batch: (64 of its 256 samples, L = 64) with lengths
    L2 = 64
    lengths = [L2 - (b % 7) for b in range(B)]
    x2 = x0[:, :L2].contiguous().clone()
    pad = torch.arange(L2)[None] >= torch.tensor(lengths)[:, None]
    x2[pad.cuda()] = 4099
    seq = torch.full((B, L2), 5, dtype=torch.int64)
    seq[:, 0] = 0
    for b in range(B):
        seq[b, lengths[b] - 1] = 2
    seq[pad] = 1
    eng.set_lengths(lengths)
    try:
        xt2, _ = eng.q_xt(x2, [chance] * B, sequence_tokens=seq.cuda(), seed=D.QXT_SEED, sample_index=list(range(100, 100 + B)),
                          draw=[b % 3 for b in range(B)])
    finally:
        eng.set_lengths(None)
    got = (xt2 == D.MASK).cpu().numpy()
    assert not got[pad.numpy()].any()
    want = D.oracle_q_xt(B, L2, chance, D.QXT_SEED, list(range(100, 100 + B)), [b % 3 for b in range(B)], lengths)
    assert np.array_equal(got, want)


# ---- planted: the statistics fail on the device's own draws when they should -------------------------------------------------------
def test_planted_cases_fail_on_the_device_draws(ddpm0):
    scale, mc_t, mc_s = D.DDPM_PROBLEMS[0]
    z = D.logit_row(scale, 0)
    q = D.ddpm_probs(z, mc_t, mc_s)
    wrong = D.ddpm_probs(z, mc_t, mc_s * 1.02)
    p_wrong = D.chi_square(ddpm0, wrong)[2]
    z_wrong = D.binomial_z(int((ddpm0 == D.MASK).sum()), ddpm0.size, wrong[D.MASK])
    again = _ddpm_device(0)                                 # the same (seed, sample, step) requested twice: every uniform shared
    z_same = D.coincidence_z(ddpm0, again, q)
    shifted = _ddpm_device(0, sample_offset=D.DDPM_OFFSET + 1)    # sample b of one is sample b + 1 of the other
    z_shift = D.coincidence_z(ddpm0[1:], shifted[:-1], q)
    print(f"MEASURED sampler distribution device planted: mc_s off by 2 % chi2 p {p_wrong:.3g}, MASK fraction z {z_wrong:.1f}; the same "
          f"counters twice z {z_same:.0f}; offset + 1 against the next sample z {z_shift:.0f}")
    assert p_wrong < 1e-8 and abs(z_wrong) > D.Z_BAR
    assert np.array_equal(ddpm0, again) and abs(z_same) > 10
    assert np.array_equal(ddpm0[1:], shifted[:-1]) and abs(z_shift) > 10

"""Scoring on the device (csrc/score.hip, esmdiff_q_xt / esmdiff_nelbo_rows / esmdiff_nelbo_eval, esmdiff_amd/nelbo.py): the kernels
bit for bit against the CPU restatement (tests/nelbo_ref.py, the C oracle's canonical order), model_step against the oracle
network, batch independence of the estimator, the fused entry against its three parts, the CLI."""
import json

import numpy as np
import pytest
import torch

from tests import nelbo_ref as NR

pytestmark = pytest.mark.gpu
MASK, V = 4096, 4101
# logit tolerance of the existing per-sample-sigma forward test at this model and shape (tests/test_gpu_strict.py::
# test_forward_with_one_sigma_per_sample, TINY seed 4, B = 5, L = 40): 5e-5 float32-grade, 0.05 sixteen-bit
LOGIT_TOL = {"f32": 5e-5, "f32_split": 5e-5, "bf16": 0.05, "f16": 0.05}
_MODELS = {}


def _model(precision, **flags):
    from esmdiff_amd.config import TINY
    from esmdiff_amd.model import MaskedDiffusionLanguageModeling
    from esmdiff_amd.schedule import LogLinearNoise
    from esmdiff_amd.weights import random_init_state_dict
    key = (precision, tuple(sorted(flags.items())))
    if key not in _MODELS:
        _MODELS[key] = MaskedDiffusionLanguageModeling(random_init_state_dict(TINY, seed=4), TINY, LogLinearNoise(), max_batch=40, max_len=64,
                                                       device=0, precision=precision, **flags)
    return _MODELS[key]


def _tokens(B, L, seed):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.randint(0, 4096, (B, L), generator=g)
    x0[:, 0], x0[:, -1] = 4098, 4097
    seq = torch.randint(4, 24, (B, L), generator=g)
    seq[:, 0], seq[:, -1] = 0, 2
    return x0, seq


@pytest.mark.parametrize("ld", [4104, 4352])
@pytest.mark.parametrize("scale", [0.6, 6.0])
def test_nelbo_rows_equals_the_c_oracle_bit_for_bit(ld, scale):
    from esmdiff_amd.config import TINY
    from esmdiff_amd.engine import Engine
    from esmdiff_amd.weights import random_init_state_dict
    B, L = 3, 300                                      # L > 256: the reduction's second lap
    g = torch.Generator().manual_seed(int(ld + scale * 10))
    buf = torch.randn(B, L, ld, generator=g) * scale
    x0 = torch.randint(0, 4096, (B, L), generator=g)
    xt = torch.where(torch.rand(B, L, generator=g) < 0.6, torch.full_like(x0, MASK), x0)
    x0[0, 3], xt[0, 3] = 4099, MASK                    # a special id as the label of a masked row
    x0[1, 5], xt[1, 5] = MASK, MASK                    # the MASK column itself: z - 1e6 - lse
    xt[2, 7] = (x0[2, 7] + 1) % 4096                   # an unmasked row that disagrees with x0: -1e6
    w = -torch.tensor([1.7, 0.01, 930.0])
    lm = torch.rand(B, L, generator=g) < 0.8
    big = Engine(TINY, random_init_state_dict(TINY, seed=4), max_batch=B, max_len=L, precision="f32_split")
    logits = buf.cuda()[..., :V]
    ssum, scnt, lp = big.nelbo_rows(logits, xt, x0, w, loss_mask=lm)
    want_lp = NR.log_p_ref(buf.numpy(), xt.numpy(), x0.numpy())
    assert np.array_equal(lp.cpu().numpy().view(np.int32), want_lp.view(np.int32))
    unm = (xt != MASK).numpy()
    assert set(np.unique(want_lp[unm]).tolist()) == {0.0, -1000000.0} and want_lp[2, 7] == -1000000.0
    want_s, want_c = NR.canonical_sums(want_lp, w.numpy(), lm.numpy())
    assert np.array_equal(ssum.cpu().numpy().view(np.int32), want_s.view(np.int32)) and np.array_equal(scnt.cpu().numpy(), want_c)
    # no loss mask, no log_p output: every position counts, the sums are those of the full mask
    s2, c2, none = big.nelbo_rows(logits, xt, x0, w, return_log_p=False)
    full_s, full_c = NR.canonical_sums(want_lp, w.numpy())
    assert none is None and np.array_equal(s2.cpu().numpy().view(np.int32), full_s.view(np.int32)) and c2.tolist() == [L] * B
    big.close()


def test_q_xt_explicit_philox_lengths_and_coupled():
    eng = _model("f32_split").net
    B, L = 6, 50
    x0, seq = _tokens(B, L, 1)
    g = torch.Generator().manual_seed(2)
    mc = torch.tensor([0.0, 0.2, 0.5, 0.9, 1.0, 0.999])
    u = torch.rand(B, L, generator=g)
    nm = torch.rand(B, L, generator=g) < 0.3
    # explicit uniforms == torch.where (model.py:503-511)
    xt, cs = eng.q_xt(x0, mc, sequence_tokens=seq, coupled=True, non_moving_mask=nm, u=u)
    moved = (u < mc[:, None]) & ~nm
    assert torch.equal(xt.cpu(), torch.where(moved, MASK, x0)) and torch.equal(cs.cpu(), torch.where(moved, 32, seq))
    xt2, cs2 = eng.q_xt(x0, mc, sequence_tokens=seq, u=u)
    assert torch.equal(xt2.cpu(), torch.where(u < mc[:, None], MASK, x0)) and torch.equal(cs2.cpu(), seq)
    assert int((xt2[0] == MASK).sum()) == 0 and int((xt2[4] == MASK).sum()) == L
    # Philox: the host restatement through the C oracle's generator; 64-bit sample indices; draw = the step word
    idx, draw, seed = [5, 2 ** 40 + 3, 0, 77, 5, 9], [0, 3, 1, 2, 1, 0], 1234567890123
    xp, _ = eng.q_xt(x0, mc, seed=seed, sample_index=idx, draw=draw)
    up = NR.philox_mask_uniforms(seed, idx, draw, L)
    assert np.array_equal(xp.cpu().numpy(), NR.q_xt_ref(x0.numpy(), mc.numpy(), up)[0])
    assert 0 < int((xp[2] == MASK).sum()) < L
    # the same (sample index, draw) gives the same row in any batch position
    perm = [3, 0, 5, 1, 4, 2]
    xq, _ = eng.q_xt(x0[perm], mc[perm], seed=seed, sample_index=[idx[i] for i in perm], draw=[draw[i] for i in perm])
    assert torch.equal(xq.cpu(), xp.cpu()[perm])
    one, _ = eng.q_xt(x0[1:2], mc[1:2], seed=seed, sample_index=idx[1:2], draw=draw[1:2])
    assert torch.equal(one.cpu()[0], xp.cpu()[1])
    # lengths: positions from len[b] on keep x0
    lens = [50, 20, 3, 50, 31, 50]
    xr, sr = x0.clone(), seq.clone()
    for b, n in enumerate(lens):
        xr[b, n:], sr[b, n:] = 4099, 1
    eng.set_lengths(lens)
    try:
        xl, _ = eng.q_xt(xr, mc, seed=seed, sample_index=idx, draw=draw)
    finally:
        eng.set_lengths(None)
    assert np.array_equal(xl.cpu().numpy(), NR.q_xt_ref(xr.numpy(), mc.numpy(), up, lengths=lens)[0])
    assert int((xl[4, 31:] == MASK).sum()) == 0 and int((xl[4, :31] == MASK).sum()) > 0
    with pytest.raises(RuntimeError, match="seq"):
        eng._chk(eng._lib.esmdiff_q_xt(eng._h, x0.cuda().data_ptr(), None, mc.cuda().data_ptr(), None, u.cuda().data_ptr(), 0, None, None,
                                       xt.data_ptr(), cs.data_ptr(), B, L, None))


@pytest.mark.parametrize("precision", ["f32", "f32_split", "bf16", "f16"])
def test_model_step_against_the_oracle_network(precision):
    """model_step(noise="torch-cpu") on the TINY engine against oracle/esm3_ref.py + tests/nelbo_ref.py on the same draws: xt
    identical; per row |dlog_p| <= 2 x the logit tolerance (log_p = z - lse moves by at most twice the largest logit error); the
    scalar within that bound times the mean weight of the counted masked rows."""
    from esmdiff_amd import nelbo as NL
    from esmdiff_amd.config import TINY
    from esmdiff_amd.weights import random_init_state_dict
    from oracle.esm3_ref import build_from_state_dict
    net, emb = build_from_state_dict(TINY, random_init_state_dict(TINY, seed=4))
    tol = 2 * LOGIT_TOL[precision]
    for flags, seed in (({}, 21), ({"coupled_condition_mask": True, "T": 10}, 22), ({"importance_sampling": True}, 23)):
        m = _model(precision, **flags)
        B, L = 5, 40
        x0, seq = _tokens(B, L, seed)
        mask = torch.ones(B, L, dtype=torch.int64)
        mask[:, 0] = mask[:, -1] = 0
        nm = torch.zeros(B, L, dtype=torch.bool)
        nm[:, 10:14] = True
        batch = {"structure_tokens": x0, "sequence_tokens": seq, "mask": mask, "non_moving_mask": nm}
        m.reset_parity_stream(seed)
        loss, bd = m.model_step(batch, training=False, noise="torch-cpu", seed=seed)
        last = m.last_model_step
        gen = torch.Generator().manual_seed(seed)
        u_t, u_mask = torch.rand(B, generator=gen), torch.rand(B, L, generator=gen)
        sc = NL.step_scalars(m, NL.sample_t(m, B, u_t))
        xt, cs = NR.q_xt_ref(x0.numpy(), sc["move_chance"].numpy(), u_mask.numpy(), nm.numpy(), None, seq.numpy(), m.coupled_condition_mask)
        assert np.array_equal(last["xt"].cpu().numpy(), xt) and np.array_equal(last["condition_seq"].cpu().numpy(), cs)
        assert 0 < int((xt == MASK).sum()) < B * L and int((xt[:, 10:14] == MASK).sum()) == 0
        with torch.no_grad():
            cond = emb(sc["conditioning"])[:, None, :].expand(B, L, -1)
            ref = net(structure_tokens=torch.from_numpy(xt), sequence_tokens=torch.from_numpy(cs), auxiliary_embeddings=cond).structure_logits
        want_lp = NR.log_p_ref(ref.numpy(), xt, x0.numpy())
        got_lp = last["log_p_theta"].cpu().numpy()
        masked = xt == MASK
        assert np.array_equal(got_lp[~masked], want_lp[~masked])
        d_lp = float(np.abs(got_lp[masked] - want_lp[masked]).max())
        lm = mask.numpy() != 0
        want_s, want_c = NR.canonical_sums(want_lp, sc["weight"].numpy(), lm)
        want = float(want_s.astype(np.float64).sum() / want_c.sum())
        bar = tol * float((np.abs(sc["weight"].numpy())[:, None] * (masked & lm)).sum() / lm.sum())
        print(f"{precision} {flags}: max |dlog_p| {d_lp:.3g} (bar {tol:.3g}); nelbo {float(loss):.6f} vs {want:.6f}, off {abs(float(loss) - want):.3g} (bar {bar:.3g})")
        assert d_lp <= tol, (precision, flags, d_lp)
        assert abs(float(loss) - want) <= bar, (precision, flags, float(loss), want, bar)
        assert float(bd["nelbo"]) == float(loss) and loss.dtype == torch.float64
    with pytest.raises(NotImplementedError):
        m.model_step(batch, training=True)


def test_nelbo_is_batch_independent_on_f32_split_and_eval_equals_its_parts():
    from esmdiff_amd import nelbo as NL
    from esmdiff_amd.schedule import timestep_embedding
    m = _model("f32_split")
    L, K, seed = 40, 3, 9
    x0, seq = _tokens(8, L, 5)
    idx = [11, 3, 2 ** 35, 8, 1, 0, 99, 4]
    alone, se1, lp1 = m.nelbo(x0[2:3], seq[2:3], num_draws=K, seed=seed, sample_index=idx[2:3], return_log_p=True)
    full, se8, lp8 = m.nelbo(x0, seq, num_draws=K, seed=seed, sample_index=idx, return_log_p=True)
    small, _ = m.nelbo(x0, seq, num_draws=K, seed=seed, sample_index=idx, max_batch=5)
    assert float(full[2]) == float(alone[0]) and float(se8[2]) == float(se1[0]) and torch.equal(lp8[2], lp1[0])
    assert torch.equal(full, small) and bool((full > 0).all()) and len(set(full.tolist())) == 8
    # ragged pack: the structure cut to 25 tokens, alone at L = 25 and among longer ones
    xs, ss = x0.clone(), seq.clone()
    xs[2, 24], ss[2, 24] = 4097, 2
    xs[2, 25:], ss[2, 25:] = 4099, 1
    r1, _, rl1 = m.nelbo(xs[2:3, :25], ss[2:3, :25], num_draws=K, seed=seed, sample_index=idx[2:3], return_log_p=True)
    r3, _, rl3 = m.nelbo(xs[[0, 2, 5]], ss[[0, 2, 5]], num_draws=K, seed=seed, sample_index=[idx[0], idx[2], idx[5]], lengths=[L, 25, L],
                         return_log_p=True)
    assert float(r3[1]) == float(r1[0]) and torch.equal(rl3[1, :25], rl1[0]) and float(r3[0]) == float(full[0])
    # esmdiff_nelbo_eval == esmdiff_q_xt + esmdiff_forward_logits_sigmas + esmdiff_nelbo_rows, bit for bit
    eng = m.net
    B = 6
    sc = NL.step_scalars(m, NL.sample_t(m, B, torch.linspace(0.05, 0.95, B)))
    tf = timestep_embedding(sc["conditioning"], m.cfg.freq_dim)
    lm = torch.ones(B, L, dtype=torch.bool)
    lm[:, 0] = False
    nm = torch.zeros(B, L, dtype=torch.bool)
    nm[:, 5:9] = True
    for coupled in (False, True):
        kw = dict(seed=seed, sample_index=idx[:B], draw=[0, 1, 2, 0, 1, 2])
        s_e, c_e, lp_e = eng.nelbo_eval(seq[:B], x0[:B], tf, sc["move_chance"], sc["weight"], non_moving_mask=nm, loss_mask=lm, coupled=coupled,
                                        return_log_p=True, **kw)
        xt, cs = eng.q_xt(x0[:B], sc["move_chance"], sequence_tokens=seq[:B], coupled=coupled, non_moving_mask=nm, **kw)
        logits = eng.forward_logits(xt, cs, tf)
        s_p, c_p, lp_p = eng.nelbo_rows(logits, xt, x0[:B], sc["weight"], loss_mask=lm)
        assert torch.equal(s_e, s_p) and torch.equal(c_e, c_p) and torch.equal(lp_e, lp_p), coupled
        assert c_e.tolist() == [L - 1] * B and bool((s_e >= 0).all()) and int((s_e > 0).sum()) >= B - 1   # (the earliest time may mask nothing)
    # errors follow the conventions: a negative status with text
    with pytest.raises(RuntimeError, match="capacity"):
        eng.nelbo_eval(seq[:1].repeat(41, 1), x0[:1].repeat(41, 1), None, [0.5] * 41, [-1.0] * 41, seed=0, sample_index=list(range(41)))
    with pytest.raises(ValueError, match="uniforms"):
        eng.nelbo_eval(seq[:B], x0[:B], tf, sc["move_chance"], sc["weight"])


def test_score_cli_end_to_end(tmp_path):
    """sample 4 structures with sample_esmdiff --random_init --tiny, score them with score_esmdiff, compare the json with model.nelbo."""
    from esmdiff_amd import sample_esmdiff, score_esmdiff
    from esmdiff_amd.config import TINY
    from esmdiff_amd.model import random_init_model
    from esmdiff_amd.pdbio import write_backbone_pdb
    seq = "RPDFCLEPPYTGPCKARIIRYFYNAKAGLC"
    d = tmp_path / "targets"
    d.mkdir()
    xyz = np.cumsum(np.random.default_rng(0).normal(size=(len(seq), 3, 3)) * 1.5, axis=0)
    write_backbone_pdb(d / "toy.pdb", seq, xyz)
    sample_esmdiff.main(["--input", str(d), "--random_init", "--tiny", "--mode", "ddpm", "--num_samples", "4", "--num_steps", "5", "--seed", "1",
                         "--no_timestamp", "--precision", "f32_split", "--output", str(tmp_path / "s")])
    tok = next((tmp_path / "s").rglob("toy.tokens.npy"))
    assert np.load(tok).shape == (4, len(seq))
    score_esmdiff.main(["--input", str(d), "--tokens", str(tok.parent), "--random_init", "--tiny", "--num_draws", "6", "--seed", "1",
                        "--output", str(tmp_path / "n")])
    rec = json.loads((tmp_path / "n" / "toy.nelbo.json").read_text())
    assert rec["num_draws"] == 6 and rec["seed"] == 1 and rec["precision"] == "f32_split" and "abi=8" in rec["build_info"]
    model = random_init_model(TINY, seed=1, max_batch=7, max_len=len(seq) + 2, precision="f32_split")
    want, se = score_esmdiff.score_target(model, seq, np.load(tok), 6, 1)
    assert rec["nelbo"] == [float(v) for v in want] and rec["stderr"] == [float(v) for v in se]
    assert rec["ranking"] == sorted(range(4), key=lambda i: rec["nelbo"][i]) and len(rec["nelbo"]) == 4
    assert all(np.isfinite(rec["nelbo"])) and all(v > 0 for v in rec["nelbo"])


def test_nelbo_rows_is_not_slower_than_the_existing_ddpm_step():
    """100 x 258 all-MASK rows on the same logits, HIP events in one process, alternating windows, medians
    (tools/measure_nelbo.py::measure_kernels): the scoring kernels read the bytes ddpm_step_kernel reads and do less arithmetic
    (no Philox per element, no divide), so they must not take longer than that existing step."""
    import importlib.util
    from pathlib import Path
    spec = importlib.util.spec_from_file_location("measure_nelbo", Path(__file__).resolve().parent.parent / "tools" / "measure_nelbo.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    r = mod.measure_kernels(100, 258)
    print(json.dumps(r))
    assert r["nelbo_rows_ms"] <= r["ddpm_step_ms"], r

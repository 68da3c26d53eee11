"""CPU: the oracle (torch restatement + C canonical-order restatement) against the golden vectors that
tests/golden/make_goldens.py produced by running the REFERENCE's own sampler code."""
import json
import os
import tempfile
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import c_oracle
from oracle import sampler_ref as R
from tests.recorded_math import recorded_math
from tests.standin_net import StandinNet, standin_sigma_embedder_state

torch.set_num_threads(1)


def _ulp_diff(a, b):
    a = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


@recorded_math
def test_g1_schedules(golden_dir):
    g = np.load(golden_dir / "g1_schedules.npz")
    for T in (5, 25, 50):
        for nm, noise in (("loglinear", R.LogLinearNoiseRef()), ("cosine", R.CosineNoiseRef(1e-3))):
            s = R.ddpm_schedule_ref(T, 1e-5, 1.0, noise)
            assert np.array_equal(s["timesteps"].numpy(), g[f"timesteps_T{T}"])
            assert s["dt"] == float(g[f"dt_T{T}"])
            for k in ("sigma_t", "sigma_s", "mc_t", "mc_s"):
                assert np.array_equal(s[k].numpy(), g[f"{nm}_{k}_T{T}"]), (nm, k, T)
            ds = noise(s["timesteps"][:, None])[1].squeeze(-1).numpy()
            assert np.array_equal(ds, g[f"{nm}_dsigma_t_T{T}"])
    # D.2 spot values
    assert abs(float(g["loglinear_sigma_t_T25"][0]) - 6.90776825) < 1e-5
    assert abs(float(g["loglinear_mc_t_T25"][1]) - 0.95904040) < 1e-6


@recorded_math
def test_g1b_other_schedules(golden_dir):
    """The schedules `get_noise` can also build (noise_utils.py:75-90, :138-185), recorded from the reference at the sampler's
    T = 25 grid: oracle restatement and the product classes, bit for bit."""
    from esmdiff_amd import schedule as S
    g = np.load(golden_dir / "g1b_schedules_other.npz")
    T, eps = 25, 1e-5
    for nm, ref, prod in (("cosinesqr", R.CosineSqrNoiseRef(1e-3), S.get_noise("cosinesqr")),
                          ("linear", R.LinearNoiseRef(0, 10), S.get_noise("linear", 0, 10)),
                          ("geometric", R.GeometricNoiseRef(1e-3, 1), S.get_noise("geometric", 1e-3, 1))):
        s = R.ddpm_schedule_ref(T, eps, 1.0, ref)
        for k in ("sigma_t", "sigma_s", "mc_t", "mc_s"):
            assert np.array_equal(s[k].numpy(), g[f"{nm}_{k}"]), (nm, k)
        t = s["timesteps"][:, None]
        assert np.array_equal((ref(t)[1] * torch.ones_like(t)).squeeze(-1).numpy(), g[f"{nm}_dsigma_t"]), nm
        p = S.ddpm_schedule(T, eps, 1.0, prod)
        for k in ("sigma_t", "mc_t", "mc_s"):
            assert np.array_equal(getattr(p, k).numpy(), g[f"{nm}_{k}"]), (nm, k)
        assert np.array_equal((prod(t)[1] * torch.ones_like(t)).squeeze(-1).numpy(), g[f"{nm}_dsigma_t"]), nm
    grid = torch.from_numpy(g["t_grid"])
    assert np.array_equal(R.LinearNoiseRef(1e-3, 10).importance_sampling_transformation(grid).numpy(), g["linear_importance"])
    assert np.array_equal(S.Linear(1e-3, 10).importance_sampling_transformation(grid).numpy(), g["linear_importance"])
    assert float(np.abs(g["linear_importance"]).max()) > 0.5                      # (a live case, not the degenerate one below)
    # sigma_min = 0 (log1p(-1) = -inf inside): the reference returns zeros and a nan; so do the restatements
    assert np.array_equal(S.Linear(0, 10).importance_sampling_transformation(grid).numpy(), g["linear_importance_sigma_min0"],
                          equal_nan=True)
    assert np.array_equal(R.loglinear_importance_sampling_ref(grid).numpy(), g["loglinear_importance"])
    assert np.array_equal(S.LogLinearNoise().importance_sampling_transformation(grid).numpy(), g["loglinear_importance"])
    g1 = np.load(golden_dir / "g1_schedules.npz")
    assert np.array_equal(S.LogLinearNoise().sigma_max.numpy(), g1["loglinear_sigma_max"])
    assert np.array_equal(S.LogLinearNoise().sigma_min.numpy(), g1["loglinear_sigma_min"])
    assert isinstance(S.get_noise("loglinear"), S.LogLinearNoise) and isinstance(S.get_noise("cosine"), S.CosineNoise)
    with pytest.raises(ValueError, match="not a valid noise"):
        S.get_noise("sigmoid")


@recorded_math
def test_g2_timestep_embedding(golden_dir):
    g = np.load(golden_dir / "g2_timestep.npz")
    sig = torch.from_numpy(g["sigma"])
    assert np.array_equal(R.timestep_embedding_ref(sig, 256).numpy(), g["freq_embedding_256"])
    assert np.array_equal(R.timestep_embedding_ref(sig, 7).numpy(), g["freq_embedding_7"])
    for h in (32, 64):
        emb = R.TimestepEmbedderRef(h)
        emb.load_state_dict(standin_sigma_embedder_state(h))
        with torch.no_grad():
            out = emb(sig).numpy()
        np.testing.assert_allclose(out, g[f"mlp_out_h{h}"], rtol=0, atol=2e-6)


def test_g3_logits_parameterization(golden_dir):
    g = np.load(golden_dir / "g3_logits_param.npz")
    lp = R.logits_parameterization_ref(torch.from_numpy(g["logits"]), torch.from_numpy(g["xt"])).numpy()
    assert np.array_equal(lp, g["log_p"])
    # C oracle: canonical reduction order -> within a few ulp of torch's logsumexp
    lpc = c_oracle.logits_parameterization(g["logits"], g["xt"])
    masked = g["xt"] == R.MASK
    assert np.array_equal(lpc[~masked], g["log_p"][~masked])
    fin = g["log_p"][masked] > -1e5
    np.testing.assert_allclose(lpc[masked][fin], g["log_p"][masked][fin], rtol=0, atol=4e-6)
    assert (lpc[masked][~fin] < -9e5).all()


def test_g4_sample_categorical(golden_dir):
    g = np.load(golden_dir / "g4_categorical.npz")
    probs = torch.from_numpy(g["probs"])
    torch.manual_seed(int(g["seed"]))
    ids = R.sample_categorical_ref(probs)            # draws its own uniforms like model.py:27
    assert np.array_equal(ids.numpy(), g["ids"])
    ids_u = R.sample_categorical_ref(probs, torch.from_numpy(g["u"]))
    assert np.array_equal(ids_u.numpy(), g["ids"])
    torch.manual_seed(int(g["seed"]))
    assert np.array_equal(torch.rand(*probs.shape).numpy(), g["u"])   # D.3: shape-independent MT stream


def _model(hidden=32):
    emb = R.TimestepEmbedderRef(hidden)
    emb.load_state_dict(standin_sigma_embedder_state(hidden))
    return R.MDLMSamplerRef(StandinNet(hidden), emb, R.LogLinearNoiseRef(), True, True)


def test_g5_ddpm_update(golden_dir):
    g = np.load(golden_dir / "g5_ddpm_update.npz")
    m = _model()
    x = torch.from_numpy(g["x"])
    seq = torch.from_numpy(g["seq"])
    t = torch.from_numpy(g["t"])
    with torch.no_grad():
        torch.manual_seed(int(g["seed"]))
        new, logp = m.ddpm_update(x.clone(), t, seq, float(g["dt"]), return_logp=True)
    np.testing.assert_allclose(logp.numpy(), g["log_p"], rtol=0, atol=4e-6)
    assert np.array_equal(new.numpy(), g["x_new"])
    # C oracle on the RAW logits of the stand-in net + the recorded uniforms -> identical ids
    with torch.no_grad():
        sigma_t = m.noise(t)[0].squeeze(-1)
        cond = torch.tile(m.sigma_embedder(sigma_t)[:, None, :], (1, x.shape[1], 1))
        raw = m.net(structure_tokens=x, sequence_tokens=seq, auxiliary_embeddings=cond).structure_logits
    s = R.ddpm_schedule_ref(int(g["T"]))
    i = int(g["step"])
    xc = c_oracle.ddpm_step(g["x"], raw.numpy(), s["mc_t"][i].item(), s["mc_s"][i].item(), u=g["u"])
    assert np.array_equal(xc, g["x_new"])


@pytest.mark.parametrize("tag", ["T5_noprior", "T25_noprior", "T25_prior", "T5_prior"])
def test_g6_ddpm_sample(golden_dir, tag):
    g = np.load(golden_dir / "g6_ddpm_sample.npz")
    m = _model()
    seq = torch.from_numpy(g[f"{tag}_seq"])
    prior = torch.from_numpy(g[f"{tag}_prior"]) if f"{tag}_prior" in g else None
    traj = []
    torch.manual_seed(int(g[f"{tag}_seed"]))
    xf = m.ddpm_sample(seq, int(g[f"{tag}_T"]), 1e-5, prior, 1.0, trajectory=traj)
    assert np.array_equal(torch.stack(traj).numpy(), g[f"{tag}_traj"])
    assert np.array_equal(xf.numpy(), g[f"{tag}_final"])


@pytest.mark.parametrize("tag", ["T25_noprior", "T5_prior"])
def test_g6_c_oracle_trajectory(golden_dir, tag):
    """Drive the C oracle step by step with the reference's uniform stream: ids match every step."""
    g = np.load(golden_dir / "g6_ddpm_sample.npz")
    m = _model()
    seq = torch.from_numpy(g[f"{tag}_seq"])
    T = int(g[f"{tag}_T"])
    B, L = seq.shape
    x = g[f"{tag}_prior"].copy() if f"{tag}_prior" in g else np.full((B, L), R.MASK, np.int64)
    s = R.ddpm_schedule_ref(T)
    torch.manual_seed(int(g[f"{tag}_seed"]))
    with torch.no_grad():
        for i in range(T + 1):
            sig = s["sigma_t"][i] * torch.ones(B)
            cond = torch.tile(m.sigma_embedder(sig)[:, None, :], (1, L, 1))
            raw = m.net(structure_tokens=torch.from_numpy(x), sequence_tokens=seq,
                        auxiliary_embeddings=cond).structure_logits.numpy()
            if i < T:
                u = torch.rand(B, L, R.VOCAB).numpy()
                x = c_oracle.ddpm_step(x, raw, s["mc_t"][i].item(), s["mc_s"][i].item(), u=u)
                assert np.array_equal(x, g[f"{tag}_traj"][i]), i
            else:
                x = c_oracle.ddpm_step(x, raw, 0.0, 0.0, final=True)
    assert np.array_equal(x, g[f"{tag}_final"])


def test_g7_batch_split(golden_dir):
    cases = json.loads((golden_dir / "g7_batch_split.json").read_text())
    for key, want in cases.items():
        L, N = (int(v) for v in key.split(","))
        assert R.batch_split_ref(L, N) == want
    assert R.batch_split_ref(258, 100) == [63, 37] and R.batch_split_ref(1026, 32) == [3] * 8 + [8]


def test_g8_merge_pdbfiles(golden_dir):
    g = json.loads((golden_dir / "g8_merge_pdb.json").read_text())
    with tempfile.TemporaryDirectory() as d:
        pa, pb, pm = Path(d) / "a.pdb", Path(d) / "b.pdb", Path(d) / "m.pdb"
        pa.write_text(g["a"])
        pb.write_text(g["b"])
        R.merge_pdbfiles_ref([pa, pb], pm)
        assert pm.read_text() == g["merged"]


def test_shared_math_accuracy():
    """ed_math.h exp/log vs float64 libm: <= 2 ulp over the ranges the sampler uses."""
    rs = np.random.RandomState(0)
    x = np.concatenate([rs.uniform(-87, 0, 200000), rs.uniform(-1e-3, 1e-3, 1000), [0.0, -103.0, -1e6, 88.0]])
    x = x.astype(np.float32)
    got = c_oracle.expf(x)
    want = np.exp(x.astype(np.float64)).astype(np.float32)
    normal = want > 1.2e-38
    assert _ulp_diff(got[normal], want[normal]).max() <= 2
    assert got[-2] == 0.0 and got[-4] == 1.0
    y = np.concatenate([rs.uniform(1e-10, 1.0, 200000), rs.uniform(1, 5000, 100000),
                        [1.0, 1e-10, 2.0 ** -24 + 1e-10]]).astype(np.float32)
    gl = c_oracle.logf(y)
    wl = np.log(y.astype(np.float64))
    err = np.abs(gl.astype(np.float64) - wl)
    ulp = np.maximum(np.spacing(np.abs(wl).astype(np.float32)), 1e-45)
    assert (err / np.maximum(ulp, 2.0 ** -24 * 1e-1)).max() <= 2.5 or (err <= 1.2e-7).all()
    assert gl[-3] == 0.0


def test_philox_known_answer():
    """Random123 known-answer vectors for Philox4x32-10."""
    assert c_oracle.philox([0, 0, 0, 0], [0, 0]) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert c_oracle.philox([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6,
                                                                   0x6D5451FD]
    assert c_oracle.philox([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0]) == [
        0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]
    u = c_oracle.philox_uniforms(7, 3, 2, 5)
    assert u.min() >= 0.0 and u.max() < 1.0 and abs(u.mean() - 0.5) < 0.02


def test_g10_rmsd_after_alignment(golden_dir):
    """oracle.geom_ref.squared_deviation / find_rigid_alignment vs the reference's geo_utils.py:58-122 (the RMSD the decode
    bar is stated in): fixture made by the reference's own functions."""
    from oracle.geom_ref import backbone_rmsd, find_rigid_alignment, squared_deviation
    g = np.load(golden_dir / "g10_rmsd.npz")
    src, tgt = torch.as_tensor(g["src"]), torch.as_tensor(g["tgt"])
    rmsd = squared_deviation(src, tgt, reduction="rmsd").numpy()
    sd = squared_deviation(src, tgt).numpy()
    # torch.svd (the reference) and torch.linalg.svd may differ in the last bits; the noise-free pair is ~1e-14 either way
    np.testing.assert_allclose(rmsd[1:], g["rmsd"][1:], rtol=1e-9)
    assert rmsd[0] < 1e-12 and g["rmsd"][0] < 1e-12
    np.testing.assert_allclose(sd[1:], g["sd"][1:], rtol=1e-7, atol=1e-18)
    np.testing.assert_allclose(g["rmsd_np_entry"], g["rmsd"], rtol=0, atol=0)
    R, t = find_rigid_alignment(src, tgt)
    np.testing.assert_allclose(R.numpy(), g["R"], atol=1e-12)
    np.testing.assert_allclose(t.numpy(), g["t"], atol=1e-10)
    # the backbone wrapper is the same function over the flattened atoms
    bb = torch.as_tensor(g["src"]).reshape(5, 16, 3, 3)
    bt = torch.as_tensor(g["tgt"]).reshape(5, 16, 3, 3)
    np.testing.assert_allclose(backbone_rmsd(bb, bt).numpy()[1:], g["rmsd"][1:], rtol=1e-9)


def test_g11_rotary_convention_vs_hf_esm(golden_dir):
    """The oracle network's rotary (oracle/esm3_ref.py::MultiHeadAttentionRef._rope, rotate_half) against Hugging Face's port of
    the ESM family's rotary (transformers modeling_esm.apply_rotary_pos_emb; fixture by tests/golden/make_goldens_hf.py): the
    rotate-half pairing (d with d + 32), the sign, inv_freq = 10000^(-2i/64), positions from 0.  Pins the convention, not esm."""
    from oracle.esm3_ref import MultiHeadAttentionRef, rotate_half
    g = np.load(golden_dir / "g11_hf_conventions.npz")
    q, k = torch.as_tensor(g["q"]), torch.as_tensor(g["k"])               # (B, H, L, 64)
    np.testing.assert_array_equal(rotate_half(q).numpy(), g["rotate_half_q"])
    B, H, L, d = q.shape
    mha = MultiHeadAttentionRef(H * d, H)
    # _rope takes (B, L, H * d) token-major rows and returns (B, L, H, d)
    qr, kr = mha._rope(q.transpose(1, 2).reshape(B, L, H * d), k.transpose(1, 2).reshape(B, L, H * d))
    np.testing.assert_allclose(qr.transpose(1, 2).numpy(), g["q_rot"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(kr.transpose(1, 2).numpy(), g["k_rot"], rtol=0, atol=2e-6)
    # the engine's host-side tables (csrc/engine.hip builds cos / sin of l * 10000^(-2i/64) per position) are the same numbers
    np.testing.assert_allclose(g["cos"][0, :, :32], np.cos(np.arange(L)[:, None] * (1.0 / 10000.0 ** (np.arange(0, 64, 2) / 64.0))[None]),
                               atol=1e-6)


def test_g11_gram_schmidt_frames_vs_openfold(golden_dir):
    """Backbone frames (esmdiff_amd/geometry.py, oracle/geom_ref.py) against OpenFold's Rigid.from_3_points(C, CA, N) as shipped in
    transformers (AlphaFold-2 algorithm 21): first axis CA - C, second in the plane of N, third = first x second (right-handed),
    axes are the COLUMNS of the rotation, origin CA."""
    from esmdiff_amd.geometry import build_affine3d_from_coordinates
    from oracle.geom_ref import frames_from_backbone
    g = np.load(golden_dir / "g11_hf_conventions.npz")
    n, ca, c = (torch.as_tensor(g[k]) for k in ("n", "ca", "c"))
    rot_o, trans_o = frames_from_backbone(n, ca, c)
    np.testing.assert_allclose(rot_o.numpy(), g["rot"], atol=2e-6)
    np.testing.assert_allclose(trans_o.numpy(), g["trans"], atol=0)
    rot, trans, has = build_affine3d_from_coordinates(torch.stack([n, ca, c], dim=-2))
    assert bool(has.all())
    np.testing.assert_allclose(rot.numpy(), g["rot"], atol=2e-6)
    np.testing.assert_allclose(trans.numpy(), g["trans"], atol=0)
    assert np.allclose(np.linalg.det(g["rot"]), 1.0, atol=1e-5)              # proper rotations


# ---------------------------------------------------------------------------------------------------------------------------------
# esm==3.0.4 itself.  tests/golden/esm/*.npz are written by tools/dump_esm_vectors.py on a machine that has
# the package; they pin oracle/esm3_ref.py, decoder_ref.py, encoder_ref.py and gibbs_ref.py to esm's own arithmetic.  Absent
# files skip WITH THE REASON (parity of those parts stays "unpinned"); the harness itself is exercised on
# files the oracle fills in the same format.
@pytest.mark.parametrize("name", ["esm3_stack.npz", "structure_decoder.npz", "structure_encoder.npz", "sampling.npz"])
def test_esm_golden_vectors_pin_the_restatements(name):
    from tests import esm_golden
    path = esm_golden.ESM_DIR / name
    if not path.exists():
        pytest.skip(f"{path.relative_to(esm_golden.ESM_DIR.parent.parent.parent)} absent: esm==3.0.4 is not installable offline — run "
                    "`python tools/dump_esm_vectors.py` where the reference runs and commit the files (README: turning parity green)")
    print(name, esm_golden.CHECKS[name](path))


def test_esm_golden_harness_selfcheck(tmp_path):
    """The consumers of tests/golden/esm/*.npz on files of the same format filled by the oracle itself: every checker loads its
    file, rebuilds the restatement from the state dict inside it and compares — so key names, shapes and tolerance code are known
    to work; a perturbed output must FAIL the check (the comparison is real)."""
    import numpy as np
    from tests import esm_golden
    esm_golden.write_selfcheck_vectors(tmp_path)
    for name, fn in esm_golden.CHECKS.items():
        fn(tmp_path / name)
    z = dict(np.load(tmp_path / "esm3_stack.npz"))
    z["out::structure_logits"] = z["out::structure_logits"] + 0.01
    np.savez_compressed(tmp_path / "bad.npz", **z)
    with pytest.raises(AssertionError):
        esm_golden.check_esm3_stack(tmp_path / "bad.npz")


# ---- the two oracles against each other, at scale ----------------------------------------------------------
def _torch_update(x, logits, mc_t, mc_s, u):
    """One `_ddpm_update` after the network, in the reference's torch operation order (model.py:527-533, 602-607, 24-28) — the
    restatement that reproduces the goldens made by the reference's own code (oracle/sampler_ref.py)."""
    from oracle.sampler_ref import MASK, logits_parameterization_ref, sample_categorical_ref
    log_p = logits_parameterization_ref(logits, x)
    q = log_p.exp() * (mc_t - mc_s)
    q[:, :, MASK] = mc_s
    drawn = sample_categorical_ref(q, u)
    keep = (x != MASK).to(x.dtype)
    return keep * x + (1 - keep) * drawn


def _equivalence_run(n_trials, rows, seed):
    """C oracle (csrc/ed_math.h exp / log, canonical reduction order — what the HIP kernel equals bit for bit) vs the torch op
    order on `n_trials` batches of (rows/258, 258) rows: five logit scales, four schedule points, explicit uniforms, ~30 % known
    rows.  Returns (masked draws compared, differing ids)."""
    from oracle import c_oracle
    from oracle.sampler_ref import MASK, VOCAB
    g = torch.Generator().manual_seed(seed)
    B, L = rows // 258, 258
    points = [(0.999, 0.95904), (0.5, 0.46004), (0.12, 0.08004), (0.04096, 1e-5)]
    draws = diff = 0
    for trial in range(n_trials):
        scale = [0.1, 0.6, 2.0, 6.0, 20.0][trial % 5]
        mc_t, mc_s = points[trial % 4]
        logits = torch.randn(B, L, VOCAB, generator=g) * scale
        u = torch.rand(B, L, VOCAB, generator=g)
        x = torch.full((B, L), MASK, dtype=torch.int64)
        known = torch.rand(B, L, generator=g) < 0.3
        x[known] = torch.randint(0, 4096, (int(known.sum()),), generator=g)
        want = _torch_update(x, logits, torch.tensor(mc_t), torch.tensor(mc_s), u).numpy()
        got = c_oracle.ddpm_step(x.numpy(), logits.numpy(), mc_t, mc_s, u=u.numpy())
        m = (x == MASK).numpy()
        draws += int(m.sum())
        diff += int((got != want)[m].sum())
        assert np.array_equal(got[~m], x.numpy()[~m])
    return draws, diff


def test_c_oracle_equals_torch_op_order_36k_draws():
    """SURVEY D.1 expected O(1e-6) flips per draw between two float reduction orders; measured: none.  ~36 000 masked draws in
    the default suite; the 1.2-million-draw run is test_c_oracle_equals_torch_op_order_1m_draws (profiles/r06_oracle_equivalence.json)."""
    draws, diff = _equivalence_run(n_trials=10, rows=20 * 258, seed=2024)
    assert draws > 35_000 and diff == 0, (draws, diff)


@pytest.mark.slow
@pytest.mark.skipif(not os.environ.get("ESMDIFF_RUN_SLOW"), reason="several minutes of CPU: ESMDIFF_RUN_SLOW=1; last result in "
                                                                   "profiles/r06_oracle_equivalence.json")
def test_c_oracle_equals_torch_op_order_1m_draws():
    """>= 1 million masked draws (40 x 258 rows x 170 trials x ~70 % masked).  Writes profiles/r06_oracle_equivalence.json."""
    import json
    import time
    t0 = time.time()
    draws, diff = _equivalence_run(n_trials=170, rows=40 * 258, seed=7)
    rec = {"what": "C oracle (oracle/csrc/sampler_oracle.c) vs torch op order of model.py:527-533, 602-607, 24-28 (oracle/sampler_ref.py), "
                   "explicit uniforms, 5 logit scales x 4 schedule points, ~30 % known rows",
           "masked_draws": draws, "differing_ids": diff, "seconds": round(time.time() - t0, 1),
           "flip_rate_upper_bound_95": round(3.0 / draws, 9) if diff == 0 else None}
    out = Path(__file__).resolve().parent.parent / "profiles" / "r06_oracle_equivalence.json"
    out.write_text(json.dumps(rec, indent=1))
    assert draws >= 1_000_000 and diff == 0, rec

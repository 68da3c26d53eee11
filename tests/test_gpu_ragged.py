"""Ragged batches (esmdiff_set_lengths): B samples padded to one L, sample b valid on tokens [0, len[b]).

The contract: a valid position's logits and ids depend only on its own sample's valid positions.  Attention is the only
kernel family where positions interact, so the kernels are checked alone first (bit-identical to each sample launched alone
at its own length, and against float64), then the whole forward (padding content never reaches a valid row; each sample
equals its solo forward), then sampling (packed ddpm with per-row Philox indices, mixed-length iterative_sampling_raw).
TINY engines only (2 blocks of d 512)."""
import pytest
import torch

from esmdiff_amd import constants as C
from tests import rowwise_ref as rr

pytestmark = pytest.mark.gpu

PRECISIONS = ["bf16", "f16", "f32_split", "f32"]
DTYPE = {"bf16": torch.bfloat16, "f16": torch.float16, "f32_split": torch.float32, "f32": torch.float32}
LENS = [3, 60, 64, 65, 97, 128, 129, 258]


@pytest.fixture(scope="module")
def engines():
    from esmdiff_amd.config import TINY
    from esmdiff_amd.engine import Engine
    from esmdiff_amd.weights import random_init_state_dict
    sd = random_init_state_dict(TINY, seed=5, with_geom=True)
    out = {p: Engine(TINY, sd, max_batch=8, max_len=300, precision=p) for p in PRECISIONS}
    yield TINY, sd, out
    for e in out.values():
        e.close()


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_ragged_attention_kernels(engines, precision):
    """Lengths {3, 60, 64, 65, 97, 128, 129, 258} padded to 258 (one tile, partial tiles, exact tiles, the HALF tail,
    whole padded query blocks): valid rows bit-identical to the sample alone at its length, within the float64 bar,
    padded context rows exactly 0 — with garbage in the padded qkv rows."""
    from esmdiff_amd.engine import v_split
    QS32 = float(torch.tensor(rr.QSCALE, dtype=torch.float32))               # log2(e) / 8 as the engine passes it
    cfg, _, engs = engines
    eng, dt = engs[precision], DTYPE[precision]
    D, H, B, L = cfg.d_model, cfg.n_heads, len(LENS), max(LENS)
    g = torch.Generator().manual_seed(7)
    qw, kw = (1 + 0.3 * torch.randn(D, generator=g)).cuda(), (1 + 0.3 * torch.randn(D, generator=g)).cuda()
    qkv = torch.randn(B, L, 3 * D, generator=g)
    for b, n in enumerate(LENS):
        qkv[b, n:] = 50 * torch.randn(L - n, 3 * D, generator=g)          # padding: large garbage that must never matter
    qkv = qkv.to(dt).cuda()
    got = eng.attention_ragged(qkv.reshape(B * L, -1).contiguous(), qw, kw, B, L, lengths=LENS).view(B, L, D)
    worst, worst32 = 0.0, 0.0
    for b, n in enumerate(LENS):
        solo_in = qkv[b, :n].contiguous()
        solo = eng.attention_ragged(solo_in, qw, kw, 1, n)
        assert torch.equal(_bits(got[b, :n]), _bits(solo)), (precision, n)
        assert bool((got[b, n:] == 0).all()), (precision, n)
        ref, unit = rr.attention_ref64(solo_in, qw, kw, 1, n, H, torch.float16 if dt == torch.float16 else torch.bfloat16)
        if dt == torch.float32:
            err = float((solo.double() - ref).abs().max())
            worst = max(worst, err)
            assert err < 1e-4, (precision, n, err)
            # ... and the float32-grade unit bar (an absolute 1e-4 cannot tell 11-bit operands from float32): the attention
            # kernel against float64 attention of the very operands it was handed, which the same q/k and v launchers
            # this entry runs produce again (deterministic kernels)
            if precision == "f32_split":
                q2, k2 = eng.qk_norm_rope_f32(solo_in, qw, kw, 1, n, H, split=True, q_scale=QS32, k_scale=1.0)
                ops = (rr.split_operand_value(q2, 1.0) * rr.LN2_8, rr.split_operand_value(k2, 1.0),
                       rr.split_operand_value(v_split(solo_in, 1.0), 1.0))
            else:
                ops = (*eng.qk_norm_rope_f32(solo_in, qw, kw, 1, n, H), solo_in[:, 2 * D:])
            ref32, unit32 = rr.attention32_ref64(*ops, 1, n, H)
            r32 = float(rr.ratio(solo, ref32, dt, rr.ATT32_COEF * unit32).max())
            worst32 = max(worst32, r32)
            assert r32 <= 1.0, (precision, n, r32)
        else:
            r = float(rr.ratio(solo, ref, dt, rr.ATT_COEF * unit).max())
            worst = max(worst, r)
            assert r <= 1.0, (precision, n, r)
    assert bool(torch.isfinite(got.float()).all())
    print(f"MEASURED ragged attention {precision}: worst {'abs err' if dt == torch.float32 else 'ratio'} {worst:.3g}"
          + (f", ratio to the float32-grade bar {worst32:.3f}" if dt == torch.float32 else ""))


def _batch(lens, L, seed):
    g = torch.Generator().manual_seed(seed)
    B = len(lens)
    seq = torch.full((B, L), C.SEQUENCE_PAD_TOKEN, dtype=torch.int64)
    x = torch.full((B, L), C.STRUCTURE_PAD_TOKEN, dtype=torch.int64)
    for b, n in enumerate(lens):
        seq[b, 0], seq[b, n - 1] = 0, 2
        seq[b, 1:n - 1] = torch.randint(4, 24, (n - 2,), generator=g)
        x[b, 0], x[b, n - 1] = C.STRUCTURE_BOS_TOKEN, C.STRUCTURE_EOS_TOKEN
        x[b, 1:n - 1] = torch.where(torch.rand(n - 2, generator=g) < 0.5, torch.randint(0, 4096, (n - 2,), generator=g),
                                    torch.full((n - 2,), C.STRUCTURE_MASK_TOKEN))
    return seq, x


@pytest.mark.parametrize("precision", PRECISIONS)
def test_ragged_forward_pad_invariance_and_solo(engines, precision):
    """Whole forward with lengths set.  (a) Random tokens in the padded positions (the engine is driven through
    set_lengths directly, which does not look at the padding) leave every valid logit bit-identical, and every logit is finite.
    (b) Each sample against its solo forward: f32 bit for bit; the others within the bf16 forward's bar (batch composition
    moves GEMM kernel choice and the small-batch path).  One batch of 2 400 padded tokens takes the two-stream split."""
    from esmdiff_amd.schedule import ddpm_schedule
    cfg, _, engs = engines
    eng = engs[precision]
    tf = ddpm_schedule(4).t_freq[1]
    for lens, L in (([5, 40, 71, 33], 71), ([300, 120, 64, 200, 299, 3, 150, 250], 300)):
        B = len(lens)
        seq, x = _batch(lens, L, seed=L)
        eng.set_lengths(lens)
        try:
            a = eng.forward_logits(x.cuda(), seq.cuda(), tf).float().cpu().clone()
            g = torch.Generator().manual_seed(1)
            seq2, x2 = seq.clone(), x.clone()
            for b, n in enumerate(lens):
                seq2[b, n:] = torch.randint(0, 33, (L - n,), generator=g)
                x2[b, n:] = torch.randint(0, 4101, (L - n,), generator=g)
            b2 = eng.forward_logits(x2.cuda(), seq2.cuda(), tf).float().cpu().clone()
            if L == 300 and precision in ("bf16", "f16"):
                assert "ragged=1" in eng.describe_plan(B, L) and "streams=2" in eng.describe_plan(B, L)
        finally:
            eng.set_lengths(None)
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b2).all())
        worst = 0.0
        for b, n in enumerate(lens):
            assert torch.equal(a[b, :n], b2[b, :n]), (precision, L, n)
            solo = eng.forward_logits(x[b:b + 1, :n].cuda(), seq[b:b + 1, :n].cuda(), tf).float().cpu()[0]
            if precision == "f32":
                assert torch.equal(a[b, :n], solo), (L, n, float((a[b, :n] - solo).abs().max()))
            else:
                err = (a[b, :n] - solo).abs()
                worst = max(worst, float(err.max()))
                assert float(err.max()) < 0.12 and float(err.mean()) < 1.2e-2, (precision, L, n, float(err.max()))
        print(f"MEASURED ragged forward {precision} B={B} L={L}: max |packed - solo| {worst:.3g}")
    # the contract's refusals: B other than the set B, a length above L, a length below 3
    eng.set_lengths([10, 20])
    try:
        with pytest.raises(RuntimeError, match="lengths were set"):
            eng.forward_logits(x[:3, :20].cuda(), seq[:3, :20].cuda(), tf)
        with pytest.raises(RuntimeError, match="exceeds"):
            eng.forward_logits(x[:2, :15].cuda(), seq[:2, :15].cuda(), tf)
    finally:
        eng.set_lengths(None)
    with pytest.raises(RuntimeError, match="outside"):
        eng.set_lengths([2, 10])
    with pytest.raises(ValueError, match="pad id"):
        eng.forward_logits(x[:2, :20].cuda(), seq[:2, :20].cuda(), tf, lengths=[10, 20])


def test_packed_ddpm_equals_per_target_runs(engines):
    """f32, TINY: three targets of different lengths, two samples each, packed into one ragged batch with Philox sample
    index offset_t + j per row, give id for id what each target's own ddpm_sample gives."""
    from esmdiff_amd.schedule import ddpm_schedule
    _, _, engs = engines
    eng = engs["f32"]
    sch = ddpm_schedule(5)
    lens, per = [24, 41, 57], 2
    L = max(lens)
    seq1, _ = _batch(lens, L, seed=3)
    rows = [(t, j) for t in range(len(lens)) for j in range(per)]
    seq = torch.stack([seq1[t] for t, _ in rows])
    row_lens = [lens[t] for t, _ in rows]
    got = eng.ddpm_sample(seq.cuda(), sch, seed=11, lengths=row_lens, sample_index=[j for _, j in rows]).cpu()
    for r, (t, j) in enumerate(rows):
        n = lens[t]
        solo = eng.ddpm_sample(seq1[t:t + 1, :n].repeat(per, 1).cuda(), sch, seed=11).cpu()
        assert torch.equal(got[r, :n], solo[j]), (t, j)
        assert bool((got[r, n:] == C.STRUCTURE_PAD_TOKEN).all())
    assert int((got == C.STRUCTURE_MASK_TOKEN).sum()) == 0
    # the device loop with lengths (sample index = offset + row) and the exact noise-removal skip: each row is its own run
    eng.set_final_skip(True)
    try:
        dev = eng.ddpm_sample(seq.cuda(), sch, seed=11, sample_offset=4, lengths=row_lens).cpu()
    finally:
        eng.set_final_skip(False)
    for r, (t, _) in enumerate(rows):
        n = lens[t]
        solo = eng.ddpm_sample(seq1[t:t + 1, :n].cuda(), sch, seed=11, sample_offset=4 + r).cpu()
        assert torch.equal(dev[r, :n], solo[0]), r


def test_mixed_length_iterative_sampling_raw(engines):
    """f32, TINY with geometric-attention weights: proteins of different lengths and different step counts T, one of them
    carrying coordinates, in ONE iterative_sampling_raw call — each protein's tokens equal its own call at the same sample
    index, and come back trimmed to its own length."""
    from esmdiff_amd.gibbs import iterative_sampling_raw
    from esmdiff_amd.sdk import ESMProtein, GenerationConfig
    _, _, engs = engines
    eng = engs["f32"]
    g = torch.Generator().manual_seed(9)
    aa = "ACDEFGHIKLMNPQRSTVWY"
    mk = lambda n: "".join(aa[int(i)] for i in torch.randint(0, 20, (n,), generator=g))
    n_xyz = 45
    ca = torch.cumsum(torch.randn(n_xyz, 3, generator=g) * 2.2, 0)
    xyz = torch.stack([ca + torch.randn(n_xyz, 3, generator=g) * 0.8, ca, ca + torch.randn(n_xyz, 3, generator=g) * 0.8], 1)
    known = torch.randint(0, 4096, (70,), generator=g)
    known[10:14] = C.STRUCTURE_MASK_TOKEN                         # 4 masked positions: T = 4 for this protein
    proteins = [ESMProtein(sequence=mk(30)),
                ESMProtein(sequence=mk(n_xyz), coordinates=xyz),
                ESMProtein(sequence=mk(70), structure_tokens=known),
                ESMProtein(sequence=mk(12))]
    cfg = GenerationConfig(num_steps=8, temperature=1.0, top_p=0.9)
    out = iterative_sampling_raw(eng, proteins, [cfg] * len(proteins), seed=5, sample_offset=3)
    for b, p in enumerate(proteins):
        solo = iterative_sampling_raw(eng, [p], [cfg], seed=5, sample_offset=3 + b)[0]
        assert out[b].structure_tokens.shape == (len(p.sequence),)
        assert torch.equal(out[b].structure_tokens, solo.structure_tokens), b
        assert int((out[b].structure_tokens >= 4096).sum()) == 0, b
    assert torch.equal(out[2].structure_tokens[:10], known[:10])


@pytest.mark.parametrize("mode", ["ddpm", "gibbs"])
def test_cli_pack_targets_equals_per_target_run(tmp_path, mode):
    """Four toy PDBs of different lengths, --precision f32: --pack_targets writes the per-target run's .tokens.npy, a .json
    with its "pack" record and a decoded .pdb per target."""
    import json

    import numpy as np

    from esmdiff_amd.pdbio import write_backbone_pdb
    from esmdiff_amd.sample_esmdiff import main
    g = np.random.default_rng(1)
    aa = "ACDEFGHIKLMNPQRSTVWY"
    d = tmp_path / "in"
    d.mkdir()
    for name, n in (("a", 20), ("b", 33), ("c", 27), ("d", 45)):
        ca = np.cumsum(g.normal(size=(n, 3)) * 2.2, 0)
        write_backbone_pdb(d / f"{name}.pdb", "".join(aa[i] for i in g.integers(0, 20, n)),
                           np.stack([ca + g.normal(size=ca.shape) * 0.8, ca, ca + g.normal(size=ca.shape) * 0.8], 1))
    common = ["--random_init", "--tiny", "--input", str(d), "--mode", mode, "--precision", "f32", "--num_samples", "3",
              "--num_steps", "4", "--seed", "2", "--no_timestamp"]
    main(common + ["--output", str(tmp_path / "solo")])
    main(common + ["--output", str(tmp_path / "packed"), "--pack_targets", "--pack_tokens", "200", "--random_init_decoder"])
    sub = "step4_eps1e-05_N3" if mode == "ddpm" else "T1.4_step4_topp0.9_N3"
    packs = set()
    for name, n in (("a", 20), ("b", 33), ("c", 27), ("d", 45)):
        want = np.load(tmp_path / "solo" / sub / f"{name}.tokens.npy")
        got = np.load(tmp_path / "packed" / sub / f"{name}.tokens.npy")
        assert want.shape == (3, n) and np.array_equal(got, want), name
        meta = json.loads((tmp_path / "packed" / sub / f"{name}.json").read_text())
        assert meta["pack"] and all(name in p["targets"] and p["padded_row_share"] <= 0.25 for p in meta["pack"])
        packs |= {p["id"] for p in meta["pack"]}
        text = (tmp_path / "packed" / sub / f"{name}.pdb").read_text().splitlines()
        assert sum(l.startswith("MODEL") for l in text) == 3
    assert len(packs) > 1                                        # the 200-token budget cuts the 12 rows into several packs

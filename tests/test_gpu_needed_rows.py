"""Needed rows (ESMDIFF_OPT_NEEDED_ROWS): esmdiff_ddpm_sample runs the last block's branches and the head only on the rows that
hold MASK, the rows whose logits its sampler reads (csrc/engine_forward.hip: needed_tail).  The option must not change one id
or one logit bit on the rows that are read; it must really shrink the work; and it must keep callers from reading the stale rows.

Production width (d_model 1536: what the GEMM kernels need), two blocks, bf16 and f16.  (24, 258): two launch queues on the
regular path; (9, 258): cut 4 + 5, sub-batches of 1 032 and 1 290 rows; (6, 60): the small-batch path, where the option is inert."""
import pytest
import torch

pytestmark = pytest.mark.gpu

MASK, PAD = 4096, 4099
SHAPES = ((24, 258), (9, 258), (6, 60))
T = 4


def _seq(B, L, g):
    return torch.cat([torch.tensor([0]), torch.randint(4, 24, (L - 2,), generator=g), torch.tensor([2])])[None].repeat(B, 1)


@pytest.fixture(scope="module", params=["bf16", "f16"])
def eng(request):
    from esmdiff_amd.config import ModelConfig
    from esmdiff_amd.engine import Engine
    from esmdiff_amd.weights import random_init_state_dict
    cfg = ModelConfig(n_layers=2)
    e = Engine(cfg, random_init_state_dict(cfg, seed=11), max_batch=24, max_len=258, precision=request.param)
    yield e
    e.close()


def _first_part(B):
    """Samples of the first of the two sub-batches a regular-path forward cuts B into (engine_forward.hip: cut_batch)."""
    return B // 2


def _priors(B, L, g):
    """name -> (B, L) prior.  Unmasked positions hold random structure tokens."""
    tok = torch.randint(0, 4096, (B, L), generator=g)
    out = {"all_mask": torch.full((B, L), MASK, dtype=torch.int64)}
    p = tok.clone()
    p[:, 0::2] = MASK
    out["every_second"] = p
    p = torch.full((B, L), MASK, dtype=torch.int64)
    p[:_first_part(B)] = tok[:_first_part(B)]           # nothing to do on the first queue, everything on the other
    out["first_part_unmasked"] = p
    p = tok.clone()
    p[B - 1, L // 2] = MASK
    out["one_mask"] = p
    for n in (255, 256, 257):                           # the 256-row tile edge: the first sub-batch holds exactly n masked rows
        p = torch.full((B, L), MASK, dtype=torch.int64)
        first = p[:_first_part(B)].reshape(-1)
        first[:] = tok[:_first_part(B)].reshape(-1)
        first[torch.randperm(first.numel(), generator=g)[:n]] = MASK
        out[f"first_part_{n}_masked"] = p
    return out


def _sample(e, seq, sch, prior, on, **kw):
    e.set_needed_rows(on)
    e.counters(reset=True)
    e.tail_rows(reset=True)
    ids = e.ddpm_sample(seq, sch, seed=5, sample_offset=3, input_prior=prior.cuda(), **kw).cpu()
    return ids, e.counters(reset=True), e.tail_rows(reset=True)


def _expected_tail_rows(e, seq, sch, prior, want):
    """The chain once more as a host loop of full forwards and single updates (the same ids: checked), counting before each
    forward what the option lets through: per sub-batch its masked rows when they are at most 7/8 of its rows, else all of them."""
    B, L = prior.shape
    x = prior.clone().cuda()
    tf = e.conditioning_rows(sch.t_freq)
    cut = _first_part(B) * L
    total = 0
    for i in range(T + 1):
        m = (x == MASK).reshape(-1)
        for part in (m[:cut], m[cut:]):
            n = int(part.sum())
            total += n if n * 8 <= part.numel() * 7 else part.numel()
        lg = e.forward_logits(x, seq, None if tf is None else tf[i], check_ids=False)
        fin = i == T
        e.ddpm_step(x, lg, 0.0 if fin else float(sch.mc_t[i]), 0.0 if fin else float(sch.mc_s[i]), final=fin, seed=5,
                    sample_offset=3, step=i)
    assert torch.equal(x.cpu(), want)
    return total


@pytest.mark.parametrize("B,L", SHAPES)
def test_ids_bit_identical_and_work_shrinks(eng, B, L):
    """ddpm_sample with the option on against off: the same ids, the same token_rows; the rows that ran the last block's branches
    are the masked rows of every sub-batch that had at most 7/8 of its rows masked (all rows at step 0 of an all-MASK prior), and
    all rows on the small-batch path."""
    from esmdiff_amd.schedule import ddpm_schedule
    sch = ddpm_schedule(T, eps=0.3)
    g = torch.Generator().manual_seed(B * 1000 + L)
    seq = _seq(B, L, g).cuda()
    small = "small-batch" in eng.describe_plan(B, L)
    assert small == (B * L < 1152)
    assert " needed_rows=1" in eng.describe_plan(B, L)
    for name, prior in _priors(B, L, g).items():
        want, c_off, t_off = _sample(eng, seq, sch, prior, False)
        got, c_on, t_on = _sample(eng, seq, sch, prior, True)
        assert torch.equal(got, want), (B, L, name)
        assert c_on == c_off == {"forwards": T + 1, "token_rows": (T + 1) * B * L}, (name, c_on, c_off)
        assert t_off == (T + 1) * B * L, (name, t_off)
        if small:
            assert t_on == t_off, (name, t_on)          # the option is inert: 0 rows skipped
        else:
            eng.set_needed_rows(False)
            assert t_on == _expected_tail_rows(eng, seq, sch, prior, want), (name, t_on)
            assert t_on < t_off, (name, t_on, t_off)    # (all_mask: step 0 runs every row, the later steps drop the unmasked ones)
    eng.set_needed_rows(True)


@pytest.mark.parametrize("B,L", SHAPES[:2])
def test_ids_bit_identical_shared_step0_with_compact_tail(eng, B, L):
    """N samples inpainted from one structure: every sample starts from the same prior with half of its rows masked, so step-0
    sharing and the compact tail are on in the same forward and the update reads row_map[((row / L) % shared) L + row % L]
    (csrc/sampler.hip).  Needed rows, step-0 sharing and final skip all on against all three off: the same ids."""
    from esmdiff_amd.schedule import ddpm_schedule
    sch = ddpm_schedule(T, eps=0.3)
    g = torch.Generator().manual_seed(B * 1000 + L + 1)
    seq = _seq(B, L, g).cuda()
    prior = _priors(B, L, g)["every_second"][:1].repeat(B, 1)
    try:
        want, c_off, t_off = _sample(eng, seq, sch, prior, False)
        eng.set_step0_sharing(True)
        eng.set_final_skip(True)
        got, c_on, t_on = _sample(eng, seq, sch, prior, True)
    finally:
        eng.set_step0_sharing(False)
        eng.set_final_skip(False)
        eng.set_needed_rows(True)
    assert torch.equal(got, want), (B, L, int((got != want).sum()))
    assert c_off["token_rows"] == t_off == (T + 1) * B * L
    if (B, L) == (24, 258):
        assert eng.shared_forward_batch(B, L) < B
        assert c_on["token_rows"] < (T + 1) * B * L, c_on       # step 0 ran on the shared sub-batch
        assert t_on < c_on["token_rows"], (t_on, c_on)          # and its tail on the masked rows of that sub-batch


def test_ids_bit_identical_ragged(eng):
    """A ragged batch (set_lengths): padding rows hold the pad id, never MASK, and drop out of the row lists by themselves."""
    from esmdiff_amd.schedule import ddpm_schedule
    sch = ddpm_schedule(T, eps=0.3)
    B, L = 9, 258
    lens = [3, 97, 258] * 3
    g = torch.Generator().manual_seed(77)
    seq = _seq(B, L, g)
    prior = torch.full((B, L), MASK, dtype=torch.int64)
    for b, n in enumerate(lens):
        seq[b, n - 1] = 2
        seq[b, n:] = 1
        prior[b, n:] = PAD
    want, _, t_off = _sample(eng, seq.cuda(), sch, prior, False, lengths=lens)
    got, _, t_on = _sample(eng, seq.cuda(), sch, prior, True, lengths=lens)
    assert torch.equal(got, want)
    assert t_on < t_off == (T + 1) * B * L      # the 4 + 5 cut: 361 of 1 032 and 713 of 1 290 rows are valid, both compact at step 0
    eng.set_needed_rows(True)


@pytest.mark.parametrize("B,L", SHAPES[:2])
@pytest.mark.parametrize("case", ["half", "one"])
def test_logits_bit_identical_on_masked_rows(eng, B, L, case):
    """esmdiff_forward_logits_needed against esmdiff_forward_logits: equal bits on the masked rows, the other rows untouched, and
    the counter equal to the number of masked rows."""
    from esmdiff_amd.schedule import ddpm_schedule
    sch = ddpm_schedule(T, eps=0.3)
    g = torch.Generator().manual_seed(B + L)
    seq = _seq(B, L, g).cuda()
    x = torch.randint(0, 4096, (B, L), generator=g)
    if case == "half":
        x[torch.rand(B, L, generator=g) < 0.5] = MASK
    else:
        x[B - 1, 7] = MASK
    masked = (x == MASK)
    x = x.cuda()
    full = eng.forward_logits(x, seq, sch.t_freq[1]).clone()
    eng.set_needed_rows(True)
    eng.counters(reset=True)
    eng.tail_rows(reset=True)
    sentinel = -12345.0
    out = torch.full((B, L, eng.ld_logits), sentinel, dtype=torch.float32, device="cuda")
    eng.forward_logits_needed(x, seq, sch.t_freq[1], out)
    got = out[..., :full.shape[-1]].cpu()
    assert torch.equal(got[masked], full.cpu()[masked])
    assert bool((out.cpu()[~masked] == sentinel).all())
    assert eng.counters(reset=True) == {"forwards": 1, "token_rows": B * L}
    assert eng.tail_rows(reset=True) == int(masked.sum())
    # all MASK: above the fraction, the plain path, every row runs
    xm = torch.full((B, L), MASK, dtype=torch.int64, device="cuda")
    eng.forward_logits_needed(xm, seq, sch.t_freq[0], out)
    assert eng.tail_rows(reset=True) == B * L
    assert torch.equal(out[..., :full.shape[-1]], eng.forward_logits(xm, seq, sch.t_freq[0]))


def test_stale_rows_are_refused(eng):
    """After a row-skipped ddpm_sample the hidden state of the unmasked rows is stale: embeddings() raises until a full forward."""
    from esmdiff_amd.schedule import ddpm_schedule
    sch = ddpm_schedule(T, eps=0.3)
    B, L = 9, 258
    g = torch.Generator().manual_seed(3)
    seq = _seq(B, L, g).cuda()
    prior = _priors(B, L, g)["every_second"]
    ids, _, t_on = _sample(eng, seq, sch, prior, True)
    assert t_on < (T + 1) * B * L and int((ids == MASK).sum()) == 0
    with pytest.raises(RuntimeError, match="NEEDED_ROWS"):
        eng.embeddings(B, L)
    eng.forward_logits(ids.cuda(), seq, sch.t_freq[0])
    assert eng.embeddings(B, L).shape == (B, L, eng.cfg.d_model)

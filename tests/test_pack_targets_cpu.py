"""--pack_targets on the CPU: the pack planner's invariants and the CLI's refusals."""
import pytest

from esmdiff_amd.dist import shard_samples
from esmdiff_amd.sample_esmdiff import DEFAULT_PACK_TOKENS, pack_stats, plan_packs

# token lengths (BOS and EOS included) like a directory of short targets: 16 targets of 50-150 residues
LENGTHS = [52, 152, 101, 77, 130, 64, 99, 118, 141, 88, 57, 123, 110, 72, 146, 95]


@pytest.mark.parametrize("num_samples,world,budget", [(10, 1, DEFAULT_PACK_TOKENS), (10, 1, 3000), (7, 3, 2000),
                                                      (100, 1, DEFAULT_PACK_TOKENS), (2, 4, 500), (10, 2, 100)])
def test_plan_covers_every_sample_once_within_budget_and_padding(num_samples, world, budget):
    """Every (target, sample) of the world appears exactly once, on the rank shard_samples gives it, with its global Philox
    sample index; each pack holds rows x longest length <= budget (or is a single row) and at most 25 % padding."""
    seen = []
    for rank in range(world):
        offset, count = shard_samples(num_samples, world, rank)
        plan = plan_packs(LENGTHS, num_samples, world, rank, budget)
        for pack in plan:
            rows, L, pad = pack_stats(pack, LENGTHS)
            assert rows * L <= budget or rows == 1, (rows, L)
            assert pad <= 0.25 + 1e-12, pad
            for t, i in pack:
                assert offset <= i < offset + count
                seen.append((t, i))
        assert plan == plan_packs(LENGTHS, num_samples, world, rank, budget)     # deterministic
    assert sorted(seen) == [(t, i) for t in range(len(LENGTHS)) for i in range(num_samples)]


def test_plan_is_the_same_whatever_rank_computes_it():
    """The whole world's plan is a function of (lengths, num_samples, world, budget): any process gets the same list."""
    world_plan = lambda: [plan_packs(LENGTHS, 10, 4, r, 2000) for r in range(4)]
    assert world_plan() == world_plan()
    # sorted by length: packs are filled shortest first, a target's samples may span packs
    plan = plan_packs(LENGTHS, 10, 1, 0, 2000)
    firsts = [LENGTHS[p[0][0]] for p in plan]
    assert firsts == sorted(firsts)
    assert len({t for p in plan for t, _ in p}) == len(LENGTHS) and len(plan) > 1


def test_cli_refuses_pack_targets_with_certified_and_parity(tmp_path):
    from esmdiff_amd.sample_esmdiff import main
    base = ["--random_init", "--tiny", "--synthetic_len", "20", "--output", str(tmp_path), "--pack_targets"]
    with pytest.raises(SystemExit, match=r"--precision f16\|bf16\|f32_split\|f32"):
        main(base + ["--precision", "certified"])
    with pytest.raises(SystemExit, match="--parity"):
        main(base + ["--precision", "f32", "--parity"])

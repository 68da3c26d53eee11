"""Ragged batches on the CPU: mixed-length iterative_sampling_raw on a stand-in engine that models the contract (a row's ids
are a function of its sample index and its own valid positions only), the certified refusal, and the C ABI surface."""
import re
from pathlib import Path

import pytest
import torch

from esmdiff_amd import constants as C

ROOT = Path(__file__).resolve().parents[1]


class RaggedStandin:
    """gibbs_sample with the engine's call shape and its ragged contract: padding must hold the pad ids, MASK positions get ids
    that depend only on (seed, sample index, position) — so a padded row and the same protein alone agree exactly."""
    device = torch.device("cpu")
    has_geom = False

    def __init__(self):
        self.calls = []

    def gibbs_sample(self, seq, x0, table, temperature, top_p, *, seed, sample_offset=0, lengths=None):
        B, L = x0.shape
        lens = [L] * B if lengths is None else list(lengths)
        self.calls.append((B, L, None if lengths is None else lens))
        for b, n in enumerate(lens):
            assert 3 <= n <= L
            assert bool((seq[b, n:] == C.SEQUENCE_PAD_TOKEN).all()) and bool((x0[b, n:] == C.STRUCTURE_PAD_TOKEN).all())
            assert int(seq[b, n - 1]) == 2 and int(x0[b, n - 1]) == C.STRUCTURE_EOS_TOKEN
        idx = torch.arange(sample_offset, sample_offset + B)[:, None]
        ids = (seed * 7 + idx * 131 + torch.arange(L)[None] * 17) % 4096
        return torch.where(x0 == C.STRUCTURE_MASK_TOKEN, ids, x0)

    def set_gibbs_options(self, *a, **k):
        pass


def test_iterative_sampling_raw_mixed_lengths_trimmed_in_order():
    """Proteins of 5, 12 and 8 residues in one call: one padded batch with the lengths passed down, each protein trimmed to
    its own length, in input order, equal to its own call at the same sample index; known tokens are kept."""
    from esmdiff_amd.gibbs import iterative_sampling_raw
    from esmdiff_amd.sdk import ESMProtein, GenerationConfig
    known = torch.tensor([5, C.STRUCTURE_MASK_TOKEN, 7, C.STRUCTURE_MASK_TOKEN, 9, 11, 13, 15])
    proteins = [ESMProtein(sequence="ACDEF"), ESMProtein(sequence="GHIKLMNPQRST"), ESMProtein(sequence="VWYACDEF", structure_tokens=known)]
    cfg = [GenerationConfig(num_steps=4)] * 3
    eng = RaggedStandin()
    out = iterative_sampling_raw(eng, proteins, cfg, seed=3, sample_offset=10)
    assert eng.calls == [(3, 14, [7, 14, 10])]
    assert [o.sequence for o in out] == [p.sequence for p in proteins]
    assert [tuple(o.structure_tokens.shape) for o in out] == [(5,), (12,), (8,)]
    for b, p in enumerate(proteins):
        solo = iterative_sampling_raw(RaggedStandin(), [p], [cfg[0]], seed=3, sample_offset=10 + b)[0]
        assert torch.equal(out[b].structure_tokens, solo.structure_tokens), b
    assert torch.equal(out[2].structure_tokens[[0, 2, 4, 5, 6, 7]], known[[0, 2, 4, 5, 6, 7]])
    # a batch of one length runs exactly as before: no lengths are passed
    eng = RaggedStandin()
    iterative_sampling_raw(eng, proteins[:1] * 2, cfg[:2], seed=3)
    assert eng.calls == [(2, 7, None)]


def test_iterative_sampling_raw_mixed_lengths_refused_when_certified():
    from esmdiff_amd.gibbs import iterative_sampling_raw
    from esmdiff_amd.sdk import ESMProtein, GenerationConfig

    class Certified:
        net = RaggedStandin()
        fast = RaggedStandin()
        certified = object()

    with pytest.raises(NotImplementedError, match="f16, bf16, f32_split or f32"):
        iterative_sampling_raw(Certified(), [ESMProtein(sequence="ACD"), ESMProtein(sequence="ACDE")], [GenerationConfig()] * 2)


def test_set_lengths_is_exported_and_declared():
    from esmdiff_amd import _native
    lib = _native.lib()
    assert hasattr(lib, "esmdiff_set_lengths") and hasattr(lib, "esmdiff_attention_ragged")
    hdr = (ROOT / "include" / "esmdiff_hip.h").read_text()
    assert re.search(r"int esmdiff_set_lengths\(esmdiff_engine\* eng, const int32_t\* lens, int32_t B\);", hdr)
    assert "esmdiff_attention_ragged(" in (ROOT / "include" / "esmdiff_hip_test.h").read_text()
    assert lib.esmdiff_set_lengths(None, None, 0) == -1          # no engine: ESMDIFF_E_INVALID, nothing touched

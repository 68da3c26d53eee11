"""Packed targets against one target per batch (sample_esmdiff.py --pack_targets) on one GPU, at production width.

A synthetic evaluation set like the reference's (many short targets): 16 targets of 50-150 residues, 10 samples each, 25 ddpm
steps, bf16, ESM3-open-sized random weights.  Prints

  * samples/s of the per-target run (one ddpm_sample call per target, as the CLI does by default) and of the packed run
    (plan_packs at the default budget, one ragged call per pack, per-row Philox sample indices), and their ratio;
  * the packs: rows, padded length, padded-row share;
  * the attention kernel time of one forward of the largest pack: ragged (lengths set) against the same batch padded;
  * how many packed ids differ from the per-target run's (bf16: near-ties may, see --pack_targets).

    python tools/packed_targets_bench.py [--targets 16] [--samples 10] [--steps 25] [--reps 2] [--out profiles/r07_packed_targets.txt]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # the repository root
from esmdiff_amd import constants as C                                              # noqa: E402
from esmdiff_amd.config import ESM3_OPEN                                              # noqa: E402
from esmdiff_amd.model import random_init_model                                       # noqa: E402
from esmdiff_amd.sample_esmdiff import DEFAULT_PACK_TOKENS, pack_stats, plan_packs   # noqa: E402
from esmdiff_amd.sdk import encode_sequence                                           # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--targets", type=int, default=16)
ap.add_argument("--samples", type=int, default=10)
ap.add_argument("--steps", type=int, default=25)
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--pack_tokens", type=int, default=DEFAULT_PACK_TOKENS)
ap.add_argument("--out", default=None)
args = ap.parse_args()

lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


g = torch.Generator().manual_seed(0)
n_res = [int(v) for v in torch.linspace(50, 150, args.targets).round()]
seqs = ["".join(C.SEQUENCE_VOCAB[int(i)] for i in torch.randint(4, 24, (n,), generator=g)) for n in n_res]
lengths = [n + 2 for n in n_res]
packs = plan_packs(lengths, args.samples, 1, 0, args.pack_tokens)
max_b = max(max(len(p) for p in packs), args.samples)
model = random_init_model(ESM3_OPEN, seed=0, max_batch=max_b, max_len=max(lengths), precision="bf16")
eng = model.net
n_total = args.targets * args.samples


def per_target():
    out = []
    for s in seqs:
        out.append(model.ddpm_sample(encode_sequence(s)[None].repeat(args.samples, 1), num_steps=args.steps, seed=1).cpu())
    return out


def packed():
    out = [[None] * args.samples for _ in seqs]
    for pack in packs:
        _, L, _ = pack_stats(pack, lengths)
        seq = torch.full((len(pack), L), C.SEQUENCE_PAD_TOKEN, dtype=torch.int64)
        for r, (t, _) in enumerate(pack):
            seq[r, :lengths[t]] = encode_sequence(seqs[t])
        x = model.ddpm_sample(seq, num_steps=args.steps, seed=1, lengths=[lengths[t] for t, _ in pack],
                              sample_index=[i for _, i in pack]).cpu()
        for r, (t, i) in enumerate(pack):
            out[t][i] = x[r, :lengths[t]]
    return [torch.stack(o) for o in out]


def timed(fn):
    fn()                                                   # warm-up (first-touch of every shape)
    best, res = float("inf"), None
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best, res


say(f"packed_targets_bench: {args.targets} targets of {min(n_res)}-{max(n_res)} residues, {args.samples} samples each, "
    f"{args.steps} ddpm steps, bf16, d_model {ESM3_OPEN.d_model} x {ESM3_OPEN.n_layers} blocks (random weights), "
    f"pack budget {args.pack_tokens} tokens; best of {args.reps} after a warm-up")
for k, p in enumerate(packs):
    rows, L, pad = pack_stats(p, lengths)
    say(f"  pack {k}: {rows:4d} rows x {L:3d} tokens = {rows * L:6d} padded tokens, padded-row share {pad:.1%}, "
        f"{len({t for t, _ in p})} targets")
tot_pad = sum(pack_stats(p, lengths)[0] * pack_stats(p, lengths)[1] for p in packs)
say(f"  padded-row share over all packs: {1 - args.samples * sum(lengths) / tot_pad:.1%}")
t_solo, ids_solo = timed(per_target)
t_pack, ids_pack = timed(packed)
say(f"per-target: {t_solo:.3f} s  {n_total / t_solo:.1f} samples/s")
say(f"packed:     {t_pack:.3f} s  {n_total / t_pack:.1f} samples/s")
say(f"packed / per-target: {t_solo / t_pack:.2f}x")
diff = sum(int((a != b).sum()) for a, b in zip(ids_solo, ids_pack))
say(f"ids differing from the per-target run: {diff} of {sum(a.numel() for a in ids_solo)} (bf16 near-ties between batch compositions)")

# attention kernel time of one forward of the largest pack: ragged against the same batch padded (profiling section "attention")
big = max(packs, key=lambda p: pack_stats(p, lengths)[0] * pack_stats(p, lengths)[1])
rows, L, _ = pack_stats(big, lengths)
lens = [lengths[t] for t, _ in big]
seq = torch.full((rows, L), C.SEQUENCE_PAD_TOKEN, dtype=torch.int64)
x = torch.full((rows, L), C.STRUCTURE_PAD_TOKEN, dtype=torch.int64)
for r, (t, _) in enumerate(big):
    seq[r, :lens[r]] = encode_sequence(seqs[t])
    x[r, :lens[r]] = C.STRUCTURE_MASK_TOKEN
    x[r, 0], x[r, lens[r] - 1] = C.STRUCTURE_BOS_TOKEN, C.STRUCTURE_EOS_TOKEN
seq, x = seq.cuda(), x.cuda()
tf = eng.conditioning_rows(torch.zeros(eng.cfg.freq_dim))


def attn_ms(ragged: bool, n=5):
    eng.forward_logits(x, seq, tf, lengths=lens if ragged else None)
    eng.set_profiling(1)
    for _ in range(n):
        eng.forward_logits(x, seq, tf, lengths=lens if ragged else None)
    torch.cuda.synchronize()
    prof = eng.get_profile()
    eng.set_profiling(0)
    return prof["attention"]["ms"] / n, sum(v["ms"] for k, v in prof.items() if k != "gemm_ffn_up_union") / n


a_rag, f_rag = attn_ms(True)
a_pad, f_pad = attn_ms(False)
say(f"largest pack ({rows} x {L}, {sum(lens)} valid tokens of {rows * L}): attention {a_rag:.3f} ms ragged vs {a_pad:.3f} ms "
    f"padded per forward ({a_pad / a_rag:.2f}x); all sections {f_rag:.2f} vs {f_pad:.2f} ms (one stream under profiling)")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")

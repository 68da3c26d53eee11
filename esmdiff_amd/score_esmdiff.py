"""Score sampled structures by model likelihood: the per-structure negative ELBO of esmdiff_amd.nelbo (the reference's
validation metric, /root/reference/slm/models/model.py:386-462, as an estimator over --num_draws noise draws).

    python -m esmdiff_amd.score_esmdiff --input data/targets/bpti --tokens output/.../bpti.tokens.npy \
        (--ckpt release_v0.pt | --random_init) [--num_draws 32] [--seed 0] [--precision f32_split] --output scores/

--input   a directory of target PDB files, as sample_esmdiff takes it (the sequence each structure is scored under)
--tokens  a `<name>.tokens.npy` as sample_esmdiff writes it ((N, L_res) int16 structure tokens without BOS / EOS), or a
          directory of them, matched to the targets by name.  BOS / EOS are added here and are outside the loss mask: the
          score counts residues.
Writes `<output>/<name>.nelbo.json` per target: per-sample nelbo (nats per residue, lower = more likely under the model), its
spread over the draws (std / sqrt(K): an upper estimate of the standard error, the draws being stratified in t), the ranking
(sample indices, most likely first), K, seed, precision, the model's scoring flags and the library's build info.

--precision defaults to f32_split: a likelihood is compared across runs and batches, and that engine's rows are
batch-independent bit for bit, so a structure's score does not depend on what it was scored with.
"""
from __future__ import annotations

import argparse
import json
from pathlib import Path

import numpy as np
import torch

from . import constants as C
from .sdk import ESMProtein, encode_sequence


def get_argparser(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--input", type=str, required=True, help="Directory of target PDB files (the sequences).")
    p.add_argument("--tokens", type=str, required=True, help="<name>.tokens.npy, or a directory of them.")
    p.add_argument("--ckpt", type=str, default=None, help="Path to the model checkpoint.")
    p.add_argument("--random_init", action="store_true", help="ESM3-open-sized random weights instead of --ckpt")
    p.add_argument("--tiny", action="store_true", help=argparse.SUPPRESS)   # tests: 2-block model with --random_init
    p.add_argument("--num_draws", type=int, default=32, help="Noise draws (time + mask) per structure.")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--output", type=str, default="output/score_esmdiff")
    p.add_argument("--precision", choices=["bf16", "f16", "f32_split", "f32"], default="f32_split")
    p.add_argument("--max_batch", type=int, default=64, help="(structure, draw) pairs per forward.")
    return p.parse_args(argv)


def structure_tokens_with_bos_eos(tokens: np.ndarray) -> torch.Tensor:
    """(N, L_res) residue tokens -> (N, L_res + 2) int64 with BOS / EOS, as the sampler held them (sample_esmdiff.py:220-221)."""
    t = torch.as_tensor(np.asarray(tokens).astype(np.int64))
    if t.dim() != 2:
        raise ValueError(f"tokens must be (N, L_res), got {tuple(t.shape)}")
    n = t.shape[0]
    return torch.cat([torch.full((n, 1), C.STRUCTURE_BOS_TOKEN), t, torch.full((n, 1), C.STRUCTURE_EOS_TOKEN)], dim=1)


def score_target(model, sequence: str, tokens: np.ndarray, num_draws: int, seed: int, max_batch=None):
    """(nelbo (N,), stderr (N,)) of the N structures of one target; residues only (BOS / EOS outside the loss mask)."""
    x0 = structure_tokens_with_bos_eos(tokens)
    seq = encode_sequence(sequence)
    if seq.numel() != x0.shape[1]:
        raise ValueError(f"{x0.shape[1] - 2} structure tokens per sample for a sequence of {seq.numel() - 2} residues")
    mask = torch.ones_like(x0)
    mask[:, 0] = mask[:, -1] = 0
    return model.nelbo(x0, seq, num_draws=num_draws, seed=seed, mask=mask, max_batch=max_batch)


def main(argv=None):
    args = get_argparser(argv)
    if args.ckpt is None and not args.random_init:
        raise SystemExit("no weights: pass --ckpt <release_v0.pt> or --random_init (synthetic weights)")
    data_path, tok_path = Path(args.input), Path(args.tokens)
    assert data_path.is_dir(), f"Invalid directory {data_path} (Currently we only support pdb files in a folder as input)."
    targets = [(p.stem, ESMProtein.from_pdb(p).sequence) for p in sorted(q for q in data_path.iterdir() if q.suffix == ".pdb")]
    if tok_path.is_dir():
        files = {name: tok_path / f"{name}.tokens.npy" for name, _ in targets}
        files = {n: f for n, f in files.items() if f.exists()}
    else:
        name = tok_path.name[:-len(".tokens.npy")] if tok_path.name.endswith(".tokens.npy") else tok_path.stem
        files = {name: tok_path}
    work = [(n, s, files[n]) for n, s in targets if n in files]
    if not work:
        raise SystemExit(f"no <name>.tokens.npy under {tok_path} matches a target of {data_path} ({[n for n, _ in targets]})")
    from . import _native
    from .model import SCORING_FLAGS, load_state_dict_from_lightning_ckpt, random_init_model
    max_len = max(len(s) for _, s, _ in work) + 2
    if args.random_init:
        from .config import ESM3_OPEN, TINY
        model = random_init_model(TINY if args.tiny else ESM3_OPEN, seed=args.seed, max_batch=args.max_batch, max_len=max_len,
                                  precision=args.precision)
    else:
        model = load_state_dict_from_lightning_ckpt(args.ckpt, max_batch=args.max_batch, max_len=max_len, precision=args.precision)
    out_dir = Path(args.output)
    out_dir.mkdir(parents=True, exist_ok=True)
    info = _native.build_info()
    for name, sequence, f in work:
        nelbo, stderr = score_target(model, sequence, np.load(f), args.num_draws, args.seed)
        order = sorted(range(nelbo.numel()), key=lambda i: float(nelbo[i]))
        (out_dir / f"{name}.nelbo.json").write_text(json.dumps(
            {"target": name, "sequence": sequence, "tokens": str(f), "num_samples": int(nelbo.numel()), "nelbo": [float(v) for v in nelbo],
             "stderr": [float(v) for v in stderr], "ranking": order, "unit": "nats per residue", "num_draws": args.num_draws,
             "seed": args.seed, "precision": args.precision, "build_info": info,
             "stderr_is": ("std over the draws / sqrt(num_draws): the standard error for independent draws; an upper estimate "
                           "when the draws are stratified in t (antithetic_sampling)"),
             "scoring_flags": {k: getattr(model, k) for k in SCORING_FLAGS}}, indent=1))
        print(f"{name}: {nelbo.numel()} structures, nelbo {float(nelbo.min()):.4f} .. {float(nelbo.max()):.4f} "
              f"-> {out_dir / f'{name}.nelbo.json'}")


if __name__ == "__main__":
    main()

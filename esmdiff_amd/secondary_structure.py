"""Secondary structure of one sampled ensemble on the device, without targets (PED / IDP ensembles).

    python -m esmdiff_amd.secondary_structure --samples <multi-MODEL pdb> --output <dir> [--max_models N] [--seed 0]

Writes <output>/<samples stem>.dssp.json — the "dssp" block of `python -m esmdiff_amd.analyze_ensemble --dssp` without its target
entries: the legend, the eight-state string of every analysed MODEL, counts (L, 8), the three-state propensity per residue (helix,
strand, coil) and the ensemble's content — and <output>/<samples stem>.ss, one string per MODEL.  The states are those of
esmdiff_amd/secondary.py (csrc/dssp.hip; [DSSP-RECALL], parity with mkdssp unpinned); the carbonyl O is inferred
from N / CA / C, and the prolines named in the file's first model donate no hydrogen bond.  More than --max_models models: a random
subset of that size (seeded), as in analyze_ensemble."""
from __future__ import annotations

import argparse
import json
from pathlib import Path

from .analyze_ensemble import _jsonable, dssp_report
from .pdbio import load_coords


def parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--samples", required=True, help="multi-MODEL PDB of the sampled ensemble")
    ap.add_argument("--output", required=True, help="output directory")
    ap.add_argument("--max_models", type=int, default=None, help="analyse at most this many models (default: all)")
    ap.add_argument("--seed", type=int, default=0, help="seed of the down-sampling to --max_models")
    return ap


def main(argv=None) -> Path:
    import numpy as np
    args = parser().parse_args(argv)
    keep = None
    if args.max_models is not None:
        n = len(load_coords(Path(args.samples), max_n_model=None, verbose=False))
        if n > args.max_models:
            keep = np.sort(np.random.default_rng(args.seed).choice(n, args.max_models, replace=False))
    block = dssp_report(args.samples, [], keep)
    out = Path(args.output)
    out.mkdir(parents=True, exist_ok=True)
    stem = Path(args.samples).stem
    path = out / f"{stem}.dssp.json"
    path.write_text(json.dumps({k: _jsonable(v) for k, v in block.items()}, indent=1) + "\n")
    (out / f"{stem}.ss").write_text("\n".join(block["strings"]) + "\n")
    print(path)
    return path


if __name__ == "__main__":
    main()

"""Evaluate one sampled ensemble against its target structures on the device.

    python -m esmdiff_amd.analyze_ensemble --samples <multi-MODEL pdb> --targets a.pdb [b.pdb ...] --output <dir> [--max_models 100]

Two targets: the apo / holo (or CoDNaS) row of the reference's analysis/apo_analysis.py:222-272 — esmdiff_amd.ensemble.apo_report.
Any other number K: the BPTI-style evaluation of analysis/bpti_analysis.py:116-129 — tm_n_ensemble's per-target lists and the
three columns of bpti_tm_rmsd_div.csv (TM-ens, RMSD-ens, TM-div).  Writes <output>/<samples stem>.ensemble.json.
TM-scores are [TMSCORE-RECALL], parity unpinned (esmdiff_amd/ensemble.py)."""
from __future__ import annotations

import argparse
import json
from pathlib import Path

import numpy as np

from . import ensemble
from .pdbio import load_coords


def _jsonable(v):
    if isinstance(v, np.ndarray):
        return [_jsonable(x) for x in v.tolist()]
    if isinstance(v, (list, tuple)):
        return [_jsonable(x) for x in v]
    if isinstance(v, (float, np.floating)):
        return None if np.isnan(v) else float(v)       # JSON has no NaN: an unresolved residue is null
    return v


def analyze(samples_path, target_paths, max_models: int = 100, seed: int = 0) -> dict:
    samples = load_coords(Path(samples_path), max_n_model=None, verbose=False)
    if len(samples) > max_models:
        samples = samples[np.sort(np.random.default_rng(seed).choice(len(samples), max_models, replace=False))]
    targets = [load_coords(Path(p), max_n_model=None, verbose=False)[0] for p in target_paths]
    for p, t in zip(target_paths, targets):
        if t.shape[0] != samples.shape[1]:
            raise ValueError(f"{p} has {t.shape[0]} residues, the samples {samples.shape[1]}: the correspondence is residue to residue")
    if len(targets) == 2:
        return ensemble.apo_report(samples, targets[0], targets[1])
    best_tm, best_rmsd = ensemble.tm_n_ensemble(samples, np.stack(targets), max_n_model=max_models, rng=seed)
    return {"best_tm": best_tm, "best_rmsd": best_rmsd, "TM-ens": float(np.mean(best_tm)), "RMSD-ens": float(np.mean(best_rmsd)),
            "TM-div": ensemble.tm_diversity(samples)}


def main(argv=None) -> Path:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--samples", required=True, help="multi-MODEL PDB of the sampled ensemble")
    ap.add_argument("--targets", required=True, nargs="+", help="target structures, one PDB each (same sequence as the samples)")
    ap.add_argument("--output", required=True, help="output directory")
    ap.add_argument("--max_models", type=int, default=100)
    ap.add_argument("--seed", type=int, default=0, help="seed of the down-sampling to --max_models")
    args = ap.parse_args(argv)
    report = analyze(args.samples, args.targets, args.max_models, args.seed)
    out = Path(args.output)
    out.mkdir(parents=True, exist_ok=True)
    path = out / f"{Path(args.samples).stem}.ensemble.json"
    path.write_text(json.dumps({k: _jsonable(v) for k, v in report.items()}, indent=1) + "\n")
    print(path)
    return path


if __name__ == "__main__":
    main()

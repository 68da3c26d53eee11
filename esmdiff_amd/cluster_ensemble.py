"""Cluster one sampled ensemble on the device and write its representatives.

    python -m esmdiff_amd.cluster_ensemble --samples <multi-MODEL pdb> --cutoff <float> --output <dir> [--metric rmsd|tm|lddt]
                                           [--max_models N] [--seed 0]

GROMOS clustering (esmdiff_amd/clustering.py) of the models' CA traces under an RMSD cutoff in Angstrom (--metric rmsd, the
default) or a cutoff on the symmetric mean TM-score (--metric tm) or CA-lDDT (--metric lddt, no superposition).  Writes two files into <output>:
  <stem>.clusters.json   metric, cutoff, n, n_clusters, sizes, centres and models (0-based MODEL positions in the input: of the
                         cluster centres and of all n clustered models), labels (one per clustered model), and per cluster the
                         mean and the maximum distance of its members to the centre (tm, lddt: distance = 1 - score);
  <stem>.clusters.pdb    the centre models in cluster order: MODEL k + 1 is the representative of cluster k, its ATOM / TER
                         records copied from the input.
More than --max_models models (default: all are kept) are down-sampled without replacement from --seed, in input order.
TM-scores are [TMSCORE-RECALL], parity unpinned (esmdiff_amd/ensemble.py)."""
from __future__ import annotations

import argparse
import json
import tempfile
from pathlib import Path

import numpy as np

from . import clustering
from .pdbio import load_coords, merge_pdbfiles, split_pdbfile


def parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--samples", required=True, help="multi-MODEL PDB of the sampled ensemble")
    ap.add_argument("--cutoff", required=True, type=float, help="neighbour cutoff: RMSD in Angstrom, or the TM-score / lDDT with --metric tm / lddt")
    ap.add_argument("--output", required=True, help="output directory")
    ap.add_argument("--metric", choices=("rmsd", "tm", "lddt"), default="rmsd")
    ap.add_argument("--max_models", type=int, default=None, help="cluster at most this many models (default: all)")
    ap.add_argument("--seed", type=int, default=0, help="seed of the down-sampling to --max_models")
    return ap


def report(result, distances, models, metric: str, cutoff: float) -> dict:
    """The JSON document: `result` a Clustering of the models at input positions `models`, `distances` (n,) what
    centre_distances gives (tm, lddt: the score; the document holds 1 - score)."""
    labels, distances, models = np.asarray(result.labels), np.asarray(distances, np.float64), np.asarray(models)
    if metric in ("tm", "lddt"):
        distances = 1.0 - distances
    members = [distances[labels == k] for k in range(result.n_clusters)]
    out = {"metric": metric, "cutoff": float(cutoff), "n": int(len(labels)), "n_clusters": int(result.n_clusters),
           "sizes": [int(s) for s in result.sizes], "centres": [int(models[c]) for c in result.centres],
           "models": [int(m) for m in models], "labels": [int(x) for x in labels],
           "mean_distance": [float(np.mean(m)) for m in members], "max_distance": [float(np.max(m)) for m in members]}
    if metric == "tm":
        out["tm_score"] = clustering.TM_NOTE
    return out


def write_centres(samples_path, centres, save_to) -> None:
    """The MODEL blocks of `samples_path` at the 0-based positions `centres`, in that order, as one multi-MODEL file."""
    blocks = split_pdbfile(samples_path, verbose=False)
    with tempfile.TemporaryDirectory() as tmp:
        files = []
        for k, c in enumerate(centres):
            files.append(Path(tmp) / f"centre_{k}.pdb")
            files[-1].write_text(blocks[c])
        merge_pdbfiles(files, Path(save_to), verbose=False)


def main(argv=None):
    args = parser().parse_args(argv)
    samples = load_coords(Path(args.samples), max_n_model=None, verbose=False)
    models = np.arange(len(samples))
    if args.max_models is not None and len(samples) > args.max_models:
        models = np.sort(np.random.default_rng(args.seed).choice(len(samples), args.max_models, replace=False))
        samples = samples[models]
    result = clustering.cluster_ensemble(samples, args.cutoff, metric=args.metric)
    doc = report(result, clustering.centre_distances(samples, result, metric=args.metric), models, args.metric, args.cutoff)
    out = Path(args.output)
    out.mkdir(parents=True, exist_ok=True)
    stem = Path(args.samples).stem
    json_path, pdb_path = out / f"{stem}.clusters.json", out / f"{stem}.clusters.pdb"
    json_path.write_text(json.dumps(doc, indent=1) + "\n")
    write_centres(args.samples, doc["centres"], pdb_path)
    print(json_path)
    print(pdb_path)
    return json_path, pdb_path


if __name__ == "__main__":
    main()

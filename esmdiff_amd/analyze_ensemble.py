"""Evaluate one sampled ensemble against its target structures on the device.

    python -m esmdiff_amd.analyze_ensemble --samples <multi-MODEL pdb> --targets a.pdb [b.pdb ...] --output <dir> [--max_models 100]
                                           [--lddt] [--plddt_scale 1.0] [--flex] [--pca_components 3] [--dssp]
                                           [--contacts] [--contact_cutoff 8.0] [--contact_min_sep 3]
                                           [--torsions] [--rama_bins 36]
                                           [--shape] [--pr_bins 100] [--saxs] [--saxs_qmax 0.5] [--saxs_points 51] [--saxs_data FILE]
                                           [--sasa] [--sasa_points 96] [--sasa_probe 1.4] [--sasa_threshold 0.2]
                                           [--tica --trajectory REF] [--lagtime 20] [--tica_dim 2] [--lagtimes 5 10 20 ...]
                                           [--msm] [--msm_states 100] [--msm_lagtime LAG] [--msm_metastable 2] [--msm_seed 0]
                                           [--compare --trajectory REF] [--compare_ref target|first] [--compare_modes 2]
                                           [--coverage --trajectory REF] [--coverage_cutoffs 1 2 3]

Two targets: the apo / holo (or CoDNaS) row of the reference's analysis/apo_analysis.py:222-272 — esmdiff_amd.ensemble.apo_report.
Any other number K: the BPTI-style evaluation of analysis/bpti_analysis.py:116-129 — tm_n_ensemble's per-target lists and the
three columns of bpti_tm_rmsd_div.csv (TM-ens, RMSD-ens, TM-div).  Writes <output>/<samples stem>.ensemble.json.
TM-scores are [TMSCORE-RECALL], parity unpinned (esmdiff_amd/ensemble.py).
--lddt adds the superposition-free scores of csrc/lddt.hip (integer counts, held exactly to numpy): lddt_ens (the best sample's
CA-lDDT per target, averaged), lddt_div (the mean symmetric lDDT over sample pairs), best_lddt / best_lddt_model / best_lddt_residue
(per target: the best sample's lDDT, its position among the analysed samples, its per-residue lDDT) and, when the samples' PDB
carries B-factors (the decoder's pLDDT, divided by --plddt_scale), plddt_agreement: per target the per-residue mean observed lDDT,
the mean predicted one, their Pearson r and the mean absolute difference.
--flex adds a "flex" block (esmdiff_amd/flexibility.py, csrc/flex.hip): the mean structure of the samples (n_iter, converged, mean,
rmsd_to_mean), the RMSF about it (rmsf), the reference's pairwise RMSF (pair_rmsf), and the Cartesian PCA of the samples superposed
on the mean (pca: explained_variance, explained_variance_ratio, projections of the samples, target_projections; --pca_components
modes).  With exactly two targets also resflex (Pearson / Spearman / Kendall between the report's apo-holo deviation `rmsd` and its
`rmsf`, the reference's per-target numbers), resflex_mean_structure (the same against the mean-structure RMSF) and
displacement_overlap (the share of the displacement between the two targets that the leading modes span, cumulative).
--dssp adds a "dssp" block (esmdiff_amd/secondary.py, csrc/dssp.hip; [DSSP-RECALL], parity with mkdssp unpinned): the legend, the
samples' eight-state strings, counts (L, 8), the three-state propensity (helix, strand, coil per residue) and content, per target its
string and the agreement of the samples with it (q3 per sample, q3_mean, q3_best, best_model, per_residue) and, with exactly two
targets, switch_residues: the residues whose three-state class differs between the two, with the ensemble's share in each target's
class — the secondary-structure counterpart of ResFlex.  Samples and targets are read again as N / CA / C with the carbonyl O inferred
on both alike; the samples' prolines donate no hydrogen bond.
--contacts adds a "contacts" block (esmdiff_amd/contacts.py, csrc/contacts.hip): the parameters (cutoff, min_separation, and the
convention lam = 1.2, beta = 5 of Q), the ensemble's contacts as a sparse list [a, b, frequency, mean_distance] of the pairs a < b in
contact in at least one sample (--contact_cutoff Angstrom between CA atoms, |a - b| >= --contact_min_sep), the internal scaling
profile (separation, rms_distance) and its Flory exponent, per target the number of its contacts and every sample's hard and soft
fraction of native contacts (q, q_soft, q_mean, q_soft_mean, q_best, best_model), q_ens (the mean of q_best) and, with exactly two
targets, contact_switches: the contacts formed in one target only, with the samples' frequency of each.
--torsions adds a "torsions" block (esmdiff_amd/torsions.py, csrc/torsions.hip): the parameters (bins, break_distance, the region
rectangles), per residue the counts (phi, psi, both, omega defined, cis), the circular means and variances of phi / psi / omega, the
region propensities (alpha, beta, ppII, left, other: a stated convention), the cis fraction and the entropy of the --rama_bins x
--rama_bins Ramachandran map, the geometry summary of the samples (bond lengths and angles against ideal values, outliers per sample),
per target its phi / psi, its region string and the agreement of the samples with it (share per sample, share_mean, share_best,
best_model, per_residue), js_ramachandran: the Jensen-Shannon distance between the samples' maps and those of the targets taken
together as one ensemble (thin with few targets: each target fills one cell per residue) and, with exactly two targets,
region_switches: the residues whose region differs between the two, with the samples' share in each.  Samples and targets are read
again as N / CA / C backbones, on the analysed subset.
--shape adds a "shape" block (esmdiff_amd/shape.py, csrc/shape.hip): per sample the number of residues, the centroid, the eigenvalues
of the gyration tensor, Rg, asphericity, acylindricity, the relative shape anisotropy, the end-to-end distance, Dmax and the Kirkwood
hydrodynamic radius; their summary (mean, std, min, max); the pair-distance distribution p(r) of the samples in --pr_bins cells up to
the largest Dmax rounded up to a whole Angstrom; per target its own descriptors; and js_shape: the Jensen-Shannon distance between the
samples' distribution of rg, ree, rh and asphericity and that of the targets taken together as one ensemble (thin with few targets:
each target fills one cell per quantity).
--saxs adds a "saxs" block: q (0 .. --saxs_qmax in --saxs_points steps, 1 / Angstrom), the mean Debye intensity of the samples as point
scatterers at the CA positions, i0, the normalised curve, the Guinier fit (rg, i0, q_max, n_points) beside the coordinate Rg, and the
dimensionless Kratky curve.  --saxs_data FILE (three whitespace-separated columns q, I, sigma; lines starting with # are ignored;
implies --saxs) evaluates at the file's q instead and adds chi2_mean, the reduced chi^2 of the mean profile after the least-squares
scale, and chi2_samples: that of every sample, with the best one.
--sasa adds a "sasa" block (esmdiff_amd/accessibility.py, csrc/sasa.hip; Shrake & Rupley on N / CA / C and the inferred O, parity with
NACCESS / freesasa / mdtraj unpinned): the parameters (--sasa_points, --sasa_probe, --sasa_threshold, the radii), per residue the mean
area, the mean relative exposure and the share of samples in which it is exposed, per sample the total area with its summary, per target
its own per-residue values and exposed_jaccard (the Jaccard index of the residues the target exposes and those the samples expose in
more than half of their frames) and, with exactly two targets, exposure_switches: the residues exposed in one target only, with the
samples' frequency of each.  Samples and targets are read again as N / CA / C backbones, on the analysed subset.
--tica --trajectory REF adds a "tica" block (esmdiff_amd/kinetics.py, csrc/lagged.hip; [DEEPTIME-RECALL], parity unpinned): REF is an MD
trajectory of the same chain, a .npy (n, L, 3) CA array (memory-mapped, uploaded --tica_chunk pairs at a time) or a multi-MODEL PDB.  A
TICA model of its CA distances is fitted at --lagtime with --tica_dim components; the block holds the parameters, the eigenvalues,
timescales and n_kept, the VAMP-2 score, per TIC the Jensen-Shannon distance of the samples against the trajectory (js_tic) and their
mean (js_tica), the projections of the samples and of every target, with --lagtimes the implied-timescale table, and the trajectory's
free-energy grid over TIC 1 x TIC 2 (-ln p, null in an empty cell).
--msm (with --tica --trajectory REF) adds an "msm" block (esmdiff_amd/states.py, csrc/msm.hip; [DEEPTIME-RECALL], parity unpinned): the
trajectory's TICA coordinates are clustered into --msm_states microstates by k-means (kmeans++ from --msm_seed), the transitions are
counted at --msm_lagtime frames (default: --lagtime) and a reversible Markov state model is estimated on the largest connected set.  The
block holds the parameters, the inertia and the iterations, the size of the active set and the total of the count matrix, the leading
eigenvalues and timescales, the stationary distribution over the microstates, --msm_metastable metastable sets (the inner-simplex step
of PCCA+) with their weights and mean TIC position, the microstate of every sample and of every target, and compare_populations: the
Jensen-Shannon distance of the samples' microstate histogram against the stationary distribution, the populations per metastable set
beside the model's and the share of the samples outside the active set.
--compare --trajectory REF adds a "compare" block (esmdiff_amd/covariance.py, csrc/aligned.hip; [ALPHAFLOW-RECALL], parity unpinned):
the samples against the trajectory in Cartesian space, both superposed on --compare_ref (the first target, or the trajectory's first
frame) and reduced to their mean and 3L x 3L covariance on the device.  The block holds per residue the Gaussian W2 distance with its
translation and variance parts, their root means (rmwd), the W2 distance in the trajectory's and in the joint PCA space of
--compare_modes modes and in all 3L dimensions, the per-component W2 of the projections, RMSIP and the mode cosines, the Pearson
correlations of the two cross-correlation maps and of the two RMSF profiles, the frames that entered and were dropped, and the
projections of the samples and of every target on the trajectory's modes.  A .npy trajectory is read --tica_chunk frames at a time.
--coverage --trajectory REF adds a "coverage" block (esmdiff_amd/neighbours.py, csrc/rmsd_nn.hip): nearest neighbours under the Kabsch
RMSD between the samples and every frame of the trajectory, on the residues resolved in the first sample, the first frame and every
target.  Per --coverage_cutoffs value the recall (the share of trajectory frames with a sample within it) and the precision (the share of
samples within it of some frame), the mean nearest RMSD each way (mat_r, mat_p), for each sample its nearest frame and RMSD, the samples
beyond the largest cutoff of every frame (novel), per target the nearest sample and the nearest frame, the mean pairwise RMSD of the
samples and of the trajectory, and the frames used and dropped.  A .npy trajectory is read --tica_chunk frames at a time."""
from __future__ import annotations

import argparse
import json
from pathlib import Path

import numpy as np

from . import accessibility, contacts, covariance, ensemble, flexibility, kinetics, neighbours, secondary, shape, states, torsions
from .pdbio import load_coords, read_pdb_backbone, read_pdb_bfactors


def _jsonable(v):
    if isinstance(v, np.ndarray):
        return [_jsonable(x) for x in v.tolist()]
    if isinstance(v, dict):
        return {k: _jsonable(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_jsonable(x) for x in v]
    if isinstance(v, (float, np.floating)):
        return None if np.isnan(v) else float(v)       # JSON has no NaN: an unresolved residue is null
    return v


def lddt_report(samples, targets, plddt=None, plddt_scale: float = 1.0) -> dict:
    """The --lddt keys: samples (n, L, 3), targets (K, L, 3), plddt (n, L) or None."""
    score, res = ensemble.lddt_matrix(samples, targets, per_residue=True)
    best = np.where(np.isnan(score), -1.0, score).argmax(0)          # a sample without a defined score is never the best
    out = {"lddt_ens": ensemble.lddt_ensemble(samples, targets), "lddt_div": ensemble.lddt_diversity(samples),
           "best_lddt": [float(score[i, k]) for k, i in enumerate(best)], "best_lddt_model": [int(i) for i in best],
           "best_lddt_residue": [res[i, k] for k, i in enumerate(best)]}
    if plddt is not None:
        out["plddt_agreement"] = [ensemble.plddt_agreement(samples, t, plddt, plddt_scale) for t in targets]
    return out


def flex_report(samples, targets, report: dict, pca_components: int = 3) -> dict:
    """The --flex block: samples (n, L, 3), targets (K, L, 3), report: what analyze computed so far (two targets: apo_report's)."""
    ms = flexibility.mean_structure(samples)
    out = {"n_iter": ms.n_iter, "converged": ms.converged, "rmsd_to_mean": ms.rmsd_to_mean, "mean": ms.mean, "rmsf": ms.rmsf,
           "pair_rmsf": flexibility.pair_rmsf(samples)}
    p = flexibility.pca(samples, n_components=pca_components)
    out["pca"] = {"explained_variance": p.explained_variance, "explained_variance_ratio": p.explained_variance_ratio,
                  "projections": p.projections, "target_projections": p.project(targets)}
    if len(targets) == 2:
        out["resflex"] = flexibility.flexibility_correlation(report["rmsd"], report["rmsf"])
        out["resflex_mean_structure"] = flexibility.flexibility_correlation(report["rmsd"], ms.rmsf)
        out["displacement_overlap"] = p.displacement_overlap(targets[0], targets[1])
    return out


def dssp_report(samples_path, target_paths, keep=None) -> dict:
    """The --dssp block: the files read again as N / CA / C backbones (`keep`: the analysed subset of the samples' models), O inferred;
    the proline flags come from the residue names of the samples' first model."""
    backbones = load_coords(Path(samples_path), max_n_model=None, ca_only=False, verbose=False)
    if keep is not None:
        backbones = backbones[keep]
    sequence = None
    if Path(samples_path).name.endswith(".pdb") and Path(samples_path).is_file():
        sequence = read_pdb_backbone(samples_path)[0]
        if len(sequence) != backbones.shape[1]:
            sequence = None
    targets = [load_coords(Path(p), max_n_model=None, ca_only=False, verbose=False)[0] for p in target_paths]
    return secondary.report(secondary.dssp(backbones, sequence), [secondary.dssp(t, sequence) for t in targets])


def torsions_report(samples_path, target_paths, keep=None, bins: int = 36) -> dict:
    """The --torsions block: the files read again as N / CA / C backbones (`keep`: the analysed subset of the samples' models)."""
    backbones = load_coords(Path(samples_path), max_n_model=None, ca_only=False, verbose=False)
    if keep is not None:
        backbones = backbones[keep]
    targets = [load_coords(Path(p), max_n_model=None, ca_only=False, verbose=False)[0] for p in target_paths]
    return torsions.report(backbones, targets, bins)


def load_ca(samples_path, target_paths, max_models: int = 100, seed: int = 0):
    """-> the analysed samples (n, L, 3), the targets [(L, 3)], the number of models in the file and the positions of the analysed ones."""
    samples = load_coords(Path(samples_path), max_n_model=None, verbose=False)
    n_all, keep = len(samples), np.arange(len(samples))
    if len(samples) > max_models:
        keep = np.sort(np.random.default_rng(seed).choice(len(samples), max_models, replace=False))
        samples = samples[keep]
    targets = [load_coords(Path(p), max_n_model=None, verbose=False)[0] for p in target_paths]
    for p, t in zip(target_paths, targets):
        if t.shape[0] != samples.shape[1]:
            raise ValueError(f"{p} has {t.shape[0]} residues, the samples {samples.shape[1]}: the correspondence is residue to residue")
    return samples, targets, n_all, keep


def contacts_report(samples_path, target_paths, max_models: int = 100, seed: int = 0, cutoff: float = 8.0, min_sep: int = 3) -> dict:
    """The --contacts block, on the samples analyze() takes for the same max_models and seed."""
    samples, targets, _, _ = load_ca(samples_path, target_paths, max_models, seed)
    return contacts.report(samples, np.stack(targets), cutoff, min_sep)


def shape_report(samples_path, target_paths, max_models: int = 100, seed: int = 0, pr_bins: int = 100) -> dict:
    """The --shape block, on the samples analyze() takes for the same max_models and seed."""
    samples, targets, _, _ = load_ca(samples_path, target_paths, max_models, seed)
    return shape.report(samples, np.stack(targets), pr_bins)


def saxs_report(samples_path, target_paths, max_models: int = 100, seed: int = 0, q_max: float = 0.5, points: int = 51, data=None) -> dict:
    """The --saxs block, on the same samples; data: the path of a q, I, sigma file or None."""
    samples, _, _, _ = load_ca(samples_path, target_paths, max_models, seed)
    return shape.saxs_report(samples, q_max, points, None if data is None else shape.read_saxs_data(data))


def sasa_report(samples_path, target_paths, keep=None, points: int = 96, probe: float = 1.4, threshold: float = 0.2) -> dict:
    """The --sasa block: the files read again as N / CA / C backbones (`keep`: the analysed subset of the samples' models), O inferred."""
    backbones = load_coords(Path(samples_path), max_n_model=None, ca_only=False, verbose=False)
    if keep is not None:
        backbones = backbones[keep]
    targets = [load_coords(Path(p), max_n_model=None, ca_only=False, verbose=False)[0] for p in target_paths]
    return accessibility.report(backbones, targets, points, probe, threshold)


def _trajectory(trajectory_path, samples, chunk: int):
    """-> the trajectory and the frame pairs it is uploaded in at a time: a .npy (n, L, 3) array, opened memory-mapped, or a multi-MODEL
    PDB (whole)."""
    if str(trajectory_path).endswith(".npy"):
        trajectory, chunk_frames = np.load(trajectory_path, mmap_mode="r"), int(chunk)
    else:
        trajectory, chunk_frames = load_coords(Path(trajectory_path), max_n_model=None, verbose=False), None
    if trajectory.ndim != 3 or trajectory.shape[1:] != samples.shape[1:]:
        raise ValueError(f"{trajectory_path} holds {trajectory.shape}, the samples {samples.shape[1:]} per frame: the correspondence is residue to residue")
    return trajectory, chunk_frames


def tica_report(samples_path, target_paths, trajectory_path, max_models: int = 100, seed: int = 0, lagtime: int = 20, dim: int = 2,
                lagtimes=None, chunk: int = 65536) -> dict:
    """The --tica block, on the samples analyze() takes for the same max_models and seed; the trajectory: a .npy (n, L, 3) array, opened
    memory-mapped and uploaded `chunk` pairs at a time, or a multi-MODEL PDB."""
    samples, targets, _, _ = load_ca(samples_path, target_paths, max_models, seed)
    trajectory, chunk_frames = _trajectory(trajectory_path, samples, chunk)
    return kinetics.report(trajectory, samples, np.stack(targets), lagtime, dim, lagtimes, chunk_frames=chunk_frames)


def msm_report(samples_path, target_paths, trajectory_path, max_models: int = 100, seed: int = 0, lagtime: int = 20, dim: int = 2,
               n_states: int = 100, msm_lagtime=None, metastable: int = 2, msm_seed: int = 0, chunk: int = 65536) -> dict:
    """The --msm block, on the same samples and the same trajectory as the --tica block."""
    samples, targets, _, _ = load_ca(samples_path, target_paths, max_models, seed)
    trajectory, chunk_frames = _trajectory(trajectory_path, samples, chunk)
    return states.report(trajectory, samples, np.stack(targets), lagtime, dim, n_states, msm_lagtime, metastable, msm_seed, chunk_frames=chunk_frames)


def compare_report(samples_path, target_paths, trajectory_path, max_models: int = 100, seed: int = 0, ref: str = "target", modes: int = 2,
                   chunk: int = 65536) -> dict:
    """The --compare block, on the samples analyze() takes for the same max_models and seed and the trajectory --tica takes; ref:
    "target" (the first target) or "first" (the trajectory's first frame) is the structure both ensembles are superposed on."""
    samples, targets, _, _ = load_ca(samples_path, target_paths, max_models, seed)
    trajectory, chunk_frames = _trajectory(trajectory_path, samples, chunk)
    return covariance.compare(trajectory, samples, targets[0] if ref == "target" else None, modes, chunk_frames, targets=np.stack(targets))


def coverage_report(samples_path, target_paths, trajectory_path, max_models: int = 100, seed: int = 0, cutoffs=(1.0, 2.0, 3.0),
                    chunk: int = 65536) -> dict:
    """The --coverage block, on the samples analyze() takes for the same max_models and seed and the trajectory --tica takes."""
    samples, targets, _, _ = load_ca(samples_path, target_paths, max_models, seed)
    trajectory, chunk_frames = _trajectory(trajectory_path, samples, chunk)
    cutoffs = tuple(float(c) for c in cutoffs)
    select = np.isfinite(samples[0]).all(-1) & np.isfinite(np.asarray(trajectory[0])).all(-1) & np.isfinite(np.stack(targets)).all((0, 2))
    cov = neighbours.coverage(samples, trajectory, cutoffs, select=select, chunk_frames=chunk_frames)
    by_target = neighbours.nearest(np.stack(targets), samples, select)
    in_trajectory = neighbours.nearest(np.stack(targets), trajectory, select, chunk_frames=chunk_frames)
    out = {"cutoffs": list(cutoffs), "n_residues": int(select.sum()), "reflection": False}
    out.update({k: cov[k] for k in ("recall", "precision", "mat_r", "mat_p", "nearest_frame", "nearest_frame_rmsd", "novel", "samples_used",
                                    "samples_dropped", "frames_used", "frames_dropped")})
    out["targets"] = {"nearest_sample": by_target.index_a, "nearest_sample_rmsd": by_target.rmsd_a,
                      "nearest_frame": in_trajectory.index_a, "nearest_frame_rmsd": in_trajectory.rmsd_a}
    out["mean_pairwise_rmsd"] = {"samples": neighbours.mean_pairwise_rmsd(samples, select),
                                 "trajectory": neighbours.mean_pairwise_rmsd(trajectory, select, chunk_frames=chunk_frames)}
    return out


def analyze(samples_path, target_paths, max_models: int = 100, seed: int = 0, lddt: bool = False, plddt_scale: float = 1.0,
            flex: bool = False, pca_components: int = 3, dssp: bool = False) -> dict:
    samples, targets, n_all, keep = load_ca(samples_path, target_paths, max_models, seed)
    if len(targets) == 2:
        report = ensemble.apo_report(samples, targets[0], targets[1])
    else:
        best_tm, best_rmsd = ensemble.tm_n_ensemble(samples, np.stack(targets), max_n_model=max_models, rng=seed)
        report = {"best_tm": best_tm, "best_rmsd": best_rmsd, "TM-ens": float(np.mean(best_tm)), "RMSD-ens": float(np.mean(best_rmsd)),
                  "TM-div": ensemble.tm_diversity(samples)}
    if lddt:
        plddt = None
        if Path(samples_path).name.endswith(".pdb") and Path(samples_path).is_file():
            b = read_pdb_bfactors(samples_path)
            if b.shape[0] == n_all:
                b = b[keep]
            if b.shape == samples.shape[:2] and np.any(b != 0):        # all zero: written without a confidence
                plddt = b
        report.update(lddt_report(samples, np.stack(targets), plddt, plddt_scale))
    if flex:
        report["flex"] = flex_report(samples, np.stack(targets), report, pca_components)
    if dssp:
        report["dssp"] = dssp_report(samples_path, target_paths, keep)
    return report


def parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--samples", required=True, help="multi-MODEL PDB of the sampled ensemble")
    ap.add_argument("--targets", required=True, nargs="+", help="target structures, one PDB each (same sequence as the samples)")
    ap.add_argument("--output", required=True, help="output directory")
    ap.add_argument("--max_models", type=int, default=100)
    ap.add_argument("--seed", type=int, default=0, help="seed of the down-sampling to --max_models")
    ap.add_argument("--lddt", action="store_true", help="add the CA-lDDT scores (no superposition) and the pLDDT agreement")
    ap.add_argument("--plddt_scale", type=float, default=1.0, help="the samples' B-factors divided by this are pLDDT in [0, 1]")
    ap.add_argument("--flex", action="store_true", help="add the mean structure, RMSF, pairwise RMSF, PCA and the ResFlex correlations")
    ap.add_argument("--pca_components", type=int, default=3, help="modes of the --flex PCA")
    ap.add_argument("--dssp", action="store_true", help="add the DSSP states, the three-state propensities and the agreement with the targets")
    ap.add_argument("--contacts", action="store_true", help="add the contact map, the fractions of native contacts Q and the scaling profile")
    ap.add_argument("--contact_cutoff", type=float, default=8.0, help="CA-CA distance below which a pair is a contact (Angstrom)")
    ap.add_argument("--contact_min_sep", type=int, default=3, help="the smallest sequence separation |a - b| of a contact")
    ap.add_argument("--torsions", action="store_true", help="add the backbone torsions: Ramachandran statistics, regions, geometry, agreement with the targets")
    ap.add_argument("--rama_bins", type=int, default=36, help="cells per axis of the --torsions Ramachandran maps (1 to 72)")
    ap.add_argument("--shape", action="store_true", help="add the gyration tensor's shape descriptors, Ree, Dmax, Rh and p(r)")
    ap.add_argument("--pr_bins", type=int, default=100, help="cells of the --shape pair-distance distribution")
    ap.add_argument("--saxs", action="store_true", help="add the Debye SAXS profile of the samples, its Guinier Rg and Kratky curve")
    ap.add_argument("--saxs_qmax", type=float, default=0.5, help="the largest q of the --saxs profile (1 / Angstrom)")
    ap.add_argument("--saxs_points", type=int, default=51, help="values of q of the --saxs profile, from 0 to --saxs_qmax")
    ap.add_argument("--saxs_data", default=None, help="a measured curve (columns q, I, sigma): evaluate at its q and add the reduced chi^2")
    ap.add_argument("--sasa", action="store_true", help="add the backbone's solvent accessibility: areas, relative exposure, exposed frequency")
    ap.add_argument("--sasa_points", type=int, default=96, help="points on every atom's sphere of the --sasa point test (1 to 1024)")
    ap.add_argument("--sasa_probe", type=float, default=1.4, help="probe radius of --sasa (Angstrom)")
    ap.add_argument("--sasa_threshold", type=float, default=0.2, help="relative exposure above which --sasa calls a residue exposed")
    ap.add_argument("--tica", action="store_true", help="add the slow coordinates of --trajectory: TICA eigenvalues, timescales, projections, JS")
    ap.add_argument("--trajectory", default=None, help="the MD trajectory --tica is fitted on: a .npy (n, L, 3) CA array or a multi-MODEL PDB")
    ap.add_argument("--lagtime", type=int, default=20, help="lag time of --tica, in frames of the trajectory")
    ap.add_argument("--tica_dim", type=int, default=2, help="components of the --tica model (1 to 16)")
    ap.add_argument("--lagtimes", type=int, nargs="+", default=None, help="lag times of the --tica implied-timescale table")
    ap.add_argument("--tica_chunk", type=int, default=65536, help="frame pairs of a .npy --trajectory uploaded at a time")
    ap.add_argument("--msm", action="store_true", help="add the metastable states of --trajectory: k-means on the TICA coordinates, a Markov state model, populations")
    ap.add_argument("--msm_states", type=int, default=100, help="microstates (k-means centres) of --msm (1 to 4096)")
    ap.add_argument("--msm_lagtime", type=int, default=None, help="lag time of the --msm transition counts, in frames (default: --lagtime)")
    ap.add_argument("--msm_metastable", type=int, default=2, help="metastable sets of --msm (below 2: none)")
    ap.add_argument("--msm_seed", type=int, default=0, help="seed of the kmeans++ initialisation of --msm")
    ap.add_argument("--compare", action="store_true", help="add the Cartesian comparison with --trajectory: per-residue W2, RMWD, PCA W2, RMSIP, DCCM and RMSF correlations")
    ap.add_argument("--compare_ref", choices=("target", "first"), default="target", help="the structure --compare superposes both ensembles on: the first target or the trajectory's first frame")
    ap.add_argument("--compare_modes", type=int, default=2, help="modes of the --compare PCA distances and projections (1 to 16)")
    ap.add_argument("--coverage", action="store_true", help="add the nearest-neighbour coverage of --trajectory by the samples: recall, precision, nearest pairs, mean pairwise RMSD")
    ap.add_argument("--coverage_cutoffs", type=float, nargs="+", default=[1.0, 2.0, 3.0], help="RMSD cutoffs of --coverage (Angstrom, at most 8)")
    return ap


def main(argv=None) -> Path:
    ap = parser()
    args = ap.parse_args(argv)
    if args.msm and not (args.tica and args.trajectory):
        ap.error("--msm needs --tica --trajectory REF")
    if args.compare and not args.trajectory:
        ap.error("--compare needs --trajectory REF")
    if args.coverage and not args.trajectory:
        ap.error("--coverage needs --trajectory REF")
    report = analyze(args.samples, args.targets, args.max_models, args.seed, args.lddt, args.plddt_scale, args.flex, args.pca_components,
                     args.dssp)
    if args.contacts:
        report["contacts"] = contacts_report(args.samples, args.targets, args.max_models, args.seed, args.contact_cutoff, args.contact_min_sep)
    if args.torsions:
        keep = load_ca(args.samples, args.targets, args.max_models, args.seed)[3]
        report["torsions"] = torsions_report(args.samples, args.targets, keep, args.rama_bins)
    if args.shape:
        report["shape"] = shape_report(args.samples, args.targets, args.max_models, args.seed, args.pr_bins)
    if args.saxs or args.saxs_data:
        report["saxs"] = saxs_report(args.samples, args.targets, args.max_models, args.seed, args.saxs_qmax, args.saxs_points, args.saxs_data)
    if args.sasa:
        keep = load_ca(args.samples, args.targets, args.max_models, args.seed)[3]
        report["sasa"] = sasa_report(args.samples, args.targets, keep, args.sasa_points, args.sasa_probe, args.sasa_threshold)
    if args.tica:
        if not args.trajectory:
            raise SystemExit("--tica needs --trajectory REF")
        report["tica"] = tica_report(args.samples, args.targets, args.trajectory, args.max_models, args.seed, args.lagtime, args.tica_dim,
                                     args.lagtimes, args.tica_chunk)
    if args.msm:
        report["msm"] = msm_report(args.samples, args.targets, args.trajectory, args.max_models, args.seed, args.lagtime, args.tica_dim,
                                   args.msm_states, args.msm_lagtime, args.msm_metastable, args.msm_seed, args.tica_chunk)
    if args.compare:
        report["compare"] = compare_report(args.samples, args.targets, args.trajectory, args.max_models, args.seed, args.compare_ref,
                                           args.compare_modes, args.tica_chunk)
    if args.coverage:
        report["coverage"] = coverage_report(args.samples, args.targets, args.trajectory, args.max_models, args.seed, args.coverage_cutoffs,
                                             args.tica_chunk)
    out = Path(args.output)
    out.mkdir(parents=True, exist_ok=True)
    path = out / f"{Path(args.samples).stem}.ensemble.json"
    path.write_text(json.dumps({k: _jsonable(v) for k, v in report.items()}, indent=1) + "\n")
    print(path)
    return path


if __name__ == "__main__":
    main()

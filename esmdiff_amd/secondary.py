"""Secondary structure of an ensemble on the device: the eight DSSP states of Kabsch & Sander 1983 per residue and structure, their
three-state reduction, per-residue propensities, and the agreement of samples with target structures.  DESIGN.md §3.22 states the
definition; the kernels are csrc/dssp.hip, held exactly to tests/dssp_ref.py.  [DSSP-RECALL]: the `mkdssp` program is not pinned —
no beta-bulge promotion, no rounding of energies, the classic priority H > E, B > G > I > T > S, no sheet labels, no accessibility.

  dssp            backbones (N, CA, C and O; O inferred when absent) -> SecondaryStructure
  ss_agreement    Q3 of every sample against one target, and per residue the share of samples in the target's class
  switch_residues the residues whose three-state class differs between two targets, with the ensemble's share in each class
  report          the "dssp" block of `python -m esmdiff_amd.analyze_ensemble --dssp` and `python -m esmdiff_amd.secondary_structure`

Inputs follow esmdiff_amd/ensemble.py: Angstrom, arrays, tensors or a PDB path; residues with NaN backbone atoms are absent, `mask`
(n, L) removes more.  A file's own O atoms are NOT read: samples are written with the inferred O (pdbio.write_backbone_pdb), and
placing it the same way on targets treats both alike.  With a crystal structure's own O a borderline turn can differ (BPTI: residues
25-27 are GGG with the file's O and TTT with the inferred one, 0.13 A apart in RMSD).  There is no CPU fallback."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import pairs

LEGEND = "-STIGBEH"                      # code -> letter: loop, bend, turn, pi-helix, 3-10 helix, bridge, strand, alpha-helix
REDUCED_LEGEND = "HEC"                   # reduced code -> letter: helix (H, G, I), strand (E, B), coil (the rest)
REDUCED_NAMES = ("helix", "strand", "coil")
_REDUCE = np.array([2, 2, 2, 0, 0, 1, 1, 0], np.uint8)
_O_LOCAL = (0.6240, -1.0613, 0.0103)     # pdbio._O_LOCAL


def infer_oxygen(backbone) -> np.ndarray:
    """pdbio.infer_oxygen in float64 over any number of leading axes: (..., L, >=3, 3) N / CA / C -> (..., L, 3), the carbonyl O as a
    fixed vector in the frame of CA_i -> C_i and N_{i+1}; NaN for the last residue and wherever one of the three atoms is missing."""
    x = np.asarray(backbone, np.float64)
    out = np.full(x.shape[:-2] + (3,), np.nan)
    if x.shape[-3] < 2:
        return out
    ca, c, n_next = x[..., :-1, 1, :], x[..., :-1, 2, :], x[..., 1:, 0, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        e0 = c - ca
        e0 = e0 / np.linalg.norm(e0, axis=-1, keepdims=True)
        v = n_next - c
        e1 = v - e0 * np.sum(e0 * v, axis=-1, keepdims=True)
        e1 = e1 / np.linalg.norm(e1, axis=-1, keepdims=True)
        e2 = np.cross(e0, e1)
        out[..., :-1, :] = c + _O_LOCAL[0] * e0 + _O_LOCAL[1] * e1 + _O_LOCAL[2] * e2
    return out


def backbone_array(backbone) -> np.ndarray:
    """A PDB path (N / CA / C of every MODEL), an array or a tensor, (L, A, 3) or (n, L, A, 3) with A = 4 (N, CA, C, O) or A = 3 (O is
    inferred) -> float64 (n, L, 4, 3) on the host."""
    return pairs.atoms(backbone, (3, 4), infer_o=True, what="backbones should be (n, L, 4, 3) N / CA / C / O or (n, L, 3, 3) N / CA / C")


def reduce_codes(codes) -> np.ndarray:
    """Eight states -> three: 0 helix (H, G, I), 1 strand (E, B), 2 coil."""
    return _REDUCE[np.asarray(codes)]


def _fractions(counts: np.ndarray) -> np.ndarray:
    total = counts.sum(-1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(total > 0, counts / total, np.nan)


@dataclass
class SecondaryStructure:
    codes: np.ndarray                        # (n, L) uint8, indices into LEGEND; 0 where the residue is absent
    present: np.ndarray                      # (n, L) bool: not masked, N / CA / C resolved
    counts: np.ndarray                       # (L, 8) structures in which the residue is present and has the code
    acceptor: Optional[np.ndarray] = None    # (n, L, 2) int32: the acceptors of residue j's N-H, -1 for none
    energy: Optional[np.ndarray] = None      # (n, L, 2) kcal/mol, 0.0 for none

    @classmethod
    def from_codes(cls, codes, present=None) -> "SecondaryStructure":
        """From codes alone (n, L) or (L,): the counts are taken on the host."""
        codes = np.atleast_2d(np.asarray(codes, np.uint8))
        present = np.ones(codes.shape, bool) if present is None else np.atleast_2d(np.asarray(present, bool))
        assert present.shape == codes.shape and codes.max(initial=0) < 8
        counts = np.stack([((codes == c) & present).sum(0) for c in range(8)], axis=1).astype(np.int32)
        return cls(np.where(present, codes, 0).astype(np.uint8), present, counts)

    @property
    def strings(self):
        return ["".join(LEGEND[c] for c in row) for row in self.codes]

    @property
    def n_present(self) -> np.ndarray:
        return self.counts.sum(1)

    def reduced(self) -> np.ndarray:
        """(n, L) uint8, indices into REDUCED_LEGEND."""
        return reduce_codes(self.codes)

    def reduced_counts(self) -> np.ndarray:
        return np.stack([self.counts[:, _REDUCE == k].sum(1) for k in range(3)], axis=1)

    def propensity(self, reduced: bool = True) -> np.ndarray:
        """(L, 3) (helix, strand, coil) or (L, 8) fractions of the structures that have the residue; NaN where none has."""
        return _fractions(self.reduced_counts() if reduced else self.counts)

    def content(self, reduced: bool = True) -> dict:
        """The share of each state over all present residues of all structures (NaN for an ensemble without residues)."""
        c = (self.reduced_counts() if reduced else self.counts).sum(0)
        return dict(zip(REDUCED_NAMES if reduced else LEGEND, (float(v) for v in _fractions(c[None])[0])))


def dssp(backbone, sequence: Optional[str] = None, mask=None) -> SecondaryStructure:
    """The DSSP states of every structure.  backbone: see backbone_array; sequence: one-letter codes, sets the no-donor flag of
    prolines (None: every residue's N carries an H); mask (n, L) or (L,): residues to leave out."""
    pairs.need_device("esmdiff_amd.secondary")
    x = backbone_array(backbone)
    n, L = x.shape[:2]
    given, mk = pairs.given_mask(mask, n, L)
    no_donor = None
    if sequence is not None:
        assert len(sequence) == L, f"a sequence of {len(sequence)} residues for backbones of {L}"
        no_donor = torch.as_tensor(np.array([c == "P" for c in sequence], np.uint8), device="cuda")
    X = torch.as_tensor(x, device="cuda")
    ss, counts, acceptor, energy = pairs.dssp(X, mk, no_donor)
    present = given & np.isfinite(x[:, :, :3]).all((2, 3))
    return SecondaryStructure(ss.cpu().numpy(), present, counts.cpu().numpy(), acceptor.cpu().numpy(), energy.cpu().numpy())


def _as_ss(x) -> SecondaryStructure:
    return x if isinstance(x, SecondaryStructure) else dssp(x)


def ss_agreement(samples, target) -> dict:
    """samples, target: SecondaryStructure, or anything `dssp` takes (the target's first structure is used) ->
      q3           (n,) the share of residues present in both whose three-state class equals the target's (NaN when there is none)
      q3_mean, q3_best, best_model
      per_residue  (L,) the share of the samples having the residue that are in the target's class there (NaN where the target lacks
                   the residue or no sample has it)"""
    s, t = _as_ss(samples), _as_ss(target)
    assert s.codes.shape[1] == t.codes.shape[1], f"{s.codes.shape[1]} and {t.codes.shape[1]} residues: the correspondence is residue to residue"
    same = s.reduced() == t.reduced()[0][None]
    both = s.present & t.present[0][None]
    with np.errstate(invalid="ignore", divide="ignore"):
        q3 = np.where(both.sum(1) > 0, (same & both).sum(1) / both.sum(1), np.nan)
        per_residue = np.where(both.sum(0) > 0, (same & both).sum(0) / both.sum(0), np.nan)
    some = np.isfinite(q3)
    best = int(np.where(some, q3, -1.0).argmax()) if some.any() else -1
    return {"q3": q3, "q3_mean": float(q3[some].mean()) if some.any() else float("nan"),
            "q3_best": float(q3[best]) if best >= 0 else float("nan"), "best_model": best, "per_residue": per_residue}


def switch_residues(samples, target1, target2) -> list:
    """The residues present in both targets whose three-state class differs between them, each as {"residue": index from 0,
    "classes": the two letters of REDUCED_LEGEND, "share": the fraction of samples (having the residue) in target 1's class and in
    target 2's; None where no sample has the residue}."""
    s, a, b = _as_ss(samples), _as_ss(target1), _as_ss(target2)
    ra, rb, prop = a.reduced()[0], b.reduced()[0], s.propensity()
    out = []
    for l in np.nonzero(a.present[0] & b.present[0] & (ra != rb))[0]:
        share = [None if np.isnan(prop[l, r]) else float(prop[l, r]) for r in (ra[l], rb[l])]
        out.append({"residue": int(l), "classes": [REDUCED_LEGEND[ra[l]], REDUCED_LEGEND[rb[l]]], "share": share})
    return out


def report(samples, targets=()) -> dict:
    """The "dssp" block: the legends, the samples' strings, counts (L, 8), three-state propensity (L, 3) and content, and per target
    its string and ss_agreement; with exactly two targets also switch_residues."""
    s = _as_ss(samples)
    ts = [_as_ss(t) for t in targets]
    out = {"legend": LEGEND, "reduced_legend": REDUCED_LEGEND, "strings": s.strings, "counts": s.counts, "propensity": s.propensity(),
           "content": s.content()}
    if ts:
        out["targets"] = [{"string": t.strings[0], "agreement": ss_agreement(s, t)} for t in ts]
    if len(ts) == 2:
        out["switch_residues"] = switch_residues(s, ts[0], ts[1])
    return out

#!/usr/bin/env python3
"""Backbones with their own carbonyl O for the secondary-structure tests (tests/dssp_ref.py, tests/test_dssp_cpu.py,
tests/test_gpu_dssp.py): three of the reference's target files, read as data.

Runs only in the build container (needs /root/reference/data/targets).  Fixture: tests/golden/g14_backbones.npz — per chain
`<name>_xyz` float64 (L, 4, 3), the ATOM records' N, CA, C, O (first alternate location; NaN where an atom is missing), and
`<name>_seq`, the one-letter sequence.  Coordinates and sequences only.
"""
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
TARGETS = Path("/root/reference/data/targets")
FILES = {"bpti": "bpti/bpti.pdb", "1fmf_A": "apo/1fmf.A.pdb", "1c54_A": "apo/1c54.A.pdb"}
THREE_TO_ONE = {
    "ALA": "A", "ARG": "R", "ASN": "N", "ASP": "D", "CYS": "C", "GLN": "Q", "GLU": "E", "GLY": "G", "HIS": "H",
    "ILE": "I", "LEU": "L", "LYS": "K", "MET": "M", "PHE": "F", "PRO": "P", "SER": "S", "THR": "T", "TRP": "W",
    "TYR": "Y", "VAL": "V",
}
ATOMS = {"N": 0, "CA": 1, "C": 2, "O": 3}


def read(path):
    seq, xyz, index, first_alt = [], [], {}, {}
    for line in path.read_text().splitlines():
        if line.startswith("ENDMDL"):
            break
        if not line.startswith("ATOM"):
            continue
        key = (line[21], line[22:27])
        if line[16] != " " and first_alt.setdefault(key, line[16]) != line[16]:
            continue
        if key not in index:
            index[key] = len(seq)
            seq.append(THREE_TO_ONE.get(line[17:20].strip(), "X"))
            xyz.append(np.full((4, 3), np.nan))
        a = ATOMS.get(line[12:16].strip())
        if a is not None and np.isnan(xyz[index[key]][a]).all():
            xyz[index[key]][a] = (float(line[30:38]), float(line[38:46]), float(line[46:54]))
    return "".join(seq), np.stack(xyz)


def main():
    out = {}
    for name, rel in FILES.items():
        seq, xyz = read(TARGETS / rel)
        out[f"{name}_xyz"], out[f"{name}_seq"] = xyz, np.array(seq)
        print(name, xyz.shape, int(np.isnan(xyz).any((1, 2)).sum()), "residues with a missing atom", seq)
    np.savez_compressed(HERE / "g14_backbones.npz", **out)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Golden vectors for the superposition kernels (esmdiff_amd/csrc/superpose.hip), produced by the code the REFERENCE's
evaluations run:

  * /root/reference/slm/utils/geo_utils.py squared_deviation :58-88 ('none' and 'rmsd') and _find_rigid_alignment :91-122 —
    R = V U^T from torch.svd with NO determinant correction (a mirror image aligns with RMSD 0);
  * scipy.spatial.transform.Rotation.align_vectors exactly as analysis/apo_analysis.py get_structures :201-206 uses it: each
    structure centred with nanmean over its own resolved residues, a rotation-only fit on the residues resolved in both, the
    per-residue distances of :235 / :257 taken afterwards.  (apo_analysis.py itself imports Bio, pandas and seaborn at module
    level; the five lines are restated here around scipy's own function, which does the arithmetic.)

Runs only in the build container (needs /root/reference and scipy; geo_utils is imported through make_goldens' stubs).
Fixture: tests/golden/g13_superposition.npz — numeric arrays only.  Cases are seeded random-walk CA chains (3.8 A steps) with
rigidly moved copies: noise 0 / 1e-3 / 0.3 / 2 A, a mirror image, a pair with NaN-masked residues (different ones in the two
structures), a planar chain, L = 2.
"""
import sys
import warnings
from pathlib import Path

import numpy as np
import torch
from scipy.spatial.transform import Rotation

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import make_goldens  # noqa: F401,E402  (inert stubs for the packages slm.utils' __init__ drags in; /root/reference on sys.path)
from slm.utils import geo_utils as G  # noqa: E402

PLAIN, MIRROR, MASKED, PLANAR, TWO = range(5)


def random_rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def chain(rng, L, planar=False):
    step = rng.normal(size=(L, 3))
    if planar:
        step[:, 2] = 0
    return np.cumsum(3.8 * step / np.linalg.norm(step, axis=-1, keepdims=True), axis=0)


def get_structures_tail(struct1, struct2):
    """analysis/apo_analysis.py:201-208 on two NaN-padded (L, 3) arrays -> struct1, struct2 (as returned), rot."""
    struct1 = struct1 - np.nanmean(struct1, 0)
    struct2 = struct2 - np.nanmean(struct2, 0)
    mask = ~np.isnan(struct1[:, 0]) & ~np.isnan(struct2[:, 0])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # "not uniquely defined" on the planar / two-residue cases
        rot = Rotation.align_vectors(struct1[mask], struct2[mask])[0].as_matrix()
    return struct1, struct2 @ rot.T, rot


def main():
    rng = np.random.default_rng(20261017)
    spec = [(PLAIN, 48, 0.0), (PLAIN, 48, 1e-3), (PLAIN, 48, 0.3), (PLAIN, 37, 2.0), (MIRROR, 48, 0.0), (MASKED, 40, 0.3),
            (PLANAR, 30, 0.3), (TWO, 2, 0.3)]
    out = {"kind": np.array([s[0] for s in spec]), "noise": np.array([s[2] for s in spec])}
    for c, (kind, L, noise) in enumerate(spec):
        tgt = chain(rng, L, planar=kind == PLANAR)
        eps = rng.normal(size=(L, 3)) * noise
        if kind == PLANAR:
            eps[:, 2] = 0
        src = tgt + eps
        if kind == MIRROR:
            src = src * np.array([1.0, 1.0, -1.0])
        src = src @ random_rotation(rng).T + rng.normal(size=3) * 20
        if kind == MASKED:
            src[[3, 4, 17]] = np.nan
            tgt[[17, 30, 31, 39]] = np.nan
        ok = ~np.isnan(src[:, 0]) & ~np.isnan(tgt[:, 0])
        s, t_ = torch.as_tensor(src[ok])[None], torch.as_tensor(tgt[ok])[None]
        sd = np.full(L, np.nan)
        sd[ok] = G.squared_deviation(s, t_, reduction="none")[0].numpy()
        R, t = G._find_rigid_alignment(s, t_)
        s1, s2, rot = get_structures_tail(src, tgt)
        out.update({f"src_{c}": src, f"tgt_{c}": tgt, f"sd_{c}": sd,
                    f"rmsd_{c}": G.squared_deviation(s, t_, reduction="rmsd")[0].numpy(),
                    f"rmsd_np_entry_{c}": G.squared_deviation(src[ok][None], tgt[ok][None], reduction="rmsd")[0],
                    f"R_{c}": R[0].numpy(), f"t_{c}": t[0].numpy(),
                    f"scipy_rot_{c}": rot, f"scipy_dist_{c}": np.square(s1 - s2).sum(-1) ** 0.5})
        print(c, kind, L, noise, "rmsd(reflection allowed)", float(out[f"rmsd_{c}"]),
              "rmsd(proper, scipy)", float(np.sqrt(np.nanmean(out[f"scipy_dist_{c}"] ** 2))))
    np.savez(HERE / "g13_superposition.npz", **out)


if __name__ == "__main__":
    main()

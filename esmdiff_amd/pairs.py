"""The device side of the all-pairs layer: input preparation and one function per C entry of csrc/superpose.hip, csrc/lddt.hip,
csrc/cluster.hip, csrc/flex.hip, csrc/dssp.hip, csrc/contacts.hip, csrc/torsions.hip, csrc/shape.hip, csrc/sasa.hip, csrc/lagged.hip, csrc/msm.hip, csrc/aligned.hip and csrc/rmsd_nn.hip.  Each function owns its entry's argument list, output allocation and error text; tensors on the device in, tensors
on the device out, no host transfer.  esmdiff_amd/ensemble.py, esmdiff_amd/clustering.py and esmdiff_amd/flexibility.py are the
host-facing layers above it.  The frame-wise layers (secondary, torsions, accessibility) share one input stage here: need_device,
atoms and given_mask; every frame-wise entry below asserts its input through _frames.
Row blocks are contiguous slices (A[r0:r1]): a slice carries its own pointer, dtype and shape.  There is no CPU fallback."""
from __future__ import annotations

import ctypes
import os
from pathlib import Path
from typing import Optional

import numpy as np
import torch

from . import _native as N

LDDT_R0 = 15.0
LDDT_THRESHOLDS = (0.5, 1.0, 2.0, 4.0)


def need_device(what: str):
    """The one refusal of a host without the device; what: the module or function that was called."""
    if not torch.cuda.is_available():
        raise RuntimeError(f"{what} needs an MI355X (gfx950); there is no CPU fallback")


def coords(x, what: str = "coords") -> torch.Tensor:
    """A path (pdbio.load_coords), an array or a tensor -> float64 (n, L, 3) on the device."""
    need_device("esmdiff_amd.ensemble")
    if isinstance(x, (str, os.PathLike)):
        from .pdbio import load_coords
        x = load_coords(Path(x), max_n_model=None, verbose=False)
    t = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))
    if t.dim() == 2:
        t = t[None]
    if t.dim() != 3 or t.shape[-1] != 3 or t.shape[0] == 0 or t.shape[1] == 0:
        raise AssertionError(f"{what} should be (n, L, 3) CA coordinates, got {tuple(t.shape)}")
    return t.to(device="cuda", dtype=torch.float64).contiguous()


def valid_mask(t: torch.Tensor, mask) -> Optional[torch.Tensor]:
    """u8 (n, L): resolved (no NaN coordinate) and not masked by the caller; None when every residue is valid."""
    ok = ~torch.isnan(t).any(-1)
    if mask is not None:
        m = torch.as_tensor(np.asarray(mask) if not torch.is_tensor(mask) else mask).to("cuda").bool()
        if m.dim() == 1:
            m = m[None]
        assert m.shape == ok.shape, f"mask {tuple(m.shape)} does not match the coordinates {tuple(ok.shape)}"
        ok = ok & m
    return None if bool(ok.all()) else ok.to(torch.uint8).contiguous()


def pair_args(a, b, mask_a, mask_b):
    """-> A, B, ma, mb as every function below takes them; b = None: B and mb are None, a against itself."""
    A = coords(a)
    ma = valid_mask(A, mask_a)
    if b is None:
        assert mask_b is None, "mask_b without b"
        return A, None, ma, None
    B = coords(b)
    assert B.shape[1] == A.shape[1], f"structures of different lengths: {A.shape[1]} and {B.shape[1]} (the correspondence is residue to residue)"
    return A, B, ma, valid_mask(B, mask_b)


def atoms(x, allowed, infer_o: bool = False, ca_traces: bool = False, what: str = "atoms should be (n, L, A, 3)") -> np.ndarray:
    """The input stage of the frame-wise layers (secondary, torsions, accessibility).  x: a PDB path (N / CA / C of every MODEL), an
    array or a tensor, (L, A, 3) or (n, L, A, 3) with A in `allowed` -> float64 (n, L, A, 3) on the host.  infer_o: A = 3 gains the
    inferred carbonyl O (secondary.infer_oxygen) and leaves as A = 4.  ca_traces: a 3-D input whose middle axis is no atom count (1, 3
    or 4) is (n, L, 3) CA traces and leaves as A = 1.  what: the text of the shape error, up to ", got"."""
    if isinstance(x, (str, os.PathLike)):
        from .pdbio import load_coords
        x = load_coords(Path(x), max_n_model=None, ca_only=False, verbose=False)
    x = np.asarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x, np.float64)
    if x.ndim == 3:
        x = x[:, :, None, :] if ca_traces and x.shape[1] not in (1, 3, 4) else x[None]
    if x.ndim != 4 or x.shape[2] not in allowed or x.shape[3] != 3 or x.shape[1] == 0:
        raise AssertionError(f"{what}, got {tuple(x.shape)}")
    if infer_o and x.shape[2] == 3:
        from .secondary import infer_oxygen
        x = np.concatenate([x, infer_oxygen(x)[:, :, None]], axis=2)
    return np.ascontiguousarray(x)


def given_mask(mask, n: int, L: int):
    """mask: (n, L) or (L,), an array or a tensor, or None -> the residues the caller gives as bool (n, L) on the host, and as u8 (n, L)
    on the device, None when all are given."""
    if mask is None:
        return np.ones((n, L), bool), None
    m = (mask.detach().cpu().numpy() if torch.is_tensor(mask) else np.asarray(mask)).astype(bool)
    given = np.broadcast_to(m[None] if m.ndim == 1 else m, (n, L)).copy()
    return given, None if given.all() else torch.as_tensor(given.astype(np.uint8), device="cuda")


def _p(t: Optional[torch.Tensor]):
    assert t is None or t.is_contiguous(), "a row block should be a contiguous slice"
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _sizes(A: torch.Tensor, B: Optional[torch.Tensor]):
    assert B is None or B.shape[1:] == A.shape[1:], f"structures of different lengths: {A.shape[1]} and {B.shape[1]}"
    return A.shape[0], (A if B is None else B).shape[0], A.shape[1]


def _frames(X, mask, last):
    """What every frame-wise entry asserts of its input: X is f64 (n, L) + last, where an entry of `last` is a size, a tuple of sizes
    or None (any: the entry itself refuses), and mask is u8 (n, L) or None -> n, L."""
    text = ", ".join("A" if d is None else " or ".join(map(str, d)) if isinstance(d, tuple) else str(d) for d in last)
    fits = X.dim() == 2 + len(last) and all(d is None or s in (d if isinstance(d, tuple) else (d,)) for s, d in zip(X.shape[2:], last))
    assert fits and X.dtype == torch.float64, f"f64 (n, L, {text}) frames, got {X.dtype} {tuple(X.shape)}"
    n, L = X.shape[:2]
    assert mask is None or (mask.dtype == torch.uint8 and tuple(mask.shape) == (n, L)), "the mask is u8 (n, L)"
    return n, L


def _new(shape, dtype=torch.float64) -> torch.Tensor:
    return torch.empty(shape, dtype=dtype, device="cuda")


def _check(entry: str, code: int, capacity=None, invalid=None):
    """An entry's return code -> RuntimeError; capacity / invalid: what -5 / -1 mean for that entry, functions called only then."""
    if code != 0:
        text = {-5: capacity, -1: invalid}.get(code)
        raise RuntimeError(text() if text else f"libesmdiff_hip {entry} failed ({code})")


def superpose(A, B, ma, mb, reflection: bool, want, out=None) -> dict:
    """One esmdiff_superpose_pairs launch -> {name: tensor} for the names in `want`: rmsd (n, m), sd (n, m, L), R (n, m, 3, 3),
    t (n, m, 3).  out: {name: tensor} to write into instead of allocating (a caller's row-block buffer)."""
    n, m, L = _sizes(A, B)
    shapes = {"rmsd": (n, m), "sd": (n, m, L), "R": (n, m, 3, 3), "t": (n, m, 3)}
    res = {k: out[k] if out and k in out else _new(shapes[k]) for k in want}
    assert all(tuple(v.shape) == shapes[k] and v.dtype == torch.float64 for k, v in res.items()), f"the launch writes f64 {shapes}"
    code = N.lib().esmdiff_superpose_pairs(_p(A), n, _p(B), m, L, _p(ma), _p(mb), int(bool(reflection)), _p(res.get("rmsd")),
                                           _p(res.get("sd")), _p(res.get("R")), _p(res.get("t")), _stream())
    _check("esmdiff_superpose_pairs", code, capacity=lambda: f"esmdiff_superpose_pairs: {n} x {m} pairs are more than one launch "
                                                             f"takes (2^31 - 1 workgroups of 4 pairs); pass the rows in blocks")
    return res


def tm(A, B, ma, mb, transform: bool = False):
    """One esmdiff_tm_pairs launch -> tm (n, m), normalised by B's valid residues; transform: (tm, R (n, m, 3, 3), t (n, m, 3))."""
    n, m, L = _sizes(A, B)
    score = _new((n, m))
    R, t = (_new((n, m, 3, 3)), _new((n, m, 3))) if transform else (None, None)
    code = N.lib().esmdiff_tm_pairs(_p(A), n, _p(B), m, L, _p(ma), _p(mb), _p(score), _p(R), _p(t), _stream())
    _check("esmdiff_tm_pairs", code, capacity=lambda: f"esmdiff_tm_pairs: L = {L} is beyond the kernel's limit ({N.TM_MAX_L} "
                                                      f"residues: both structures of a pair are staged in LDS); there is no slow path")
    return (score, R, t) if transform else score


def lddt_counts(A, B, ma, mb, per_residue: bool = False, r0: float = LDDT_R0, thresholds=LDDT_THRESHOLDS, seq_sep: int = 1):
    """One esmdiff_lddt_pairs launch -> int32 tensors kept (n, m), total (m,), and with per_residue kept_res (n, m, L) and
    total_res (m, L) (else None, and never allocated)."""
    n, m, L = _sizes(A, B)
    thr = [float(t) for t in thresholds]
    kept, total = _new((n, m), torch.int32), _new((m,), torch.int32)
    kept_res, total_res = (_new((n, m, L), torch.int32), _new((m, L), torch.int32)) if per_residue else (None, None)
    code = N.lib().esmdiff_lddt_pairs(_p(A), n, _p(B), m, L, _p(ma), _p(mb), float(r0), (ctypes.c_double * len(thr))(*thr), len(thr),
                                      int(seq_sep), _p(kept), _p(total), _p(kept_res), _p(total_res), _stream())
    _check("esmdiff_lddt_pairs", code,
           capacity=lambda: f"esmdiff_lddt_pairs: L = {L} is beyond the kernel's limit ({N.LDDT_MAX_L} residues: a model is staged "
                            f"in LDS); there is no slow path",
           invalid=lambda: f"esmdiff_lddt_pairs: invalid argument: L = {L} (at least 2), seq_sep = {seq_sep} (at least 1), "
                           f"{len(thr)} thresholds (1 to {N.LDDT_MAX_THRESHOLDS})")
    return kept, total, kept_res, total_res


def lddt(A, B, ma, mb, r0: float = LDDT_R0, thresholds=LDDT_THRESHOLDS, seq_sep: int = 1) -> torch.Tensor:
    """lDDT (n, m) float64: kept / (n_thresholds total), NaN where the native has no pair."""
    kept, total, _, _ = lddt_counts(A, B, ma, mb, False, r0, thresholds, seq_sep)
    return kept.to(torch.float64) / (len(thresholds) * total).to(torch.float64)[None]


def dssp(X, mask, no_donor, counts: bool = True):
    """One esmdiff_dssp call: X f64 (n, L, 4, 3) N / CA / C / O, mask u8 (n, L) or None, no_donor u8 (L,) or None -> ss u8 (n, L),
    counts i32 (L, 8) (None without `counts`), acceptor i32 (n, L, 2), energy f64 (n, L, 2)."""
    n, L = _frames(X, mask, (4, 3))
    assert no_donor is None or (no_donor.dtype == torch.uint8 and tuple(no_donor.shape) == (L,)), "no_donor is u8 (L,)"
    ss, table = _new((n, L), torch.uint8), _new((L, 8), torch.int32) if counts else None
    acceptor, energy = _new((n, L, 2), torch.int32), _new((n, L, 2))
    code = N.lib().esmdiff_dssp(_p(X), n, L, _p(mask), _p(no_donor), _p(ss), _p(table), _p(acceptor), _p(energy), _stream())
    _check("esmdiff_dssp", code, invalid=lambda: f"esmdiff_dssp: invalid argument: L = {L} (1 to {N.DSSP_MAX_L} residues)")
    return ss, table, acceptor, energy


def contact_map(X, mask, cutoff: float, min_sep: int, sums: bool = True):
    """One esmdiff_contact_map call: X f64 (n, L, 3), mask u8 (n, L) or None -> valid i32 (L, L), count i32 (L, L), and with `sums`
    sum_d, sum_d2 f64 (L, L) (else None, and never allocated).  The (n, L, L) distances are never stored: the scratch holds
    N.contact_chunks(n, L) partial tiles per tile of the triangle, and nothing when that is one chunk."""
    n, L = _frames(X, mask, (3,))
    valid, count = _new((L, L), torch.int32), _new((L, L), torch.int32)
    sum_d, sum_d2 = (_new((L, L)), _new((L, L))) if sums else (None, None)
    size = N.contact_scratch_bytes(n, L) if 2 <= L <= N.CONTACT_MAX_L and n >= 1 else 0
    scratch = _new((size // 8,)) if size else None
    code = N.lib().esmdiff_contact_map(_p(X), n, L, _p(mask), float(cutoff), int(min_sep), _p(valid), _p(count), _p(sum_d), _p(sum_d2),
                                       _p(scratch), size, _stream())
    _check("esmdiff_contact_map", code,
           capacity=lambda: f"esmdiff_contact_map: L = {L} is beyond the kernel's limit ({N.CONTACT_MAX_L} residues); there is no slow path",
           invalid=lambda: f"esmdiff_contact_map: invalid argument: n = {n} (at least 1), L = {L} (at least 2), min_sep = {min_sep} "
                           f"(at least 1), cutoff = {cutoff} (not NaN)")
    return valid, count, sum_d, sum_d2


def native_contacts(A, B, ma, mb, cutoff: float, min_sep: int, lam: float, beta: float, per_residue: bool = False, soft: bool = True):
    """One esmdiff_native_contacts launch -> kept i32 (n, m), total i32 (m,), kept_res i32 (n, m, L) and total_res i32 (m, L) with
    per_residue, q_soft f64 (n, m) with soft (else None, and never allocated)."""
    n, m, L = _sizes(A, B)
    kept, total = _new((n, m), torch.int32), _new((m,), torch.int32)
    kept_res, total_res = (_new((n, m, L), torch.int32), _new((m, L), torch.int32)) if per_residue else (None, None)
    q_soft = _new((n, m)) if soft else None
    code = N.lib().esmdiff_native_contacts(_p(A), n, _p(B), m, L, _p(ma), _p(mb), float(cutoff), int(min_sep), float(lam), float(beta),
                                           _p(kept), _p(total), _p(kept_res), _p(total_res), _p(q_soft), _stream())
    _check("esmdiff_native_contacts", code,
           capacity=lambda: f"esmdiff_native_contacts: L = {L} is beyond the kernel's limit ({N.CONTACT_MAX_L} residues: a model is "
                            f"staged in LDS); there is no slow path",
           invalid=lambda: f"esmdiff_native_contacts: invalid argument: L = {L} (at least 2), min_sep = {min_sep} (at least 1), "
                           f"cutoff = {cutoff}, lam = {lam}, beta = {beta} (not NaN)")
    return kept, total, kept_res, total_res, q_soft


def backbone_torsions(X, mask, break_distance: float, geometry: bool = False):
    """One esmdiff_backbone_torsions call: X f64 (n, L, 3 or 4, 3) N / CA / C (/ O, never read), mask u8 (n, L) or None -> phi, psi,
    omega f64 (n, L) in radians (NaN where undefined) and, with `geometry`, geom f64 (n, L, 6) (else None, and never allocated)."""
    n, L = _frames(X, mask, ((3, 4), 3))
    phi, psi, omega = _new((n, L)), _new((n, L)), _new((n, L))
    geom = _new((n, L, 6)) if geometry else None
    code = N.lib().esmdiff_backbone_torsions(_p(X), n, L, X.shape[2], _p(mask), float(break_distance), _p(phi), _p(psi), _p(omega), _p(geom),
                                             _stream())
    _check("esmdiff_backbone_torsions", code,
           invalid=lambda: f"esmdiff_backbone_torsions: invalid argument: L = {L} (at least 1), break_distance = {break_distance} "
                           f"(positive and finite)",
           capacity=lambda: f"esmdiff_backbone_torsions: {n} x {L} residues are more than one launch takes; pass the structures in blocks")
    return phi, psi, omega, geom


def ramachandran(X, mask, break_distance: float, bins: int, sums: bool = True):
    """One esmdiff_ramachandran call: X and mask as backbone_torsions takes them -> hist i32 (L, bins, bins), counts i32 (L, 5) and, with
    `sums`, sums f64 (L, 6) (else None, and never allocated).  No (n, L) angle array exists: the scratch holds N.rama_chunks(n, L)
    partial sums per residue, and nothing when that is one chunk."""
    n, L = _frames(X, mask, ((3, 4), 3))
    bins = int(bins)
    ok = 1 <= bins <= N.RAMA_MAX_BINS
    hist, counts = _new((L, bins, bins) if ok else (1,), torch.int32), _new((L, 5), torch.int32)     # not ok: the entry refuses, writes nothing
    out = _new((L, 6)) if sums else None
    size = N.rama_scratch_bytes(n, L) if sums else 0
    scratch = _new((size // 8,)) if size else None
    code = N.lib().esmdiff_ramachandran(_p(X), n, L, X.shape[2], _p(mask), float(break_distance), bins, _p(hist), _p(counts), _p(out),
                                        _p(scratch), size, _stream())
    _check("esmdiff_ramachandran", code,
           capacity=lambda: f"esmdiff_ramachandran: bins = {bins} is beyond the kernel's limit ({N.RAMA_MAX_BINS} per axis)",
           invalid=lambda: f"esmdiff_ramachandran: invalid argument: L = {L} (at least 1), bins = {bins} (at least 1), "
                           f"break_distance = {break_distance} (positive and finite)")
    return hist, counts, out


def shape_frames(X, mask, width: Optional[float] = None, bins: int = 0):
    """One esmdiff_shape_frames call: X f64 (n, L, 3), mask u8 (n, L) or None -> count i32 (n,), desc f64 (n, 12) (the centroid, the six
    sums of (r - c)(r - c)^T undivided, sum_inv_d, dmax, ree) and, with a `width`, hist i64 (bins + 1,): the pair distances of all frames
    in cells of that width, the last cell the overflow (else None, and never allocated)."""
    n, L = _frames(X, mask, (3,))
    count, desc = _new((n,), torch.int32), _new((n, 12))
    bins = int(bins)
    hist = None if width is None else _new((bins + 1 if 1 <= bins <= N.SHAPE_MAX_BINS else 1,), torch.int64)   # refused: nothing is written
    code = N.lib().esmdiff_shape_frames(_p(X), n, L, _p(mask), _p(count), _p(desc), _p(hist), 0.0 if width is None else float(width),
                                        bins, _stream())
    _check("esmdiff_shape_frames", code,
           capacity=lambda: f"esmdiff_shape_frames: L = {L} or bins = {bins} is beyond the kernel's limits ({N.SHAPE_MAX_L} residues: a "
                            f"frame is staged in LDS; {N.SHAPE_MAX_BINS} cells); there is no slow path",
           invalid=lambda: f"esmdiff_shape_frames: invalid argument: L = {L} (at least 1), bins = {bins} (at least 1), width = {width} "
                           f"(positive and finite)")
    return count, desc, hist


def debye_frames(X, mask, q, ff=None):
    """One esmdiff_debye_frames call: X f64 (n, L, 3), mask u8 (n, L) or None, q f64 (Q,) and ff f64 (L, Q) or None on the device ->
    intensity f64 (n, Q).  The entry does not look at q: its values are the caller's to check (esmdiff_amd/shape.py does)."""
    n, L = _frames(X, mask, (3,))
    assert q.dim() == 1 and q.dtype == torch.float64 and q.is_cuda, "q is f64 (Q,) on the device"
    Q = q.shape[0]
    assert ff is None or (ff.dtype == torch.float64 and ff.is_cuda and tuple(ff.shape) == (L, Q)), f"the form factors are f64 ({L}, {Q}) on the device"
    intensity = _new((n, Q))
    code = N.lib().esmdiff_debye_frames(_p(X), n, L, _p(mask), _p(q), Q, _p(ff), _p(intensity), _stream())
    _check("esmdiff_debye_frames", code,
           capacity=lambda: f"esmdiff_debye_frames: L = {L} or Q = {Q} is beyond the kernel's limits ({N.SHAPE_MAX_L} residues: a frame "
                            f"is staged in LDS; {N.DEBYE_MAX_Q} values of q a call); there is no slow path",
           invalid=lambda: f"esmdiff_debye_frames: invalid argument: L = {L} (at least 1), Q = {Q} (at least 1)")
    return intensity


SASA_OUTPUTS = ("count", "sum_count", "valid", "exposed", "exposed_count", "present_count")


def sasa_frames(X, mask, radii, points, threshold: float = 0.0, want=SASA_OUTPUTS) -> dict:
    """One esmdiff_sasa_frames call: X f64 (n, L, A, 3) with A = 1, 3 or 4, mask u8 (n, L) or None, radii f64 (L, A) already expanded by
    the probe and points f64 (P, 3), all on the device -> {name: tensor} for the names in `want`: count i32 (n, L, A) (-1 for an absent
    atom), sum_count i64 (L, A), valid i32 (L, A), exposed u8 (n, L) (0, 1, or 2 for a residue without atoms), exposed_count and
    present_count i32 (L,).  What is not wanted is never allocated."""
    (n, L), A = _frames(X, mask, (None, 3)), X.shape[2]
    assert radii.dtype == torch.float64 and radii.is_cuda and tuple(radii.shape) == (L, A), f"the radii are f64 ({L}, {A}) on the device"
    assert points.dim() == 2 and points.shape[1] == 3 and points.dtype == torch.float64 and points.is_cuda, "the points are f64 (P, 3) on the device"
    P = points.shape[0]
    assert set(want) <= set(SASA_OUTPUTS), f"outputs are {SASA_OUTPUTS}"
    shapes = {"count": ((n, L, A), torch.int32), "sum_count": ((L, A), torch.int64), "valid": ((L, A), torch.int32),
              "exposed": ((n, L), torch.uint8), "exposed_count": ((L,), torch.int32), "present_count": ((L,), torch.int32)}
    res = {k: _new(*shapes[k]) for k in want}
    code = N.lib().esmdiff_sasa_frames(_p(X), n, L, A, _p(mask), _p(radii), _p(points), P, float(threshold),
                                       *[_p(res.get(k)) for k in SASA_OUTPUTS], _stream())
    _check("esmdiff_sasa_frames", code,
           capacity=lambda: f"esmdiff_sasa_frames: {L} x {A} atoms or P = {P} is beyond the kernel's limits ({N.SASA_MAX_ATOMS} atoms: a "
                            f"frame is staged in LDS; {N.SASA_MAX_POINTS} points); there is no slow path",
           invalid=lambda: f"esmdiff_sasa_frames: invalid argument: L = {L} (at least 1), A = {A} (1, 3 or 4), P = {P} (at least 1), "
                           f"threshold = {threshold} (not NaN)")
    return res


def cooccurrence(flags):
    """One esmdiff_cooccurrence call: flags u8 (n, L) on the device, 0 or 1 and anything else undefined -> out i32 (3, L, L): the frames
    where a and b are both defined, of those the frames where a is 1, and where both are 1."""
    assert flags.dim() == 2 and flags.dtype == torch.uint8 and flags.is_cuda, f"u8 (n, L) flags on the device, got {flags.dtype} {tuple(flags.shape)}"
    n, L = flags.shape
    out = _new((3, L, L), torch.int32)
    size = N.coocc_scratch_bytes(n, L)
    scratch = _new((size // 8,), torch.int64) if size else None
    code = N.lib().esmdiff_cooccurrence(_p(flags), n, L, _p(out), _p(scratch), size, _stream())
    _check("esmdiff_cooccurrence", code,
           capacity=lambda: f"esmdiff_cooccurrence: L = {L} is beyond the entry's limit ({N.COOCC_MAX_L} residues)",
           invalid=lambda: f"esmdiff_cooccurrence: invalid argument: L = {L} (at least 1)")
    return out


LAGGED_WORKGROUPS = 512       # the chunks one round of esmdiff_lagged_moments runs at once are chosen to give about this many workgroups (two a CU)
LAGGED_SCRATCH_CAP = 1 << 28  # ... within this many bytes of scratch, or one slot where one slot is larger


def _lagged_input(X, pwd_offset: int):
    """X f64 (n, D) with pwd_offset 0 or f64 (n, L, 3) with pwd_offset >= 1, on the device -> n, L_or_D, D."""
    assert X.dtype == torch.float64 and X.is_cuda, f"f64 frames on the device, got {X.dtype}"
    if pwd_offset == 0:
        assert X.dim() == 2, f"the feature form takes f64 (n, D), got {tuple(X.shape)}"
        return X.shape[0], X.shape[1], X.shape[1]
    assert X.dim() == 3 and X.shape[2] == 3, f"the coordinate form takes f64 (n, L, 3), got {tuple(X.shape)}"
    return X.shape[0], X.shape[1], max(N.lagged_features(X.shape[1], pwd_offset), 0) if pwd_offset < X.shape[1] else 0


def lagged_slots(D: int, chunks: int, moments: bool) -> int:
    """The slots of scratch a call gets: enough chunks at once to fill the device, within LAGGED_SCRATCH_CAP bytes, at least one.  The
    number changes no bit of the result (include/esmdiff_hip.h)."""
    tiles = (D + 63) // 64
    want = -(-LAGGED_WORKGROUPS // (tiles * (tiles + 1) // 2)) if moments else chunks
    fit = LAGGED_SCRATCH_CAP // max(N.lagged_scratch_bytes(D, 1, moments) - D * 8, 1)
    return max(1, min(chunks, want, fit))


def _lagged_invalid(entry, n, L_or_D, pwd_offset, lag=None, dim=None):
    lag_text = "" if lag is None else f", lag = {lag} (at least 1, below n)"
    dim_text = "" if dim is None else f", dim = {dim} (1 to {N.LAGGED_MAX_DIM})"
    return lambda: (f"{entry}: invalid argument: n = {n}{lag_text}{dim_text}, pwd_offset = {pwd_offset} (0: features, up to "
                    f"{N.LAGGED_MAX_D} of them; k >= 1: CA coordinates of k < L <= {N.LAGGED_MAX_L} residues), L or D = {L_or_D}; there is no slow path")


def _lagged_scratch(D: int, n: int, lag: int, moments: bool, slots):
    chunks = max(-(-(n - lag) // N.LAGGED_FRAME_CHUNK), 1)
    size = N.lagged_scratch_bytes(max(D, 1), lagged_slots(max(D, 1), chunks, moments) if slots is None else slots, moments)
    return _new((size // 8,), torch.int64), size


def lagged_means(X, lag: int, pwd_offset: int = 1, slots=None):
    """One esmdiff_lagged_means call: X f64 (n, L, 3) (pwd_offset >= 1) or (n, D) (pwd_offset = 0) on the device -> mean0 (D,),
    meant (D,): the means of the features over the frames t < n - lag and over t + lag.  slots: the chunk sums the scratch holds
    (default: lagged_slots); no bit depends on it."""
    n, L_or_D, D = _lagged_input(X, pwd_offset)
    mean0, meant = _new((D,)), _new((D,))
    scratch, size = _lagged_scratch(D, n, lag, False, slots)
    code = N.lib().esmdiff_lagged_means(_p(X), n, L_or_D, int(pwd_offset), int(lag), _p(mean0), _p(meant), _p(scratch), size, _stream())
    _check("esmdiff_lagged_means", code, invalid=_lagged_invalid("esmdiff_lagged_means", n, L_or_D, pwd_offset, lag))
    return mean0, meant


def lagged_moments(X, lag: int, center, pwd_offset: int = 1, slots=None, out=None) -> dict:
    """One esmdiff_lagged_moments call: X as lagged_means takes it, center f64 (D,) on the device -> {S00, S0t, Stt: (D, D), r0, rt:
    (D,)}, the raw sums of a a^T, a b^T, b b^T, a and b with a = f(x_t) - center, b = f(x_{t + lag}) - center over t < n - lag.
    out: {name: tensor} to write into instead of allocating."""
    n, L_or_D, D = _lagged_input(X, pwd_offset)
    assert center is not None and center.dtype == torch.float64 and center.is_cuda and tuple(center.shape) == (D,), f"the centre is f64 ({D},) on the device"
    shapes = {"S00": (D, D), "S0t": (D, D), "Stt": (D, D), "r0": (D,), "rt": (D,)}
    res = {k: out[k] if out and k in out else _new(s) for k, s in shapes.items()}
    assert all(tuple(v.shape) == shapes[k] and v.dtype == torch.float64 for k, v in res.items()), f"the call writes f64 {shapes}"
    scratch, size = _lagged_scratch(D, n, lag, True, slots)
    code = N.lib().esmdiff_lagged_moments(_p(X), n, L_or_D, int(pwd_offset), int(lag), _p(center), *[_p(res[k]) for k in shapes],
                                          _p(scratch), size, _stream())
    _check("esmdiff_lagged_moments", code, invalid=_lagged_invalid("esmdiff_lagged_moments", n, L_or_D, pwd_offset, lag))
    return res


def lagged_project(X, mean, W, pwd_offset: int = 1):
    """One esmdiff_lagged_project call: X as lagged_means takes it, mean f64 (D,), W f64 (D, dim) on the device -> Y (n, dim) =
    (f(x_t) - mean) W, every frame's row in the same fixed tree."""
    n, L_or_D, D = _lagged_input(X, pwd_offset)
    assert mean.dtype == torch.float64 and mean.is_cuda and tuple(mean.shape) == (D,), f"the mean is f64 ({D},) on the device"
    assert W.dim() == 2 and W.dtype == torch.float64 and W.is_cuda and W.shape[0] == D, f"the directions are f64 ({D}, dim) on the device"
    dim = W.shape[1]
    Y = _new((n, dim))
    size = max(D, 1) * 8
    scratch = _new((size // 8,), torch.int64)
    code = N.lib().esmdiff_lagged_project(_p(X), n, L_or_D, int(pwd_offset), _p(mean), _p(W), dim, _p(Y), _p(scratch), size, _stream())
    _check("esmdiff_lagged_project", code, invalid=_lagged_invalid("esmdiff_lagged_project", n, L_or_D, pwd_offset, dim=dim))
    return Y


KMEANS_SCRATCH_CAP = 1 << 28  # the chunk sums one round of esmdiff_kmeans_step keeps, in bytes, or one slot where one slot is larger


def _kmeans_input(Y, centres):
    """Y f64 (n, d) and centres f64 (k, d) on the device -> n, d, k."""
    assert Y.dim() == 2 and Y.dtype == torch.float64 and Y.is_cuda, f"f64 (n, d) frames on the device, got {Y.dtype} {tuple(Y.shape)}"
    assert centres.dim() == 2 and centres.dtype == torch.float64 and centres.is_cuda and centres.shape[1] == Y.shape[1], \
        f"f64 (k, {Y.shape[1]}) centres on the device, got {centres.dtype} {tuple(centres.shape)}"
    return Y.shape[0], Y.shape[1], centres.shape[0]


def _kmeans_text(entry, n, d, k):
    invalid = lambda: f"{entry}: invalid argument: n = {n}, d = {d}, k = {k} (at least one component and one centre)"
    capacity = lambda: (f"{entry}: d = {d} components (up to {N.LAGGED_MAX_DIM}) or k = {k} centres (up to {N.KMEANS_MAX_K}) are beyond the "
                        f"entry's limits, or the scratch is smaller than one chunk's sums; there is no slow path")
    return {"invalid": invalid, "capacity": capacity}


def kmeans_slots(k: int, d: int, chunks: int) -> int:
    """The slots of scratch a step gets: every chunk at once within KMEANS_SCRATCH_CAP bytes, at least one.  The number changes no bit of
    the result (include/esmdiff_hip.h)."""
    return max(1, min(chunks, KMEANS_SCRATCH_CAP // N.kmeans_slot_bytes(k, d)))


def kmeans_assign(Y, centres, dist2: bool = True):
    """One esmdiff_kmeans_assign call: Y f64 (n, d), centres f64 (k, d) on the device -> labels i32 (n,) (the smallest index of a nearest
    centre, -1 for a frame with a non-finite component or when no centre is finite) and dist2 f64 (n,) (None with dist2=False)."""
    n, d, k = _kmeans_input(Y, centres)
    labels, d2 = _new((n,), torch.int32), _new((n,)) if dist2 else None
    code = N.lib().esmdiff_kmeans_assign(_p(Y), n, d, _p(centres), k, _p(labels), _p(d2), _stream())
    _check("esmdiff_kmeans_assign", code, **_kmeans_text("esmdiff_kmeans_assign", n, d, k))
    return labels, d2


def kmeans_step(Y, centres, labels: bool = True, slots=None) -> dict:
    """One esmdiff_kmeans_step call: Y f64 (n, d), centres f64 (k, d) on the device -> {labels: i32 (n,) (absent with labels=False),
    counts: i64 (k,), sums: f64 (k, d), inertia: f64 (1,)}.  slots: the chunk sums the scratch holds (default: kmeans_slots); no bit
    depends on it."""
    n, d, k = _kmeans_input(Y, centres)
    res = {"labels": _new((n,), torch.int32)} if labels else {}
    res.update(counts=_new((k,), torch.int64), sums=_new((k, d)), inertia=_new((1,)))
    size = N.kmeans_step_scratch_bytes(max(k, 1), max(d, 1), kmeans_slots(max(k, 1), max(d, 1), N.kmeans_chunks(n)) if slots is None else slots)
    scratch = _new((size // 8,), torch.int64)
    code = N.lib().esmdiff_kmeans_step(_p(Y), n, d, _p(centres), k, _p(res.get("labels")), _p(res["counts"]), _p(res["sums"]), _p(res["inertia"]),
                                       _p(scratch), size, _stream())
    _check("esmdiff_kmeans_step", code, **_kmeans_text("esmdiff_kmeans_step", n, d, k))
    return res


def transition_counts(labels, k: int, lag: int):
    """One esmdiff_transition_counts call: labels i32 (n,) on the device -> counts i64 (k, k): the pairs (labels[t], labels[t + lag]),
    t < n - lag, both >= 0.  A label >= k is refused."""
    assert labels.dim() == 1 and labels.dtype == torch.int32 and labels.is_cuda, f"i32 (n,) labels on the device, got {labels.dtype} {tuple(labels.shape)}"
    n = labels.shape[0]
    counts = _new((max(int(k), 0), max(int(k), 0)), torch.int64)
    scratch = _new((N.TRANSITION_SCRATCH_BYTES // 8,), torch.int64)
    code = N.lib().esmdiff_transition_counts(_p(labels), n, int(k), int(lag), _p(counts), _p(scratch), N.TRANSITION_SCRATCH_BYTES, _stream())
    _check("esmdiff_transition_counts", code,
           capacity=lambda: f"esmdiff_transition_counts: k = {k} states are beyond the entry's limit ({N.KMEANS_MAX_K})",
           invalid=lambda: f"esmdiff_transition_counts: invalid argument: k = {k} (at least 1), lag = {lag} (at least 1), or a label >= k")
    return counts


def adjacency(n: int) -> torch.Tensor:
    """The empty neighbour relation of n structures: one bit per pair, int64 (n, ceil(n / 64))."""
    return torch.zeros((n, (n + 63) // 64), dtype=torch.int64, device="cuda")


def threshold(block: torch.Tensor, row0: int, cutoff: float, larger_is_closer: bool, adj: torch.Tensor):
    """block f64 (rows, n): rows row0 .. of the n x n matrix -> their bits of adj (esmdiff_cluster_threshold)."""
    rows, n = block.shape
    assert block.dtype == torch.float64 and adj.dtype == torch.int64 and tuple(adj.shape) == (n, (n + 63) // 64)
    _check("esmdiff_cluster_threshold", N.lib().esmdiff_cluster_threshold(_p(block), rows, row0, n, float(cutoff),
                                                                          int(bool(larger_is_closer)), _p(adj), _stream()))


def gromos(adj: torch.Tensor):
    """esmdiff_cluster_gromos on the relation (symmetrised in place) -> int32 out (3, n): labels, centres, sizes, the last two
    filled up to the number of clusters, and that number k (1,)."""
    n = adj.shape[0]
    assert adj.dtype == torch.int64 and tuple(adj.shape) == (n, (n + 63) // 64)
    out, k = _new((3, n), torch.int32), _new((1,), torch.int32)             # the kernel writes k whatever it finds
    code = N.lib().esmdiff_cluster_gromos(_p(adj), n, _p(out[0]), _p(out[1]), _p(out[2]), _p(k), _stream())
    _check("esmdiff_cluster_gromos", code)
    return out, k


def _flex_invalid(entry: str, n: int, L: int):
    return lambda: f"{entry}: invalid argument: n = {n} (at least 1), L = {L} (at least 2)"


def pair_msf(A, ma):
    """One esmdiff_flex_pair_msf call -> sum_sq f64 (L,), count i64 (L,): over the pairs i < j of A (n, L, 3) fitted on the residues
    valid in both, the sum of each residue's squared deviation and the number of pairs it was valid in.  The (n, n, L) deviations are
    never stored: the scratch holds N.flex_pair_slots(n) partial sums per residue."""
    n, L = _frames(A, ma, (3,))
    sum_sq, count = _new((L,)), _new((L,), torch.int64)
    size = N.flex_pair_slots(n) * L * 12
    scratch = _new((size // 4,), torch.int32)
    code = N.lib().esmdiff_flex_pair_msf(_p(A), n, L, _p(ma), _p(sum_sq), _p(count), _p(scratch), size, _stream())
    _check("esmdiff_flex_pair_msf", code, invalid=_flex_invalid("esmdiff_flex_pair_msf", n, L),
           capacity=lambda: f"esmdiff_flex_pair_msf: a scratch of {size} bytes is too small for n = {n}, L = {L}")
    return sum_sq, count


def fit(A, ma, ref, mref):
    """One esmdiff_flex_fit call: every A[i] fitted onto ref (L, 3) on the residues valid in both (mref u8 (L,) or None) ->
    aligned f64 (n, L, 3) (the whole structure moved; a NaN coordinate stays NaN), rmsd f64 (n,).  Fewer than 2 common residues: NaN."""
    n, L = _frames(A, ma, (3,))
    assert ref.dtype == torch.float64 and tuple(ref.shape) == (L, 3), f"the reference is f64 ({L}, 3), got {tuple(ref.shape)}"
    assert mref is None or (mref.dtype == torch.uint8 and tuple(mref.shape) == (L,)), "the reference's mask is u8 (L,)"
    aligned, rmsd = _new((n, L, 3)), _new((n,))
    code = N.lib().esmdiff_flex_fit(_p(A), n, L, _p(ma), _p(ref), _p(mref), _p(aligned), _p(rmsd), _stream())
    _check("esmdiff_flex_fit", code, invalid=_flex_invalid("esmdiff_flex_fit", n, L))
    return aligned, rmsd


def flex_transforms(A, ma, ref, mref):
    """One esmdiff_flex_transforms call: fit's fit with the transform written out -> T f64 (n, 12) (row-major rot, then tr, with
    rot a + tr ~ ref), rmsd f64 (n,) (fit's bits), ok u8 (n,).  Fewer than 2 common residues: ok = 0 and NaN in T and rmsd."""
    n, L = _frames(A, ma, (3,))
    assert ref.dtype == torch.float64 and tuple(ref.shape) == (L, 3), f"the reference is f64 ({L}, 3), got {tuple(ref.shape)}"
    assert mref is None or (mref.dtype == torch.uint8 and tuple(mref.shape) == (L,)), "the reference's mask is u8 (L,)"
    T, rmsd, ok = _new((n, 12)), _new((n,)), _new((n,), torch.uint8)
    code = N.lib().esmdiff_flex_transforms(_p(A), n, L, _p(ma), _p(ref), _p(mref), _p(T), _p(rmsd), _p(ok), _stream())
    _check("esmdiff_flex_transforms", code, invalid=_flex_invalid("esmdiff_flex_transforms", n, L))
    return T, rmsd, ok


ALIGNED_WORKGROUPS = 2048      # the chunks one round of esmdiff_aligned_moments runs at once are chosen to give about this many workgroups (eight a CU)
ALIGNED_SCRATCH_CAP = 1 << 28  # ... within this many bytes of scratch, or one slot where one slot is larger


def aligned_slots(L: int, chunks: int) -> int:
    """The slots of scratch a call gets: enough chunks at once to fill the device, within ALIGNED_SCRATCH_CAP bytes, at least one.  The
    number changes no bit of the result (include/esmdiff_hip.h)."""
    tiles = (3 * L + 63) // 64
    want = -(-ALIGNED_WORKGROUPS // (tiles * (tiles + 1) // 2))
    return max(1, min(chunks, want, ALIGNED_SCRATCH_CAP // N.aligned_scratch_bytes(L, 1)))


def _aligned_input(X, T):
    assert X.dim() == 3 and X.shape[2] == 3 and X.dtype == torch.float64 and X.is_cuda, f"f64 (n, L, 3) frames on the device, got {X.dtype} {tuple(X.shape)}"
    n, L = X.shape[:2]
    assert T is None or (T.dtype == torch.float64 and T.is_cuda and tuple(T.shape) == (n, 12)), f"the transforms are f64 ({n}, 12) on the device"
    return n, L


def _aligned_text(entry, n, L, dim=None):
    dim_text = "" if dim is None else f", dim = {dim} (1 to {N.ALIGNED_MAX_DIM})"
    return {"invalid": lambda: f"{entry}: invalid argument: n = {n} (at least 1), L = {L} (at least 1){dim_text}",
            "capacity": lambda: f"{entry}: L = {L} is beyond the kernel's limit ({N.ALIGNED_MAX_L} residues); there is no slow path"}


def aligned_moments(X, T, use, center, slots=None, out=None) -> dict:
    """One esmdiff_aligned_moments call: X f64 (n, L, 3), T f64 (n, 12) or None (the identity), use u8 (n,) or None (every frame),
    center f64 (3L,), all on the device -> {S: (3L, 3L), r: (3L,), count: i64 (1,)}: the raw sums of a a^T and a over the used frames,
    a = (rot x + tr) - center.  slots: the chunk sums the scratch holds (default: aligned_slots); no bit depends on it.  out: {name:
    tensor} to write into instead of allocating."""
    n, L = _aligned_input(X, T)
    D = 3 * L
    assert use is None or (use.dtype == torch.uint8 and use.is_cuda and tuple(use.shape) == (n,)), f"the flags are u8 ({n},) on the device"
    assert center is not None and center.dtype == torch.float64 and center.is_cuda and tuple(center.shape) == (D,), f"the centre is f64 ({D},) on the device"
    shapes = {"S": ((D, D), torch.float64), "r": ((D,), torch.float64), "count": ((1,), torch.int64)}
    res = {k: out[k] if out and k in out else _new(*s) for k, s in shapes.items()}
    assert all(tuple(v.shape) == shapes[k][0] and v.dtype == shapes[k][1] for k, v in res.items()), f"the call writes {shapes}"
    chunks = max(-(-n // N.ALIGNED_FRAME_CHUNK), 1)
    size = N.aligned_scratch_bytes(max(L, 1), aligned_slots(max(L, 1), chunks) if slots is None else slots)
    scratch = _new((size // 8,), torch.int64)
    code = N.lib().esmdiff_aligned_moments(_p(X), n, L, _p(T), _p(use), _p(center), _p(res["S"]), _p(res["r"]), _p(res["count"]),
                                           _p(scratch), size, _stream())
    _check("esmdiff_aligned_moments", code, **_aligned_text("esmdiff_aligned_moments", n, L))
    return res


def aligned_project(X, T, mean, W):
    """One esmdiff_aligned_project call: X f64 (n, L, 3), T f64 (n, 12) or None, mean f64 (3L,), W f64 (3L, dim) on the device ->
    Y (n, dim) = ((rot x + tr) - mean) W, every frame's row in the same fixed tree."""
    n, L = _aligned_input(X, T)
    D = 3 * L
    assert mean.dtype == torch.float64 and mean.is_cuda and tuple(mean.shape) == (D,), f"the mean is f64 ({D},) on the device"
    assert W.dim() == 2 and W.dtype == torch.float64 and W.is_cuda and W.shape[0] == D, f"the directions are f64 ({D}, dim) on the device"
    dim = W.shape[1]
    Y = _new((n, dim))
    code = N.lib().esmdiff_aligned_project(_p(X), n, L, _p(T), _p(mean), _p(W), dim, _p(Y), _stream())
    _check("esmdiff_aligned_project", code, **_aligned_text("esmdiff_aligned_project", n, L, dim))
    return Y


RMSD_NN_WORKGROUPS = 2048         # the rectangles one round of esmdiff_rmsd_nearest runs at once (eight a CU) ...
RMSD_NN_SCRATCH_CAP = 1 << 28     # ... within this many bytes of slots


def rmsd_nn_slots(rectangles: int) -> int:
    """The slots of scratch a call gets: enough rectangles at once to fill the device, within RMSD_NN_SCRATCH_CAP bytes, at least one.
    The number changes no bit of the result (include/esmdiff_hip.h)."""
    return max(1, min(rectangles, RMSD_NN_WORKGROUPS, RMSD_NN_SCRATCH_CAP // N.RMSD_NN_SLOT_BYTES))


def rmsd_prepare(X, sel=None, n_sel=None) -> dict:
    """One esmdiff_rmsd_prepare call: X f64 (n, L, 3) on the device, sel u8 (L,) on the device or None (every residue), n_sel the
    number of nonzero sel (counted here when not given: one read-back) -> {P: (n, 3, K) the centred, compacted, zero-padded frames
    with K = N.rmsd_nn_padded(n_sel), info: (n, 4) centroid and G, use: u8 (n,), n_sel}."""
    assert X.dim() == 3 and X.shape[2] == 3 and X.dtype == torch.float64 and X.is_cuda, f"f64 (n, L, 3) frames on the device, got {X.dtype} {tuple(X.shape)}"
    n, L = X.shape[:2]
    assert sel is None or (sel.dtype == torch.uint8 and sel.is_cuda and tuple(sel.shape) == (L,)), f"the selection is u8 ({L},) on the device"
    if n_sel is None:
        n_sel = L if sel is None else int((sel != 0).sum())
    K = N.rmsd_nn_padded(max(n_sel, 0))
    P, info, use = _new((n, 3, K)), _new((n, 4)), _new((n,), torch.uint8)
    code = N.lib().esmdiff_rmsd_prepare(_p(X), n, L, _p(sel), n_sel, _p(P), _p(info), _p(use), _stream())
    _check("esmdiff_rmsd_prepare", code,
           invalid=lambda: f"esmdiff_rmsd_prepare: invalid argument: n = {n} (at least 1), L = {L}, {n_sel} selected residues (2 to L)")
    return {"P": P, "info": info, "use": use, "n_sel": n_sel}


RMSD_NN_OUTPUTS = ("rmsd", "index", "sum", "pairs", "count")


def rmsd_nearest(a: dict, b: Optional[dict] = None, reflection: bool = False, cutoffs=(), bins: int = 0, width: float = 1.0,
                 want=("row", "col"), dense=(), slots=None, scratch_bytes=None) -> dict:
    """One esmdiff_rmsd_nearest call on prepared sides (rmsd_prepare's dicts; b None: a against itself over pairs i != j) ->
    {row_rmsd (n,), row_index i32 (n,), row_sum (n,), row_pairs i64 (n,), row_count i64 (n, T), col_* the same for b (not for b None),
    hist i64 (bins,) when bins > 0, msd (n, m) / cross (n, m, 9) for the names in `dense`}.  cutoffs: up to N.RMSD_NN_MAX_CUTOFFS
    host numbers.  slots: the rectangles' partials the scratch holds (default: rmsd_nn_slots); no bit depends on it."""
    n, n_sel = a["P"].shape[0], a["n_sel"]
    m = n if b is None else b["P"].shape[0]
    for side in (a,) + (() if b is None else (b,)):
        k = side["P"].shape[0]
        assert side["n_sel"] == n_sel and tuple(side["P"].shape) == (k, 3, N.rmsd_nn_padded(n_sel)), "both sides are prepared on one residue set"
        assert side["P"].dtype == torch.float64 and tuple(side["info"].shape) == (k, 4) and side["info"].dtype == torch.float64
        assert tuple(side["use"].shape) == (k,) and side["use"].dtype == torch.uint8
    cut = np.ascontiguousarray(np.asarray(cutoffs, np.float64).reshape(-1))
    T = len(cut)
    res = {}
    for side, k in (("row", n),) + ((("col", m),) if b is not None else ()):
        if side in want:
            res.update({f"{side}_rmsd": _new((k,)), f"{side}_index": _new((k,), torch.int32), f"{side}_sum": _new((k,)),
                        f"{side}_pairs": _new((k,), torch.int64), f"{side}_count": _new((k, T), torch.int64)})
    if bins > 0:
        res["hist"] = _new((bins,), torch.int64)
    if "msd" in dense:
        res["msd"] = _new((n, m))
    if "cross" in dense:
        res["cross"] = _new((n, m, 9))
    blocks = lambda k: -(-k // N.RMSD_NN_RECT)
    rectangles = blocks(n) * (blocks(n) + 1) // 2 if b is None else blocks(n) * blocks(m)
    if scratch_bytes is None:
        scratch_bytes = N.rmsd_nn_scratch_bytes(n, 0 if b is None else m, rmsd_nn_slots(rectangles) if slots is None else slots)
    scratch = _new((max(scratch_bytes, 8) // 8,), torch.int64)
    g = res.get
    outs = [g(f"{s}_{k}") for s in ("row", "col") for k in RMSD_NN_OUTPUTS]
    code = N.lib().esmdiff_rmsd_nearest(_p(a["P"]), _p(a["info"]), _p(a["use"]), n, _p(b and b["P"]), _p(b and b["info"]), _p(b and b["use"]),
                                        m, n_sel, int(bool(reflection)), ctypes.c_void_p(cut.ctypes.data if T else 0), T, bins, float(width),
                                        *[_p(t) for t in outs], _p(g("hist")), _p(g("msd")), _p(g("cross")), _p(scratch), scratch_bytes, _stream())
    _check("esmdiff_rmsd_nearest", code,
           invalid=lambda: (f"esmdiff_rmsd_nearest: invalid argument: n = {n}, m = {m} (at least 1), {n_sel} selected residues (at least 2), "
                            f"{T} cutoffs (0 to {N.RMSD_NN_MAX_CUTOFFS}), bins = {bins} (0 or more, with a positive width: {width})"),
           capacity=lambda: (f"esmdiff_rmsd_nearest: bins = {bins} is beyond the kernel's limit ({N.RMSD_NN_MAX_BINS}), or the scratch "
                             f"({scratch_bytes} bytes) is smaller than one slot's ({N.rmsd_nn_scratch_bytes(n, 0 if b is None else m, 1)})"))
    return res


def moments(X, mask):
    """One esmdiff_flex_moments call -> mean f64 (L, 3), msf f64 (L,), count i32 (L,): per residue, over the structures valid there,
    the mean position and the mean squared distance from it (NaN where count is 0)."""
    n, L = _frames(X, mask, (3,))
    mean, msf, count = _new((L, 3)), _new((L,)), _new((L,), torch.int32)
    code = N.lib().esmdiff_flex_moments(_p(X), n, L, _p(mask), _p(mean), _p(msf), _p(count), _stream())
    _check("esmdiff_flex_moments", code, invalid=_flex_invalid("esmdiff_flex_moments", n, L))
    return mean, msf, count

"""Scoring: how likely the model finds a structure.  Host side of the reference's forward-only validation metric,
MaskedDiffusionLanguageModeling.model_step(batch, training=False) (/root/reference/slm/models/model.py:386-462), and of the
per-structure estimator built from it.

  _sample_t                   model.py:517-525   sample_t
  T rounding, sigma, move chance, change_of_variables, loss weight   model.py:404-418, :438-443   step_scalars
  q_xt                        model.py:494-512   Engine.q_xt (csrc/score.hip)
  gather + weighting + sum    model.py:432-445   Engine.nelbo_rows (csrc/score.hip)

The scalars are computed here with torch float32 in the reference's operation order (schedule arithmetic is
never re-derived in device code); the masking, the network and the scoring run on the device.  The functions take the model
object `m` (esmdiff_amd.model.MaskedDiffusionLanguageModeling, or anything with its attributes: tests drive them with a CPU
stand-in engine).

Philox keys of the scoring noise (include/esmdiff_hip.h, next to esmdiff_rng).  For the draw k of the structure with GLOBAL
index i under `seed`:
    mask uniform of position l   = Philox(seed, sample = i, step = k, l, column 4104)      (drawn on the device, q_xt_kernel)
    time uniform u_k             = Philox(seed, sample = i, step = k, l = 0, column 4105)  (drawn here, philox_uniform)
Neither column is read by a sampler (include/esmdiff_hip.h lists the reserved columns: 4104, 4105 and the gibbs "random"
strategy's 4352), so a score never reuses a uniform that produced the sample it scores; and both are a pure function of
(seed, i, k): the result does not depend on which other structures share a batch, on max_batch, or on how structures are sharded
over processes.  The time uniform is needed on the HOST (the schedule scalars are host torch code) and the library exports no
host generator, hence philox_uniform below: ed_math.h's function on Python integers, checked against the C oracle's.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence

import torch

from ._native import QXT_PHILOX_COLUMN      # the mask uniforms' column (ESMDIFF_QXT_PHILOX_COLUMN)
from .constants import SEQUENCE_MASK_TOKEN, SEQUENCE_PAD_TOKEN, STRUCTURE_PAD_TOKEN, STRUCTURE_VOCAB
from .schedule import timestep_embedding

TIME_PHILOX_COLUMN = QXT_PHILOX_COLUMN + 1     # at l = 0: the time uniform of a (structure, draw) pair
_M32 = 0xFFFFFFFF


def philox4x32_10(c: Sequence[int], k: Sequence[int]) -> List[int]:
    """Philox4x32-10 (Salmon et al., SC'11) on Python integers: csrc/ed_math.h::ed_philox4x32_10."""
    c0, c1, c2, c3 = (int(v) & _M32 for v in c)
    k0, k1 = (int(v) & _M32 for v in k)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _M32, (p0 >> 32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return [c0, c1, c2, c3]


def philox_uniform(seed: int, sample: int, step: int, l: int, v: int) -> float:
    """csrc/ed_math.h::ed_philox_uniform: the 24-bit uniform in [0, 1) of (sample, step, position l, column v)."""
    seed, sample = int(seed) & 0xFFFFFFFFFFFFFFFF, int(sample) & 0xFFFFFFFFFFFFFFFF
    o = philox4x32_10([v >> 2, l, sample & _M32, (int(step) & _M32) ^ (((sample >> 32) << 16) & _M32)], [seed & _M32, seed >> 32])
    return (o[v & 3] >> 8) * 2.0 ** -24


def time_uniform(seed: int, sample_index: int, draw: int) -> float:
    return philox_uniform(seed, sample_index, draw, 0, TIME_PHILOX_COLUMN)


def sample_t(m, n: int, eps_t: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """model.py:517-525.  eps_t: the n uniforms (default: torch.rand(n) on `generator`)."""
    _eps_t = torch.rand(n, generator=generator) if eps_t is None else torch.as_tensor(eps_t, dtype=torch.float32)
    if m.antithetic_sampling:
        offset = torch.arange(n) / n
        _eps_t = (_eps_t / n + offset) % 1
    t = (1 - m.sampling_eps) * _eps_t + m.sampling_eps
    if m.importance_sampling:
        return m.noise.importance_sampling_transformation(t)
    return t


def step_scalars(m, t: torch.Tensor) -> Dict[str, Optional[torch.Tensor]]:
    """model.py:405-418 and the factor of :438-443 for times t (n,): {t (after the T rounding), sigma, dsigma (None under
    change_of_variables), conditioning (what the network is conditioned on), move_chance, weight (SIGNED: loss = log_p * weight)},
    each (n,) float32."""
    n = t.shape[0]
    if m.T > 0:                                   # round time step
        t = (t * m.T).to(torch.int) / m.T
        t = t + (1 / m.T)
    sigma = dsigma = None
    if m.change_of_variables:
        conditioning = t
        f_T = torch.log1p(-torch.exp(-m.noise.sigma_max))
        f_0 = torch.log1p(-torch.exp(-m.noise.sigma_min))
        move_chance = torch.exp(f_0 + t * (f_T - f_0))
    else:
        sigma, dsigma = m.noise(t)
        conditioning = sigma
        move_chance = 1 - torch.exp(-sigma)
    if m.change_of_variables or m.importance_sampling:
        weight = torch.log1p(-torch.exp(-m.noise.sigma_min)) * torch.ones(n)
    else:
        weight = -(dsigma / torch.expm1(sigma)) * torch.ones(n)       # -log_p * w == log_p * (-w), bit for bit
    f32 = lambda v: None if v is None else (v * torch.ones(n)).to(torch.float32)
    return {"t": f32(t), "sigma": f32(sigma), "dsigma": f32(dsigma), "conditioning": f32(conditioning),
            "move_chance": f32(move_chance), "weight": f32(weight)}


def _conditioning_rows(m, conditioning: torch.Tensor) -> Optional[torch.Tensor]:
    """_model_wrapper's conditions (model.py:464-471) as the sinusoid rows the engine takes: one per sample."""
    return m.net.conditioning_rows(timestep_embedding(conditioning.to(torch.float32), m.cfg.freq_dim))


def _refuse(m, training: bool) -> None:
    if training:
        raise NotImplementedError("model_step(training=True): there is no backward pass here, and condition dropout / condition "
                                  "masking are training-only; the validation path (training=False) is what this engine runs")
    if getattr(m, "sequence_prediction", False):
        raise NotImplementedError("model_step with sequence_prediction=True: the auxiliary sequence term is not implemented")
    if m.change_of_variables and m.importance_sampling:
        raise AssertionError("change_of_variables and importance_sampling exclude each other")      # model.py:377


def q_xt(m, x, move_chance, condition_seq=None, non_moving_mask=None, *, u=None, seed: Optional[int] = None,
         sample_index=None, draw=None):
    """The reference's q_xt(x, move_chance, condition_seq, non_moving_mask) (model.py:494-512) on the device.  Noise: explicit
    uniforms u (B, L) — what torch.rand(*x.shape) draws — or Philox(seed, sample_index[b], draw[b]).  Returns (xt, condition_seq)."""
    coupled = bool(m.coupled_condition_mask) and condition_seq is not None
    xt, seq = m.net.q_xt(x, torch.as_tensor(move_chance, dtype=torch.float32).reshape(-1), sequence_tokens=condition_seq,
                         coupled=coupled, non_moving_mask=non_moving_mask, u=u, seed=seed, sample_index=sample_index, draw=draw)
    return xt, (seq if condition_seq is not None else None)


def model_step(m, batch, training: bool = False, *, noise: str = "philox", seed: int = 0, sample_index=None):
    """model.py:386-462 with training=False: (loss, {"nelbo": loss}), loss = sum(loss * loss_mask) / sum(loss_mask) over the
    batch as a float64 scalar formed from the per-sample device sums.  batch: structure_tokens, sequence_tokens, mask and
    optionally non_moving_mask, (B, L) each.  noise="philox": times and masks from the keys in the module docstring (draw 0 of
    sample_index[b], default b); "torch-cpu": the reference's stream, torch.rand(B) for the times and then torch.rand(B, L) for
    the mask on the model's parity generator (reset_parity_stream).  m.last_model_step keeps the intermediate values."""
    _refuse(m, training)
    x0 = torch.as_tensor(batch["structure_tokens"]).detach().to("cpu", torch.int64).clone()
    condition_seq = batch["sequence_tokens"]
    B, L = x0.shape
    loss_mask = torch.as_tensor(batch["mask"]).to("cpu") * (x0 != STRUCTURE_PAD_TOKEN)
    idx = list(range(B)) if sample_index is None else [int(v) for v in sample_index]
    gen = None
    if noise == "torch-cpu":
        if m._parity_gen is None or m._parity_seed != seed:
            m.reset_parity_stream(seed)
        gen = m._parity_gen
        eps_t = torch.rand(B, generator=gen)
    elif noise == "philox":
        eps_t = torch.tensor([time_uniform(seed, i, 0) for i in idx], dtype=torch.float32)
    else:
        raise ValueError(f"unknown noise source {noise!r}")
    sc = step_scalars(m, sample_t(m, B, eps_t))
    if m.structure_only:
        condition_seq = None
    u = torch.rand(B, L, generator=gen) if gen is not None else None          # == torch.rand(*x.shape), model.py:503
    xt, condition_seq = q_xt(m, x0, sc["move_chance"], condition_seq, batch.get("non_moving_mask", None), u=u, seed=seed,
                             sample_index=idx, draw=[0] * B)
    net_seq = condition_seq if condition_seq is not None else torch.full((B, L), SEQUENCE_MASK_TOKEN, dtype=torch.int64)   # net.py:412-416
    logits = m.net.forward_logits(xt, net_seq, _conditioning_rows(m, sc["conditioning"]))
    ssum, scnt, log_p = m.net.nelbo_rows(logits, xt, x0, sc["weight"], loss_mask=loss_mask, return_log_p=True)
    ssum, scnt = ssum.detach().cpu().double(), scnt.detach().cpu().to(torch.int64)
    loss = ssum.sum() / scnt.sum()
    m.last_model_step = dict(sc, xt=xt, condition_seq=condition_seq, log_p_theta=log_p, sample_sum=ssum, sample_count=scnt,
                             loss_mask=loss_mask)
    return loss, {"nelbo": loss.detach().clone()}


def draw_scalars(m, seed: int, index: int, num_draws: int) -> Dict[str, Optional[torch.Tensor]]:
    """step_scalars of the num_draws draws of the structure with global index `index`: a pure function of (seed, index,
    num_draws) — one call per structure, so not even the shape of a torch operation depends on the rest of the batch.
    Draw k uses eps_t = (u_k + k) / K in the reference's form (u_k / K + k / K) % 1: its antithetic formula applied across one
    structure's draws (u_k alone with antithetic_sampling off)."""
    u = torch.tensor([time_uniform(seed, index, k) for k in range(num_draws)], dtype=torch.float32)
    return step_scalars(m, sample_t(m, num_draws, u))


def nelbo(m, structure_tokens, sequence_tokens, num_draws: int = 8, seed: int = 0, lengths=None, sample_index=None, mask=None,
          non_moving_mask=None, *, max_batch: Optional[int] = None, return_log_p: bool = False):
    """Per-structure negative ELBO in nats per counted token: for every structure the mean over num_draws independent draws of
    model_step's value on a batch of that one structure (sum(loss * loss_mask) / sum(loss_mask)).

    structure_tokens (N, L) with BOS / EOS (pad id 4099 from lengths[i] on); sequence_tokens (N, L) or (L,) (pad id 1 from
    lengths[i] on; ignored with structure_only); mask (N, L) multiplies the loss mask `labels != 4099` (default: ones — pass one
    that is 0 at BOS / EOS to count residues only); sample_index (N,): the GLOBAL index of each structure (default 0..N-1).
    Every (structure, draw) pair is an independent batch row with its own sigma; pairs are packed into forwards of up to
    max_batch rows (default: the engine's), each trimmed to its longest row and ragged (esmdiff_set_lengths) when rows differ.
    Noise: the keys in the module docstring — draw k of structure i uses the time uniform Philox(seed, i, k, 0, 4105), stratified
    as eps_t = (u_k + k) / K, and the mask uniforms Philox(seed, i, k, l, 4104).  The result of a structure is therefore the same
    alone, in any batch, with any max_batch (bit for bit on an engine whose rows are batch-independent: f32_split, f32).

    Returns (nelbo float64 (N,), spread float64 (N,)) and, with return_log_p, the mean over the draws of log p(x0) per position
    float64 (N, L) (0 on unmasked and padded positions).  spread = std over the draws / sqrt(K) (nan for one draw): the standard
    error of the mean when the draws are independent (antithetic_sampling off).  With antithetic_sampling (the default) the draws
    are stratified in t, one per stratum, not i.i.d.: the figure then still contains the between-strata variation that
    stratification removes, so it is an UPPER estimate of the standard error of the stratified mean, not that error itself.
    A structure whose loss mask is empty has no score: ValueError."""
    _refuse(m, False)
    x0 = torch.as_tensor(structure_tokens).to("cpu", torch.int64)
    N, L = x0.shape
    K = int(num_draws)
    if K < 1:
        raise ValueError("num_draws must be at least 1")
    if m.structure_only or sequence_tokens is None:
        seq = torch.full((N, L), SEQUENCE_MASK_TOKEN, dtype=torch.int64)
        if lengths is not None:
            seq[torch.arange(L)[None] >= torch.tensor([int(v) for v in lengths])[:, None]] = SEQUENCE_PAD_TOKEN
    else:
        seq = torch.as_tensor(sequence_tokens).to("cpu", torch.int64)
        seq = seq[None].expand(N, L) if seq.dim() == 1 else seq
    lens = [L] * N if lengths is None else [int(v) for v in lengths]
    idx = list(range(N)) if sample_index is None else [int(v) for v in sample_index]
    if len(lens) != N or len(idx) != N:
        raise ValueError(f"lengths / sample_index must have one entry per structure ({N})")
    lm = (x0 != STRUCTURE_PAD_TOKEN) if mask is None else (torch.as_tensor(mask).to("cpu") != 0) & (x0 != STRUCTURE_PAD_TOKEN)
    nm = None if non_moving_mask is None else torch.as_tensor(non_moving_mask).to("cpu") != 0
    counted = (lm & (torch.arange(L)[None] < torch.tensor(lens)[:, None])).sum(dim=1)
    if bool((counted == 0).any()):
        raise ValueError(f"structures {[i for i in range(N) if int(counted[i]) == 0]} have an empty loss mask (mask, pad ids and lengths "
                         "leave no token to count): their nelbo would be 0 / 0")
    # ids are checked here once, on the host tensors, so that no chunk pays a device -> host read for it
    if bool(((seq < 0) | (seq > 63)).any()) or bool(((x0 < 0) | (x0 >= STRUCTURE_VOCAB)).any()):
        raise ValueError(f"token id out of range: sequence ids must be in 0..63, structure ids in 0..{STRUCTURE_VOCAB - 1}")
    sc = [draw_scalars(m, seed, idx[i], K) for i in range(N)]
    pairs = [(i, k) for i in range(N) for k in range(K)]
    cap = int(max_batch or m.net.max_batch)
    coupled = bool(m.coupled_condition_mask) and not m.structure_only and sequence_tokens is not None
    sums, cnts, lps = [], [], []
    for c0 in range(0, len(pairs), cap):
        chunk = pairs[c0:c0 + cap]
        rows = torch.tensor([i for i, _ in chunk])
        Lc = max(lens[i] for i, _ in chunk)
        clens = [lens[i] for i, _ in chunk]
        pick = lambda key: torch.stack([sc[i][key][k] for i, k in chunk])
        ssum, scnt, lp = m.net.nelbo_eval(seq[rows, :Lc], x0[rows, :Lc], _conditioning_rows(m, pick("conditioning")),
                                          pick("move_chance"), pick("weight"), non_moving_mask=None if nm is None else nm[rows, :Lc],
                                          seed=seed, sample_index=[idx[i] for i, _ in chunk], draw=[k for _, k in chunk],
                                          loss_mask=lm[rows, :Lc], coupled=coupled, return_log_p=return_log_p,
                                          lengths=clens if min(clens) < Lc else None, check_ids=False)
        sums.append(ssum)
        cnts.append(scnt)
        if return_log_p:
            lps.append(torch.nn.functional.pad(lp.double(), (0, L - Lc)))
    ssum = torch.cat(sums).detach().cpu().double().reshape(N, K)           # (the results' read-back; a uniform-length chunk waits for nothing before it,
                                                                           #  a ragged one pays esmdiff_set_lengths' synchronisation)
    scnt = torch.cat(cnts).detach().cpu().double().reshape(N, K)
    per_draw = ssum / scnt
    # one structure at a time: a reduction over an (N, K) tensor may sum a row in an order that depends on N
    mean = torch.stack([r.mean() for r in per_draw])
    stderr = (torch.stack([r.std(unbiased=True) for r in per_draw]) / math.sqrt(K) if K > 1
              else torch.full((N,), float("nan"), dtype=torch.float64))
    m.last_nelbo = {"per_draw": per_draw, "count": scnt[:, 0]}
    if return_log_p:
        lp = torch.cat(lps).detach().cpu().reshape(N, K, L)
        return mean, stderr, torch.stack([r.sum(dim=0) / K for r in lp])
    return mean, stderr

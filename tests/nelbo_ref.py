"""TEST INFRASTRUCTURE — CPU restatement of the scoring kernels (esmdiff_amd/csrc/score.hip) and a CPU stand-in engine with the
call shapes esmdiff_amd/nelbo.py uses, for tests/test_nelbo_cpu.py and tests/test_gpu_nelbo.py.

  q_xt_ref              model.py:494-512 with explicit uniforms
  philox_mask_uniforms  the device's mask uniforms, restated through the C oracle's Philox (oracle.c_oracle.philox)
  log_p_ref             logits_parameterization + gather at x0 in the CANONICAL operation order (oracle/csrc/sampler_oracle.c)
  canonical_sums        nelbo_reduce_kernel's fixed summation order in float32
  StandinScoreEngine    tests/standin_engine.py plus q_xt / forward_logits / nelbo_rows / nelbo_eval around tests/standin_net.py
(paths relative to /root/reference/slm/models)
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import c_oracle
from oracle import sampler_ref as R
from tests.standin_engine import StandinEngine
from tests.standin_net import StandinNet, standin_sigma_embedder_state

MASK, SEQ_MASK, V = 4096, 32, 4101
QXT_COLUMN = 4104          # ESMDIFF_QXT_PHILOX_COLUMN (include/esmdiff_hip.h)


def philox_uniform(seed, sample, step, l, v):
    """ed_philox_uniform (csrc/ed_math.h) through the C oracle's Philox4x32-10."""
    seed, sample = int(seed), int(sample)
    o = c_oracle.philox([v >> 2, l, sample & 0xFFFFFFFF, (step ^ (((sample >> 32) << 16))) & 0xFFFFFFFF],
                        [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF])
    return np.float32((o[v & 3] >> 8) * 2.0 ** -24)


def philox_mask_uniforms(seed, sample_index, draw, L):
    """(B, L) float32: the uniform q_xt_kernel compares with move_chance[b] at (b, l)."""
    return np.array([[philox_uniform(seed, s, d, l, QXT_COLUMN) for l in range(L)] for s, d in zip(sample_index, draw)],
                    dtype=np.float32)


def q_xt_ref(x0, move_chance, u, non_moving=None, lengths=None, seq=None, coupled=False):
    """model.py:503-511: (xt, seq) as int64 numpy arrays."""
    x0 = np.asarray(x0, dtype=np.int64)
    B, L = x0.shape
    moved = np.asarray(u, dtype=np.float32) < np.asarray(move_chance, dtype=np.float32).reshape(B, 1)
    if non_moving is not None:
        moved &= ~(np.asarray(non_moving) != 0)
    if lengths is not None:
        moved &= np.arange(L)[None] < np.asarray(lengths).reshape(B, 1)
    xt = np.where(moved, MASK, x0)
    if seq is None:
        return xt, None
    seq = np.asarray(seq, dtype=np.int64)
    return xt, (np.where(moved, SEQ_MASK, seq) if coupled else seq)


def log_p_ref(logits, xt, x0):
    """(B, L) float32: logits_parameterization(logits, xt) gathered at x0, canonical order — the value nelbo_rows_kernel writes."""
    xt, x0 = np.asarray(xt, dtype=np.int64), np.asarray(x0, dtype=np.int64)
    lp = c_oracle.logits_parameterization(np.asarray(logits, dtype=np.float32), xt)
    return np.take_along_axis(lp, x0[..., None], axis=-1)[..., 0]


def _halving_tree(part):
    """part (256,) float32 -> the kernels' four-wave sum."""
    w = []
    for c in range(4):
        t = part[c * 64:(c + 1) * 64].astype(np.float32).copy()
        off = 32
        while off >= 1:
            t[:off] = t[:off] + t[off:2 * off]
            off >>= 1
        w.append(t[0])
    return np.float32(np.float32(w[0] + w[1]) + np.float32(w[2] + w[3]))


def canonical_sums(log_p, weight, loss_mask=None, lengths=None):
    """nelbo_rows_kernel's row_loss = log_p * weight[b] and nelbo_reduce_kernel's sums: (sample_sum float32 (B,), count int32 (B,))."""
    log_p = np.asarray(log_p, dtype=np.float32)
    B, L = log_p.shape
    on = np.ones((B, L), dtype=bool) if loss_mask is None else np.asarray(loss_mask) != 0
    if lengths is not None:
        on = on & (np.arange(L)[None] < np.asarray(lengths).reshape(B, 1))
    row_loss = log_p * np.asarray(weight, dtype=np.float32).reshape(B, 1)
    sums = np.zeros(B, dtype=np.float32)
    for b in range(B):
        part = np.zeros(256, dtype=np.float32)
        for l in range(L):
            part[l % 256] = part[l % 256] + row_loss[b, l] * np.float32(on[b, l])
        sums[b] = _halving_tree(part)
    return sums, on.sum(axis=1).astype(np.int32)


class StandinScoreEngine(StandinEngine):
    """The engine calls of esmdiff_amd/nelbo.py on the CPU: the lookup stand-in net with the stand-in sigma embedder as the
    network, the restatements above as the kernels.  Records every nelbo_eval call in `calls`."""

    def __init__(self, max_batch=64, max_len=64, hidden=32, uniform_logits=False):
        super().__init__(max_batch=max_batch, max_len=max_len)
        self.emb = R.TimestepEmbedderRef(hidden)
        self.emb.load_state_dict(standin_sigma_embedder_state(hidden))
        self.netmod = StandinNet(hidden)
        self.uniform_logits = uniform_logits       # every logit 0 but the MASK column: log_p = -log 4100 on masked rows
        self.calls = []

    def conditioning_rows(self, t_freq):
        return t_freq

    def forward_logits(self, x, seq, t_freq, **kw):
        x, seq = torch.as_tensor(x), torch.as_tensor(seq)
        if self.uniform_logits:
            z = torch.zeros(*x.shape, V)
            z[..., MASK] = 3.0
            return z
        cond = None
        if t_freq is not None:
            with torch.no_grad():    # one row at a time: a CPU matmul's bits depend on its batch, the engine's rows must not
                c = torch.cat([self.emb.mlp(t_freq[b:b + 1].to(torch.float32)) for b in range(x.shape[0])])
                cond = torch.tile(c[:, None, :], (1, x.shape[1], 1))
        return self.netmod(structure_tokens=x, sequence_tokens=seq, auxiliary_embeddings=cond).structure_logits

    def q_xt(self, x0, move_chance, *, sequence_tokens=None, coupled=False, non_moving_mask=None, u=None, seed=None,
             sample_index=None, draw=None, lengths=None):
        x0 = torch.as_tensor(x0)
        if u is None:
            u = philox_mask_uniforms(seed, sample_index, [0] * len(sample_index) if draw is None else draw, x0.shape[1])
        xt, seq = q_xt_ref(x0.numpy(), torch.as_tensor(move_chance).numpy(), np.asarray(u), non_moving_mask, lengths,
                           None if sequence_tokens is None else torch.as_tensor(sequence_tokens).numpy(), coupled)
        return torch.from_numpy(xt), (None if seq is None else torch.from_numpy(seq))

    def nelbo_rows(self, logits, xt, x0, weight, *, loss_mask=None, return_log_p=True, lengths=None):
        lp = log_p_ref(logits.numpy(), torch.as_tensor(xt).numpy(), torch.as_tensor(x0).numpy())
        s, c = canonical_sums(lp, torch.as_tensor(weight).numpy(), None if loss_mask is None else torch.as_tensor(loss_mask).numpy(),
                              lengths)
        return torch.from_numpy(s), torch.from_numpy(c), (torch.from_numpy(lp) if return_log_p else None)

    def nelbo_eval(self, seq, x0, t_freq, move_chance, weight, *, non_moving_mask=None, u=None, seed=None, sample_index=None,
                   draw=None, loss_mask=None, coupled=False, return_log_p=False, lengths=None, check_ids=True):
        assert x0.shape[0] <= self.max_batch, "the host must chunk to the engine capacity"
        self.calls.append({"B": x0.shape[0], "L": x0.shape[1], "sample_index": list(sample_index), "draw": list(draw),
                           "lengths": None if lengths is None else list(lengths)})
        xt, net_seq = self.q_xt(x0, move_chance, sequence_tokens=seq, coupled=coupled, non_moving_mask=non_moving_mask, u=u,
                                seed=seed, sample_index=sample_index, draw=draw, lengths=lengths)
        logits = self.forward_logits(xt, net_seq, t_freq)
        return self.nelbo_rows(logits, xt, x0, weight, loss_mask=loss_mask, return_log_p=return_log_p, lengths=lengths)


class ScoreModel:
    """The attributes esmdiff_amd/nelbo.py reads from a model, around a stand-in engine (no GPU, no Engine)."""

    def __init__(self, net, noise, *, antithetic_sampling=True, importance_sampling=False, change_of_variables=False, T=0,
                 sampling_eps=1e-3, structure_only=False, coupled_condition_mask=False, freq_dim=256):
        from types import SimpleNamespace
        self.net, self.noise = net, noise
        self.cfg = SimpleNamespace(freq_dim=freq_dim)
        self.antithetic_sampling, self.importance_sampling, self.change_of_variables = antithetic_sampling, importance_sampling, change_of_variables
        self.T, self.sampling_eps, self.structure_only, self.coupled_condition_mask = T, sampling_eps, structure_only, coupled_condition_mask
        self.sequence_prediction = False
        self._parity_gen = self._parity_seed = None

    def reset_parity_stream(self, seed):
        self._parity_gen = torch.Generator().manual_seed(seed)
        self._parity_seed = seed

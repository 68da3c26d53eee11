"""Python host side of the C ABI (include/esmdiff_hip.h): owns an esmdiff_engine and exposes the call
sites of the reference's hot path with PyTorch-ROCm tensors as plain device-memory containers.

  Engine.forward_logits  <- self.net(...).structure_logits           model.py:475-481
  Engine.ddpm_step       <- _ddpm_update's sampling half              model.py:583-607, 24-28
  Engine.ddpm_sample     <- MaskedDiffusionLanguageModeling.ddpm_sample  model.py:543-581
(paths relative to /root/reference/slm/models)
"""
from __future__ import annotations

import ctypes
import contextlib
from typing import Dict, Optional, Sequence

import torch

from . import _native as N
from .config import ModelConfig
from .constants import SEQUENCE_PAD_TOKEN, STRUCTURE_MASK_TOKEN, STRUCTURE_PAD_TOKEN, STRUCTURE_VOCAB
from .schedule import DDPMSchedule


def _ptr(t: Optional[torch.Tensor]):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _stream() -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _require_gpu():
    if not torch.cuda.is_available():
        raise RuntimeError("esmdiff_amd needs an MI355X (gfx950) GPU: torch.cuda.is_available() is False and "
                           "there is no CPU fallback")


def _weight_table(state_dict: Dict[str, torch.Tensor], device: torch.device):
    """(keep, table): the caller's tensors (any float dtype) uploaded as device containers, and the esmdiff_weight array that
    names them.  A create entry makes its own bf16 / re-laid-out copies, after which `keep` is released.  Call it with `device`
    current."""
    keep, table = [], (N.Weight * len(state_dict))()
    for i, (name, t) in enumerate(state_dict.items()):
        if t.dtype not in (torch.float32, torch.bfloat16):
            t = t.float()
        d = t.detach().to(device).contiguous()
        keep.append(d)
        shape = (ctypes.c_int64 * 4)(*(list(d.shape) + [0] * (4 - d.dim())))
        table[i] = N.Weight(name.encode(), d.data_ptr(), N.DT_F32 if d.dtype == torch.float32 else N.DT_BF16, d.dim(), shape)
    torch.cuda.synchronize()
    return keep, table


class _Handle:
    """Lifetime of one native handle `_h` of `_lib`: `_destroy` names the entry that frees it."""
    _destroy = ""

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            getattr(self._lib, self._destroy)(self._h)
            self._h = ctypes.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Engine(_Handle):
    """One engine per (process, device).  Not thread-safe.  All work is enqueued on torch's current stream."""
    _destroy = "esmdiff_engine_destroy"

    def __init__(self, cfg: ModelConfig, state_dict: Dict[str, torch.Tensor], max_batch: int, max_len: int,
                 device: int = 0, precision: str = "bf16", head_precision: Optional[str] = None):
        """precision: "bf16" (the throughput path: bf16 MFMA, f32 accumulate and residual stream), "f32" (the strict
        path, csrc/strict.hip: float32 weights and activations on the f32-input MFMA — the reference's own arithmetic,
        checkpoint_utils.py:59-73; ~1/12 of the throughput; the referee) or "f32_split" (the strict path with every large
        linear as three f16 MFMA passes over split operands, csrc/gemm_split.hip: float32-grade, ~1/4 of the bf16 throughput) or
        "f16" (the bf16 path's kernels compiled with IEEE-half operands, csrc/ed_half.h: same speed, 1/8 of the operand rounding).
        head_precision="f32" (bf16 / f16 engines): final LayerNorm + output head in float32 grade on the split kernels."""
        _require_gpu()
        if precision not in N.PRECISION:
            raise ValueError(f"precision must be one of {sorted(N.PRECISION)}, got {precision!r}")
        if head_precision not in (None, "f32") and head_precision != precision:
            raise ValueError(f"head_precision must be None / {precision!r} (the body's precision) or 'f32', got {head_precision!r}")
        self.precision = precision
        self.head_precision = "f32" if (head_precision == "f32" or precision in ("f32", "f32_split")) else precision
        self.cfg = cfg
        self.device = torch.device("cuda", device)
        self.max_batch, self.max_len = max_batch, max_len
        self._lib = N.lib()
        self._h = ctypes.c_void_p(0)
        c = N.Config(cfg.d_model, cfg.n_heads, cfg.n_layers, cfg.ffn_hidden, cfg.n_structure_heads, cfg.freq_dim,
                     max_batch, max_len, cfg.residue_scale, int(cfg.time_conditioning), N.PRECISION[precision],
                     1 if (head_precision == "f32" and precision in ("bf16", "f16")) else 0)
        with torch.cuda.device(self.device):
            keep, table = _weight_table(state_dict, self.device)
            code = self._lib.esmdiff_engine_create(ctypes.byref(c), table, len(state_dict), device,
                                                   ctypes.byref(self._h))
        if code != 0:
            raise RuntimeError(f"esmdiff_engine_create failed ({code}): "
                               f"{self._lib.esmdiff_last_error(None).decode()}")
        del keep
        self.ld_logits = (cfg.n_structure_heads + 3) // 4 * 4
        self.has_geom = any(k.endswith("transformer.blocks.0.geom_attn.proj.weight") for k in state_dict)
        self.has_sigma_embedder = any(k.startswith("sigma_embedder.mlp.0.") for k in state_dict)
        self.n_sequence_heads = next((int(v.shape[0]) for k, v in state_dict.items() if k.endswith("output_heads.sequence_head.3.weight")), 0)
        self._frames = None
        self._lengths = None   # set_lengths

    def branch_linear_layernorm(self, A: torch.Tensor, W: torch.Tensor, x: torch.Tensor, alpha: float, w: torch.Tensor,
                                b: Optional[torch.Tensor]):
        """x += alpha * (A @ W^T) in place (f32), returns (LayerNorm(x) * w (+ b) as bf16, K slices used): the small-batch
        form of a residual branch (esmdiff_branch_linear_layernorm)."""
        M, K = A.shape
        Nn = W.shape[0]
        assert A.dtype == W.dtype == torch.bfloat16 and x.dtype == torch.float32 and x.shape == (M, Nn)
        assert A.is_contiguous() and W.is_contiguous() and x.is_contiguous()
        y = torch.empty(M, Nn, dtype=torch.bfloat16, device=A.device)
        S = ctypes.c_int32(0)
        self._chk(self._lib.esmdiff_branch_linear_layernorm(self._h, _ptr(A), _ptr(W), _ptr(x), float(alpha),
                                                            _ptr(w.float().contiguous()),
                                                            _ptr(None if b is None else b.float().contiguous()), _ptr(y),
                                                            M, Nn, K, ctypes.byref(S), _stream()))
        return y, int(S.value)

    # ------------------------------------------------------------------------------------------
    def _chk(self, code):
        N.check(code, self._h)

    def _tok(self, t: torch.Tensor, B: int, L: int) -> torch.Tensor:
        t = t.to(device=self.device, dtype=torch.int64)
        if t.dim() == 1:
            t = t[None].expand(B, L)
        return t.contiguous()

    def _check_ids(self, seq: torch.Tensor, x: torch.Tensor) -> None:
        """The embedding tables hold 64 sequence rows and 4101 structure rows (net.py:445-466; -1 means MASK): an id
        outside them is a caller error, reported here instead of being looked up."""
        bad = ((seq < 0) | (seq > 63)).any() | ((x < -1) | (x >= STRUCTURE_VOCAB)).any()
        if bool(bad):
            raise ValueError(f"token id out of range: sequence ids must be in 0..63 (got {int(seq.min())}..{int(seq.max())}), "
                             f"structure ids in -1..{STRUCTURE_VOCAB - 1} (got {int(x.min())}..{int(x.max())})")

    def conditioning_rows(self, t_freq: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
        """What `_model_wrapper` conditions on (model.py:464-471): sigma_embedder(sigma) with time conditioning,
        sigma_embedder(0) without it when the embedder exists (_process_sigma zeroes sigma, model.py:535-541), nothing
        for a model without a sigma embedder.  In: (n, freq_dim) sinusoids of the real sigmas; out: the rows to feed."""
        if t_freq is None or not self.has_sigma_embedder:
            return None
        if self.cfg.time_conditioning:
            return t_freq
        from .schedule import timestep_embedding
        zero = timestep_embedding(torch.zeros(1, dtype=torch.float32), self.cfg.freq_dim)
        return zero.expand(t_freq.shape[0], -1).contiguous() if t_freq.dim() == 2 else zero[0]

    # ---- ragged batches (esmdiff_set_lengths) ------------------------------------------------------------------------------
    def set_lengths(self, lengths: Optional[Sequence[int]]) -> None:
        """Ragged batch for the following calls (esmdiff_set_lengths): sample b of a (B, L) batch is valid on tokens [0, lengths[b])
        (BOS and EOS counted) and holds the pad ids beyond (sequence 1, structure 4099).  A valid position's logits and ids are
        then what the sample gives alone at L = lengths[b].  None clears it."""
        if lengths is None:
            self._chk(self._lib.esmdiff_set_lengths(self._h, None, 0))
            self._lengths = None
            return
        lens = [int(v) for v in lengths]
        arr = (ctypes.c_int32 * max(1, len(lens)))(*lens)
        self._chk(self._lib.esmdiff_set_lengths(self._h, arr, len(lens)))
        self._lengths = lens

    def _check_padding(self, lens: Sequence[int], seq: torch.Tensor, x: Optional[torch.Tensor]) -> None:
        """Host check of a ragged batch: every length in 3..L, the pad ids from each length on."""
        B, L = seq.shape
        if len(lens) != B:
            raise ValueError(f"{len(lens)} lengths for a batch of {B}")
        if min(lens) < 3 or max(lens) > L:
            raise ValueError(f"lengths must be in 3..L={L} (BOS, one residue, EOS), got {min(lens)}..{max(lens)}")
        pos = torch.arange(L, device=seq.device)[None]
        pad = pos >= torch.tensor(lens, device=seq.device)[:, None]
        if bool((pad & (seq != SEQUENCE_PAD_TOKEN)).any()):
            raise ValueError(f"ragged batch: sequence positions from each length on must hold the pad id {SEQUENCE_PAD_TOKEN}")
        if x is not None and bool((pad & (x != STRUCTURE_PAD_TOKEN)).any()):
            raise ValueError(f"ragged batch: structure positions from each length on must hold the pad id {STRUCTURE_PAD_TOKEN}")

    @contextlib.contextmanager
    def _lengths_for_call(self, lengths: Optional[Sequence[int]], seq: torch.Tensor, x: Optional[torch.Tensor]):
        """`lengths=` of one call: set for the call and cleared afterwards (None: whatever set_lengths left in place)."""
        if lengths is None:
            yield
            return
        lens = [int(v) for v in lengths]
        self._check_padding(lens, seq, x)
        self.set_lengths(lens)
        try:
            yield
        finally:
            self.set_lengths(None)

    def forward_logits(self, x: torch.Tensor, sequence_tokens: torch.Tensor, t_freq: Optional[torch.Tensor],
                       out: Optional[torch.Tensor] = None, check_ids: bool = True,
                       lengths: Optional[Sequence[int]] = None) -> torch.Tensor:
        """x, sequence_tokens: (B,L) int64.  t_freq: (freq_dim,) f32 sinusoid of the sigma all samples share, (B, freq_dim) for
        one sigma per sample (esmdiff_forward_logits_sigmas), or None.  lengths: a ragged batch for this call (set_lengths).
        Returns raw structure logits, a (B,L,4101) view of a (B,L,ld) float32 buffer."""
        B, L = x.shape
        x = self._tok(x, B, L)
        seq = self._tok(sequence_tokens, B, L)
        if lengths is not None:
            with self._lengths_for_call(lengths, seq, x):
                return self.forward_logits(x, seq, t_freq, out, check_ids)
        if check_ids:      # (a device -> host read-back: loops that feed the engine its own output skip it after the first call)
            self._check_ids(seq, x)
        if out is None:
            out = torch.empty(B, L, self.ld_logits, dtype=torch.float32, device=self.device)
        tf = None if t_freq is None else t_freq.to(device=self.device, dtype=torch.float32).contiguous()
        if tf is not None and tf.dim() == 2:
            if tf.shape[0] != B:
                raise ValueError(f"per-sample conditioning: {tf.shape[0]} sinusoid rows for a batch of {B}")
            fn = self._lib.esmdiff_forward_logits_sigmas
        else:
            fn = self._lib.esmdiff_forward_logits
        self._chk(fn(self._h, _ptr(seq), _ptr(x), _ptr(tf), _ptr(out), out.shape[-1], B, L, _stream()))
        return out[..., :self.cfg.n_structure_heads]

    def embeddings(self, B: int, L: int) -> torch.Tensor:
        """ESMOutput.embeddings of the forward that just ran (net.py:468-469): the pre-norm hidden state, (B, L, d) f32."""
        out = torch.empty(B, L, self.cfg.d_model, dtype=torch.float32, device=self.device)
        self._chk(self._lib.esmdiff_get_embeddings(self._h, _ptr(out), B, L, _stream()))
        return out

    def sequence_logits(self, B: int, L: int) -> torch.Tensor:
        """ESMOutput.sequence_logits of the forward that just ran (net.py:310-311; esmdiff_get_sequence_logits): (B, L,
        n_sequence_heads) f32.  Needs output_heads.sequence_head.* in the state dict."""
        n = self.n_sequence_heads
        if not n:
            raise RuntimeError("this engine was built without output_heads.sequence_head.* weights")
        out = torch.empty(B, L, n, dtype=torch.float32, device=self.device)
        self._chk(self._lib.esmdiff_get_sequence_logits(self._h, _ptr(out), n, B, L, _stream()))
        return out

    def ddpm_step(self, x: torch.Tensor, logits: torch.Tensor, mc_t: float, mc_s: float, *, final: bool = False,
                  u: Optional[torch.Tensor] = None, seed: Optional[int] = None, sample_offset: int = 0,
                  step: int = 0) -> torch.Tensor:
        """In-place update of x (B,L) int64 from RAW logits (B,L,>=4101) float32 (last dim may be a strided
        view of a padded buffer).  Noise: explicit `u` (B,L,4101) or Philox(seed, sample_offset, step)."""
        B, L = x.shape
        assert x.dtype == torch.int64 and x.is_cuda and x.is_contiguous()
        assert logits.dtype == torch.float32 and logits.is_cuda and logits.stride(-1) == 1
        ld = logits.stride(1)
        assert logits.stride(0) == ld * L and ld >= STRUCTURE_VOCAB
        rng = None
        if u is not None:
            u = u.to(device=self.device, dtype=torch.float32).contiguous()
            assert u.shape == (B, L, STRUCTURE_VOCAB)
        elif not final:
            if seed is None:
                raise ValueError("ddpm_step needs explicit uniforms `u` or a Philox `seed`")
        if seed is not None:
            rng = N.Rng(int(seed), int(sample_offset))
        self._chk(self._lib.esmdiff_ddpm_step(self._h, _ptr(x), _ptr(logits), ld, float(mc_t), float(mc_s),
                                              int(final), _ptr(u), ctypes.byref(rng) if rng else None, int(step),
                                              B, L, _stream()))
        return x

    def ddpm_step_margin(self, x: torch.Tensor, logits: torch.Tensor, mc_t: float, mc_s: float, *, final: bool,
                         seed: int, sample_offset: int, step: int, margin: float, flags: torch.Tensor) -> torch.Tensor:
        """ddpm_step (Philox noise) that also sets flags[b] = 1 (int32 [B], zeroed by the caller) when some masked row of
        sample b was decided by less than `margin` (esmdiff_ddpm_step_margin; used by certified.py)."""
        B, L = x.shape
        assert x.dtype == torch.int64 and x.is_cuda and x.is_contiguous()
        assert logits.dtype == torch.float32 and logits.is_cuda and logits.stride(-1) == 1
        ld = logits.stride(1)
        assert logits.stride(0) == ld * L and ld >= STRUCTURE_VOCAB
        assert flags.dtype == torch.int32 and flags.is_cuda and flags.numel() == B and flags.is_contiguous()
        rng = N.Rng(int(seed), int(sample_offset))
        self._chk(self._lib.esmdiff_ddpm_step_margin(self._h, _ptr(x), _ptr(logits), ld, float(mc_t), float(mc_s), int(final),
                                                     ctypes.byref(rng), int(step), B, L, float(margin), _ptr(flags),
                                                     _stream()))
        return x

    @staticmethod
    def sample_step_params_host(sample_index, mc_t, mc_s, step, final):
        """Host sequences (one entry per sample) -> the esmdiff_sample_step records as a uint8 numpy array (n, 24)."""
        import numpy as np
        n = len(sample_index)
        rec = np.zeros(n, dtype=N.SAMPLE_STEP_DTYPE)
        rec["sample_index"], rec["step"], rec["final"] = sample_index, step, final
        rec["move_chance_t"], rec["move_chance_s"] = mc_t, mc_s
        return rec.view(np.uint8).reshape(n, -1)

    def sample_step_params(self, sample_index, mc_t, mc_s, step, final) -> torch.Tensor:
        """... as the device array ddpm_step_rows takes."""
        return torch.from_numpy(self.sample_step_params_host(sample_index, mc_t, mc_s, step, final)).to(self.device)

    def ddpm_step_rows(self, x: torch.Tensor, logits: torch.Tensor, params: torch.Tensor, *, seed: int,
                       eps: Optional[float] = None, flags: Optional[torch.Tensor] = None,
                       gaps: Optional[torch.Tensor] = None) -> torch.Tensor:
        """ddpm_step with one parameter set per sample (esmdiff_ddpm_step_rows): params from sample_step_params.  With `eps`
        (a bound on the logit error, certified.py) flags[b] (int32, zeroed by the caller) is set where a masked row of sample b
        was decided by less than exp(2 eps) (final passes: 2 eps in log p), and gaps[b] (f32, +inf on entry) gets the sample's
        smallest gap in log units."""
        import math
        B, L = x.shape
        assert x.dtype == torch.int64 and x.is_cuda and x.is_contiguous()
        assert logits.dtype == torch.float32 and logits.is_cuda and logits.stride(-1) == 1
        ld = logits.stride(1)
        assert logits.stride(0) == ld * L and ld >= STRUCTURE_VOCAB
        assert params.dtype == torch.uint8 and params.is_cuda and params.shape == (B, 24) and params.is_contiguous()
        for t_, dt in ((flags, torch.int32), (gaps, torch.float32)):
            assert t_ is None or (t_.dtype == dt and t_.is_cuda and t_.numel() == B and t_.is_contiguous())
        if (flags is not None or gaps is not None) and eps is None:
            raise ValueError("flags / gaps need eps")
        e2 = 0.0 if eps is None else 2.0 * float(eps)
        self._chk(self._lib.esmdiff_ddpm_step_rows(self._h, _ptr(x), _ptr(logits), ld, _ptr(params), int(seed), B, L,
                                                   math.exp(e2), e2, _ptr(flags), _ptr(gaps), _stream()))
        return x

    def logit_error_stats(self, a: torch.Tensor, b: torch.Tensor, x: torch.Tensor, all_columns: bool = False) -> torch.Tensor:
        """(n, L, 8) f32 = per token row {max |e|, sum e^2, max |d|, sum d^2, max e - min e, H(a) - H(b), H(b), 0}, e = a - b over the
        columns a decision reads — all but the MASK column (the ddpm draw), or every column with all_columns (the gibbs step) — of
        the rows of x (n, L) that are MASK; d = the error of neighbouring logit differences, the range bounds the error of ANY
        pair's difference, H = the row's softmax entropy; zeros elsewhere (esmdiff_logit_error_stats)."""
        n, L = x.shape
        for t_ in (a, b):
            assert t_.dtype == torch.float32 and t_.is_cuda and t_.stride(-1) == 1 and t_.shape[:2] == (n, L)
            assert t_.stride(0) == t_.stride(1) * L
        assert x.dtype == torch.int64 and x.is_cuda and x.is_contiguous()
        out = torch.empty(n, L, 8, dtype=torch.float32, device=self.device)
        N.check(self._lib.esmdiff_logit_error_stats(_ptr(a), a.stride(1), _ptr(b), b.stride(1), _ptr(x), n * L,
                                                    self.cfg.n_structure_heads, int(bool(all_columns)), _ptr(out), _stream()))
        return out

    # ---- scoring (esmdiff_q_xt / esmdiff_nelbo_rows / esmdiff_nelbo_eval; host side in esmdiff_amd/nelbo.py) ----------------
    def _per_sample(self, v, B: int, dtype: torch.dtype, what: str) -> torch.Tensor:
        t = torch.as_tensor(v).reshape(-1).to(device=self.device, dtype=dtype).contiguous()
        if t.numel() != B:
            raise ValueError(f"{what}: {t.numel()} values for a batch of {B}")
        return t

    def _mask_u8(self, m, B: int, L: int, what: str) -> Optional[torch.Tensor]:
        if m is None:
            return None
        m = (torch.as_tensor(m) != 0).to(device=self.device, dtype=torch.uint8).contiguous()
        if tuple(m.shape) != (B, L):
            raise ValueError(f"{what}: shape {tuple(m.shape)}, expected {(B, L)}")
        return m

    def _noise_args(self, B: int, L: int, u, seed, sample_index, draw):
        """Explicit uniforms (B, L), or the Philox key arrays (u64 as int64 bits, int32)."""
        if u is not None:
            u = torch.as_tensor(u).to(device=self.device, dtype=torch.float32).contiguous()
            if tuple(u.shape) != (B, L):
                raise ValueError(f"u: shape {tuple(u.shape)}, expected {(B, L)}")
            return u, None, None, 0
        if seed is None or sample_index is None:
            raise ValueError("masking noise: explicit uniforms `u` (B, L), or a Philox `seed` with `sample_index` (and `draw`)")
        si = self._per_sample([int(v) for v in sample_index], B, torch.int64, "sample_index")
        dr = self._per_sample([0] * B if draw is None else [int(v) for v in draw], B, torch.int32, "draw")
        return None, si, dr, int(seed)

    def q_xt(self, x0: torch.Tensor, move_chance, *, sequence_tokens: Optional[torch.Tensor] = None, coupled: bool = False,
             non_moving_mask=None, u=None, seed: Optional[int] = None, sample_index=None, draw=None):
        """The forward (masking) process, model.py:494-512 (esmdiff_q_xt): xt = MASK where u < move_chance[b] and the position
        is not in non_moving_mask (and below the sample's length while lengths are set), else x0.  u: explicit uniforms (B, L),
        or Philox(seed, sample_index[b], draw[b], l).  Returns (xt, sequence) — the sequence with the coupled mask when
        `coupled`, else as given."""
        B, L = x0.shape
        x0 = self._tok(x0, B, L)
        seq = None if sequence_tokens is None else self._tok(sequence_tokens, B, L)
        mc = self._per_sample(move_chance, B, torch.float32, "move_chance")
        nm = self._mask_u8(non_moving_mask, B, L, "non_moving_mask")
        u, si, dr, seed = self._noise_args(B, L, u, seed, sample_index, draw)
        xt = torch.empty_like(x0)
        seq_out = torch.empty_like(seq) if (coupled and seq is not None) else None
        self._chk(self._lib.esmdiff_q_xt(self._h, _ptr(x0), _ptr(seq), _ptr(mc), _ptr(nm), _ptr(u), seed, _ptr(si), _ptr(dr),
                                         _ptr(xt), _ptr(seq_out), B, L, _stream()))
        return xt, (seq_out if seq_out is not None else seq)

    def nelbo_rows(self, logits: torch.Tensor, xt: torch.Tensor, x0: torch.Tensor, weight, *, loss_mask=None,
                   return_log_p: bool = True, check_ids: bool = True):
        """RAW logits (B, L, >= 4101) f32 -> (sample_sum f32 (B,), sample_count int32 (B,), log_p f32 (B, L) or None):
        log p(x0) of the re-parameterised rows, times the signed per-sample weight, summed over the loss mask per sample in a
        fixed order (esmdiff_nelbo_rows)."""
        B, L = xt.shape
        assert logits.dtype == torch.float32 and logits.is_cuda and logits.stride(-1) == 1 and tuple(logits.shape[:2]) == (B, L)
        ld = logits.stride(1)
        assert logits.stride(0) == ld * L and ld >= STRUCTURE_VOCAB and logits.shape[-1] >= STRUCTURE_VOCAB
        xt, x0 = self._tok(xt, B, L), self._tok(x0, B, L)
        if check_ids and bool(((x0 < 0) | (x0 >= STRUCTURE_VOCAB)).any()):     # (a device -> host read-back)
            raise ValueError(f"structure ids must be in 0..{STRUCTURE_VOCAB - 1}")
        w = self._per_sample(weight, B, torch.float32, "weight")
        lm = self._mask_u8(loss_mask, B, L, "loss_mask")
        ssum = torch.empty(B, dtype=torch.float32, device=self.device)
        scnt = torch.empty(B, dtype=torch.int32, device=self.device)
        lp = torch.empty(B, L, dtype=torch.float32, device=self.device) if return_log_p else None
        self._chk(self._lib.esmdiff_nelbo_rows(self._h, _ptr(logits), ld, _ptr(xt), _ptr(x0), _ptr(w), _ptr(lm), _ptr(lp),
                                               _ptr(ssum), _ptr(scnt), B, L, _stream()))
        return ssum, scnt, lp

    def nelbo_eval(self, sequence_tokens: torch.Tensor, x0: torch.Tensor, t_freq: Optional[torch.Tensor], move_chance, weight, *,
                   non_moving_mask=None, u=None, seed: Optional[int] = None, sample_index=None, draw=None, loss_mask=None,
                   coupled: bool = False, return_log_p: bool = False, lengths: Optional[Sequence[int]] = None,
                   check_ids: bool = True):
        """Mask, forward with one sigma per sample, score — one batch, queued without a host synchronisation
        (esmdiff_nelbo_eval).  t_freq (B, freq_dim): the sinusoids of the conditioning sigmas as conditioning_rows returns
        them, or None.  Returns (sample_sum f32 (B,), sample_count int32 (B,), log_p (B, L) or None) on the device."""
        B, L = x0.shape
        x0 = self._tok(x0, B, L)
        seq = self._tok(sequence_tokens, B, L)
        if lengths is not None:
            with self._lengths_for_call(lengths, seq, x0):
                return self.nelbo_eval(seq, x0, t_freq, move_chance, weight, non_moving_mask=non_moving_mask, u=u, seed=seed,
                                       sample_index=sample_index, draw=draw, loss_mask=loss_mask, coupled=coupled,
                                       return_log_p=return_log_p, check_ids=check_ids)
        if check_ids:
            self._check_ids(seq, x0)
            if bool((x0 < 0).any()):
                raise ValueError(f"structure ids must be in 0..{STRUCTURE_VOCAB - 1}")
        tf = None
        if t_freq is not None:
            tf = t_freq.to(device=self.device, dtype=torch.float32).contiguous()
            if tuple(tf.shape) != (B, self.cfg.freq_dim):
                raise ValueError(f"t_freq: shape {tuple(tf.shape)}, expected {(B, self.cfg.freq_dim)} (one sinusoid per sample)")
        mc = self._per_sample(move_chance, B, torch.float32, "move_chance")
        w = self._per_sample(weight, B, torch.float32, "weight")
        nm = self._mask_u8(non_moving_mask, B, L, "non_moving_mask")
        lm = self._mask_u8(loss_mask, B, L, "loss_mask")
        u, si, dr, seed = self._noise_args(B, L, u, seed, sample_index, draw)
        ssum = torch.empty(B, dtype=torch.float32, device=self.device)
        scnt = torch.empty(B, dtype=torch.int32, device=self.device)
        lp = torch.empty(B, L, dtype=torch.float32, device=self.device) if return_log_p else None
        self._chk(self._lib.esmdiff_nelbo_eval(self._h, _ptr(seq), _ptr(x0), _ptr(tf), _ptr(mc), _ptr(w), _ptr(nm), _ptr(u), seed,
                                               _ptr(si), _ptr(dr), _ptr(lm), int(bool(coupled)), _ptr(ssum), _ptr(scnt), _ptr(lp),
                                               B, L, _stream()))
        return ssum, scnt, lp

    def ddpm_sample(self, sequence_tokens: torch.Tensor, schedule: DDPMSchedule, *, seed: int,
                    sample_offset: int = 0, input_prior: Optional[torch.Tensor] = None,
                    lengths: Optional[Sequence[int]] = None, sample_index: Optional[Sequence[int]] = None) -> torch.Tensor:
        """Whole ancestral sampling loop on the device with Philox noise (esmdiff_ddpm_sample).  lengths: a ragged batch
        (set_lengths; without input_prior the padded positions start as the structure pad id).  sample_index: (B,) Philox sample
        index of each row instead of sample_offset + b — then the loop runs on the host, one forward and one
        esmdiff_ddpm_step_rows per update, and every row draws exactly what its own sample index gives in a plain call."""
        B, L = sequence_tokens.shape
        seq = self._tok(sequence_tokens, B, L)
        if input_prior is None:
            x = torch.full((B, L), STRUCTURE_MASK_TOKEN, dtype=torch.int64, device=self.device)
            if lengths is not None:
                pos = torch.arange(L, device=self.device)[None]
                x[pos >= torch.tensor([int(v) for v in lengths], device=self.device)[:, None]] = STRUCTURE_PAD_TOKEN
        else:
            if tuple(input_prior.shape) != (B, L):
                raise ValueError(f"Invalid input_prior shape: {tuple(input_prior.shape)} v.s. (seq) {(B, L)}")
            x = input_prior.to(device=self.device, dtype=torch.int64).contiguous().clone()
        self._check_ids(seq, x)
        if sample_index is not None and len(sample_index) != B:
            raise ValueError(f"sample_index: {len(sample_index)} entries for a batch of {B}")
        T = schedule.num_steps
        f32 = lambda t: t.detach().to("cpu", torch.float32).contiguous()
        mc_t, mc_s = f32(schedule.mc_t[:T]), f32(schedule.mc_s[:T])
        tf = self.conditioning_rows(schedule.t_freq)
        tf = None if tf is None else f32(tf)
        with self._lengths_for_call(lengths, seq, x):
            if sample_index is not None:
                return self._ddpm_sample_rows(seq, x, T, mc_t, mc_s, tf, seed, sample_index)
            return self._ddpm_sample_device(seq, x, T, mc_t, mc_s, tf, seed, sample_offset)

    def _ddpm_sample_rows(self, seq, x, T, mc_t, mc_s, tf, seed, sample_index) -> torch.Tensor:
        """esmdiff_ddpm_sample's loop on the host with per-row sample indices: forward i with sinusoid i, update i (the noise
        removal pass at i = T) through esmdiff_ddpm_step_rows."""
        B, L = x.shape
        idx = [int(v) for v in sample_index]
        logits = torch.empty(B, L, self.ld_logits, dtype=torch.float32, device=self.device)
        for i in range(T + 1):
            fin = i == T
            lg = self.forward_logits(x, seq, None if tf is None else tf[i], out=logits, check_ids=False)
            params = self.sample_step_params(idx, 0.0 if fin else float(mc_t[i]), 0.0 if fin else float(mc_s[i]), i, int(fin))
            self.ddpm_step_rows(x, lg, params, seed=seed)
        return x

    def _ddpm_sample_device(self, seq, x, T, mc_t, mc_s, tf, seed, sample_offset) -> torch.Tensor:
        B, L = x.shape
        rng = N.Rng(int(seed), int(sample_offset))
        as_p = lambda t: t.numpy().ctypes.data_as(N.c_f32p)
        self._chk(self._lib.esmdiff_ddpm_sample(self._h, _ptr(seq), _ptr(x), B, L, T, as_p(mc_t), as_p(mc_s),
                                                None if tf is None else as_p(tf),
                                                ctypes.byref(rng), _stream()))
        return x

    def gibbs_step(self, x: torch.Tensor, sequence_tokens: torch.Tensor, logits: torch.Tensor, temperature: float,
                   top_p: float, n_unmask: torch.Tensor, *, u: Optional[torch.Tensor] = None,
                   seed: Optional[int] = None, sample_offset: int = 0, step: int = 0) -> torch.Tensor:
        """One entropy-ordered unmasking step in place (esmdiff_gibbs_step).  n_unmask: (B,) int32."""
        B, L = x.shape
        assert x.dtype == torch.int64 and x.is_cuda and x.is_contiguous()
        assert logits.dtype == torch.float32 and logits.is_cuda and logits.stride(-1) == 1
        ld = logits.stride(1)
        seq = self._tok(sequence_tokens, B, L)
        nu = n_unmask.to(device=self.device, dtype=torch.int32).contiguous()
        rng = None
        if u is not None:
            u = u.to(device=self.device, dtype=torch.float32).contiguous()
            assert u.shape == (B, L, 4096)
        elif seed is None:
            raise ValueError("gibbs_step needs explicit uniforms `u` or a Philox `seed`")
        if seed is not None:
            rng = N.Rng(int(seed), int(sample_offset))
        self._chk(self._lib.esmdiff_gibbs_step(self._h, _ptr(x), _ptr(seq), _ptr(logits), ld, float(temperature),
                                               float(top_p), _ptr(nu), _ptr(u), ctypes.byref(rng) if rng else None,
                                               int(step), B, L, _stream()))
        return x

    @staticmethod
    def gibbs_step_params_host(sample_index, step, n_unmask):
        """Host sequences (one entry per prompt) -> the esmdiff_gibbs_sample_step records as a uint8 numpy array (n, 16)."""
        import numpy as np
        n = len(sample_index)
        rec = np.zeros(n, dtype=N.GIBBS_STEP_DTYPE)
        rec["sample_index"], rec["step"], rec["n_unmask"] = sample_index, step, n_unmask
        return rec.view(np.uint8).reshape(n, -1)

    def gibbs_step_rows(self, x: torch.Tensor, sequence_tokens: torch.Tensor, logits: torch.Tensor, temperature: float,
                        top_p: float, params: torch.Tensor, *, seed: int, pair_bound: Optional[float] = None,
                        entropy_bound: Optional[float] = None, flags: Optional[torch.Tensor] = None,
                        gaps: Optional[torch.Tensor] = None) -> torch.Tensor:
        """gibbs_step (Philox noise) with one parameter set per prompt (esmdiff_gibbs_step_rows): params from
        gibbs_step_params_host, uploaded.  With pair_bound R and entropy_bound E (bounds on the error of a row's logit differences
        and of its entropy, certified.py) flags[b] (int32, zeroed by the caller) gets bit 0 / 1 / 2 where the race / the nucleus
        membership / the entropy order of the rows prompt b unmasks could come out differently for logits within the bounds, and
        gaps[b] (f32 (B, 2), +inf on entry) the smallest race gap (logit units) and the selected-to-unselected entropy distance."""
        B, L = x.shape
        assert x.dtype == torch.int64 and x.is_cuda and x.is_contiguous()
        assert logits.dtype == torch.float32 and logits.is_cuda and logits.stride(-1) == 1
        ld = logits.stride(1)
        assert logits.stride(0) == ld * L
        seq = self._tok(sequence_tokens, B, L)
        assert params.dtype == torch.uint8 and params.is_cuda and params.shape == (B, 16) and params.is_contiguous()
        assert flags is None or (flags.dtype == torch.int32 and flags.is_cuda and flags.numel() == B and flags.is_contiguous())
        assert gaps is None or (gaps.dtype == torch.float32 and gaps.is_cuda and gaps.shape == (B, 2) and gaps.is_contiguous())
        if (flags is not None or gaps is not None) and pair_bound is None:
            raise ValueError("flags / gaps need pair_bound and entropy_bound")
        R = -1.0 if pair_bound is None else float(pair_bound)
        E = 0.0 if entropy_bound is None else float(entropy_bound)
        self._chk(self._lib.esmdiff_gibbs_step_rows(self._h, _ptr(x), _ptr(seq), _ptr(logits), ld, float(temperature), float(top_p),
                                                    _ptr(params), int(seed), B, L, R, E, _ptr(flags), _ptr(gaps), _stream()))
        return x

    def gibbs_sample(self, sequence_tokens: torch.Tensor, x0: torch.Tensor, n_unmask_table: torch.Tensor,
                     temperature: float, top_p: float, *, seed: int, sample_offset: int = 0,
                     lengths: Optional[Sequence[int]] = None, sample_index: Optional[Sequence[int]] = None) -> torch.Tensor:
        """Whole iterative-unmasking loop on the device (esmdiff_gibbs_sample).  n_unmask_table: (T,B) int32.  lengths: a ragged
        batch (set_lengths; x0 holds the structure pad id beyond each length).  sample_index: (B,) Philox sample index per row
        instead of sample_offset + b — a host loop of forward + esmdiff_gibbs_step_rows, per row the ids of a plain call."""
        B, L = sequence_tokens.shape
        seq = self._tok(sequence_tokens, B, L)
        x = x0.to(device=self.device, dtype=torch.int64).contiguous().clone()
        self._check_ids(seq, x)
        tab = n_unmask_table.detach().to("cpu", torch.int32).contiguous()
        T = tab.shape[0]
        assert tab.shape == (T, B)
        if sample_index is not None and len(sample_index) != B:
            raise ValueError(f"sample_index: {len(sample_index)} entries for a batch of {B}")
        with self._lengths_for_call(lengths, seq, x):
            if sample_index is not None:
                idx = [int(v) for v in sample_index]
                logits = torch.empty(B, L, self.ld_logits, dtype=torch.float32, device=self.device)
                for i in range(T):
                    lg = self.forward_logits(x, seq, None, out=logits, check_ids=False)
                    params = torch.from_numpy(self.gibbs_step_params_host(idx, i, tab[i].numpy())).to(self.device)
                    self.gibbs_step_rows(x, seq, lg, temperature, top_p, params, seed=seed)
                return x
            return self._gibbs_sample_device(seq, x, tab, temperature, top_p, seed, sample_offset)

    def _gibbs_sample_device(self, seq, x, tab, temperature, top_p, seed, sample_offset) -> torch.Tensor:
        B, L = x.shape
        T = tab.shape[0]
        rng = N.Rng(int(seed), int(sample_offset))
        self._chk(self._lib.esmdiff_gibbs_sample(self._h, _ptr(seq), _ptr(x), B, L, T, float(temperature), float(top_p),
                                                 tab.numpy().ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                                 ctypes.byref(rng), _stream()))
        return x

    def set_frames(self, rot: Optional[torch.Tensor], trans: Optional[torch.Tensor] = None,
                   has_frame: Optional[torch.Tensor] = None) -> None:
        """Coordinate conditioning for the following forwards (esmdiff_set_frames): rot (B,L,3,3), trans (B,L,3),
        has_frame (B,L) bool — see esmdiff_amd.geometry.build_affine3d_from_coordinates.  None clears them."""
        if rot is None:
            self._chk(self._lib.esmdiff_set_frames(self._h, None, None, None, 0, 0, _stream()))
            self._frames = None
            return
        B, L = rot.shape[:2]
        r = rot.to(device=self.device, dtype=torch.float32).contiguous()
        t = trans.to(device=self.device, dtype=torch.float32).contiguous()
        m = has_frame.to(device=self.device, dtype=torch.uint8).contiguous()
        assert r.shape == (B, L, 3, 3) and t.shape == (B, L, 3) and m.shape == (B, L)
        self._chk(self._lib.esmdiff_set_frames(self._h, _ptr(r), _ptr(t), _ptr(m), B, L, _stream()))
        self._frames = (r, t, m)   # keep the staging tensors alive until the async copies have run

    def gemm(self, A: torch.Tensor, W: torch.Tensor, epilogue: int, *, bias: Optional[torch.Tensor] = None,
             alpha: float = 1.0, out: Optional[torch.Tensor] = None, n_valid: Optional[int] = None) -> torch.Tensor:
        """The GEMM exactly as the forward issues it (esmdiff_gemm_bf16_ws: split-K workspace attached).  `out`: the output
        buffer (its row stride is ldc); required for the f32 epilogues, a fresh bf16 tensor otherwise."""
        M, K = A.shape
        Nn = W.shape[0]
        assert A.dtype == W.dtype == torch.bfloat16 and A.is_contiguous() and W.is_contiguous() and W.shape[1] == K
        if out is None:
            if epilogue in (N.EPI_RESID_F32, N.EPI_BIAS_F32):
                raise ValueError("f32 epilogues need an explicit `out`")
            out = torch.empty(M, Nn // 2 if epilogue == N.EPI_SWIGLU_BF16 else Nn, dtype=torch.bfloat16, device=A.device)
        self._chk(self._lib.esmdiff_gemm_bf16_ws(self._h, _ptr(A), _ptr(W), _ptr(out), _ptr(bias), M, Nn, K, out.stride(0),
                                                 Nn if n_valid is None else n_valid, float(alpha), epilogue, _stream()))
        return out

    @property
    def gemm_workspace_floats(self) -> int:
        """Floats in the split-K workspace `gemm` hands its launch (esmdiff_gemm_workspace_floats); 0 for float32 engines."""
        n = ctypes.c_int64(0)
        self._chk(self._lib.esmdiff_gemm_workspace_floats(self._h, ctypes.byref(n)))
        return int(n.value)

    def set_gibbs_options(self, strategy: str = "entropy", invalid_ids=()) -> None:
        """GenerationConfig.strategy ("entropy" | "random") and .invalid_ids for the following gibbs steps
        (esmdiff_set_gibbs_options); the defaults restore esm's default behaviour."""
        if strategy not in ("entropy", "random"):
            raise ValueError(f"strategy must be 'entropy' or 'random', got {strategy!r}")
        ids = [int(v) for v in invalid_ids]
        arr = (ctypes.c_int32 * max(1, len(ids)))(*ids)
        self._chk(self._lib.esmdiff_set_gibbs_options(self._h, 1 if strategy == "random" else 0, arr if ids else None, len(ids)))

    def set_streams(self, n_streams: int, min_tokens: Optional[int] = None) -> None:
        """Sub-batch launch queues of the 16-bit forward (esmdiff_set_option: 1 .. 4, default 2) and the token count from which a
        batch is cut into sub-batches (default 2200).  No result bit depends on either: the dispatch path of a (B, L) forward is the
        default options' choice, a setting that would move the sub-batches onto the other path is reduced (esmdiff_set_option)."""
        self._chk(self._lib.esmdiff_set_option(self._h, N.OPT_STREAMS, int(n_streams)))
        if min_tokens is not None:
            self._chk(self._lib.esmdiff_set_option(self._h, N.OPT_DUAL_MIN_TOKENS, int(min_tokens)))

    def describe_plan(self, B: int, L: int) -> str:
        """How a (B, L) forward will be dispatched on this engine, as text (esmdiff_describe_plan)."""
        buf = ctypes.create_string_buffer(2048)
        n = self._lib.esmdiff_describe_plan(self._h, int(B), int(L), buf, 2048)
        if n < 0:
            self._chk(n)
        return buf.value.decode()

    def set_step0_sharing(self, on: bool) -> None:
        """Exact step-0 sharing (esmdiff_set_step0_sharing): when every sample of a ddpm_sample / gibbs_sample call starts
        from identical tokens (checked on the device), the first forward runs on a sub-batch and serves all samples; ids are
        bit-identical to the unshared run.  Off by default."""
        self._chk(self._lib.esmdiff_set_step0_sharing(self._h, int(bool(on))))

    def shared_forward_batch(self, B: int, L: int) -> int:
        """Smallest n <= B whose (n, L) forward takes the dispatch path of a (B, L) forward — bit-identical logits per sample
        (esmdiff_shared_forward_batch); B when there is none."""
        n = self._lib.esmdiff_shared_forward_batch(self._h, int(B), int(L))
        if n < 0:
            self._chk(n)
        return int(n)

    def set_small_batch_splitk(self, on: bool) -> None:
        """F32_SPLIT engines: K-sliced residual linears for forwards of <= 4096 rows (esmdiff_set_small_batch_splitk) — faster
        small batches, at the price of the bit-for-bit batch independence across that row count.  Off by default."""
        self._chk(self._lib.esmdiff_set_small_batch_splitk(self._h, int(bool(on))))

    def set_final_skip(self, on: bool) -> None:
        """Exact skip of the noise-removal forward (esmdiff_set_final_skip): after the last update only the samples that still
        hold a MASK run forward T + 1 (none, almost always); ids are bit-identical to the full run.  Off by default."""
        self._chk(self._lib.esmdiff_set_final_skip(self._h, int(bool(on))))

    def set_needed_rows(self, on: bool) -> None:
        """Needed rows (esmdiff_set_option(ESMDIFF_OPT_NEEDED_ROWS)): ddpm_sample's forwards run the last block's branches and
        the head only on the rows that hold MASK, the rows its sampler reads; ids are bit-identical to the full run.  On by default."""
        self._chk(self._lib.esmdiff_set_option(self._h, N.OPT_NEEDED_ROWS, int(bool(on))))

    def forward_logits_needed(self, x: torch.Tensor, sequence_tokens: torch.Tensor, t_freq: Optional[torch.Tensor],
                              out: torch.Tensor) -> torch.Tensor:
        """One forward as ddpm_sample runs it (esmdiff_forward_logits_needed): writes the rows of `out` (B, L, ld) float32 whose
        token in x is MASK and leaves the others as they are."""
        B, L = x.shape
        x, seq = self._tok(x, B, L), self._tok(sequence_tokens, B, L)
        tf = None if t_freq is None else t_freq.to(device=self.device, dtype=torch.float32).contiguous()
        self._chk(self._lib.esmdiff_forward_logits_needed(self._h, _ptr(seq), _ptr(x), _ptr(tf), _ptr(out), out.shape[-1], B, L, _stream()))
        return out

    def tail_rows(self, reset: bool = False) -> int:
        """Token rows that ran the last block's branches and the head since create / the last reset (esmdiff_get_tail_rows):
        counters()["token_rows"] minus the rows a needed-rows forward skipped."""
        r = ctypes.c_int64(0)
        self._chk(self._lib.esmdiff_get_tail_rows(self._h, ctypes.byref(r), int(reset)))
        return int(r.value)

    def counters(self, reset: bool = False) -> Dict[str, int]:
        """Network forwards issued and token rows pushed through them since create / the last reset (executed work)."""
        f, r = ctypes.c_int64(0), ctypes.c_int64(0)
        self._chk(self._lib.esmdiff_get_counters(self._h, ctypes.byref(f), ctypes.byref(r), int(reset)))
        return {"forwards": int(f.value), "token_rows": int(r.value)}

    # ---- per-kernel entry points (parity tests / roofline bench) ---------------------------------
    def set_profiling(self, mode):
        """0/False off; 1/True HIP events around every launch; 2 only around the dominant kernel (FFN-up GEMM)."""
        self._chk(self._lib.esmdiff_set_profiling(self._h, int(mode)))

    def get_profile(self) -> Dict[str, Dict[str, float]]:
        ms = (ctypes.c_float * 16)()
        n = (ctypes.c_int32 * 16)()
        self._chk(self._lib.esmdiff_get_profile(self._h, ms, n))
        out = {s: {"ms": float(ms[i]), "launches": int(n[i])} for i, s in enumerate(N.SECTIONS)}
        # profiling mode 2: union of the FFN-up launches' busy intervals over all streams (slot 15 of the C ABI arrays)
        out["gemm_ffn_up_union"] = {"ms": float(ms[15]), "launches": int(n[15])}
        return out

    def attention(self, qkv: torch.Tensor, q_ln_w: torch.Tensor, k_ln_w: torch.Tensor, B: int, L: int) -> torch.Tensor:
        """q/k LayerNorm + rotary + attention of a qkv GEMM output: esmdiff_attention_bf16 for a bfloat16 qkv,
        esmdiff_attention_f16 (f16 engines) for a float16 one."""
        D = self.cfg.d_model
        assert qkv.dtype in (torch.bfloat16, torch.float16) and qkv.shape == (B * L, 3 * D) and qkv.is_contiguous()
        ctx = torch.empty(B * L, D, dtype=qkv.dtype, device=self.device)
        fn = self._lib.esmdiff_attention_bf16 if qkv.dtype == torch.bfloat16 else self._lib.esmdiff_attention_f16
        self._chk(fn(self._h, _ptr(qkv), _ptr(q_ln_w.float().contiguous()), _ptr(k_ln_w.float().contiguous()), _ptr(ctx),
                     B, L, _stream()))
        return ctx

    def attention_ragged(self, qkv: torch.Tensor, q_ln_w: torch.Tensor, k_ln_w: torch.Tensor, B: int, L: int,
                         lengths: Optional[Sequence[int]] = None) -> torch.Tensor:
        """q/k LayerNorm + rotary + attention in this engine's precision (esmdiff_attention_ragged): qkv [B*L, 3*D] bf16 / f16
        (16-bit engines) or f32 (f32, f32_split) -> ctx [B*L, D] of the same dtype; `lengths` (B,) selects the ragged kernels."""
        D = self.cfg.d_model
        want = {"bf16": torch.bfloat16, "f16": torch.float16}.get(self.precision, torch.float32)
        assert qkv.dtype == want and qkv.shape == (B * L, 3 * D) and qkv.is_contiguous()
        ctx = torch.full((B * L, D), float("nan"), dtype=qkv.dtype, device=self.device)   # NaN: a row the kernel skips shows
        arr = None if lengths is None else (ctypes.c_int32 * B)(*[int(v) for v in lengths])
        self._chk(self._lib.esmdiff_attention_ragged(self._h, _ptr(qkv), _ptr(q_ln_w.float().contiguous()),
                                                     _ptr(k_ln_w.float().contiguous()), _ptr(ctx), arr, B, L, _stream()))
        return ctx

    def qk_norm_rope(self, qkv: torch.Tensor, q_ln_w: torch.Tensor, k_ln_w: torch.Tensor, B: int, L: int, H: int):
        """The q/k LayerNorm + rotary kernel alone in the engine's 16-bit build (esmdiff_qk_norm_rope): qkv [B*L, 3*H*64]
        -> (q, k) [B*L, H*64], q pre-scaled by log2(e)/8."""
        D = H * 64
        assert qkv.dtype == (torch.float16 if self.precision == "f16" else torch.bfloat16)
        assert qkv.shape == (B * L, 3 * D) and qkv.is_contiguous() and q_ln_w.numel() == k_ln_w.numel() == D
        q = torch.empty(B * L, D, dtype=qkv.dtype, device=self.device)
        k = torch.empty_like(q)
        self._chk(self._lib.esmdiff_qk_norm_rope(self._h, _ptr(qkv), _ptr(q_ln_w.float().contiguous()),
                                                 _ptr(k_ln_w.float().contiguous()), _ptr(q), _ptr(k), B, L, H, _stream()))
        return q, k

    def qk_norm_rope_f32(self, qkv: torch.Tensor, q_ln_w: torch.Tensor, k_ln_w: torch.Tensor, B: int, L: int, H: int, *,
                         split: bool = False, q_scale: float = 1.0, k_scale: float = 1.0):
        """The q/k LayerNorm + rotary kernel of the float32-grade engines alone, with this engine's rotary tables
        (esmdiff_qk_norm_rope_f32): qkv f32 [B*L, 3*H*64] -> (q, k) f32 [B*L, H*64] unscaled, or with split [hi | lo] f16
        [B*L, 2*H*64] of the rotated rows * q_scale / k_scale."""
        D = H * 64
        assert qkv.dtype == torch.float32 and qkv.shape == (B * L, 3 * D) and qkv.is_contiguous()
        assert q_ln_w.numel() == k_ln_w.numel() == D
        q = torch.full((B * L, 2 * D if split else D), float("nan"), dtype=torch.float16 if split else torch.float32,
                       device=self.device)
        k = q.clone()
        self._chk(self._lib.esmdiff_qk_norm_rope_f32(self._h, _ptr(qkv), _ptr(q_ln_w.float().contiguous()),
                                                     _ptr(k_ln_w.float().contiguous()), int(split), float(q_scale), float(k_scale),
                                                     _ptr(q), _ptr(k), B, L, H, _stream()))
        return q, k

    def attention_scales(self, layer: int):
        """(att_qk, att_v): the power-of-two operand scales block `layer` of an f32_split engine chose at create."""
        qk, v = ctypes.c_float(0), ctypes.c_float(0)
        self._chk(self._lib.esmdiff_get_attention_scales(self._h, int(layer), ctypes.byref(qk), ctypes.byref(v)))
        return float(qk.value), float(v.value)


class StructureDecoder(_Handle):
    """Structure tokens -> backbone coordinates on the device (esmdiff_decoder_create / esmdiff_decoder_decode): what the
    reference gets from `esm3.decode(ESMProteinTensor(structure=...))`, /root/reference/slm/sample_esmdiff.py:40-61."""
    _destroy = "esmdiff_engine_destroy"

    def __init__(self, cfg, state_dict: Dict[str, torch.Tensor], max_batch: int, max_len: int, device: int = 0,
                 precision: str = "f32"):
        """precision defaults to "f32": the reference decodes in the model's float32 and north_star's bar for this output
        is a backbone within 1e-4 A; decoding is 3e13 FLOP per 100 samples and sits outside the timed sampling metric.
        "bf16" is the r01 / r02 MFMA path (0.05 A mean off the f32 result, ~10x faster)."""
        _require_gpu()
        if precision not in N.PRECISION:
            raise ValueError(f"precision must be one of {sorted(N.PRECISION)}, got {precision!r}")
        self.precision = precision
        self.cfg = cfg
        self.device = torch.device("cuda", device)
        self._lib = N.lib()
        self._h = ctypes.c_void_p(0)
        c = N.Config(cfg.d_model, cfg.n_heads, cfg.n_layers, cfg.ffn_hidden, 23, 1, max_batch, max_len, 1.0, 0,
                     N.PRECISION[precision], 0)
        with torch.cuda.device(self.device):
            keep, table = _weight_table(state_dict, self.device)
            code = self._lib.esmdiff_decoder_create(ctypes.byref(c), table, len(state_dict), device, ctypes.byref(self._h))
        if code != 0:
            raise RuntimeError(f"esmdiff_decoder_create failed ({code}): {self._lib.esmdiff_last_error(None).decode()}")
        del keep
        self.max_batch, self.max_len = max_batch, max_len
        self.has_plddt = any(k == "plddt_head.3.weight" for k in state_dict)
        self.has_ptm = any(k == "pairwise_classification_head.linear2.weight" for k in state_dict)

    def set_pair_chunk_bytes(self, nbytes: int) -> None:
        """esmdiff_decoder_set_pair_chunk_bytes: the pairwise head's pair-row budget per chunk of whole samples (768 B per
        pair row in bf16, 1280 B in f32); 0 restores the default.  For the tests of the chunk loop."""
        N.check(self._lib.esmdiff_decoder_set_pair_chunk_bytes(self._h, int(nbytes)), self._h)

    def decode(self, structure_tokens: torch.Tensor, return_plddt: bool = False, return_ptm: bool = False,
               return_pae: bool = False):
        """structure_tokens (B, L) int64 including BOS / EOS -> backbone coordinates (B, L - 2, 3, 3) float32 (N, CA, C);
        with return_plddt also the per-residue pLDDT (B, L - 2) in [0, 1] (None when the weights carry no plddt_head);
        with return_ptm / return_pae also pTM (B,) and the predicted aligned error (B, L, L, BOS / EOS rows kept, as esm
        returns it) — None when the weights carry no pairwise_classification_head.  Return order: coords[, plddt][, ptm][, pae]."""
        B, L = structure_tokens.shape
        tok = structure_tokens.to(device=self.device, dtype=torch.int64).contiguous()
        if int(tok.min()) < 0 or int(tok.max()) >= STRUCTURE_VOCAB:
            raise ValueError(f"structure token id out of range 0..{STRUCTURE_VOCAB - 1}")
        out = torch.empty(B, L, 3, 3, dtype=torch.float32, device=self.device)
        pl = torch.empty(B, L, dtype=torch.float32, device=self.device) if (return_plddt and self.has_plddt) else None
        want_pair = (return_ptm or return_pae) and self.has_ptm
        ptm = torch.empty(B, dtype=torch.float32, device=self.device) if want_pair else None
        pae = torch.empty(B, L, L, dtype=torch.float32, device=self.device) if (return_pae and self.has_ptm) else None
        N.check(self._lib.esmdiff_decoder_decode(self._h, _ptr(tok), _ptr(out), _ptr(pl), _ptr(ptm), _ptr(pae), B, L,
                                                 float(self.cfg.trans_scale), _stream()), self._h)
        res = [out[:, 1:-1]]
        if return_plddt:
            res.append(None if pl is None else pl[:, 1:-1])
        if return_ptm:
            res.append(ptm)
        if return_pae:
            res.append(pae)
        return res[0] if len(res) == 1 else tuple(res)


class StructureEncoder(_Handle):
    """Backbone coordinates -> structure tokens on the device (esmdiff_encoder_create / esmdiff_encoder_encode): what the
    reference gets from `model.encode(ESMProtein(coordinates=...))`, /root/reference/slm/models/utils.py:136-137."""
    _destroy = "esmdiff_encoder_destroy"

    def __init__(self, cfg, state_dict: Dict[str, torch.Tensor], device: int = 0, precision: str = "f32"):
        """precision defaults to "f32" (csrc/strict.hip): the encoder runs once per input structure on B*L*16 neighbourhood
        rows, and its output is a nearest-code search where bf16 GEMM noise flips 1-2 % of the codes at near-ties."""
        _require_gpu()
        if precision not in N.PRECISION:
            raise ValueError(f"precision must be one of {sorted(N.PRECISION)}, got {precision!r}")
        self.precision = precision
        self.cfg = cfg
        self.device = torch.device("cuda", device)
        self._lib = N.lib()
        self._h = ctypes.c_void_p(0)
        with torch.cuda.device(self.device):
            keep, table = _weight_table(state_dict, self.device)
            code = self._lib.esmdiff_encoder_create(cfg.d_model, cfg.v_heads, cfg.n_layers, cfg.ffn_hidden, cfg.d_out,
                                                    cfg.n_codes, cfg.knn, cfg.relpos_bins, N.PRECISION[precision], table,
                                                    len(state_dict), device,
                                                    ctypes.byref(self._h))
        if code != 0:
            raise RuntimeError(f"esmdiff_encoder_create failed ({code}): {self._lib.esmdiff_encoder_last_error(None).decode()}")
        del keep

    def encode(self, coordinates: torch.Tensor) -> torch.Tensor:
        """coordinates (B, L, >=3, 3) with N, CA, C first (NaN / Inf where unknown) -> structure tokens (B, L) int64 on the
        device; MASK (4096) where a residue has no coordinates.  BOS / EOS are the caller's to add."""
        from .geometry import build_affine3d_from_coordinates
        rot, trans, has = build_affine3d_from_coordinates(coordinates)
        B, L = has.shape
        ca = torch.where(has[..., None], coordinates[..., 1, :].to(torch.float32), torch.zeros(B, L, 3))
        dev = lambda t, dt: t.to(device=self.device, dtype=dt).contiguous()  # noqa: E731
        ca, rot, trans, hm = dev(ca, torch.float32), dev(rot, torch.float32), dev(trans, torch.float32), dev(has, torch.uint8)
        tok = torch.empty(B, L, dtype=torch.int64, device=self.device)
        code = self._lib.esmdiff_encoder_encode(self._h, _ptr(ca), _ptr(rot), _ptr(trans), _ptr(hm), _ptr(tok), B, L, _stream())
        if code != 0:
            raise RuntimeError(f"esmdiff_encoder_encode failed ({code}): {self._lib.esmdiff_encoder_last_error(self._h).decode()}")
        return tok


def _gemm16(dtype: torch.dtype, A, W, epilogue, out, bias, alpha, n_valid) -> torch.Tensor:
    """gemm_bf16 / gemm_f16: one body, the entry and the type of A, W and the 16-bit outputs chosen by `dtype`."""
    _require_gpu()
    M, K = A.shape
    Nn = W.shape[0]
    assert A.dtype == W.dtype == dtype and A.is_contiguous() and W.is_contiguous() and W.shape[1] == K
    if out is None:
        if epilogue in (N.EPI_BF16, N.EPI_BIAS_GELU_BF16):
            out = torch.empty(M, Nn, dtype=dtype, device=A.device)
        elif epilogue == N.EPI_SWIGLU_BF16:
            out = torch.empty(M, Nn // 2, dtype=dtype, device=A.device)
        else:
            raise ValueError("f32 epilogues need an explicit `out`")
    fn = N.lib().esmdiff_gemm_bf16 if dtype == torch.bfloat16 else N.lib().esmdiff_gemm_f16
    N.check(fn(_ptr(A), _ptr(W), _ptr(out), _ptr(bias), M, Nn, K, out.stride(0), Nn if n_valid is None else n_valid,
               float(alpha), epilogue, _stream()))
    return out


def gemm_bf16(A: torch.Tensor, W: torch.Tensor, epilogue: int, *, out: Optional[torch.Tensor] = None,
              bias: Optional[torch.Tensor] = None, alpha: float = 1.0, n_valid: Optional[int] = None) -> torch.Tensor:
    """out = epilogue(A[M,K] @ W[N,K]^T) through esmdiff_gemm_bf16 (N % 128 == 0, K % 64 == 0)."""
    return _gemm16(torch.bfloat16, A, W, epilogue, out, bias, alpha, n_valid)


def gemm_f16(A: torch.Tensor, W: torch.Tensor, epilogue: int, *, out: Optional[torch.Tensor] = None,
             bias: Optional[torch.Tensor] = None, alpha: float = 1.0, n_valid: Optional[int] = None) -> torch.Tensor:
    """gemm_bf16's contract on the f16 build of the kernels (esmdiff_gemm_f16): A, W and 16-bit outputs are torch.float16."""
    return _gemm16(torch.float16, A, W, epilogue, out, bias, alpha, n_valid)


def gemm_f32(A: torch.Tensor, W: torch.Tensor, epilogue: int = 0, *, out: Optional[torch.Tensor] = None,
             bias: Optional[torch.Tensor] = None, div: float = 1.0) -> torch.Tensor:
    """The strict path's linear (esmdiff_gemm_f32): out f32 [M,N] = epi(A f32 [M,K] @ W f32 [N,K]^T); K % 32 == 0.
    epilogue N.F32EPI_RESID_DIV updates `out` in place: out + acc / div."""
    _require_gpu()
    M, K = A.shape
    Nn = W.shape[0]
    assert A.dtype == W.dtype == torch.float32 and A.stride(1) == 1 and W.is_contiguous() and W.shape[1] == K
    if out is None:
        if epilogue == N.F32EPI_RESID_DIV:
            raise ValueError("the residual epilogue updates `out` in place: pass it")
        out = torch.empty(M, Nn, dtype=torch.float32, device=A.device)
    assert out.dtype == torch.float32 and out.stride(1) == 1
    N.check(N.lib().esmdiff_gemm_f32(_ptr(A), A.stride(0), _ptr(W), _ptr(out), _ptr(bias), M, Nn, K, out.stride(0), Nn,
                                     float(div), epilogue, _stream()))
    return out


def split_rows(A: torch.Tensor):
    """f32 [M,K] -> (a3 f16 [M,3K] = [hi | lo | hi] of the row scaled by a power of two, rs f32 [M] = 1 / scale): the
    activation operand of the F32_SPLIT linears (esmdiff_split_rows)."""
    _require_gpu()
    M, K = A.shape
    assert A.dtype == torch.float32 and A.stride(1) == 1
    a2 = torch.empty(M, 3 * K, dtype=torch.float16, device=A.device)
    rs = torch.empty(M, dtype=torch.float32, device=A.device)
    N.check(N.lib().esmdiff_split_rows(_ptr(A), A.stride(0), _ptr(a2), _ptr(rs), M, K, _stream()))
    return a2, rs


def split_weight(W: torch.Tensor):
    """f32 [N,K] -> (w3 f16 [N_pad,3K] = [lo | hi | hi] of W * 2^k, rows padded with zeros to a multiple of 256, 2^-k)."""
    _require_gpu()
    Nn, K = W.shape
    assert W.dtype == torch.float32 and W.is_contiguous()
    n_pad = (Nn + 255) // 256 * 256
    w2 = torch.empty(n_pad, 3 * K, dtype=torch.float16, device=W.device)
    inv = ctypes.c_float(0)
    torch.cuda.synchronize()
    N.check(N.lib().esmdiff_split_weight(_ptr(W), _ptr(w2), Nn, n_pad, K, ctypes.byref(inv)))
    return w2, float(inv.value)


def gemm_split(a2: torch.Tensor, rs: Optional[torch.Tensor], w2: torch.Tensor, w_inv: float, n_out: int,
               epilogue: int = 0, *, out: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
               div: float = 1.0) -> torch.Tensor:
    """out f32 [M, n_out] = epi(A . W^T) from split operands on three f16 MFMA passes (esmdiff_gemm_split).
    epilogue N.F32EPI_SPLIT_SWIGLU: w2 rows interleaved gate / up in blocks of 32, out f32 [M, n_pad / 2] = silu(gate) * up."""
    _require_gpu()
    M, K3 = a2.shape
    n_pad = w2.shape[0]
    width = n_pad // 2 if epilogue == N.F32EPI_SPLIT_SWIGLU else n_pad
    assert a2.dtype == w2.dtype == torch.float16 and w2.shape[1] == K3 and a2.is_contiguous() and w2.is_contiguous()
    if out is None:
        if epilogue == N.F32EPI_RESID_DIV:
            raise ValueError("the residual epilogue updates `out` in place: pass it")
        out = torch.empty(M, width, dtype=torch.float32, device=a2.device)      # the kernel writes whole padded rows
    assert out.dtype == torch.float32 and out.stride(1) == 1 and out.stride(0) >= width
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.numel() >= n_pad
    N.check(N.lib().esmdiff_gemm_split(_ptr(a2), _ptr(rs), _ptr(w2), float(w_inv), _ptr(out), _ptr(bias), M, n_pad, K3 // 3,
                                       out.stride(0), float(div), epilogue, _stream()))
    return out[:, :n_out]


def gemm_split_k(a2: torch.Tensor, rs: Optional[torch.Tensor], w2: torch.Tensor, w_inv: float, x: torch.Tensor, S: int,
                 div: float = 1.0, *, parts: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The K-sliced split GEMM and its reduce (esmdiff_gemm_split_k): x f32 [M, N] += (sum of the S slice products of
    a2 [M, 3K] . w2 [N, 3K]^T * w_inv) * rs / div, in place; returns the slice planes f32 [S, M rounded up to 256, N] (the caller's
    `parts` when given; rows M .. of each plane are unspecified)."""
    _require_gpu()
    M, K3 = a2.shape
    Nn = w2.shape[0]
    assert a2.dtype == w2.dtype == torch.float16 and w2.shape[1] == K3 and a2.is_contiguous() and w2.is_contiguous()
    assert x.dtype == torch.float32 and x.shape == (M, Nn) and x.is_contiguous()
    assert rs is None or (rs.dtype == torch.float32 and rs.numel() == M)
    shape = (max(int(S), 1), (M + 255) // 256 * 256, Nn)
    if parts is None:
        parts = torch.empty(shape, dtype=torch.float32, device=a2.device)
    assert parts.dtype == torch.float32 and tuple(parts.shape) == shape and parts.is_contiguous() and parts.device == a2.device
    N.check(N.lib().esmdiff_gemm_split_k(_ptr(a2), _ptr(rs), _ptr(w2), float(w_inv), _ptr(parts), _ptr(x), M, Nn, K3 // 3, int(S),
                                         float(div), _stream()))
    return parts


def layernorm_f32rows(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], *, split: bool, gelu_in: bool = False,
                      delta: Optional[torch.Tensor] = None, want_y32: bool = True):
    """One LayerNorm kernel of the float32-grade engines (esmdiff_layernorm_f32rows).  split False: layernorm_f32_kernel ->
    y32 f32 [M, D].  split True: layernorm_split_kernel of gelu(x) when gelu_in, of x + delta (bf16 / f16 [M, D]) when given
    -> (a3 f16 [M, 3D] = [hi | lo | hi], rs f32 [M], y32 or None)."""
    _require_gpu()
    M, D = x.shape
    assert x.dtype == w.dtype == torch.float32 and x.is_contiguous() and w.numel() == D
    assert b is None or (b.dtype == torch.float32 and b.numel() == D)
    assert delta is None or (delta.dtype in (torch.bfloat16, torch.float16) and delta.shape == (M, D) and delta.is_contiguous())
    y32 = torch.full((M, D), float("nan"), dtype=torch.float32, device=x.device) if (want_y32 or not split) else None
    a3 = torch.full((M, 3 * D), float("nan"), dtype=torch.float16, device=x.device) if split else None
    rs = torch.full((M,), float("nan"), dtype=torch.float32, device=x.device) if split else None
    N.check(N.lib().esmdiff_layernorm_f32rows(_ptr(x), _ptr(w), _ptr(b), int(split), int(gelu_in), _ptr(delta),
                                              int(delta is not None and delta.dtype == torch.float16), _ptr(a3), _ptr(rs),
                                              _ptr(y32), M, D, _stream()))
    return (a3, rs, y32) if split else y32


def swiglu_f32(gu: torch.Tensor) -> torch.Tensor:
    """gu f32 [M, 2 FH] = [gate | up] -> silu(gate) * up f32 [M, FH] (esmdiff_swiglu_f32: the F32 engine's own pass)."""
    _require_gpu()
    M, FH2 = gu.shape
    assert gu.dtype == torch.float32 and gu.is_contiguous() and FH2 % 2 == 0
    mid = torch.full((M, FH2 // 2), float("nan"), dtype=torch.float32, device=gu.device)
    N.check(N.lib().esmdiff_swiglu_f32(_ptr(gu), _ptr(mid), M, FH2 // 2, _stream()))
    return mid


def v_split(qkv: torch.Tensor, scale: float) -> torch.Tensor:
    """qkv f32 [M, 3D] -> [hi | lo] f16 [M, 2D] of its V third * scale (esmdiff_v_split)."""
    _require_gpu()
    M, D3 = qkv.shape
    assert qkv.dtype == torch.float32 and qkv.is_contiguous() and D3 % 3 == 0
    v2 = torch.full((M, 2 * (D3 // 3)), float("nan"), dtype=torch.float16, device=qkv.device)
    N.check(N.lib().esmdiff_v_split(_ptr(qkv), _ptr(v2), M, D3 // 3, float(scale), _stream()))
    return v2


def attention_f32_parts(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, B: int, L: int, H: int, *,
                        qk_scale_product: float = 1.0, v_scale: float = 1.0,
                        lengths: Optional[Sequence[int]] = None) -> torch.Tensor:
    """One attention kernel of the float32-grade engines (esmdiff_attention_f32_parts) -> ctx f32 [B*L, H*64] (NaN where
    the kernel wrote nothing).  float32 q, k [B*L, H*64] and v = a qkv buffer [B*L, 3*H*64]: attention_f32_kernel; float16
    [hi | lo] rows [B*L, 2*H*64] each: attention_split_kernel with its two scale arguments."""
    _require_gpu()
    D = H * 64
    split = q.dtype == torch.float16
    want = ((B * L, 2 * D),) * 3 if split else ((B * L, D), (B * L, D), (B * L, 3 * D))
    for t, shape in zip((q, k, v), want):
        assert t.dtype == (torch.float16 if split else torch.float32) and t.shape == shape and t.is_contiguous()
    ctx = torch.full((B * L, D), float("nan"), dtype=torch.float32, device=q.device)
    arr = None if lengths is None else (ctypes.c_int32 * B)(*[int(n) for n in lengths])
    N.check(N.lib().esmdiff_attention_f32_parts(_ptr(q), _ptr(k), _ptr(v), int(split), float(qk_scale_product), float(v_scale),
                                                _ptr(ctx), arr, B, L, H, _stream()))
    return ctx


def attention_16_parts(q: torch.Tensor, k: torch.Tensor, qkv: torch.Tensor, B: int, L: int, H: int, *,
                       lengths: Optional[Sequence[int]] = None) -> torch.Tensor:
    """The 16-bit attention kernel alone (esmdiff_attention_16_parts) -> ctx [B*L, H*64] of the operands' type (NaN where the
    kernel wrote nothing).  q, k bfloat16 / float16 [B*L, H*64], q already times log2(e)/8; qkv [B*L, 3*H*64], whose V third is read."""
    _require_gpu()
    D = H * 64
    assert q.dtype in (torch.bfloat16, torch.float16)
    for t, shape in zip((q, k, qkv), ((B * L, D), (B * L, D), (B * L, 3 * D))):
        assert t.dtype == q.dtype and t.shape == shape and t.is_contiguous()
    ctx = torch.full((B * L, D), float("nan"), dtype=q.dtype, device=q.device)
    arr = None if lengths is None else (ctypes.c_int32 * B)(*[int(n) for n in lengths])
    N.check(N.lib().esmdiff_attention_16_parts(int(q.dtype == torch.float16), _ptr(q), _ptr(k), _ptr(qkv), _ptr(ctx), arr, B, L, H,
                                               _stream()))
    return ctx


# ---- weight conversion at create and the input stage, one launcher at a time (include/esmdiff_hip_test.h) ----
_SRC_DT = {torch.float32: N.DT_F32, torch.bfloat16: N.DT_BF16}
_DST_KIND = {torch.bfloat16: 0, torch.float16: 1, torch.float32: 2}


def _weight_src(t: torch.Tensor) -> int:
    assert t.dtype in _SRC_DT and t.is_cuda and t.is_contiguous(), (t.dtype, t.device)
    return _SRC_DT[t.dtype]


def convert_weight(src: torch.Tensor, dst_dtype: torch.dtype, *, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """esmdiff_convert_weight: a float32 / bfloat16 tensor -> bfloat16 (round to nearest even), float16 (saturating) or float32
    (exact), as the create entries convert a state dict.  out: a buffer of dst_dtype with at least src.numel() elements (the
    elements beyond are not written)."""
    _require_gpu()
    n = src.numel()
    if out is None:
        out = torch.empty(src.shape, dtype=dst_dtype, device=src.device)
    assert out.dtype == dst_dtype and out.is_contiguous() and out.numel() >= n
    N.check(N.lib().esmdiff_convert_weight(_ptr(src), _weight_src(src), _ptr(out), _DST_KIND[dst_dtype], n, _stream()))
    return out


def interleave_swiglu(src: torch.Tensor, dst_dtype: torch.dtype) -> torch.Tensor:
    """esmdiff_interleave_swiglu: the FFN-up weight [2H, K] = [gate rows | up rows] (float32 / bfloat16) -> [2H, K] bfloat16 /
    float16 with rows in blocks of 32, [gate 32t..32t+31 | up 32t..32t+31]."""
    _require_gpu()
    H2, K = src.shape
    assert dst_dtype in (torch.bfloat16, torch.float16) and H2 % 2 == 0
    out = torch.empty(H2, K, dtype=dst_dtype, device=src.device)
    N.check(N.lib().esmdiff_interleave_swiglu(_ptr(src), _weight_src(src), _ptr(out), _DST_KIND[dst_dtype], H2 // 2, K, _stream()))
    return out


def split_weight_from(W: torch.Tensor, *, interleave_h: int = 0, n_pad: Optional[int] = None):
    """esmdiff_split_weight_from: split_weight from a float32 or bfloat16 [N, K] weight, rows interleaved as interleave_swiglu
    interleaves them when interleave_h = N / 2 -> (w3 f16 [n_pad, 3K], 2^-k).  The padding rows come back as zeros."""
    _require_gpu()
    Nn, K = W.shape
    n_pad = (Nn + 255) // 256 * 256 if n_pad is None else n_pad
    w3 = torch.full((n_pad, 3 * K), float("nan"), dtype=torch.float16, device=W.device)
    inv = ctypes.c_float(0)
    torch.cuda.synchronize()
    N.check(N.lib().esmdiff_split_weight_from(_ptr(W), _weight_src(W), _ptr(w3), Nn, n_pad, K, int(interleave_h), ctypes.byref(inv)))
    return w3, float(inv.value)


def weight_rownorm_max(W: torch.Tensor, r0: int, rows: int) -> float:
    """esmdiff_weight_rownorm_max: the largest L2 norm among rows r0 .. r0 + rows - 1 of a float32 / bfloat16 [*, K] weight, as
    an F32_SPLIT create measures the q / k / v thirds of a qkv weight."""
    _require_gpu()
    R, K = W.shape
    assert 0 <= r0 and 0 < rows and r0 + rows <= R
    out = ctypes.c_float(0)
    torch.cuda.synchronize()
    N.check(N.lib().esmdiff_weight_rownorm_max(_ptr(W), _weight_src(W), int(r0), int(rows), K, ctypes.byref(out)))
    return float(out.value)


def embed_rows(seq: torch.Tensor, xtok: torch.Tensor, e_seq: torch.Tensor, e_struct: torch.Tensor, cvec: torch.Tensor,
               cond: Optional[torch.Tensor], cond_stride: int) -> torch.Tensor:
    """esmdiff_embed_rows: the input stage alone.  seq, xtok int64 [B, L] (any values: the kernel clamps), e_seq f32 [64, D],
    e_struct f32 [4101, D], cvec f32 [D], cond f32 (one vector with cond_stride 0, [B, cond_stride] otherwise) or None
    -> f32 [B, L, D]."""
    _require_gpu()
    B, L = seq.shape
    D = cvec.numel()
    for t in (seq, xtok):
        assert t.dtype == torch.int64 and t.shape == (B, L) and t.is_contiguous() and t.is_cuda
    assert e_seq.shape == (64, D) and e_struct.shape == (STRUCTURE_VOCAB, D)
    for t in (e_seq, e_struct, cvec) + (() if cond is None else (cond,)):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.is_cuda
    assert cond is None or cond.numel() >= (B - 1) * cond_stride + D
    out = torch.full((B, L, D), float("nan"), dtype=torch.float32, device=seq.device)
    N.check(N.lib().esmdiff_embed_rows(_ptr(seq), _ptr(xtok), _ptr(e_seq), _ptr(e_struct), _ptr(cvec), _ptr(cond), int(cond_stride),
                                       _ptr(out), B, L, D, _stream()))
    return out


def gather_table_rows(tok: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    """esmdiff_gather_table_rows: out f32 [M, D] = table[tok clamped to the table's rows] (the structure decoder's embedding)."""
    _require_gpu()
    n_rows, D = table.shape
    assert tok.dtype == torch.int64 and tok.dim() == 1 and tok.is_contiguous() and tok.is_cuda
    assert table.dtype == torch.float32 and table.is_contiguous() and table.is_cuda
    out = torch.full((tok.numel(), D), float("nan"), dtype=torch.float32, device=tok.device)
    N.check(N.lib().esmdiff_gather_table_rows(_ptr(tok), _ptr(table), _ptr(out), tok.numel(), D, n_rows, _stream()))
    return out


def sigma_mlp(t_freq: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor):
    """esmdiff_sigma_mlp: t_freq f32 [n_sigma, F] -> (hidden = silu(w1 t_freq + b1), cond = w2 hidden + b2), f32 [n_sigma, D]."""
    _require_gpu()
    n_sigma, F = t_freq.shape
    D = w1.shape[0]
    assert w1.shape == (D, F) and w2.shape == (D, D) and b1.shape == (D,) and b2.shape == (D,)
    for t in (t_freq, w1, b1, w2, b2):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.is_cuda
    hidden = torch.full((n_sigma, D), float("nan"), dtype=torch.float32, device=t_freq.device)
    cond = torch.full((n_sigma, D), float("nan"), dtype=torch.float32, device=t_freq.device)
    N.check(N.lib().esmdiff_sigma_mlp(_ptr(t_freq), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(hidden), _ptr(cond), F, D, n_sigma,
                                      _stream()))
    return hidden, cond


def layernorm_16in(x16: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor]) -> torch.Tensor:
    """esmdiff_layernorm_16in: LayerNorm of a bfloat16 / float16 [M, D] input in that type's build (the head's LayerNorm after
    GELU, the pLDDT and pairwise heads' LayerNorms) -> the same type."""
    _require_gpu()
    M, D = x16.shape
    assert x16.dtype in (torch.bfloat16, torch.float16) and x16.is_contiguous() and x16.is_cuda
    assert w.dtype == torch.float32 and w.numel() == D and (b is None or (b.dtype == torch.float32 and b.numel() == D))
    y = torch.full((M, D), float("nan"), dtype=x16.dtype, device=x16.device)
    N.check(N.lib().esmdiff_layernorm_16in(0 if x16.dtype == torch.bfloat16 else 1, _ptr(x16), _ptr(w), _ptr(b), _ptr(y), M, D,
                                           _stream()))
    return y


def gemm_bf16_timed(A, W, out, epilogue, iters=20, bias=None, alpha=1.0) -> float:
    """Average milliseconds per launch, HIP events on the launch stream (esmdiff_gemm_bf16_timed, the one entry point
    that -DED_DEBUG adds to the library; that flag changes nothing else)."""
    _require_gpu()
    if not hasattr(N.lib(), "esmdiff_gemm_bf16_timed"):
        raise RuntimeError("esmdiff_gemm_bf16_timed is a measurement aid of -DED_DEBUG builds: "
                           "ESMDIFF_EXTRA_CXXFLAGS=-DED_DEBUG python -m esmdiff_amd.build --force")
    M, K = A.shape
    ms = ctypes.c_float(0)
    N.check(N.lib().esmdiff_gemm_bf16_timed(_ptr(A), _ptr(W), _ptr(out), _ptr(bias), M, W.shape[0], K,
                                            out.stride(0), W.shape[0], float(alpha), epilogue, iters,
                                            ctypes.byref(ms), _stream()))
    return float(ms.value)


def layernorm_bf16(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor]) -> torch.Tensor:
    _require_gpu()
    M, D = x.shape
    y = torch.empty(M, D, dtype=torch.bfloat16, device=x.device)
    N.check(N.lib().esmdiff_layernorm_bf16(_ptr(x.float().contiguous()), _ptr(w.float().contiguous()),
                                           _ptr(None if b is None else b.float().contiguous()), _ptr(y), M, D,
                                           _stream()))
    return y


def add_layernorm(dtype: torch.dtype, x: torch.Tensor, delta: Optional[torch.Tensor], delta2: Optional[torch.Tensor],
                  write_x: bool, w: torch.Tensor, b: Optional[torch.Tensor]) -> torch.Tensor:
    """The fused residual add + LayerNorm (esmdiff_add_layernorm): v = (x + delta) + delta2 (either may be None), x = v in
    place when write_x; returns LayerNorm(v) * w (+ b).  dtype torch.bfloat16 runs the ed build, torch.float16 the ed16
    build; the deltas and the result are of that type."""
    _require_gpu()
    M, D = x.shape
    assert dtype in (torch.bfloat16, torch.float16) and x.dtype == torch.float32 and x.is_contiguous()
    for t in (delta, delta2):
        assert t is None or (t.dtype == dtype and t.shape == (M, D) and t.is_contiguous())
    y = torch.empty(M, D, dtype=dtype, device=x.device)
    N.check(N.lib().esmdiff_add_layernorm(0 if dtype == torch.bfloat16 else 1, _ptr(x), _ptr(delta), _ptr(delta2),
                                          int(bool(write_x)), _ptr(w.float().contiguous()),
                                          _ptr(None if b is None else b.float().contiguous()), _ptr(y), M, D, _stream()))
    return y


# ---- the needed-rows and sub-batch bookkeeping kernels, one at a time (include/esmdiff_hip_test.h).  Every output is a buffer
# of the caller's, written in place: the tests hand in buffers filled with a sentinel and look at what was left alone. ----
def _dev(t: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    assert t.dtype == dtype and t.is_cuda and t.is_contiguous(), (t.dtype, t.device)
    return t


def mask_row_list(x: torch.Tensor, n_parts: int, rows_list: torch.Tensor, rows_map: torch.Tensor, count: torch.Tensor) -> None:
    """esmdiff_mask_row_list: x i64 [B, L] cut into n_parts -> rows_list / rows_map i32 [>= B L], count i32 [>= n_parts]."""
    _require_gpu()
    B, L = x.shape
    assert rows_list.numel() >= B * L and rows_map.numel() >= B * L and count.numel() >= n_parts
    N.check(N.lib().esmdiff_mask_row_list(_ptr(_dev(x, torch.int64)), B, L, int(n_parts), _ptr(_dev(rows_list, torch.int32)),
                                          _ptr(_dev(rows_map, torch.int32)), _ptr(_dev(count, torch.int32)), _stream()))


def gather_rows16(src: torch.Tensor, rows: torch.Tensor, dst: torch.Tensor) -> None:
    """esmdiff_gather_rows16: dst [i] = src [rows[i]] for the rows.numel() first rows of dst; 2-byte elements of any dtype."""
    _require_gpu()
    n, D = rows.numel(), src.shape[1]
    assert src.element_size() == 2 and dst.dtype == src.dtype and src.is_contiguous() and dst.is_contiguous() and src.is_cuda
    assert dst.shape[1] == D and dst.shape[0] >= n
    N.check(N.lib().esmdiff_gather_rows16(_ptr(src), _ptr(_dev(rows, torch.int32)), _ptr(dst), n, D, _stream()))


def add_layernorm_rows(dtype: torch.dtype, x: torch.Tensor, delta: Optional[torch.Tensor], rows: torch.Tensor,
                       delta2: Optional[torch.Tensor], x_out: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor],
                       y: torch.Tensor) -> None:
    """esmdiff_add_layernorm_rows on M = rows.numel() compact rows: x f32 and delta (dtype) are full-size [*, D], delta2 (dtype)
    is compact [M, D]; x_out f32 and y (dtype) [>= M, D] receive compact rows 0 .. M - 1.  dtype as add_layernorm."""
    _require_gpu()
    M, D = rows.numel(), x.shape[1]
    assert dtype in (torch.bfloat16, torch.float16) and _dev(x, torch.float32).dim() == 2
    assert delta is None or _dev(delta, dtype).shape == x.shape
    assert delta2 is None or _dev(delta2, dtype).shape == (M, D)
    assert _dev(x_out, torch.float32).shape[1] == D and _dev(y, dtype).shape[1] == D and x_out.shape[0] >= M and y.shape[0] >= M
    N.check(N.lib().esmdiff_add_layernorm_rows(0 if dtype == torch.bfloat16 else 1, _ptr(x), _ptr(delta), _ptr(_dev(rows, torch.int32)),
                                               _ptr(delta2), _ptr(x_out), _ptr(_dev(w, torch.float32)),
                                               _ptr(None if b is None else _dev(b, torch.float32)), _ptr(y), M, D, _stream()))


def copy_masked_logits(x: torch.Tensor, logits: torch.Tensor, rows_map: Optional[torch.Tensor], out: torch.Tensor, V: int) -> None:
    """esmdiff_copy_masked_logits: out [row, :V] = logits [rows_map[row] (or row), :V] on the rows of x (i64, flat) that hold
    MASK; logits / out f32 [>= rows, ld] / [>= rows, ld_out]."""
    _require_gpu()
    rows = x.numel()
    assert _dev(logits, torch.float32).dim() == 2 and _dev(out, torch.float32).dim() == 2
    assert logits.shape[0] >= rows and out.shape[0] >= rows
    N.check(N.lib().esmdiff_copy_masked_logits(_ptr(_dev(x, torch.int64)), _ptr(logits), logits.shape[1],
                                               _ptr(None if rows_map is None else _dev(rows_map, torch.int32)), _ptr(out),
                                               out.shape[1], int(V), rows, _stream()))


def ddpm_step_mapped(x: torch.Tensor, logits: torch.Tensor, V: int, mc_t: float, mc_s: float, *, final: bool = False, seed: int = 0,
                     sample_offset: int = 0, step: int = 0, logits_period: int = 0,
                     rows_map: Optional[torch.Tensor] = None) -> torch.Tensor:
    """esmdiff_ddpm_step_mapped: Engine.ddpm_step's in-place update of x i64 [B, L] with Philox noise, each row reading the
    logits row (of logits f32 [*, ld]) that logits_period and rows_map send it to."""
    _require_gpu()
    B, L = x.shape
    assert _dev(logits, torch.float32).dim() == 2
    rng = N.Rng(int(seed), int(sample_offset))
    N.check(N.lib().esmdiff_ddpm_step_mapped(_ptr(_dev(x, torch.int64)), _ptr(logits), logits.shape[1], int(V), float(mc_t),
                                             float(mc_s), int(final), ctypes.byref(rng), int(step), B, L, int(logits_period),
                                             _ptr(None if rows_map is None else _dev(rows_map, torch.int32)), _stream()))
    return x


def move_token_rows(src: torch.Tensor, dst: torch.Tensor, idx: torch.Tensor, n: int, gather: bool) -> None:
    """esmdiff_move_token_rows: n rows of L int64: dst [i] = src [idx[i]] (gather) or dst [idx[i]] = src [i] (scatter)."""
    _require_gpu()
    L = src.shape[1]
    assert _dev(src, torch.int64).dim() == 2 and _dev(dst, torch.int64).shape[1] == L and idx.numel() >= n
    N.check(N.lib().esmdiff_move_token_rows(_ptr(src), _ptr(dst), _ptr(_dev(idx, torch.int32)), int(n), L, int(bool(gather)),
                                            _stream()))


def samples_with_mask(x: torch.Tensor, has: torch.Tensor) -> None:
    """esmdiff_samples_with_mask: has i32 [b] = 1 if row b of x i64 [B, L] holds a MASK, else 0."""
    _require_gpu()
    B, L = x.shape
    assert has.numel() >= B
    N.check(N.lib().esmdiff_samples_with_mask(_ptr(_dev(x, torch.int64)), B, L, _ptr(_dev(has, torch.int32)), _stream()))


def rows_identical(seq: torch.Tensor, x: torch.Tensor, flag: torch.Tensor) -> None:
    """esmdiff_rows_identical: flag i32 [0] = non-zero if every row of seq and of x (i64 [B, L]) equals its row 0, else 0."""
    _require_gpu()
    B, L = x.shape
    assert seq.shape == x.shape
    N.check(N.lib().esmdiff_rows_identical(_ptr(_dev(seq, torch.int64)), _ptr(_dev(x, torch.int64)), B, L,
                                           _ptr(_dev(flag, torch.int32)), _stream()))


MATH_EVAL_UNITS = {"sampler": 0, "score": 1, "gibbs": 2}
MATH_EVAL_KINDS = {"exp": 0, "log": 1, "noise": 2, "philox": 3}


def math_eval(unit: str, kind: str, src: torch.Tensor) -> torch.Tensor:
    """esmdiff_math_eval: csrc/ed_math.h as `unit` ("sampler", "score", "gibbs") compiled it, one element at a time.  kind "exp",
    "log", "noise" (1e-10f - ed_logf(u + 1e-10f)): src f32 [n]; "philox": src u8 [n, 32], the bytes of records of
    _native.MATH_EVAL_PHILOX_DTYPE.  Returns f32 [n]."""
    _require_gpu()
    if kind == "philox":
        assert _dev(src, torch.uint8).dim() == 2 and src.shape[1] == 32
        n = src.shape[0]
    else:
        n = _dev(src, torch.float32).numel()
    out = torch.empty(n, dtype=torch.float32, device=src.device)
    N.check(N.lib().esmdiff_math_eval(MATH_EVAL_UNITS[unit], MATH_EVAL_KINDS[kind], _ptr(src), _ptr(out), n, _stream()))
    return out


GEOM_DTYPES = {torch.bfloat16: 0, torch.float16: 1, torch.float32: 2}


def geom_attention(P: torch.Tensor, rot: torch.Tensor, trans: torch.Tensor, has_frame: torch.Tensor,
                   rotation_scale, distance_scale) -> torch.Tensor:
    """Block 0's geometric attention alone (esmdiff_geom_attention, synchronous): P [B, L, 15*VH] proj output (bfloat16,
    float16 or float32 selects the build), frames rot [B, L, 3, 3], trans [B, L, 3], has_frame [B, L]; the per-head scales
    are the RAW parameters (softplus is applied inside).  Returns [B, L, 3*VH] in P's dtype."""
    _require_gpu()
    B, L, C = P.shape
    VH = C // 15
    assert C == 15 * VH and P.dtype in GEOM_DTYPES and P.is_contiguous()
    assert rot.shape == (B, L, 3, 3) and trans.shape == (B, L, 3) and has_frame.shape == (B, L)
    r = rot.to(device=P.device, dtype=torch.float32).contiguous()
    t = trans.to(device=P.device, dtype=torch.float32).contiguous()
    m = has_frame.to(device=P.device, dtype=torch.uint8).contiguous()
    ws = [torch.as_tensor(v, dtype=torch.float32).cpu().contiguous() for v in (rotation_scale, distance_scale)]
    assert all(v.numel() == VH for v in ws)
    out = torch.empty(B, L, 3 * VH, dtype=P.dtype, device=P.device)
    f32p = ctypes.POINTER(ctypes.c_float)
    N.check(N.lib().esmdiff_geom_attention(_ptr(P), GEOM_DTYPES[P.dtype], _ptr(r), _ptr(t), _ptr(m),
                                           ctypes.cast(ws[0].data_ptr(), f32p), ctypes.cast(ws[1].data_ptr(), f32p),
                                           _ptr(out), B, L, VH, _stream()))
    return out


# ---- the ends of the structure decoder and the encoder's glue kernels, one at a time (include/esmdiff_hip_test.h) ----
def _f32_rows(v: torch.Tensor) -> torch.Tensor:
    assert v.dtype == torch.float32 and v.dim() == 2 and v.stride(1) == 1 and v.is_cuda
    return v


def dim6_to_backbone(v: torch.Tensor, trans_scale: float) -> torch.Tensor:
    """esmdiff_dim6_to_backbone: v f32 [M, ld] (a view with a row stride is fine) -> N, CA, C f32 [M, 3, 3]."""
    _require_gpu()
    M = _f32_rows(v).shape[0]
    out = torch.empty(M, 3, 3, dtype=torch.float32, device=v.device)
    N.check(N.lib().esmdiff_dim6_to_backbone(_ptr(v), v.stride(0), _ptr(out), M, float(trans_scale), _stream()))
    return out


def plddt_mean(v: torch.Tensor, n_bins: int) -> torch.Tensor:
    """esmdiff_plddt_mean: logits f32 [M, ld], the first n_bins columns of each row -> f32 [M]."""
    _require_gpu()
    M = _f32_rows(v).shape[0]
    out = torch.empty(M, dtype=torch.float32, device=v.device)
    N.check(N.lib().esmdiff_plddt_mean(_ptr(v), v.stride(0), int(n_bins), _ptr(out), M, _stream()))
    return out


def pair_features(qk: torch.Tensor) -> torch.Tensor:
    """esmdiff_pair_features: qk [nb, L, 128] bfloat16 or float32 -> [nb, L, L, 128], (b, i, j) = [q_j * k_i | q_j - k_i]."""
    _require_gpu()
    nb, L, C = qk.shape
    assert C == 128 and qk.dtype in (torch.bfloat16, torch.float32) and qk.is_contiguous()
    X = torch.empty(nb, L, L, 128, dtype=qk.dtype, device=qk.device)
    N.check(N.lib().esmdiff_pair_features(_ptr(qk), GEOM_DTYPES[qk.dtype], _ptr(X), nb, L, _stream()))
    return X


def pae_tm(logits: torch.Tensor, tokens: torch.Tensor, max_bin: float = 31.0, want_pae: bool = True):
    """esmdiff_pae_tm: logits f32 [nb, L, L, 64], tokens i64 [nb, L] -> (tm_rows [nb, L], pae [nb, L, L] or None, ptm [nb])."""
    _require_gpu()
    nb, L = tokens.shape
    assert logits.shape == (nb, L, L, 64) and logits.dtype == torch.float32 and logits.is_contiguous()
    assert tokens.dtype == torch.int64 and tokens.is_contiguous()
    tm = torch.empty(nb, L, dtype=torch.float32, device=logits.device)
    pae = torch.empty(nb, L, L, dtype=torch.float32, device=logits.device) if want_pae else None
    ptm = torch.empty(nb, dtype=torch.float32, device=logits.device)
    N.check(N.lib().esmdiff_pae_tm(_ptr(logits), _ptr(tokens), _ptr(tm), _ptr(pae), _ptr(ptm), nb, L, float(max_bin), _stream()))
    return tm, pae, ptm


def _enc_check(code: int) -> None:
    if code != 0:
        raise RuntimeError(f"libesmdiff_hip error {code}: {N.lib().esmdiff_encoder_last_error(None).decode()}")


def encoder_knn(ca: torch.Tensor, has: torch.Tensor, knn: int) -> torch.Tensor:
    """esmdiff_encoder_knn: ca f32 [B, L, 3], has [B, L] -> edges i32 [B, L, min(knn, L)]."""
    _require_gpu()
    B, L, _ = ca.shape
    assert ca.dtype == torch.float32 and ca.is_contiguous() and has.shape == (B, L)
    hm = has.to(device=ca.device, dtype=torch.uint8).contiguous()
    edges = torch.empty(B, L, min(knn, L), dtype=torch.int32, device=ca.device)
    _enc_check(N.lib().esmdiff_encoder_knn(_ptr(ca), _ptr(hm), B, L, int(knn), _ptr(edges), _stream()))
    return edges


def encoder_neighbourhood(edges: torch.Tensor, table: torch.Tensor, rot: torch.Tensor, trans: torch.Tensor,
                          has: torch.Tensor, bins: int):
    """esmdiff_encoder_neighbourhood: edges i32 [B, L, K], table f32 [2 bins + 2, D], rot [B, L, 3, 3], trans [B, L, 3],
    has [B, L] -> (x [B, L, K, D], nrot [B, L, K, 3, 3], ntrans [B, L, K, 3], nmask u8 [B, L, K])."""
    _require_gpu()
    B, L, K = edges.shape
    D = table.shape[1]
    dev = edges.device
    assert edges.dtype == torch.int32 and edges.is_contiguous() and table.shape[0] == 2 * bins + 2
    t = table.to(device=dev, dtype=torch.float32).contiguous()
    r = rot.to(device=dev, dtype=torch.float32).contiguous()
    tr = trans.to(device=dev, dtype=torch.float32).contiguous()
    hm = has.to(device=dev, dtype=torch.uint8).contiguous()
    assert r.shape == (B, L, 3, 3) and tr.shape == (B, L, 3) and hm.shape == (B, L)
    x = torch.empty(B, L, K, D, dtype=torch.float32, device=dev)
    nrot = torch.empty(B, L, K, 3, 3, dtype=torch.float32, device=dev)
    ntrans = torch.empty(B, L, K, 3, dtype=torch.float32, device=dev)
    nmask = torch.empty(B, L, K, dtype=torch.uint8, device=dev)
    _enc_check(N.lib().esmdiff_encoder_neighbourhood(_ptr(edges), _ptr(t), _ptr(r), _ptr(tr), _ptr(hm), B, L, K, D, int(bins),
                                                     _ptr(x), _ptr(nrot), _ptr(ntrans), _ptr(nmask), _stream()))
    return x, nrot, ntrans, nmask


def encoder_nearest_code(z: torch.Tensor, code: torch.Tensor, has: torch.Tensor) -> torch.Tensor:
    """esmdiff_encoder_nearest_code: z f32 [R, d_out], code f32 [n_codes, d_out], has [R] -> tok i64 [R]."""
    _require_gpu()
    R, d_out = z.shape
    assert z.dtype == code.dtype == torch.float32 and z.is_contiguous() and code.is_contiguous() and code.shape[1] == d_out
    hm = has.to(device=z.device, dtype=torch.uint8).contiguous()
    assert hm.shape == (R,)
    tok = torch.empty(R, dtype=torch.int64, device=z.device)
    _enc_check(N.lib().esmdiff_encoder_nearest_code(_ptr(z), _ptr(code), _ptr(hm), R, code.shape[0], d_out, _ptr(tok), _stream()))
    return tok

"""ctypes binding of libesmdiff_hip.so (include/esmdiff_hip.h).  There is NO fallback: if the library is
missing or no gfx950 device is present, every entry point raises."""
from __future__ import annotations

import ctypes
from pathlib import Path

import os

# ESMDIFF_LIB: another build of the same library (ablation / A-B variants made by scratch/build_variant.py); never a fallback
_LIB_PATH = Path(os.environ.get("ESMDIFF_LIB") or Path(__file__).resolve().parent / "lib" / "libesmdiff_hip.so")
_lib = None

c_f32p = ctypes.POINTER(ctypes.c_float)
c_i64p = ctypes.POINTER(ctypes.c_int64)

EPI_BF16, EPI_RESID_F32, EPI_SWIGLU_BF16, EPI_BIAS_GELU_BF16, EPI_BIAS_F32 = range(5)
DT_F32, DT_BF16 = 0, 1
PRECISION = {"bf16": 0, "f32": 1, "f32_split": 2, "f16": 3}       # esmdiff_precision
F32EPI_STORE, F32EPI_BIAS_GELU, F32EPI_RESID_DIV = range(3)
# launcher codes of the split GEMM alone (csrc/gemm256w4_split.hip): 3 is what STORE with a bias runs as (never passed in),
# 4 the fused SwiGLU writing f32 [M, N / 2] (esmdiff_gemm_split accepts it)
F32EPI_SPLIT_STORE_BIAS, F32EPI_SPLIT_SWIGLU = 3, 4
SECTIONS = ["embed", "layernorm", "gemm_qkv", "qk_norm_rope", "attention", "gemm_out", "gemm_ffn_up",
            "gemm_ffn_down", "head", "sampler"]


class Config(ctypes.Structure):
    _fields_ = [("d_model", ctypes.c_int32), ("n_heads", ctypes.c_int32), ("n_layers", ctypes.c_int32),
                ("ffn_hidden", ctypes.c_int32), ("vocab_out", ctypes.c_int32), ("freq_dim", ctypes.c_int32),
                ("max_batch", ctypes.c_int32), ("max_len", ctypes.c_int32), ("residue_scale", ctypes.c_float),
                ("time_conditioning", ctypes.c_int32), ("precision", ctypes.c_int32), ("head_precision", ctypes.c_int32)]


class Weight(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char_p), ("data", ctypes.c_void_p), ("dtype", ctypes.c_int32),
                ("ndim", ctypes.c_int32), ("shape", ctypes.c_int64 * 4)]


# esmdiff_sample_step as a numpy record (one per sample; uploaded as raw bytes)
SAMPLE_STEP_DTYPE = [("sample_index", "<u8"), ("move_chance_t", "<f4"), ("move_chance_s", "<f4"), ("step", "<i4"), ("final", "<i4")]
# esmdiff_math_eval_philox (kind 3 of esmdiff_math_eval)
MATH_EVAL_PHILOX_DTYPE = [("seed", "<u8"), ("sample", "<u8"), ("step", "<u4"), ("l", "<u4"), ("v", "<u4"), ("reserved", "<u4")]
# esmdiff_gibbs_sample_step
GIBBS_STEP_DTYPE = [("sample_index", "<u8"), ("step", "<i4"), ("n_unmask", "<i4")]


class Rng(ctypes.Structure):
    _fields_ = [("seed", ctypes.c_uint64), ("sample_offset", ctypes.c_uint64)]


EXPORTS = [
    "esmdiff_abi_version", "esmdiff_engine_create", "esmdiff_engine_destroy", "esmdiff_last_error",
    "esmdiff_forward_logits", "esmdiff_ddpm_step", "esmdiff_ddpm_sample", "esmdiff_gibbs_step",
    "esmdiff_gibbs_sample", "esmdiff_gemm_bf16", "esmdiff_branch_linear_layernorm",
    "esmdiff_layernorm_bf16", "esmdiff_attention_bf16", "esmdiff_set_profiling",
    "esmdiff_get_profile", "esmdiff_set_frames", "esmdiff_gemm_bf16_ws", "esmdiff_decoder_create",
    "esmdiff_decoder_decode", "esmdiff_metrics_js_pwd", "esmdiff_metrics_js_rg", "esmdiff_metrics_validity",
    "esmdiff_metrics_bonding_validity", "esmdiff_metrics_pwd", "esmdiff_metrics_js_columns", "esmdiff_encoder_create", "esmdiff_encoder_destroy", "esmdiff_encoder_last_error",
    "esmdiff_encoder_encode", "esmdiff_gemm_f32", "esmdiff_set_step0_sharing", "esmdiff_get_counters",
    "esmdiff_set_gibbs_options", "esmdiff_split_rows", "esmdiff_split_weight", "esmdiff_gemm_split",
    "esmdiff_get_embeddings", "esmdiff_set_final_skip", "esmdiff_gemm_f16", "esmdiff_ddpm_step_margin", "esmdiff_forward_logits_sigmas", "esmdiff_set_small_batch_splitk",
    "esmdiff_ddpm_step_rows", "esmdiff_logit_error_stats", "esmdiff_get_build_info", "esmdiff_describe_plan", "esmdiff_set_option",
    "esmdiff_get_sequence_logits", "esmdiff_gibbs_step_rows", "esmdiff_shared_forward_batch",
    "esmdiff_attention_f16", "esmdiff_qk_norm_rope", "esmdiff_add_layernorm", "esmdiff_geom_attention",
    "esmdiff_set_lengths", "esmdiff_attention_ragged", "esmdiff_attention_16_parts",
    "esmdiff_q_xt", "esmdiff_nelbo_rows", "esmdiff_nelbo_eval",
    "esmdiff_superpose_pairs", "esmdiff_tm_pairs",
    "esmdiff_cluster_threshold", "esmdiff_cluster_gromos",
    "esmdiff_lddt_pairs",
    "esmdiff_flex_pair_msf", "esmdiff_flex_fit", "esmdiff_flex_moments", "esmdiff_flex_transforms",
    "esmdiff_aligned_moments", "esmdiff_aligned_project",
    "esmdiff_rmsd_prepare", "esmdiff_rmsd_nearest",
    "esmdiff_dssp",
    "esmdiff_contact_map", "esmdiff_native_contacts",
    "esmdiff_backbone_torsions", "esmdiff_ramachandran",
    "esmdiff_shape_frames", "esmdiff_debye_frames",
    "esmdiff_sasa_frames", "esmdiff_cooccurrence",
    "esmdiff_lagged_means", "esmdiff_lagged_moments", "esmdiff_lagged_project",
    "esmdiff_kmeans_assign", "esmdiff_kmeans_step", "esmdiff_transition_counts",
    "esmdiff_describe_gemm_choice", "esmdiff_gemm_workspace_floats",
    "esmdiff_dim6_to_backbone", "esmdiff_plddt_mean", "esmdiff_pair_features", "esmdiff_pae_tm",
    "esmdiff_decoder_set_pair_chunk_bytes",
    "esmdiff_encoder_knn", "esmdiff_encoder_neighbourhood", "esmdiff_encoder_nearest_code",
    "esmdiff_forward_logits_needed", "esmdiff_get_tail_rows",
    "esmdiff_layernorm_f32rows", "esmdiff_swiglu_f32", "esmdiff_qk_norm_rope_f32", "esmdiff_v_split",
    "esmdiff_attention_f32_parts", "esmdiff_gemm_split_k", "esmdiff_get_attention_scales",
    "esmdiff_convert_weight", "esmdiff_interleave_swiglu", "esmdiff_split_weight_from", "esmdiff_weight_rownorm_max",
    "esmdiff_embed_rows", "esmdiff_gather_table_rows", "esmdiff_sigma_mlp", "esmdiff_layernorm_16in",
    "esmdiff_mask_row_list", "esmdiff_gather_rows16", "esmdiff_add_layernorm_rows", "esmdiff_copy_masked_logits",
    "esmdiff_ddpm_step_mapped", "esmdiff_move_token_rows", "esmdiff_samples_with_mask", "esmdiff_rows_identical",
    "esmdiff_math_eval",
]
LDDT_MAX_L, LDDT_MAX_THRESHOLDS = 4096, 8    # ESMDIFF_LDDT_MAX_L, ESMDIFF_LDDT_MAX_THRESHOLDS
DSSP_MAX_L = 4096                            # ESMDIFF_DSSP_MAX_L
TM_MAX_L = 1280                              # ESMDIFF_TM_MAX_L
CONTACT_MAX_L, CONTACT_TILE, CONTACT_MAX_CHUNKS = 4096, 64, 256    # ESMDIFF_CONTACT_MAX_L, ESMDIFF_CONTACT_TILE, ESMDIFF_CONTACT_MAX_CHUNKS
RAMA_MAX_BINS = 72                           # ESMDIFF_RAMA_MAX_BINS
SHAPE_MAX_L, SHAPE_MAX_BINS = 4096, 4096     # ESMDIFF_SHAPE_MAX_L, ESMDIFF_SHAPE_MAX_BINS
DEBYE_MAX_Q, DEBYE_Q_CHUNK = 1024, 8         # ESMDIFF_DEBYE_MAX_Q, ESMDIFF_DEBYE_Q_CHUNK
SASA_MAX_ATOMS, SASA_MAX_POINTS = 4096, 1024    # ESMDIFF_SASA_MAX_ATOMS, ESMDIFF_SASA_MAX_POINTS
COOCC_MAX_L = 32768                          # ESMDIFF_COOCC_MAX_L
LAGGED_MAX_L, LAGGED_MAX_D, LAGGED_MAX_DIM, LAGGED_FRAME_CHUNK = 128, 8192, 16, 2048    # ESMDIFF_LAGGED_MAX_L, _MAX_D, _MAX_DIM, _FRAME_CHUNK
ALIGNED_MAX_L, ALIGNED_MAX_DIM, ALIGNED_FRAME_CHUNK = 1280, 16, 128    # ESMDIFF_ALIGNED_MAX_L, _MAX_DIM, _FRAME_CHUNK
KMEANS_MAX_K, KMEANS_CENTRE_TILE, KMEANS_FRAME_CHUNK = 4096, 128, 1024   # ESMDIFF_KMEANS_MAX_K, _CENTRE_TILE, _FRAME_CHUNK
TRANSITION_FRAME_CHUNK, TRANSITION_LDS_MAX_K, TRANSITION_SCRATCH_BYTES = 4096, 128, 8    # ESMDIFF_TRANSITION_FRAME_CHUNK, _LDS_MAX_K, _SCRATCH_BYTES
RMSD_NN_TILE, RMSD_NN_RECT, RMSD_NN_MAX_CUTOFFS, RMSD_NN_MAX_BINS = 32, 128, 8, 2048    # ESMDIFF_RMSD_NN_TILE, _RECT, _MAX_CUTOFFS, _MAX_BINS
RMSD_NN_STATE_BYTES, RMSD_NN_SLOT_BYTES = 96, 2 * 128 * 56    # ESMDIFF_RMSD_NN_STATE_BYTES, _SLOT_BYTES

CLUSTER_MAX_N = 16384                       # ESMDIFF_CLUSTER_MAX_N
QXT_PHILOX_COLUMN = 4104                     # ESMDIFF_QXT_PHILOX_COLUMN (the header lists the reserved Philox columns)
OPT_STREAMS, OPT_DUAL_MIN_TOKENS, OPT_NEEDED_ROWS = 1, 2, 3      # esmdiff_option


def flex_pair_slots(n: int) -> int:
    """ESMDIFF_FLEX_PAIR_SLOTS: the partial sums esmdiff_flex_pair_msf keeps per residue (12 bytes each, in the caller's scratch)."""
    rows = (n + 1) // 2
    return 4 * rows * min(16, max(1, 2048 // rows))


def contact_pair_tiles(L: int) -> int:
    """ESMDIFF_CONTACT_PAIR_TILES: the 64 x 64 tiles on and above the diagonal of the L x L maps."""
    tiles = (L + CONTACT_TILE - 1) // CONTACT_TILE
    return tiles * (tiles + 1) // 2


def contact_chunk_frames(n: int, L: int) -> int:
    """ESMDIFF_CONTACT_CHUNK_FRAMES: the consecutive frames esmdiff_contact_map adds in one chunk."""
    cap = min(CONTACT_MAX_CHUNKS, max(1, 1024 // contact_pair_tiles(L)))
    return max(16, (n + cap - 1) // cap)


def contact_chunks(n: int, L: int) -> int:
    """ESMDIFF_CONTACT_CHUNKS: the chunks esmdiff_contact_map cuts n frames into; its sums add them in increasing index."""
    frames = contact_chunk_frames(n, L)
    return (n + frames - 1) // frames


def contact_scratch_bytes(n: int, L: int) -> int:
    """ESMDIFF_CONTACT_SCRATCH_BYTES: the scratch esmdiff_contact_map needs (none with one chunk)."""
    chunks = contact_chunks(n, L)
    return 0 if chunks == 1 else chunks * contact_pair_tiles(L) * CONTACT_TILE * CONTACT_TILE * 24


def rama_chunk_frames(n: int, L: int) -> int:
    """ESMDIFF_RAMA_CHUNK_FRAMES: the consecutive frames esmdiff_ramachandran adds in one chunk."""
    cap = min(1024, max(1, 65536 // L))
    return max(16, (n + cap - 1) // cap)


def rama_chunks(n: int, L: int) -> int:
    """ESMDIFF_RAMA_CHUNKS: the chunks esmdiff_ramachandran cuts n frames into; its sums add them in increasing index."""
    frames = rama_chunk_frames(n, L)
    return (n + frames - 1) // frames


def rama_scratch_bytes(n: int, L: int) -> int:
    """ESMDIFF_RAMA_SCRATCH_BYTES: the scratch esmdiff_ramachandran's sums need (none with one chunk)."""
    chunks = rama_chunks(n, L)
    return 0 if chunks <= 1 else chunks * L * 48


def shape_waves(L: int) -> int:
    """ESMDIFF_SHAPE_WAVES: the waves that share one frame in esmdiff_shape_frames / esmdiff_debye_frames; their sums' order follows it."""
    return 1 if L <= 128 else 8


def coocc_scratch_bytes(n: int, L: int) -> int:
    """ESMDIFF_COOCC_SCRATCH_BYTES: the scratch esmdiff_cooccurrence needs: a word per residue and 64 frames, in two planes."""
    return ((n + 63) // 64) * L * 16


def lagged_features(L: int, k: int) -> int:
    """ESMDIFF_LAGGED_FEATURES: the pairs (i, j >= i + k) of L residues."""
    return (L - k) * (L - k + 1) // 2


def lagged_scratch_bytes(D: int, slots: int, moments: bool) -> int:
    """ESMDIFF_LAGGED_MOMENTS_SCRATCH_BYTES / ESMDIFF_LAGGED_MEANS_SCRATCH_BYTES: the pair table, then `slots` chunk sums."""
    return D * 8 + slots * ((3 * D * D + 2 * D) if moments else 2 * D) * 8


def aligned_scratch_bytes(L: int, slots: int) -> int:
    """ESMDIFF_ALIGNED_MOMENTS_SCRATCH_BYTES: `slots` chunk sums, each S (3L, 3L) then r (3L,)."""
    return slots * (9 * L * L + 3 * L) * 8


def rmsd_nn_padded(n_sel: int) -> int:
    """ESMDIFF_RMSD_NN_PADDED: the row length of a prepared frame's component, the selected count rounded up to a multiple of 4."""
    return (n_sel + 3) // 4 * 4


def rmsd_nn_scratch_bytes(n: int, m: int, slots: int) -> int:
    """ESMDIFF_RMSD_NN_SCRATCH_BYTES: the per-frame state of both sides (m = 0 for an ensemble against itself), then `slots` rectangles' partials."""
    return (n + m) * RMSD_NN_STATE_BYTES + slots * RMSD_NN_SLOT_BYTES


def kmeans_chunks(n: int) -> int:
    """ESMDIFF_KMEANS_CHUNKS: the chunks esmdiff_kmeans_step cuts n frames into; its sums add them in increasing index."""
    return (n + KMEANS_FRAME_CHUNK - 1) // KMEANS_FRAME_CHUNK


def kmeans_slot_bytes(k: int, d: int) -> int:
    """ESMDIFF_KMEANS_SLOT_BYTES: one chunk's sums (k, d), counts (k,) and inertia."""
    return (k * d + k + 1) * 8


def kmeans_step_scratch_bytes(k: int, d: int, slots: int) -> int:
    """ESMDIFF_KMEANS_STEP_SCRATCH_BYTES: `slots` chunk sums."""
    return slots * kmeans_slot_bytes(k, d)


def lib_path() -> Path:
    return _LIB_PATH


def lib():
    """Load the shared library (building is __graft_entry__.build()'s / `python -m esmdiff_amd.build`'s job)."""
    global _lib
    if _lib is not None:
        return _lib
    # torch FIRST: PyTorch-ROCm ships its own libamdhip64 / HSA runtime, and the tensors handed to this library live in that
    # runtime's context.  libesmdiff_hip.so only names "libamdhip64.so.7"; loaded after torch it binds to the copy torch
    # already mapped (one runtime per process), loaded before torch it would pull in /opt/rocm's and the process would hold
    # two runtimes — the second one then reports no devices (seen with `python __graft_entry__.py --smoke`, where build()
    # loaded this library before smoke() imported torch).
    import torch  # noqa: F401
    if not _LIB_PATH.exists():
        raise RuntimeError(
            f"{_LIB_PATH} not found: build it with `python -m esmdiff_amd.build` (needs hipcc). "
            "esmdiff_amd has no CPU fallback.")
    L = ctypes.CDLL(str(_LIB_PATH))
    vp, i32, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float
    L.esmdiff_abi_version.restype = ctypes.c_int
    L.esmdiff_engine_create.argtypes = [ctypes.POINTER(Config), ctypes.POINTER(Weight), i32, i32,
                                        ctypes.POINTER(vp)]
    L.esmdiff_engine_destroy.argtypes = [vp]
    L.esmdiff_engine_destroy.restype = None
    L.esmdiff_last_error.argtypes = [vp]
    L.esmdiff_last_error.restype = ctypes.c_char_p
    L.esmdiff_forward_logits.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, vp]
    L.esmdiff_forward_logits_sigmas.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, vp]
    L.esmdiff_forward_logits_sigmas.restype = ctypes.c_int
    L.esmdiff_forward_logits_needed.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, vp]
    L.esmdiff_get_tail_rows.argtypes = [vp, c_i64p, i32]
    L.esmdiff_ddpm_step.argtypes = [vp, vp, vp, i32, f32, f32, i32, vp, ctypes.POINTER(Rng), i32, i32, i32, vp]
    L.esmdiff_ddpm_step_margin.argtypes = [vp, vp, vp, i32, f32, f32, i32, ctypes.POINTER(Rng), i32, i32, i32, f32, vp, vp]
    L.esmdiff_ddpm_step_margin.restype = ctypes.c_int
    L.esmdiff_ddpm_step_rows.argtypes = [vp, vp, vp, i32, vp, ctypes.c_uint64, i32, i32, f32, f32, vp, vp, vp]
    L.esmdiff_logit_error_stats.argtypes = [vp, i32, vp, i32, vp, i32, i32, i32, vp, vp]
    L.esmdiff_gibbs_step_rows.argtypes = [vp, vp, vp, vp, i32, f32, f32, vp, ctypes.c_uint64, i32, i32, f32, f32, vp, vp, vp]
    L.esmdiff_get_build_info.argtypes = [ctypes.c_char_p, i32]
    L.esmdiff_describe_plan.argtypes = [vp, i32, i32, ctypes.c_char_p, i32]
    L.esmdiff_set_option.argtypes = [vp, i32, ctypes.c_int64]
    L.esmdiff_ddpm_sample.argtypes = [vp, vp, vp, i32, i32, i32, c_f32p, c_f32p, c_f32p, ctypes.POINTER(Rng), vp]
    L.esmdiff_gibbs_step.argtypes = [vp, vp, vp, vp, i32, f32, f32, vp, vp, ctypes.POINTER(Rng), i32, i32, i32, vp]
    L.esmdiff_gibbs_sample.argtypes = [vp, vp, vp, i32, i32, i32, f32, f32, ctypes.POINTER(i32), ctypes.POINTER(Rng), vp]
    L.esmdiff_gemm_bf16.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, f32, i32, vp]
    L.esmdiff_gemm_f16.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, f32, i32, vp]
    if hasattr(L, "esmdiff_gemm_bf16_timed"):      # -DED_DEBUG builds only (scratch/bench_gemm.py)
        L.esmdiff_gemm_bf16_timed.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, f32, i32, i32, c_f32p, vp]
        L.esmdiff_gemm_bf16_timed.restype = ctypes.c_int
    L.esmdiff_branch_linear_layernorm.argtypes = [vp, vp, vp, vp, f32, vp, vp, vp, i32, i32, i32, ctypes.POINTER(i32), vp]
    L.esmdiff_layernorm_bf16.argtypes = [vp, vp, vp, vp, i32, i32, vp]
    L.esmdiff_attention_bf16.argtypes = [vp, vp, vp, vp, vp, i32, i32, vp]
    L.esmdiff_attention_f16.argtypes = [vp, vp, vp, vp, vp, i32, i32, vp]
    L.esmdiff_qk_norm_rope.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, i32, vp]
    L.esmdiff_add_layernorm.argtypes = [i32, vp, vp, vp, i32, vp, vp, vp, i32, i32, vp]
    L.esmdiff_geom_attention.argtypes = [vp, i32, vp, vp, vp, c_f32p, c_f32p, vp, i32, i32, i32, vp]
    L.esmdiff_set_profiling.argtypes = [vp, i32]
    L.esmdiff_get_profile.argtypes = [vp, c_f32p, ctypes.POINTER(i32)]
    L.esmdiff_set_frames.argtypes = [vp, vp, vp, vp, i32, i32, vp]
    L.esmdiff_set_lengths.argtypes = [vp, ctypes.POINTER(i32), i32]
    L.esmdiff_q_xt.argtypes = [vp, vp, vp, vp, vp, vp, ctypes.c_uint64, vp, vp, vp, vp, i32, i32, vp]
    L.esmdiff_nelbo_rows.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp]
    L.esmdiff_nelbo_eval.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, ctypes.c_uint64, vp, vp, vp, i32, vp, vp, vp, i32, i32, vp]
    L.esmdiff_attention_ragged.argtypes = [vp, vp, vp, vp, vp, ctypes.POINTER(i32), i32, i32, vp]
    L.esmdiff_attention_16_parts.argtypes = [i32, vp, vp, vp, vp, ctypes.POINTER(i32), i32, i32, i32, vp]
    L.esmdiff_decoder_create.argtypes = L.esmdiff_engine_create.argtypes
    L.esmdiff_decoder_decode.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, f32, vp]
    f64, f64p = ctypes.c_double, ctypes.POINTER(ctypes.c_double)
    L.esmdiff_metrics_js_pwd.argtypes = [vp, i32, vp, vp, i32, vp, i32, i32, i32, i32, f64p, vp]
    L.esmdiff_metrics_js_rg.argtypes = [vp, i32, vp, vp, i32, vp, i32, i32, i32, f64p, vp]
    L.esmdiff_metrics_pwd.argtypes = [vp, i32, i32, i32, vp, vp]
    L.esmdiff_metrics_js_columns.argtypes = [vp, i32, vp, vp, i32, vp, i32, i32, i32, f64p, vp]
    L.esmdiff_metrics_validity.argtypes = [vp, i32, i32, f64, f64, i32, f64p, vp]
    L.esmdiff_metrics_bonding_validity.argtypes = [vp, i32, vp, i32, i32, f64p, vp]
    L.esmdiff_superpose_pairs.argtypes = [vp, i32, vp, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp]
    L.esmdiff_tm_pairs.argtypes = [vp, i32, vp, i32, i32, vp, vp, vp, vp, vp, vp]
    L.esmdiff_cluster_threshold.argtypes = [vp, i32, i32, i32, f64, i32, vp, vp]
    L.esmdiff_cluster_gromos.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    L.esmdiff_lddt_pairs.argtypes = [vp, i32, vp, i32, i32, vp, vp, f64, f64p, i32, i32, vp, vp, vp, vp, vp]
    L.esmdiff_flex_pair_msf.argtypes = [vp, i32, i32, vp, vp, vp, vp, ctypes.c_int64, vp]
    L.esmdiff_flex_fit.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp]
    L.esmdiff_flex_moments.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp]
    L.esmdiff_flex_transforms.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    L.esmdiff_aligned_moments.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, ctypes.c_int64, vp]
    L.esmdiff_aligned_project.argtypes = [vp, i32, i32, vp, vp, vp, i32, vp, vp]
    L.esmdiff_rmsd_prepare.argtypes = [vp, i32, i32, vp, i32, vp, vp, vp, vp]
    L.esmdiff_rmsd_nearest.argtypes = [vp, vp, vp, i32, vp, vp, vp, i32, i32, i32, vp, i32, i32, f64] + [vp] * 13 + [vp, ctypes.c_int64, vp]
    L.esmdiff_dssp.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    L.esmdiff_contact_map.argtypes = [vp, i32, i32, vp, f64, i32, vp, vp, vp, vp, vp, ctypes.c_int64, vp]
    L.esmdiff_native_contacts.argtypes = [vp, i32, vp, i32, i32, vp, vp, f64, i32, f64, f64, vp, vp, vp, vp, vp, vp]
    L.esmdiff_backbone_torsions.argtypes = [vp, i32, i32, i32, vp, f64, vp, vp, vp, vp, vp]
    L.esmdiff_ramachandran.argtypes = [vp, i32, i32, i32, vp, f64, i32, vp, vp, vp, vp, ctypes.c_int64, vp]
    L.esmdiff_shape_frames.argtypes = [vp, i32, i32, vp, vp, vp, vp, f64, i32, vp]
    L.esmdiff_debye_frames.argtypes = [vp, i32, i32, vp, vp, i32, vp, vp, vp]
    L.esmdiff_sasa_frames.argtypes = [vp, i32, i32, i32, vp, vp, vp, i32, f64, vp, vp, vp, vp, vp, vp, vp]
    L.esmdiff_cooccurrence.argtypes = [vp, i32, i32, vp, vp, ctypes.c_int64, vp]
    L.esmdiff_lagged_means.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp, ctypes.c_int64, vp]
    L.esmdiff_lagged_moments.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, ctypes.c_int64, vp]
    L.esmdiff_lagged_project.argtypes = [vp, i32, i32, i32, vp, vp, i32, vp, vp, ctypes.c_int64, vp]
    L.esmdiff_kmeans_assign.argtypes = [vp, i32, i32, vp, i32, vp, vp, vp]
    L.esmdiff_kmeans_step.argtypes = [vp, i32, i32, vp, i32, vp, vp, vp, vp, vp, ctypes.c_int64, vp]
    L.esmdiff_transition_counts.argtypes = [vp, i32, i32, i32, vp, vp, ctypes.c_int64, vp]
    L.esmdiff_encoder_create.argtypes = [i32] * 9 + [ctypes.POINTER(Weight), i32, i32, ctypes.POINTER(vp)]
    L.esmdiff_encoder_destroy.argtypes = [vp]
    L.esmdiff_encoder_destroy.restype = None
    L.esmdiff_encoder_last_error.argtypes = [vp]
    L.esmdiff_encoder_last_error.restype = ctypes.c_char_p
    L.esmdiff_encoder_encode.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, vp]
    L.esmdiff_set_gibbs_options.argtypes = [vp, i32, ctypes.POINTER(i32), i32]
    L.esmdiff_set_step0_sharing.argtypes = [vp, i32]
    L.esmdiff_shared_forward_batch.argtypes = [vp, i32, i32]
    L.esmdiff_set_final_skip.argtypes = [vp, i32]
    L.esmdiff_set_small_batch_splitk.argtypes = [vp, i32]
    L.esmdiff_get_counters.argtypes = [vp, c_i64p, c_i64p, i32]
    L.esmdiff_gemm_f32.argtypes = [vp, i32, vp, vp, vp, i32, i32, i32, i32, i32, f32, i32, vp]
    L.esmdiff_get_embeddings.argtypes = [vp, vp, i32, i32, vp]
    L.esmdiff_get_sequence_logits.argtypes = [vp, vp, i32, i32, i32, vp]
    L.esmdiff_split_rows.argtypes = [vp, i32, vp, vp, i32, i32, vp]
    L.esmdiff_split_weight.argtypes = [vp, vp, i32, i32, i32, c_f32p]
    L.esmdiff_gemm_split.argtypes = [vp, vp, vp, f32, vp, vp, i32, i32, i32, i32, f32, i32, vp]
    L.esmdiff_gemm_bf16_ws.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, f32, i32, vp]
    L.esmdiff_describe_gemm_choice.argtypes = [i32, i32, i32, ctypes.c_int64] + [ctypes.POINTER(i32)] * 4
    L.esmdiff_gemm_workspace_floats.argtypes = [vp, c_i64p]
    L.esmdiff_dim6_to_backbone.argtypes = [vp, i32, vp, i32, f32, vp]
    L.esmdiff_plddt_mean.argtypes = [vp, i32, i32, vp, i32, vp]
    L.esmdiff_pair_features.argtypes = [vp, i32, vp, i32, i32, vp]
    L.esmdiff_pae_tm.argtypes = [vp, vp, vp, vp, vp, i32, i32, f32, vp]
    L.esmdiff_decoder_set_pair_chunk_bytes.argtypes = [vp, ctypes.c_int64]
    L.esmdiff_encoder_knn.argtypes = [vp, vp, i32, i32, i32, vp, vp]
    L.esmdiff_encoder_neighbourhood.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp]
    L.esmdiff_encoder_nearest_code.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp]
    L.esmdiff_layernorm_f32rows.argtypes = [vp, vp, vp, i32, i32, vp, i32, vp, vp, vp, i32, i32, vp]
    L.esmdiff_swiglu_f32.argtypes = [vp, vp, i32, i32, vp]
    L.esmdiff_qk_norm_rope_f32.argtypes = [vp, vp, vp, vp, i32, f32, f32, vp, vp, i32, i32, i32, vp]
    L.esmdiff_v_split.argtypes = [vp, vp, i32, i32, f32, vp]
    L.esmdiff_attention_f32_parts.argtypes = [vp, vp, vp, i32, f32, f32, vp, ctypes.POINTER(i32), i32, i32, i32, vp]
    L.esmdiff_gemm_split_k.argtypes = [vp, vp, vp, f32, vp, vp, i32, i32, i32, i32, f32, vp]
    L.esmdiff_get_attention_scales.argtypes = [vp, i32, c_f32p, c_f32p]
    L.esmdiff_convert_weight.argtypes = [vp, i32, vp, i32, ctypes.c_int64, vp]
    L.esmdiff_interleave_swiglu.argtypes = [vp, i32, vp, i32, i32, i32, vp]
    L.esmdiff_split_weight_from.argtypes = [vp, i32, vp, i32, i32, i32, i32, c_f32p]
    L.esmdiff_weight_rownorm_max.argtypes = [vp, i32, ctypes.c_int64, i32, i32, c_f32p]
    L.esmdiff_embed_rows.argtypes = [vp, vp, vp, vp, vp, vp, i32, vp, i32, i32, i32, vp]
    L.esmdiff_gather_table_rows.argtypes = [vp, vp, vp, i32, i32, i32, vp]
    L.esmdiff_sigma_mlp.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp]
    L.esmdiff_layernorm_16in.argtypes = [i32, vp, vp, vp, vp, i32, i32, vp]
    L.esmdiff_mask_row_list.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp]
    L.esmdiff_gather_rows16.argtypes = [vp, vp, vp, i32, i32, vp]
    L.esmdiff_add_layernorm_rows.argtypes = [i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp]
    L.esmdiff_copy_masked_logits.argtypes = [vp, vp, i32, vp, vp, i32, i32, i32, vp]
    L.esmdiff_ddpm_step_mapped.argtypes = [vp, vp, i32, i32, f32, f32, i32, ctypes.POINTER(Rng), i32, i32, i32, i32, vp, vp]
    L.esmdiff_move_token_rows.argtypes = [vp, vp, vp, i32, i32, i32, vp]
    L.esmdiff_samples_with_mask.argtypes = [vp, i32, i32, vp, vp]
    L.esmdiff_rows_identical.argtypes = [vp, vp, i32, i32, vp, vp]
    L.esmdiff_math_eval.argtypes = [i32, i32, vp, vp, ctypes.c_int64, vp]
    for n in EXPORTS:
        if n not in ("esmdiff_engine_destroy", "esmdiff_last_error", "esmdiff_encoder_destroy", "esmdiff_encoder_last_error"):
            getattr(L, n).restype = ctypes.c_int
    if L.esmdiff_abi_version() != 8:
        raise RuntimeError("libesmdiff_hip.so ABI version mismatch")
    _lib = L
    return L


def gemm_choice(M: int, N: int, K: int, ws_floats: int = 0) -> dict:
    """esmdiff_describe_gemm_choice: which GEMM launch (M, N, K) gets, from the launcher's own dispatcher; runs no kernel.
    {"w4": the 256x256 kernel, "rows": rows per tile, "S": K slices, "stages": LDS stages}."""
    v = [ctypes.c_int32(0) for _ in range(4)]
    check(lib().esmdiff_describe_gemm_choice(M, N, K, int(ws_floats), *[ctypes.byref(x) for x in v]))
    return {"w4": bool(v[0].value), "rows": int(v[1].value), "S": int(v[2].value), "stages": int(v[3].value)}


def build_info() -> str:
    """esmdiff_get_build_info: ABI, arch, whether this is a -DED_DEBUG build (the kind that exports esmdiff_gemm_bf16_timed)."""
    buf = ctypes.create_string_buffer(1024)
    lib().esmdiff_get_build_info(buf, 1024)
    return buf.value.decode()


def check(code: int, eng=None):
    if code != 0:
        msg = lib().esmdiff_last_error(eng)
        raise RuntimeError(f"libesmdiff_hip error {code}: {msg.decode() if msg else '?'}")

/*
 * esmdiff_hip.h — C ABI of libesmdiff_hip.so, the MI355X (gfx950) engine for the
 * ESMDiff sampling hot path.
 *
 * The reference (lujiarui/esmdiff) has no FFI: its hot path is a chain of Python
 * call sites.  Each entry point below is what a binding for ONE of those call
 * sites would bind; the call site it replaces is cited as file:line relative to
 * the reference tree.  INTEGRATION.md shows the ctypes stubs a maintainer of the
 * reference would add.
 *
 * Conventions
 *   ownership  every pointer passed in/out is DEVICE memory owned by the caller
 *              (e.g. a PyTorch-ROCm tensor's data_ptr()) unless marked [host].
 *              A [host] array, pageable or pinned, is consumed before the entry
 *              returns: the caller may change or free it then.
 *              The engine owns only its bf16 weight copies and its workspace,
 *              both sized at create time for (max_batch, max_len).
 *   errors     every entry returns int: 0 = ok, <0 = esmdiff_status.  Nothing
 *              throws across the boundary.  esmdiff_last_error() gives the text.
 *   threading  one engine per (process, device); not thread-safe.  All work is
 *              enqueued on the caller's hipStream_t (passed as void*); no entry
 *              synchronises the stream except where stated.  The stream may be
 *              any stream, a non-blocking one included: an entry that takes a
 *              stream launches nothing on the null stream, and an engine-owned
 *              side stream is forked from and joined back into the caller's
 *              (tests/test_gpu_stream_order.py).
 *              esmdiff_set_lengths and esmdiff_set_gibbs_options, which take no
 *              stream, wait for the whole device.
 *   dtypes     token ids int64 (the reference's LongTensor), logits float32,
 *              schedule scalars float32 computed by the HOST exactly as
 *              model.py:564-567,584-595 does and passed in.
 */
#ifndef ESMDIFF_HIP_H
#define ESMDIFF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ESMDIFF_ABI_VERSION 8   /* 8: + esmdiff_backbone_torsions, esmdiff_ramachandran (additions, the number stays); + esmdiff_q_xt, esmdiff_nelbo_rows, esmdiff_nelbo_eval (additions only, the number stays); + esmdiff_gibbs_step_rows, esmdiff_set_lengths (an addition); esmdiff_logit_error_stats writes 8 floats per row and takes all_columns; 7: + esmdiff_ddpm_step_rows, esmdiff_logit_error_stats (additions only); 6: + esmdiff_ddpm_step_margin, esmdiff_forward_logits_sigmas, esmdiff_set_small_batch_splitk */

/* structure-track vocabulary: esm constants mirrored at model.py:380-381 */
#define ESMDIFF_VOCAB 4101
#define ESMDIFF_MASK_ID 4096
#define ESMDIFF_STRUCT_EOS 4097
#define ESMDIFF_STRUCT_BOS 4098
#define ESMDIFF_STRUCT_PAD 4099
#define ESMDIFF_STRUCT_CHAINBREAK 4100

typedef enum {
  ESMDIFF_OK = 0,
  ESMDIFF_E_INVALID = -1,   /* bad argument (the reference: assert / ValueError)   */
  ESMDIFF_E_MISSING = -2,   /* weight missing from the table (load_state_dict strict) */
  ESMDIFF_E_SHAPE = -3,     /* weight has the wrong shape / dtype                   */
  ESMDIFF_E_HIP = -4,       /* HIP runtime error                                    */
  ESMDIFF_E_CAPACITY = -5,  /* B > max_batch or L > max_len                         */
  ESMDIFF_E_NODEVICE = -6   /* no gfx950 device                                     */
} esmdiff_status;

typedef enum { ESMDIFF_F32 = 0, ESMDIFF_BF16 = 1 } esmdiff_dtype;

/* Arithmetic of the network (esmdiff_config.precision).
 *   BF16  the throughput path: bf16 weights and GEMM operands on the bf16 MFMA, f32 accumulation, f32 residual stream.
 *   F32   the "strict" path (csrc/strict.hip): float32 weights and activations end to end, every linear on the f32-input
 *         MFMA (one f32 fmaf chain per output element, in a fixed batch-independent K order), correctly rounded divide / sqrt — the arithmetic the reference itself runs in
 *         (checkpoint_utils.py:59-73 loads float32; decode at sample_esmdiff.py:40-61), ~1/12 of the bf16 throughput.
 *         It is what north_star's floating-point bars are stated against (ids equal under a fixed seed, decoded backbone
 *         within 1e-4 A) and the structure decoder's default on the Python side.  A row's result does not depend on the
 *         batch it is computed in.  Coordinate conditioning (esmdiff_set_frames) runs in float32 too.
 *   F32_SPLIT (ABI 5; csrc/gemm_split.hip)  the F32 path with every large linear computed as THREE passes of the f16 MFMA
 *         over operands split into two f16 numbers each (x = hi + lo to 2^-22, rows scaled by powers of two so that nothing
 *         can overflow; f16 x f16 products are exact in f32; the dropped lo.lo term is 2^-22): float32-grade products with
 *         f32 accumulation at ~1/3 of the bf16 MFMA rate instead of 1/16.  Attention runs the same way (attention_split.hip).
 *         LayerNorm, rotary and GELU are the F32 path's arithmetic; the softmax exponentials and the SwiGLU (fused into the
 *         FFN-up epilogue) use the hardware's exp2 / reciprocal (1 ulp each) where F32 calls expf and divides.  Logits agree
 *         with the F32 engine to 7e-6 and the id chains are equal at BASELINE configs[1]'s full size; F32 stays the referee.  A
 *         row's result does not depend on the batch it is computed in.
 *   F16 (ABI 5)  the BF16 path's kernels and launch sequence with IEEE half operands instead of bfloat16 (the same sources
 *         compiled a second time, csrc/ed_half.h): the f16 forms of the same MFMA instructions run at the same rate on the
 *         same bytes, and an 11-bit significand instead of 8 cuts every operand rounding — and with it the logit error and
 *         the rate of near-tie id flips against the float32 chain — by 8.  f16's narrower exponent is not an issue for this
 *         network (weights, LayerNorm / attention / SwiGLU outputs are O(1e-3 .. 1e2)); conversions saturate at +-65504. */
typedef enum { ESMDIFF_PRECISION_BF16 = 0, ESMDIFF_PRECISION_F32 = 1, ESMDIFF_PRECISION_F32_SPLIT = 2, ESMDIFF_PRECISION_F16 = 3 } esmdiff_precision;

/* Hyper-parameters of CustomizedESM3 (net.py:322-332) + TimestepEmbedder (net.py:487) +
 * StructureOutputHeads (net.py:299); values for ESM3-open: 1536 / 24 / 48 / 4096 / 4101 / 256. */
typedef struct {
  int32_t d_model;
  int32_t n_heads;      /* head dim must be 64 */
  int32_t n_layers;
  int32_t ffn_hidden;   /* SwiGLU hidden (gate+up is 2x this) */
  int32_t vocab_out;    /* n_structure_heads: 4101 (ESMDiff) or 4096 (stock ESM3) */
  int32_t freq_dim;     /* TimestepEmbedder.frequency_embedding_size */
  int32_t max_batch;
  int32_t max_len;      /* tokens incl. BOS/EOS */
  float residue_scale;  /* sqrt(n_layers/36) — esm TransformerStack */
  int32_t time_conditioning; /* mdlm.yaml:41 */
  int32_t precision;    /* one of the esmdiff_precision values; new in ABI 4 */
  int32_t head_precision; /* ABI 5.  0: the head runs in `precision`.  1 (with precision = BF16): the final LayerNorm and the
                           * output head (net.py:298-308: Linear, GELU, LayerNorm, Linear) run in float32 grade on the
                           * F32_SPLIT kernels from the f32 residual stream — the logits' own rounding (64 % of the bf16
                           * engine's logit-error variance, profiles/r04_head_decomposition.json) goes away for +1 % time */
} esmdiff_config;

/* One state-dict entry.  `name` uses the reference's key layout for the ESMDiff
 * checkpoint ('module' dict, checkpoint_utils.py:62-64): "net.transformer.blocks.0.attn.…",
 * "sigma_embedder.mlp.0.weight", …  `data` is a DEVICE pointer to a contiguous tensor. */
typedef struct {
  const char* name;
  const void* data;
  int32_t dtype;     /* esmdiff_dtype */
  int32_t ndim;
  int64_t shape[4];
} esmdiff_weight;

/* Counter-based noise source (performance mode).  Uniform for (sample, step, position l,
 * vocabulary id v) = Philox4x32-10(key = seed, counter = {v>>2, l, sample, step})[v&3] >> 8 · 2^-24,
 * so results do not depend on batch composition or on how samples are sharded over GPUs.  In words of 32 bits: key = (seed's low
 * word, seed's high word); counter = (v >> 2, l, sample's low word, step ^ (sample's high word << 16)).  Two draws share a
 * uniform only if they share all of it: distinct for step < 2^16 and sample < 2^48 (csrc/ed_math.h: ed_philox_uniform;
 * restated in tests/shared_math_ref.py). */
typedef struct {
  uint64_t seed;
  uint64_t sample_offset; /* global index of batch row 0 */
} esmdiff_rng;

/* Philox columns reserved beyond the vocabulary (the single list; a new user takes a column that is not on it).  The draws read
 * columns 0 .. 4100 (ddpm) and 0 .. 4095 (gibbs); beyond them:
 *   4104  ESMDIFF_QXT_PHILOX_COLUMN: the mask uniform of position l in the scoring path (esmdiff_q_xt, esmdiff_nelbo_eval), key
 *         (sample, draw, l, 4104) — `draw`, the index of the noise draw of that structure, sits in the counter word the samplers
 *         use for the step;
 *   4105  at l = 0: the HOST's draw of the time of that (sample, draw) pair (esmdiff_amd/nelbo.py);
 *   4352  the per-position uniform of the gibbs "random" strategy (csrc/gibbs.hip).
 * The three differ from each other and from every drawn column, so a score never reuses a uniform that produced the sample it
 * scores. */
#define ESMDIFF_QXT_PHILOX_COLUMN 4104

typedef struct esmdiff_engine esmdiff_engine;

int esmdiff_abi_version(void);

/* What this library is and how an engine will run a batch — for logs (the CLI prints both beside "Sampling token time").
 * No build of the library reads an ESMDIFF_* environment variable (one exception: it refuses to create an engine while
 * ESMDIFF_DEBUG_SKIP, the launch-skipping switch of the retired A/B experiments, is set); debug_env=1 in the build info only
 * means a -DED_DEBUG build, which also exports the timing aid declared in esmdiff_hip_test.h.  Both write a NUL-terminated
 * text into buf [host, cap bytes] and return the length the full text needs (excluding the NUL), or < 0.
 *   esmdiff_get_build_info   "abi=7 arch=gfx950 debug_env=0 ..."
 *   esmdiff_describe_plan    the dispatch plan of a (B, L) forward on this engine: precision, head precision, number of
 *                            sub-batch streams and their sizes, regular / small-batch path, the GEMM kernel of each block
 *                            linear, the exact shortcuts that are on. */
int esmdiff_get_build_info(char* buf, int32_t cap);
int esmdiff_describe_plan(const esmdiff_engine* eng, int32_t B, int32_t L, char* buf, int32_t cap);

/* Explicit dispatch options (ABI 7) — what used to be environment switches and may legitimately be chosen by a caller.  Neither
 * changes a result bit: the dispatch PATH of a (B, L) forward (the small-batch K-slice kernels below 1 152 rows per sub-batch,
 * the regular kernels above: two summation orders) is what the DEFAULT options choose, a function of (B, L) alone; an option
 * only changes how many launch queues run the batch, and a value that would push the sub-batches across that row count is
 * reduced until they stay on the default path's side (r06; esmdiff_describe_plan shows the count in use).  On one path a row's
 * K order depends on (N, K) only.  tests/test_gpu_kernels.py::test_stream_counts_bit_identical (inside one path),
 * tests/test_gpu_fullwidth.py::test_stream_options_never_change_a_bit (settings that would cross the threshold).
 *   ESMDIFF_OPT_STREAMS           sub-batch launch queues of the 16-bit forward: 1 .. 4 (default 2)
 *   ESMDIFF_OPT_DUAL_MIN_TOKENS   batches of at least this many tokens are cut into sub-batches (default 2200)
 *   ESMDIFF_OPT_NEEDED_ROWS       0 / 1 (default 1): esmdiff_ddpm_sample runs the last block's branches and the head only on the rows
 *                                 that hold MASK — the rows whose logits its sampler reads; see esmdiff_ddpm_sample */
typedef enum { ESMDIFF_OPT_STREAMS = 1, ESMDIFF_OPT_DUAL_MIN_TOKENS = 2, ESMDIFF_OPT_NEEDED_ROWS = 3 } esmdiff_option;
int esmdiff_set_option(esmdiff_engine* eng, int32_t option, int64_t value);

/* Replaces load_state_dict_from_lightning_ckpt (checkpoint_utils.py:41-74) + hydra instantiate
 * of mdlm.yaml:26-58: builds bf16 device copies (SwiGLU rows interleaved, head padded) of the
 * weights in `table` [host array of n entries] on `device` and allocates the workspace.
 * Synchronous. */
int esmdiff_engine_create(const esmdiff_config* cfg, const esmdiff_weight* table, int32_t n,
                          int32_t device, esmdiff_engine** out);
void esmdiff_engine_destroy(esmdiff_engine* eng);

/* Text of the last error on `eng`.  With eng == NULL: the calling thread's handle-less string, which every call without a
 * handle writes on failure — a failed create of any kind (engine, decoder, encoder) and the handle-less entries.  It is ONE
 * string: esmdiff_encoder_last_error(NULL) returns the same text. [host] */
const char* esmdiff_last_error(const esmdiff_engine* eng);

/* Replaces self.net(structure_tokens=x, sequence_tokens=seq, auxiliary_embeddings=cond).structure_logits
 * (model.py:475-481 -> net.py:371-483) including conditions = sigma_embedder(sigma) (model.py:466-471,
 * net.py:519-522).  t_freq = TimestepEmbedder.timestep_embedding(sigma, freq_dim) [freq_dim] floats for
 * the single sigma all rows share (model.py:570-571), or NULL for no auxiliary embedding at all (esm's own forward,
 * the gibbs path).  The MLP runs whenever sigma_embedder.* weights were in the table: a model built with
 * time_conditioning = false still adds sigma_embedder(0) in the reference (_process_sigma, model.py:535-541), so its
 * caller passes the sinusoid of sigma = 0.
 * seq, x: [B,L] int64; seq ids outside 0..63 and structure ids outside -1..4100 are clamped (the Python host raises
 * before it gets here).  logits_out: [B,L,ld_logits] float32, ld_logits >= vocab_out. */
int esmdiff_forward_logits(esmdiff_engine* eng, const int64_t* seq, const int64_t* x,
                           const float* t_freq, float* logits_out, int32_t ld_logits,
                           int32_t B, int32_t L, void* stream);

/* The same forward with ONE SIGMA PER SAMPLE, as `_model_wrapper(x, sequence_tokens, sigma)` takes it (model.py:464-481: sigma is
 * a (B,) vector, conditions = sigma_embedder(sigma) is (B, d_model), tiled over each sample's rows): t_freq = the sinusoids
 * [B, freq_dim] (device).  The sampling loops always pass one sigma for the whole batch; this entry is for callers that mix
 * noise levels in one batch (a training-style evaluation of the denoiser, or samples at different updates in one forward). */
int esmdiff_forward_logits_sigmas(esmdiff_engine* eng, const int64_t* seq, const int64_t* x, const float* t_freq,
                                  float* logits_out, int32_t ld_logits, int32_t B, int32_t L, void* stream);

/* F32_SPLIT engines, off by default: forwards of at most 4096 rows run their two residual linears (out-proj, FFN-down: 6 column
 * tiles each, i.e. a few dozen of the 256 CUs at such sizes) as K slices in ONE launch (3 and 4 slices as extra row blocks of the
 * persistent GEMM) plus a pass that sums the slices in order and adds into the residual stream.  Float32 grade as before, but the
 * summation order over K differs from the unsliced kernel's, so with the option ON a sample's last bits depend on whether its
 * batch had more than 4096 rows; OFF (default) the engine stays batch-independent bit for bit.  Used by the certified sampler
 * for its re-runs (small batches by construction). */
int esmdiff_set_small_batch_splitk(esmdiff_engine* eng, int32_t on);

/* ESMOutput.embeddings of the forward that just ran (net.py:468-469, :312-320: the transformer stack's pre-norm hidden
 * state, the second value `self.transformer(...)` returns): out f32 [B,L,d_model].  (B, L) must be the last forward's. */
int esmdiff_get_embeddings(esmdiff_engine* eng, float* out, int32_t B, int32_t L, void* stream);

/* ESMOutput.sequence_logits of the forward that just ran, for networks built with a sequence head (net.py:299-311:
 * StructureOutputHeads(..., n_sequence_heads > 0), a RegressionHead on the same normalised hidden state as the structure head;
 * what _model_wrapper returns next to the structure logits when sequence_prediction is on, model.py:488-490).  The head is
 * created when the weight table holds output_heads.sequence_head.{0,2,3}.{weight,bias} (1 .. 128 outputs) and then runs with
 * every forward; out f32 [B, L, ld_out], ld_out >= n_sequence_heads.  ESMDIFF_E_MISSING without those weights.  (ABI 7) */
int esmdiff_get_sequence_logits(esmdiff_engine* eng, float* out, int32_t ld_out, int32_t B, int32_t L, void* stream);

/* Replaces logits_parameterization + the sampling half of _ddpm_update + _sample_categorical
 * (model.py:527-533, 602-607, 24-28): given RAW network logits, writes x' in place.
 *   final == 0: x' = where(x != MASK, x, argmax_v q_v / (1e-10 - log(u_v + 1e-10)))
 *   final != 0: noise-removal step (model.py:575-579): x' = argmax_v log_p_v
 * Noise: `u` = explicit uniforms [B,L,vocab] row-major (what torch.rand_like draws, model.py:27),
 * or u == NULL and `rng` != NULL for the Philox source at step index `step`. */
int esmdiff_ddpm_step(esmdiff_engine* eng, int64_t* x_inout, const float* logits, int32_t ld_logits,
                      float move_chance_t, float move_chance_s, int32_t final, const float* u,
                      const esmdiff_rng* rng, int32_t step, int32_t B, int32_t L, void* stream);

/* esmdiff_ddpm_step with the Philox source, plus a per-sample report of how close the draw was: sample_flags[b]
 * (device int32 [B], zeroed by the caller) is set to 1 when some masked row of sample b was decided by less than `margin`
 * — update (final == 0): winner <= margin * runner-up of q_v / g_v (margin = exp(2 eps) covers logits known to +-eps:
 * between two tokens the logsumexp cancels and z_a - z_b moves by at most 2 eps; against the mask column z_a moves by
 * eps and the logsumexp by eps); final pass: winner - runner-up <= margin in log-probability (margin = 2 eps).  An unflagged sample's ids are the ids ANY logits within eps of these
 * would have produced.  The ids written are those of esmdiff_ddpm_step, bit for bit.  No reference counterpart: it is
 * what lets a reduced-precision engine hand the few close calls to an f32-grade one (esmdiff_amd/certified.py). */
int esmdiff_ddpm_step_margin(esmdiff_engine* eng, int64_t* x_inout, const float* logits, int32_t ld_logits,
                             float move_chance_t, float move_chance_s, int32_t final, const esmdiff_rng* rng,
                             int32_t step, int32_t B, int32_t L, float margin, int32_t* sample_flags, void* stream);

/* esmdiff_ddpm_step_margin with ONE PARAMETER SET PER SAMPLE (ABI 7).  The reference's loop (model.py:570-573) moves the whole
 * batch through the same update, but nothing couples its samples (model.py:583-607 is row-wise and `_sample_categorical` draws
 * per element), so a batch may hold samples that sit at DIFFERENT updates of their chains: params[b] (DEVICE array of B entries)
 * gives sample b its global Philox sample index (what esmdiff_rng.sample_offset + b is in the plain entry), its move chances,
 * its Philox step index and whether its pass is the noise-removal one.  Per sample the ids written are those esmdiff_ddpm_step
 * would write for that sample alone with the same scalars, bit for bit (tests/test_gpu_kernels.py).  margin_ratio (>= 1) is the
 * bound of the updates, margin_diff (>= 0) of the final passes, as in esmdiff_ddpm_step_margin; sample_flags may be NULL (plain
 * draws).  sample_min_gap (f32 [B], optional, set to +inf by the caller): the smallest winner-over-runner-up gap among the
 * sample's masked rows in log units — log(winner / runner-up) of q_v / g_v for an update, the log-probability difference for a
 * final pass; a sample is flagged exactly when that gap is <= log(margin_ratio) (resp. margin_diff), up to float rounding of the
 * logarithm.  It is a statistic (the re-run share as a function of eps), not an input of the draw.
 * Used by esmdiff_amd/certified.py: verification batches of the f32-grade engine and the fast lane after a roll-back. */
typedef struct {
  uint64_t sample_index;   /* Philox key: the sample's GLOBAL index */
  float move_chance_t;     /* model.py:592-595; ignored when final != 0 */
  float move_chance_s;
  int32_t step;            /* Philox step index = index of the update in the sample's chain */
  int32_t final;           /* != 0: noise-removal pass (model.py:575-579) */
} esmdiff_sample_step;
int esmdiff_ddpm_step_rows(esmdiff_engine* eng, int64_t* x_inout, const float* logits, int32_t ld_logits,
                           const esmdiff_sample_step* params, uint64_t seed, int32_t B, int32_t L, float margin_ratio,
                           float margin_diff, int32_t* sample_flags, float* sample_min_gap, void* stream);

/* How far two engines' logits are apart on the same input (ABI 7, widened in ABI 8; no reference counterpart — the reference
 * has one precision).  a, b: f32 [rows, ld_a / ld_b] raw logits of the same token rows; x: int64 [rows] the tokens that went in.
 * For every row that is MASK (the only rows whose decisions read the logits), over the columns a decision reads — all v < vocab
 * but the MASK column for the ddpm draw (all_columns = 0: model.py:528 pushes that column to -1e6), every v < vocab for the gibbs
 * step (all_columns = 1: nucleus and entropy span the whole row): e_v = a_v - b_v; d_v = e_v - e_(v+1), the error of the logit
 * difference of two NEIGHBOURING tokens (a sample of the pair-error distribution); max e - min e, the bound on the error of the
 * difference of ANY two tokens of the row, which is what decides a draw between them; and the entropy H of softmax over the same
 * columns for both inputs.  out f32 [rows, 8] = { max |e|, sum e^2, max |d|, sum d^2, max e - min e, H(a) - H(b), H(b), 0 };
 * zeros for rows that are not MASK. */
int esmdiff_logit_error_stats(const float* a, int32_t ld_a, const float* b, int32_t ld_b, const int64_t* x, int32_t rows,
                              int32_t vocab, int32_t all_columns, float* out, void* stream);

/* ---- Scoring: the forward-only validation metric, MaskedDiffusionLanguageModeling.model_step(training=False), model.py:386-446.
 *
 * esmdiff_q_xt replaces q_xt (model.py:494-512): xt_out[b,l] = (u < move_chance[b] && !non_moving[b,l]) ? MASK : x0[b,l].
 *   move_chance f32 [B] DEVICE (one per sample: every sample has its own time); non_moving u8 [B,L] or NULL;
 *   u f32 [B,L] explicit uniforms (what torch.rand(*x.shape) draws, :503), or NULL for the Philox source: the uniform of
 *   (seed, sample_index[b], draw[b], l, ESMDIFF_QXT_PHILOX_COLUMN) — sample_index u64 [B], draw i32 [B], DEVICE; a row's mask
 *   depends on its own (sample_index, draw) only, not on its batch position.  seq_out != NULL (needs seq): the coupled sequence
 *   mask of :510-511, seq_out = moved ? SEQUENCE_MASK (32) : seq.  xt_out may be x0 itself, seq_out may be seq.  While lengths
 *   are set (esmdiff_set_lengths) positions l >= lens[b] keep x0.
 *
 * esmdiff_nelbo_rows replaces logits_parameterization + gather + the loss weighting and the masked sum (model.py:527-533,
 *   :432-445) on RAW logits f32 [B,L,ld_logits]: log_p[b,l] = log p(x0[b,l]) of the re-parameterised row — for a MASK row of xt
 *   z[x0] - logsumexp (mask column pushed by -1e6) in the sampler's canonical operation order (bit for bit the C oracle's
 *   value); for any other row 0 where x0 == xt, else -1e6, without reading the logits.  weight f32 [B] DEVICE is the SIGNED
 *   per-sample factor: -(dsigma / expm1(sigma)) (:443), or +log1p(-exp(-sigma_min)) in the change_of_variables /
 *   importance_sampling branch (:439).  sample_sum[b] (f32 [B]) = sum_l log_p * weight[b] * loss_mask[b,l] in a fixed order
 *   (position l is added by lane l % 256 in ascending l, then a halving tree per 64 lanes, then (w0 + w1) + (w2 + w3)),
 *   sample_count[b] (i32 [B]) = sum_l loss_mask[b,l]: both a function of the sample alone.  loss_mask u8 [B,L] of 0 / 1 or NULL
 *   (all ones); log_p_out f32 [B,L] or NULL.  While lengths are set, positions l >= lens[b] are outside the loss mask.
 *   The batch scalar of :445 is sum_b sample_sum / sum_b sample_count, left to the caller.
 *
 * esmdiff_nelbo_eval runs the three steps for one batch on `stream` without a host synchronisation: esmdiff_q_xt into the
 *   engine's own token buffers, esmdiff_forward_logits_sigmas (t_freq [B, freq_dim] DEVICE, one sinusoid per sample; NULL: a
 *   network without conditioning) into the engine's own logits workspace, esmdiff_nelbo_rows.  coupled != 0: the network sees
 *   the coupled sequence mask.  Honours esmdiff_set_lengths and esmdiff_set_frames like the forward.  The outputs equal those of
 *   the three separate calls bit for bit (tests/test_gpu_nelbo.py). */
int esmdiff_q_xt(esmdiff_engine* eng, const int64_t* x0, const int64_t* seq, const float* move_chance, const uint8_t* non_moving,
                 const float* u, uint64_t seed, const uint64_t* sample_index, const int32_t* draw, int64_t* xt_out,
                 int64_t* seq_out, int32_t B, int32_t L, void* stream);
int esmdiff_nelbo_rows(esmdiff_engine* eng, const float* logits, int32_t ld_logits, const int64_t* xt, const int64_t* x0,
                       const float* weight, const uint8_t* loss_mask, float* log_p_out, float* sample_sum, int32_t* sample_count,
                       int32_t B, int32_t L, void* stream);
int esmdiff_nelbo_eval(esmdiff_engine* eng, const int64_t* seq, const int64_t* x0, const float* t_freq, const float* move_chance,
                       const float* weight, const uint8_t* non_moving, const float* u, uint64_t seed, const uint64_t* sample_index,
                       const int32_t* draw, const uint8_t* loss_mask, int32_t coupled, float* sample_sum, int32_t* sample_count,
                       float* log_p_out, int32_t B, int32_t L, void* stream);

/* Replaces MaskedDiffusionLanguageModeling.ddpm_sample (model.py:543-581) for one batch, entirely on
 * the device, Philox noise: T updates + the noise-removal pass.  x_inout holds the prior on entry
 * (all MASK, model.py:555, or input_prior, :561) and the sample on return.
 * mc_t, mc_s: [T] move chances per step [host]; t_freq: [(T+1), freq_dim] [host] (row T = noise removal).
 *
 * Needed rows (ESMDIFF_OPT_NEEDED_ROWS, on by default; exact).  The update reads logits only on rows that hold MASK: any other row
 * keeps its token whatever the network says (model.py:530-532, 606-607).  Everything after the last block's attention is row-wise
 * and feeds only those logits, so on the regular path of a bf16 / f16 engine (no float32-grade head, no extra output head, at
 * least two blocks) each forward of this entry runs the last block's out-projection and FFN, the final LayerNorm and the head on
 * the MASK rows of each sub-batch alone, gathered into compact buffers, when they are at most 7/8 of its rows.  A GEMM row does
 * not depend on how many rows are beside it, so the ids are bit-identical to the full run.  ONE HOST WAIT PER FORWARD: the row
 * count of each sub-batch is written to pinned host memory by a kernel at the start of the forward, and the host waits for
 * that kernel (an event, not the stream) after it has enqueued every block up to the last attention, then enqueues the rest
 * at the exact sizes — by then the device has the whole body of the forward queued behind the kernel waited for.  This is the
 * only entry whose forwards wait on the device; during stream capture, and for every other entry, the forward is the full
 * one and nothing waits.  Afterwards the hidden state and logits of the other rows are stale: esmdiff_get_embeddings and
 * esmdiff_get_sequence_logits refuse until the next full forward. */
int esmdiff_ddpm_sample(esmdiff_engine* eng, const int64_t* seq, int64_t* x_inout, int32_t B, int32_t L,
                        int32_t T, const float* mc_t, const float* mc_s, const float* t_freq,
                        const esmdiff_rng* rng, void* stream);

/* Step-0 sharing (off by default; exact).  The reference's loop (model.py:570-573) runs the network on the whole batch at
 * every step; at step 0 of a run whose samples all start from the same tokens (the CLI repeats ONE sequence and an all-MASK
 * or identical prior, sample_esmdiff.py:196-209) every sample's inputs — and so its logits — are identical.  With the
 * option on, esmdiff_ddpm_sample / esmdiff_gibbs_sample verify ON THE DEVICE that all rows of seq and x_inout are equal,
 * run the first forward on the smallest sub-batch that takes the same dispatch path as the whole batch (bit-identical
 * logits: tests/test_gpu_fullwidth.py::test_logits_across_dispatch_paths) and let every sample draw from those logits with
 * its own noise: the ids are bit-identical to the unshared run (test_step0_sharing_is_exact) and 1 of the T + 1 forwards
 * shrinks to a fraction.  Costs one 4-byte read-back per sampling call.  Not used with coordinate conditioning.
 * esmdiff_get_counters: network forwards issued and token rows pushed through them since create / the last reset — the
 * work actually executed, for FLOP accounting (bench.py reports the shared run as a separate, labelled figure). */
int esmdiff_set_step0_sharing(esmdiff_engine* eng, int32_t on);
/* The sub-batch size step-0 sharing uses (ABI 8): the smallest number of samples n <= B whose (n, L) forward takes the same
 * dispatch path — and so produces the same logits bit for bit — as a (B, L) forward; B when there is none.  Returns n >= 1, or a
 * negative esmdiff_status.  Callers that drive the loop themselves (esmdiff_amd/certified.py) share their first forward with it. */
int esmdiff_shared_forward_batch(const esmdiff_engine* eng, int32_t B, int32_t L);
/* Exact skip of the noise-removal forward (off by default; exact).  The last of the T + 1 forwards of esmdiff_ddpm_sample only
 * serves `x = argmax(log p)` (model.py:575-579), and for a position that is no longer MASK the re-parameterised log p is 0 at its
 * own token and -1e6 elsewhere (model.py:530-532): a sample without a MASK comes back unchanged.  With the option on, the
 * engine counts on the device which samples still hold a MASK after update T (one B x 4-byte read-back), skips the forward
 * when none does, and otherwise runs it on those samples only — as a sub-batch on the same dispatch path as the whole batch
 * (padded with complete samples when smaller), so the ids are bit-identical to the full run
 * (tests/test_gpu_fullwidth.py::test_final_skip_is_exact).  P(a masked row stays masked at the last update) = mc_s / mc_t. */
int esmdiff_set_final_skip(esmdiff_engine* eng, int32_t on);
int esmdiff_get_counters(esmdiff_engine* eng, int64_t* forwards, int64_t* token_rows, int32_t reset);

/* Replaces, for ONE step, the per-prompt half of esm.utils.generation.iterative_sampling_raw as the reference calls
 * it in "gibbs" mode (sample_esmdiff.py:114-122; [ESM-RECALL]): for every still-masked position
 * entropy of softmax(logits over the 4096 codebook ids), nucleus filter (top_p), temperature, categorical draw; then
 * per prompt the n_unmask[b] lowest-entropy masked positions (never BOS/EOS/PAD of `seq`) take their token.
 * n_unmask: [B] int32 DEVICE; u: explicit uniforms [B,L,4096] or NULL with rng; temperature >= 0 (0: the arg-max
 * of the filtered logits, no noise drawn — esm's sample_logits [ESM-RECALL]). */
int esmdiff_gibbs_step(esmdiff_engine* eng, int64_t* x_inout, const int64_t* seq, const float* logits,
                       int32_t ld_logits, float temperature, float top_p, const int32_t* n_unmask, const float* u,
                       const esmdiff_rng* rng, int32_t step, int32_t B, int32_t L, void* stream);

/* GenerationConfig fields the reference leaves at their defaults (sample_esmdiff.py:116-119 sets only track / num_steps /
 * temperature / top_p) [ESM-RECALL]: strategy 0 = "entropy" (the k lowest-entropy masked positions are unmasked), 1 =
 * "random" (a uniformly random k-subset of the masked positions: the k smallest of one Philox uniform per position; needs the
 * rng noise source); invalid_ids [host, n_invalid]: codebook ids that are never drawn — masked after the nucleus cut exactly
 * like the special ids >= 4096.  Applies to every following esmdiff_gibbs_step / esmdiff_gibbs_sample of this engine;
 * (0, NULL, 0) restores the defaults.  Takes no stream: it waits for the whole device (hipDeviceSynchronize), so that no gibbs step still
 * queued on any stream reads the new mask, then uploads 512 bytes with a blocking copy that is complete on return. */
int esmdiff_set_gibbs_options(esmdiff_engine* eng, int32_t strategy, const int32_t* invalid_ids, int32_t n_invalid);

/* esmdiff_gibbs_step (Philox source) with ONE PARAMETER SET PER PROMPT (ABI 8), and optionally a report of how close the step's
 * decisions were.  iterative_sampling_raw moves a batch through the same step index, but nothing couples its prompts (every
 * decision above is per row or per prompt), so a batch may hold prompts that sit at DIFFERENT steps of their chains: params[b]
 * (DEVICE array of B entries) gives prompt b its global Philox sample index (what esmdiff_rng.sample_offset + b is in the plain
 * entry), its Philox step index and the number of positions it unmasks.  Per prompt the ids written are those esmdiff_gibbs_step
 * writes for that prompt alone with the same scalars, bit for bit (tests/test_gpu_kernels.py).
 * pair_bound < 0: plain draws (sample_flags / sample_gaps must be NULL).  pair_bound = R >= 0, entropy_bound = E >= 0: the logits
 * are taken to be known only up to an error whose difference between any two columns of a row is at most R (so every probability
 * up to the factor exp(+-R)) and which moves a row's entropy by at most E.  sample_flags[b] (int32 [B], zeroed by the caller) then
 * gets, over the rows prompt b UNMASKS in this step: bit 0 — a draw's winner does not lead the best other possibly-kept token by
 * more than exp(R / temperature) (temperature 0: R); bit 1 — the winner's membership of the nucleus, or a better token's, depends
 * on the error (kept for sure: mass{z_j >= z_v - R} exp(R) <= top_p S; dropped for sure: mass{z_j >= z_v + R} exp(-R) > top_p S),
 * or the fall-back was taken; bit 2 — the largest selected and the smallest unselected entropy are not more than 2 E apart
 * (strategy "entropy" only).  An unflagged prompt's new ids are those ANY logits within the bounds would have produced.
 * sample_gaps (f32 [B, 2], optional, +inf on entry): the smallest race gap of the unmasked rows in logit units, and the entropy
 * distance above — statistics, not inputs of the step.  Used by esmdiff_amd/certified.py (CertifiedSampler.gibbs_sample). */
typedef struct {
  uint64_t sample_index;   /* Philox key: the prompt's GLOBAL index */
  int32_t step;            /* Philox step index = index of the step in the prompt's chain */
  int32_t n_unmask;        /* positions to unmask in this step (<= 0: the prompt is left alone) */
} esmdiff_gibbs_sample_step;
int esmdiff_gibbs_step_rows(esmdiff_engine* eng, int64_t* x_inout, const int64_t* seq, const float* logits, int32_t ld_logits,
                            float temperature, float top_p, const esmdiff_gibbs_sample_step* params, uint64_t seed, int32_t B,
                            int32_t L, float pair_bound, float entropy_bound, int32_t* sample_flags, float* sample_gaps,
                            void* stream);

/* The whole loop of iterative_sampling_raw for one batch on the device (Philox noise, no time conditioning):
 * T x (forward, gibbs step).  n_unmask_table: [T,B] int32 [host] = positions to unmask per step and prompt
 * (cosine schedule, computed by the host: esmdiff_amd/gibbs.py). */
int esmdiff_gibbs_sample(esmdiff_engine* eng, const int64_t* seq, int64_t* x_inout, int32_t B, int32_t L, int32_t T,
                         float temperature, float top_p, const int32_t* n_unmask_table, const esmdiff_rng* rng,
                         void* stream);

/* Coordinate conditioning (block 0's geometric attention).  Replaces what the reference does inside
 * CustomizedESM3.forward when structure_coords is given (/root/reference/slm/models/net.py:433-441, :468):
 * the caller passes the per-residue backbone frames that esm's build_affine3d_from_coordinates derives from the
 * N/CA/C coordinates (esmdiff_amd/geometry.py computes them on the host), and every following forward of this engine
 * with the same (B, L) adds the geometric-attention branch of block 0.  rot: f32 [B,L,3,3] row-major rotation matrices,
 * trans: f32 [B,L,3], has_frame: u8 [B,L] (0 = no coordinates for that residue) — device pointers, copied on `stream`.
 * rot == NULL clears the frames (the branch is then exactly zero, as in the reference with all-NaN coordinates, and is
 * skipped).  Needs the transformer.blocks.0.geom_attn.* weights in the table given to esmdiff_engine_create
 * (ESMDIFF_E_MISSING otherwise). */
int esmdiff_set_frames(esmdiff_engine* eng, const float* rot, const float* trans, const uint8_t* has_frame,
                       int32_t B, int32_t L, void* stream);

/* Ragged batch for the following calls: B samples padded to one L, sample b valid on tokens [0, lens[b]) (lens counts BOS and
 * EOS; each in 3..max_len).  Padding sits at the end of a row and holds the pad ids (sequence 1, structure 4099 = never MASK).
 * A valid position's logits and ids then depend only on its own sample's valid positions: attention masks the padded keys and
 * writes zeros for padded query rows, every other kernel is row-wise.  lens is a HOST array, copied to a device buffer of
 * max_batch entries after a wait for the whole device (hipDeviceSynchronize: the entry takes no stream, and no forward still queued
 * on any stream may read the new lengths), with a blocking copy that is complete on return; NULL clears it and waits for nothing.  Stateful like esmdiff_set_frames: while set, esmdiff_forward_logits[_sigmas],
 * esmdiff_ddpm_sample, esmdiff_gibbs_sample and the *_step_rows entries refuse (ESMDIFF_E_INVALID) a call whose B differs
 * from the set B or whose L is below a length, step-0 sharing is off, and esmdiff_describe_plan(B) reports
 * "ragged=1 valid_tokens=...".  The GEMMs still run the padded rows. */
int esmdiff_set_lengths(esmdiff_engine* eng, const int32_t* lens, int32_t B);

/* VQ-VAE structure-token decoder: structure tokens -> backbone coordinates.  Replaces `esm3.decode(...)` as the
 * reference's decode() helper calls it once per sample (/root/reference/slm/sample_esmdiff.py:40-61, :225-230; the
 * reference also moves the whole ESM3 model between CPU and GPU around it, :58, :176).  The decoder is esm's
 * StructureTokenDecoder [ESM-RECALL, SURVEY.md 8f-1]: nn.Embedding(4101, d) -> the same pre-LN block stack as ESM3
 * (no geometric attention, residue scaling 1) -> Dim6RotStructureHead.  cfg: d_model 1280, n_heads 20, n_layers 30,
 * ffn_hidden 3584 for esm3_structure_decoder_v0; vocab_out / freq_dim / time_conditioning are ignored, residue_scale
 * should be 1.  Weight names: embed.weight, decoder_stack.blocks.{i}.<as ESM3>, decoder_stack.norm.weight,
 * affine_output_projection.{ffn1,norm,proj}.{weight,bias}.  Destroy with esmdiff_engine_destroy.
 * Optional: plddt_head.{0,2,3}.{weight,bias} (esm's RegressionHead(d, 50) on the same hidden state) enables `plddt`.
 * esmdiff_decoder_decode: tokens int64 [B,L] INCLUDING BOS (4098) / EOS (4097); bb_coords f32 [B,L,3,3] = N, CA, C
 * per position (rows 0 and L-1 belong to BOS/EOS and are to be dropped); plddt f32 [B,L] or NULL = mean of the
 * categorical mixture over the 50 bins of [0,1] (what ESMProtein.to_pdb writes into the B-factor column,
 * sample_esmdiff.py:56-61); trans_scale = 10 in esm.
 * Optional: pairwise_classification_head.{downproject,linear1,linear2}.weight + .norm.{weight,bias} (esm's
 * PairwisePredictionHead(d, 128, 128, 64 + 96 + 64 bins, bias=False)) enables `ptm` f32 [B] and `pae` f32 [B,L,L]
 * (NULL to skip; pae needs ptm): decoder_output["ptm"] / ["predicted_aligned_error"] of the reference's decode path
 * (/root/reference/slm/models/utils.py:64-76) — softmax over the 64 predicted-aligned-error bins (max bin 31 A) of every
 * token pair, PAE = expected bin centre, pTM = max_i mean_j E[1 / (1 + (e / d0)^2)] over non-special tokens; pairs with
 * BOS/EOS/special tokens carry the uniform-distribution value in `pae`, as esm leaves them.  Only the PAE slice of
 * linear2 is evaluated (the distogram / direction slices are training targets).
 * esmdiff_decoder_decode is enqueued on `stream` like a forward; its one wait: a call with ptm that finds the pairwise head's
 * workspace too small (the first, or one with more pair rows than any before) synchronises `stream` before it frees and regrows it. */
int esmdiff_decoder_create(const esmdiff_config* cfg, const esmdiff_weight* table, int32_t n_weights,
                           int32_t device, esmdiff_engine** out);
int esmdiff_decoder_decode(esmdiff_engine* dec, const int64_t* tokens, float* bb_coords, float* plddt, float* ptm,
                           float* pae, int32_t B, int32_t L, float trans_scale, void* stream);

/* VQ-VAE structure-token ENCODER: backbone frames -> structure tokens.  Replaces `model.encode(ESMProtein(coordinates))`
 * as protseq_to_data calls it for the DDPM inpainting prior (/root/reference/slm/models/utils.py:136-137,
 * /root/reference/slm/sample_esmdiff.py:196-201).  esm's StructureTokenEncoder [ESM-RECALL, SURVEY.md 8f-4]: 16 nearest
 * residues per residue -> relative-position embedding -> 2 x (geometric attention + SwiGLU FFN, with biases) per
 * neighbourhood -> Linear(d, 128) -> nearest of 4096 codebook vectors.  esm3_structure_encoder_v0: d_model 1024, v_heads
 * 128, n_layers 2, ffn_hidden 4096, d_out 128, n_codes 4096, knn 16, relpos_bins 32.  Weight names:
 * relative_positional_embedding.embedding.weight, transformer.blocks.{i}.geom_attn.{s_norm.weight, proj.{weight,bias},
 * out_proj.{weight,bias}, rotation_scale_per_head, distance_scale_per_head}, transformer.blocks.{i}.ffn.{0,1,3}.{weight,
 * bias}, pre_vq_proj.{weight,bias}, codebook.embeddings.
 * precision (ABI 4): ESMDIFF_PRECISION_F32 runs the two blocks and the projection in float32 (csrc/strict.hip) — the codes then
 * equal a float32 encoder's except at exact distance ties; BF16 is the MFMA path (98-99 % identical codes, every difference a
 * near-tie).
 * encode: ca f32 [B,L,3] (CA positions), rot f32 [B,L,3,3], trans f32 [B,L,3], has_frame u8 [B,L] (the frames of
 * esmdiff_set_frames; residues WITHOUT BOS/EOS) -> tokens int64 [B,L] (device), 4096 (MASK) where has_frame == 0.
 * Synchronises `stream` before returning. */
typedef struct esmdiff_encoder esmdiff_encoder;
int esmdiff_encoder_create(int32_t d_model, int32_t v_heads, int32_t n_layers, int32_t ffn_hidden, int32_t d_out,
                           int32_t n_codes, int32_t knn, int32_t relpos_bins, int32_t precision /* esmdiff_precision */,
                           const esmdiff_weight* table, int32_t n_weights, int32_t device, esmdiff_encoder** out);
void esmdiff_encoder_destroy(esmdiff_encoder* enc);
/* Text of the last error on `enc`; with enc == NULL the handle-less string that esmdiff_last_error(NULL) returns too. */
const char* esmdiff_encoder_last_error(const esmdiff_encoder* enc);
int esmdiff_encoder_encode(esmdiff_encoder* enc, const float* ca, const float* rot, const float* trans,
                           const uint8_t* has_frame, int64_t* tokens, int32_t B, int32_t L, void* stream);

/* Ensemble metrics on CA traces (float64, device pointers in, one double out on the host; each call synchronises
 * `stream`).  They replace the numpy / scipy functions of /root/reference/slm/utils/eval_utils.py that score a generated
 * ensemble against a reference ensemble: js_pwd :227-255 (Jensen-Shannon distance of the per-pair CA distance
 * histograms, bins spanning the reference's range, pseudo count 1e-6, mean over pairs), js_rg :290-316, validity
 * :158-173 (fraction of frames without a CA-CA distance below 2*radius - overlap among pairs |i-j| > k_exclusion),
 * bonding_validity :176-188 (fraction of frames whose adjacent CA distances all stay below the reference's maximum
 * + 1e-6).  ca_*: f64 [n, L, 3].  Values are returned unrounded (the reference rounds to 4 decimals last).
 * w_model / w_ref: per-frame histogram weights f64 [n] or NULL (the reference's `weights=` dictionaries, default ones);
 * kl != 0: mean of scipy.special.kl_div over all bins and columns instead of the mean JS distance (`kl=True`).
 * esmdiff_metrics_pwd: the pairwise-distance features alone, out f64 [n, D], D = pairs (i, j >= i + offset) in
 * numpy.triu_indices order (eval_utils.py:90-102) — what js_tica (:258-289) feeds its TICA fit; esmdiff_metrics_js_columns:
 * the histogram + JS / KL tail on any feature matrix [n, D] (js_tica: D = 2 projected coordinates). */
int esmdiff_metrics_js_pwd(const double* ca_model, int32_t n_model, const double* w_model, const double* ca_ref,
                           int32_t n_ref, const double* w_ref, int32_t L, int32_t n_bins, int32_t pwd_offset, int32_t kl,
                           double* js_out, void* stream);
int esmdiff_metrics_js_rg(const double* ca_model, int32_t n_model, const double* w_model, const double* ca_ref,
                          int32_t n_ref, const double* w_ref, int32_t L, int32_t n_bins, int32_t kl, double* js_out,
                          void* stream);
int esmdiff_metrics_pwd(const double* ca, int32_t n, int32_t L, int32_t pwd_offset, double* out, void* stream);
int esmdiff_metrics_js_columns(const double* x_model, int32_t n_model, const double* w_model, const double* x_ref,
                               int32_t n_ref, const double* w_ref, int32_t D, int32_t n_bins, int32_t kl, double* out,
                               void* stream);
int esmdiff_metrics_validity(const double* ca, int32_t n, int32_t L, double ca_vdw_radius, double allowable_overlap,
                             int32_t k_exclusion, double* out, void* stream);
int esmdiff_metrics_bonding_validity(const double* ca_model, int32_t n_model, const double* ca_ref, int32_t n_ref,
                                     int32_t L, double* out, void* stream);

/* Superposition of ensembles (float64, device pointers in and out; each call synchronises `stream`): what the reference's
 * evaluations compute pair by pair on the host — /root/reference/slm/utils/geo_utils.py:58-122 (squared_deviation through
 * _find_rigid_alignment), analysis/apo_analysis.py:182-288 (scipy's align_vectors on sample pairs) and slm/utils/tm_utils.py
 * (one `TMscore -seq` subprocess per pair).  (An addition; the ABI number stays.)
 * A f64 [n, L, 3] is superposed onto B f64 [m, L, 3], residue i onto residue i; B == NULL: A against itself (m is ignored,
 * maskB = maskA).  maskA u8 [n, L] / maskB u8 [m, L] or NULL (all valid): a pair's aligned set is the AND of both; masked
 * coordinates are never read into a sum (they may be NaN).
 *
 * esmdiff_superpose_pairs: the least-squares (Kabsch) superposition of every pair.  allow_reflection = 1: R = V U^T of the SVD
 * of the covariance with no determinant correction, as geo_utils._find_rigid_alignment (a mirror image aligns with RMSD 0);
 * allow_reflection = 0: the proper rotation (det R = +1: scipy's Rotation.align_vectors, the RMSD `TMscore` prints).  Outputs,
 * each may be NULL: rmsd f64 [n, m] (sqrt of the mean squared deviation over the aligned set); sd f64 [n, m, L] per-residue
 * squared deviation after alignment, NaN where masked; R f64 [n, m, 3, 3] and t f64 [n, m, 3] with R a + t ~ b.  A pair with
 * fewer than 2 aligned residues gives NaN everywhere.  Rank-deficient covariances (2 residues, collinear, planar) give the
 * right RMSD and an orthogonal R.  Any L >= 1 (the structures are read from global memory).
 *
 * esmdiff_tm_pairs: tm f64 [n, m] = the TM-score of model A[i] against native B[j] with the fixed residue-to-residue
 * correspondence (`TMscore -seq` on identical sequences), normalised by the number Ln of valid residues of B[j],
 * d0 = max(0.5, 1.24 cbrt(Ln - 15) - 1.8); the maximisation over superpositions is the TMscore program's fragment-seeded
 * heuristic search as DESIGN.md ("Superposition") states it — [TMSCORE-RECALL], restated from memory, PARITY UNPINNED: the
 * program itself is in no tree this project can reach.  R / t (optional, shapes as above): the best superposition found.
 * L > ESMDIFF_TM_MAX_L (both structures of a pair are staged in LDS) returns ESMDIFF_E_CAPACITY: there is no slow path.
 * Both entries are deterministic (fixed reduction order, no float atomics) and a pair's value does not depend on the launch. */
#define ESMDIFF_TM_MAX_L 1280
int esmdiff_superpose_pairs(const double* A, int32_t n, const double* B, int32_t m, int32_t L, const uint8_t* maskA,
                            const uint8_t* maskB, int32_t allow_reflection, double* rmsd, double* sd, double* R, double* t,
                            void* stream);
int esmdiff_tm_pairs(const double* A, int32_t n, const double* B, int32_t m, int32_t L, const uint8_t* maskA,
                     const uint8_t* maskB, double* tm, double* R, double* t, void* stream);

/* Clustering of an ensemble (device pointers in and out; each call synchronises `stream`): the GROMOS algorithm (Daura et al.
 * 1999, the `gromos` method of `gmx cluster`) on a neighbour relation, as DESIGN.md ("Clustering") states it.  (An addition; the
 * ABI number stays.)  The reference clusters nothing itself: analysis/bpti_analysis.py reads the five kinetic clusters of BPTI
 * from files.
 * The relation is a bit matrix adj u64 [n, W], W = ceil(n / 64): bit (j % 64) of adj[i, j / 64] = "i and j are neighbours";
 * the padding bits of a row's last word are zero.  n > ESMDIFF_CLUSTER_MAX_N (the loop keeps one int32 count per structure
 * in LDS) returns ESMDIFF_E_CAPACITY, n < 1 ESMDIFF_E_INVALID, before anything is launched.
 *
 * esmdiff_cluster_threshold: d f64 [rows, n] holds rows row0 .. row0 + rows - 1 of an n x n matrix (a caller may feed the matrix
 * block by block and never hold all of it).  For every row i of the block and every j > i the bit (i, j) is set iff
 * d[i, j] <= cutoff (larger_is_closer = 1, similarities: d[i, j] >= cutoff); a NaN entry sets nothing; the bit (i, i) is always
 * set; entries with j < i are never read, and no bit below the diagonal is written.  Bits are OR-ed into adj: the caller zeroes
 * adj once before the first block.
 *
 * esmdiff_cluster_gromos: first makes adj symmetric IN PLACE from its bits on and above the diagonal (bit (j, i) = bit (i, j)
 * for i < j; whatever stood below the diagonal or in the padding on entry is ignored and overwritten; the diagonal is set), then
 * runs the loop in one launch of one persistent workgroup: among the structures not yet assigned, the one with the most
 * unassigned neighbours (itself included; ties: the lowest index) is the centre of the next cluster, the cluster is the centre
 * and all its unassigned neighbours; repeat until none is left.  labels i32 [n]: the cluster of each structure, clusters
 * numbered in order of creation; centres i32 [n] and sizes i32 [n]: the first n_clusters[0] entries are valid (sizes are
 * non-increasing); n_clusters i32 [1].  Integers only: the result is a pure function of adj's upper triangle. */
#define ESMDIFF_CLUSTER_MAX_N 16384
int esmdiff_cluster_threshold(const double* d, int32_t rows, int32_t row0, int32_t n, double cutoff, int32_t larger_is_closer,
                              uint64_t* adj, void* stream);
int esmdiff_cluster_gromos(uint64_t* adj, int32_t n, int32_t* labels, int32_t* centres, int32_t* sizes, int32_t* n_clusters,
                           void* stream);

/* All-pairs CA-lDDT (Mariani et al. 2013) of models against natives: superposition-free, local, and INTEGER — the counts of
 * preserved distances, held exactly to the numpy restatement tests/lddt_ref.py.  (An addition; the ABI number stays.)  DESIGN.md
 * §3.20 states the definition.  A f64 [n, L, 3] models, B f64 [m, L, 3] natives, residue to residue, device pointers; B == NULL:
 * A against itself (m is ignored, maskB = maskA).  maskA u8 [n, L] / maskB u8 [m, L] on the device, or NULL (all valid); a masked
 * coordinate is never read.  `thresholds` is a HOST array of n_thresholds (1 .. ESMDIFF_LDDT_MAX_THRESHOLDS) doubles; r0 the
 * inclusion radius; seq_sep >= 1.
 *   pair set of native j (ordered pairs):  (a, b) with |a - b| >= seq_sep, maskB[j, a] and maskB[j, b], and
 *                                          dn = |B[j, a] - B[j, b]| < r0 (strict)
 *   total_res i32 [m, L] (or NULL)        the number of b with (a, b) in the set;   total i32 [m] = its sum over a
 *   kept_res i32 [n, m, L] (or NULL)      sum over the thresholds t of the number of b with (a, b) in the set, maskA[i, a] and
 *                                          maskA[i, b], and | |A[i, a] - A[i, b]| - dn | < t (strict): a pair whose model residue
 *                                          is missing keeps nothing and stays in `total`;   kept i32 [n, m] = its sum over a
 * per-residue lDDT = kept_res / (n_thresholds total_res), global lDDT = kept / (n_thresholds total): the caller divides.
 * Distances are sqrt((dx dx + dy dy) + dz dz) in float64, correctly rounded square root, no FMA contraction.  Every element of
 * every output that is not NULL is written; nothing has to be zeroed by the caller.  Integer sums only: two runs are bit-identical
 * and a pair's counts do not depend on the launch.  The call synchronises `stream`.
 * n, m < 1, L < 2, seq_sep < 1 or a threshold count outside 1 .. 8 return ESMDIFF_E_INVALID; L > ESMDIFF_LDDT_MAX_L (one model of
 * the longest chain, 96 KiB of float64 planes, has to fit in LDS) returns ESMDIFF_E_CAPACITY, before anything is launched. */
#define ESMDIFF_LDDT_MAX_L 4096
#define ESMDIFF_LDDT_MAX_THRESHOLDS 8
int esmdiff_lddt_pairs(const double* A, int32_t n, const double* B, int32_t m, int32_t L, const uint8_t* maskA,
                       const uint8_t* maskB, double r0, const double* thresholds, int32_t n_thresholds, int32_t seq_sep,
                       int32_t* kept, int32_t* total, int32_t* kept_res, int32_t* total_res, void* stream);

/* Residue flexibility of an ensemble (float64, device pointers in and out; each call synchronises `stream`): DESIGN.md §3.21.
 * (An addition; the ABI number stays.)  A f64 [n, L, 3] CA traces, residue to residue; maskA u8 [n, L] or NULL (all valid): a masked
 * coordinate is never read into a sum (it may be NaN).  Every fit is the proper rotation (det R = +1) of esmdiff_superpose_pairs.
 * n < 1 or L < 2 return ESMDIFF_E_INVALID before anything is launched; there is no limit on L.  No float atomics: the order of every
 * sum is a function of (n, L) alone (csrc/flex.hip states it), so two runs are bit-identical.
 *
 * esmdiff_flex_pair_msf: the reference's pairwise "RMSF" (analysis/apo_analysis.py:252-260) without its [n, n, L] array.  For every
 * pair i < j, a_i is fitted onto a_j on the residues valid in both; the squared deviation of every such residue is added to
 * sum_sq f64 [L] and 1 to count i64 [L].  A pair with fewer than 2 common residues contributes nothing and is not counted.  The
 * per-pair deviations never reach memory: each wave of the launch keeps one partial sum per residue in `scratch`, and a second pass
 * adds the partials in a fixed order.  scratch: at least ESMDIFF_FLEX_PAIR_SLOTS(n) * L * 12 bytes on the device, 8-byte aligned,
 * need not be zeroed (f64 [slots, L] partial sums, then i32 [slots, L] partial counts); a smaller scratch_bytes, or scratch == NULL,
 * returns ESMDIFF_E_CAPACITY.  n = 1 has no pair: sum_sq = 0, count = 0.
 *
 * esmdiff_flex_fit: every A[i] fitted onto ONE reference ref f64 [L, 3] (mask_ref u8 [L] or NULL) on the residues valid in both.
 * aligned f64 [n, L, 3] (or NULL): the whole transformed structure, masked residues included (a NaN coordinate stays NaN);
 * rmsd f64 [n] (or NULL): over the common residues.  Fewer than 2 common residues: NaN everywhere for that structure.
 *
 * esmdiff_flex_transforms: esmdiff_flex_fit's fit with the transform written out instead of the moved structure (required): T f64
 * [n, 12], row-major rot[9] then tr[3] with rot a + tr ~ ref, what esmdiff_aligned_moments and esmdiff_aligned_project apply inside
 * their kernels; rmsd f64 [n] (or NULL), esmdiff_flex_fit's bit for bit; ok u8 [n] (required): 1 where the fit had at least 2
 * common residues, else 0 with NaN in T[i] and rmsd[i].  The argument checks and error codes of esmdiff_flex_fit, and a NULL T or ok
 * is ESMDIFF_E_INVALID.
 *
 * esmdiff_flex_moments: per residue l, over the structures i with mask[i, l] (NULL: all): mean f64 [L, 3] the mean position,
 * msf f64 [L] the mean squared distance from that mean (two passes: the mean first, then the deviations), count i32 [L] the number
 * of structures; count = 0 gives NaN in mean and msf. */
#define ESMDIFF_FLEX_PAIR_CHUNKS(n) (2048 / (((n) + 1) / 2) < 1 ? 1 : (2048 / (((n) + 1) / 2) > 16 ? 16 : 2048 / (((n) + 1) / 2)))
#define ESMDIFF_FLEX_PAIR_SLOTS(n) ((int64_t)4 * (((n) + 1) / 2) * ESMDIFF_FLEX_PAIR_CHUNKS(n))
int esmdiff_flex_pair_msf(const double* A, int32_t n, int32_t L, const uint8_t* maskA, double* sum_sq, int64_t* count, void* scratch,
                          int64_t scratch_bytes, void* stream);
int esmdiff_flex_fit(const double* A, int32_t n, int32_t L, const uint8_t* maskA, const double* ref, const uint8_t* mask_ref,
                     double* aligned, double* rmsd, void* stream);
int esmdiff_flex_transforms(const double* A, int32_t n, int32_t L, const uint8_t* maskA, const double* ref, const uint8_t* mask_ref,
                            double* T, double* rmsd, uint8_t* ok, void* stream);
int esmdiff_flex_moments(const double* X, int32_t n, int32_t L, const uint8_t* mask, double* mean, double* msf, int32_t* count,
                         void* stream);

/* Secondary structure of backbones after Kabsch & Sander 1983 ("DSSP"): float64 geometry in, backbone hydrogen bonds, INTEGER state
 * codes and their per-residue counts out, held exactly to the numpy restatement tests/dssp_ref.py.  (An addition; the ABI number
 * stays.)  DESIGN.md §3.22 states the definition — presence, chain breaks, donors and acceptors, the energy, the two-best rule, turns,
 * bridges, ladders and the passes — and the deliberate differences from the `mkdssp` program [DSSP-RECALL: parity unpinned].
 * X f64 [n, L, 4, 3]: N, CA, C, O per residue; mask u8 [n, L] or NULL (all given); no_donor u8 [L] or NULL: residues whose N carries
 * no H (proline), shared by all structures.  All pointers are device pointers; the library allocates nothing.
 *   ss       u8  [n, L]     0 '-', 1 S, 2 T, 3 I, 4 G, 5 B, 6 E, 7 H; a residue that is masked or lacks N, CA or C gets 0
 *   counts   i32 [L, 8]     or NULL: the number of structures in which residue l is present and has code c
 *   acceptor i32 [n, L, 2]  required: the two acceptors of donor j's N-H of lowest energy among those below -0.5 kcal/mol, ordered
 *                           by (energy, index); -1 in an empty slot
 *   energy   f64 [n, L, 2]  required: their energies, 0.0 in an empty slot
 * Distances are sqrt((dx dx + dy dy) + dz dz) in float64, correctly rounded square root and division, no FMA contraction.  On
 * success every element of every output is written; masked or absent residues' coordinates never influence anything (they may be NaN
 * or garbage).  Integer atomics only: two runs are bit-identical, and a structure's rows do not depend on the batch.  The call
 * synchronises `stream`.  n == 0 succeeds and zeroes counts.  n < 0, L < 1, L > ESMDIFF_DSSP_MAX_L or a required pointer that is
 * NULL return ESMDIFF_E_INVALID and touch no output. */
#define ESMDIFF_DSSP_MAX_L 4096
int esmdiff_dssp(const double* X, int32_t n, int32_t L, const uint8_t* mask, const uint8_t* no_donor, uint8_t* ss, int32_t* counts,
                 int32_t* acceptor, double* energy, void* stream);

/* Contacts of CA traces (float64 coordinates, device pointers in and out; each call synchronises `stream`): DESIGN.md §3.23, held to
 * the numpy restatement tests/contacts_ref.py.  (An addition; the ABI number stays.)  A distance is sqrt((dx dx + dy dy) + dz dz) in
 * float64, correctly rounded square root, no FMA contraction, so every comparison falls as numpy's does.  No float atomics.  Every
 * element of every output that is not NULL is written; the caller zeroes nothing.  L > ESMDIFF_CONTACT_MAX_L returns
 * ESMDIFF_E_CAPACITY, any other bad argument ESMDIFF_E_INVALID, before anything is launched.
 *
 * esmdiff_contact_map: an ensemble X f64 [n, L, 3] reduced over its frames into L x L maps.  mask u8 [n, L] or NULL (all given): a
 * masked coordinate is never read; a residue whose coordinate is NaN counts as masked in that frame.  For every pair with
 * |a - b| >= min_sep (min_sep >= 1), with V the frames in which both residues are valid:
 *   valid  i32 [L, L]            |V|
 *   count  i32 [L, L]            the number of frames of V with d(a, b) < cutoff (strict)
 *   sum_d  f64 [L, L] (or NULL)  the sum over V of d(a, b)
 *   sum_d2 f64 [L, L] (or NULL)  the sum over V of (dx dx + dy dy) + dz dz, the square root's own argument
 * (sum_d and sum_d2 are given or NULL together.)  All maps are symmetric and 0 where |a - b| < min_sep.
 * THE ORDER OF THE TWO SUMS is a function of (n, L) alone.  The frames are cut into C = ESMDIFF_CONTACT_CHUNKS(n, L) chunks of
 * F = ESMDIFF_CONTACT_CHUNK_FRAMES(n, L) consecutive frames (the last one may be shorter, none is empty).  Inside a chunk the frames
 * are added one after another in increasing index, starting from the first; a frame in which the pair is not valid adds nothing.  The
 * chunk sums are then added in increasing chunk index, starting from chunk 0's.  So two runs are bit-identical on any device, and
 * tests/contacts_ref.py follows the order bit for bit.  C is chosen so that (pair tiles x C) fills the machine: at most
 * ESMDIFF_CONTACT_MAX_CHUNKS for short chains with many frames, 1 from L = 1985 on, where the 64 x 64 tiles of the triangle alone do.
 * scratch: ESMDIFF_CONTACT_SCRATCH_BYTES(n, L) bytes on the device, 8-byte aligned, need not be zeroed (the chunks' partial tiles);
 * 0 bytes — scratch may be NULL — when there is one chunk.  A smaller scratch_bytes returns ESMDIFF_E_CAPACITY.
 *
 * esmdiff_native_contacts: every model A f64 [n, L, 3] against every native B f64 [m, L, 3], laid out as esmdiff_lddt_pairs (B == NULL:
 * A against itself, m ignored, maskB = maskA; maskA u8 [n, L] / maskB u8 [m, L] or NULL).  The native contact set of native j is
 *   C_j = {(a, b) ordered : |a - b| >= min_sep, maskB[j, a] and maskB[j, b], d0 = |B[j, a] - B[j, b]| < cutoff}   (strict)
 *   total     i32 [m]               |C_j|
 *   kept      i32 [n, m]            the number of (a, b) in C_j with maskA[i, a], maskA[i, b] and d_i(a, b) < lambda d0 (strict;
 *                                   lambda d0 is one float64 product): a pair whose model residue is missing keeps nothing and
 *                                   stays in `total`
 *   total_res i32 [m, L] (or NULL), kept_res i32 [n, m, L] (or NULL)   the same per residue a, as in esmdiff_lddt_pairs
 *   q_soft    f64 [n, m] (or NULL)  the sum over C_j of 1 / (1 + exp(beta (d_i(a, b) - lambda d0))) (Best, Hummer & Eaton 2013); a
 *                                   pair whose model residue is missing adds 0
 * Q = kept / total, soft Q = q_soft / total: the caller divides.  The order of the q_soft sum is a function of L alone (csrc/contacts.hip
 * states it: per row a its contacts in increasing b dealt to 64 lane sums, an xor butterfly, the rows a = w, w + 8 ... added per wave w,
 * the eight wave sums as a fixed tree), so two runs are bit-identical.  L > ESMDIFF_CONTACT_MAX_L (one model of the longest chain, 96 KiB
 * of float64 planes, has to fit in LDS) returns ESMDIFF_E_CAPACITY. */
#define ESMDIFF_CONTACT_MAX_L 4096
#define ESMDIFF_CONTACT_TILE 64
#define ESMDIFF_CONTACT_MAX_CHUNKS 256
#define ESMDIFF_CONTACT_TILES(L) (((L) + ESMDIFF_CONTACT_TILE - 1) / ESMDIFF_CONTACT_TILE)
#define ESMDIFF_CONTACT_PAIR_TILES(L) ((int64_t)ESMDIFF_CONTACT_TILES(L) * (ESMDIFF_CONTACT_TILES(L) + 1) / 2)
/* the most chunks a chain of L residues is ever cut into: 1024 workgroups wanted */
#define ESMDIFF_CONTACT_CHUNK_CAP(L)                                            \
  (1024 / ESMDIFF_CONTACT_PAIR_TILES(L) < 1 ? (int64_t)1                        \
   : (1024 / ESMDIFF_CONTACT_PAIR_TILES(L) > ESMDIFF_CONTACT_MAX_CHUNKS ? (int64_t)ESMDIFF_CONTACT_MAX_CHUNKS \
                                                                       : 1024 / ESMDIFF_CONTACT_PAIR_TILES(L)))
/* frames per chunk: at least 16 */
#define ESMDIFF_CONTACT_CHUNK_FRAMES(n, L)                                      \
  ((((n) + ESMDIFF_CONTACT_CHUNK_CAP(L) - 1) / ESMDIFF_CONTACT_CHUNK_CAP(L)) < 16 ? (int64_t)16 \
   : (((n) + ESMDIFF_CONTACT_CHUNK_CAP(L) - 1) / ESMDIFF_CONTACT_CHUNK_CAP(L)))
#define ESMDIFF_CONTACT_CHUNKS(n, L) (((n) + ESMDIFF_CONTACT_CHUNK_FRAMES(n, L) - 1) / ESMDIFF_CONTACT_CHUNK_FRAMES(n, L))
/* per chunk and pair tile 64 x 64 cells of two f64 and two i32; nothing with one chunk */
#define ESMDIFF_CONTACT_SCRATCH_BYTES(n, L)                                     \
  (ESMDIFF_CONTACT_CHUNKS(n, L) == 1 ? (int64_t)0                               \
   : ESMDIFF_CONTACT_CHUNKS(n, L) * ESMDIFF_CONTACT_PAIR_TILES(L) * ESMDIFF_CONTACT_TILE * ESMDIFF_CONTACT_TILE * 24)
int esmdiff_contact_map(const double* X, int32_t n, int32_t L, const uint8_t* mask, double cutoff, int32_t min_sep, int32_t* valid,
                        int32_t* count, double* sum_d, double* sum_d2, void* scratch, int64_t scratch_bytes, void* stream);
int esmdiff_native_contacts(const double* A, int32_t n, const double* B, int32_t m, int32_t L, const uint8_t* maskA,
                            const uint8_t* maskB, double cutoff, int32_t min_sep, double lambda, double beta, int32_t* kept,
                            int32_t* total, int32_t* kept_res, int32_t* total_res, double* q_soft, void* stream);

/* Backbone torsions phi / psi / omega and the Ramachandran maps of an ensemble (float64 coordinates, device pointers in and out; each
 * call synchronises `stream`): DESIGN.md §3.24, held to the numpy restatement tests/torsions_ref.py.  (An addition; the ABI number
 * stays.)  X f64 [n, L, atoms, 3] with atoms = 3 (N, CA, C) or 4 (N, CA, C, O; O is never read: the array made for esmdiff_dssp goes
 * in as it is); mask u8 [n, L] or NULL (all given).  No FMA contraction, correctly rounded square root and division.
 *   present   residue i is not masked and its N, CA and C are all finite; the coordinates of any other residue influence nothing
 *   link      i -> i + 1: both present and |C_i - N_{i+1}| <= break_distance, the length sqrt((dx dx + dy dy) + dz dz)
 *   dihedral  of p0 .. p3: b1 = p1 - p0, b2 = p2 - p1, b3 = p3 - p2, n1 = b1 x b2, n2 = b2 x b3, x = n1 . n2,
 *             y = sqrt(b2 . b2) (b1 . n2), angle = atan2(y, x), with a x b = (ay bz - az by, az bx - ax bz, ax by - ay bx) and
 *             a . b = (ax bx + ay by) + az bz; undefined when x == 0 and y == 0 or either is not finite
 *   phi_i = dihedral(C_{i-1}, N_i, CA_i, C_i) needs the link i - 1 -> i; psi_i = dihedral(N_i, CA_i, C_i, N_{i+1}) and
 *   omega_i = dihedral(CA_i, C_i, N_{i+1}, CA_{i+1}) need the link i -> i + 1
 * n < 0, L < 1, atoms not 3 or 4, a break_distance that is not positive and finite or a required pointer that is NULL return
 * ESMDIFF_E_INVALID and touch nothing.  There is no limit on L.
 *
 * esmdiff_backbone_torsions: phi, psi, omega f64 [n, L] in radians, NaN where undefined; geom f64 [n, L, 6] or NULL: the lengths
 * N-CA, CA-C, C_i-N_{i+1} (sqrt of the dot product above) and the angles N-CA-C, CA_i-C_i-N_{i+1}, C_i-N_{i+1}-CA_{i+1} in radians
 * as atan2(|u x v|, u . v) of the two bonds leaving the middle atom, NaN where a residue they touch is not present (the two that reach
 * into i + 1 do not need the link).  Every element of every output that is not NULL is written; a structure's rows do not depend on
 * its batch; n == 0 succeeds.
 *
 * esmdiff_ramachandran: the ensemble reduced over its frames, from the coordinates; memory is O(L bins^2) whatever n is.
 *   hist   i32 [L, bins, bins]  the frames in which phi_i and psi_i are both defined, at [i][bin of phi][bin of psi]; the bin of an
 *                               angle is b = (int)floor((angle * 57.29577951308232 + 180.0) / (360.0 / bins)), b -= bins where
 *                               b >= bins (+180 degrees is bin 0), b += bins where b < 0 (it is not, with atan2 in [-pi, pi])
 *   counts i32 [L, 5]           the frames with phi defined, psi defined, both, omega defined, and cis (omega defined and x > 0)
 *   sums   f64 [L, 6] or NULL   the sums of cos phi, sin phi, cos psi, sin psi, cos omega, sin omega over the frames in which that
 *                               angle is defined, with cos = x / r, sin = y / r, r = sqrt(x x + y y): no trigonometric function
 * bins is 1 .. ESMDIFF_RAMA_MAX_BINS, beyond that ESMDIFF_E_CAPACITY.  Every output is written, the caller zeroes nothing; n == 0
 * gives zeros.  Integer atomics only.  x and y are computed by the function esmdiff_backbone_torsions uses: the same bits.
 * THE ORDER OF THE SUMS is a function of (n, L) alone.  The frames are cut into C = ESMDIFF_RAMA_CHUNKS(n, L) chunks of
 * F = ESMDIFF_RAMA_CHUNK_FRAMES(n, L) consecutive frames (the last one may be shorter, none is empty).  Inside a chunk a residue's
 * terms are added one after another in increasing frame index, starting from the first defined one (a chunk without one has the sum
 * +0.0).  The chunk sums are then added in increasing chunk index, starting from chunk 0's.  So two runs are bit-identical, and
 * tests/torsions_ref.py follows the order bit for bit.
 * scratch: ESMDIFF_RAMA_SCRATCH_BYTES(n, L) bytes on the device, 8-byte aligned, need not be zeroed (C x L x 6 chunk sums); not
 * read — it may be NULL — when there is one chunk or sums is NULL.  A smaller scratch_bytes returns ESMDIFF_E_CAPACITY. */
#define ESMDIFF_RAMA_MAX_BINS 72
/* the most chunks a chain of L residues is ever cut into: one thread per (residue, chunk), about 65536 of them wanted */
#define ESMDIFF_RAMA_CHUNK_CAP(L) \
  (65536 / (int64_t)(L) < 1 ? (int64_t)1 : (65536 / (int64_t)(L) > 1024 ? (int64_t)1024 : 65536 / (int64_t)(L)))
/* frames per chunk: at least 16 */
#define ESMDIFF_RAMA_CHUNK_FRAMES(n, L)                                   \
  ((((n) + ESMDIFF_RAMA_CHUNK_CAP(L) - 1) / ESMDIFF_RAMA_CHUNK_CAP(L)) < 16 ? (int64_t)16 \
   : (((n) + ESMDIFF_RAMA_CHUNK_CAP(L) - 1) / ESMDIFF_RAMA_CHUNK_CAP(L)))
#define ESMDIFF_RAMA_CHUNKS(n, L) (((n) + ESMDIFF_RAMA_CHUNK_FRAMES(n, L) - 1) / ESMDIFF_RAMA_CHUNK_FRAMES(n, L))
#define ESMDIFF_RAMA_SCRATCH_BYTES(n, L) \
  (ESMDIFF_RAMA_CHUNKS(n, L) <= 1 ? (int64_t)0 : ESMDIFF_RAMA_CHUNKS(n, L) * (int64_t)(L) * 48)
int esmdiff_backbone_torsions(const double* X, int32_t n, int32_t L, int32_t atoms, const uint8_t* mask, double break_distance,
                              double* phi, double* psi, double* omega, double* geom, void* stream);
int esmdiff_ramachandran(const double* X, int32_t n, int32_t L, int32_t atoms, const uint8_t* mask, double break_distance,
                         int32_t bins, int32_t* hist, int32_t* counts, double* sums, void* scratch, int64_t scratch_bytes,
                         void* stream);

/* Size, shape and scattering of every frame of an ensemble of CA traces (float64 coordinates in Angstrom, device pointers in and out;
 * each call synchronises `stream`): DESIGN.md §3.25, held to the numpy restatement tests/shape_ref.py.  (An addition; the ABI number
 * stays.)  X f64 [n, L, 3]; mask u8 [n, L] or NULL (all given).  A residue is VALID in a frame when it is not masked and none of its
 * three coordinates is NaN; a masked coordinate is never read.  A distance is d = sqrt((dx dx + dy dy) + dz dz) with no FMA contraction
 * and the correctly rounded square root and division.  No float atomics.  Every element of every output that is not NULL is
 * written; the caller zeroes nothing; a frame's row does not depend on n or on the other frames; n == 0 succeeds.  A NULL required
 * pointer, n < 0, L < 1 (and with hist: bins < 1, a width that is not positive and finite; for Debye Q < 1) return
 * ESMDIFF_E_INVALID before anything is launched and touch no output; L > ESMDIFF_SHAPE_MAX_L (one frame of the longest chain, 96 KiB of
 * float64 planes, has to fit in LDS: the limit and the reason of ESMDIFF_CONTACT_MAX_L) returns ESMDIFF_E_CAPACITY.
 *
 * THE ORDER OF EVERY SUM is a function of L alone, through W = ESMDIFF_SHAPE_WAVES(L) (the waves that share a frame):
 *   over residues  lane l of 64 adds the terms of the residues b = l, l + 64, l + 128 ... in increasing b, starting from +0.0, a
 *                  residue that is not valid adding nothing; the 64 lane sums v are combined by the xor butterfly
 *                  v[l] = v[l] + v[l ^ off] for off = 32, 16, 8, 4, 2, 1.
 *   over pairs     a < b, both valid.  Wave w of W takes the rows a = w, w + W, w + 2 W ... in that order; in row a lane l takes
 *                  b = a + 1 + l, a + 1 + l + 64 ... in increasing b.  A lane keeps ONE sum, starting from +0.0, across all the
 *                  rows of its wave; a pair that is not valid adds nothing.  Then the butterfly above per wave, and for W = 8 the
 *                  wave sums as ((w0 + w1) + (w2 + w3)) + ((w4 + w5) + (w6 + w7)).
 * So two runs are bit-identical and tests/shape_ref.py follows the orders bit for bit.
 *
 * esmdiff_shape_frames: per frame i, over its N_i valid residues,
 *   count i32 [n]       N_i
 *   desc  f64 [n, 12]   [0..2]  the centroid c = (sum of r) / N_i, component by component (over residues; one division)
 *                       [3..8]  the sums of (r - c)(r - c)^T in the order xx, yy, zz, xy, xz, yz, taken in a second pass about that
 *                               centroid (over residues) and NOT divided: the gyration tensor is these / N_i, and the caller divides
 *                       [9]     sum_inv_d = the sum of 1 / d_ab (over pairs); +inf when two valid residues coincide
 *                       [10]    dmax = the largest d_ab
 *                       [11]    ree = |r_{L-1} - r_0|, NaN unless both ends are valid (L == 1: 0)
 *                       N_i == 0: the centroid is NaN, the six sums, sum_inv_d and dmax are 0, ree is NaN.  N_i == 1: the centroid
 *                       is the residue, the six sums, sum_inv_d and dmax are 0.
 *   hist  i64 [bins + 1] or NULL (width and bins are then ignored): over all frames and valid pairs a < b, cell
 *                       (int)floor(d / width), every cell >= bins counted in cell `bins` (overflow).  Zeroed by the entry; integer
 *                       atomics.  bins > ESMDIFF_SHAPE_MAX_BINS (the workgroup's histogram in LDS) returns ESMDIFF_E_CAPACITY.
 *
 * esmdiff_debye_frames: intensity f64 [n, Q], I_i(q) = sum_a f_a^2 + 2 sum_{a<b} f_a f_b s(q d_ab) over valid residues and pairs, with
 * q f64 [Q] ON THE DEVICE and ff f64 [L, Q] the form factor of residue a at q[k] at ff[a Q + k], or NULL: every f is 1 (point
 * scatterers).  x = q d is one float64 product, s(x) = sin(x) / x for x != 0 and exactly 1.0 for x == 0 (q = 0 and coincident atoms
 * give no NaN), a pair's term is (f_a f_b) s — s itself with ff == NULL — added in the order over pairs; sum_a f_a^2 is summed in
 * the order over residues, and I = that + 2.0 (pair sum).  With ff == NULL, I(q = 0) is N_i^2 exactly.  The order for a given
 * (frame, q) does not depend on n, on Q or on the position of q in the array (the kernel walks ESMDIFF_DEBYE_Q_CHUNK values of q at
 * a time, each with a sum of its own): the same q gives the same bits inside any q array.  A frame without a valid residue gives 0.
 * The entry cannot inspect q without a copy: a negative or non-finite q is the caller's to reject (esmdiff_amd/shape.py does).
 * Q > ESMDIFF_DEBYE_MAX_Q returns ESMDIFF_E_CAPACITY. */
#define ESMDIFF_SHAPE_MAX_L 4096
#define ESMDIFF_SHAPE_MAX_BINS 4096
#define ESMDIFF_SHAPE_WAVES(L) ((L) <= 128 ? 1 : 8)
#define ESMDIFF_DEBYE_MAX_Q 1024
#define ESMDIFF_DEBYE_Q_CHUNK 8
int esmdiff_shape_frames(const double* X, int32_t n, int32_t L, const uint8_t* mask, int32_t* count, double* desc, int64_t* hist,
                         double width, int32_t bins, void* stream);
int esmdiff_debye_frames(const double* X, int32_t n, int32_t L, const uint8_t* mask, const double* q, int32_t Q, const double* ff,
                         double* intensity, void* stream);

/* Solvent accessibility of every frame of an ensemble of backbones by the point test of Shrake & Rupley 1973, and the co-occurrence
 * counts of a table of two-state flags (float64 coordinates in Angstrom, device pointers in and out; each call synchronises `stream`):
 * DESIGN.md §3.26, held exactly to the numpy restatement tests/sasa_ref.py.  (An addition; the ABI number stays.)  Parity with
 * NACCESS / freesasa / mdtraj is unpinned: only the definition below is tested.
 *
 * esmdiff_sasa_frames: X f64 [n, L, A, 3] with A = 1, 3 or 4 atoms a residue; mask u8 [n, L] or NULL (all given); radii f64 [L, A], the
 * radius of every atom ALREADY EXPANDED by the probe; points f64 [P, 3], the unit points of the test sphere (the entry evaluates no
 * cosine: esmdiff_amd.accessibility.sphere_points makes the golden-section spiral in numpy).  An atom is ABSENT in a frame when its
 * residue is masked or one of its coordinates is NaN: it has no count and buries nothing, and a masked coordinate is never read.
 * Point k of atom i with centre c and radius R is p = c + R u_k, one product and one add per component with no FMA; it is BURIED
 * when some other atom j present in the frame has ((dx dx + dy dy) + dz dz) < R_j R_j, d = p - c_j, strictly; atoms of the same
 * residue and bonded neighbours are ordinary neighbours; an atom is never tested against itself.  The kernel culls candidates
 * conservatively (csrc/sasa.hip argues the margin): no count depends on it.  Outputs, each may be NULL, each one that is not is
 * written in full and the caller zeroes nothing:
 *   count         i32 [n, L, A]  the exposed points of the atom, -1 for an absent atom
 *   sum_count     i64 [L, A]     the sum of count over the frames where the atom is present
 *   valid         i32 [L, A]     the number of those frames
 *   exposed       u8  [n, L]     2 when no atom of the residue is present; else, with the atom area (s c) / P, s = 12.566370614359172
 *                                (R R), c the count as float64, the residue area ((a0 + a1) + a2) + a3 over its present atoms and the
 *                                same sum with every c = P, 1 when area / that sum > threshold and 0 when not: one division, one
 *                                comparison
 *   exposed_count i32 [L]        the frames with flag 1
 *   present_count i32 [L]        the frames with flag 0 or 1
 * The reductions over frames are integer atomics; memory for them is O(L A) whatever n is.  n == 0 zeroes the four ensemble outputs.
 * A NULL input, n < 0, L < 1, A not 1, 3 or 4, P < 1, or a NaN threshold with one of the last three outputs return ESMDIFF_E_INVALID;
 * L A > ESMDIFF_SASA_MAX_ATOMS (one frame's x, y, z, R planes and its counts, 144 KiB, have to fit in LDS) or
 * P > ESMDIFF_SASA_MAX_POINTS return ESMDIFF_E_CAPACITY; both before anything is launched or written.  Coordinates and radii are
 * assumed below 1e150 in magnitude (no square overflows).
 *
 * esmdiff_cooccurrence: flags u8 [n, L], 0 or 1, anything else undefined (2 above) -> out i32 [3, L, L]:
 *   out[0][a][b]  the frames in which a and b are both defined
 *   out[1][a][b]  of those, the frames in which a is 1
 *   out[2][a][b]  of those, the frames in which both are 1
 * Nothing in it knows about exposure.  A first pass packs 64 frames into a word per residue by ballot (a plane of ones and a plane
 * of defined), a second ANDs the words of a and b and counts bits.  scratch: ESMDIFF_COOCC_SCRATCH_BYTES(n, L) bytes on the device,
 * 8-byte aligned, need not be zeroed; a smaller scratch_bytes returns ESMDIFF_E_CAPACITY, as does L > ESMDIFF_COOCC_MAX_L.  n == 0
 * needs no scratch (it may be NULL) and gives zeros.  NULL flags or out, a NULL scratch where one is needed, n < 0, L < 1 return
 * ESMDIFF_E_INVALID.  A refused call writes nothing. */
#define ESMDIFF_SASA_MAX_ATOMS 4096
#define ESMDIFF_SASA_MAX_POINTS 1024
#define ESMDIFF_COOCC_MAX_L 32768
#define ESMDIFF_COOCC_SCRATCH_BYTES(n, L) ((((int64_t)(n) + 63) / 64) * (int64_t)(L) * 16)
int esmdiff_sasa_frames(const double* X, int32_t n, int32_t L, int32_t A, const uint8_t* mask, const double* radii, const double* points,
                        int32_t P, double threshold, int32_t* count, int64_t* sum_count, int32_t* valid, uint8_t* exposed,
                        int32_t* exposed_count, int32_t* present_count, void* stream);
int esmdiff_cooccurrence(const uint8_t* flags, int32_t n, int32_t L, int32_t* out, void* scratch, int64_t scratch_bytes, void* stream);

/* The time-lagged moments of a trajectory's features, fused from the coordinates: what a TICA / VAMP fit needs of n frames in
 * O(D^2) memory (float64, device pointers in and out; each call synchronises `stream`): DESIGN.md §3.27, restated in numpy by
 * tests/kinetics_ref.py.  (An addition; the ABI number stays.)  csrc/lagged.hip; the layer above is esmdiff_amd/kinetics.py.
 *
 * INPUT, the same in the three entries: pwd_offset = 0: X is a feature matrix f64 [n, D] and L_or_D is D (up to
 * ESMDIFF_LAGGED_MAX_D).  pwd_offset = k >= 1: X is CA coordinates f64 [n, L, 3], L_or_D is L (k < L <= ESMDIFF_LAGGED_MAX_L), and
 * the D = ESMDIFF_LAGGED_FEATURES(L, k) features are the distances of the pairs (i, j >= i + k) in numpy.triu_indices order, each
 * sqrt((dx dx + dy dy) + dz dz) with no FMA: the bits of esmdiff_metrics_pwd.  The distances are recomputed inside the kernels; no
 * [n, D] array exists.  Non-finite input is not looked for (esmdiff_amd/kinetics.py refuses it).
 *
 * With m = n - lag, a_t = f(x_t) - c and b_t = f(x_{t + lag}) - c for t < m.  The t are cut into chunks of
 * ESMDIFF_LAGGED_FRAME_CHUNK; a chunk's sums go to a slot of `scratch` and the slots are added to the outputs in increasing chunk
 * index, starting from chunk 0's own sums.  scratch (device, 8-byte aligned, need not be zeroed) holds the pair table
 * (ESMDIFF_LAGGED_TABLE_BYTES(D)) and then as many slots as fit, at least one: ESMDIFF_LAGGED_MEANS_SCRATCH_BYTES(D, slots) /
 * ESMDIFF_LAGGED_MOMENTS_SCRATCH_BYTES(D, slots).  More slots let more chunks run at once and change no bit: every output is a
 * function of (X, c, n, lag) alone, the same on every run and every device.
 *
 * esmdiff_lagged_means: mean0[D], meant[D] = the means of f over t < m and over t + lag.  A chunk's sum is s = 0, s = s + f(x_t)
 * in increasing t; the total of the chunks (in order) is divided by m once.
 * esmdiff_lagged_moments: center c[D] (required) -> S00 = sum a a^T, S0t = sum a b^T, Stt = sum b b^T (f64 [D, D] each, raw sums,
 * undivided) and r0 = sum a, rt = sum b ([D], summed as the means are, a_t = f(x_t) - c the summand).  A chunk's matrix sums are
 * accumulated by v_mfma_f64_16x16x4_f64 over its t in increasing order, four t to an instruction.  S00 and Stt are computed for
 * column tile >= row tile only and mirrored: they are exactly symmetric.
 * esmdiff_lagged_project: Y[n, dim] = (f(x_t) - mean) W with W f64 [D, dim], 1 <= dim <= ESMDIFF_LAGGED_MAX_DIM.  Per frame and
 * column, p_l = 0 then p_l = p_l + (f_d - mean_d) * W[d][k] for d = l, l + 64, ... (l = 0 .. 63), then p_l = p_l + p_{l ^ s} for
 * s = 32, 16, 8, 4, 2, 1: a tree that depends on D alone, so a frame's row does not depend on the batch.  scratch: the pair table
 * only (may be NULL when pwd_offset = 0); n = 0 is allowed and writes nothing.
 *
 * ESMDIFF_E_INVALID, before anything is launched or written: a NULL pointer (center included), lag < 1, n <= lag, pwd_offset < 0 or
 * >= L, L > ESMDIFF_LAGGED_MAX_L, D > ESMDIFF_LAGGED_MAX_D in the feature form, dim outside 1 .. ESMDIFF_LAGGED_MAX_DIM, a scratch
 * smaller than one slot's. */
#define ESMDIFF_LAGGED_MAX_L 128
#define ESMDIFF_LAGGED_MAX_D 8192
#define ESMDIFF_LAGGED_MAX_DIM 16
#define ESMDIFF_LAGGED_FRAME_CHUNK 2048
#define ESMDIFF_LAGGED_FEATURES(L, k) ((((int64_t)(L) - (k)) * ((int64_t)(L) - (k) + 1)) / 2)
#define ESMDIFF_LAGGED_TABLE_BYTES(D) ((int64_t)(D) * 8)
#define ESMDIFF_LAGGED_MEANS_SCRATCH_BYTES(D, slots) (ESMDIFF_LAGGED_TABLE_BYTES(D) + (int64_t)(slots) * 2 * (int64_t)(D) * 8)
#define ESMDIFF_LAGGED_MOMENTS_SCRATCH_BYTES(D, slots) \
  (ESMDIFF_LAGGED_TABLE_BYTES(D) + (int64_t)(slots) * (3 * (int64_t)(D) * (int64_t)(D) + 2 * (int64_t)(D)) * 8)
int esmdiff_lagged_means(const double* X, int32_t n, int32_t L_or_D, int32_t pwd_offset, int32_t lag, double* mean0, double* meant,
                         void* scratch, int64_t scratch_bytes, void* stream);
int esmdiff_lagged_moments(const double* X, int32_t n, int32_t L_or_D, int32_t pwd_offset, int32_t lag, const double* center, double* S00,
                           double* S0t, double* Stt, double* r0, double* rt, void* scratch, int64_t scratch_bytes, void* stream);
int esmdiff_lagged_project(const double* X, int32_t n, int32_t L_or_D, int32_t pwd_offset, const double* mean, const double* W, int32_t dim,
                           double* Y, void* scratch, int64_t scratch_bytes, void* stream);

/* The discrete side of the kinetics pipeline: k-means on the slow coordinates and the lagged transition counts of the labels, what a
 * Markov state model needs of n frames in O(k d + k^2) memory (float64 and integers, device pointers in and out; each call
 * synchronises `stream`): DESIGN.md §3.28, restated in numpy by tests/states_ref.py.  (An addition; the ABI number stays.)
 * csrc/msm.hip; the layer above is esmdiff_amd/states.py.
 *
 * INPUT.  Y is f64 [n, d] with 1 <= d <= ESMDIFF_LAGGED_MAX_DIM (what esmdiff_lagged_project writes), centres f64 [k, d] with
 * 1 <= k <= ESMDIFF_KMEANS_MAX_K.  The squared distance of a frame to centre j is s = 0, then s = s + (y_c - c_jc) * (y_c - c_jc)
 * for c = 0 ... d - 1, a product and an add, no FMA.  The label is the SMALLEST j that attains the minimum: the running (minimum,
 * index) starts as (+inf, -1) and centre j, taken in increasing j through LDS tiles of ESMDIFF_KMEANS_CENTRE_TILE, replaces it when
 * s < minimum, strictly.  A distance that is not finite (a non-finite component of the centre or of the frame, or squares that
 * overflow) is never below the minimum: such a centre is never chosen, a frame with a non-finite component is labelled -1, and so is
 * every frame when no centre is finite.  The dist2 of a frame labelled -1 is NaN.
 *
 * esmdiff_kmeans_assign: labels i32 [n], dist2 f64 [n] (may be NULL).  n = 0 writes nothing.
 * esmdiff_kmeans_step: one Lloyd step in one pass over Y: labels (may be NULL) as above, counts i64 [k] (the frames of every label),
 * sums f64 [k, d] and inertia f64 [1].  The frames are cut into ESMDIFF_KMEANS_CHUNKS(n) chunks of ESMDIFF_KMEANS_FRAME_CHUNK.  Within
 * a chunk cluster j's sum in component c is s = +0.0, then s = s + y_tc over the chunk's frames labelled j in increasing t, and the
 * chunk's inertia is the same running sum of dist2 over its frames labelled >= 0.  A chunk's sums go to a slot of `scratch`
 * (ESMDIFF_KMEANS_SLOT_BYTES(k, d)) and the slots are added to the outputs in increasing chunk index, starting from chunk 0's own
 * sums: an empty cluster gives +0.0 and count 0.  Frames labelled -1 contribute to nothing.  scratch (device, 8-byte aligned, need not
 * be zeroed) holds as many slots as fit, at least one: ESMDIFF_KMEANS_STEP_SCRATCH_BYTES(k, d, slots).  More slots let more chunks run
 * at once and change no bit: every output is a function of (Y, centres) alone, the same on every run and every device.  n = 0 gives
 * zeros.  No float atomics.
 * esmdiff_transition_counts: labels i32 [n], lag >= 1 -> counts i64 [k, k], counts[a][b] = the number of t < n - lag with
 * labels[t] = a and labels[t + lag] = b, both >= 0 (the sliding-window count; a negative label takes part in no pair); lag >= n gives
 * zeros.  The entry zeroes counts itself.  A label >= k is looked for by a pass of its own, whose flag (scratch, at least
 * ESMDIFF_TRANSITION_SCRATCH_BYTES) the entry reads back before anything is written.  Integer atomics: a workgroup-private LDS
 * histogram over ESMDIFF_TRANSITION_FRAME_CHUNK values of t while k <= ESMDIFF_TRANSITION_LDS_MAX_K (k * k i32 in 64 KiB), added to
 * counts with 64-bit global atomics; above that one 64-bit global atomic per pair.
 *
 * Before anything is launched or written: ESMDIFF_E_INVALID for a NULL pointer (scratch included; not the optional outputs, nor the frames' arrays of n = 0), n < 0,
 * d < 1, k < 1, lag < 1, and, after the check pass alone, for a label >= k; ESMDIFF_E_CAPACITY for d > ESMDIFF_LAGGED_MAX_DIM,
 * k > ESMDIFF_KMEANS_MAX_K and a scratch smaller than one slot's (the flag's). */
#define ESMDIFF_KMEANS_MAX_K 4096
#define ESMDIFF_KMEANS_CENTRE_TILE 128
#define ESMDIFF_KMEANS_FRAME_CHUNK 1024
#define ESMDIFF_KMEANS_CHUNKS(n) (((int64_t)(n) + ESMDIFF_KMEANS_FRAME_CHUNK - 1) / ESMDIFF_KMEANS_FRAME_CHUNK)
#define ESMDIFF_KMEANS_SLOT_BYTES(k, d) (((int64_t)(k) * (int64_t)(d) + (int64_t)(k) + 1) * 8)
#define ESMDIFF_KMEANS_STEP_SCRATCH_BYTES(k, d, slots) ((int64_t)(slots) * ESMDIFF_KMEANS_SLOT_BYTES(k, d))
#define ESMDIFF_TRANSITION_FRAME_CHUNK 4096
#define ESMDIFF_TRANSITION_LDS_MAX_K 128
#define ESMDIFF_TRANSITION_SCRATCH_BYTES 8
int esmdiff_kmeans_assign(const double* Y, int32_t n, int32_t d, const double* centres, int32_t k, int32_t* labels, double* dist2, void* stream);
int esmdiff_kmeans_step(const double* Y, int32_t n, int32_t d, const double* centres, int32_t k, int32_t* labels, int64_t* counts, double* sums,
                        double* inertia, void* scratch, int64_t scratch_bytes, void* stream);
int esmdiff_transition_counts(const int32_t* labels, int32_t n, int32_t k, int32_t lag, int64_t* counts, void* scratch, int64_t scratch_bytes,
                              void* stream);

/* The mean and the 3L x 3L covariance of an ensemble's frames superposed on a reference, as raw sums, and the projection of the
 * superposed frames: what a comparison of two ensembles in Cartesian space needs of n frames in O(L^2) memory (float64, device
 * pointers in and out; each call synchronises `stream`): DESIGN.md §3.29, restated in numpy by tests/aligned_ref.py.  (An addition;
 * the ABI number stays.)  csrc/aligned.hip; the layer above is esmdiff_amd/covariance.py.
 *
 * INPUT, the same in both entries: X f64 [n, L, 3] CA coordinates, 1 <= L <= ESMDIFF_ALIGNED_MAX_L; T f64 [n, 12] (row-major rot[9],
 * then tr[3]: what esmdiff_flex_transforms writes) or NULL (the identity).  With D = 3 L, d = 3 l + c and (x, y, z) = X[t][l] the
 * feature is f_d(t) = (((R[c][0] x + R[c][1] y) + R[c][2] z) + tr[c]), products and adds in that order with no FMA; T == NULL:
 * f_d(t) = X[t][l][c] exactly.  The transform is applied inside the kernels; no moved [n, L, 3] array exists.  Non-finite input is
 * not looked for (esmdiff_amd/covariance.py leaves such frames out through `use`).
 *
 * esmdiff_aligned_moments: center c f64 [D] (required), use u8 [n] or NULL (every frame) -> with a(t) = f(t) - c over the t with
 * use[t] != 0: S f64 [D, D] = sum a a^T and r f64 [D] = sum a (raw sums, undivided), count i64 [1] = the number of those t.  A frame
 * with use[t] == 0 is staged as zeros and not counted; its coordinates and its T row are never read (they may be NaN) and it changes
 * no bit of any sum.  The t are cut into chunks of ESMDIFF_ALIGNED_FRAME_CHUNK; a chunk's sums go to a slot of `scratch` and the
 * slots are added to the outputs in increasing chunk index, starting from chunk 0's own sums.  Within a chunk S is accumulated by
 * v_mfma_f64_16x16x4_f64 over its t in increasing order, four t to an instruction, for column tile >= row tile only and mirrored: S
 * is exactly symmetric; r_d is s = +0.0, then s = s + a_d(t) in increasing t.  scratch (device, 8-byte aligned, need not be zeroed)
 * holds as many slots as fit, at least one: ESMDIFF_ALIGNED_MOMENTS_SCRATCH_BYTES(L, slots).  More slots let more chunks run at once
 * and change no bit: every output is a function of (X, T, use, c, n, L) alone, the same on every run and every device.  No float
 * atomics.
 * esmdiff_aligned_project: Y[n, dim] = (f(t) - mean) W with mean f64 [D], W f64 [D, dim], 1 <= dim <= ESMDIFF_ALIGNED_MAX_DIM.  Per
 * frame and column, p_l = 0 then p_l = p_l + (f_d - mean_d) * W[d][k] for d = l, l + 64, ... (l = 0 .. 63), then p_l = p_l + p_{l ^ s}
 * for s = 32, 16, 8, 4, 2, 1 (esmdiff_lagged_project's order): a tree that depends on D alone, so a frame's row does not depend on
 * the batch.  n = 0 is allowed and writes nothing.
 *
 * Before anything is launched or written: ESMDIFF_E_INVALID for a NULL required pointer (center and scratch included), n < 1 (the
 * projection: n < 0), L < 1, dim outside 1 .. ESMDIFF_ALIGNED_MAX_DIM, a scratch smaller than one slot's; ESMDIFF_E_CAPACITY for
 * L > ESMDIFF_ALIGNED_MAX_L (the TM kernel's cap: D = 3840, a slot of 118 MB). */
#define ESMDIFF_ALIGNED_MAX_L 1280
#define ESMDIFF_ALIGNED_MAX_DIM 16
#define ESMDIFF_ALIGNED_FRAME_CHUNK 128
#define ESMDIFF_ALIGNED_MOMENTS_SCRATCH_BYTES(L, slots) \
  ((int64_t)(slots) * (9 * (int64_t)(L) * (int64_t)(L) + 3 * (int64_t)(L)) * 8)
int esmdiff_aligned_moments(const double* X, int32_t n, int32_t L, const double* T, const uint8_t* use, const double* center, double* S,
                            double* r, int64_t* count, void* scratch, int64_t scratch_bytes, void* stream);
int esmdiff_aligned_project(const double* X, int32_t n, int32_t L, const double* T, const double* mean, const double* W, int32_t dim,
                            double* Y, void* stream);

/* Nearest neighbours between two ensembles under the least-squares RMSD, with neither a rotation nor an (n, m) matrix (float64, device
 * pointers in and out; each call synchronises `stream`): DESIGN.md §3.30, restated in numpy by tests/neighbours_ref.py.  (An addition;
 * the ABI number stays.)  csrc/rmsd_nn.hip; the layer above is esmdiff_amd/neighbours.py.  With both sides centred on ONE set of N
 * residues: msd(i, j) = max(0, ((G_a[i] + G_b[j]) - 2 ((s1 + s2) + sigma s3)) / N), G = sum |x - c|^2, s1 >= s2 >= s3 the singular
 * values of H_ij = sum_l a_il b_jl^T; sigma = -1 when allow_reflection == 0 and det H_ij < 0, else +1.
 *
 * esmdiff_rmsd_prepare: X f64 [n, L, 3]; sel u8 [L] or NULL (every residue); n_sel = the number of nonzero sel (L when NULL), which the
 * caller counts.  Per frame over the selected residues: info f64 [n, 4] = the centroid, then G about it; use u8 [n] = 0 when a selected
 * coordinate is non-finite or G is not finite (then info = 0 and the frame's P is zeros), else 1; P f64 [n, 3, K] with
 * K = ESMDIFF_RMSD_NN_PADDED(n_sel): P[t][c][k] = component c of the k-th selected residue minus the centroid, k >= n_sel zero.  The
 * sums: lane l of a wave adds the selected residues among l, l + 64, ... in increasing order from +0.0, then s_l = s_l + s_{l ^ d} for
 * d = 32, 16, 8, 4, 2, 1; the centroid is that sum / n_sel, G the same walk over ((dx dx + dy dy) + dz dz).  ESMDIFF_E_INVALID before
 * any launch for a NULL pointer, n < 1, L < 1, n_sel < 2, n_sel > L, sel == NULL with n_sel != L.
 *
 * esmdiff_rmsd_nearest: the prepared sides (P, info, use) of A (n frames) and B (m frames) with the same n_sel.  PB == NULL: A against
 * itself over pairs i != j (m, infoB, useB ignored; the col_* outputs are not written).  A frame with use == 0 is never read and takes
 * part in no pair.  Outputs, each may be NULL: row_rmsd f64 [n] = sqrt of the minimum msd over j and row_index i32 [n] the lowest j that
 * attains it (NaN and -1 without a pair); row_sum f64 [n] = sum_j sqrt(msd) and row_pairs i64 [n] the pairs in it; row_count i64
 * [n, n_cutoffs] the j with sqrt(msd) <= cutoffs[t] (cutoffs: a HOST array of n_cutoffs <= ESMDIFF_RMSD_NN_MAX_CUTOFFS values, read
 * before the call returns); col_* the same for the frames of B; hist i64 [bins], bin min(bins - 1, floor(sqrt(msd) / width)) over
 * every pair (PB == NULL: every unordered pair once), bins <= ESMDIFF_RMSD_NN_MAX_BINS, bins == 0: no histogram; msd f64 [n, m] (NaN
 * where a frame is unused; PB == NULL: [n, n], symmetric, diagonal 0) and cross f64 [n, m, 9] the raw H_ij, for tests and small
 * problems.  msd(i, j) is a pure function of the two frames' P rows and G.  The pairs are cut into rectangles of ESMDIFF_RMSD_NN_RECT
 * frames a side, numbered row-major (PB == NULL: column block >= row block); within a rectangle a row's pairs are taken in increasing j
 * and a column's in increasing i (sum = sum + sqrt(msd) from +0.0, minimum by strict <), a rectangle's partials go to a slot of
 * `scratch`, and a frame's partials are folded in increasing rectangle number (PB == NULL: its pairs j < i before its pairs j > i).
 * scratch (device, 8-byte aligned, need not be zeroed): ESMDIFF_RMSD_NN_SCRATCH_BYTES(n, m, slots) with m = 0 for PB == NULL and at
 * least one slot; more slots let more rectangles run at once and change no bit.  No float atomics.
 * Before anything is launched or written: ESMDIFF_E_INVALID for a NULL required pointer, n < 1, m < 1 with PB, n_sel < 2, n_cutoffs
 * outside 0 .. ESMDIFF_RMSD_NN_MAX_CUTOFFS, bins < 0, bins > 0 without hist or a positive width; ESMDIFF_E_CAPACITY for
 * bins > ESMDIFF_RMSD_NN_MAX_BINS and for a NULL or too small scratch. */
#define ESMDIFF_RMSD_NN_TILE 32
#define ESMDIFF_RMSD_NN_RECT 128
#define ESMDIFF_RMSD_NN_MAX_CUTOFFS 8
#define ESMDIFF_RMSD_NN_MAX_BINS 2048
#define ESMDIFF_RMSD_NN_PADDED(n_sel) (((n_sel) + 3) / 4 * 4)
#define ESMDIFF_RMSD_NN_STATE_BYTES 96
#define ESMDIFF_RMSD_NN_SLOT_BYTES (2 * ESMDIFF_RMSD_NN_RECT * 56)
#define ESMDIFF_RMSD_NN_SCRATCH_BYTES(n, m, slots) \
  (((int64_t)(n) + (int64_t)(m)) * ESMDIFF_RMSD_NN_STATE_BYTES + (int64_t)(slots) * ESMDIFF_RMSD_NN_SLOT_BYTES)
int esmdiff_rmsd_prepare(const double* X, int32_t n, int32_t L, const uint8_t* sel, int32_t n_sel, double* P, double* info, uint8_t* use,
                         void* stream);
int esmdiff_rmsd_nearest(const double* PA, const double* infoA, const uint8_t* useA, int32_t n, const double* PB, const double* infoB,
                         const uint8_t* useB, int32_t m, int32_t n_sel, int32_t allow_reflection, const double* cutoffs, int32_t n_cutoffs,
                         int32_t bins, double width, double* row_rmsd, int32_t* row_index, double* row_sum, int64_t* row_pairs,
                         int64_t* row_count, double* col_rmsd, int32_t* col_index, double* col_sum, int64_t* col_pairs, int64_t* col_count,
                         int64_t* hist, double* msd, double* cross, void* scratch, int64_t scratch_bytes, void* stream);

/* Per-kernel entry points of the parity tests, the per-section profiler of bench.py's roofline leg and the -DED_DEBUG
 * measurement aids are declared in esmdiff_hip_test.h: they are exported by the same library but are not part of the surface a
 * binding of the reference's call sites needs. */

#ifdef __cplusplus
}
#endif
#endif /* ESMDIFF_HIP_H */

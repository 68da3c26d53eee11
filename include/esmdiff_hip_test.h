/*
 * esmdiff_hip_test.h — entry points of libesmdiff_hip.so that are NOT part of the drop-in surface (esmdiff_hip.h): one kernel
 * at a time for the parity tests (tests/test_gpu_*.py compare each against a float32 / float64 statement of the same op), the
 * per-section device-time profiler bench.py's roofline leg reads, and the timing aid of -DED_DEBUG builds.  No call site
 * of the reference binds any of them; same conventions as esmdiff_hip.h (device pointers owned by the caller, int status,
 * caller's stream).
 */
#ifndef ESMDIFF_HIP_TEST_H
#define ESMDIFF_HIP_TEST_H

#include "esmdiff_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* C[M,N] (+)= A[M,K] · W[N,K]^T, bf16 in, f32 accumulate.  epilogue: see esmdiff_gemm_epilogue. */
typedef enum {
  ESMDIFF_EPI_BF16 = 0,       /* out bf16 [M,N]                                   */
  ESMDIFF_EPI_RESID_F32 = 1,  /* out f32 [M,N] += acc * alpha   (residual stream)   */
  ESMDIFF_EPI_SWIGLU_BF16 = 2,/* W rows interleaved gate/up in blocks of 32; out bf16 [M,N/2] */
  ESMDIFF_EPI_BIAS_GELU_BF16 = 3, /* out bf16 = gelu(acc + bias[N])                 */
  ESMDIFF_EPI_BIAS_F32 = 4    /* out f32 [M,ldc] = acc + bias; a 4-column group is skipped only when it would cross ldc */
} esmdiff_gemm_epilogue;

/* n_valid is not a bound of these kernels (neither the 128-column nor the 256x256 one reads it): with ESMDIFF_EPI_BIAS_F32 every
 * 4-column group that ends at or before ldc is stored, so columns n_valid .. ldc-1 receive acc + bias like the others (with zero
 * weight rows from n_valid up, as the engine pads them: the bias).  ldc % 4 == 0 and the caller allocates ldc columns per row;
 * nothing is written at or past ldc.  (esmdiff_gemm_f32 below does stop at n_valid.) */

int esmdiff_gemm_bf16(const void* A, const void* W, void* out, const float* bias, int32_t M, int32_t N,
                      int32_t K, int32_t ldc, int32_t n_valid, float alpha, int32_t epilogue, void* stream);

/* The same kernels in their f16 build (csrc/ed_half.h, namespace ed16; what precision = ESMDIFF_PRECISION_F16 engines run): A, W and
 * the 16-bit outputs are IEEE half instead of bfloat16, conversions saturate at +-65504; everything else as esmdiff_gemm_bf16. */
int esmdiff_gemm_f16(const void* A, const void* W, void* out, const float* bias, int32_t M, int32_t N,
                     int32_t K, int32_t ldc, int32_t n_valid, float alpha, int32_t epilogue, void* stream);

/* The strict path's linear (csrc/strict.hip): out f32 [M,ldc] = epi(A f32 [M,K] (row stride lda) . W f32 [N,K]^T), every
 * product and sum in float32 on v_mfma_f32_32x32x2_f32 (fixed, batch-independent K order per output element; not ascending k);
 * K % 32 == 0; columns >= n_valid are not written. */
typedef enum {
  ESMDIFF_F32EPI_STORE = 0,      /* out = acc (+ bias[N] when bias != NULL)                        */
  ESMDIFF_F32EPI_BIAS_GELU = 1,  /* out = gelu(acc + bias), exact (erf) GELU                        */
  ESMDIFF_F32EPI_RESID_DIV = 2   /* out = out + acc / div  (x + branch / scaling_factor, in place)  */
} esmdiff_gemm_f32_epilogue;
int esmdiff_gemm_f32(const float* A, int32_t lda, const float* W, float* out, const float* bias, int32_t M, int32_t N,
                     int32_t K, int32_t ldc, int32_t n_valid, float div, int32_t epilogue, void* stream);

/* The F32_SPLIT path's linear and its operand preparation (csrc/gemm_split.hip, csrc/gemm256w4_split.hip).
 *   esmdiff_split_rows    src f32 [M,K] (row stride ld) -> a3 f16 [M,3K] = [hi | lo | hi] of src * 2^k(row), rs[M] = 2^-k(row)
 *   esmdiff_split_weight  src f32 [N,K] -> w3 f16 [N_pad,3K] = [lo | hi | hi] of src * 2^k (rows N..N_pad-1 zero-filled,
 *                         N_pad a multiple of 256 >= N), *inv_scale_out [host] = 2^-k; synchronous
 *   esmdiff_gemm_split    out f32 [M,ldc] = epi(rs[m] * w_inv_scale * A . W^T [+ bias[N]]); N (= N_pad) % 256 == 0,
 *                         K % 128 == 0, ldc % 4 == 0, ldc >= N: whole padded rows are written (the kernel carries no column
 *                         bound); rows >= M and columns N .. ldc-1 are never written.  rs NULL: no row scale.  epilogue:
 *                           ESMDIFF_F32EPI_STORE      out = v; with bias != NULL the bias kernel runs (launcher code 3): v + bias[n]
 *                           ESMDIFF_F32EPI_RESID_DIV  out = out + v / div, in place (bias ignored)
 *                           4                         the fused SwiGLU of FFN-up: W rows interleaved gate / up in blocks of 32
 *                                                     (rows 64t .. 64t+31 gate 32t .., rows 64t+32 .. 64t+63 up 32t ..: what
 *                                                     esmdiff_interleave_swiglu makes), out f32 [M, N / 2] = silu(g) * u with
 *                                                     g, u the scaled products, as g * rcp(1 + exp2(-g log2 e)) * u; ldc >= N / 2,
 *                                                     columns N / 2 .. ldc-1 never written (bias ignored)
 *                         anything else (3 included) is refused, as is every shape above, before any launch. */
int esmdiff_split_rows(const float* src, int32_t ld, void* a2, float* rs, int32_t M, int32_t K, void* stream);
int esmdiff_split_weight(const float* src, void* w2, int32_t N, int32_t N_pad, int32_t K, float* inv_scale_out);
int esmdiff_gemm_split(const void* a2, const float* rs, const void* w2, float w_inv_scale, float* out, const float* bias,
                       int32_t M, int32_t N, int32_t K, int32_t ldc, float div, int32_t epilogue, void* stream);

/* The same GEMM as the engine issues it: with the engine's split-K workspace, so the small-M path (M < 1152 rows,
 * K >= 2048: FFN-down) runs as K slices + a fixed-order reduce kernel (csrc/gemm.hip).  Not re-entrant per engine. */
int esmdiff_gemm_bf16_ws(esmdiff_engine* eng, const void* A, const void* W, void* out, const float* bias, int32_t M,
                         int32_t N, int32_t K, int32_t ldc, int32_t n_valid, float alpha, int32_t epilogue,
                         void* stream);

/* What launch of esmdiff_gemm_bf16 / _f16 / _bf16_ws a shape gets, as numbers and without running anything: answered by the
 * dispatcher the launcher itself calls (csrc/gemm.hip: choose_gemm).  ws_floats: size of the split-K workspace the launch would be
 * handed (0: none, as esmdiff_gemm_bf16 and _f16 run).  M > 0, N % 128 == 0, K % 64 == 0.
 *   *w4_out      1: the four-wave 256x256 kernel (csrc/gemm256w4.hip), then rows = 256, splits = 1, stages = 2;  0: the 128-column kernel
 *   *rows_out    rows per tile (64 or 128)      *splits_out  K slices S (> 1: slices + the fixed-order reduce kernel)
 *   *stages_out  LDS stages (4: the counted-vmcnt ring, 2: double buffer) */
int esmdiff_describe_gemm_choice(int32_t M, int32_t N, int32_t K, int64_t ws_floats, int32_t* w4_out, int32_t* rows_out,
                                 int32_t* splits_out, int32_t* stages_out);
/* Floats in the split-K workspace esmdiff_gemm_bf16_ws hands its launch (0: the engine has none): the ws_floats of that engine. */
int esmdiff_gemm_workspace_floats(const esmdiff_engine* eng, int64_t* floats_out);

/* The small-batch form of a residual branch (M < 1152 rows; csrc/engine_forward.hip::forward): the branch linear A[M,K] W[N,K]^T
 * is left as S raw f32 K-slice planes in the engine's workspace (S = *splits_out, a function of N and K only) and the
 * LayerNorm kernel that follows sums them:  x[M,N] f32 += alpha * (A W^T);  y bf16 [M,N] = LayerNorm(x) * w (+ b).
 * N = d_model of the engine's shapes (N % 128 == 0, N <= 2048), K % 64 == 0.  Not re-entrant per engine. */
int esmdiff_branch_linear_layernorm(esmdiff_engine* eng, const void* A, const void* W, float* x, float alpha,
                                    const float* w, const float* b, void* y, int32_t M, int32_t N, int32_t K,
                                    int32_t* splits_out, void* stream);

/* y bf16 [M,D] = LayerNorm(x f32 [M,D]) * w (+ b); b may be NULL.  eps = 1e-5. */
int esmdiff_layernorm_bf16(const float* x, const float* w, const float* b, void* y, int32_t M, int32_t D,
                           void* stream);

/* Attention over pre-processed heads: qkv bf16 [B*L, 3*D] (GEMM output) -> ctx bf16 [B*L, D].
 * Applies the full-width q/k LayerNorm (weights f32 [D]), rotary, 1/sqrt(64) scaling, non-causal softmax. */
int esmdiff_attention_bf16(esmdiff_engine* eng, const void* qkv, const float* q_ln_w, const float* k_ln_w,
                           void* ctx, int32_t B, int32_t L, void* stream);

/* esmdiff_attention_bf16 for f16 engines (precision = ESMDIFF_PRECISION_F16): qkv and ctx are IEEE half; refuses other engines. */
int esmdiff_attention_f16(esmdiff_engine* eng, const void* qkv, const float* q_ln_w, const float* k_ln_w,
                          void* ctx, int32_t B, int32_t L, void* stream);

/* Ragged attention (esmdiff_set_lengths' kernels) in the engine's own precision: q/k LayerNorm + rotary + attention of qkv
 * [B*L, 3*D] -> ctx [B*L, D], bf16 / f16 for 16-bit engines, f32 for F32 and F32_SPLIT ones (F32_SPLIT: unit split scales).
 * lens: HOST int32 [B], each in 1..L (sample b valid on tokens [0, lens[b]), its context rows beyond are written as zeros), or
 * NULL for the plain kernels.  Synchronous when lens is given. */
int esmdiff_attention_ragged(esmdiff_engine* eng, const void* qkv, const float* q_ln_w, const float* k_ln_w, void* ctx,
                             const int32_t* lens, int32_t B, int32_t L, void* stream);

/* The q/k LayerNorm + rotary kernel alone, in the engine's 16-bit build (bf16 or f16; float32 engines are refused) with its
 * rotary tables: qkv [B*L, 3*H*64] -> q, k [B*L, H*64] token-major, q pre-scaled by log2(e)/8.  H (1 .. 32) is explicit and
 * independent of the engine's n_heads; L <= max_len. */
int esmdiff_qk_norm_rope(esmdiff_engine* eng, const void* qkv, const float* q_ln_w, const float* k_ln_w, void* q, void* k,
                         int32_t B, int32_t L, int32_t H, void* stream);

/* The 16-bit attention kernel alone (csrc/attention.hip: attention_kernel_occ4, with lens its ragged twin), on operands the
 * caller made: softmax(q k^T) v per 64-wide head, base 2.  dtype 0: bf16 (namespace ed), 1: f16 (ed16).  q, k [B*L, H*64] as
 * launch_attention takes them: q already multiplied by log2(e)/8 and rounded to the 16-bit type (what esmdiff_qk_norm_rope
 * writes).  qkv [B*L, 3*H*64]: only its V third is read, in place.  ctx [B*L, H*64].  lens: HOST int32 [B], each in 1..L, or
 * NULL (as esmdiff_attention_f32_parts: with lens the call waits for `stream`, without it is enqueued and returns).  No engine;
 * 1 <= H <= 32; every argument is checked before the first HIP call (ESMDIFF_E_INVALID). */
int esmdiff_attention_16_parts(int32_t dtype, const void* q, const void* k, const void* qkv, void* ctx,
                               const int32_t* lens, int32_t B, int32_t L, int32_t H, void* stream);

/* Fused residual add + LayerNorm (csrc/norm.hip): v = (x + delta) + delta2 (16-bit [M,D] each, either may be NULL); x = v
 * when write_x; y [M,D] = LayerNorm(v) * w (+ b), eps 1e-5.  dtype 0: bf16 delta / y (namespace ed), 1: f16 (ed16).
 * M > 0, D % 256 == 0, 0 < D <= 2048. */
int esmdiff_add_layernorm(int32_t dtype, float* x, const void* delta, const void* delta2, int32_t write_x, const float* w,
                          const float* b, void* y, int32_t M, int32_t D, void* stream);

/* Block 0's geometric attention alone (csrc/geom.hip): P [B*L, 15*VH] (proj output) + frames rot f32 [B*L, 9], trans f32
 * [B*L, 3], has_frame u8 [B*L] -> out [B*L, 3*VH].  dtype 0: P / out bf16, 1: f16, 2: f32 (the strict path's build).
 * rotation_scale / distance_scale [VH] [host] are the RAW per-head parameters; softplus is applied as at engine create.
 * 0 < L <= 3200 (the kernel's LDS request).  Synchronous. */
int esmdiff_geom_attention(const void* P, int32_t dtype, const float* rot, const float* trans, const uint8_t* has_frame,
                           const float* rotation_scale, const float* distance_scale, void* out, int32_t B, int32_t L,
                           int32_t VH, void* stream);

/* ---- The ends of the structure decoder, one kernel at a time (tests/test_gpu_decoder_ends.py).  All synchronous; every argument
 * is checked before anything is launched (ESMDIFF_E_INVALID). ----
 *   esmdiff_dim6_to_backbone  v f32 [M, ld] (columns 0..8 read: trans 3 | x 3 | y 3; ld >= 9) -> out f32 [M, 3, 3] = N, CA, C:
 *                             csrc/embed.hip, the tail of esm's Dim6RotStructureHead
 *   esmdiff_plddt_mean        v f32 [M, ld] (n_bins logits per row, ld >= n_bins) -> out f32 [M] = sum softmax(v) (i + 0.5) / n_bins
 *   esmdiff_pair_features     qk [nb*L, 128] = [q 64 | k 64] -> X [nb*L*L, 128], row (b, i, j) = [q_j * k_i | q_j - k_i].
 *                             dtype 0: bf16, 2: f32 (the pairwise head has no f16 build: 1 is refused)
 *   esmdiff_pae_tm            logits f32 [nb*L*L, 64] PAE-bin logits, tokens i64 [nb, L] (ids >= 4096 are special: masked out)
 *                             -> tm_rows f32 [nb, L], pae f32 [nb, L, L] (or NULL), ptm f32 [nb] = max over rows (csrc/pairwise.hip)
 *   esmdiff_decoder_set_pair_chunk_bytes   bytes of pair rows that one chunk of whole samples of esmdiff_decoder_decode's pairwise
 *                             head may occupy (768 B per pair row in bf16, 1280 B in f32); 0 restores the default (1.5 GB).
 *                             Decoder engines only; not synchronous (it launches nothing). */
int esmdiff_dim6_to_backbone(const float* v, int32_t ld, float* out, int32_t M, float trans_scale, void* stream);
int esmdiff_plddt_mean(const float* v, int32_t ld, int32_t n_bins, float* out, int32_t M, void* stream);
int esmdiff_pair_features(const void* qk, int32_t dtype, void* X, int32_t nb, int32_t L, void* stream);
int esmdiff_pae_tm(const float* logits, const int64_t* tokens, float* tm_rows, float* pae, float* ptm, int32_t nb, int32_t L,
                   float max_bin, void* stream);
int esmdiff_decoder_set_pair_chunk_bytes(esmdiff_engine* eng, int64_t bytes);

/* ---- The structure encoder's glue kernels (csrc/encoder.hip), launched as esmdiff_encoder_encode launches them.  Synchronous;
 * errors are read with esmdiff_encoder_last_error(NULL). ----
 *   esmdiff_encoder_knn           ca f32 [B, L, 3], has u8 [B, L] -> edges i32 [B, L, K], K = min(knn, L), L <= 8192: the K nearest
 *                                 residues by CA distance (sequence distance * 100 + 1e6 where either residue is unknown),
 *                                 nearest first, lowest index first among equal keys
 *   esmdiff_encoder_neighbourhood edges i32 [B, L, K] (each in 0 .. L-1: checked on the host), table f32 [2 bins + 2, D], frames
 *                                 rot f32 [B*L, 9], trans f32 [B*L, 3], has u8 [B*L] -> x f32 [B*L*K, D] = table[clamp(edge -
 *                                 edge_0, +-bins) + bins + 1], nrot [B*L*K, 9], ntrans [B*L*K, 3], nmask u8 [B*L*K]: the
 *                                 neighbours' frames.  D % 4 == 0
 *   esmdiff_encoder_nearest_code  z f32 [R, d_out], code f32 [n_codes, d_out], has u8 [R] -> tok i64 [R] = the code nearest in
 *                                 squared distance, lowest index among equals; 4096 where has == 0.  d_out <= 8192 */
int esmdiff_encoder_knn(const float* ca, const uint8_t* has, int32_t B, int32_t L, int32_t knn, int32_t* edges, void* stream);
int esmdiff_encoder_neighbourhood(const int32_t* edges, const float* table, const float* rot, const float* trans, const uint8_t* has,
                                  int32_t B, int32_t L, int32_t K, int32_t D, int32_t bins, float* x, float* nrot, float* ntrans,
                                  uint8_t* nmask, void* stream);
int esmdiff_encoder_nearest_code(const float* z, const float* code, const uint8_t* has, int32_t R, int32_t n_codes, int32_t d_out,
                                 int64_t* tok, void* stream);

/* ---- The float32-grade row kernels between the GEMMs of F32 and F32_SPLIT engines (csrc/strict.hip, csrc/gemm_split.hip,
 * csrc/attention_split.hip), one launcher at a time (tests/test_gpu_f32_rows.py).  Enqueued on `stream` without a wait, like the
 * engine's own entries (esmdiff_attention_f32_parts waits for `stream` when lens is given, for its host array); every argument is
 * checked before the first HIP call (ESMDIFF_E_INVALID).  f16 buffers are IEEE half bits. ----
 *   esmdiff_layernorm_f32rows  LayerNorm of x f32 [M, D] * w (+ b), eps 1e-5; D % 4 == 0, D <= 2048.
 *                              split 0 (launch_layernorm_f32): y32 f32 [M, D]; gelu_in 0, delta, a3 and rs NULL.
 *                              split 1 (launch_layernorm_split): LayerNorm of gelu(x) when gelu_in, of x + delta when delta
 *                              ([M, D], delta_dtype 0 bf16 / 1 f16) -> a3 f16 [M, 3D] = [hi | lo | hi] of the row scaled by a
 *                              power of two, rs f32 [M] = 1 / scale, and the f32 row into y32 when non-NULL
 *   esmdiff_swiglu_f32         gu f32 [M, 2 FH] = [gate | up] -> mid f32 [M, FH] = silu(gate) * up; FH % 4 == 0
 *   esmdiff_qk_norm_rope_f32   qkv f32 [B*L, 3*H*64] -> full-width LayerNorm of q and k (no bias) + rotary with the engine's tables
 *                              (H 1 .. 32 explicit, as esmdiff_qk_norm_rope; any ESM3 engine).  split 0: q, k f32 [B*L, H*64],
 *                              unscaled (q_scale, k_scale ignored).  split 1: q, k f16 [B*L, 2*H*64] = [hi | lo] of the rotated
 *                              row * q_scale / k_scale (finite, > 0; the caller folds log2(e)/8 into q_scale, as the engine does)
 *   esmdiff_v_split            qkv f32 [M, 3D] -> v2 f16 [M, 2D] = [hi | lo] of the V third * scale; D % 4 == 0
 *   esmdiff_attention_f32_parts  softmax(q k^T / 8) v per 64-wide head -> ctx f32 [B*L, H*64], operands as the kernel takes them.
 *                              split 0 (attention_f32_kernel): q, k f32 [B*L, H*64], v = the qkv buffer f32 [B*L, 3*H*64] (its V third
 *                              is read).  split 1 (attention_split_kernel): q, k, v f16 [B*L, 2*H*64] = [hi | lo] of q * log2(e)/8 *
 *                              q_scale, k * k_scale, v * v_scale; qk_scale_product = q_scale * k_scale.  lens: HOST int32 [B],
 *                              each in 1..L, or NULL (as esmdiff_attention_ragged)
 *   esmdiff_gemm_split_k       launch_gemm256w4_splitk + launch_splitk_reduce_resid: parts f32 [S, M rounded up to 256, N]
 *                              (caller-owned) = the S K-slice products of a3 [M, 3K] . w3 [N, 3K]^T * w_inv_scale, then
 *                              x f32 [M, N] = x + ((parts[0] + parts[1]) + ...) * rs[m] / div.  S >= 2, N % 256 == 0, 3K / S a
 *                              multiple of 128 and at least 384.  Rows M .. of each plane are written with unspecified values
 *                              (products of the last row, which the operand loads clamp to) and never read; nothing outside
 *                              [S, M rounded up to 256, N] is written
 *   esmdiff_get_attention_scales  the power-of-two operand scales layer `layer` of an F32_SPLIT engine chose at create */
int esmdiff_layernorm_f32rows(const float* x, const float* w, const float* b, int32_t split, int32_t gelu_in, const void* delta,
                              int32_t delta_dtype, void* a3, float* rs, float* y32, int32_t M, int32_t D, void* stream);
int esmdiff_swiglu_f32(const float* gu, float* mid, int32_t M, int32_t FH, void* stream);
int esmdiff_qk_norm_rope_f32(esmdiff_engine* eng, const float* qkv, const float* q_ln_w, const float* k_ln_w, int32_t split,
                             float q_scale, float k_scale, void* q, void* k, int32_t B, int32_t L, int32_t H, void* stream);
int esmdiff_v_split(const float* qkv, void* v2, int32_t M, int32_t D, float scale, void* stream);
int esmdiff_attention_f32_parts(const void* q, const void* k, const void* v, int32_t split, float qk_scale_product, float v_scale,
                                float* ctx, const int32_t* lens, int32_t B, int32_t L, int32_t H, void* stream);
int esmdiff_gemm_split_k(const void* a3, const float* rs, const void* w3, float w_inv_scale, float* parts, float* x, int32_t M,
                         int32_t N, int32_t K, int32_t S, float div, void* stream);
int esmdiff_get_attention_scales(esmdiff_engine* eng, int32_t layer, float* qk_out, float* v_out);

/* ---- Weight conversion at create (csrc/convert.hip, csrc/gemm_split.hip, csrc/attention_split.hip: what every create's loader,
 * csrc/engine_weights.hip, runs on each tensor of the state dict) and the input stage (csrc/embed.hip, csrc/norm.hip), one launcher
 * at a time (tests/test_gpu_loader.py).  Enqueued on `stream` without a wait, except esmdiff_split_weight_from and
 * esmdiff_weight_rownorm_max, which take no stream and are synchronous; every argument is checked before the first HIP call
 * (ESMDIFF_E_INVALID, nothing touched).  src_dtype: esmdiff_dtype of the source tensor (ESMDIFF_F32 / ESMDIFF_BF16). ----
 *   esmdiff_convert_weight      src [n] -> dst [n].  dst_kind 0: bfloat16, round to nearest even (ed::launch_to_bf16); 1: IEEE half,
 *                               saturating at +-65504, NaN stays NaN (ed16::launch_to_bf16); 2: float32, exact (launch_to_f32)
 *   esmdiff_interleave_swiglu   src [2H, K] (gate rows 0..H-1, up rows H..2H-1) -> dst [2H, K] of dst_kind 0 / 1 as above, rows in
 *                               blocks of 32: [gate 32t..32t+31 | up 32t..32t+31]; H % 32 == 0
 *   esmdiff_split_weight_from   esmdiff_split_weight from either source dtype, with the FFN-up row interleave: interleave_h = 0, or
 *                               interleave_h % 32 == 0 and N == 2 interleave_h (rows permuted as esmdiff_interleave_swiglu permutes)
 *   esmdiff_weight_rownorm_max  *out [host] = the largest L2 norm among rows r0 .. r0 + rows - 1 of src [*, K]
 *   esmdiff_embed_rows          out f32 [B*L, D] = ((e_seq[s] + e_struct[t']) + cvec) + cond[(row / L) * cond_stride ..]: seq, xtok i64
 *                               [B*L]; s = seq clamped to 0..63; t' = xtok with -1 -> MASK, clamped to 0..4100, then BOS / PAD / EOS /
 *                               chainbreak where s is 0 / 1 / 2 / 31; e_seq f32 [64, D], e_struct f32 [4101, D], cvec f32 [D]; cond f32 or
 *                               NULL, cond_stride >= 0 a multiple of 4 (0: one vector for every sample); D % 4 == 0
 *   esmdiff_gather_table_rows   out f32 [M, D] = table[tok clamped to 0 .. n_rows-1]; tok i64 [M]; D % 4 == 0
 *   esmdiff_sigma_mlp           hidden f32 [n_sigma, D] = silu(w1 [D, F] . t_freq [n_sigma, F] + b1), cond f32 [n_sigma, D] =
 *                               w2 [D, D] . hidden + b2, float32
 *   esmdiff_layernorm_16in      y16 [M, D] = LayerNorm(x16 [M, D]) * w (+ b; may be NULL), eps 1e-5: launch_layernorm_bf16_in.
 *                               dtype 0: bf16 in and out (namespace ed), 1: f16 (ed16).  D % 4 == 0, D <= 2048 */
int esmdiff_convert_weight(const void* src, int32_t src_dtype, void* dst, int32_t dst_kind, int64_t n, void* stream);
int esmdiff_interleave_swiglu(const void* src, int32_t src_dtype, void* dst, int32_t dst_kind, int32_t H, int32_t K, void* stream);
int esmdiff_split_weight_from(const void* src, int32_t src_dtype, void* w3, int32_t N, int32_t N_pad, int32_t K, int32_t interleave_h,
                              float* inv_scale_out);
int esmdiff_weight_rownorm_max(const void* src, int32_t src_dtype, int64_t r0, int32_t rows, int32_t K, float* out);
int esmdiff_embed_rows(const int64_t* seq, const int64_t* xtok, const float* e_seq, const float* e_struct, const float* cvec,
                       const float* cond, int32_t cond_stride, float* out, int32_t B, int32_t L, int32_t D, void* stream);
int esmdiff_gather_table_rows(const int64_t* tok, const float* table, float* out, int32_t M, int32_t D, int32_t n_rows, void* stream);
int esmdiff_sigma_mlp(const float* t_freq, const float* w1, const float* b1, const float* w2, const float* b2, float* hidden,
                      float* cond, int32_t F, int32_t D, int32_t n_sigma, void* stream);
int esmdiff_layernorm_16in(int32_t dtype, const void* x16, const float* w, const float* b, void* y16, int32_t M, int32_t D,
                           void* stream);

/* ---- Needed rows (ESMDIFF_OPT_NEEDED_ROWS,esmdiff_ddpm_sample in esmdiff_hip.h), one forward at a time ----
 *   esmdiff_forward_logits_needed  esmdiff_forward_logits as a forward of esmdiff_ddpm_sample runs it: the rows to keep are
 *                                  derived from x (those that hold MASK), and logits_out is written on those rows only — every
 *                                  other row of logits_out is left as it was.  Bit-identical to esmdiff_forward_logits on the rows
 *                                  written.  Engines and batches the option does not reach run the full forward and still
 *                                  write the MASK rows only.  One host wait, like a forward of esmdiff_ddpm_sample.
 *   esmdiff_get_tail_rows          *rows_out = the token rows that ran the last block's branches and the head, summed over the
 *                                  forwards since create / the last reset: equal to esmdiff_get_counters' token_rows when nothing
 *                                  was skipped. */
int esmdiff_forward_logits_needed(esmdiff_engine* eng, const int64_t* seq, const int64_t* x, const float* t_freq,
                                  float* logits_out, int32_t ld_logits, int32_t B, int32_t L, void* stream);
int esmdiff_get_tail_rows(esmdiff_engine* eng, int64_t* rows_out, int32_t reset);

/* ---- The needed-rows and sub-batch bookkeeping kernels (csrc/sampler.hip, csrc/norm.hip), one launcher at a time
 * (tests/test_gpu_row_bookkeeping.py against tests/needed_rows_ref.py).  No engine; enqueued on `stream` without a wait; every
 * argument is checked before the first HIP call (ESMDIFF_E_INVALID, nothing touched).  MASK = ESMDIFF_MASK_ID. ----
 *   esmdiff_mask_row_list       x i64 [B, L] cut into np parts (part pi = samples [B pi / np, B (pi + 1) / np), first row t0, `rows`
 *                               rows): list i32 [t0 + i] = the i-th row of the part that holds MASK, relative to t0, ascending;
 *                               map i32 [t0 + r] = t0 + (count * 8 <= rows * 7 ? i : r) on those rows; count i32 [np] (device memory
 *                               here; the engine hands pinned host memory).  Every other entry of list and map is left as it was.
 *                               1 <= np <= B, B * L < 2^31
 *   esmdiff_gather_rows16       dst [i, :] = src [list[i], :], n rows of D 16-bit values; D % 8 == 0
 *   esmdiff_add_layernorm_rows  the fused add + LayerNorm on M compact rows: v = (x [rows[i]] + delta [rows[i]]) + delta2 [i]
 *                               (x f32 and delta 16-bit of the full batch, delta2 16-bit [M, D]; either delta may be NULL),
 *                               x_out f32 [i] = v, y [i] = LayerNorm(v) * w (+ b), eps 1e-5; x is only read.  dtype 0: bf16, 1: f16.
 *                               D % 256 == 0, 0 < D <= 2048
 *   esmdiff_copy_masked_logits  out [row, 0 .. V) = logits [map ? map[row] : row, 0 .. V) on the rows of x i64 [rows] that hold MASK
 *                               (row strides ld / ld_out >= V); nothing else of out is written
 *   esmdiff_ddpm_step_mapped    the update of esmdiff_ddpm_step with Philox noise, reading the logits of row r at row
 *                               row_map[p] of `logits`, p = ((r / L) % logits_period) * L + r % L when logits_period > 0, else r
 *                               (row_map NULL: row p itself).  V <= 5120; rng may be NULL on a final pass
 *   esmdiff_move_token_rows     gather 1: dst [i, :] = src [idx[i], :]; gather 0: dst [idx[i], :] = src [i, :]; n rows of L int64.
 *                               n = 0 does nothing
 *   esmdiff_samples_with_mask   has i32 [b] = 1 if row b of x i64 [B, L] holds a MASK, else 0
 *   esmdiff_rows_identical      flag i32 [1] = non-zero if every row of seq and of x (i64 [B, L] each) equals its row 0, else 0 */
int esmdiff_mask_row_list(const int64_t* x, int32_t B, int32_t L, int32_t np, int32_t* list, int32_t* map, int32_t* count,
                          void* stream);
int esmdiff_gather_rows16(const void* src, const int32_t* list, void* dst, int32_t n, int32_t D, void* stream);
int esmdiff_add_layernorm_rows(int32_t dtype, const float* x, const void* delta, const int32_t* rows, const void* delta2,
                               float* x_out, const float* w, const float* b, void* y, int32_t M, int32_t D, void* stream);
int esmdiff_copy_masked_logits(const int64_t* x, const float* logits, int32_t ld, const int32_t* map, float* out, int32_t ld_out,
                               int32_t V, int32_t rows, void* stream);
int esmdiff_ddpm_step_mapped(int64_t* x, const float* logits, int32_t ld, int32_t V, float mc_t, float mc_s, int32_t final_,
                             const esmdiff_rng* rng, int32_t step, int32_t B, int32_t L, int32_t logits_period,
                             const int32_t* row_map, void* stream);
int esmdiff_move_token_rows(const int64_t* src, int64_t* dst, const int32_t* idx, int32_t n, int32_t L, int32_t gather,
                            void* stream);
int esmdiff_samples_with_mask(const int64_t* x, int32_t B, int32_t L, int32_t* has, void* stream);
int esmdiff_rows_identical(const int64_t* seq, const int64_t* x, int32_t B, int32_t L, int32_t* flag, void* stream);

/* ---- The shared math of csrc/ed_math.h as ONE unit compiled it (tests/test_gpu_shared_math.py against the C oracle and float64).
 * sampler.hip, score.hip and gibbs.hip each inline their own copy of that header under the unit's own flags, and every bit-exact
 * test of those units rests on each copy giving the host's bits.  The kernel body is csrc/ed_math_eval.inc, instantiated inside each
 * of the three units.  No engine; enqueued on `stream` without a wait; every argument is checked before the first HIP call
 * (ESMDIFF_E_INVALID, nothing touched).  (An addition; the ABI number stays.)
 *   unit  0: sampler.hip, 1: score.hip, 2: gibbs.hip
 *   kind  0: out f32 [n] = ed_expf of in f32 [n]          1: ed_logf, likewise
 *         2: 1e-10f - ed_logf(in + 1e-10f), the noise of the race as the three kernels write it
 *         3: ed_philox_uniform of in = n records of 32 bytes, esmdiff_math_eval_philox -> out f32 [n]
 *   n >= 0 (0 launches nothing); in and out do not overlap. */
typedef struct {
  uint64_t seed;
  uint64_t sample;
  uint32_t step;
  uint32_t l;
  uint32_t v;
  uint32_t reserved;   /* the C layout's tail padding, named: not read */
} esmdiff_math_eval_philox;
int esmdiff_math_eval(int32_t unit, int32_t kind, const void* in, void* out, int64_t n, void* stream);

/* Accumulated per-section device time of the esmdiff_forward_logits/ddpm_sample calls since profiling was
 * enabled: esmdiff_set_profiling(eng, 1) brackets every launch with HIP events on the launch stream (no sync);
 * mode 2 brackets only the dominant kernel (FFN-up GEMM, section 6), cheap enough for a timed region; 0 = off. sections: 0 embed, 1 layernorm, 2 gemm_qkv,
 * 3 qk_norm_rope, 4 attention, 5 gemm_out, 6 gemm_ffn_up, 7 gemm_ffn_down, 8 head, 9 sampler.
 * ms_out: [16] floats, launches_out: [16] ints [host].  Synchronises the device. */
int esmdiff_set_profiling(esmdiff_engine* eng, int32_t on);
int esmdiff_get_profile(esmdiff_engine* eng, float* ms_out, int32_t* launches_out);

#ifdef ED_DEBUG
/* ---- measurement aid: exported only by libraries built with -DED_DEBUG (ESMDIFF_EXTRA_CXXFLAGS=-DED_DEBUG python -m
 * esmdiff_amd.build).  That flag switches nothing else: no build reads an ESMDIFF_* tuning variable.  Used by
 * scratch/bench_gemm.py only. ---- */
/* Runs the GEMM `iters` times on `stream` bracketed by
 * HIP events on that stream and returns the average milliseconds per launch in *ms_out [host]. */
int esmdiff_gemm_bf16_timed(const void* A, const void* W, void* out, const float* bias, int32_t M,
                            int32_t N, int32_t K, int32_t ldc, int32_t n_valid, float alpha,
                            int32_t epilogue, int32_t iters, float* ms_out, void* stream);
#endif /* ED_DEBUG */

#ifdef __cplusplus
}
#endif
#endif /* ESMDIFF_HIP_TEST_H */

// kernels_ns.inc — the launch functions of one operand-type build of the kernels; included by kernels.h (namespace ed) and,
// in engine.h, a second time with `#define ed ed16` for the f16 build of the same sources (ed_half.h).  No include guard.
namespace ed {

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) applies to the CURRENT device only: once per (kernel, device), thread-safe,
// return code checked (ADVICE r03: a `static bool once` left a second device's launches without the attribute).
inline hipError_t ensure_dynamic_lds(const void* fn, int bytes) {
  static std::mutex mu;
  static std::map<std::pair<const void*, int>, int> done;
  int dev = 0;
  hipError_t s = hipGetDevice(&dev);
  if (s != hipSuccess) return s;
  std::lock_guard<std::mutex> g(mu);
  auto it = done.find({fn, dev});
  if (it != done.end() && it->second >= bytes) return hipSuccess;
  s = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (s == hipSuccess) done[{fn, dev}] = bytes;
  return s;
}

// ---- sampler.hip -----------------------------------------------------------------------------
hipError_t launch_ddpm_step(int64_t* x, const float* logits, int ld, int V, float mc_t, float mc_s, int final_,
                            const float* u, int use_philox, uint64_t seed, uint64_t sample_offset, int step,
                            int B, int L, hipStream_t stream, int logits_period = 0, float margin = 0.f,
                            int32_t* sample_flags = nullptr);
// the same update with one parameter set per sample (esmdiff_ddpm_step_rows); flags / gap may be null
hipError_t launch_ddpm_step_rows(int64_t* x, const float* logits, int ld, int V, const esmdiff_sample_step* sp, uint64_t seed,
                                 int B, int L, float margin_ratio, float margin_diff, int32_t* sample_flags, float* sample_gap,
                                 hipStream_t stream);
// out[row, 8] = { max |e|, sum e^2, max |d|, sum d^2, max e - min e, H(a) - H(b), H(b), 0 }, e = a - b over the masked rows' columns
// (all but the MASK column, or all of them) (esmdiff_logit_error_stats)
hipError_t launch_logit_error_stats(const float* a, int lda, const float* b, int ldb, const int64_t* x, int rows, int V, int all_columns,
                                    float* out, hipStream_t stream);
// has[b] = 1 if sample b of x [B, L] still holds a MASK token
hipError_t launch_samples_with_mask(const int64_t* x, int B, int L, int32_t* has, hipStream_t stream);
// gather (dst[i] = src[idx[i]]) or scatter (dst[idx[i]] = src[i]) of n token rows of L int64
hipError_t launch_move_token_rows(const int64_t* src, int64_t* dst, const int32_t* idx, int n, int L, int gather, hipStream_t stream);
// flag[0] (device int32) = -1 if every row of seq and x [B, L] equals row 0, else 0
hipError_t launch_rows_identical(const int64_t* seq, const int64_t* x, int B, int L, int32_t* flag, hipStream_t stream);

// ---- score.hip -----------------------------------------------------------------------------
// xt = (u < move_chance[b] and not non_moving and l < lens[b]) ? MASK : x0, and seq_out likewise with the sequence MASK when not
// null; u: explicit uniforms [B,L], or null for Philox(seed, sample_index[b], draw[b], l, ESMDIFF_QXT_PHILOX_COLUMN)
hipError_t launch_q_xt(const int64_t* x0, const int64_t* seq, const float* move_chance, const uint8_t* non_moving, const float* u,
                       uint64_t seed, const uint64_t* sample_index, const int32_t* draw, const int32_t* lens, int64_t* xt,
                       int64_t* seq_out, int B, int L, hipStream_t stream);
// log_p (may be null) and row_loss [B,L] of the re-parameterised logits gathered at x0, then the per-sample masked sums in a
// fixed order (esmdiff_nelbo_rows); loss_mask / lens may be null
hipError_t launch_nelbo_rows(const float* logits, int ld, int V, const int64_t* xt, const int64_t* x0, const float* weight,
                             const uint8_t* loss_mask, const int32_t* lens, float* log_p, float* row_loss, float* sample_sum,
                             int32_t* sample_count, int B, int L, hipStream_t stream);

// ---- gibbs.hip ---------------------------------------------------------------------------------
// one entropy-ordered unmasking step: per masked row nucleus(top_p) + temperature draw + entropy, then per prompt
// the n_unmask[b] lowest-entropy masked positions take their token.  u: [B,L,4096] explicit uniforms or null.
hipError_t launch_gibbs_step(int64_t* x, const int64_t* seq, const float* logits, int ld, int vocab, float temperature,
                             float top_p, const int32_t* n_unmask, const float* u, int use_philox, uint64_t seed,
                             uint64_t sample_offset, int step, int32_t* sampled, float* entropy, int B, int L,
                             hipStream_t stream, int logits_period = 0, int strategy = 0, const uint32_t* inv_mask = nullptr);
// the same step with one parameter set per prompt; pair_bound >= 0: also the certified sampler's per-prompt report
hipError_t launch_gibbs_step_rows(int64_t* x, const int64_t* seq, const float* logits, int ld, int vocab, float temperature,
                                  float top_p, const esmdiff_gibbs_sample_step* sp, uint64_t seed, int32_t* sampled, float* entropy,
                                  int B, int L, float pair_bound, float entropy_bound, uint8_t* row_flag, float* row_gap,
                                  int32_t* sample_flags, float* sample_gaps, hipStream_t stream, int strategy = 0,
                                  const uint32_t* inv_mask = nullptr);

// ---- gemm.hip --------------------------------------------------------------------------------
// out = epilogue(A[M,K] · W[N,K]^T); K % 64 == 0, N % 128 == 0 (weights are padded at load time).
// ws (optional): split-K workspace for the small-M path — room for f32 partial tiles, owned by ONE launch queue
// (concurrent launches need their own).  Without it every tile runs its whole K range.
// n_valid is informative only: neither kernel reads it.  ESMDIFF_EPI_BIAS_F32 skips a 4-column group only when it would cross
// ldc; columns n_valid .. ldc-1 are written from the (zero-padded) weight rows and the bias, so the caller allocates ldc for them.
using GemmWorkspace = ::EdGemmWorkspace;   // (one type for both operand-type builds, kernels.h)
hipError_t launch_gemm_bf16(const bf16_t* A, const bf16_t* W, void* out, const float* bias, int M, int N,
                            int K, int ldc, int n_valid, float alpha, int epilogue, hipStream_t stream,
                            const GemmWorkspace* ws = nullptr);

// the kernel launch_gemm_bf16 would pick for (M, N, K), as text
void describe_gemm(int M, int N, int K, size_t ws_floats, char* out, size_t cap);
// ... and as numbers: 256x256 kernel or not, rows per tile, K slices, LDS stages (esmdiff_describe_gemm_choice)
void describe_gemm_choice(int M, int N, int K, size_t ws_floats, int* w4, int* rows, int* S, int* stages);

// Row count below which a (sub-)batch takes the small-batch path (DESIGN 3.8).
inline int small_max_rows() {
  return 1152;  // r02: 1 024 -> 1 152 (+4 % at 1 032 - 1 080 rows; 2 048 loses 5 - 20 % from 1 440 rows)
}

// Small-batch path (M < small_max_rows()): the product as S raw f32 K-slice planes in `ws` (plane stride `stride` floats, row stride
// N), consumed by launch_add_partials_layernorm_bf16.  S = gemm_partial_splits(N, K), a function of the shape only.
using GemmPartials = ::EdGemmPartials;
int gemm_partial_splits(int N, int K);
hipError_t launch_gemm_partials(const bf16_t* A, const bf16_t* W, const GemmWorkspace* ws, int M, int N, int K,
                                hipStream_t stream, GemmPartials* res);

// gemm256w4.hip: the same tile with 4 waves x 128x128 wave tiles, hand-placed v_mfma_f32_16x16x32 main loop, accumulators in
// AGPRs; K % 128 == 0
hipError_t launch_gemm256w4_bf16(const bf16_t* A, const bf16_t* W, void* out, const float* bias, int M, int N,
                                 int K, int ldc, float alpha, int epilogue, hipStream_t stream);

// ---- norm.hip --------------------------------------------------------------------------------
hipError_t launch_layernorm_bf16(const float* x, const float* w, const float* b, bf16_t* y, int M, int D,
                                 hipStream_t stream);
// v = (x + delta) + delta2 (bf16 or null each); x = v if write_x; y = LayerNorm(v) * w (+ b)
hipError_t launch_add_layernorm_bf16(float* x, const bf16_t* delta, const bf16_t* delta2, int write_x, const float* w,
                                     const float* b, bf16_t* y, int M, int D, hipStream_t stream);
// x += alpha * (P[0] + P[1] + ... + P[S-1]) (f32 K-slice planes of a branch linear); x written back;
// y = LayerNorm(x) * w (+ b)
hipError_t launch_add_partials_layernorm_bf16(float* x, const GemmPartials& P, int N, float alpha, const float* w,
                                              const float* b, bf16_t* y, int M, int D, hipStream_t stream);
hipError_t launch_layernorm_bf16_in(const bf16_t* x, const float* w, const float* b, bf16_t* y, int M, int D,
                                    hipStream_t stream);
// qkv bf16 [M,3D] -> q,k bf16 [M,D] token-major (LayerNorm over D, rotary, q pre-scaled); v stays in qkv
hipError_t launch_qk_norm_rope(const bf16_t* qkv, const float* q_ln_w, const float* k_ln_w,
                               const float* rope_cos, const float* rope_sin, bf16_t* q, bf16_t* k,
                               int B, int L, int H, hipStream_t stream);

// ---- attention.hip ---------------------------------------------------------------------------
// q,k [B*L, H*64] token-major, v read in place from qkv [B*L, 3*H*64] (columns 2*H*64 ..) -> ctx bf16 [B*L, H*64].
// lens (device, [B], each in 1..L, or null = all L): sample b is valid on tokens [0, lens[b]); keys beyond are masked and
// its context rows from lens[b] on are written as zeros.
hipError_t launch_attention(const bf16_t* q, const bf16_t* k, const bf16_t* qkv, bf16_t* ctx, int B, int L,
                            int H, hipStream_t stream, const int32_t* lens = nullptr);

// ---- geom.hip --------------------------------------------------------------------------------
// P bf16 [B*L, 15*VH] (proj output) + frames -> out bf16 [B*L, 3*VH]; w_rot / w_dist = softplus(scale) per head
hipError_t launch_geom_attention(const bf16_t* P, const float* rot, const float* trans, const uint8_t* fmask,
                                 const float* w_rot, const float* w_dist, bf16_t* out, int B, int L, int VH,
                                 hipStream_t stream);

hipError_t launch_geom_attention_f32(const float* P, const float* rot, const float* trans, const uint8_t* fmask,
                                     const float* w_rot, const float* w_dist, float* out, int B, int L, int VH,
                                     hipStream_t stream);

// ---- embed.hip -------------------------------------------------------------------------------
// x[b,l,:] = E_seq[seq] + E_struct[struct'] + c + cond   (net.py:445-466)
hipError_t launch_embed(const int64_t* seq, const int64_t* xtok, const float* e_seq, const float* e_struct,
                        const float* cvec, const float* cond, float* out, int B, int L, int D,
                        hipStream_t stream, int cond_stride = 0);
// cond = W2 · silu(W1 · t_freq + b1) + b2   (net.py:489-492,519-522), f32
hipError_t launch_gather_rows(const int64_t* tok, const float* table, float* out, int M, int D, int n_rows,
                              hipStream_t stream);
// v f32 [M, ld] (23 used) -> backbone N/CA/C coordinates f32 [M, 3, 3]
hipError_t launch_dim6_to_backbone(const float* v, int ld, float* out, int M, float trans_scale, hipStream_t stream);
// pairwise.hip: the decoder's pairwise confidence head (pair features; PAE / pTM from the 64 PAE bin logits)
hipError_t launch_pair_features(const bf16_t* qk, bf16_t* X, int nb, int L, hipStream_t stream);
hipError_t launch_pair_features_f32(const float* qk, float* X, int nb, int L, hipStream_t stream);
hipError_t launch_pae_tm(const float* logits, const int64_t* tokens, float* tm_rows, float* pae, float* ptm, int nb, int L,
                         float max_bin, hipStream_t stream);
hipError_t launch_plddt_mean(const float* v, int ld, int n_bins, float* out, int M, hipStream_t stream);
hipError_t launch_sigma_mlp(const float* t_freq, const float* w1, const float* b1, const float* w2,
                            const float* b2, float* hidden, float* cond, int F, int D, hipStream_t stream,
                            int n_sigma = 1);

// ---- strict.hip: the float32 precision path (esmdiff_config.precision = ESMDIFF_PRECISION_F32) -----------------
hipError_t launch_gemm_f32(const float* A, int lda, const float* W, float* out, const float* bias, int M, int n_rows, int K,
                           int ldc, int n_valid, float div, int epi, hipStream_t stream);
hipError_t launch_layernorm_f32(const float* x, const float* w, const float* b, float* y, int M, int D, hipStream_t stream);
hipError_t launch_swiglu_f32(const float* gu, float* mid, int M, int FH, hipStream_t stream);
hipError_t launch_qk_norm_rope_f32(const float* qkv, const float* q_ln_w, const float* k_ln_w, const float* rope_cos,
                                   const float* rope_sin, float* q, float* k, int B, int L, int H, hipStream_t stream);
hipError_t launch_attention_f32(const float* q, const float* k, const float* qkv, float* ctx, int B, int L, int H,
                                hipStream_t stream, const int32_t* lens = nullptr);   // lens: as launch_attention's

// ---- gemm_split.hip + gemm256w4_split.hip: float32-grade linears as three f16 MFMA passes over split operands ----
// (gemm256w4_split.hip is compiled once, into namespace ed; the ed16 view of this header declares its launchers without a definition)
// A3 f16 [M, 3K] = [hi | lo | hi] scaled per row (rs[M] = 1 / row scale), W3 f16 [N_pad, 3K] = [lo | hi | hi] scaled per
// matrix (w_inv_scale = 1 / scale); out f32 [M, ldc] = epi(rs[m] * w_inv_scale * A . W^T); N % 256 == 0, K % 128 == 0,
// ldc >= N (no column bound in the kernel); epi: ESMDIFF_F32EPI_STORE (+ bias[N] when non-null) or ESMDIFF_F32EPI_RESID_DIV.
hipError_t launch_gemm256w4_split(const uint16_t* A2, const float* rs, const uint16_t* W2, float w_inv_scale, float* out,
                                  const float* bias, int M, int N, int K, int ldc, float div, int epi, hipStream_t stream);
// K-sliced form for launches with few tiles (S slices as extra row blocks; gemm256w4_split.hip) and the pass that sums the slices
// in order, applies the row scales and adds the result into the residual stream: x = x + (sum_s parts[s]) * rs[m] / div
hipError_t launch_gemm256w4_splitk(const uint16_t* A2, const uint16_t* W2, float w_scale, float* parts, int M, int N, int K,
                                   int S, hipStream_t stream);
hipError_t launch_splitk_reduce_resid(const float* parts, const float* rs, float* x, int M, int N, int S, float div,
                                      hipStream_t stream);
hipError_t launch_split_rows(const float* src, int ld, uint16_t* dst, float* rs, int M, int K, hipStream_t stream);
// LayerNorm (of gelu(x) when gelu_in; of x + delta when delta, a bf16 — or f16 — [M, D] branch output, is non-null) in the strict path's
// arithmetic -> split row (+ the f32 row into y32 when non-null)
hipError_t launch_layernorm_split(const float* x, const float* w, const float* b, uint16_t* dst, float* rs, float* y32,
                                  int M, int D, int gelu_in, hipStream_t stream, const uint16_t* delta = nullptr,
                                  int delta_is_f16 = 0);
// create time, synchronous: dst [rows_pad, 3K] (caller zero-fills the padding rows); scratch_bits: 4 device bytes
hipError_t split_weight(const void* src, int src_dtype, uint16_t* dst, int64_t rows, int K, uint32_t* scratch_bits,
                        float* inv_scale_out, int interleave_h = 0);

// ---- attention_split.hip: float32-grade attention on the f16 MFMA (three products per split operand pair) -----------------
// q2 / k2 / v2: [B L, 2 D] f16 rows = [hi(D) | lo(D)] of x * scale (power-of-two scales chosen per layer at create); q is also
// pre-multiplied by log2(e) / 8 (q_scale carries that factor, qk_scale_product does not); ctx f32 [B L, D]
hipError_t launch_qk_norm_rope_split(const float* qkv, const float* q_ln_w, const float* k_ln_w, const float* rope_cos,
                                     const float* rope_sin, uint16_t* q2, uint16_t* k2, int B, int L, int H, float q_scale,
                                     float k_scale, hipStream_t stream);
hipError_t launch_v_split(const float* qkv, uint16_t* v2, int M, int D, float scale, hipStream_t stream);
hipError_t launch_attention_split(const uint16_t* q2, const uint16_t* k2, const uint16_t* v2, float* ctx, int B, int L, int H,
                                  float qk_scale_product, float v_scale, hipStream_t stream,
                                  const int32_t* lens = nullptr);   // lens: as launch_attention's
hipError_t weight_rownorm_max(const void* src, int src_dtype, int64_t r0, int rows, int K, uint32_t* scratch_bits, float* out);

// ---- convert.hip (weight preparation at engine create) ---------------------------------------
hipError_t launch_to_bf16(const void* src, int src_dtype, bf16_t* dst, int64_t n, hipStream_t stream);
hipError_t launch_to_f32(const void* src, int src_dtype, float* dst, int64_t n, hipStream_t stream);
// dst rows: blocks of 32: [gate 32t..32t+31 | up 32t..32t+31]; src [2H, K]: gate rows 0..H-1, up rows H..2H-1
hipError_t launch_interleave_swiglu(const void* src, int src_dtype, bf16_t* dst, int H, int K,
                                    hipStream_t stream);

}  // namespace ed

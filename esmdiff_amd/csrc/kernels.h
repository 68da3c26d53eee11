// kernels.h — internal launch functions of libesmdiff_hip.so (gfx950 only).
// Every launch function enqueues on `stream` and returns the hipError_t of the launch; finish_entry below is the one that waits.
// Declared here, once: what exists in one build only.  The launchers of F16_UNITS (build.py) are in kernels_typed.inc, included last.
#pragma once
#include <stdlib.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/esmdiff_hip.h"
#include "../../include/esmdiff_hip_test.h"

#include <map>
#include <mutex>
#include <utility>

typedef uint16_t bf16_t;  // raw bfloat16 bits

// Types shared by the two operand-type builds of the kernels (namespace ed = bf16, ed16 = f16, see ed_half.h).
struct EdGemmWorkspace {
  float* partial;
  size_t partial_floats;
};
struct EdGemmPartials {
  const float* p;
  int S;
  int64_t stride;
};

// The tail of a C entry that returns when its work is done: the last launch's error, then the stream's -> 0 / ESMDIFF_E_HIP.
inline int finish_entry(hipStream_t st) {
  if (hipGetLastError() != hipSuccess) return ESMDIFF_E_HIP;
  return hipStreamSynchronize(st) == hipSuccess ? 0 : ESMDIFF_E_HIP;
}

namespace ed {

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) applies to the CURRENT device only: once per (kernel, device), thread-safe,
// return code checked (a `static bool once` left a second device's launches without the attribute).
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
                            int32_t* sample_flags = nullptr, const int32_t* row_map = nullptr);   // row_map: see launch_mask_row_list
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
// A sub-batch of `rows` rows of which `count` hold MASK runs the last block's branches and the head on those rows only: up to 7/8 of
// the rows.  Above that (step 0: every row) the gathers cost more than the rows they drop.  Asked by the host and by
// mask_row_list_kernel of the same count.
__host__ __device__ inline bool needed_rows_compact(int count, int rows) { return (int64_t)count * 8 <= (int64_t)rows * 7; }
// Per sub-batch of x [B, L] (np of them, cut as the forward cuts them): the ascending list of its rows with x == MASK (relative to
// the sub-batch), their count into pinned host memory, and for every such row the logits row the sampler reads (row_map)
hipError_t launch_mask_row_list(const int64_t* x, int B, int L, int np, int32_t* list, int32_t* map, int32_t* count_host,
                                hipStream_t stream);
// dst[i, :] = src[list[i], :]: n rows of D 16-bit values
hipError_t launch_gather_rows16(const uint16_t* src, const int32_t* list, uint16_t* dst, int n, int D, hipStream_t stream);
// out[row, :V] = logits[map ? map[row] : row, :V] on the rows of x that hold MASK; the others are not written
hipError_t launch_copy_masked_logits(const int64_t* x, const float* logits, int ld, const int32_t* map, float* out, int ld_out,
                                     int V, int rows, hipStream_t stream);

// ---- sampler.hip, score.hip, gibbs.hip: csrc/ed_math_eval.inc, one instance per unit ----
// out f32 [n] = ed_expf / ed_logf / the race's noise of in f32 [n] (kind 0 / 1 / 2), or ed_philox_uniform of n records (kind 3), as
// the unit of the name compiled csrc/ed_math.h
hipError_t launch_math_eval_sampler(int kind, const void* in, float* out, int64_t n, hipStream_t stream);
hipError_t launch_math_eval_score(int kind, const void* in, float* out, int64_t n, hipStream_t stream);
hipError_t launch_math_eval_gibbs(int kind, const void* in, float* out, int64_t n, hipStream_t stream);

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

// ---- embed.hip -------------------------------------------------------------------------------
// x[b,l,:] = E_seq[seq] + E_struct[struct'] + c + cond   (net.py:445-466)
hipError_t launch_embed(const int64_t* seq, const int64_t* xtok, const float* e_seq, const float* e_struct,
                        const float* cvec, const float* cond, float* out, int B, int L, int D,
                        hipStream_t stream, int cond_stride = 0);
hipError_t launch_gather_rows(const int64_t* tok, const float* table, float* out, int M, int D, int n_rows,
                              hipStream_t stream);
// v f32 [M, ld] (23 used) -> backbone N/CA/C coordinates f32 [M, 3, 3]
hipError_t launch_dim6_to_backbone(const float* v, int ld, float* out, int M, float trans_scale, hipStream_t stream);
hipError_t launch_plddt_mean(const float* v, int ld, int n_bins, float* out, int M, hipStream_t stream);
// cond = W2 · silu(W1 · t_freq + b1) + b2   (net.py:489-492,519-522), f32
hipError_t launch_sigma_mlp(const float* t_freq, const float* w1, const float* b1, const float* w2,
                            const float* b2, float* hidden, float* cond, int F, int D, hipStream_t stream,
                            int n_sigma = 1);

// ---- pairwise.hip: the decoder's pairwise confidence head (pair features; PAE / pTM from the 64 PAE bin logits) ----
hipError_t launch_pair_features(const bf16_t* qk, bf16_t* X, int nb, int L, hipStream_t stream);
hipError_t launch_pair_features_f32(const float* qk, float* X, int nb, int L, hipStream_t stream);
hipError_t launch_pae_tm(const float* logits, const int64_t* tokens, float* tm_rows, float* pae, float* ptm, int nb, int L,
                         float max_bin, hipStream_t stream);

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

}  // namespace ed

#include "kernels_typed.inc"

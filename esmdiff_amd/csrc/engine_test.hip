// engine_test.hip — the kernel-level entries of include/esmdiff_hip_test.h: single launchers behind a C signature, for the test
// suite and the measurement tools.  No product path calls them.
#include "engine.h"

using namespace ed;
using namespace eng;

// The result of a test entry's launch: 0, or the launcher's error with hipErrorInvalidValue (a shape it refuses) as the caller's.
static int launched(esmdiff_engine* e, hipError_t s, const char* name) {
  if (s == hipSuccess) return 0;
  return fail(e, s == hipErrorInvalidValue ? ESMDIFF_E_INVALID : ESMDIFF_E_HIP, "%s: %s", name, hipGetErrorString(s));
}

extern "C" {

int esmdiff_gemm_bf16(const void* A, const void* W, void* out, const float* bias, int32_t M, int32_t N, int32_t K,
                      int32_t ldc, int32_t n_valid, float alpha, int32_t epilogue, void* stream) {
  if (!A || !W || !out) return ESMDIFF_E_INVALID;
  hipError_t s = launch_gemm_bf16((const bf16_t*)A, (const bf16_t*)W, out, bias, M, N, K, ldc, n_valid, alpha, epilogue,
                                  (hipStream_t)stream);
  return launched(nullptr, s, "gemm");
}

int esmdiff_gemm_f16(const void* A, const void* W, void* out, const float* bias, int32_t M, int32_t N, int32_t K,
                     int32_t ldc, int32_t n_valid, float alpha, int32_t epilogue, void* stream) {
  if (!A || !W || !out) return ESMDIFF_E_INVALID;
  hipError_t s = ed16::launch_gemm_bf16((const bf16_t*)A, (const bf16_t*)W, out, bias, M, N, K, ldc, n_valid, alpha, epilogue,
                                        (hipStream_t)stream);
  return launched(nullptr, s, "gemm_f16");
}

int esmdiff_gemm_f32(const float* A, int32_t lda, const float* W, float* out, const float* bias, int32_t M, int32_t N,
                     int32_t K, int32_t ldc, int32_t n_valid, float div, int32_t epilogue, void* stream) {
  if (!A || !W || !out) return ESMDIFF_E_INVALID;
  hipError_t s = launch_gemm_f32(A, lda, W, out, bias, M, N, K, ldc, n_valid, div, epilogue, (hipStream_t)stream);
  return launched(nullptr, s, "gemm_f32");
}

int esmdiff_split_rows(const float* src, int32_t ld, void* a2, float* rs, int32_t M, int32_t K, void* stream) {
  if (!src || !a2 || !rs) return ESMDIFF_E_INVALID;
  hipError_t s = launch_split_rows(src, ld, (uint16_t*)a2, rs, M, K, (hipStream_t)stream);
  return launched(nullptr, s, "split_rows");
}

int esmdiff_split_weight_from(const void* src, int32_t src_dtype, void* w3, int32_t N, int32_t N_pad, int32_t K, int32_t interleave_h,
                              float* inv_scale_out) {
  if (!src || !w3 || !inv_scale_out || N <= 0 || N_pad < N || N_pad % 256 || K <= 0 || K % 128) return ESMDIFF_E_INVALID;
  if (src_dtype != ESMDIFF_F32 && src_dtype != ESMDIFF_BF16)
    return fail(nullptr, ESMDIFF_E_INVALID, "split_weight: src_dtype %d (0 f32, 1 bf16)", src_dtype);
  if (interleave_h != 0 && (interleave_h < 0 || interleave_h % 32 || N != 2 * interleave_h))
    return fail(nullptr, ESMDIFF_E_INVALID, "split_weight: interleave_h=%d must be 0, or a multiple of 32 with N (%d) == 2 interleave_h",
                interleave_h, N);
  uint32_t* bits = nullptr;
  if (hipMalloc(&bits, 4) != hipSuccess) return fail(nullptr, ESMDIFF_E_HIP, "split_weight: hipMalloc failed");
  hipError_t s = hipSuccess;
  if (N_pad > N) s = hipMemset((uint16_t*)w3 + (size_t)N * 3 * K, 0, (size_t)(N_pad - N) * 3 * K * 2);
  if (s == hipSuccess) s = split_weight(src, src_dtype, (uint16_t*)w3, N, K, bits, inv_scale_out, interleave_h);
  if (s == hipSuccess) s = hipDeviceSynchronize();
  hipFree(bits);
  if (s != hipSuccess) return fail(nullptr, ESMDIFF_E_HIP, "split_weight: %s", hipGetErrorString(s));
  return 0;
}

int esmdiff_split_weight(const float* src, void* w2, int32_t N, int32_t N_pad, int32_t K, float* inv_scale_out) {
  return esmdiff_split_weight_from(src, ESMDIFF_F32, w2, N, N_pad, K, 0, inv_scale_out);
}

int esmdiff_gemm_split(const void* a2, const float* rs, const void* w2, float w_inv_scale, float* out, const float* bias,
                       int32_t M, int32_t N, int32_t K, int32_t ldc, float div, int32_t epilogue, void* stream) {
  if (!a2 || !w2 || !out) return ESMDIFF_E_INVALID;
  hipError_t s = launch_gemm256w4_split((const uint16_t*)a2, rs, (const uint16_t*)w2, w_inv_scale, out, bias, M, N, K, ldc, div,
                                        epilogue, (hipStream_t)stream);
  return launched(nullptr, s, "gemm_split");
}

int esmdiff_gemm_bf16_ws(esmdiff_engine* e, const void* A, const void* W, void* out, const float* bias, int32_t M,
                         int32_t N, int32_t K, int32_t ldc, int32_t n_valid, float alpha, int32_t epilogue, void* stream) {
  if (!e || !A || !W || !out) return ESMDIFF_E_INVALID;
  hipError_t s = launch_gemm_bf16((const bf16_t*)A, (const bf16_t*)W, out, bias, M, N, K, ldc, n_valid, alpha, epilogue,
                                  (hipStream_t)stream, e->gemm_ws[0].partial ? &e->gemm_ws[0] : nullptr);
  return launched(e, s, "gemm");
}

int esmdiff_describe_gemm_choice(int32_t M, int32_t N, int32_t K, int64_t ws_floats, int32_t* w4_out, int32_t* rows_out,
                                 int32_t* splits_out, int32_t* stages_out) {
  if (!w4_out || !rows_out || !splits_out || !stages_out || M <= 0 || N <= 0 || K <= 0 || N % 128 || K % 64 || ws_floats < 0)
    return ESMDIFF_E_INVALID;
  int w4 = 0, rows = 0, S = 0, stages = 0;
  ed::describe_gemm_choice(M, N, K, (size_t)ws_floats, &w4, &rows, &S, &stages);
  *w4_out = w4;
  *rows_out = rows;
  *splits_out = S;
  *stages_out = stages;
  return 0;
}

int esmdiff_gemm_workspace_floats(const esmdiff_engine* e, int64_t* floats_out) {
  if (!e || !floats_out) return ESMDIFF_E_INVALID;
  *floats_out = e->gemm_ws[0].partial ? (int64_t)e->gemm_ws[0].partial_floats : 0;
  return 0;
}

#ifdef ED_DEBUG   // measurement aid (scratch/bench_gemm.py), not a switch
int esmdiff_gemm_bf16_timed(const void* A, const void* W, void* out, const float* bias, int32_t M, int32_t N,
                            int32_t K, int32_t ldc, int32_t n_valid, float alpha, int32_t epilogue, int32_t iters,
                            float* ms_out, void* stream) {
  if (!ms_out || iters <= 0) return ESMDIFF_E_INVALID;
  hipStream_t st = (hipStream_t)stream;
  hipEvent_t a, b;
  hipEventCreate(&a);
  hipEventCreate(&b);
  int r = esmdiff_gemm_bf16(A, W, out, bias, M, N, K, ldc, n_valid, alpha, epilogue, stream);  // warm-up
  hipEventRecord(a, st);
  for (int i = 0; i < iters && r == 0; ++i) r = esmdiff_gemm_bf16(A, W, out, bias, M, N, K, ldc, n_valid, alpha, epilogue, stream);
  hipEventRecord(b, st);
  hipEventSynchronize(b);
  float ms = 0;
  hipEventElapsedTime(&ms, a, b);
  *ms_out = ms / iters;
  hipEventDestroy(a);
  hipEventDestroy(b);
  return r;
}
#endif  // ED_DEBUG

int esmdiff_branch_linear_layernorm(esmdiff_engine* e, const void* A, const void* W, float* x, float alpha, const float* w,
                                    const float* b, void* y, int32_t M, int32_t N, int32_t K, int32_t* splits_out,
                                    void* stream) {
  if (!e || !A || !W || !x || !w || !y) return ESMDIFF_E_INVALID;
  if (!e->gemm_ws[0].partial) return fail(e, ESMDIFF_E_INVALID, "engine has no split-K workspace (f32 / f32_split engines have none)");
  ed::GemmPartials P{};
  hipError_t s = launch_gemm_partials((const bf16_t*)A, (const bf16_t*)W, &e->gemm_ws[0], M, N, K, (hipStream_t)stream, &P);
  if (s == hipSuccess) s = launch_add_partials_layernorm_bf16(x, P, N, alpha, w, b, (bf16_t*)y, M, N, (hipStream_t)stream);
  if (int r = launched(e, s, "branch linear + layernorm")) return r;
  if (splits_out) *splits_out = P.S;
  return 0;
}

int esmdiff_layernorm_bf16(const float* x, const float* w, const float* b, void* y, int32_t M, int32_t D, void* stream) {
  if (!x || !w || !y) return ESMDIFF_E_INVALID;
  hipError_t s = launch_layernorm_bf16(x, w, b, (bf16_t*)y, M, D, (hipStream_t)stream);
  if (s != hipSuccess) return fail(nullptr, ESMDIFF_E_HIP, "layernorm: %s", hipGetErrorString(s));
  return 0;
}

int esmdiff_attention_bf16(esmdiff_engine* e, const void* qkv, const float* q_ln_w, const float* k_ln_w, void* ctx,
                           int32_t B, int32_t L, void* stream) {
  if (!e) return ESMDIFF_E_INVALID;
  if (!qkv || !q_ln_w || !k_ln_w || !ctx) return fail(e, ESMDIFF_E_INVALID, "null pointer");
  if (e->strict || e->f16) return fail(e, ESMDIFF_E_INVALID, "esmdiff_attention_bf16 needs a bf16 engine (this one is float32 or f16)");
  if (int r = check_bl(e, B, L)) return r;
  HIP_TRY(e, launch_qk_norm_rope((const bf16_t*)qkv, q_ln_w, k_ln_w, e->rope_cos, e->rope_sin, e->q, e->k, B, L,
                                 e->cfg.n_heads, (hipStream_t)stream));
  HIP_TRY(e, launch_attention(e->q, e->k, (const bf16_t*)qkv, (bf16_t*)ctx, B, L, e->cfg.n_heads, (hipStream_t)stream));
  return 0;
}

int esmdiff_attention_f16(esmdiff_engine* e, const void* qkv, const float* q_ln_w, const float* k_ln_w, void* ctx,
                          int32_t B, int32_t L, void* stream) {
  if (!e) return ESMDIFF_E_INVALID;
  if (!qkv || !q_ln_w || !k_ln_w || !ctx) return fail(e, ESMDIFF_E_INVALID, "null pointer");
  if (!e->f16) return fail(e, ESMDIFF_E_INVALID, "esmdiff_attention_f16 needs an f16 engine");
  if (int r = check_bl(e, B, L)) return r;
  HIP_TRY(e, ed16::launch_qk_norm_rope((const bf16_t*)qkv, q_ln_w, k_ln_w, e->rope_cos, e->rope_sin, e->q, e->k, B, L,
                                       e->cfg.n_heads, (hipStream_t)stream));
  HIP_TRY(e, ed16::launch_attention(e->q, e->k, (const bf16_t*)qkv, (bf16_t*)ctx, B, L, e->cfg.n_heads, (hipStream_t)stream));
  return 0;
}

int esmdiff_attention_ragged(esmdiff_engine* e, const void* qkv, const float* q_ln_w, const float* k_ln_w, void* ctx,
                             const int32_t* lens, int32_t B, int32_t L, void* stream) {
  if (!e) return ESMDIFF_E_INVALID;
  if (!qkv || !q_ln_w || !k_ln_w || !ctx) return fail(e, ESMDIFF_E_INVALID, "null pointer");
  if (e->kind != 0) return fail(e, ESMDIFF_E_INVALID, "esmdiff_attention_ragged needs an ESM3 engine");
  if (int r = check_bl(e, B, L)) return r;
  hipStream_t st = (hipStream_t)stream;
  const int H = e->cfg.n_heads, D = e->cfg.d_model;
  const int32_t* dl = nullptr;
  if (lens) {   // host lengths -> the engine's sub-batch length buffer (validated here: the kernels index with them)
    for (int b = 0; b < B; ++b)
      if (lens[b] < 1 || lens[b] > L) return fail(e, ESMDIFF_E_INVALID, "lens[%d] = %d outside 1..L (%d)", b, lens[b], L);
    HIP_TRY(e, hipStreamSynchronize(st));
    HIP_TRY(e, hipMemcpy(e->lens_sub_dev, lens, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice));
    dl = e->lens_sub_dev;
  }
  if (e->strict && e->split) {   // f32 qkv -> split q / k / v rows (unit scales) -> float32-grade attention on the f16 MFMA
    uint16_t *q2 = reinterpret_cast<uint16_t*>(e->fq), *k2 = reinterpret_cast<uint16_t*>(e->fk), *v2 = reinterpret_cast<uint16_t*>(e->fh);
    HIP_TRY(e, launch_qk_norm_rope_split((const float*)qkv, q_ln_w, k_ln_w, e->rope_cos, e->rope_sin, q2, k2, B, L, H,
                                         0.18033688011112042f /* log2(e) / 8 */, 1.0f, st));
    HIP_TRY(e, launch_v_split((const float*)qkv, v2, B * L, D, 1.0f, st));
    HIP_TRY(e, launch_attention_split(q2, k2, v2, (float*)ctx, B, L, H, 1.0f, 1.0f, st, dl));
  } else if (e->strict) {
    HIP_TRY(e, launch_qk_norm_rope_f32((const float*)qkv, q_ln_w, k_ln_w, e->rope_cos, e->rope_sin, e->fq, e->fk, B, L, H, st));
    HIP_TRY(e, launch_attention_f32(e->fq, e->fk, (const float*)qkv, (float*)ctx, B, L, H, st, dl));
  } else {
    HIP_TRY(e, ED_KN(e->f16, launch_qk_norm_rope((const bf16_t*)qkv, q_ln_w, k_ln_w, e->rope_cos, e->rope_sin, e->q, e->k, B, L, H, st)));
    HIP_TRY(e, ED_KN(e->f16, launch_attention(e->q, e->k, (const bf16_t*)qkv, (bf16_t*)ctx, B, L, H, st, dl)));
  }
  if (lens) HIP_TRY(e, hipStreamSynchronize(st));   // the next call may rewrite lens_sub_dev
  return 0;
}

int esmdiff_qk_norm_rope(esmdiff_engine* e, const void* qkv, const float* q_ln_w, const float* k_ln_w, void* q, void* k,
                         int32_t B, int32_t L, int32_t H, void* stream) {
  if (!e) return ESMDIFF_E_INVALID;
  if (!qkv || !q_ln_w || !k_ln_w || !q || !k) return fail(e, ESMDIFF_E_INVALID, "null pointer");
  if (e->strict) return fail(e, ESMDIFF_E_INVALID, "esmdiff_qk_norm_rope needs a bf16 or f16 engine (this one is float32)");
  if (H <= 0 || H > 32) return fail(e, ESMDIFF_E_INVALID, "H=%d: 1 .. 32 heads of 64", H);
  if (int r = check_bl(e, B, L)) return r;   // the rotary tables hold max_len positions
  HIP_TRY(e, ED_KN(e->f16, launch_qk_norm_rope((const bf16_t*)qkv, q_ln_w, k_ln_w, e->rope_cos, e->rope_sin, (bf16_t*)q, (bf16_t*)k, B, L, H,
                                               (hipStream_t)stream)));
  return 0;
}

// attention_kernel_occ4 / attention_kernel_ragged_occ4 alone, on operands the caller made: no q/k LayerNorm, no rotary, no engine
int esmdiff_attention_16_parts(int32_t dtype, const void* q, const void* k, const void* qkv, void* ctx, const int32_t* lens,
                               int32_t B, int32_t L, int32_t H, void* stream) {
  if (!q || !k || !qkv || !ctx) return fail(nullptr, ESMDIFF_E_INVALID, "attention_16_parts: null pointer");
  if (dtype != 0 && dtype != 1) return fail(nullptr, ESMDIFF_E_INVALID, "attention_16_parts: dtype %d (0 bf16, 1 f16)", dtype);
  if (B <= 0 || L <= 0 || H <= 0 || H > 32 || (int64_t)B * L > 0x3fffffffll)
    return fail(nullptr, ESMDIFF_E_INVALID, "attention_16_parts: B=%d L=%d must be positive (B * L < 2^30), H=%d in 1 .. 32", B, L, H);
  if (lens)   // the kernel indexes with them
    for (int b = 0; b < B; ++b)
      if (lens[b] < 1 || lens[b] > L)
        return fail(nullptr, ESMDIFF_E_INVALID, "attention_16_parts: lens[%d] = %d outside 1..L (%d)", b, lens[b], L);
  const hipStream_t st = (hipStream_t)stream;
  int32_t* dl = nullptr;
  if (lens && hipMalloc(&dl, (size_t)B * sizeof(int32_t)) != hipSuccess) return fail(nullptr, ESMDIFF_E_HIP, "attention_16_parts: hipMalloc failed");
  hipError_t s = lens ? hipMemcpyAsync(dl, lens, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, st) : hipSuccess;
  if (s == hipSuccess)
    s = ED_KN(dtype == 1, launch_attention((const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)qkv, (bf16_t*)ctx, B, L, H, st, dl));
  if (dl) {   // with lengths the call waits: the length buffer and the caller's host copy die here
    const hipError_t s2 = hipStreamSynchronize(st);
    if (s == hipSuccess) s = s2;
    hipFree(dl);
  }
  return launched(nullptr, s, "attention_16_parts");
}

int esmdiff_add_layernorm(int32_t dtype, float* x, const void* delta, const void* delta2, int32_t write_x, const float* w,
                          const float* b, void* y, int32_t M, int32_t D, void* stream) {
  if (!x || !w || !y) return fail(nullptr, ESMDIFF_E_INVALID, "add_layernorm: null pointer");
  if (dtype != 0 && dtype != 1) return fail(nullptr, ESMDIFF_E_INVALID, "add_layernorm: dtype %d (0 bf16, 1 f16)", dtype);
  if (M <= 0 || D <= 0) return fail(nullptr, ESMDIFF_E_INVALID, "add_layernorm: M=%d D=%d must be positive", M, D);
  return launched(nullptr, ED_KN(dtype, launch_add_layernorm_bf16(x, (const bf16_t*)delta, (const bf16_t*)delta2, write_x, w, b, (bf16_t*)y, M, D,
                                                                  (hipStream_t)stream)), "add_layernorm");
}

int esmdiff_geom_attention(const void* P, int32_t dtype, const float* rot, const float* trans, const uint8_t* has_frame,
                           const float* rotation_scale, const float* distance_scale, void* out, int32_t B, int32_t L,
                           int32_t VH, void* stream) {
  if (!P || !rot || !trans || !has_frame || !rotation_scale || !distance_scale || !out)
    return fail(nullptr, ESMDIFF_E_INVALID, "geom_attention: null pointer");
  if (dtype < 0 || dtype > 2) return fail(nullptr, ESMDIFF_E_INVALID, "geom_attention: dtype %d (0 bf16, 1 f16, 2 f32)", dtype);
  if (B <= 0 || L <= 0 || VH <= 0) return fail(nullptr, ESMDIFF_E_INVALID, "geom_attention: B=%d L=%d VH=%d must be positive", B, L, VH);
  if (L > 3200) return fail(nullptr, ESMDIFF_E_INVALID, "geom_attention: L=%d exceeds the kernel's 150 KB of LDS (L <= 3200)", L);
  std::vector<float> hw(2 * (size_t)VH);
  std::copy(rotation_scale, rotation_scale + VH, hw.begin());
  std::copy(distance_scale, distance_scale + VH, hw.begin() + VH);
  softplus_host(hw.data(), 2 * VH);
  float* dw = nullptr;
  if (hipMalloc(&dw, hw.size() * sizeof(float)) != hipSuccess) return fail(nullptr, ESMDIFF_E_HIP, "geom_attention: hipMalloc failed");
  const hipStream_t st = (hipStream_t)stream;
  hipError_t s = hipMemcpyAsync(dw, hw.data(), hw.size() * sizeof(float), hipMemcpyHostToDevice, st);
  if (s == hipSuccess) {
    if (dtype == 2)
      s = ed::launch_geom_attention_f32((const float*)P, rot, trans, has_frame, dw, dw + VH, (float*)out, B, L, VH, st);
    else
      s = ED_KN(dtype == 1, launch_geom_attention((const bf16_t*)P, rot, trans, has_frame, dw, dw + VH, (bf16_t*)out, B, L, VH, st));
  }
  const hipError_t s2 = hipStreamSynchronize(st);   // synchronous: the scale buffer and the host copy die here
  if (s == hipSuccess) s = s2;
  hipFree(dw);
  return launched(nullptr, s, "geom_attention");
}

// ---- the structure decoder's heads, one kernel at a time (synchronous) ----
// a launch on the caller's stream followed by its completion
static int launched_sync(hipError_t s, hipStream_t st, const char* name) {
  const hipError_t s2 = hipStreamSynchronize(st);
  return launched(nullptr, s == hipSuccess ? s2 : s, name);
}

int esmdiff_dim6_to_backbone(const float* v, int32_t ld, float* out, int32_t M, float trans_scale, void* stream) {
  if (!v || !out) return fail(nullptr, ESMDIFF_E_INVALID, "dim6_to_backbone: null pointer");
  if (M <= 0 || ld < 9) return fail(nullptr, ESMDIFF_E_INVALID, "dim6_to_backbone: M=%d must be positive, ld=%d at least 9", M, ld);
  const hipStream_t st = (hipStream_t)stream;
  return launched_sync(launch_dim6_to_backbone(v, ld, out, M, trans_scale, st), st, "dim6_to_backbone");
}

int esmdiff_plddt_mean(const float* v, int32_t ld, int32_t n_bins, float* out, int32_t M, void* stream) {
  if (!v || !out) return fail(nullptr, ESMDIFF_E_INVALID, "plddt_mean: null pointer");
  if (M <= 0 || n_bins <= 0 || ld < n_bins)
    return fail(nullptr, ESMDIFF_E_INVALID, "plddt_mean: M=%d n_bins=%d must be positive, ld=%d at least n_bins", M, n_bins, ld);
  const hipStream_t st = (hipStream_t)stream;
  return launched_sync(launch_plddt_mean(v, ld, n_bins, out, M, st), st, "plddt_mean");
}

int esmdiff_pair_features(const void* qk, int32_t dtype, void* X, int32_t nb, int32_t L, void* stream) {
  if (!qk || !X) return fail(nullptr, ESMDIFF_E_INVALID, "pair_features: null pointer");
  if (dtype != 0 && dtype != 2)
    return fail(nullptr, ESMDIFF_E_INVALID, "pair_features: dtype %d (0 bf16, 2 f32; the pairwise head has no f16 build)", dtype);
  if (nb <= 0 || L <= 0 || (int64_t)nb * L * L > 0x7fffffffll)
    return fail(nullptr, ESMDIFF_E_INVALID, "pair_features: nb=%d L=%d must be positive with nb * L^2 < 2^31", nb, L);
  const hipStream_t st = (hipStream_t)stream;
  const hipError_t s = dtype == 2 ? launch_pair_features_f32((const float*)qk, (float*)X, nb, L, st)
                                  : launch_pair_features((const bf16_t*)qk, (bf16_t*)X, nb, L, st);
  return launched_sync(s, st, "pair_features");
}

int esmdiff_pae_tm(const float* logits, const int64_t* tokens, float* tm_rows, float* pae, float* ptm, int32_t nb, int32_t L,
                   float max_bin, void* stream) {
  if (!logits || !tokens || !tm_rows || !ptm) return fail(nullptr, ESMDIFF_E_INVALID, "pae_tm: null pointer");
  if (nb <= 0 || L <= 0 || (int64_t)nb * L * L > 0x7fffffffll || !(max_bin > 0.f))
    return fail(nullptr, ESMDIFF_E_INVALID, "pae_tm: nb=%d L=%d max_bin=%g must be positive with nb * L^2 < 2^31", nb, L, (double)max_bin);
  const hipStream_t st = (hipStream_t)stream;
  return launched_sync(launch_pae_tm(logits, tokens, tm_rows, pae, ptm, nb, L, max_bin, st), st, "pae_tm");
}

// ---- the float32-grade row kernels of F32 / F32_SPLIT engines, one launcher at a time, enqueued on the caller's stream ----
int esmdiff_layernorm_f32rows(const float* x, const float* w, const float* b, int32_t split, int32_t gelu_in, const void* delta,
                              int32_t delta_dtype, void* a3, float* rs, float* y32, int32_t M, int32_t D, void* stream) {
  if (!x || !w) return fail(nullptr, ESMDIFF_E_INVALID, "layernorm_f32rows: null pointer");
  if (split != 0 && split != 1) return fail(nullptr, ESMDIFF_E_INVALID, "layernorm_f32rows: split %d (0 f32 rows, 1 split rows)", split);
  if (M <= 0 || D <= 0 || D % 4 || D > 2048)
    return fail(nullptr, ESMDIFF_E_INVALID, "layernorm_f32rows: M=%d must be positive, D=%d a positive multiple of 4 up to 2048", M, D);
  const hipStream_t st = (hipStream_t)stream;
  if (!split) {
    if (!y32 || gelu_in || delta || a3 || rs)
      return fail(nullptr, ESMDIFF_E_INVALID, "layernorm_f32rows: the f32 kernel writes y32 only and takes neither gelu_in nor delta");
    return launched(nullptr, launch_layernorm_f32(x, w, b, y32, M, D, st), "layernorm_f32");
  }
  if (!a3 || !rs) return fail(nullptr, ESMDIFF_E_INVALID, "layernorm_f32rows: the split kernel needs a3 and rs");
  if ((gelu_in != 0 && gelu_in != 1) || (delta_dtype != 0 && delta_dtype != 1))
    return fail(nullptr, ESMDIFF_E_INVALID, "layernorm_f32rows: gelu_in %d (0 / 1), delta_dtype %d (0 bf16, 1 f16)", gelu_in, delta_dtype);
  return launched(nullptr, launch_layernorm_split(x, w, b, (uint16_t*)a3, rs, y32, M, D, gelu_in, st, (const uint16_t*)delta, delta_dtype),
                  "layernorm_split");
}

int esmdiff_swiglu_f32(const float* gu, float* mid, int32_t M, int32_t FH, void* stream) {
  if (!gu || !mid) return fail(nullptr, ESMDIFF_E_INVALID, "swiglu_f32: null pointer");
  if (M <= 0 || FH <= 0 || FH % 4)
    return fail(nullptr, ESMDIFF_E_INVALID, "swiglu_f32: M=%d must be positive, FH=%d a positive multiple of 4", M, FH);
  const hipStream_t st = (hipStream_t)stream;
  return launched(nullptr, launch_swiglu_f32(gu, mid, M, FH, st), "swiglu_f32");
}

int esmdiff_qk_norm_rope_f32(esmdiff_engine* e, const float* qkv, const float* q_ln_w, const float* k_ln_w, int32_t split,
                             float q_scale, float k_scale, void* q, void* k, int32_t B, int32_t L, int32_t H, void* stream) {
  if (!e) return ESMDIFF_E_INVALID;
  if (!qkv || !q_ln_w || !k_ln_w || !q || !k) return fail(e, ESMDIFF_E_INVALID, "null pointer");
  if (!e->rope_cos || !e->rope_sin) return fail(e, ESMDIFF_E_INVALID, "esmdiff_qk_norm_rope_f32 needs an engine with rotary tables");
  if (split != 0 && split != 1) return fail(e, ESMDIFF_E_INVALID, "split %d (0 f32 rows, 1 [hi | lo] f16 rows)", split);
  if (H <= 0 || H > 32) return fail(e, ESMDIFF_E_INVALID, "H=%d: 1 .. 32 heads of 64", H);
  if (B <= 0 || L <= 0 || L > e->cfg.max_len || (int64_t)B * L > 0x3fffffffll)   // the rotary tables hold max_len positions
    return fail(e, ESMDIFF_E_INVALID, "B=%d L=%d: positive, L <= max_len (%d), B * L < 2^30", B, L, e->cfg.max_len);
  if (split && !(q_scale > 0.f && k_scale > 0.f && std::isfinite(q_scale) && std::isfinite(k_scale)))
    return fail(e, ESMDIFF_E_INVALID, "q_scale=%g k_scale=%g must be finite and positive", (double)q_scale, (double)k_scale);
  const hipStream_t st = (hipStream_t)stream;
  const hipError_t s = split ? launch_qk_norm_rope_split(qkv, q_ln_w, k_ln_w, e->rope_cos, e->rope_sin, (uint16_t*)q, (uint16_t*)k, B, L, H,
                                                         q_scale, k_scale, st)
                             : launch_qk_norm_rope_f32(qkv, q_ln_w, k_ln_w, e->rope_cos, e->rope_sin, (float*)q, (float*)k, B, L, H, st);
  return launched(e, s, split ? "qk_norm_rope_split" : "qk_norm_rope_f32");
}

int esmdiff_v_split(const float* qkv, void* v2, int32_t M, int32_t D, float scale, void* stream) {
  if (!qkv || !v2) return fail(nullptr, ESMDIFF_E_INVALID, "v_split: null pointer");
  if (M <= 0 || D <= 0 || D % 4 || !(scale > 0.f) || !std::isfinite(scale))
    return fail(nullptr, ESMDIFF_E_INVALID, "v_split: M=%d must be positive, D=%d a positive multiple of 4, scale=%g finite and positive", M, D,
                (double)scale);
  const hipStream_t st = (hipStream_t)stream;
  return launched(nullptr, launch_v_split(qkv, (uint16_t*)v2, M, D, scale, st), "v_split");
}

int esmdiff_attention_f32_parts(const void* q, const void* k, const void* v, int32_t split, float qk_scale_product, float v_scale,
                                float* ctx, const int32_t* lens, int32_t B, int32_t L, int32_t H, void* stream) {
  if (!q || !k || !v || !ctx) return fail(nullptr, ESMDIFF_E_INVALID, "attention_f32_parts: null pointer");
  if (split != 0 && split != 1) return fail(nullptr, ESMDIFF_E_INVALID, "attention_f32_parts: split %d (0 f32, 1 [hi | lo] f16 operands)", split);
  if (B <= 0 || L <= 0 || H <= 0 || H > 32 || B > 65535 || (int64_t)B * L > 0x3fffffffll)
    return fail(nullptr, ESMDIFF_E_INVALID, "attention_f32_parts: B=%d L=%d must be positive (B <= 65535, B * L < 2^30), H=%d in 1 .. 32", B, L, H);
  if (split && !(qk_scale_product > 0.f && v_scale > 0.f && std::isfinite(qk_scale_product) && std::isfinite(v_scale)))
    return fail(nullptr, ESMDIFF_E_INVALID, "attention_f32_parts: qk_scale_product=%g v_scale=%g must be finite and positive",
                (double)qk_scale_product, (double)v_scale);
  if (lens)   // the kernels index with them
    for (int b = 0; b < B; ++b)
      if (lens[b] < 1 || lens[b] > L)
        return fail(nullptr, ESMDIFF_E_INVALID, "attention_f32_parts: lens[%d] = %d outside 1..L (%d)", b, lens[b], L);
  const hipStream_t st = (hipStream_t)stream;
  int32_t* dl = nullptr;
  if (lens && hipMalloc(&dl, (size_t)B * sizeof(int32_t)) != hipSuccess) return fail(nullptr, ESMDIFF_E_HIP, "attention_f32_parts: hipMalloc failed");
  hipError_t s = lens ? hipMemcpyAsync(dl, lens, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, st) : hipSuccess;
  if (s == hipSuccess) {
    if (split)
      s = launch_attention_split((const uint16_t*)q, (const uint16_t*)k, (const uint16_t*)v, ctx, B, L, H, qk_scale_product, v_scale, st, dl);
    else
      s = launch_attention_f32((const float*)q, (const float*)k, (const float*)v, ctx, B, L, H, st, dl);
  }
  if (dl) {   // with lengths the call waits: the length buffer and the caller's host copy die here
    const hipError_t s2 = hipStreamSynchronize(st);
    if (s == hipSuccess) s = s2;
    hipFree(dl);
  }
  return launched(nullptr, s, split ? "attention_split" : "attention_f32");
}

int esmdiff_gemm_split_k(const void* a3, const float* rs, const void* w3, float w_inv_scale, float* parts, float* x, int32_t M,
                         int32_t N, int32_t K, int32_t S, float div, void* stream) {
  if (!a3 || !w3 || !parts || !x) return fail(nullptr, ESMDIFF_E_INVALID, "gemm_split_k: null pointer");
  if (M <= 0 || N <= 0 || K <= 0 || K > 0x7fffffff / 3 || !(div != 0.f))
    return fail(nullptr, ESMDIFF_E_INVALID, "gemm_split_k: M=%d N=%d K=%d must be positive, div=%g non-zero", M, N, K, (double)div);
  if (S < 2 || N % 256 || (3 * K) % S || ((3 * K) / S) % 128 || (3 * K) / S < 384)   // what launch_gemm256w4_splitk accepts
    return fail(nullptr, ESMDIFF_E_INVALID, "gemm_split_k: S=%d >= 2, N=%d %% 256 == 0, 3K / S (K=%d) a multiple of 128 and at least 384", S, N, K);
  const hipStream_t st = (hipStream_t)stream;
  hipError_t s = launch_gemm256w4_splitk((const uint16_t*)a3, (const uint16_t*)w3, w_inv_scale, parts, M, N, K, S, st);
  if (s == hipSuccess) s = launch_splitk_reduce_resid(parts, rs, x, M, N, S, div, st);
  return launched(nullptr, s, "gemm_split_k");
}

int esmdiff_get_attention_scales(esmdiff_engine* e, int32_t layer, float* qk_out, float* v_out) {
  if (!e) return ESMDIFF_E_INVALID;
  if (!qk_out || !v_out) return fail(e, ESMDIFF_E_INVALID, "null pointer");
  if (!(e->strict && e->split)) return fail(e, ESMDIFF_E_INVALID, "esmdiff_get_attention_scales needs an F32_SPLIT engine");
  if (layer < 0 || layer >= (int)e->layers.size()) return fail(e, ESMDIFF_E_INVALID, "layer %d outside 0 .. %d", layer, (int)e->layers.size() - 1);
  *qk_out = e->layers[layer].att_qk;
  *v_out = e->layers[layer].att_v;
  return 0;
}

int esmdiff_decoder_set_pair_chunk_bytes(esmdiff_engine* e, int64_t bytes) {
  if (!e) return ESMDIFF_E_INVALID;
  if (e->kind != 1) return fail(e, ESMDIFF_E_INVALID, "not a decoder engine");
  if (bytes < 0) return fail(e, ESMDIFF_E_INVALID, "pair chunk bytes %lld: positive, or 0 for the default", (long long)bytes);
  e->pair_chunk_bytes = bytes ? bytes : kDefaultPairChunkBytes;
  return 0;
}

// ---- weight conversion at create and the input stage, one launcher at a time, enqueued on the caller's stream ----
static bool weight_dtype_ok(int32_t dt) { return dt == ESMDIFF_F32 || dt == ESMDIFF_BF16; }

int esmdiff_convert_weight(const void* src, int32_t src_dtype, void* dst, int32_t dst_kind, int64_t n, void* stream) {
  if (!src || !dst) return fail(nullptr, ESMDIFF_E_INVALID, "convert_weight: null pointer");
  if (!weight_dtype_ok(src_dtype) || dst_kind < 0 || dst_kind > 2)
    return fail(nullptr, ESMDIFF_E_INVALID, "convert_weight: src_dtype %d (0 f32, 1 bf16), dst_kind %d (0 bf16, 1 f16, 2 f32)", src_dtype, dst_kind);
  if (n <= 0) return fail(nullptr, ESMDIFF_E_INVALID, "convert_weight: n=%lld must be positive", (long long)n);
  const hipStream_t st = (hipStream_t)stream;
  if (dst_kind == 2) return launched(nullptr, launch_to_f32(src, src_dtype, (float*)dst, n, st), "to_f32");
  return launched(nullptr, ED_KN(dst_kind == 1, launch_to_bf16(src, src_dtype, (bf16_t*)dst, n, st)), "to_bf16");
}

int esmdiff_interleave_swiglu(const void* src, int32_t src_dtype, void* dst, int32_t dst_kind, int32_t H, int32_t K, void* stream) {
  if (!src || !dst) return fail(nullptr, ESMDIFF_E_INVALID, "interleave_swiglu: null pointer");
  if (!weight_dtype_ok(src_dtype) || (dst_kind != 0 && dst_kind != 1))
    return fail(nullptr, ESMDIFF_E_INVALID, "interleave_swiglu: src_dtype %d (0 f32, 1 bf16), dst_kind %d (0 bf16, 1 f16)", src_dtype, dst_kind);
  if (H <= 0 || H % 32 || K <= 0)
    return fail(nullptr, ESMDIFF_E_INVALID, "interleave_swiglu: H=%d a positive multiple of 32, K=%d positive", H, K);
  const hipStream_t st = (hipStream_t)stream;
  return launched(nullptr, ED_KN(dst_kind == 1, launch_interleave_swiglu(src, src_dtype, (bf16_t*)dst, H, K, st)), "interleave_swiglu");
}

int esmdiff_weight_rownorm_max(const void* src, int32_t src_dtype, int64_t r0, int32_t rows, int32_t K, float* out) {
  if (!src || !out) return fail(nullptr, ESMDIFF_E_INVALID, "weight_rownorm_max: null pointer");
  if (!weight_dtype_ok(src_dtype) || r0 < 0 || rows <= 0 || K <= 0)
    return fail(nullptr, ESMDIFF_E_INVALID, "weight_rownorm_max: src_dtype %d (0 f32, 1 bf16), r0=%lld >= 0, rows=%d and K=%d positive", src_dtype,
                (long long)r0, rows, K);
  uint32_t* bits = nullptr;
  if (hipMalloc(&bits, 4) != hipSuccess) return fail(nullptr, ESMDIFF_E_HIP, "weight_rownorm_max: hipMalloc failed");
  hipError_t s = weight_rownorm_max(src, src_dtype, r0, rows, K, bits, out);
  if (s == hipSuccess) s = hipDeviceSynchronize();
  hipFree(bits);
  return launched(nullptr, s, "weight_rownorm_max");
}

int esmdiff_embed_rows(const int64_t* seq, const int64_t* xtok, const float* e_seq, const float* e_struct, const float* cvec,
                       const float* cond, int32_t cond_stride, float* out, int32_t B, int32_t L, int32_t D, void* stream) {
  if (!seq || !xtok || !e_seq || !e_struct || !cvec || !out) return fail(nullptr, ESMDIFF_E_INVALID, "embed_rows: null pointer");
  if (B <= 0 || L <= 0 || (int64_t)B * L > 0x7fffffffll || D <= 0 || D % 4)
    return fail(nullptr, ESMDIFF_E_INVALID, "embed_rows: B=%d L=%d must be positive with B * L < 2^31, D=%d a positive multiple of 4", B, L, D);
  if (cond_stride < 0 || cond_stride % 4)
    return fail(nullptr, ESMDIFF_E_INVALID, "embed_rows: cond_stride=%d must be a non-negative multiple of 4", cond_stride);
  const hipStream_t st = (hipStream_t)stream;
  return launched(nullptr, launch_embed(seq, xtok, e_seq, e_struct, cvec, cond, out, B, L, D, st, cond_stride), "embed");
}

int esmdiff_gather_table_rows(const int64_t* tok, const float* table, float* out, int32_t M, int32_t D, int32_t n_rows, void* stream) {
  if (!tok || !table || !out) return fail(nullptr, ESMDIFF_E_INVALID, "gather_table_rows: null pointer");
  if (M <= 0 || D <= 0 || D % 4 || n_rows <= 0)
    return fail(nullptr, ESMDIFF_E_INVALID, "gather_table_rows: M=%d and n_rows=%d must be positive, D=%d a positive multiple of 4", M, n_rows, D);
  const hipStream_t st = (hipStream_t)stream;
  return launched(nullptr, launch_gather_rows(tok, table, out, M, D, n_rows, st), "gather_rows");
}

int esmdiff_sigma_mlp(const float* t_freq, const float* w1, const float* b1, const float* w2, const float* b2, float* hidden,
                      float* cond, int32_t F, int32_t D, int32_t n_sigma, void* stream) {
  if (!t_freq || !w1 || !b1 || !w2 || !b2 || !hidden || !cond) return fail(nullptr, ESMDIFF_E_INVALID, "sigma_mlp: null pointer");
  if (F <= 0 || D <= 0 || n_sigma <= 0 || n_sigma > 65535)
    return fail(nullptr, ESMDIFF_E_INVALID, "sigma_mlp: F=%d and D=%d must be positive, n_sigma=%d in 1 .. 65535", F, D, n_sigma);
  const hipStream_t st = (hipStream_t)stream;
  return launched(nullptr, launch_sigma_mlp(t_freq, w1, b1, w2, b2, hidden, cond, F, D, st, n_sigma), "sigma_mlp");
}

int esmdiff_layernorm_16in(int32_t dtype, const void* x16, const float* w, const float* b, void* y16, int32_t M, int32_t D,
                           void* stream) {
  if (!x16 || !w || !y16) return fail(nullptr, ESMDIFF_E_INVALID, "layernorm_16in: null pointer");
  if (dtype != 0 && dtype != 1) return fail(nullptr, ESMDIFF_E_INVALID, "layernorm_16in: dtype %d (0 bf16, 1 f16)", dtype);
  if (M <= 0 || D <= 0 || D % 4 || D > 2048)
    return fail(nullptr, ESMDIFF_E_INVALID, "layernorm_16in: M=%d must be positive, D=%d a positive multiple of 4 up to 2048", M, D);
  const hipStream_t st = (hipStream_t)stream;
  return launched(nullptr, ED_KN(dtype == 1, launch_layernorm_bf16_in((const bf16_t*)x16, w, b, (bf16_t*)y16, M, D, st)), "layernorm_16in");
}

// ---- the needed-rows and sub-batch bookkeeping kernels, one launcher at a time, enqueued on the caller's stream ----
int esmdiff_mask_row_list(const int64_t* x, int32_t B, int32_t L, int32_t np, int32_t* list, int32_t* map, int32_t* count,
                          void* stream) {
  if (!x || !list || !map || !count) return fail(nullptr, ESMDIFF_E_INVALID, "mask_row_list: null pointer");
  if (B <= 0 || L <= 0 || np <= 0 || np > B || (int64_t)B * L > 0x7fffffffll)
    return fail(nullptr, ESMDIFF_E_INVALID, "mask_row_list: B=%d L=%d must be positive with B * L < 2^31, np=%d in 1 .. B", B, L, np);
  return launched(nullptr, launch_mask_row_list(x, B, L, np, list, map, count, (hipStream_t)stream), "mask_row_list");
}

int esmdiff_gather_rows16(const void* src, const int32_t* list, void* dst, int32_t n, int32_t D, void* stream) {
  if (!src || !list || !dst) return fail(nullptr, ESMDIFF_E_INVALID, "gather_rows16: null pointer");
  if (n <= 0 || D <= 0 || D % 8) return fail(nullptr, ESMDIFF_E_INVALID, "gather_rows16: n=%d must be positive, D=%d a positive multiple of 8", n, D);
  return launched(nullptr, launch_gather_rows16((const uint16_t*)src, list, (uint16_t*)dst, n, D, (hipStream_t)stream), "gather_rows16");
}

int esmdiff_add_layernorm_rows(int32_t dtype, const float* x, const void* delta, const int32_t* rows, const void* delta2,
                               float* x_out, const float* w, const float* b, void* y, int32_t M, int32_t D, void* stream) {
  if (!x || !w || !y) return fail(nullptr, ESMDIFF_E_INVALID, "add_layernorm_rows: null pointer");
  if (dtype != 0 && dtype != 1) return fail(nullptr, ESMDIFF_E_INVALID, "add_layernorm_rows: dtype %d (0 bf16, 1 f16)", dtype);
  if (M <= 0 || D <= 0) return fail(nullptr, ESMDIFF_E_INVALID, "add_layernorm_rows: M=%d D=%d must be positive", M, D);
  return launched(nullptr, ED_KN(dtype, launch_add_layernorm_rows_bf16(x, (const bf16_t*)delta, rows, (const bf16_t*)delta2, x_out, w, b,
                                                                       (bf16_t*)y, M, D, (hipStream_t)stream)), "add_layernorm_rows");
}

int esmdiff_copy_masked_logits(const int64_t* x, const float* logits, int32_t ld, const int32_t* map, float* out, int32_t ld_out,
                               int32_t V, int32_t rows, void* stream) {
  if (!x || !logits || !out) return fail(nullptr, ESMDIFF_E_INVALID, "copy_masked_logits: null pointer");
  if (rows <= 0 || V <= 0 || ld < V || ld_out < V)
    return fail(nullptr, ESMDIFF_E_INVALID, "copy_masked_logits: rows=%d V=%d must be positive, ld=%d and ld_out=%d at least V", rows, V, ld, ld_out);
  return launched(nullptr, launch_copy_masked_logits(x, logits, ld, map, out, ld_out, V, rows, (hipStream_t)stream), "copy_masked_logits");
}

int esmdiff_ddpm_step_mapped(int64_t* x, const float* logits, int32_t ld, int32_t V, float mc_t, float mc_s, int32_t final_,
                             const esmdiff_rng* rng, int32_t step, int32_t B, int32_t L, int32_t logits_period,
                             const int32_t* row_map, void* stream) {
  if (!x || !logits || (!final_ && !rng)) return fail(nullptr, ESMDIFF_E_INVALID, "ddpm_step_mapped: null pointer");
  if (B <= 0 || L <= 0 || (int64_t)B * L > 0x7fffffffll || V <= ESMDIFF_MASK_ID || ld < V || logits_period < 0)
    return fail(nullptr, ESMDIFF_E_INVALID, "ddpm_step_mapped: B=%d L=%d must be positive with B * L < 2^31, V=%d above the mask column, ld=%d at "
                "least V, logits_period=%d not negative", B, L, V, ld, logits_period);
  return launched(nullptr, launch_ddpm_step(x, logits, ld, V, mc_t, mc_s, final_, nullptr, 1, rng ? rng->seed : 0,
                                            rng ? rng->sample_offset : 0, step, B, L, (hipStream_t)stream, logits_period, 0.f, nullptr,
                                            row_map), "ddpm_step_mapped");
}

int esmdiff_move_token_rows(const int64_t* src, int64_t* dst, const int32_t* idx, int32_t n, int32_t L, int32_t gather,
                            void* stream) {
  if (!src || !dst || !idx) return fail(nullptr, ESMDIFF_E_INVALID, "move_token_rows: null pointer");
  if (n < 0 || L <= 0 || (gather != 0 && gather != 1))
    return fail(nullptr, ESMDIFF_E_INVALID, "move_token_rows: n=%d not negative, L=%d positive, gather %d (0 scatter, 1 gather)", n, L, gather);
  return launched(nullptr, launch_move_token_rows(src, dst, idx, n, L, gather, (hipStream_t)stream), "move_token_rows");
}

int esmdiff_samples_with_mask(const int64_t* x, int32_t B, int32_t L, int32_t* has, void* stream) {
  if (!x || !has) return fail(nullptr, ESMDIFF_E_INVALID, "samples_with_mask: null pointer");
  if (B <= 0 || L <= 0) return fail(nullptr, ESMDIFF_E_INVALID, "samples_with_mask: B=%d L=%d must be positive", B, L);
  return launched(nullptr, launch_samples_with_mask(x, B, L, has, (hipStream_t)stream), "samples_with_mask");
}

int esmdiff_rows_identical(const int64_t* seq, const int64_t* x, int32_t B, int32_t L, int32_t* flag, void* stream) {
  if (!seq || !x || !flag) return fail(nullptr, ESMDIFF_E_INVALID, "rows_identical: null pointer");
  if (B <= 0 || L <= 0) return fail(nullptr, ESMDIFF_E_INVALID, "rows_identical: B=%d L=%d must be positive", B, L);
  return launched(nullptr, launch_rows_identical(seq, x, B, L, flag, (hipStream_t)stream), "rows_identical");
}

// ---- csrc/ed_math.h as one of the three units compiled it (the kernel is csrc/ed_math_eval.inc inside that unit, not here: this unit
// carries no -ffp-contract=off) ----
int esmdiff_math_eval(int32_t unit, int32_t kind, const void* in, void* out, int64_t n, void* stream) {
  if (unit < 0 || unit > 2 || kind < 0 || kind > 3)
    return fail(nullptr, ESMDIFF_E_INVALID, "math_eval: unit %d (0 sampler, 1 score, 2 gibbs), kind %d (0 exp, 1 log, 2 noise, 3 philox)", unit, kind);
  if (n < 0 || ((!in || !out) && n > 0)) return fail(nullptr, ESMDIFF_E_INVALID, "math_eval: n=%lld must not be negative, in and out not null", (long long)n);
  const hipStream_t st = (hipStream_t)stream;
  float* o = (float*)out;
  return launched(nullptr, unit == 0 ? launch_math_eval_sampler(kind, in, o, n, st)
                         : unit == 1 ? launch_math_eval_score(kind, in, o, n, st)
                                     : launch_math_eval_gibbs(kind, in, o, n, st), "math_eval");
}

}  // extern "C"

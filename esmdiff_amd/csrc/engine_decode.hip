// engine_decode.hip — the structure-token decoder's entry: one forward, the backbone, and the confidence heads (pLDDT, pTM / PAE).
#include "engine.h"

using namespace ed;
using namespace eng;

// pTM (and optionally the PAE matrix) of the samples just decoded: pair rows of whole samples at a time through
// linear1 -> GELU -> LayerNorm -> linear2[PAE bins] on the MFMA GEMM, then the bin reduction (csrc/pairwise.hip).
static int pairwise_confidence(esmdiff_engine* e, const int64_t* tokens, float* ptm, float* pae, int B, int L, hipStream_t st) {
  const int64_t LL = (int64_t)L * L;
  // chunk of whole samples: ~1.5 GB of pair rows at most (768 B per row: features, hidden, 64 f32 logits; 1280 B in float32)
  const size_t esz = e->strict ? 4 : 2;
  int cb = (int)std::max<int64_t>(1, std::min<int64_t>(B, e->pair_chunk_bytes / (LL * (int64_t)(256 * esz + 256))));
  if (e->pair_rows_cap < (int64_t)cb * LL) {
    HIP_TRY(e, hipStreamSynchronize(st));
    for (void* p : {(void*)e->pair_x, (void*)e->pair_h, (void*)e->pair_logits})
      if (p) hipFree(p);
    e->pair_x = e->pair_h = nullptr;
    e->pair_logits = nullptr;
    e->pair_rows_cap = 0;
    const size_t rows = (size_t)cb * LL;
    if (hipMalloc(&e->pair_x, rows * 128 * esz) != hipSuccess || hipMalloc(&e->pair_h, rows * 128 * esz) != hipSuccess ||
        hipMalloc(&e->pair_logits, rows * 64 * 4) != hipSuccess)
      return fail(e, ESMDIFF_E_HIP, "pairwise head workspace for %d x %d^2 pair rows: out of memory", cb, L);
    e->pair_rows_cap = (int64_t)rows;
    e->fpair_x = reinterpret_cast<float*>(e->pair_x);   // the same allocations, viewed as float32 on a strict engine
    e->fpair_h = reinterpret_cast<float*>(e->pair_h);
  }
  for (int b0 = 0; b0 < B; b0 += cb) {
    const int nb = std::min(cb, B - b0);
    const int64_t rows = (int64_t)nb * LL;
    if (rows > 0x7fffffffll) return fail(e, ESMDIFF_E_INVALID, "pairwise head: too many pair rows in one chunk");
    if (e->strict) {   // linear1 -> GELU -> LayerNorm -> linear2[PAE rows 160..223], all float32 (no biases in this head)
      HIP_TRY(e, launch_pair_features_f32(e->fpair_qk + (int64_t)b0 * L * 128, e->fpair_x, nb, L, st));
      HIP_TRY(e, launch_gemm_f32(e->fpair_x, 128, e->pw_l1.f32(), e->fpair_h, nullptr, (int)rows, 128, 128, 128, 128, 1.f, ESMDIFF_F32EPI_BIAS_GELU, st));
      HIP_TRY(e, launch_layernorm_f32(e->fpair_h, e->pw_ln_w, e->pw_ln_b, e->fpair_x, (int)rows, 128, st));
      HIP_TRY(e, launch_gemm_f32(e->fpair_x, 128, e->pw_l2.f32() + 160 * 128, e->pair_logits, nullptr, (int)rows, 64, 128, 64, 64, 1.f, ESMDIFF_F32EPI_STORE, st));
      HIP_TRY(e, launch_pae_tm(e->pair_logits, tokens + (int64_t)b0 * L, e->tm_rows + (int64_t)b0 * L, pae ? pae + (int64_t)b0 * LL : nullptr,
                               ptm + b0, nb, L, 31.0f, st));
      continue;
    }
    HIP_TRY(e, launch_pair_features(e->pair_qk + (int64_t)b0 * L * 128, e->pair_x, nb, L, st));
    HIP_TRY(e, launch_gemm_bf16(e->pair_x, e->pw_l1.w16(), e->pair_h, e->zeros128, (int)rows, 128, 128, 128, 128, 1.f, ESMDIFF_EPI_BIAS_GELU_BF16, st));
    HIP_TRY(e, launch_layernorm_bf16_in(e->pair_h, e->pw_ln_w, e->pw_ln_b, e->pair_x, (int)rows, 128, st));
    HIP_TRY(e, launch_gemm_bf16(e->pair_x, e->pw_l2.w16() + 160 * 128, e->pair_logits, e->zeros128, (int)rows, 128, 128, 64, 64, 1.f, ESMDIFF_EPI_BIAS_F32, st));
    HIP_TRY(e, launch_pae_tm(e->pair_logits, tokens + (int64_t)b0 * L, e->tm_rows + (int64_t)b0 * L, pae ? pae + (int64_t)b0 * LL : nullptr,
                             ptm + b0, nb, L, 31.0f, st));
  }
  return 0;
}

extern "C" {

int esmdiff_decoder_decode(esmdiff_engine* e, const int64_t* tokens, float* bb_coords, float* plddt, float* ptm, float* pae,
                           int32_t B, int32_t L, float trans_scale, void* stream) {
  if (!e || !tokens || !bb_coords) return ESMDIFF_E_INVALID;
  if (e->kind != 1) return fail(e, ESMDIFF_E_INVALID, "not a decoder engine");
  if (plddt && !e->has_plddt) return fail(e, ESMDIFF_E_MISSING, "plddt requested but the weight table had no plddt_head.* tensors");
  if ((ptm || pae) && !e->has_pair) return fail(e, ESMDIFF_E_MISSING, "ptm / pae requested but the weight table had no pairwise_classification_head.* tensors");
  if (pae && !ptm) return fail(e, ESMDIFF_E_INVALID, "pae is produced together with ptm: pass both");
  if (int r = check_bl(e, B, L)) return r;
  HIP_TRY(e, hipSetDevice(e->device));
  hipStream_t st = (hipStream_t)stream;
  if (int r = forward(e, tokens, tokens, nullptr, e->logits, e->ld_logits, B, L, st)) return r;
  HIP_TRY(e, launch_dim6_to_backbone(e->logits, e->ld_logits, bb_coords, B * L, trans_scale, st));
  if (plddt) HIP_TRY(e, launch_plddt_mean(e->pl_logits, e->ld_plddt, e->plddt_bins, plddt, B * L, st));
  if (ptm) return pairwise_confidence(e, tokens, ptm, pae, B, L, st);
  return 0;
}

}  // extern "C"

// engine_forward.hip — one forward of an engine: the batch planner and the per-forward launch sequence for the ESM3-open
// structure-token transformer as the reference wires it (slm/models/net.py:371-483, model.py:464-492, 543-607), and the C
// entries that are one forward and nothing else.
//
// Per forward (B x L tokens, M = B*L rows):
//   sigma_mlp (2 GEMV)  -> embed -> 48 x [ add+LN -> QKV GEMM -> q/k LN + rotary (V stays in the QKV buffer) ->
//   attention -> out-proj GEMM (bf16 delta / scale) -> add+LN -> FFN-up GEMM (SwiGLU epilogue) -> FFN-down GEMM
//   (bf16 delta) ] -> final LN -> head GEMM (bias+GELU) -> LN -> head GEMM (bias) -> f32 logits -> fused sampler.
// Block 0's geometric attention contributes exactly 0 when coordinates are all-NaN (the DDPM path: affine_mask all
// False, net.py:433-441 with mask_and_zero_frameless=True, net.py:344) and is skipped; with frames set through
// esmdiff_set_frames it runs between the attention branch and the FFN of block 0 (geom.hip).
// Work is enqueued on the caller's stream, plus one engine-owned stream for the second half of a large batch
// (forked and joined with events, see forward()); a forward never synchronises — except a forward of esmdiff_ddpm_sample, which
// waits once for the count of the rows its sampler will read (needed_tail()).
#include "engine.h"

using namespace ed;
using namespace eng;

namespace {

// Workspace of one sub-batch: the engine's buffers are all sample-major, so a sub-batch is a pointer offset.  An engine holds the
// 16-bit workspace or the float32 one (fh2, a2, rs: also a 16-bit engine with the float32-grade head); the rest stays null here.
struct Part {
  const int64_t *seq, *xtok;
  float *x, *logits, *pl_logits;
  bf16_t *h, *h2, *qkv, *q, *k, *ctx, *mid, *dlt, *dlt2, *gp, *gctx, *pair_qk;
  float *fh, *fh2, *fqkv, *fq, *fk, *fctx, *fgu, *fmid, *fgp, *fgctx, *fpair_qk;   // fgu: F32 engines only
  uint16_t* a2;   // split rows feeding the next float32-grade linear, and their row scales
  float* rs;
  const float *f_rot, *f_trans;
  const uint8_t* f_mask;
  const int32_t* lens;   // ragged batch: this sub-batch's lengths (device), else null
  int b0, B;             // first sample of the sub-batch in the batch, and how many
  hipStream_t st;        // queue pi: the caller's stream (pi = 0) or side[pi - 1]
  const GemmWorkspace *gws, *gws2;   // queue pi's split-K workspaces, null where the engine has none
};

// Cuts B samples into np sub-batches, part pi = samples [B pi / np, B (pi + 1) / np), and offsets every buffer the engine holds.
void cut_batch(esmdiff_engine* e, Part* parts, int np, const int64_t* seq, const int64_t* xtok, float* logits, int ld, int B, int L,
               hipStream_t st) {
  const int64_t D = e->cfg.d_model, FH = e->cfg.ffn_hidden, VH = e->v_heads;
  const int64_t a2_row = 3 * (e->strict ? std::max(D, FH) : D);   // float32-grade engine: also the FFN-down's split rows
  for (int pi = 0; pi < np; ++pi) {
    const int b0 = (int)((int64_t)B * pi / np), b1 = (int)((int64_t)B * (pi + 1) / np);
    const int64_t t0 = (int64_t)b0 * L;
    auto off = [t0](auto* p, int64_t stride) { return p ? p + t0 * stride : nullptr; };
    parts[pi] = Part{off(seq, 1), off(xtok, 1), off(e->x, D), off(logits, ld), off(e->pl_logits, e->ld_plddt),
                     off(e->h, D), off(e->h2, D), off(e->qkv, 3 * D), off(e->q, D), off(e->k, D), off(e->ctx, D), off(e->mid, FH),
                     off(e->dlt, D), off(e->dlt2, D), off(e->gp, 15 * VH), off(e->gctx, 3 * VH), off(e->pair_qk, 128),
                     off(e->fh, D), off(e->fh2, D), off(e->fqkv, 3 * D), off(e->fq, D), off(e->fk, D), off(e->fctx, D),
                     off(e->fgu, 2 * FH), off(e->fmid, FH), off(e->fgp, 15 * VH), off(e->fgctx, 3 * VH), off(e->fpair_qk, 128),
                     off(e->a2, a2_row), off(e->rs, 1), off(e->f_rot, 9), off(e->f_trans, 3), off(e->f_mask, 1),
                     e->cur_lens ? e->cur_lens + b0 : nullptr, b0, b1 - b0, pi == 0 ? st : e->side[pi - 1],
                     e->gemm_ws[pi].partial ? &e->gemm_ws[pi] : nullptr, e->gemm_ws2[pi].partial ? &e->gemm_ws2[pi] : nullptr};
  }
}

// How forward() will cut a batch: number of sub-batch streams, and whether the sub-batches take the small-batch path.
// The PATH (small-batch K-slice planes vs the regular kernels: two summation orders, logits that differ at rounding level) is a
// function of (B, L) alone — it is what the default options choose.  esmdiff_set_option may change how many launch queues run
// the batch, never the path: a stream count or token threshold that would push the sub-batches across small_max_rows() is
// reduced until they stay on the default path's side (tests/test_gpu_fullwidth.py::test_stream_options_never_change_a_bit).
int parts_for(const esmdiff_engine* e, int B, int L, int n_streams, int64_t dual_min_tokens) {
  const int64_t tokens = (int64_t)B * L;
  if (!e->side.empty() && e->profiling != 1 && B >= 2 &&
      (tokens >= dual_min_tokens || (B >= 8 && tokens <= kDualSmallMaxTokens && tokens >= std::min<int64_t>(768, dual_min_tokens))))
    return std::min<int>({(int)e->side.size() + 1, n_streams, B, 4});
  return 1;
}
bool parts_small(const esmdiff_engine* e, int B, int L, int np) {
  if (e->strict) return false;
  const int b_first = (int)((int64_t)B * 1 / np), b_last = B - (int)((int64_t)B * (np - 1) / np);
  return e->gemm_ws[0].partial && e->gemm_ws2[0].partial && (int64_t)b_last * L < ed::small_max_rows() &&
         (int64_t)b_first * L < ed::small_max_rows();
}
struct BatchPlan {
  int np;       // sub-batch launch queues
  bool small;   // the sub-batches take the small-batch path
};
BatchPlan plan_batch(const esmdiff_engine* e, int B, int L) {
  // float32-grade engines: one path, and two queues only for F32_SPLIT at large batches.  (r06: with frames set the two-queue forward
  // was not deterministic while geom_attention_kernel held packed float ops beside the other queue's GEMM: geom.hip.)
  if (e->strict)
    return BatchPlan{(e->split && !e->side.empty() && e->profiling != 1 && B >= 2 && (int64_t)B * L >= kStrictDualMinTokens) ? 2 : 1, false};
  const int np_def = parts_for(e, B, L, kDefaultStreams, kDefaultDualMinTokens);
  const bool small = parts_small(e, B, L, np_def);
  int np = parts_for(e, B, L, e->n_streams, e->dual_min_tokens);
  while (np > 1 && parts_small(e, B, L, np) != small) --np;
  if (parts_small(e, B, L, np) != small) np = np_def;
  return BatchPlan{np, small};
}
int plan_parts(const esmdiff_engine* e, int B, int L) { return plan_batch(e, B, L).np; }
bool plan_small(const esmdiff_engine* e, int B, int L) { return plan_batch(e, B, L).small; }

// A forward on np launch queues — the caller's stream and side[0 .. np - 2]: the side streams start after everything enqueued
// on the caller's stream so far (fork), and the caller's stream goes on after everything they ran (join).
int fork_streams(esmdiff_engine* e, hipStream_t st, int np) {
  if (np > 1) HIP_TRY(e, hipEventRecord(e->ev_fork, st));
  for (int pi = 1; pi < np; ++pi) HIP_TRY(e, hipStreamWaitEvent(e->side[pi - 1], e->ev_fork, 0));
  return 0;
}
int join_streams(esmdiff_engine* e, hipStream_t st, int np) {
  for (int pi = 1; pi < np; ++pi) {
    HIP_TRY(e, hipEventRecord(e->ev_join[pi - 1], e->side[pi - 1]));
    HIP_TRY(e, hipStreamWaitEvent(st, e->ev_join[pi - 1], 0));
  }
  return 0;
}

// precision = F32: the same network in float32 end to end (csrc/strict.hip).  One stream, one launch per op, residual
// adds in the branch GEMMs' epilogues as x + r / scaling_factor (esm's own expression).  Sections are timed like the
// bf16 path's.  Block 0's geometric branch runs between the attention and the FFN branch while frames are set.
// F32_SPLIT at large batches: two sub-batches on two streams, as the 16-bit engine does (every kernel's row results are
// independent of the batch, so the cut changes no bit): the persistent split GEMMs leave CUs idle in their last round and the
// other sub-batch's kernels fill them.  This is one sub-batch, enqueued whole; cond: its first conditioning row.
int strict_part(esmdiff_engine* e, const Part& w, const float* cond, int ld, int L) {
  const esmdiff_config& c = e->cfg;
  const int D = c.d_model, H = c.n_heads, FH = c.ffn_hidden;
  const bool geom = e->has_geom && e->frames_B > 0;
  const int VH = e->v_heads;
  // precision = F32_SPLIT: the same op sequence; every LayerNorm / SwiGLU / attention output that feeds a linear is written
  // as a split row (a2, rs) and the linear runs as three f16 MFMA passes (gemm_split.hip); everything else is unchanged
  const bool sp = e->split;
  uint16_t* a2 = w.a2;
  float* rs = w.rs;
  float* logits = w.logits;
  hipStream_t st = w.st;
  const int B = w.B, M = B * L;
  Prof p{e, st};
  // K-sliced residual linears: only where the slicing constraints hold for this model (3 D / 3 and 3 FH / 4 multiples of 128)
  // this part's slice planes: the parts of a two-stream forward use disjoint regions (4 planes of its padded rows each)
  float* const skp = e->sk_parts ? e->sk_parts + (size_t)4 * D * ((size_t)round_up(w.b0 * L, 256) + (w.b0 ? 256 : 0)) : nullptr;
  const bool sk = sp && e->splitk_small && e->sk_parts && M <= kSplitkMaxRows && e->kind == 0 && D % 128 == 0 && (3 * FH) % 512 == 0 &&
                  D >= 384 && 3 * FH / 4 >= 384;
  if (e->kind == 1) RUN(S_EMBED, launch_gather_rows(w.xtok, e->e_struct, w.x, M, D, ESMDIFF_VOCAB, st));
  else RUN(S_EMBED, launch_embed(w.seq, w.xtok, e->e_seq, e->e_struct, e->cvec, cond, w.x, B, L, D, st, e->sigma_rows > 1 ? D : 0));
  // a linear by its slot's form: SPLIT reads the split rows (a2, rs) the kernel before it wrote, F32 the float32 rows A32
  auto lin = [&](int section, const Linear& W, const float* A32, int lda, int Kdim, float* out, const float* bias, int n_rows, int ldc,
                 int n_valid, float div, int epi) -> int {
    if (W.form == Linear::SPLIT) RUN(section, launch_gemm256w4_split(a2, rs, W.split(), W.inv, out, bias, M, round_up(n_rows, 256), Kdim, ldc, div, epi, st));
    else RUN(section, launch_gemm_f32(A32, lda, W.f32(), out, bias, M, n_rows, Kdim, ldc, n_valid, div, epi, st));
    return 0;
  };
  for (int i = 0; i < c.n_layers; ++i) {
    const Layer& ly = e->layers[i];
    if (sp) RUN(S_LN, launch_layernorm_split(w.x, ly.ln1_w, ly.ln1_b, a2, rs, nullptr, M, D, 0, st));
    else RUN(S_LN, launch_layernorm_f32(w.x, ly.ln1_w, ly.ln1_b, w.fh, M, D, st));
    if (int r = lin(S_QKV, ly.w_qkv, w.fh, D, D, w.fqkv, nullptr, 3 * D, 3 * D, 3 * D, 1.f, ESMDIFF_F32EPI_STORE)) return r;
    if (sp) {   // float32-grade attention on the f16 MFMA: q / k / v as [hi | lo] rows in fq / fk / fh (attention_split.hip)
      uint16_t *q2 = reinterpret_cast<uint16_t*>(w.fq), *k2 = reinterpret_cast<uint16_t*>(w.fk), *v2 = reinterpret_cast<uint16_t*>(w.fh);
      RUN(S_QKROPE, launch_qk_norm_rope_split(w.fqkv, ly.q_ln_w, ly.k_ln_w, e->rope_cos, e->rope_sin, q2, k2, B, L, H,
                                              ly.att_qk * 0.18033688011112042f /* log2(e) / 8 */, ly.att_qk, st));
      RUN(S_QKROPE, launch_v_split(w.fqkv, v2, M, D, ly.att_v, st));
      RUN(S_ATTN, launch_attention_split(q2, k2, v2, w.fctx, B, L, H, ly.att_qk * ly.att_qk, ly.att_v, st, w.lens));
      RUN(S_ATTN, launch_split_rows(w.fctx, D, a2, rs, M, D, st));
    } else {
      RUN(S_QKROPE, launch_qk_norm_rope_f32(w.fqkv, ly.q_ln_w, ly.k_ln_w, e->rope_cos, e->rope_sin, w.fq, w.fk, B, L, H, st));
      RUN(S_ATTN, launch_attention_f32(w.fq, w.fk, w.fqkv, w.fctx, B, L, H, st, w.lens));
    }
    if (sk) {
      RUN(S_OUT, launch_gemm256w4_splitk(a2, ly.w_out.split(), ly.w_out.inv, skp, M, D, D, 3, st));
      RUN(S_OUT, launch_splitk_reduce_resid(skp, rs, w.x, M, D, 3, c.residue_scale, st));
    } else {
      if (int r = lin(S_OUT, ly.w_out, w.fctx, D, D, w.x, nullptr, D, D, D, c.residue_scale, ESMDIFF_F32EPI_RESID_DIV)) return r;
    }
    if (i == 0 && geom) {   // x = x + geom_attn(s_norm(x), frames) / scaling_factor
      const bool gs = e->g_proj.form == Linear::SPLIT;   // (an F32_SPLIT engine whose v_heads do not fit runs this branch as F32)
      if (gs) RUN(S_LN, launch_layernorm_split(w.x, e->g_snorm_w, nullptr, a2, rs, nullptr, M, D, 0, st));
      else RUN(S_LN, launch_layernorm_f32(w.x, e->g_snorm_w, nullptr, w.fh, M, D, st));
      if (int r = lin(S_ATTN, e->g_proj, w.fh, D, D, w.fgp, nullptr, 15 * VH, 15 * VH, 15 * VH, 1.f, ESMDIFF_F32EPI_STORE)) return r;
      RUN(S_ATTN, launch_geom_attention_f32(w.fgp, w.f_rot, w.f_trans, w.f_mask, e->g_wrot, e->g_wdist, w.fgctx, B, L, VH, st));
      if (gs) RUN(S_ATTN, launch_split_rows(w.fgctx, 3 * VH, a2, rs, M, 3 * VH, st));
      if (int r = lin(S_ATTN, e->g_out, w.fgctx, 3 * VH, 3 * VH, w.x, nullptr, D, D, D, c.residue_scale, ESMDIFF_F32EPI_RESID_DIV)) return r;
    }
    if (sp) RUN(S_LN, launch_layernorm_split(w.x, ly.ln2_w, ly.ln2_b, a2, rs, nullptr, M, D, 0, st));
    else RUN(S_LN, launch_layernorm_f32(w.x, ly.ln2_w, ly.ln2_b, w.fh, M, D, st));
    if (sp) {
      // split FFN-up with the SwiGLU in its epilogue: reads the LayerNorm's split row (a2: [M, 3 D]), writes mid as f32 [M, FH];
      // split_rows then makes the FFN-down operand with every row's own power-of-two scale (r05: not a per-layer bound, see
      // gemm256w4.hip) — [M, 2 FH] of gate / up values never exist in memory
      RUN(S_FFN_UP, launch_gemm256w4_split(a2, rs, ly.w_up.split(), ly.w_up.inv, w.fmid, nullptr, M, 2 * FH, D, FH, 1.f, 4, st));
      RUN(S_FFN_UP, launch_split_rows(w.fmid, FH, a2, rs, M, FH, st));
      if (sk) {
        RUN(S_FFN_DOWN, launch_gemm256w4_splitk(a2, ly.w_down.split(), ly.w_down.inv, skp, M, D, FH, 4, st));
        RUN(S_FFN_DOWN, launch_splitk_reduce_resid(skp, rs, w.x, M, D, 4, c.residue_scale, st));
      } else {
        RUN(S_FFN_DOWN, launch_gemm256w4_split(a2, rs, ly.w_down.split(), ly.w_down.inv, w.x, nullptr, M, D, FH, D,
                                               c.residue_scale, ESMDIFF_F32EPI_RESID_DIV, st));
      }
    } else {   // f32 engine: gate / up rows [M, 2 FH] in memory, SwiGLU as its own pass
      RUN(S_FFN_UP, launch_gemm_f32(w.fh, D, ly.w_up.f32(), w.fgu, nullptr, M, 2 * FH, D, 2 * FH, 2 * FH, 1.f, ESMDIFF_F32EPI_STORE, st));
      RUN(S_FFN_UP, launch_swiglu_f32(w.fgu, w.fmid, M, FH, st));
      RUN(S_FFN_DOWN, launch_gemm_f32(w.fmid, FH, ly.w_down.f32(), w.x, nullptr, M, D, FH, D, D, c.residue_scale, ESMDIFF_F32EPI_RESID_DIV, st));
    }
  }
  if (sp) {
    // head: Linear + bias -> GELU -> LayerNorm -> Linear + bias; the GELU is applied by the LayerNorm as it loads the row
    // (the same erff expression on the same f32 value).  The final norm's f32 rows are kept only for the 128-wide pairwise
    // down-projection, which stays on the exact-f32 kernel.
    RUN(S_LN, launch_layernorm_split(w.x, e->final_ln_w, nullptr, a2, rs, e->has_pair ? w.fh : nullptr, M, D, 0, st));
    RUN(S_HEAD, launch_gemm256w4_split(a2, rs, e->head_w0.split(), e->head_w0.inv, w.fh2, e->head_b0, M, D, D, D, 1.f, ESMDIFF_F32EPI_STORE, st));
    if (e->has_plddt) RUN(S_HEAD, launch_gemm256w4_split(a2, rs, e->pl_w0.split(), e->pl_w0.inv, w.fctx, e->pl_b0, M, D, D, D, 1.f, ESMDIFF_F32EPI_STORE, st));
    if (e->has_pair) RUN(S_HEAD, launch_gemm_f32(w.fh, D, e->pw_down.f32(), w.fpair_qk, nullptr, M, 128, D, 128, 128, 1.f, ESMDIFF_F32EPI_STORE, st));
    RUN(S_LN, launch_layernorm_split(w.fh2, e->head_ln_w, e->head_ln_b, a2, rs, nullptr, M, D, 1, st));
    RUN(S_HEAD, launch_gemm256w4_split(a2, rs, e->head_w3.split(), e->head_w3.inv, logits, e->head_b3, M, e->vocab_pad, D, ld, 1.f, ESMDIFF_F32EPI_STORE, st));
    if (e->has_plddt) {
      RUN(S_LN, launch_layernorm_split(w.fctx, e->pl_ln_w, e->pl_ln_b, a2, rs, nullptr, M, D, 1, st));
      RUN(S_HEAD, launch_gemm256w4_split(a2, rs, e->pl_w3.split(), e->pl_w3.inv, w.pl_logits, e->pl_b3, M, 256, D, e->ld_plddt, 1.f, ESMDIFF_F32EPI_STORE, st));
    }
    return 0;
  }
  RUN(S_LN, launch_layernorm_f32(w.x, e->final_ln_w, nullptr, w.fh, M, D, st));
  RUN(S_HEAD, launch_gemm_f32(w.fh, D, e->head_w0.f32(), w.fh2, e->head_b0, M, D, D, D, D, 1.f, ESMDIFF_F32EPI_BIAS_GELU, st));
  if (e->has_plddt) RUN(S_HEAD, launch_gemm_f32(w.fh, D, e->pl_w0.f32(), w.fctx, e->pl_b0, M, D, D, D, D, 1.f, ESMDIFF_F32EPI_BIAS_GELU, st));
  if (e->has_pair)     // the pairwise confidence head's down-projection (q | k, 64 + 64 columns per token), float32 like the rest
    RUN(S_HEAD, launch_gemm_f32(w.fh, D, e->pw_down.f32(), w.fpair_qk, nullptr, M, 128, D, 128, 128, 1.f, ESMDIFF_F32EPI_STORE, st));
  RUN(S_LN, launch_layernorm_f32(w.fh2, e->head_ln_w, e->head_ln_b, w.fh, M, D, st));
  if (e->has_plddt) RUN(S_LN, launch_layernorm_f32(w.fctx, e->pl_ln_w, e->pl_ln_b, w.fq, M, D, st));
  RUN(S_HEAD, launch_gemm_f32(w.fh, D, e->head_w3.f32(), logits, e->head_b3, M, c.vocab_out, D, ld, c.vocab_out, 1.f, ESMDIFF_F32EPI_STORE, st));
  if (e->has_plddt) RUN(S_HEAD, launch_gemm_f32(w.fq, D, e->pl_w3.f32(), w.pl_logits, e->pl_b3, M, e->plddt_bins, D, e->ld_plddt, e->plddt_bins, 1.f, ESMDIFF_F32EPI_STORE, st));
  return 0;
}

#define T(call) ED_KN(e->f16, call)

// Needed rows: what follows the last block's attention, on the rows the ddpm sampler will read.  Everything from the out-projection
// on is row-wise (GEMMs, LayerNorms, SwiGLU, GELU) and feeds nothing but the logits, and the sampler reads logits only on rows
// that hold MASK (sampler.hip: ddpm_step_kernel leaves every other row at once), so a sub-batch with M' such rows of M runs
//   gather ctx -> out-proj -> add+LayerNorm (x and the pending FFN-down delta through the row list; compact x', h) -> FFN-up ->
//   FFN-down -> final add+LayerNorm -> head GEMM -> head LayerNorm -> head GEMM -> compact logits
// on M' rows.  Exact: a GEMM row does not depend on M (tests/test_gpu_gemm_dispatch.py; no launch here gets a split-K workspace,
// so a row's K order is one pass whatever kernel M' lands on), and the row kernels are one wave per row.  Compact buffers, all free
// once the last attention has run: ctx' in h2, the out-proj delta in q, x' (f32) in qkv, then h / mid / dlt / h2 from their
// starts, and the logits rows at the start of the sub-batch's own logits (read through e->rows_map).
// The host learns M' BEFORE it enqueues these launches and AFTER it has enqueued the rest of the forward: it waits for ev_rows,
// recorded behind launch_mask_row_list at the start of the forward, so what it waits for is at least a whole transformer body
// ahead of the device's queue tail and no queue runs dry.  A sub-batch with M' above 7/8 M (needed_rows_compact) runs plainly,
// one with M' = 0 launches nothing; the sub-batches decide independently and their launches interleave as in forward_16bit.
// The compact FFN-up is timed under the head section: profiling level 2 reports FFN-up launches that are all full-size.
int needed_tail(esmdiff_engine* e, const Part* parts, int np, const Layer& ly, int ld, int L) {
  const esmdiff_config& c = e->cfg;
  const int D = c.d_model, FH = c.ffn_hidden;
  const float inv_scale = 1.0f / c.residue_scale;
  Prof p{e, parts[0].st};
  HIP_TRY(e, hipEventSynchronize(e->ev_rows));
  int rows[4];
  bool cmp[4];
  for (int pi = 0; pi < np; ++pi) {
    const int M = parts[pi].B * L, n = e->rows_count[pi];
    if (n < 0 || n > M) return fail(e, ESMDIFF_E_HIP, "needed rows: sub-batch %d counted %d MASK rows of %d", pi, n, M);
    cmp[pi] = needed_rows_compact(n, M);
    rows[pi] = cmp[pi] ? n : M;
    e->stat_tail_rows += rows[pi];
    e->rows_mapped = e->rows_mapped || cmp[pi];
  }
  // one launch per sub-batch that has rows to run and is of the kind `which`: 'c' compact, 'p' plain, 'a' either.  M: the rows of
  // the launch; the buffers that differ between the two kinds are named here once
#define TAIL(which, section, expr)                                                            \
  do {                                                                                        \
    for (int pi = 0; pi < np; ++pi) {                                                         \
      const Part& w = parts[pi];                                                              \
      const int M = rows[pi];                                                                 \
      const bool k = cmp[pi];                                                                 \
      if (M == 0 || (which == 'c' && !k) || (which == 'p' && k)) continue;                    \
      const int32_t* list = e->rows_list + (int64_t)w.b0 * L;   /* the sub-batch's MASK rows */ \
      float* xc = reinterpret_cast<float*>(w.qkv);              /* compact x' */              \
      const bf16_t* ctx = k ? w.h2 : w.ctx;                                                   \
      bf16_t* dA = k ? w.q : w.dlt2;                                                          \
      float* xf = k ? xc : w.x;                                                               \
      const GemmWorkspace* gws = k ? nullptr : w.gws;                                         \
      (void)list, (void)xc, (void)ctx, (void)dA, (void)xf, (void)gws;                         \
      p.s = w.st;                                                                             \
      RUN(section, expr);                                                                     \
    }                                                                                         \
  } while (0)
  TAIL('c', S_OUT, launch_gather_rows16(w.ctx, list, w.h2, M, D, w.st));
  TAIL('a', S_OUT, T(launch_gemm_bf16(ctx, ly.w_out.w16(), dA, nullptr, M, D, D, D, D, inv_scale, ESMDIFF_EPI_BF16, w.st, gws)));
  TAIL('p', S_LN, T(launch_add_layernorm_bf16(w.x, w.dlt, w.dlt2, 1, ly.ln2_w, ly.ln2_b, w.h, M, D, w.st)));
  TAIL('c', S_LN, T(launch_add_layernorm_rows_bf16(w.x, w.dlt, list, w.q, xc, ly.ln2_w, ly.ln2_b, w.h, M, D, w.st)));
  TAIL('a', k ? S_HEAD : S_FFN_UP,   // (the section: see above)
       T(launch_gemm_bf16(w.h, ly.w_up.w16(), w.mid, nullptr, M, 2 * FH, D, FH, FH, 1.f, ESMDIFF_EPI_SWIGLU_BF16, w.st, gws)));
  TAIL('a', S_FFN_DOWN, T(launch_gemm_bf16(w.mid, ly.w_down.w16(), w.dlt, nullptr, M, D, FH, D, D, inv_scale, ESMDIFF_EPI_BF16, w.st, nullptr)));
  TAIL('a', S_LN, T(launch_add_layernorm_bf16(xf, w.dlt, nullptr, 0, e->final_ln_w, nullptr, w.h, M, D, w.st)));
  TAIL('a', S_HEAD, T(launch_gemm_bf16(w.h, e->head_w0.w16(), w.h2, e->head_b0, M, D, D, D, D, 1.f, ESMDIFF_EPI_BIAS_GELU_BF16, w.st, gws)));
  TAIL('a', S_LN, T(launch_layernorm_bf16_in(w.h2, e->head_ln_w, e->head_ln_b, w.h, M, D, w.st)));
  TAIL('a', S_HEAD, T(launch_gemm_bf16(w.h, e->head_w3.w16(), w.logits, e->head_b3, M, e->vocab_pad, D, ld, c.vocab_out, 1.f, ESMDIFF_EPI_BIAS_F32, w.st, gws)));
#undef TAIL
  e->last_pending_delta = true;
  return 0;
}

// The launch sequence of the 16-bit-operand engines (bf16, or f16: the ed16 build of the same kernel sources, ed_half.h), enqueued
// launch by launch across the sub-batches.  T(launch_x(..)) is a launcher that exists per operand type, chosen by e->f16; a
// launcher spelled plainly exists once (embed, and the float32-grade head's kernels).  needed: the forward goes on with
// needed_tail() after the last block's attention.
int forward_16bit(esmdiff_engine* e, const Part* parts, BatchPlan plan, const float* cond, int ld, int L, bool needed) {
  const esmdiff_config& c = e->cfg;
  const int D = c.d_model, H = c.n_heads, FH = c.ffn_hidden;
  const float inv_scale = 1.0f / c.residue_scale;
  const int np = plan.np;
  Prof p{e, parts[0].st};
  const int cond_stride = e->sigma_rows > 1 ? D : 0;   // esmdiff_forward_logits_sigmas: one conditioning vector per sample
#define EACH(section, expr)                  \
  do {                                       \
    for (int pi = 0; pi < np; ++pi) {        \
      const Part& w = parts[pi];             \
      const int M = w.B * L;                 \
      (void)M;                               \
      p.s = w.st;                            \
      RUN(section, expr);                    \
    }                                        \
  } while (0)

  if (e->kind == 1) {
    EACH(S_EMBED, launch_gather_rows(w.xtok, e->e_struct, w.x, M, D, ESMDIFF_VOCAB, w.st));
  } else {
    EACH(S_EMBED, launch_embed(w.seq, w.xtok, e->e_seq, e->e_struct, e->cvec,
                               cond ? cond + (int64_t)w.b0 * cond_stride : nullptr, w.x, w.B, L, D, w.st, cond_stride));
  }
  // The residual stream x stays f32.  Each branch GEMM (out-proj -> dlt2, FFN-down -> dlt) writes its output, already
  // divided by the residue scale, as a bf16 delta; the LayerNorm kernels add the deltas while they read x anyway, so no
  // GEMM epilogue does a read-modify-write.  x is written back once per block: the attention-side LayerNorm only
  // forms x + dF(previous block) in registers, the FFN-side one forms (x + dF) + dA — the same two f32 additions in the
  // same order as adding them one LayerNorm apart — and stores it.
  const bool geom = e->has_geom && e->frames_B > 0;
  const int VH = e->v_heads;
  bool pending = false;
  // Small batches (a sub-batch of < 1 152 rows, ed::small_max_rows()): the two branch linears leave their products as raw f32 K-slice planes
  // (gemm.hip: launch_gemm_partials) and the LayerNorm that follows sums the planes into x — x += dF before the
  // attention-side LayerNorm, x += dA before the FFN-side one: the same two additions in the same order — so neither a
  // split-K reduce pass nor a bf16 delta round trip runs.  Sub-batches of one forward are all on the same side of the
  // switch or results would depend on how the batch was cut; parts differ by at most one sample, so test part 0's rows.
  const bool small = plan.small;
  GemmPartials PF[4] = {}, PA[4] = {};
  for (int i = 0; i < c.n_layers; ++i) {
    const Layer& ly = e->layers[i];
    if (small) {
      if (pending) EACH(S_LN, T(launch_add_partials_layernorm_bf16(w.x, PF[pi], D, inv_scale, ly.ln1_w, ly.ln1_b, w.h, M, D, w.st)));
      else EACH(S_LN, T(launch_add_layernorm_bf16(w.x, nullptr, nullptr, 0, ly.ln1_w, ly.ln1_b, w.h, M, D, w.st)));
    } else {
      EACH(S_LN, T(launch_add_layernorm_bf16(w.x, pending ? w.dlt : nullptr, nullptr, 0, ly.ln1_w, ly.ln1_b, w.h, M, D, w.st)));
    }
    EACH(S_QKV, T(launch_gemm_bf16(w.h, ly.w_qkv.w16(), w.qkv, nullptr, M, 3 * D, D, 3 * D, 3 * D, 1.f, ESMDIFF_EPI_BF16, w.st, w.gws)));
    EACH(S_QKROPE, T(launch_qk_norm_rope(w.qkv, ly.q_ln_w, ly.k_ln_w, e->rope_cos, e->rope_sin, w.q, w.k, w.B, L, H, w.st)));
    EACH(S_ATTN, T(launch_attention(w.q, w.k, w.qkv, w.ctx, w.B, L, H, w.st, w.lens)));
    if (needed && i == c.n_layers - 1) return needed_tail(e, parts, np, ly, ld, L);   // (regular path, not block 0: forward())
    if (small) EACH(S_OUT, T(launch_gemm_partials(w.ctx, ly.w_out.w16(), w.gws2, M, D, D, w.st, &PA[pi])));
    else EACH(S_OUT, T(launch_gemm_bf16(w.ctx, ly.w_out.w16(), w.dlt2, nullptr, M, D, D, D, D, inv_scale, ESMDIFF_EPI_BF16, w.st, w.gws)));
    const bool geom_here = i == 0 && geom;
    if (geom_here) {
      // x += dA; s = s_norm(x); p = proj(s); geometric attention; dG = out_proj(.) / scale  (block 0 only; the FFN-side
      // LayerNorm below then adds dG instead of dA)
      if (small) EACH(S_LN, T(launch_add_partials_layernorm_bf16(w.x, PA[pi], D, inv_scale, e->g_snorm_w, nullptr, w.h, M, D, w.st)));
      else EACH(S_LN, T(launch_add_layernorm_bf16(w.x, nullptr, w.dlt2, 1, e->g_snorm_w, nullptr, w.h, M, D, w.st)));
      EACH(S_ATTN, T(launch_gemm_bf16(w.h, e->g_proj.w16(), w.gp, nullptr, M, 15 * VH, D, 15 * VH, 15 * VH, 1.f, ESMDIFF_EPI_BF16, w.st, w.gws)));
      EACH(S_ATTN, T(launch_geom_attention(w.gp, w.f_rot, w.f_trans, w.f_mask, e->g_wrot, e->g_wdist, w.gctx, w.B, L, VH, w.st)));
      EACH(S_ATTN, T(launch_gemm_bf16(w.gctx, e->g_out.w16(), w.dlt2, nullptr, M, D, 3 * VH, D, D, inv_scale, ESMDIFF_EPI_BF16, w.st, w.gws)));
    }
    if (small && !geom_here) {
      EACH(S_LN, T(launch_add_partials_layernorm_bf16(w.x, PA[pi], D, inv_scale, ly.ln2_w, ly.ln2_b, w.h, M, D, w.st)));
    } else if (small) {  // x already holds x + dF + dA; the geometric branch came back as a bf16 delta
      EACH(S_LN, T(launch_add_layernorm_bf16(w.x, nullptr, w.dlt2, 1, ly.ln2_w, ly.ln2_b, w.h, M, D, w.st)));
    } else {
      EACH(S_LN, T(launch_add_layernorm_bf16(w.x, pending ? w.dlt : nullptr, w.dlt2, 1, ly.ln2_w, ly.ln2_b, w.h, M, D, w.st)));
    }
    EACH(S_FFN_UP, T(launch_gemm_bf16(w.h, ly.w_up.w16(), w.mid, nullptr, M, 2 * FH, D, FH, FH, 1.f, ESMDIFF_EPI_SWIGLU_BF16, w.st, w.gws)));
    if (small) EACH(S_FFN_DOWN, T(launch_gemm_partials(w.mid, ly.w_down.w16(), w.gws, M, D, FH, w.st, &PF[pi])));
    // (no split-K workspace here: on the regular path a row's K order must not depend on how many rows its sub-batch has —
    //  with the workspace a part below 1 152 rows next to a larger one, e.g. B = 9 at L_tok = 258 cut 4 + 5, summed its FFN-down
    //  in 8 slices and the other part in one pass, and step-0 sharing / batch composition changed the last bit: ADVICE r03)
    else EACH(S_FFN_DOWN, T(launch_gemm_bf16(w.mid, ly.w_down.w16(), w.dlt, nullptr, M, D, FH, D, D, inv_scale, ESMDIFF_EPI_BF16, w.st, nullptr)));
    pending = true;
  }
  e->last_pending_delta = !small && pending;
  if (e->head_split) {
    // f32-grade head on the bf16 body (esmdiff_config.head_precision = 1): final LayerNorm of the f32 residual stream (plus
    // the last FFN-down delta, which the regular path keeps outside x) -> Linear + bias -> GELU -> LayerNorm -> Linear + bias,
    // LayerNorms in the strict path's arithmetic, linears as three f16 MFMA passes over split rows (gemm_split.hip)
    if (small && pending) EACH(S_LN, T(launch_add_partials_layernorm_bf16(w.x, PF[pi], D, inv_scale, e->final_ln_w, nullptr, w.h, M, D, w.st)));  // x += dF
    EACH(S_LN, launch_layernorm_split(w.x, e->final_ln_w, nullptr, w.a2, w.rs, nullptr, M, D, 0, w.st,
                                      (!small && pending) ? w.dlt : nullptr, e->f16 ? 1 : 0));
    EACH(S_HEAD, launch_gemm256w4_split(w.a2, w.rs, e->head_w0.split(), e->head_w0.inv, w.fh2, e->head_b0, M, D, D, D, 1.f, ESMDIFF_F32EPI_STORE, w.st));
    EACH(S_LN, launch_layernorm_split(w.fh2, e->head_ln_w, e->head_ln_b, w.a2, w.rs, nullptr, M, D, 1, w.st));
    EACH(S_HEAD, launch_gemm256w4_split(w.a2, w.rs, e->head_w3.split(), e->head_w3.inv, w.logits, e->head_b3, M, e->vocab_pad, D, ld, 1.f, ESMDIFF_F32EPI_STORE, w.st));
    return 0;
  }
  if (small && pending) EACH(S_LN, T(launch_add_partials_layernorm_bf16(w.x, PF[pi], D, inv_scale, e->final_ln_w, nullptr, w.h, M, D, w.st)));
  else EACH(S_LN, T(launch_add_layernorm_bf16(w.x, pending ? w.dlt : nullptr, nullptr, 0, e->final_ln_w, nullptr, w.h, M, D, w.st)));
  EACH(S_HEAD, T(launch_gemm_bf16(w.h, e->head_w0.w16(), w.h2, e->head_b0, M, D, D, D, D, 1.f, ESMDIFF_EPI_BIAS_GELU_BF16, w.st, w.gws)));
  // decoder: the pLDDT head reads the same normalised hidden state (w.h) before the structure head's LayerNorm reuses it;
  // its intermediates live in ctx / q, which are free after the last block
  if (e->has_plddt) EACH(S_HEAD, T(launch_gemm_bf16(w.h, e->pl_w0.w16(), w.ctx, e->pl_b0, M, D, D, D, D, 1.f, ESMDIFF_EPI_BIAS_GELU_BF16, w.st, w.gws)));
  // ... and so does the pairwise head's down-projection (q | k, 64 + 64 columns per token)
  if (e->has_pair) EACH(S_HEAD, T(launch_gemm_bf16(w.h, e->pw_down.w16(), w.pair_qk, nullptr, M, 128, D, 128, 128, 1.f, ESMDIFF_EPI_BF16, w.st, w.gws)));
  EACH(S_LN, T(launch_layernorm_bf16_in(w.h2, e->head_ln_w, e->head_ln_b, w.h, M, D, w.st)));
  if (e->has_plddt) EACH(S_LN, T(launch_layernorm_bf16_in(w.ctx, e->pl_ln_w, e->pl_ln_b, w.q, M, D, w.st)));
  EACH(S_HEAD, T(launch_gemm_bf16(w.h, e->head_w3.w16(), w.logits, e->head_b3, M, e->vocab_pad, D, ld, c.vocab_out, 1.f, ESMDIFF_EPI_BIAS_F32, w.st, w.gws)));
  if (e->has_plddt) EACH(S_HEAD, T(launch_gemm_bf16(w.q, e->pl_w3.w16(), w.pl_logits, e->pl_b3, M, 128, D, e->ld_plddt, e->plddt_bins, 1.f, ESMDIFF_EPI_BIAS_F32, w.st, w.gws)));
#undef EACH
#undef T
  return 0;
}

// what esmdiff_get_embeddings / esmdiff_get_sequence_logits answer after a forward that went on with the MASK rows only
const char kStaleRows[] =
    "the last forward ran inside esmdiff_ddpm_sample on the rows that hold MASK only (ESMDIFF_OPT_NEEDED_ROWS): the other rows' "
    "hidden state is stale; run a full forward (esmdiff_forward_logits) first, or set the option to 0";

}  // namespace

// Step-0 sharing: the number of leading samples whose forward gives, bit for bit, the logits every sample of an
// all-identical batch of B would get — a sub-batch that takes the same (regular) dispatch path as the whole batch
// (tests: test_logits_across_dispatch_paths) — or B when nothing can be saved.
int eng::shared_forward_batch(const esmdiff_engine* e, int B, int L) {
  if (e->strict) return 1;                       // every row's result is independent of the batch (fixed K order, one path)
  if (plan_small(e, B, L)) return B;             // small-batch path: the plane count is fixed, but keep it simple: no sharing
  for (int b = 1; b < B; ++b)
    if (!plan_small(e, b, L) && (int64_t)b * L >= ed::small_max_rows()) return b;
  return B;
}

// The whole network: tokens -> f32 logits [M, ld].
//
// Samples are independent, so a large batch is run as two sub-batches on two HIP streams (the caller's and one
// engine-owned stream, forked and joined with events, launches interleaved layer by layer).  Every GEMM is a
// persistent one-workgroup-per-CU kernel whose last round leaves CUs idle (N=1536: 606 tiles on 256 CUs = 2.37
// rounds); with two independent launch queues the hardware scheduler fills those tails and the gaps around the
// small LayerNorm / rotary / attention kernels with the other sub-batch's work (measured: -4.4 % per forward).
// When (r02, re-measured over B at L_tok = 60 / 128 / 258, ms per batch one stream / two):
//   * from 2 200 tokens up.  r01 kept one stream between 6 400 and 12 288 tokens because the halves' N = 1536 linears fell
//     below the 128-tile switch onto the slower 128-column kernel; with the r02 dispatch rule (gemm.hip: 256x256 from 72
//     tiles at >= 12 row tiles) two streams win or tie there too — L_tok = 258, samples/s: B = 26 46.7 / 47.9, 28 45.9 /
//     47.2, 32 47.7 / 48.1, 36 51.2 / 52.3, 40 52.0 / 52.2, 44 46.8 / 52.1, 48 47.8 / 53.1, 100 52.3 / 55.0;
//   * NOT between ~1 100 and 2 200 tokens: the halves would drop onto the small-batch path (< 1 152 rows), which per row
//     is slower than the regular path is at 1 200 - 2 000 rows — L_tok = 60: B = 24 202 / 226 ms, 32 230 / 266, 40 276 / 266;
//     L_tok = 128: B = 12 211 / 237, 16 241 / 262, 20 289 / 276; L_tok = 258: B = 5 205 / 227, 6 216 / 243, 7 238 / 255,
//     8 278 / 271;
//   * 768 .. 1 024 tokens at B >= 8: everything is small either way and two queues overlap the launch floors — L_tok = 60
//     B = 16 185 / 167 ms, L_tok = 128 B = 8 188 / 176; below ~700 tokens the halves' GEMMs each stream the whole weight
//     matrix for half the rows and lose (B = 4 at L_tok = 60: 87.0 / 95.8 ms), and B = 3 at L_tok = 258 cuts into 1 + 2.
int eng::forward(esmdiff_engine* e, const int64_t* seq, const int64_t* xtok, const float* t_freq_dev, float* logits,
                 int ld, int B, int L, hipStream_t st, bool needed_rows) {
  e->last_B = B;
  e->last_L = L;
  e->last_pending_delta = false;
  e->rows_mapped = false;
  e->stat_forwards += 1;
  e->stat_rows += (int64_t)B * L;
  if (e->has_geom && e->frames_B > 0 && (e->frames_B != B || e->frames_L != L))
    return fail(e, ESMDIFF_E_INVALID, "frames were set for B=%d L=%d, forward called with B=%d L=%d", e->frames_B, e->frames_L, B, L);
  const int D = e->cfg.d_model;
  Prof p{e, st};
  const float* cond = nullptr;
  // sigma_embedder runs whenever its weights were loaded and the caller hands a sinusoid: with time conditioning off the
  // reference still adds sigma_embedder(0) (model.py:466-471 with _process_sigma zeroing sigma, :535-541), and the
  // host passes the sinusoid of 0 for that case
  if (t_freq_dev && e->sig_w1) {
    RUN(S_EMBED, launch_sigma_mlp(t_freq_dev, e->sig_w1, e->sig_b1, e->sig_w2, e->sig_b2, e->sig_hidden, e->cond, e->cfg.freq_dim, D, st,
                                  e->sigma_rows));
    cond = e->cond;
  }
  // profiling == 1 (per-section breakdown) keeps one stream so that the sections do not overlap
  const BatchPlan plan = plan_batch(e, B, L);
  Part parts[4];
  cut_batch(e, parts, plan.np, seq, xtok, logits, ld, B, L, st);
  // needed rows: the regular path of a 16-bit engine whose only head is the structure head; needed_tail() names the buffers it
  // takes over (the extra heads' intermediates live in two of them).  Not under stream capture: the host wait cannot be captured.
  bool needed = needed_rows && e->needed_rows && e->rows_count && !e->head_split && !plan.small && !e->has_plddt && !e->has_pair &&
                e->cfg.n_layers >= 2;
  if (needed) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    HIP_TRY(e, hipStreamIsCapturing(st, &cs));
    needed = cs == hipStreamCaptureStatusNone;
  }
  if (needed) {   // the MASK rows of each sub-batch, counted for the host: first on the caller's stream, the queues fork behind it
    HIP_TRY(e, launch_mask_row_list(xtok, B, L, plan.np, e->rows_list, e->rows_map, e->rows_count, st));
    HIP_TRY(e, hipEventRecord(e->ev_rows, st));
  }
  if (int r = fork_streams(e, st, plan.np)) return r;
  if (e->strict) {   // part after part (per-sample sigmas: the part's first conditioning row)
    for (int pi = 0; pi < plan.np; ++pi)
      if (int r = strict_part(e, parts[pi], cond && e->sigma_rows > 1 ? cond + (int64_t)parts[pi].b0 * D : cond, ld, L)) return r;
  } else if (int r = forward_16bit(e, parts, plan, cond, ld, L, needed)) {
    return r;
  }
  if (!needed) e->stat_tail_rows += (int64_t)B * L;
  return join_streams(e, st, plan.np);
}

extern "C" {

int esmdiff_describe_plan(const esmdiff_engine* e, int32_t B, int32_t L, char* buf, int32_t cap) {
  if (!e || B <= 0 || L <= 0) return ESMDIFF_E_INVALID;
  const esmdiff_config& c = e->cfg;
  const int D = c.d_model, FH = c.ffn_hidden;
  char tmp[1536];
  int n = 0;
  // (every piece is appended through `add`, which never writes past tmp and keeps counting the length the full text needs)
  auto room = [&]() { return n < (int)sizeof tmp ? sizeof tmp - (size_t)n : (size_t)0; };
  auto at = [&]() { return tmp + (n < (int)sizeof tmp ? n : (int)sizeof tmp - 1); };
  const char* prec = e->strict ? (e->split ? "f32_split" : "f32") : (e->f16 ? "f16" : "bf16");
  n += snprintf(at(), room(), "precision=%s head=%s B=%d L=%d", prec, (e->strict || e->head_split) ? "f32-grade" : prec, B, L);
  const int np = plan_parts(e, B, L);
  if (e->strict) {
    const int64_t tokens = (int64_t)B * L;
    n += snprintf(at(), room(), " streams=%d path=%s k_sliced_small_batches=%d", np,
                  e->split ? "split(3 f16 MFMA passes, 256x256w4)" : "strict(f32 MFMA)", e->sk_parts && tokens <= kSplitkMaxRows ? 1 : 0);
  } else {
    const bool small = plan_small(e, B, L);
    const int m0 = (int)((int64_t)B / np) * L;
    char g1[32], g2[32], g3[32], g4[32];
    const size_t wsf = e->gemm_ws[0].partial ? e->gemm_ws[0].partial_floats : 0;
    ed::describe_gemm(m0, 3 * D, D, wsf, g1, sizeof g1);
    ed::describe_gemm(m0, D, D, wsf, g2, sizeof g2);
    ed::describe_gemm(m0, 2 * FH, D, wsf, g3, sizeof g3);
    ed::describe_gemm(m0, D, FH, 0, g4, sizeof g4);
    n += snprintf(at(), room(), " streams=%d rows_per_stream=%d path=%s", np, m0, small ? "small-batch(K-slice planes summed by the LayerNorm)" : "regular");
    if (small)
      n += snprintf(at(), room(), " gemm[qkv]=%s gemm[out]=128x*/S%d gemm[ffn_up]=%s gemm[ffn_down]=128x*/S%d", g1, ed::gemm_partial_splits(D, D), g3,
                    ed::gemm_partial_splits(D, FH));
    else
      n += snprintf(at(), room(), " gemm[qkv]=%s gemm[out]=%s gemm[ffn_up]=%s gemm[ffn_down]=%s", g1, g2, g3, g4);
  }
  n += snprintf(at(), room(), " step0_sharing=%d final_skip=%d small_max_rows=%d needed_rows=%d", e->step0_share, e->final_skip,
                ed::small_max_rows(), e->needed_rows);
  if (e->lens_B == B) {   // ragged batch (esmdiff_set_lengths): attention walks each sample's own keys
    int64_t valid = 0;
    for (int b = 0; b < B; ++b) valid += std::min<int64_t>(e->lens_host[b], L);
    n += snprintf(at(), room(), " ragged=1 valid_tokens=%lld padded_tokens=%lld", (long long)valid, (long long)B * L);
  }
  if (buf && cap > 0) snprintf(buf, (size_t)cap, "%s", tmp);
  return n;
}

int esmdiff_shared_forward_batch(const esmdiff_engine* e, int32_t B, int32_t L) {
  if (!e || B <= 0 || L <= 0 || B > e->cfg.max_batch || L > e->cfg.max_len) return ESMDIFF_E_INVALID;
  return shared_forward_batch(e, B, L);
}

int esmdiff_forward_logits(esmdiff_engine* e, const int64_t* seq, const int64_t* x, const float* t_freq,
                           float* logits_out, int32_t ld_logits, int32_t B, int32_t L, void* stream) {
  if (!e) return ESMDIFF_E_INVALID;
  if (int r = check_not_decoder(e)) return r;
  if (!seq || !x || !logits_out) return fail(e, ESMDIFF_E_INVALID, "null pointer");
  if (ld_logits < e->cfg.vocab_out || (ld_logits & 3)) return fail(e, ESMDIFF_E_INVALID, "ld_logits (%d) must be >= vocab (%d) rounded up to a multiple of 4", ld_logits, e->cfg.vocab_out);
  if (int r = check_bl(e, B, L)) return r;
  if (int r = check_lens(e, B, L)) return r;
  if ((e->split || e->head_split) && ld_logits < e->vocab_pad) {
    // the split head GEMM writes whole padded rows: run into the engine's own [M, vocab_pad] buffer, copy the valid columns
    if (int r = forward(e, seq, x, t_freq, e->logits, e->ld_logits, B, L, (hipStream_t)stream)) return r;
    HIP_TRY(e, hipMemcpy2DAsync(logits_out, (size_t)ld_logits * 4, e->logits, (size_t)e->ld_logits * 4, (size_t)e->cfg.vocab_out * 4,
                                (size_t)B * L, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
  }
  return forward(e, seq, x, t_freq, logits_out, ld_logits, B, L, (hipStream_t)stream);
}

// (esmdiff_hip_test.h) the forward as esmdiff_ddpm_sample runs it, into the engine's own logits, then the MASK rows to the caller's
int esmdiff_forward_logits_needed(esmdiff_engine* e, const int64_t* seq, const int64_t* x, const float* t_freq,
                                  float* logits_out, int32_t ld_logits, int32_t B, int32_t L, void* stream) {
  if (!e) return ESMDIFF_E_INVALID;
  if (int r = check_not_decoder(e)) return r;
  if (!seq || !x || !logits_out) return fail(e, ESMDIFF_E_INVALID, "null pointer");
  if (ld_logits < e->cfg.vocab_out) return fail(e, ESMDIFF_E_INVALID, "ld_logits (%d) below the vocabulary (%d)", ld_logits, e->cfg.vocab_out);
  if (int r = check_bl(e, B, L)) return r;
  if (int r = check_lens(e, B, L)) return r;
  hipStream_t st = (hipStream_t)stream;
  if (int r = forward(e, seq, x, t_freq, e->logits, e->ld_logits, B, L, st, true)) return r;
  HIP_TRY(e, launch_copy_masked_logits(x, e->logits, e->ld_logits, e->rows_mapped ? e->rows_map : nullptr, logits_out, ld_logits,
                                       e->cfg.vocab_out, B * L, st));
  return 0;
}

int esmdiff_forward_logits_sigmas(esmdiff_engine* e, const int64_t* seq, const int64_t* x, const float* t_freq,
                                  float* logits_out, int32_t ld_logits, int32_t B, int32_t L, void* stream) {
  if (!e) return ESMDIFF_E_INVALID;
  if (!t_freq) return fail(e, ESMDIFF_E_INVALID, "null pointer (t_freq: [B, freq_dim], one sinusoid per sample)");
  if (!e->sig_w1) return fail(e, ESMDIFF_E_INVALID, "per-sample sigmas need the sigma_embedder weights");
  if (B <= 0 || B > e->cfg.max_batch) return fail(e, ESMDIFF_E_INVALID, "B = %d outside 1..max_batch (%d)", B, e->cfg.max_batch);
  e->sigma_rows = B;
  const int r = esmdiff_forward_logits(e, seq, x, t_freq, logits_out, ld_logits, B, L, stream);
  e->sigma_rows = 1;
  return r;
}

int esmdiff_get_embeddings(esmdiff_engine* e, float* out, int32_t B, int32_t L, void* stream) {
  if (!e) return ESMDIFF_E_INVALID;
  if (!out) return fail(e, ESMDIFF_E_INVALID, "null pointer");
  if (B != e->last_B || L != e->last_L || B <= 0)
    return fail(e, ESMDIFF_E_INVALID, "embeddings of a (%d, %d) forward requested, the last forward was (%d, %d)", B, L, e->last_B, e->last_L);
  if (e->rows_mapped) return fail(e, ESMDIFF_E_INVALID, "%s", kStaleRows);
  hipStream_t st = (hipStream_t)stream;
  const size_t M = (size_t)B * L, D = e->cfg.d_model;
  HIP_TRY(e, hipMemcpyAsync(out, e->x, M * D * sizeof(float), hipMemcpyDeviceToDevice, st));
  // regular bf16 path: the last block's FFN-down delta is added by the final add+LayerNorm in registers; add it here the
  // same way (out = out + dF, one f32 addition per element; the normalised row goes to a scratch buffer nobody reads)
  if (e->last_pending_delta)
    HIP_TRY(e, ED_KN(e->f16, launch_add_layernorm_bf16(out, e->dlt, nullptr, 1, e->final_ln_w, nullptr, e->q, (int)M, (int)D, st)));
  return 0;
}

int esmdiff_get_sequence_logits(esmdiff_engine* e, float* out, int32_t ld_out, int32_t B, int32_t L, void* stream) {
  if (!e) return ESMDIFF_E_INVALID;
  if (e->kind != 0 || !e->has_plddt) return fail(e, ESMDIFF_E_MISSING, "no output_heads.sequence_head.* tensors were in the weight table");
  if (!out || ld_out < e->plddt_bins) return fail(e, ESMDIFF_E_INVALID, "bad output");
  if (B != e->last_B || L != e->last_L || B <= 0)
    return fail(e, ESMDIFF_E_INVALID, "sequence logits of a (%d, %d) forward requested, the last forward was (%d, %d)", B, L, e->last_B, e->last_L);
  if (e->rows_mapped) return fail(e, ESMDIFF_E_INVALID, "%s", kStaleRows);
  HIP_TRY(e, hipMemcpy2DAsync(out, (size_t)ld_out * 4, e->pl_logits, (size_t)e->ld_plddt * 4, (size_t)e->plddt_bins * 4, (size_t)B * L,
                              hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return 0;
}

}  // extern "C"

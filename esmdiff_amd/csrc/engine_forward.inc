// engine_forward.inc — the launch sequence of one forward of the 16-bit-operand engine (bf16 or f16), included twice by
// engine_forward.hip with KN = ed (the bf16 build of the kernels) and KN = ed16 (the f16 build of the same sources, ed_half.h); the
// split head (gemm_split.hip) and the few f32-only kernels exist once and resolve through either namespace's declarations.
static int ED_FWD_NAME(esmdiff_engine* e, const int64_t* seq, const int64_t* xtok, const float* t_freq_dev, float* logits,
                       int ld, int B, int L, hipStream_t st) {
  const esmdiff_config& c = e->cfg;
  const int D = c.d_model, H = c.n_heads, FH = c.ffn_hidden;
  const float inv_scale = 1.0f / c.residue_scale;
  Prof p{e, st};

  const float* cond = nullptr;
  // sigma_embedder runs whenever its weights were loaded and the caller hands a sinusoid: with time conditioning off the
  // reference still adds sigma_embedder(0) (model.py:466-471 with _process_sigma zeroing sigma, :535-541), and the
  // host passes the sinusoid of 0 for that case
  if (t_freq_dev && e->sig_w1) {
    RUN(S_EMBED, ed::launch_sigma_mlp(t_freq_dev, e->sig_w1, e->sig_b1, e->sig_w2, e->sig_b2, e->sig_hidden, e->cond,
                                  c.freq_dim, D, st, e->sigma_rows));
    cond = e->cond;
  }
  const int cond_stride = e->sigma_rows > 1 ? D : 0;   // esmdiff_forward_logits_sigmas: one conditioning vector per sample
  // profiling == 1 (per-section breakdown) keeps one stream so that the sections do not overlap
  Part parts[4];
  const int np = plan_parts(e, B, L);
  e->stat_forwards += 1;
  e->stat_rows += (int64_t)B * L;
  for (int pi = 0; pi < np; ++pi) {
    const int b0 = (int)((int64_t)B * pi / np), b1 = (int)((int64_t)B * (pi + 1) / np);
    parts[pi] = make_part(e, seq, xtok, logits, ld, b0, b1 - b0, L, pi == 0 ? st : e->side[pi - 1], pi);
  }
  if (int r = fork_streams(e, st, np)) return r;
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
    EACH(S_EMBED, ed::launch_gather_rows(w.xtok, e->e_struct, w.x, M, D, ESMDIFF_VOCAB, w.st));
  } else {
    EACH(S_EMBED, ed::launch_embed(w.seq, w.xtok, e->e_seq, e->e_struct, e->cvec,
                                   cond ? cond + (int64_t)w.b0 * cond_stride : nullptr, w.x, w.B, L, D, w.st, cond_stride));
  }
  // The residual stream x stays f32.  Each branch GEMM (out-proj -> dlt2, FFN-down -> dlt) writes its output, already
  // divided by the residue scale, as a bf16 delta; the LayerNorm kernels add the deltas while they read x anyway, so no
  // GEMM epilogue does a read-modify-write.  x is written back once per block: the attention-side LayerNorm only
  // forms x + dF(previous block) in registers, the FFN-side one forms (x + dF) + dA — the same two f32 additions in the
  // same order as adding them one LayerNorm apart — and stores it.
  const bool geom = e->has_geom && e->frames_B > 0;
  if (geom && (e->frames_B != B || e->frames_L != L))
    return fail(e, ESMDIFF_E_INVALID, "frames were set for B=%d L=%d, forward called with B=%d L=%d", e->frames_B, e->frames_L, B, L);
  const int VH = e->v_heads;
  bool pending = false;
  // Small batches (a sub-batch of < 1 152 rows, ed::small_max_rows()): the two branch linears leave their products as raw f32 K-slice planes
  // (gemm.hip: KN::launch_gemm_partials) and the LayerNorm that follows sums the planes into x — x += dF before the
  // attention-side LayerNorm, x += dA before the FFN-side one: the same two additions in the same order — so neither a
  // split-K reduce pass nor a bf16 delta round trip runs.  Sub-batches of one forward are all on the same side of the
  // switch or results would depend on how the batch was cut; parts differ by at most one sample, so test part 0's rows.
  const bool small = plan_small(e, B, L);
  KN::GemmPartials PF[4] = {}, PA[4] = {};
  for (int i = 0; i < c.n_layers; ++i) {
    const Layer& ly = e->layers[i];
    if (small) {
      if (pending) EACH(S_LN, KN::launch_add_partials_layernorm_bf16(w.x, PF[pi], D, inv_scale, ly.ln1_w, ly.ln1_b, w.h, M, D, w.st));
      else EACH(S_LN, KN::launch_add_layernorm_bf16(w.x, nullptr, nullptr, 0, ly.ln1_w, ly.ln1_b, w.h, M, D, w.st));
    } else {
      EACH(S_LN, KN::launch_add_layernorm_bf16(w.x, pending ? w.dlt : nullptr, nullptr, 0, ly.ln1_w, ly.ln1_b, w.h, M, D, w.st));
    }
    EACH(S_QKV, KN::launch_gemm_bf16(w.h, ly.w_qkv.w16(), w.qkv, nullptr, M, 3 * D, D, 3 * D, 3 * D, 1.f, ESMDIFF_EPI_BF16, w.st, w.gws));
    EACH(S_QKROPE, KN::launch_qk_norm_rope(w.qkv, ly.q_ln_w, ly.k_ln_w, e->rope_cos, e->rope_sin, w.q, w.k, w.B, L, H, w.st));
    EACH(S_ATTN, KN::launch_attention(w.q, w.k, w.qkv, w.ctx, w.B, L, H, w.st, w.lens));
    if (small) EACH(S_OUT, KN::launch_gemm_partials(w.ctx, ly.w_out.w16(), w.gws2, M, D, D, w.st, &PA[pi]));
    else EACH(S_OUT, KN::launch_gemm_bf16(w.ctx, ly.w_out.w16(), w.dlt2, nullptr, M, D, D, D, D, inv_scale, ESMDIFF_EPI_BF16, w.st, w.gws));
    const bool geom_here = i == 0 && geom;
    if (geom_here) {
      // x += dA; s = s_norm(x); p = proj(s); geometric attention; dG = out_proj(.) / scale  (block 0 only; the FFN-side
      // LayerNorm below then adds dG instead of dA)
      if (small) EACH(S_LN, KN::launch_add_partials_layernorm_bf16(w.x, PA[pi], D, inv_scale, e->g_snorm_w, nullptr, w.h, M, D, w.st));
      else EACH(S_LN, KN::launch_add_layernorm_bf16(w.x, nullptr, w.dlt2, 1, e->g_snorm_w, nullptr, w.h, M, D, w.st));
      EACH(S_ATTN, KN::launch_gemm_bf16(w.h, e->g_proj.w16(), w.gp, nullptr, M, 15 * VH, D, 15 * VH, 15 * VH, 1.f, ESMDIFF_EPI_BF16, w.st, w.gws));
      EACH(S_ATTN, KN::launch_geom_attention(w.gp, w.f_rot, w.f_trans, w.f_mask, e->g_wrot, e->g_wdist, w.gctx, w.B, L, VH, w.st));
      EACH(S_ATTN, KN::launch_gemm_bf16(w.gctx, e->g_out.w16(), w.dlt2, nullptr, M, D, 3 * VH, D, D, inv_scale, ESMDIFF_EPI_BF16, w.st, w.gws));
    }
    if (small && !geom_here) {
      EACH(S_LN, KN::launch_add_partials_layernorm_bf16(w.x, PA[pi], D, inv_scale, ly.ln2_w, ly.ln2_b, w.h, M, D, w.st));
    } else if (small) {  // x already holds x + dF + dA; the geometric branch came back as a bf16 delta
      EACH(S_LN, KN::launch_add_layernorm_bf16(w.x, nullptr, w.dlt2, 1, ly.ln2_w, ly.ln2_b, w.h, M, D, w.st));
    } else {
      EACH(S_LN, KN::launch_add_layernorm_bf16(w.x, pending ? w.dlt : nullptr, w.dlt2, 1, ly.ln2_w, ly.ln2_b, w.h, M, D, w.st));
    }
    EACH(S_FFN_UP, KN::launch_gemm_bf16(w.h, ly.w_up.w16(), w.mid, nullptr, M, 2 * FH, D, FH, FH, 1.f, ESMDIFF_EPI_SWIGLU_BF16, w.st, w.gws));
    if (small) EACH(S_FFN_DOWN, KN::launch_gemm_partials(w.mid, ly.w_down.w16(), w.gws, M, D, FH, w.st, &PF[pi]));
    // (no split-K workspace here: on the regular path a row's K order must not depend on how many rows its sub-batch has —
    //  with the workspace a part below 1 152 rows next to a larger one, e.g. B = 9 at L_tok = 258 cut 4 + 5, summed its FFN-down
    //  in 8 slices and the other part in one pass, and step-0 sharing / batch composition changed the last bit: ADVICE r03)
    else EACH(S_FFN_DOWN, KN::launch_gemm_bf16(w.mid, ly.w_down.w16(), w.dlt, nullptr, M, D, FH, D, D, inv_scale, ESMDIFF_EPI_BF16, w.st, nullptr));
    pending = true;
  }
  e->last_pending_delta = !small && pending;
  if (e->head_split) {
    // f32-grade head on the bf16 body (esmdiff_config.head_precision = 1): final LayerNorm of the f32 residual stream (plus
    // the last FFN-down delta, which the regular path keeps outside x) -> Linear + bias -> GELU -> LayerNorm -> Linear + bias,
    // LayerNorms in the strict path's arithmetic, linears as three f16 MFMA passes over split rows (gemm_split.hip)
    if (small && pending) EACH(S_LN, KN::launch_add_partials_layernorm_bf16(w.x, PF[pi], D, inv_scale, e->final_ln_w, nullptr, w.h, M, D, w.st));  // x += dF
    EACH(S_LN, ed::launch_layernorm_split(w.x, e->final_ln_w, nullptr, w.a2, w.rs, nullptr, M, D, 0, w.st,
                                      (!small && pending) ? w.dlt : nullptr, e->f16 ? 1 : 0));
    EACH(S_HEAD, ed::launch_gemm256w4_split(w.a2, w.rs, e->head_w0.split(), e->head_w0.inv, w.fh2, e->head_b0, M, D, D, D, 1.f, ESMDIFF_F32EPI_STORE, w.st));
    EACH(S_LN, ed::launch_layernorm_split(w.fh2, e->head_ln_w, e->head_ln_b, w.a2, w.rs, nullptr, M, D, 1, w.st));
    EACH(S_HEAD, ed::launch_gemm256w4_split(w.a2, w.rs, e->head_w3.split(), e->head_w3.inv, w.logits, e->head_b3, M, e->vocab_pad, D, ld, 1.f, ESMDIFF_F32EPI_STORE, w.st));
    return join_streams(e, st, np);
  }
  if (small && pending) EACH(S_LN, KN::launch_add_partials_layernorm_bf16(w.x, PF[pi], D, inv_scale, e->final_ln_w, nullptr, w.h, M, D, w.st));
  else EACH(S_LN, KN::launch_add_layernorm_bf16(w.x, pending ? w.dlt : nullptr, nullptr, 0, e->final_ln_w, nullptr, w.h, M, D, w.st));
  EACH(S_HEAD, KN::launch_gemm_bf16(w.h, e->head_w0.w16(), w.h2, e->head_b0, M, D, D, D, D, 1.f, ESMDIFF_EPI_BIAS_GELU_BF16, w.st, w.gws));
  // decoder: the pLDDT head reads the same normalised hidden state (w.h) before the structure head's LayerNorm reuses it;
  // its intermediates live in ctx / q, which are free after the last block
  if (e->has_plddt) EACH(S_HEAD, KN::launch_gemm_bf16(w.h, e->pl_w0.w16(), w.ctx, e->pl_b0, M, D, D, D, D, 1.f, ESMDIFF_EPI_BIAS_GELU_BF16, w.st, w.gws));
  // ... and so does the pairwise head's down-projection (q | k, 64 + 64 columns per token)
  if (e->has_pair) EACH(S_HEAD, KN::launch_gemm_bf16(w.h, e->pw_down.w16(), e->pair_qk + (int64_t)w.b0 * L * 128, nullptr, M, 128, D, 128, 128, 1.f, ESMDIFF_EPI_BF16, w.st, w.gws));
  EACH(S_LN, KN::launch_layernorm_bf16_in(w.h2, e->head_ln_w, e->head_ln_b, w.h, M, D, w.st));
  if (e->has_plddt) EACH(S_LN, KN::launch_layernorm_bf16_in(w.ctx, e->pl_ln_w, e->pl_ln_b, w.q, M, D, w.st));
  EACH(S_HEAD, KN::launch_gemm_bf16(w.h, e->head_w3.w16(), w.logits, e->head_b3, M, e->vocab_pad, D, ld, c.vocab_out, 1.f, ESMDIFF_EPI_BIAS_F32, w.st, w.gws));
  if (e->has_plddt) EACH(S_HEAD, KN::launch_gemm_bf16(w.q, e->pl_w3.w16(), w.pl_logits, e->pl_b3, M, 128, D, e->ld_plddt, e->plddt_bins, 1.f, ESMDIFF_EPI_BIAS_F32, w.st, w.gws));
#undef EACH
  return join_streams(e, st, np);
}


// engine_sample.hip — the entries that run forwards in a loop or consume logits: the ddpm and gibbs steps and samplers (with
// step-0 sharing and the final-skip sub-batch), the forward noising q_xt and the NELBO.  Forwards go through eng::forward.
#include "engine.h"

using namespace ed;
using namespace eng;

namespace {

// Step-0 sharing (esmdiff_set_step0_sharing).  Returns in *shared the number of leading samples whose forward serves the
// whole batch at step 0, or 0 when the batch is run in full: the option is off, nothing would be saved, or — checked ON THE
// DEVICE, not taken from the caller — the rows of seq / x are not all identical.  One 4-byte read-back per sampling call.
int step0_shared_batch(esmdiff_engine* e, const int64_t* seq, const int64_t* x, int B, int L, hipStream_t st, int* shared) {
  *shared = 0;
  if (!e->step0_share || B < 2) return 0;
  if (e->frames_B != 0) return 0;   // coordinate conditioning: frames may differ per sample and are not compared below
  if (e->lens_B != 0) return 0;     // ragged batch: rows of different lengths are never shared
  const int bs = shared_forward_batch(e, B, L);
  if (bs >= B) return 0;
  HIP_TRY(e, launch_rows_identical(seq, x, B, L, e->flag_dev, st));
  int32_t h = 0;
  HIP_TRY(e, hipMemcpyAsync(&h, e->flag_dev, sizeof h, hipMemcpyDeviceToHost, st));
  HIP_TRY(e, hipStreamSynchronize(st));
  if (h != 0) *shared = bs;
  return 0;
}

// Preamble checks that several entries repeat.
int check_mask_head(esmdiff_engine* e, const char* who) {
  return e->cfg.vocab_out <= ESMDIFF_MASK_ID ? fail(e, ESMDIFF_E_INVALID, "%s needs the 4101-way head (mask column)", who) : 0;
}
// ld_logits: the caller's row stride in the two step entries; null in esmdiff_gibbs_sample, which reads the engine's own logits
int check_gibbs_filter(esmdiff_engine* e, float temperature, float top_p, const int32_t* ld_logits) {
  if (!(temperature >= 0.f)) return fail(e, ESMDIFF_E_INVALID, "temperature must be >= 0 (0 = arg-max of the filtered logits)");
  if (!(top_p > 0.f) || top_p > 1.f) return fail(e, ESMDIFF_E_INVALID, "top_p must be in (0, 1]");
  if (ld_logits && (*ld_logits < 4096 || e->cfg.vocab_out < 4096 || *ld_logits < e->cfg.vocab_out)) return fail(e, ESMDIFF_E_INVALID, "bad shape");
  return 0;
}

}  // namespace

extern "C" {

int esmdiff_ddpm_step(esmdiff_engine* e, int64_t* x_inout, const float* logits, int32_t ld_logits,
                      float mc_t, float mc_s, int32_t final_, const float* u, const esmdiff_rng* rng,
                      int32_t step, int32_t B, int32_t L, void* stream) {
  if (!e) return ESMDIFF_E_INVALID;
  if (!x_inout || !logits) return fail(e, ESMDIFF_E_INVALID, "null pointer");
  if (!final_ && !u && !rng) return fail(e, ESMDIFF_E_INVALID, "need explicit uniforms or an rng");
  if (B <= 0 || L <= 0 || ld_logits < e->cfg.vocab_out) return fail(e, ESMDIFF_E_INVALID, "bad shape");
  if (int r = check_mask_head(e, "ddpm")) return r;
  Prof p{e, (hipStream_t)stream};
  RUN(S_SAMPLER, launch_ddpm_step(x_inout, logits, ld_logits, e->cfg.vocab_out, mc_t, mc_s, final_, u, u ? 0 : 1,
                                  rng ? rng->seed : 0, rng ? rng->sample_offset : 0, step, B, L, (hipStream_t)stream));
  return 0;
}

int esmdiff_ddpm_step_margin(esmdiff_engine* e, int64_t* x_inout, const float* logits, int32_t ld_logits,
                             float mc_t, float mc_s, int32_t final_, const esmdiff_rng* rng, int32_t step,
                             int32_t B, int32_t L, float margin, int32_t* sample_flags, void* stream) {
  if (!e) return ESMDIFF_E_INVALID;
  if (!x_inout || !logits || !sample_flags || !rng) return fail(e, ESMDIFF_E_INVALID, "null pointer");
  if (B <= 0 || L <= 0 || ld_logits < e->cfg.vocab_out) return fail(e, ESMDIFF_E_INVALID, "bad shape");
  if (int r = check_mask_head(e, "ddpm")) return r;
  if (!(final_ ? margin >= 0.f : margin >= 1.f))
    return fail(e, ESMDIFF_E_INVALID, "margin %g: a ratio >= 1 for an update, a difference >= 0 for the final pass", margin);
  HIP_TRY(e, launch_ddpm_step(x_inout, logits, ld_logits, e->cfg.vocab_out, mc_t, mc_s, final_, nullptr, 1, rng->seed,
                              rng->sample_offset, step, B, L, (hipStream_t)stream, 0, margin, sample_flags));
  return 0;
}

int esmdiff_ddpm_step_rows(esmdiff_engine* e, int64_t* x_inout, const float* logits, int32_t ld_logits,
                           const esmdiff_sample_step* params, uint64_t seed, int32_t B, int32_t L, float margin_ratio,
                           float margin_diff, int32_t* sample_flags, float* sample_min_gap, void* stream) {
  if (!e) return ESMDIFF_E_INVALID;
  if (!x_inout || !logits || !params) return fail(e, ESMDIFF_E_INVALID, "null pointer");
  if (B <= 0 || L <= 0 || ld_logits < e->cfg.vocab_out) return fail(e, ESMDIFF_E_INVALID, "bad shape");
  if (int r = check_mask_head(e, "ddpm")) return r;
  if (int r = check_lens(e, B, L)) return r;   // (padding holds no MASK: the step leaves it as it is)
  if ((sample_flags || sample_min_gap) && !(margin_ratio >= 1.f && margin_diff >= 0.f))
    return fail(e, ESMDIFF_E_INVALID, "margins (%g, %g): a ratio >= 1 for updates, a difference >= 0 for final passes", margin_ratio, margin_diff);
  Prof p{e, (hipStream_t)stream};
  RUN(S_SAMPLER, launch_ddpm_step_rows(x_inout, logits, ld_logits, e->cfg.vocab_out, params, seed, B, L, margin_ratio, margin_diff,
                                       sample_flags, sample_min_gap, (hipStream_t)stream));
  return 0;
}

int esmdiff_logit_error_stats(const float* a, int32_t ld_a, const float* b, int32_t ld_b, const int64_t* x, int32_t rows,
                              int32_t vocab, int32_t all_columns, float* out, void* stream) {
  if (!a || !b || !x || !out || rows < 0 || vocab <= 0 || ld_a < vocab || ld_b < vocab) return ESMDIFF_E_INVALID;
  return launch_logit_error_stats(a, ld_a, b, ld_b, x, rows, vocab, all_columns ? 1 : 0, out, (hipStream_t)stream) == hipSuccess ? 0 : ESMDIFF_E_HIP;
}

static int q_xt_checked(esmdiff_engine* e, const int64_t* x0, const int64_t* seq, const float* move_chance, const uint8_t* non_moving,
                        const float* u, uint64_t seed, const uint64_t* sample_index, const int32_t* draw, int64_t* xt_out,
                        int64_t* seq_out, int32_t B, int32_t L, hipStream_t st) {
  if (!x0 || !move_chance || !xt_out) return fail(e, ESMDIFF_E_INVALID, "null pointer");
  if (!u && (!sample_index || !draw)) return fail(e, ESMDIFF_E_INVALID, "need explicit uniforms, or sample_index and draw for the Philox source");
  if (seq_out && !seq) return fail(e, ESMDIFF_E_INVALID, "seq_out (the coupled sequence mask) needs seq");
  if (int r = check_bl(e, B, L)) return r;
  if (int r = check_lens(e, B, L)) return r;
  HIP_TRY(e, launch_q_xt(x0, seq, move_chance, non_moving, u, seed, sample_index, draw, e->cur_lens, xt_out, seq_out, B, L, st));
  return 0;
}

static int nelbo_rows_checked(esmdiff_engine* e, const float* logits, int32_t ld_logits, const int64_t* xt, const int64_t* x0,
                              const float* weight, const uint8_t* loss_mask, float* log_p_out, float* sample_sum,
                              int32_t* sample_count, int32_t B, int32_t L, hipStream_t st) {
  if (!logits || !xt || !x0 || !weight || !sample_sum || !sample_count) return fail(e, ESMDIFF_E_INVALID, "null pointer");
  if (ld_logits < e->cfg.vocab_out) return fail(e, ESMDIFF_E_INVALID, "ld_logits (%d) below the vocabulary (%d)", ld_logits, e->cfg.vocab_out);
  if (int r = check_mask_head(e, "the nelbo")) return r;
  if (int r = check_bl(e, B, L)) return r;      // (row_loss lives in the engine's workspace)
  if (int r = check_lens(e, B, L)) return r;
  Prof p{e, st};
  RUN(S_SAMPLER, launch_nelbo_rows(logits, ld_logits, e->cfg.vocab_out, xt, x0, weight, loss_mask, e->cur_lens, log_p_out, e->n_rowloss,
                                   sample_sum, sample_count, B, L, st));
  return 0;
}

int esmdiff_q_xt(esmdiff_engine* e, const int64_t* x0, const int64_t* seq, const float* move_chance, const uint8_t* non_moving,
                 const float* u, uint64_t seed, const uint64_t* sample_index, const int32_t* draw, int64_t* xt_out,
                 int64_t* seq_out, int32_t B, int32_t L, void* stream) {
  if (!e) return ESMDIFF_E_INVALID;
  if (int r = check_not_decoder(e)) return r;
  return q_xt_checked(e, x0, seq, move_chance, non_moving, u, seed, sample_index, draw, xt_out, seq_out, B, L, (hipStream_t)stream);
}

int esmdiff_nelbo_rows(esmdiff_engine* e, const float* logits, int32_t ld_logits, const int64_t* xt, const int64_t* x0,
                       const float* weight, const uint8_t* loss_mask, float* log_p_out, float* sample_sum, int32_t* sample_count,
                       int32_t B, int32_t L, void* stream) {
  if (!e) return ESMDIFF_E_INVALID;
  if (int r = check_not_decoder(e)) return r;
  return nelbo_rows_checked(e, logits, ld_logits, xt, x0, weight, loss_mask, log_p_out, sample_sum, sample_count, B, L,
                            (hipStream_t)stream);
}

int esmdiff_nelbo_eval(esmdiff_engine* e, const int64_t* seq, const int64_t* x0, const float* t_freq, const float* move_chance,
                       const float* weight, const uint8_t* non_moving, const float* u, uint64_t seed, const uint64_t* sample_index,
                       const int32_t* draw, const uint8_t* loss_mask, int32_t coupled, float* sample_sum, int32_t* sample_count,
                       float* log_p_out, int32_t B, int32_t L, void* stream) {
  if (!e) return ESMDIFF_E_INVALID;
  if (int r = check_not_decoder(e)) return r;
  if (!seq) return fail(e, ESMDIFF_E_INVALID, "null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (int r = q_xt_checked(e, x0, seq, move_chance, non_moving, u, seed, sample_index, draw, e->cx, coupled ? e->cseq : nullptr, B, L, st))
    return r;
  const int64_t* net_seq = coupled ? e->cseq : seq;
  const int rf = t_freq ? esmdiff_forward_logits_sigmas(e, net_seq, e->cx, t_freq, e->logits, e->ld_logits, B, L, stream)
                        : esmdiff_forward_logits(e, net_seq, e->cx, nullptr, e->logits, e->ld_logits, B, L, stream);
  if (rf) return rf;
  return nelbo_rows_checked(e, e->logits, e->ld_logits, e->cx, x0, weight, loss_mask, log_p_out, sample_sum, sample_count, B, L, st);
}

int esmdiff_ddpm_sample(esmdiff_engine* e, const int64_t* seq, int64_t* x_inout, int32_t B, int32_t L, int32_t T,
                        const float* mc_t, const float* mc_s, const float* t_freq, const esmdiff_rng* rng,
                        void* stream) {
  if (!e) return ESMDIFF_E_INVALID;
  if (int r = check_not_decoder(e)) return r;
  if (!seq || !x_inout || !mc_t || !mc_s || !rng) return fail(e, ESMDIFF_E_INVALID, "null pointer");
  if (T <= 0 || T + 1 > e->tfreq_rows) return fail(e, ESMDIFF_E_INVALID, "num_steps %d out of range (1..%d)", T, e->tfreq_rows - 1);
  if (e->cfg.time_conditioning && !t_freq) return fail(e, ESMDIFF_E_INVALID, "t_freq required with time conditioning");
  if (int r = check_bl(e, B, L)) return r;
  if (int r = check_lens(e, B, L)) return r;
  hipStream_t st = (hipStream_t)stream;
  const int F = e->cfg.freq_dim;
  if (t_freq) {   // through the engine's own host copy: the caller's array is consumed here (engine.h: tfreq_host)
    e->tfreq_host.assign(t_freq, t_freq + (size_t)(T + 1) * F);
    HIP_TRY(e, hipMemcpyAsync(e->tfreq, e->tfreq_host.data(), e->tfreq_host.size() * sizeof(float), hipMemcpyHostToDevice, st));
  }
  Prof p{e, st};
  int shared = 0;
  if (int r = step0_shared_batch(e, seq, x_inout, B, L, st, &shared)) return r;
  for (int i = 0; i <= T; ++i) {
    const int Bf = (i == 0 && shared) ? shared : B;   // step 0 of an all-identical batch: one sub-batch forward serves all
    if (i == T && e->final_skip && T > 0) {
      // Noise removal (model.py:575-579): x = argmax of the re-parameterised logits, which for a row without MASK is the row's own
      // token (log p = 0 there, -1e6 elsewhere, model.py:530-532) — a sample with no MASK left comes back unchanged whatever the
      // network says.  After update T the expected number of still-masked rows is mc_s / mc_t of the last step ~ 2.5e-4 of the
      // masked rows: run forward T + 1 only on the samples that hold one, as a sub-batch that takes the same dispatch path as the
      // whole batch would (bit-identical logits, shared_forward_batch), padded with the first samples when it is smaller.
      HIP_TRY(e, launch_samples_with_mask(x_inout, B, L, e->has_dev, st));
      std::vector<int32_t> has(B);
      HIP_TRY(e, hipMemcpyAsync(has.data(), e->has_dev, (size_t)B * 4, hipMemcpyDeviceToHost, st));
      HIP_TRY(e, hipStreamSynchronize(st));
      std::vector<int32_t> idx;
      for (int b = 0; b < B; ++b)
        if (has[b]) idx.push_back(b);
      const int n_live = (int)idx.size();
      if (n_live == 0) break;                                   // every sample is complete: forward T + 1 changes nothing
      const int n_min = shared_forward_batch(e, B, L);           // smallest sub-batch with the whole batch's dispatch path (B: none)
      if (n_min < B && n_live < B) {
        for (int b = 0; (int)idx.size() < n_min && b < B; ++b)
          if (!has[b]) idx.push_back(b);                         // padding: complete samples, their rows come back unchanged
        const int n_run = (int)idx.size();
        HIP_TRY(e, hipMemcpyAsync(e->idx_dev, idx.data(), (size_t)n_run * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(e, launch_move_token_rows(x_inout, e->cx, e->idx_dev, n_run, L, 1, st));
        HIP_TRY(e, launch_move_token_rows(seq, e->cseq, e->idx_dev, n_run, L, 1, st));
        std::vector<int32_t> sub_lens;
        if (e->lens_B) {   // ragged batch: the sub-batch's own lengths
          for (int j = 0; j < n_run; ++j) sub_lens.push_back(e->lens_host[idx[j]]);
          HIP_TRY(e, hipMemcpyAsync(e->lens_sub_dev, sub_lens.data(), (size_t)n_run * 4, hipMemcpyHostToDevice, st));
          e->cur_lens = e->lens_sub_dev;
        }
        const int rf = forward(e, e->cseq, e->cx, t_freq ? e->tfreq + (size_t)i * F : nullptr, e->logits, e->ld_logits, n_run, L, st, true);
        e->cur_lens = e->lens_B ? e->lens_dev : nullptr;
        if (rf) return rf;
        RUN(S_SAMPLER, launch_ddpm_step(e->cx, e->logits, e->ld_logits, e->cfg.vocab_out, 0.f, 0.f, 1, nullptr, 1, rng->seed, rng->sample_offset, i, n_run, L, st, 0,
                                        0.f, nullptr, e->rows_mapped ? e->rows_map : nullptr));
        HIP_TRY(e, launch_move_token_rows(e->cx, x_inout, e->idx_dev, n_live, L, 0, st));   // only the live samples go back
        HIP_TRY(e, hipStreamSynchronize(st));                    // idx (host vector) must outlive the H2D copy
        break;
      }
    }
    // the update reads logits on the rows that hold MASK only: the forward may run its last block's branches and its head on those
    // rows alone (engine_forward.hip: needed_tail) and then leaves them compact, found through rows_map
    if (int r = forward(e, seq, x_inout, t_freq ? e->tfreq + (size_t)i * F : nullptr, e->logits, e->ld_logits, Bf, L, st, true)) return r;
    const int fin = i == T;
    RUN(S_SAMPLER, launch_ddpm_step(x_inout, e->logits, e->ld_logits, e->cfg.vocab_out, fin ? 0.f : mc_t[i], fin ? 0.f : mc_s[i],
                                    fin, nullptr, 1, rng->seed, rng->sample_offset, i, B, L, st, Bf < B ? Bf : 0, 0.f, nullptr,
                                    e->rows_mapped ? e->rows_map : nullptr));
  }
  return 0;
}

int esmdiff_gibbs_step(esmdiff_engine* e, int64_t* x_inout, const int64_t* seq, const float* logits, int32_t ld_logits,
                       float temperature, float top_p, const int32_t* n_unmask, const float* u, const esmdiff_rng* rng,
                       int32_t step, int32_t B, int32_t L, void* stream) {
  if (!e) return ESMDIFF_E_INVALID;
  if (!x_inout || !seq || !logits || !n_unmask) return fail(e, ESMDIFF_E_INVALID, "null pointer");
  if (!u && !rng) return fail(e, ESMDIFF_E_INVALID, "need explicit uniforms or an rng");
  if (int r = check_gibbs_filter(e, temperature, top_p, &ld_logits)) return r;
  if (int r = check_bl(e, B, L)) return r;
  // (before the first profiling mark: an early return between the two marks of a section would leave an unpaired event in the
  //  pool that prof_collect walks in pairs)
  if (e->g_strategy == 1 && u) return fail(e, ESMDIFF_E_INVALID, "strategy \"random\" draws its positions from the Philox source: pass rng, not explicit uniforms");
  Prof p{e, (hipStream_t)stream};
  RUN(S_SAMPLER, launch_gibbs_step(x_inout, seq, logits, ld_logits, e->cfg.vocab_out, temperature, top_p, n_unmask, u, u ? 0 : 1, rng ? rng->seed : 0,
                                   rng ? rng->sample_offset : 0, step, e->g_sampled, e->g_entropy, B, L, (hipStream_t)stream, 0,
                                   e->g_strategy, e->g_inv_on ? e->g_inv_mask : nullptr));
  return 0;
}

int esmdiff_gibbs_step_rows(esmdiff_engine* e, int64_t* x_inout, const int64_t* seq, const float* logits, int32_t ld_logits,
                            float temperature, float top_p, const esmdiff_gibbs_sample_step* params, uint64_t seed, int32_t B,
                            int32_t L, float pair_bound, float entropy_bound, int32_t* sample_flags, float* sample_gaps,
                            void* stream) {
  if (!e) return ESMDIFF_E_INVALID;
  if (!x_inout || !seq || !logits || !params) return fail(e, ESMDIFF_E_INVALID, "null pointer");
  if (int r = check_gibbs_filter(e, temperature, top_p, &ld_logits)) return r;
  if (int r = check_bl(e, B, L)) return r;
  if (int r = check_lens(e, B, L)) return r;   // (padding holds no MASK: the step leaves it as it is)
  if (pair_bound < 0.f && (sample_flags || sample_gaps))
    return fail(e, ESMDIFF_E_INVALID, "sample_flags / sample_gaps need pair_bound >= 0 (and entropy_bound >= 0)");
  if (pair_bound >= 0.f && !(entropy_bound >= 0.f)) return fail(e, ESMDIFF_E_INVALID, "entropy_bound must be >= 0");
  Prof p{e, (hipStream_t)stream};
  RUN(S_SAMPLER, launch_gibbs_step_rows(x_inout, seq, logits, ld_logits, e->cfg.vocab_out, temperature, top_p, params, seed, e->g_sampled,
                                        e->g_entropy, B, L, pair_bound, entropy_bound, e->g_rowflag, e->g_rowgap, sample_flags, sample_gaps,
                                        (hipStream_t)stream, e->g_strategy, e->g_inv_on ? e->g_inv_mask : nullptr));
  return 0;
}

int esmdiff_gibbs_sample(esmdiff_engine* e, const int64_t* seq, int64_t* x_inout, int32_t B, int32_t L, int32_t T,
                         float temperature, float top_p, const int32_t* n_unmask_table, const esmdiff_rng* rng,
                         void* stream) {
  if (!e) return ESMDIFF_E_INVALID;
  if (int r = check_not_decoder(e)) return r;
  if (!seq || !x_inout || !n_unmask_table || !rng) return fail(e, ESMDIFF_E_INVALID, "null pointer");
  if (T <= 0 || T > e->tfreq_rows) return fail(e, ESMDIFF_E_INVALID, "num_steps %d out of range (1..%d)", T, e->tfreq_rows);
  if (int r = check_bl(e, B, L)) return r;
  if (int r = check_lens(e, B, L)) return r;
  hipStream_t st = (hipStream_t)stream;
  if (int r = check_gibbs_filter(e, temperature, top_p, nullptr)) return r;
  e->nunmask_host.assign(n_unmask_table, n_unmask_table + (size_t)T * B);   // the caller's array is consumed here (engine.h)
  HIP_TRY(e, hipMemcpyAsync(e->g_nunmask, e->nunmask_host.data(), e->nunmask_host.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
  int shared = 0;
  if (int r = step0_shared_batch(e, seq, x_inout, B, L, st, &shared)) return r;   // (0 with coordinate conditioning)
  for (int i = 0; i < T; ++i) {
    const int Bf = (i == 0 && shared) ? shared : B;
    if (int r = forward(e, seq, x_inout, nullptr, e->logits, e->ld_logits, Bf, L, st)) return r;
    Prof p{e, st};
    RUN(S_SAMPLER, launch_gibbs_step(x_inout, seq, e->logits, e->ld_logits, e->cfg.vocab_out, temperature, top_p,
                                     e->g_nunmask + (size_t)i * B, nullptr, 1, rng->seed, rng->sample_offset, i, e->g_sampled,
                                     e->g_entropy, B, L, st, Bf < B ? Bf : 0, e->g_strategy, e->g_inv_on ? e->g_inv_mask : nullptr));
  }
  return 0;
}

}  // extern "C"

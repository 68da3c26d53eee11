// engine.hip — lifetime and state of an engine of libesmdiff_hip.so (C ABI: include/esmdiff_hip.h): create and destroy, the
// setters and getters of engine state, and the helpers every engine unit uses, the error channel among them (engine.h says what
// lives where; the weights come in through engine_weights.hip).
// The engine never synchronises except in create, in the setters that say so and in the profiling readback.
#include "engine.h"

using namespace ed;
using namespace eng;

namespace {

thread_local std::string g_error;   // the handle-less error string: a failed create of any kind, a kernel-level test entry

}  // namespace

namespace eng {

int fail(Owner* o, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (o) o->err = buf; else g_error = buf;
  return code;
}

const char* last_error(const Owner* o) { return o ? o->err.c_str() : g_error.c_str(); }

int round_up(int v, int m) { return (v + m - 1) / m * m; }

// softplus of the geometric attention's per-head scales (F.softplus, threshold 20), in place: engine create and
// esmdiff_geom_attention both go through here
void softplus_host(float* v, int n) {
  for (int i = 0; i < n; ++i) v[i] = v[i] > 20.f ? v[i] : log1pf(expf(v[i]));
}

int check_bl(esmdiff_engine* e, int B, int L) {
  if (B <= 0 || L <= 0) return fail(e, ESMDIFF_E_INVALID, "B=%d L=%d must be positive", B, L);
  if (B > e->cfg.max_batch || L > e->cfg.max_len)
    return fail(e, ESMDIFF_E_CAPACITY, "B=%d L=%d exceeds the engine capacity (max_batch=%d, max_len=%d)", B, L, e->cfg.max_batch, e->cfg.max_len);
  return 0;
}

// While lengths are set (esmdiff_set_lengths) a call must cover exactly that batch, and every length must fit its L.
int check_lens(esmdiff_engine* e, int B, int L) {
  if (e->lens_B == 0) return 0;
  if (B != e->lens_B) return fail(e, ESMDIFF_E_INVALID, "lengths were set for B=%d, call has B=%d", e->lens_B, B);
  for (int b = 0; b < B; ++b)
    if (e->lens_host[b] > L) return fail(e, ESMDIFF_E_INVALID, "length %d of sample %d exceeds L=%d", e->lens_host[b], b, L);
  return 0;
}

// The entries of the ESM3 engine (forward, samplers, q_xt, the NELBO) refuse a decoder engine with this.
int check_not_decoder(esmdiff_engine* e) {
  return e->kind != 0 ? fail(e, ESMDIFF_E_INVALID, "this engine is a structure-token decoder (esmdiff_decoder_create)") : 0;
}

}  // namespace eng

namespace {

// A linear of this engine: load_linear with the engine's 16-bit operand type and the split forms' scratch word.
int engine_linear(esmdiff_engine* e, const Table& t, const std::string& name, std::initializer_list<int64_t> shape, Linear::Form form,
                  Linear* dst, int64_t pad_rows = 0, int swiglu_h = 0) {
  return load_linear(e, t, name, shape, form, dst, pad_rows, swiglu_h, e->f16, e->scratch_bits);
}

// The form of a group of weights, chosen once at create.  plain_form, the engine's non-split form: the pairwise head always, and
// block 0's geometric pair unless BOTH its shapes fit the split GEMM (create_engine).  body_form: the block stack's linears and
// the second (pLDDT / sequence) head's.  head_form: the output head's, SPLIT also under head_precision = 1.
Linear::Form plain_form(const esmdiff_engine* e) { return e->strict ? Linear::F32 : Linear::W16; }
Linear::Form body_form(const esmdiff_engine* e) { return e->split ? Linear::SPLIT : plain_form(e); }
Linear::Form head_form(const esmdiff_engine* e) { return e->head_split ? Linear::SPLIT : body_form(e); }

void prof_collect(esmdiff_engine* e) {
  if (!e->profiling || e->ev_used < 2) {
    e->ev_used = 0;
    return;
  }
  hipDeviceSynchronize();
  // mode 2 (only the FFN-up launches are bracketed, possibly on two overlapping streams): besides the per-launch sum, the
  // UNION of the launches' busy intervals on the device timeline (event timestamps share one clock across streams) —
  // slot 15 — so that FFN-up FLOP of all streams / union is a device-level rate that never counts an instant twice.
  std::vector<std::pair<float, float>> iv;
  for (size_t i = 0; i + 1 < e->ev_used; i += 2) {
    float ms = 0;
    hipEventElapsedTime(&ms, e->ev[i], e->ev[i + 1]);
    e->prof_ms[e->ev_section[i]] += ms;
    e->prof_launches[e->ev_section[i]] += 1;
    if (e->profiling == 2) {
      float t0 = 0;
      if (i) hipEventElapsedTime(&t0, e->ev[0], e->ev[i]);   // may be negative across streams: fine, only order matters
      iv.emplace_back(t0, t0 + ms);
    }
  }
  if (!iv.empty()) {
    std::sort(iv.begin(), iv.end());
    float busy = 0, lo = iv[0].first, hi = iv[0].second;
    for (size_t i = 1; i < iv.size(); ++i) {
      if (iv[i].first > hi) {
        busy += hi - lo;
        lo = iv[i].first;
        hi = iv[i].second;
      } else if (iv[i].second > hi) {
        hi = iv[i].second;
      }
    }
    busy += hi - lo;
    e->prof_ms[15] += busy;
    e->prof_launches[15] += (int)iv.size();
  }
  e->ev_used = 0;
}

}  // namespace

extern "C" {

int esmdiff_set_gibbs_options(esmdiff_engine* e, int32_t strategy, const int32_t* invalid_ids, int32_t n_invalid) {
  if (!e) return ESMDIFF_E_INVALID;
  if (strategy != 0 && strategy != 1) return fail(e, ESMDIFF_E_INVALID, "strategy %d: 0 (entropy) or 1 (random)", strategy);
  if (n_invalid < 0 || (n_invalid > 0 && !invalid_ids)) return fail(e, ESMDIFF_E_INVALID, "invalid_ids: null with n = %d", n_invalid);
  uint32_t mask[128] = {0};
  int n_set = 0;
  for (int i = 0; i < n_invalid; ++i) {
    const int v = invalid_ids[i];
    if (v < 0 || v >= ESMDIFF_VOCAB) return fail(e, ESMDIFF_E_INVALID, "invalid_ids[%d] = %d is not a structure-track id (0..%d)", i, v, ESMDIFF_VOCAB - 1);
    if (v < 4096 && !((mask[v >> 5] >> (v & 31)) & 1u)) {   // the special ids >= 4096 are never drawn anyway
      mask[v >> 5] |= 1u << (v & 31);
      ++n_set;
    }
  }
  if (n_set >= 4096) return fail(e, ESMDIFF_E_INVALID, "invalid_ids leaves no id to draw");
  HIP_TRY(e, hipSetDevice(e->device));
  // A blocking copy is ordered against the null stream and blocking streams only: a gibbs step still queued on a caller's
  // non-blocking stream would read the new mask.  Wait for the device first, as esmdiff_set_lengths does.
  HIP_TRY(e, hipDeviceSynchronize());
  HIP_TRY(e, hipMemcpy(e->g_inv_mask, mask, sizeof mask, hipMemcpyHostToDevice));
  e->g_inv_on = n_set > 0;
  e->g_strategy = strategy;
  return 0;
}

int esmdiff_set_step0_sharing(esmdiff_engine* e, int32_t on) {
  if (!e) return ESMDIFF_E_INVALID;
  e->step0_share = on ? 1 : 0;
  return 0;
}

static int add_side_stream(esmdiff_engine* e) {
  hipStream_t sd = nullptr;
  hipEvent_t ev = nullptr;
  if (hipStreamCreateWithFlags(&sd, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess)
    return fail(e, ESMDIFF_E_HIP, "side stream: %s", hipGetErrorString(hipGetLastError()));
  e->side.push_back(sd);
  e->ev_join.push_back(ev);
  return 0;
}

int esmdiff_set_option(esmdiff_engine* e, int32_t option, int64_t value) {
  if (!e) return ESMDIFF_E_INVALID;
  switch (option) {
    case ESMDIFF_OPT_STREAMS:
      if (value < 1 || value > 4) return fail(e, ESMDIFF_E_INVALID, "ESMDIFF_OPT_STREAMS: 1 .. 4, got %lld", (long long)value);
      HIP_TRY(e, hipSetDevice(e->device));
      while ((int64_t)e->side.size() + 1 < value)
        if (int r = add_side_stream(e)) return r;
      e->n_streams = (int)value;
      return 0;
    case ESMDIFF_OPT_DUAL_MIN_TOKENS:
      if (value < 1) return fail(e, ESMDIFF_E_INVALID, "ESMDIFF_OPT_DUAL_MIN_TOKENS must be positive");
      e->dual_min_tokens = value;
      return 0;
    case ESMDIFF_OPT_NEEDED_ROWS:
      if (value != 0 && value != 1) return fail(e, ESMDIFF_E_INVALID, "ESMDIFF_OPT_NEEDED_ROWS: 0 or 1, got %lld", (long long)value);
      e->needed_rows = (int)value;
      return 0;
    default:
      return fail(e, ESMDIFF_E_INVALID, "unknown option %d", option);
  }
}

int esmdiff_get_build_info(char* buf, int32_t cap) {
#ifdef ED_DEBUG
  const int dbg = 1;
#else
  const int dbg = 0;
#endif
  char tmp[512];
  const int n = snprintf(tmp, sizeof tmp,
                         "libesmdiff_hip abi=%d arch=gfx950 debug_env=%d (%s) operand_builds=bf16,f16 fp_contract_off=sampler,gibbs,metrics "
                         "compiler=%s",
                         ESMDIFF_ABI_VERSION, dbg,
                         dbg ? "-DED_DEBUG: esmdiff_gemm_bf16_timed is exported; no ESMDIFF_* tuning switch is read" : "product build: no ESMDIFF_* tuning switch is read",
                         __VERSION__);
  if (buf && cap > 0) snprintf(buf, (size_t)cap, "%s", tmp);
  return n;
}

int esmdiff_set_final_skip(esmdiff_engine* e, int32_t on) {
  if (!e) return ESMDIFF_E_INVALID;
  e->final_skip = on ? 1 : 0;
  return 0;
}

int esmdiff_set_small_batch_splitk(esmdiff_engine* e, int32_t on) {
  if (!e) return ESMDIFF_E_INVALID;
  if (on && !e->split) return fail(e, ESMDIFF_E_INVALID, "K-sliced small batches exist for the F32_SPLIT precision only");
  if (on && !e->sk_parts) {
    HIP_TRY(e, hipSetDevice(e->device));
    const int64_t rows = std::min<int64_t>(kSplitkMaxRows, (int64_t)e->cfg.max_batch * e->cfg.max_len);
    // two parts of a two-stream forward may both qualify (e.g. 2 x 4096 rows): room for two padded parts + the part offset
    const size_t n = (size_t)4 * (size_t)(2 * ((rows + 255) / 256 * 256) + 512) * e->cfg.d_model;
    if (int r = dalloc(e, &e->sk_parts, n)) return r;
  }
  e->splitk_small = on != 0;
  return 0;
}

int esmdiff_get_counters(esmdiff_engine* e, int64_t* forwards, int64_t* token_rows, int32_t reset) {
  if (!e) return ESMDIFF_E_INVALID;
  if (forwards) *forwards = e->stat_forwards;
  if (token_rows) *token_rows = e->stat_rows;
  if (reset) e->stat_forwards = e->stat_rows = 0;
  return 0;
}

int esmdiff_get_tail_rows(esmdiff_engine* e, int64_t* rows_out, int32_t reset) {
  if (!e) return ESMDIFF_E_INVALID;
  if (rows_out) *rows_out = e->stat_tail_rows;
  if (reset) e->stat_tail_rows = 0;
  return 0;
}

int esmdiff_abi_version(void) { return ESMDIFF_ABI_VERSION; }

const char* esmdiff_last_error(const esmdiff_engine* eng) { return last_error(eng); }

void esmdiff_engine_destroy(esmdiff_engine* e) {
  if (!e) return;
  hipSetDevice(e->device);
  hipDeviceSynchronize();
  for (void* p : e->allocs) hipFree(p);
  for (void* p : {(void*)e->pair_x, (void*)e->pair_h, (void*)e->pair_logits})  // the pairwise head's lazily sized workspace
    if (p) hipFree(p);
  for (hipEvent_t ev : e->ev) hipEventDestroy(ev);
  if (e->ev_fork) hipEventDestroy(e->ev_fork);
  if (e->ev_rows) hipEventDestroy(e->ev_rows);
  if (e->rows_count) hipHostFree(e->rows_count);
  for (hipEvent_t ev : e->ev_join) hipEventDestroy(ev);
  for (hipStream_t sd : e->side) hipStreamDestroy(sd);
  delete e;
}

static int create_engine(const esmdiff_config* cfg, const esmdiff_weight* table, int32_t n, int32_t device, int kind,
                         esmdiff_engine** out) {
  if (!cfg || !table || !out || n <= 0) return fail(nullptr, ESMDIFF_E_INVALID, "null argument");
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device >= ndev)
    return fail(nullptr, ESMDIFF_E_NODEVICE, "no HIP device %d (found %d) — libesmdiff_hip.so needs an MI355X (gfx950)", device, ndev);
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return fail(nullptr, ESMDIFF_E_NODEVICE, "hipGetDeviceProperties failed");
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(nullptr, ESMDIFF_E_NODEVICE, "device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName);
  const int D = cfg->d_model, H = cfg->n_heads, FH = cfg->ffn_hidden, V = cfg->vocab_out, F = cfg->freq_dim;
  if (D != H * 64) return fail(nullptr, ESMDIFF_E_INVALID, "d_model (%d) must be n_heads (%d) x 64", D, H);
  if (D % 256 || D > 2048) return fail(nullptr, ESMDIFF_E_INVALID, "d_model must be a multiple of 256, <= 2048");
  if (FH % 128 || cfg->n_layers <= 0 || cfg->max_batch <= 0 || cfg->max_len <= 0 ||
      (kind == 0 && (V < ESMDIFF_MASK_ID || V > 5120 || F <= 0)) || (kind == 1 && V != 23))
    return fail(nullptr, ESMDIFF_E_INVALID, "invalid configuration");

  if (cfg->precision < ESMDIFF_PRECISION_BF16 || cfg->precision > ESMDIFF_PRECISION_F16)
    return fail(nullptr, ESMDIFF_E_INVALID, "precision %d: expected ESMDIFF_PRECISION_BF16 (0), _F32 (1), _F32_SPLIT (2) or _F16 (3)", cfg->precision);
  if (cfg->precision == ESMDIFF_PRECISION_F16 && kind != 0)
    return fail(nullptr, ESMDIFF_E_INVALID, "the structure decoder runs in bf16, f32 or f32_split (its pairwise head has no f16 build)");
  esmdiff_engine* e = new esmdiff_engine;
  e->cfg = *cfg;
  e->kind = kind;
  e->device = device;
  e->strict = cfg->precision == ESMDIFF_PRECISION_F32 || cfg->precision == ESMDIFF_PRECISION_F32_SPLIT;
  e->split = cfg->precision == ESMDIFF_PRECISION_F32_SPLIT;
  e->f16 = cfg->precision == ESMDIFF_PRECISION_F16;
  e->head_split = !e->strict && kind == 0 && cfg->head_precision == 1;
  if (cfg->head_precision != 0 && cfg->head_precision != 1)
    return (delete e, fail(nullptr, ESMDIFF_E_INVALID, "head_precision %d: 0 (as precision) or 1 (float32 grade)", cfg->head_precision));
  const bool strict = e->strict, split = e->split, head_split = e->head_split;
  const Linear::Form bf = body_form(e), hf = head_form(e), pf = plain_form(e);
  if (split && (D % 128 || FH % 128))
    return (delete e, fail(nullptr, ESMDIFF_E_INVALID, "precision F32_SPLIT needs d_model and ffn_hidden to be multiples of 128"));
  auto bail = [&](int code) {
    g_error = e->err;
    esmdiff_engine_destroy(e);
    return code;
  };
  if (hipSetDevice(device) != hipSuccess) return bail(fail(e, ESMDIFF_E_HIP, "hipSetDevice failed"));

  const Table t(table, n, "net.");   // a Lightning checkpoint's names carry the wrapper's prefix

#define TRY(x)                  \
  do {                          \
    if (int _r = (x)) return bail(_r); \
  } while (0)

  if (split || head_split) TRY(dalloc(e, &e->scratch_bits, (size_t)4, true));
  // kind 1 (esm StructureTokenDecoder, SURVEY.md 8f-1 [ESM-RECALL]): the same block stack under decoder_stack.*, a single
  // token embedding, and affine_output_projection (Linear -> GELU -> LayerNorm -> Linear(23)) in place of the head
  const std::string stack = kind == 1 ? "decoder_stack." : "transformer.";
  const std::string head0 = kind == 1 ? "affine_output_projection.ffn1." : "output_heads.structure_head.0.";
  const std::string head2 = kind == 1 ? "affine_output_projection.norm." : "output_heads.structure_head.2.";
  const std::string head3 = kind == 1 ? "affine_output_projection.proj." : "output_heads.structure_head.3.";
  e->layers.resize(cfg->n_layers);
  for (int i = 0; i < cfg->n_layers; ++i) {
    Layer& ly = e->layers[i];
    const std::string b = stack + "blocks." + std::to_string(i) + ".";
    TRY(load_f32(e, t, b + "attn.layernorm_qkv.0.weight", {D}, &ly.ln1_w));
    TRY(load_f32(e, t, b + "attn.layernorm_qkv.0.bias", {D}, &ly.ln1_b));
    TRY(engine_linear(e, t, b + "attn.layernorm_qkv.1.weight", {3 * D, D}, bf, &ly.w_qkv));
    TRY(load_f32(e, t, b + "attn.q_ln.weight", {D}, &ly.q_ln_w));
    TRY(load_f32(e, t, b + "attn.k_ln.weight", {D}, &ly.k_ln_w));
    if (split) {   // |q|, |k| <= sqrt(2 (D - 1)) max|ln weight| (LayerNorm + rotation); |v| <= (sqrt(D) max|g| + |b|_2) max_row |W_v row|_2
      if (hipDeviceSynchronize() != hipSuccess) return bail(fail(e, ESMDIFF_E_HIP, "weight conversion failed"));
      std::vector<float> hq(D), hk(D), hg(D), hb(D);
      hipMemcpy(hq.data(), ly.q_ln_w, (size_t)D * 4, hipMemcpyDeviceToHost);
      hipMemcpy(hk.data(), ly.k_ln_w, (size_t)D * 4, hipMemcpyDeviceToHost);
      hipMemcpy(hg.data(), ly.ln1_w, (size_t)D * 4, hipMemcpyDeviceToHost);
      hipMemcpy(hb.data(), ly.ln1_b, (size_t)D * 4, hipMemcpyDeviceToHost);
      float wmax = 0.f, gmax = 0.f, b2 = 0.f, rn = 0.f;
      for (int d = 0; d < D; ++d) {
        wmax = std::max(wmax, std::max(fabsf(hq[d]), fabsf(hk[d])));
        gmax = std::max(gmax, fabsf(hg[d]));
        b2 += hb[d] * hb[d];
      }
      const esmdiff_weight* wq;
      TRY(need(e, t, b + "attn.layernorm_qkv.1.weight", {3 * D, D}, &wq));
      if (weight_rownorm_max(wq->data, wq->dtype, (int64_t)2 * D, D, D, e->scratch_bits, &rn) != hipSuccess)
        return bail(fail(e, ESMDIFF_E_HIP, "row-norm reduction of the value projection failed"));
      auto pow2_below = [](float x) { return (x > 0.f && std::isfinite(x)) ? exp2f(floorf(log2f(x))) : 1.f; };
      ly.att_qk = pow2_below(30000.f / (sqrtf(2.f * D) * wmax));
      ly.att_v = pow2_below(30000.f / ((sqrtf((float)D) * gmax + sqrtf(b2)) * rn));
    }
    TRY(engine_linear(e, t, b + "attn.out_proj.weight", {D, D}, bf, &ly.w_out));
    TRY(load_f32(e, t, b + "ffn.0.weight", {D}, &ly.ln2_w));
    TRY(load_f32(e, t, b + "ffn.0.bias", {D}, &ly.ln2_b));
    // FFN-up with the SwiGLU in the GEMM's epilogue: rows interleaved gate / up (W16, and SPLIT: mid leaves it as f32 and is split
    // with its row's own scale, strict_part); F32 keeps the checkpoint's order
    TRY(engine_linear(e, t, b + "ffn.1.weight", {2 * FH, D}, bf, &ly.w_up, 0, FH));
    TRY(engine_linear(e, t, b + "ffn.3.weight", {D, FH}, bf, &ly.w_down));
  }
  TRY(load_f32(e, t, stack + "norm.weight", {D}, &e->final_ln_w));
  TRY(engine_linear(e, t, head0 + "weight", {D, D}, hf, &e->head_w0));
  TRY(load_f32(e, t, head0 + "bias", {D}, &e->head_b0));
  TRY(load_f32(e, t, head2 + "weight", {D}, &e->head_ln_w));
  TRY(load_f32(e, t, head2 + "bias", {D}, &e->head_ln_b));
  e->vocab_pad = round_up(V, 256);  // 4101 -> 4352: 17 column tiles of the 256x256 kernel (the 128x128 kernel took 0.40 ms at M = 25 800)
  TRY(engine_linear(e, t, head3 + "weight", {V, D}, hf, &e->head_w3, e->vocab_pad));
  TRY(load_f32(e, t, head3 + "bias", {V}, &e->head_b3, e->vocab_pad));
  if (kind == 1) TRY(load_f32(e, t, "embed.weight", {ESMDIFF_VOCAB, D}, &e->e_struct));
  {
    // A second RegressionHead(d, n) (Linear, GELU, LayerNorm, Linear) on the same normalised hidden state: the decoder's pLDDT
    // head (n = 50 bins), or — r05 — the reference's optional SEQUENCE head of the ESMDiff network (net.py:299-311:
    // StructureOutputHeads(d_model, n_structure_heads, n_sequence_heads > 0), read by _model_wrapper when sequence_prediction is
    // on, model.py:488-490).  Same buffers, same launches; esmdiff_get_sequence_logits copies the valid columns out.
    const std::string sh = kind == 1 ? "plddt_head." : "output_heads.sequence_head.";
    if (const esmdiff_weight* pw = t.find(sh + "3.weight")) {
      const int nb = pw->ndim == 2 ? (int)pw->shape[0] : 0;
      if (nb <= 0 || nb > 128) return bail(fail(e, ESMDIFF_E_INVALID, "%s3.weight: %d outputs unsupported (1..128)", sh.c_str(), nb));
      if (head_split) return bail(fail(e, ESMDIFF_E_INVALID, "a sequence head and head_precision = 1 together are not built: use precision f32 / f32_split or head_precision 0"));
      e->plddt_bins = nb;
      e->ld_plddt = split ? 256 : round_up(nb, 4);   // the split GEMM has no column bound: its output row holds all N_pad columns
      TRY(engine_linear(e, t, sh + "0.weight", {D, D}, bf, &e->pl_w0));
      TRY(load_f32(e, t, sh + "0.bias", {D}, &e->pl_b0));
      TRY(load_f32(e, t, sh + "2.weight", {D}, &e->pl_ln_w));
      TRY(load_f32(e, t, sh + "2.bias", {D}, &e->pl_ln_b));
      TRY(engine_linear(e, t, sh + "3.weight", {nb, D}, bf, &e->pl_w3, split ? 256 : 128));   // one column tile of its GEMM
      TRY(load_f32(e, t, sh + "3.bias", {nb}, &e->pl_b3, 128));
      e->has_plddt = true;
    }
  }
  if (kind == 1) {
    if (t.find("pairwise_classification_head.linear2.weight")) {
      const std::string ph = "pairwise_classification_head.";
      TRY(engine_linear(e, t, ph + "downproject.weight", {128, D}, pf, &e->pw_down));
      TRY(engine_linear(e, t, ph + "linear1.weight", {128, 128}, pf, &e->pw_l1));
      TRY(load_f32(e, t, ph + "norm.weight", {128}, &e->pw_ln_w));
      TRY(load_f32(e, t, ph + "norm.bias", {128}, &e->pw_ln_b));
      // rows [distogram 64 | direction 96 | PAE 64]; padded so that the 128-row W16 GEMM tile starting at row 160 stays inside
      TRY(engine_linear(e, t, ph + "linear2.weight", {224, 128}, pf, &e->pw_l2, 384));
      TRY(dalloc(e, &e->zeros128, (size_t)128, true));
      e->has_pair = true;
    }
  } else {
    TRY(load_f32(e, t, "encoder.sequence_embed.weight", {64, D}, &e->e_seq));
    TRY(load_f32(e, t, "encoder.structure_tokens_embed.weight", {ESMDIFF_VOCAB, D}, &e->e_struct));
  }
  if (kind == 0 && (cfg->time_conditioning || t.find("sigma_embedder.mlp.0.weight"))) {
    TRY(load_f32(e, t, "sigma_embedder.mlp.0.weight", {D, F}, &e->sig_w1));
    TRY(load_f32(e, t, "sigma_embedder.mlp.0.bias", {D}, &e->sig_b1));
    TRY(load_f32(e, t, "sigma_embedder.mlp.2.weight", {D, D}, &e->sig_w2));
    TRY(load_f32(e, t, "sigma_embedder.mlp.2.bias", {D}, &e->sig_b2));
  }
  // block 0's geometric attention: optional (the DDPM path never needs it: coordinates are all-NaN there)
  if (const esmdiff_weight* pw = kind == 0 ? t.find("transformer.blocks.0.geom_attn.proj.weight") : nullptr) {
    const std::string ga = "transformer.blocks.0.geom_attn.";
    const int VH = pw->ndim == 2 ? (int)(pw->shape[0] / 15) : 0;  // proj: Linear(D, v_heads * 3 * 5)
    if (VH <= 0 || (15 * VH) % 128 || (3 * VH) % 64) return bail(fail(e, ESMDIFF_E_INVALID, "geom_attn v_heads=%d unsupported", VH));
    e->v_heads = VH;
    TRY(load_f32(e, t, ga + "s_norm.weight", {D}, &e->g_snorm_w));
    const Linear::Form gf = split && (15 * VH) % 256 == 0 && (3 * VH) % 128 == 0 ? Linear::SPLIT : pf;
    TRY(engine_linear(e, t, ga + "proj.weight", {15 * VH, D}, gf, &e->g_proj));
    TRY(engine_linear(e, t, ga + "out_proj.weight", {D, 3 * VH}, gf, &e->g_out));
    TRY(load_f32(e, t, ga + "rotation_scale_per_head", {VH}, &e->g_wrot));
    TRY(load_f32(e, t, ga + "distance_scale_per_head", {VH}, &e->g_wdist));
    if (hipDeviceSynchronize() != hipSuccess) return bail(fail(e, ESMDIFF_E_HIP, "geom weight conversion failed"));
    std::vector<float> hw(VH);
    for (float* p : {e->g_wrot, e->g_wdist}) {  // softplus once, on the host
      hipMemcpy(hw.data(), p, VH * 4, hipMemcpyDeviceToHost);
      softplus_host(hw.data(), VH);
      hipMemcpy(p, hw.data(), VH * 4, hipMemcpyHostToDevice);
    }
    e->has_geom = true;
  }
  // constant vector of the defaulted tracks (net.py:410-431 -> esm EncodeInputs): average_plddt = 1,
  // per_res_plddt = 0 through rbf(.,0,1,16) and a Linear(16,D); ss8 / sasa pad id 0; function and
  // residue-annotation pads embed to zero (padding_idx=0).
  if (kind == 0) {
    float *pw, *pb, *sw, *sb, *ss8, *sasa;
    TRY(load_f32(e, t, "encoder.plddt_projection.weight", {D, 16}, &pw));
    TRY(load_f32(e, t, "encoder.plddt_projection.bias", {D}, &pb));
    TRY(load_f32(e, t, "encoder.structure_per_res_plddt_projection.weight", {D, 16}, &sw));
    TRY(load_f32(e, t, "encoder.structure_per_res_plddt_projection.bias", {D}, &sb));
    TRY(load_f32(e, t, "encoder.ss8_embed.weight", {11, D}, &ss8));
    TRY(load_f32(e, t, "encoder.sasa_embed.weight", {19, D}, &sasa));
    if (hipDeviceSynchronize() != hipSuccess) return bail(fail(e, ESMDIFF_E_HIP, "weight conversion failed: %s", hipGetErrorString(hipGetLastError())));
    std::vector<float> hpw((size_t)D * 16), hsw((size_t)D * 16), hpb(D), hsb(D), hss8(D), hsasa(D), hc(D);
    hipMemcpy(hpw.data(), pw, hpw.size() * 4, hipMemcpyDeviceToHost);
    hipMemcpy(hsw.data(), sw, hsw.size() * 4, hipMemcpyDeviceToHost);
    hipMemcpy(hpb.data(), pb, D * 4, hipMemcpyDeviceToHost);
    hipMemcpy(hsb.data(), sb, D * 4, hipMemcpyDeviceToHost);
    hipMemcpy(hss8.data(), ss8, D * 4, hipMemcpyDeviceToHost);   // row 0
    hipMemcpy(hsasa.data(), sasa, D * 4, hipMemcpyDeviceToHost); // row 0
    float rbf1[16], rbf0[16];
    for (int i = 0; i < 16; ++i) {
      const float center = (float)i / 15.0f, stdv = 1.0f / 16.0f;
      const float z1 = (1.0f - center) / stdv, z0 = (0.0f - center) / stdv;
      rbf1[i] = expf(-z1 * z1);
      rbf0[i] = expf(-z0 * z0);
    }
    for (int d = 0; d < D; ++d) {
      float a = hpb[d], b2 = hsb[d];
      for (int i = 0; i < 16; ++i) {
        a += hpw[(size_t)d * 16 + i] * rbf1[i];
        b2 += hsw[(size_t)d * 16 + i] * rbf0[i];
      }
      hc[d] = ((a + b2) + hss8[d]) + hsasa[d];
    }
    TRY(dalloc(e, &e->cvec, (size_t)D));
    hipMemcpy(e->cvec, hc.data(), D * 4, hipMemcpyHostToDevice);
  }
  // rotary tables: inv_freq = 10000^(-2i/64), positions 0..max_len-1 (BOS is position 0)
  {
    const int Lm = cfg->max_len;
    std::vector<float> hc((size_t)Lm * 32), hs((size_t)Lm * 32);
    for (int i = 0; i < 32; ++i) {
      const float inv = 1.0f / powf(10000.0f, (float)(2 * i) / 64.0f);
      for (int l = 0; l < Lm; ++l) {
        const float ang = (float)l * inv;
        hc[(size_t)l * 32 + i] = (float)cos((double)ang);
        hs[(size_t)l * 32 + i] = (float)sin((double)ang);
      }
    }
    TRY(dalloc(e, &e->rope_cos, hc.size()));
    TRY(dalloc(e, &e->rope_sin, hs.size()));
    hipMemcpy(e->rope_cos, hc.data(), hc.size() * 4, hipMemcpyHostToDevice);
    hipMemcpy(e->rope_sin, hs.data(), hs.size() * 4, hipMemcpyHostToDevice);
  }
  // workspace
  {
    const size_t Mx = (size_t)cfg->max_batch * cfg->max_len;
    e->ld_logits = (split || head_split) ? e->vocab_pad : round_up(V, 4);   // (split: see ld_plddt)
    TRY(dalloc(e, &e->x, Mx * D));
    if (strict) {
      TRY(dalloc(e, &e->fh, Mx * D));
      TRY(dalloc(e, &e->fh2, Mx * D));
      TRY(dalloc(e, &e->fqkv, Mx * 3 * D));
      TRY(dalloc(e, &e->fq, Mx * D));
      TRY(dalloc(e, &e->fk, Mx * D));
      TRY(dalloc(e, &e->fctx, Mx * D));
      if (!split) TRY(dalloc(e, &e->fgu, Mx * 2 * FH));   // gate / up rows: the split FFN-up's SwiGLU epilogue never writes them out
      TRY(dalloc(e, &e->fmid, Mx * FH));
      if (e->has_pair) TRY(dalloc(e, &e->fpair_qk, Mx * 128));
      if (split) {
        TRY(dalloc(e, &e->a2, Mx * 3 * (size_t)std::max(D, FH)));
        TRY(dalloc(e, &e->rs, Mx));
      }
    } else {
      TRY(dalloc(e, &e->h, Mx * D));
      TRY(dalloc(e, &e->h2, Mx * D));
      TRY(dalloc(e, &e->qkv, Mx * 3 * D));
      TRY(dalloc(e, &e->q, Mx * D));
      TRY(dalloc(e, &e->k, Mx * D));
      TRY(dalloc(e, &e->ctx, Mx * D));
      TRY(dalloc(e, &e->dlt, Mx * D));
      TRY(dalloc(e, &e->dlt2, Mx * D));
      if (head_split) {
        TRY(dalloc(e, &e->a2, Mx * 3 * (size_t)D));
        TRY(dalloc(e, &e->rs, Mx));
        TRY(dalloc(e, &e->fh2, Mx * D));
      }
    }
    if (e->has_geom) {
      if (strict) {
        TRY(dalloc(e, &e->fgp, Mx * 15 * e->v_heads));
        TRY(dalloc(e, &e->fgctx, Mx * 3 * e->v_heads));
      } else {
        TRY(dalloc(e, &e->gp, Mx * 15 * e->v_heads));
        TRY(dalloc(e, &e->gctx, Mx * 3 * e->v_heads));
      }
      TRY(dalloc(e, &e->f_rot, Mx * 9));
      TRY(dalloc(e, &e->f_trans, Mx * 3));
      TRY(dalloc(e, &e->f_mask, Mx));
    }
    if (!strict) TRY(dalloc(e, &e->mid, Mx * FH));
    TRY(dalloc(e, &e->logits, Mx * e->ld_logits));
    if (e->has_plddt) TRY(dalloc(e, &e->pl_logits, Mx * e->ld_plddt));
    if (e->has_pair) {
      if (!strict) TRY(dalloc(e, &e->pair_qk, Mx * 128));   // (a float32 engine keeps the pair rows in fpair_qk)
      TRY(dalloc(e, &e->tm_rows, Mx));
      TRY(dalloc(e, &e->ptm_dev, (size_t)cfg->max_batch));
    }
    TRY(dalloc(e, &e->cond, (size_t)cfg->max_batch * D));          // one conditioning vector per sample at most
    TRY(dalloc(e, &e->sig_hidden, (size_t)cfg->max_batch * D));
    e->tfreq_rows = 1026;
    TRY(dalloc(e, &e->tfreq, (size_t)e->tfreq_rows * F));
    TRY(dalloc(e, &e->g_entropy, Mx));
    TRY(dalloc(e, &e->flag_dev, (size_t)4));
    TRY(dalloc(e, &e->has_dev, (size_t)cfg->max_batch));
    TRY(dalloc(e, &e->idx_dev, (size_t)cfg->max_batch));
    TRY(dalloc(e, &e->lens_dev, (size_t)cfg->max_batch));
    TRY(dalloc(e, &e->lens_sub_dev, (size_t)cfg->max_batch));
    TRY(dalloc(e, &e->cx, Mx));
    TRY(dalloc(e, &e->cseq, Mx));
    TRY(dalloc(e, &e->n_rowloss, Mx));
    TRY(dalloc(e, &e->g_inv_mask, (size_t)128, true));
    TRY(dalloc(e, &e->g_sampled, Mx));
    TRY(dalloc(e, &e->g_rowflag, Mx));
    TRY(dalloc(e, &e->g_rowgap, Mx));
    TRY(dalloc(e, &e->g_nunmask, (size_t)e->tfreq_rows * cfg->max_batch));
    {  // split-K workspaces: S * N <= 12288 for every shape the launcher splits; rows up to the small-batch switch
      if (!strict) {
        const size_t rows = (size_t)round_up((int)std::min<size_t>(Mx, ed::small_max_rows()), 128);
        for (int q = 0; q < 4; ++q) {
          e->gemm_ws[q].partial_floats = rows * 12288;
          TRY(dalloc(e, &e->gemm_ws[q].partial, e->gemm_ws[q].partial_floats));
          e->gemm_ws2[q].partial_floats = rows * 12288;
          TRY(dalloc(e, &e->gemm_ws2[q].partial, e->gemm_ws2[q].partial_floats));
        }
      }
    }
  }
#undef TRY
  // second launch queue for the two-stream forward (esmdiff_set_option(ESMDIFF_OPT_STREAMS) adds more)
  if (hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming) != hipSuccess)
    return bail(fail(e, ESMDIFF_E_HIP, "engine create: fork event: %s", hipGetErrorString(hipGetLastError())));
  if (int r = add_side_stream(e)) return bail(r);
  // needed rows: the row lists of a forward's sub-batches, and their counts where the host reads them (one slot per launch queue)
  if (!strict && kind == 0) {
    const size_t Mx = (size_t)cfg->max_batch * cfg->max_len;
    if (int r = dalloc(e, &e->rows_list, Mx)) return bail(r);
    if (int r = dalloc(e, &e->rows_map, Mx)) return bail(r);
    if (hipHostMalloc((void**)&e->rows_count, 4 * sizeof(int32_t), hipHostMallocDefault) != hipSuccess ||
        hipEventCreateWithFlags(&e->ev_rows, hipEventDisableTiming) != hipSuccess)
      return bail(fail(e, ESMDIFF_E_HIP, "engine create: needed-rows count slot: %s", hipGetErrorString(hipGetLastError())));
  }
  // the launch-skipping switch of the retired timing experiments gave wrong results by construction; a library that finds it in
  // the environment refuses to start rather than silently ignore a request it once honoured
  if (getenv("ESMDIFF_DEBUG_SKIP"))
    return bail(fail(e, ESMDIFF_E_INVALID, "ESMDIFF_DEBUG_SKIP is set, but no build of libesmdiff_hip.so honours it any more: unset it"));
  if (hipDeviceSynchronize() != hipSuccess) return bail(fail(e, ESMDIFF_E_HIP, "engine create: %s", hipGetErrorString(hipGetLastError())));
  *out = e;
  return 0;
}

int esmdiff_engine_create(const esmdiff_config* cfg, const esmdiff_weight* table, int32_t n, int32_t device,
                          esmdiff_engine** out) {
  return create_engine(cfg, table, n, device, 0, out);
}

int esmdiff_decoder_create(const esmdiff_config* cfg, const esmdiff_weight* table, int32_t n, int32_t device,
                           esmdiff_engine** out) {
  if (!cfg) return fail(nullptr, ESMDIFF_E_INVALID, "null argument");
  esmdiff_config c = *cfg;
  c.vocab_out = 23;  // Dim6RotStructureHead.proj: 3 translation + 3 + 3 axis seeds + 14 (unused torsion slots)
  c.freq_dim = 1;
  c.time_conditioning = 0;
  return create_engine(&c, table, n, device, 1, out);
}

int esmdiff_set_frames(esmdiff_engine* e, const float* rot, const float* trans, const uint8_t* has_frame, int32_t B,
                       int32_t L, void* stream) {
  if (!e) return ESMDIFF_E_INVALID;
  if (!rot) {
    e->frames_B = e->frames_L = 0;
    return 0;
  }
  if (!e->has_geom)
    return fail(e, ESMDIFF_E_MISSING, "coordinates given but the weight table had no transformer.blocks.0.geom_attn.* tensors");
  if (!trans || !has_frame) return fail(e, ESMDIFF_E_INVALID, "null argument");
  if (int r = check_bl(e, B, L)) return r;
  HIP_TRY(e, hipSetDevice(e->device));
  hipStream_t st = (hipStream_t)stream;
  const size_t M = (size_t)B * L;
  HIP_TRY(e, hipMemcpyAsync(e->f_rot, rot, M * 9 * sizeof(float), hipMemcpyDeviceToDevice, st));
  HIP_TRY(e, hipMemcpyAsync(e->f_trans, trans, M * 3 * sizeof(float), hipMemcpyDeviceToDevice, st));
  HIP_TRY(e, hipMemcpyAsync(e->f_mask, has_frame, M, hipMemcpyDeviceToDevice, st));
  e->frames_B = B;
  e->frames_L = L;
  return 0;
}

int esmdiff_set_lengths(esmdiff_engine* e, const int32_t* lens, int32_t B) {
  if (!e) return ESMDIFF_E_INVALID;
  if (!lens) {
    e->lens_B = 0;
    e->lens_host.clear();
    e->cur_lens = nullptr;
    return 0;
  }
  if (e->kind != 0) return fail(e, ESMDIFF_E_INVALID, "lengths are for the ESM3 engine, not the structure-token decoder");
  if (B <= 0 || B > e->cfg.max_batch) return fail(e, ESMDIFF_E_INVALID, "B = %d outside 1..max_batch (%d)", B, e->cfg.max_batch);
  for (int b = 0; b < B; ++b)
    if (lens[b] < 3 || lens[b] > e->cfg.max_len)
      return fail(e, ESMDIFF_E_INVALID, "lens[%d] = %d outside 3..max_len (%d): BOS, one residue and EOS at least", b, lens[b], e->cfg.max_len);
  HIP_TRY(e, hipSetDevice(e->device));
  HIP_TRY(e, hipDeviceSynchronize());   // no forward still in flight reads the buffer
  HIP_TRY(e, hipMemcpy(e->lens_dev, lens, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice));
  e->lens_host.assign(lens, lens + B);
  e->lens_B = B;
  e->cur_lens = e->lens_dev;
  return 0;
}

int esmdiff_set_profiling(esmdiff_engine* e, int32_t on) {
  if (!e) return ESMDIFF_E_INVALID;
  e->profiling = on;
  e->ev_used = 0;
  if (on && e->ev.size() < 8192) {  // pre-create part of the event pool outside any timed region
    for (int i = 0; i < 8192; ++i) {
      hipEvent_t ev;
      hipEventCreate(&ev);
      e->ev.push_back(ev);
      e->ev_section.push_back(0);
    }
  }
  memset(e->prof_ms, 0, sizeof e->prof_ms);
  memset(e->prof_launches, 0, sizeof e->prof_launches);
  return 0;
}

int esmdiff_get_profile(esmdiff_engine* e, float* ms_out, int32_t* launches_out) {
  if (!e || !ms_out || !launches_out) return ESMDIFF_E_INVALID;
  prof_collect(e);
  memcpy(ms_out, e->prof_ms, sizeof e->prof_ms);
  memcpy(launches_out, e->prof_launches, sizeof e->prof_launches);
  return 0;
}

}  // extern "C"

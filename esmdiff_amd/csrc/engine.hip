// engine.hip — C ABI of libesmdiff_hip.so (see include/esmdiff_hip.h) and the per-forward launch
// sequence for the ESM3-open structure-token transformer as the reference wires it
// (/root/reference/slm/models/net.py:371-483, model.py:464-492, 543-607).
//
// Per forward (B x L tokens, M = B*L rows):
//   sigma_mlp (2 GEMV)  -> embed -> 48 x [ add+LN -> QKV GEMM -> q/k LN + rotary (V stays in the QKV buffer) ->
//   attention -> out-proj GEMM (bf16 delta / scale) -> add+LN -> FFN-up GEMM (SwiGLU epilogue) -> FFN-down GEMM
//   (bf16 delta) ] -> final LN -> head GEMM (bias+GELU) -> LN -> head GEMM (bias) -> f32 logits -> fused sampler.
// Block 0's geometric attention contributes exactly 0 when coordinates are all-NaN (the DDPM path: affine_mask all
// False, net.py:433-441 with mask_and_zero_frameless=True, net.py:344) and is skipped; with frames set through
// esmdiff_set_frames it runs between the attention branch and the FFN of block 0 (geom.hip).
// Work is enqueued on the caller's stream, plus one engine-owned stream for the second half of a large batch
// (forked and joined with events, see forward()); the engine never synchronises except in create and in the
// profiling readback.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "kernels.h"
#define ed ed16            // the f16 build of the same kernel sources (ed_half.h, esmdiff_amd/build.py)
#include "kernels_ns.inc"
#undef ed

using namespace ed;

namespace {

thread_local std::string g_create_error;

enum Section { S_EMBED = 0, S_LN, S_QKV, S_QKROPE, S_ATTN, S_OUT, S_FFN_UP, S_FFN_DOWN, S_HEAD, S_SAMPLER, S_COUNT };

// One linear's weight, held in the one form its engine runs it in.  create_engine chooses the form per group of weights
// (body_form / head_form / plain_form), load_linear fills the slot, and the forwards dispatch on `form`.  An accessor of
// another form than the slot's gives null.
struct Linear {
  // W16: the engine's 16-bit type (bf16, or f16 on an f16 engine), the FFN-up's rows interleaved gate / up.  F32 (csrc/strict.hip):
  // float32 in the checkpoint's own row order, no padding, no interleave.  SPLIT (csrc/gemm_split.hip): scaled f16 plane
  // triples, and inv = 1 / scale.
  enum Form : uint8_t { NONE, W16, F32, SPLIT };
  Form form = NONE;
  void* w = nullptr;
  float inv = 1.f;
  const bf16_t* w16() const { return form == W16 ? static_cast<const bf16_t*>(w) : nullptr; }
  const float* f32() const { return form == F32 ? static_cast<const float*>(w) : nullptr; }
  const uint16_t* split() const { return form == SPLIT ? static_cast<const uint16_t*>(w) : nullptr; }
};

struct Layer {
  float *ln1_w = nullptr, *ln1_b = nullptr, *q_ln_w = nullptr, *k_ln_w = nullptr, *ln2_w = nullptr, *ln2_b = nullptr;
  Linear w_qkv, w_out, w_up, w_down;
  // F32_SPLIT: the power-of-two operand scales of the split attention (attention_split.hip), from rigorous bounds at create
  float att_qk = 1.f, att_v = 1.f;
};

}  // namespace

struct esmdiff_engine {
  esmdiff_config cfg{};
  int kind = 0;  // 0: ESM3 structure-token transformer (the sampler's network); 1: VQ-VAE structure-token decoder
  int device = 0;
  std::string err;
  std::vector<void*> allocs;
  // weights
  std::vector<Layer> layers;
  float *e_seq = nullptr, *e_struct = nullptr, *cvec = nullptr;
  float *final_ln_w = nullptr;
  Linear head_w0, head_w3;   // head_w3: rows padded to vocab_pad except as F32
  float *head_b0 = nullptr, *head_ln_w = nullptr, *head_ln_b = nullptr, *head_b3 = nullptr;
  float *sig_w1 = nullptr, *sig_b1 = nullptr, *sig_w2 = nullptr, *sig_b2 = nullptr;
  float *rope_cos = nullptr, *rope_sin = nullptr;
  int vocab_pad = 0;
  // decoder only (kind 1): esm's plddt_head = RegressionHead(d, 50) on the same final hidden state (optional weights)
  bool has_plddt = false;
  int plddt_bins = 0, ld_plddt = 0;
  Linear pl_w0, pl_w3;
  // decoder only: esm's pairwise_classification_head (PairwisePredictionHead(d, 128, 128, 224 bins, no bias)); only the
  // 64 predicted-aligned-error bins (rows 160..223 of linear2) are evaluated: pTM and the PAE matrix (csrc/pairwise.hip)
  bool has_pair = false;
  Linear pw_down, pw_l1, pw_l2;   // W16 or F32, never SPLIT
  bf16_t* pair_qk = nullptr;
  float *pw_ln_w = nullptr, *pw_ln_b = nullptr, *zeros128 = nullptr, *tm_rows = nullptr, *ptm_dev = nullptr;
  bf16_t *pair_x = nullptr, *pair_h = nullptr;   // pair rows of a chunk of samples (allocated on first use)
  float* pair_logits = nullptr;
  int64_t pair_rows_cap = 0;
  float *pl_b0 = nullptr, *pl_ln_w = nullptr, *pl_ln_b = nullptr, *pl_b3 = nullptr, *pl_logits = nullptr;
  // block 0 geometric attention (optional weights; live only while frames are set)
  bool has_geom = false;
  int v_heads = 0;  // rows of geom_attn.proj.weight / 15
  float *g_snorm_w = nullptr, *g_wrot = nullptr, *g_wdist = nullptr;
  Linear g_proj, g_out;   // SPLIT only as a pair: when both shapes fit the split GEMM
  bf16_t *gp = nullptr, *gctx = nullptr;
  float *f_rot = nullptr, *f_trans = nullptr;
  uint8_t* f_mask = nullptr;
  int frames_B = 0, frames_L = 0;
  // ragged batch (esmdiff_set_lengths): sample b valid on tokens [0, lens_host[b]) while lens_B > 0; cur_lens is what the next
  // forward's attention reads (lens_dev, or lens_sub_dev for the noise-removal sub-batch of esmdiff_ddpm_sample)
  int32_t *lens_dev = nullptr, *lens_sub_dev = nullptr;
  const int32_t* cur_lens = nullptr;
  std::vector<int32_t> lens_host;
  int lens_B = 0;
  // workspace
  float* x = nullptr;
  bf16_t *h = nullptr, *h2 = nullptr, *qkv = nullptr, *q = nullptr, *k = nullptr, *ctx = nullptr,
         *mid = nullptr, *dlt = nullptr, *dlt2 = nullptr;
  float *logits = nullptr, *cond = nullptr, *sig_hidden = nullptr, *tfreq = nullptr, *g_entropy = nullptr;
  int32_t *g_sampled = nullptr, *g_nunmask = nullptr;
  uint8_t* g_rowflag = nullptr;   // esmdiff_gibbs_step_rows with bounds: per-row report, reduced per prompt by the select kernel
  float* g_rowgap = nullptr;
  int ld_logits = 0, tfreq_rows = 0;
  int sigma_rows = 1;   // sinusoid rows the next forward reads: 1 (all samples share sigma) or B (esmdiff_forward_logits_sigmas)
  // two-stream forward: the second half of a large batch runs on `side`, forked/joined with events
  std::vector<hipStream_t> side;
  std::vector<hipEvent_t> ev_join;
  hipEvent_t ev_fork = nullptr;
  // F32_SPLIT, opt-in (esmdiff_set_small_batch_splitk): at <= splitk_max_rows rows the two residual linears (6 column tiles each)
  // run K-sliced (out-proj 3 slices, FFN-down 4) so that a small batch uses more than a few dozen CUs; partial planes in sk_parts
  bool splitk_small = false;
  float* sk_parts = nullptr;
  int64_t dual_min_tokens = 2200;  // esmdiff_set_option(ESMDIFF_OPT_DUAL_MIN_TOKENS): two streams from this many tokens, see forward()
  int n_streams = 2;         // esmdiff_set_option(ESMDIFF_OPT_STREAMS): sub-batch launch queues of the 16-bit forward
  ed::GemmWorkspace gemm_ws[4] = {};  // split-K partials of the small-M GEMM path, one per launch queue
  ed::GemmWorkspace gemm_ws2[4] = {}; // ... a second set: the out-projection's K slices stay live next to the FFN-down's
  // precision = ESMDIFF_PRECISION_F32: float32 weights / activations (forward_strict); the 16-bit workspace above stays null
  bool strict = false;
  // precision = ESMDIFF_PRECISION_F32_SPLIT: forward_strict with every large linear as three f16 MFMA passes over split
  // operands (gemm_split.hip); a2 / rs: the split activation rows feeding the next linear and their row scales
  bool split = false;
  bool f16 = false;          // precision = ESMDIFF_PRECISION_F16: the bf16 engine's launch sequence on the ed16 kernels
  bool head_split = false;   // bf16 engine with esmdiff_config.head_precision = 1: final LayerNorm + head on the split kernels
  uint16_t* a2 = nullptr;
  float* rs = nullptr;
  uint32_t* scratch_bits = nullptr;
  float *fgp = nullptr, *fgctx = nullptr;
  float *fpair_x = nullptr, *fpair_h = nullptr;   // pairwise head in float32
  float *fh = nullptr, *fh2 = nullptr, *fqkv = nullptr, *fq = nullptr, *fk = nullptr, *fctx = nullptr, *fgu = nullptr,   // (fgu: F32 engines only)
        *fmid = nullptr, *fpair_qk = nullptr;
  // step-0 sharing (esmdiff_set_step0_sharing): when every sample of a sampling call starts from identical inputs, the first
  // forward runs on a sub-batch and all samples draw from its logits; counters of the work really executed
  int step0_share = 0;
  int32_t* flag_dev = nullptr;
  // exact skip of the noise-removal forward (esmdiff_set_final_skip): only samples that still hold a MASK run forward T + 1
  int final_skip = 0;
  int32_t *has_dev = nullptr, *idx_dev = nullptr;
  int64_t *cx = nullptr, *cseq = nullptr;   // compacted token rows of those samples; esmdiff_nelbo_eval: the masked tokens xt and the coupled sequence
  float* n_rowloss = nullptr;               // esmdiff_nelbo_rows: log_p * weight per token row, read by the per-sample reduction
  // gibbs options (esmdiff_set_gibbs_options): 0 entropy-ordered / 1 random positions; bit v of inv_mask = id v is never drawn
  int g_strategy = 0;
  uint32_t* g_inv_mask = nullptr;
  bool g_inv_on = false;
  int64_t stat_forwards = 0, stat_rows = 0;
  int last_B = 0, last_L = 0;       // shape of the last forward, and whether its last FFN-down delta is still outside x
  bool last_pending_delta = false;  // (regular bf16 path: the final add+LayerNorm forms x + dF in registers only)
  // profiling
  int profiling = 0;  // 0 off, 1 every launch, 2 only the dominant kernel (FFN-up GEMM)
  std::vector<hipEvent_t> ev;
  std::vector<int> ev_section;
  size_t ev_used = 0;
  float prof_ms[16] = {0};
  int prof_launches[16] = {0};
};

namespace {

int fail(esmdiff_engine* e, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (e) e->err = buf; else g_create_error = buf;
  return code;
}

#define HIP_TRY(e, call)                                                                         \
  do {                                                                                           \
    hipError_t _s = (call);                                                                      \
    if (_s != hipSuccess) return fail(e, ESMDIFF_E_HIP, "%s: %s", #call, hipGetErrorString(_s)); \
  } while (0)

template <typename T>
int dalloc(esmdiff_engine* e, T** p, size_t n_elems, bool zero = false) {
  void* v = nullptr;
  hipError_t s = hipMalloc(&v, n_elems * sizeof(T) + 256);
  if (s != hipSuccess) return fail(e, ESMDIFF_E_HIP, "hipMalloc(%zu): %s", n_elems * sizeof(T), hipGetErrorString(s));
  if (zero) hipMemset(v, 0, n_elems * sizeof(T) + 256);
  e->allocs.push_back(v);
  *p = reinterpret_cast<T*>(v);
  return 0;
}

struct Table {
  std::map<std::string, const esmdiff_weight*> m;
  const esmdiff_weight* find(const std::string& name) const {
    auto it = m.find(name);
    if (it != m.end()) return it->second;
    it = m.find("net." + name);
    return it == m.end() ? nullptr : it->second;
  }
};

int64_t numel(const esmdiff_weight* w) {
  int64_t n = 1;
  for (int i = 0; i < w->ndim; ++i) n *= w->shape[i];
  return n;
}

int need(esmdiff_engine* e, const Table& t, const std::string& name, std::initializer_list<int64_t> shape,
         const esmdiff_weight** out) {
  const esmdiff_weight* w = t.find(name);
  if (!w) return fail(e, ESMDIFF_E_MISSING, "missing weight '%s' (state dict is loaded strictly, checkpoint_utils.py:64)", name.c_str());
  if (w->ndim != (int)shape.size()) return fail(e, ESMDIFF_E_SHAPE, "weight '%s': ndim %d, expected %zu", name.c_str(), w->ndim, shape.size());
  int i = 0;
  for (int64_t s : shape) {
    if (w->shape[i] != s) return fail(e, ESMDIFF_E_SHAPE, "weight '%s': dim %d is %lld, expected %lld", name.c_str(), i, (long long)w->shape[i], (long long)s);
    ++i;
  }
  if (w->dtype != ESMDIFF_F32 && w->dtype != ESMDIFF_BF16) return fail(e, ESMDIFF_E_SHAPE, "weight '%s': unsupported dtype %d", name.c_str(), w->dtype);
  if (!w->data) return fail(e, ESMDIFF_E_INVALID, "weight '%s': null data", name.c_str());
  *out = w;
  return 0;
}

// vectors and embeddings: float32, the tail up to pad_to elements zero
int load_f32(esmdiff_engine* e, const Table& t, const std::string& name, std::initializer_list<int64_t> shape, float** dst,
             int64_t pad_to = 0) {
  const esmdiff_weight* w;
  if (int r = need(e, t, name, shape, &w)) return r;
  const int64_t n = numel(w), n_p = pad_to > n ? pad_to : n;
  if (int r = dalloc(e, dst, (size_t)n_p, n_p != n)) return r;
  HIP_TRY(e, launch_to_f32(w->data, w->dtype, *dst, n, 0));
  return 0;
}

// A linear's weight [rows, K] into its slot in the given form.  W16 and SPLIT zero-pad the rows to pad_rows and, with
// swiglu_h = FH, interleave the FFN-up's gate / up rows for the SwiGLU epilogue; F32 does neither (launch_gemm_f32 bounds
// its rows and the SwiGLU is its own pass).  SPLIT: planes [rows_p, 3 K] + the inverse scale.
int load_linear(esmdiff_engine* e, const Table& t, const std::string& name, std::initializer_list<int64_t> shape, Linear::Form form,
                Linear* dst, int64_t pad_rows = 0, int swiglu_h = 0) {
  const esmdiff_weight* w;
  if (int r = need(e, t, name, shape, &w)) return r;
  const int64_t n = numel(w), rows = w->shape[0], K = n / rows;
  const int64_t rows_p = form != Linear::F32 && pad_rows > rows ? pad_rows : rows;
  if (form == Linear::SPLIT) {
    if (K % 128 || rows_p % 256) return fail(e, ESMDIFF_E_SHAPE, "weight '%s': [%lld, %lld] does not fit the split GEMM (rows %% 256, K %% 128)", name.c_str(), (long long)rows_p, (long long)K);
    uint16_t* p;
    if (int r = dalloc(e, &p, (size_t)(rows_p * 3 * K), rows_p != rows)) return r;
    dst->w = p;
    HIP_TRY(e, split_weight(w->data, w->dtype, p, rows, (int)K, e->scratch_bits, &dst->inv, swiglu_h));
  } else if (form == Linear::F32) {
    float* p;
    if (int r = dalloc(e, &p, (size_t)n)) return r;
    dst->w = p;
    HIP_TRY(e, launch_to_f32(w->data, w->dtype, p, n, 0));
  } else {
    bf16_t* p;
    if (int r = dalloc(e, &p, (size_t)(rows_p * K), rows_p != rows)) return r;
    dst->w = p;
    if (swiglu_h) {
      if ((e->f16 ? ed16::launch_interleave_swiglu(w->data, w->dtype, p, swiglu_h, (int)K, 0) : ed::launch_interleave_swiglu(w->data, w->dtype, p, swiglu_h, (int)K, 0)) != hipSuccess)
        return fail(e, ESMDIFF_E_HIP, "interleave_swiglu launch failed");
    } else {
      HIP_TRY(e, e->f16 ? ed16::launch_to_bf16(w->data, w->dtype, p, n, 0) : ed::launch_to_bf16(w->data, w->dtype, p, n, 0));
    }
  }
  dst->form = form;
  return 0;
}

// The form of a group of weights, chosen once at create.  plain_form, the engine's non-split form: the pairwise head always, and
// block 0's geometric pair unless BOTH its shapes fit the split GEMM (create_engine).  body_form: the block stack's linears and
// the second (pLDDT / sequence) head's.  head_form: the output head's, SPLIT also under head_precision = 1.
Linear::Form plain_form(const esmdiff_engine* e) { return e->strict ? Linear::F32 : Linear::W16; }
Linear::Form body_form(const esmdiff_engine* e) { return e->split ? Linear::SPLIT : plain_form(e); }
Linear::Form head_form(const esmdiff_engine* e) { return e->head_split ? Linear::SPLIT : body_form(e); }

// RAII-less section timer: when profiling, records an event before/after each launch.
struct Prof {
  esmdiff_engine* e;
  hipStream_t s;
  void mark(int section) {
    if (!e->profiling || (e->profiling == 2 && section != S_FFN_UP)) return;
    if (e->ev_used + 2 > e->ev.size()) {
      for (int i = 0; i < 4096; ++i) {
        hipEvent_t ev;
        hipEventCreate(&ev);
        e->ev.push_back(ev);
        e->ev_section.push_back(0);
      }
    }
    e->ev_section[e->ev_used] = section;
    hipEventRecord(e->ev[e->ev_used++], s);
  }
};

// One launch as a timed section: needs `e` and a Prof `p` in scope.
#define RUN(section, call)   \
  do {                       \
    p.mark(section);         \
    HIP_TRY(e, (call));      \
    p.mark(section);         \
  } while (0)

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

// Workspace of one sub-batch: the engine's buffers are all sample-major, so a sub-batch is a pointer offset.
struct Part {
  const int64_t *seq, *xtok;
  float *x, *logits, *pl_logits;
  bf16_t *h, *h2, *qkv, *q, *k, *ctx, *mid, *dlt, *dlt2;
  bf16_t *gp, *gctx;
  uint16_t* a2;   // head_split: split rows feeding the two head linears, their row scales, the f32 Linear-0 output
  float *rs, *fh2;
  const float *f_rot, *f_trans;
  const uint8_t* f_mask;
  const int32_t* lens;   // ragged batch: this sub-batch's lengths (device), else null
  int b0, B;             // first sample of the sub-batch in the batch, and how many
  hipStream_t st;
  const ed::GemmWorkspace* gws;
  const ed::GemmWorkspace* gws2;
};

Part make_part(esmdiff_engine* e, const int64_t* seq, const int64_t* xtok, float* logits, int ld, int b0, int nb, int L,
               hipStream_t st, int queue) {
  const esmdiff_config& c = e->cfg;
  const int64_t t0 = (int64_t)b0 * L, D = c.d_model;
  return Part{seq + t0, xtok + t0, e->x + t0 * D, logits + t0 * ld, e->pl_logits ? e->pl_logits + t0 * e->ld_plddt : nullptr, e->h + t0 * D, e->h2 + t0 * D, e->qkv + t0 * 3 * D,
              e->q + t0 * D, e->k + t0 * D, e->ctx + t0 * D, e->mid + t0 * c.ffn_hidden, e->dlt + t0 * D, e->dlt2 + t0 * D,
              e->gp ? e->gp + t0 * 15 * e->v_heads : nullptr, e->gctx ? e->gctx + t0 * 3 * e->v_heads : nullptr,
              e->a2 ? e->a2 + t0 * 3 * D : nullptr, e->rs ? e->rs + t0 : nullptr, e->fh2 ? e->fh2 + t0 * D : nullptr,
              e->f_rot ? e->f_rot + t0 * 9 : nullptr, e->f_trans ? e->f_trans + t0 * 3 : nullptr,
              e->f_mask ? e->f_mask + t0 : nullptr, e->cur_lens ? e->cur_lens + b0 : nullptr, b0, nb, st,
              e->gemm_ws[queue].partial ? &e->gemm_ws[queue] : nullptr,
              e->gemm_ws2[queue].partial ? &e->gemm_ws2[queue] : nullptr};
}

// How forward() will cut a batch: number of sub-batch streams, and whether the sub-batches take the small-batch path.
// The PATH (small-batch K-slice planes vs the regular kernels: two summation orders, logits that differ at rounding level) is a
// function of (B, L) alone — it is what the default options choose.  esmdiff_set_option may change how many launch queues run
// the batch, never the path: a stream count or token threshold that would push the sub-batches across small_max_rows() is
// reduced until they stay on the default path's side (tests/test_gpu_fullwidth.py::test_stream_options_never_change_a_bit).
constexpr int kDefaultStreams = 2;
constexpr int64_t kDefaultDualMinTokens = 2200;
constexpr int64_t kDualSmallMaxTokens = 1024;      // the all-small two-queue window reaches up to this many tokens, see forward()
constexpr int64_t kStrictDualMinTokens = 8192;     // F32_SPLIT: two sub-batch streams from this many tokens
constexpr int kSplitkMaxRows = 4096;               // esmdiff_set_small_batch_splitk: K-sliced residual linears up to this many rows
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
  const int np_def = parts_for(e, B, L, kDefaultStreams, kDefaultDualMinTokens);
  const bool small = parts_small(e, B, L, np_def);
  int np = parts_for(e, B, L, e->n_streams, e->dual_min_tokens);
  while (np > 1 && parts_small(e, B, L, np) != small) --np;
  if (parts_small(e, B, L, np) != small) np = np_def;
  return BatchPlan{np, small};
}
int plan_parts(const esmdiff_engine* e, int B, int L) { return plan_batch(e, B, L).np; }
bool plan_small(const esmdiff_engine* e, int B, int L) { return plan_batch(e, B, L).small; }
// Step-0 sharing: the number of leading samples whose forward gives, bit for bit, the logits every sample of an
// all-identical batch of B would get — a sub-batch that takes the same (regular) dispatch path as the whole batch
// (tests: test_logits_across_dispatch_paths) — or B when nothing can be saved.
int shared_forward_batch(const esmdiff_engine* e, int B, int L) {
  if (e->strict) return 1;                       // every row's result is independent of the batch (fixed K order, one path)
  if (plan_small(e, B, L)) return B;             // small-batch path: the plane count is fixed, but keep it simple: no sharing
  for (int b = 1; b < B; ++b)
    if (!plan_small(e, b, L) && (int64_t)b * L >= ed::small_max_rows()) return b;
  return B;
}

// precision = F32: the same network in float32 end to end (csrc/strict.hip).  One stream, one launch per op, residual
// adds in the branch GEMMs' epilogues as x + r / scaling_factor (esm's own expression).  Sections are timed like the
// bf16 path's.  Block 0's geometric branch runs between the attention and the FFN branch while frames are set.
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

struct SPart {   // one sub-batch of a strict forward: the engine's float32 workspace at a row offset, on its own stream
  const int64_t *seq, *xtok;
  float *x, *fh, *fh2, *fqkv, *fq, *fk, *fctx, *fgu, *fmid, *fgp, *fgctx, *fpair_qk, *logits, *pl_logits;   // fgu: F32 engines only
  uint16_t* a2;   // split rows feeding the next linear
  float* rs;
  const float *f_rot, *f_trans;
  const uint8_t* f_mask;
  const int32_t* lens;   // ragged batch: this sub-batch's lengths (device), else null
  int b0, B;             // first sample of the sub-batch in the batch, and how many
  hipStream_t st;
};

// sub-batch streams of a float32-grade forward (one function for forward_strict and esmdiff_describe_plan).  (r06: with frames set
// the two-queue forward was not deterministic while geom_attention_kernel held packed float ops beside the other queue's GEMM: geom.hip.)
static int strict_parts(const esmdiff_engine* e, int B, int L) {
  return (e->split && !e->side.empty() && e->profiling != 1 && B >= 2 && (int64_t)B * L >= kStrictDualMinTokens) ? 2 : 1;
}

static int strict_part(esmdiff_engine* e, const SPart& w, const float* cond, int ld, int L) {
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

int forward_strict(esmdiff_engine* e, const int64_t* seq, const int64_t* xtok, const float* t_freq_dev, float* logits,
                   int ld, int B, int L, hipStream_t st) {
  const esmdiff_config& c = e->cfg;
  const int D = c.d_model, FH = c.ffn_hidden;
  Prof p{e, st};
  const float* cond = nullptr;
  if (t_freq_dev && e->sig_w1) {
    RUN(S_EMBED, launch_sigma_mlp(t_freq_dev, e->sig_w1, e->sig_b1, e->sig_w2, e->sig_b2, e->sig_hidden, e->cond, c.freq_dim, D, st,
                                  e->sigma_rows));
    cond = e->cond;
  }
  const bool geom = e->has_geom && e->frames_B > 0;
  if (geom && (e->frames_B != B || e->frames_L != L))
    return fail(e, ESMDIFF_E_INVALID, "frames were set for B=%d L=%d, forward called with B=%d L=%d", e->frames_B, e->frames_L, B, L);
  // F32_SPLIT at large batches: two sub-batches on two streams, as the bf16 engine does (every kernel's row results are
  // independent of the batch, so the cut changes no bit): the persistent split GEMMs leave CUs idle in their last round and the
  // other sub-batch's kernels fill them.
  const int np = strict_parts(e, B, L);
  const int64_t WS = 3 * (int64_t)std::max(D, FH);
  SPart parts[2];
  for (int pi = 0; pi < np; ++pi) {
    const int b0 = (int)((int64_t)B * pi / np), b1 = (int)((int64_t)B * (pi + 1) / np);
    const int64_t t0 = (int64_t)b0 * L;
    auto off = [&](float* p_, int64_t stride) { return p_ ? p_ + t0 * stride : nullptr; };
    parts[pi] = SPart{seq + t0, xtok + t0, off(e->x, D), off(e->fh, D), off(e->fh2, D), off(e->fqkv, 3 * D), off(e->fq, D), off(e->fk, D),
                      off(e->fctx, D), off(e->fgu, 2 * FH), off(e->fmid, FH), off(e->fgp, 15 * e->v_heads), off(e->fgctx, 3 * e->v_heads),
                      off(e->fpair_qk, 128), logits + t0 * ld, off(e->pl_logits, e->ld_plddt), e->a2 ? e->a2 + t0 * WS : nullptr,
                      e->rs ? e->rs + t0 : nullptr, e->f_rot ? e->f_rot + t0 * 9 : nullptr, e->f_trans ? e->f_trans + t0 * 3 : nullptr,
                      e->f_mask ? e->f_mask + t0 : nullptr, e->cur_lens ? e->cur_lens + b0 : nullptr, b0, b1 - b0, pi == 0 ? st : e->side[pi - 1]};
  }
  if (int r = fork_streams(e, st, np)) return r;
  for (int pi = 0; pi < np; ++pi)   // (per-sample sigmas: the part's first conditioning row)
    if (int r = strict_part(e, parts[pi], cond && e->sigma_rows > 1 ? cond + (int64_t)parts[pi].b0 * D : cond, ld, L)) return r;
  return join_streams(e, st, np);
}

#define KN ed
#define ED_FWD_NAME forward_bf16
#include "engine_forward.inc"
#undef KN
#undef ED_FWD_NAME
#define KN ed16
#define ED_FWD_NAME forward_f16
#include "engine_forward.inc"
#undef KN
#undef ED_FWD_NAME

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
int forward(esmdiff_engine* e, const int64_t* seq, const int64_t* xtok, const float* t_freq_dev, float* logits,
            int ld, int B, int L, hipStream_t st) {
  e->last_B = B;
  e->last_L = L;
  e->last_pending_delta = false;
  if (e->strict) {
    e->stat_forwards += 1;
    e->stat_rows += (int64_t)B * L;
    return forward_strict(e, seq, xtok, t_freq_dev, logits, ld, B, L, st);
  }
  return e->f16 ? forward_f16(e, seq, xtok, t_freq_dev, logits, ld, B, L, st) : forward_bf16(e, seq, xtok, t_freq_dev, logits, ld, B, L, st);
}

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
  HIP_TRY(e, hipMemcpy(e->g_inv_mask, mask, sizeof mask, hipMemcpyHostToDevice));   // synchronous: ordered against earlier launches
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
  if (e->strict) {
    const int64_t tokens = (int64_t)B * L;
    const int np = strict_parts(e, B, L);
    n += snprintf(at(), room(), " streams=%d path=%s k_sliced_small_batches=%d", np,
                  e->split ? "split(3 f16 MFMA passes, 256x256w4)" : "strict(f32 MFMA)", e->sk_parts && tokens <= kSplitkMaxRows ? 1 : 0);
  } else {
    const int np = plan_parts(e, B, L);
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
  n += snprintf(at(), room(), " step0_sharing=%d final_skip=%d small_max_rows=%d", e->step0_share, e->final_skip, ed::small_max_rows());
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

int esmdiff_abi_version(void) { return ESMDIFF_ABI_VERSION; }

const char* esmdiff_last_error(const esmdiff_engine* eng) { return eng ? eng->err.c_str() : g_create_error.c_str(); }

void esmdiff_engine_destroy(esmdiff_engine* e) {
  if (!e) return;
  hipSetDevice(e->device);
  hipDeviceSynchronize();
  for (void* p : e->allocs) hipFree(p);
  for (void* p : {(void*)e->pair_x, (void*)e->pair_h, (void*)e->pair_logits})  // the pairwise head's lazily sized workspace
    if (p) hipFree(p);
  for (hipEvent_t ev : e->ev) hipEventDestroy(ev);
  if (e->ev_fork) hipEventDestroy(e->ev_fork);
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
    g_create_error = e->err;
    esmdiff_engine_destroy(e);
    return code;
  };
  if (hipSetDevice(device) != hipSuccess) return bail(fail(e, ESMDIFF_E_HIP, "hipSetDevice failed"));

  Table t;
  for (int i = 0; i < n; ++i)
    if (table[i].name) t.m[table[i].name] = &table[i];

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
    TRY(load_linear(e, t, b + "attn.layernorm_qkv.1.weight", {3 * D, D}, bf, &ly.w_qkv));
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
    TRY(load_linear(e, t, b + "attn.out_proj.weight", {D, D}, bf, &ly.w_out));
    TRY(load_f32(e, t, b + "ffn.0.weight", {D}, &ly.ln2_w));
    TRY(load_f32(e, t, b + "ffn.0.bias", {D}, &ly.ln2_b));
    // FFN-up with the SwiGLU in the GEMM's epilogue: rows interleaved gate / up (W16, and SPLIT: mid leaves it as f32 and is split
    // with its row's own scale, forward_strict); F32 keeps the checkpoint's order
    TRY(load_linear(e, t, b + "ffn.1.weight", {2 * FH, D}, bf, &ly.w_up, 0, FH));
    TRY(load_linear(e, t, b + "ffn.3.weight", {D, FH}, bf, &ly.w_down));
  }
  TRY(load_f32(e, t, stack + "norm.weight", {D}, &e->final_ln_w));
  TRY(load_linear(e, t, head0 + "weight", {D, D}, hf, &e->head_w0));
  TRY(load_f32(e, t, head0 + "bias", {D}, &e->head_b0));
  TRY(load_f32(e, t, head2 + "weight", {D}, &e->head_ln_w));
  TRY(load_f32(e, t, head2 + "bias", {D}, &e->head_ln_b));
  e->vocab_pad = round_up(V, 256);  // 4101 -> 4352: 17 column tiles of the 256x256 kernel (the 128x128 kernel took 0.40 ms at M = 25 800)
  TRY(load_linear(e, t, head3 + "weight", {V, D}, hf, &e->head_w3, e->vocab_pad));
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
      TRY(load_linear(e, t, sh + "0.weight", {D, D}, bf, &e->pl_w0));
      TRY(load_f32(e, t, sh + "0.bias", {D}, &e->pl_b0));
      TRY(load_f32(e, t, sh + "2.weight", {D}, &e->pl_ln_w));
      TRY(load_f32(e, t, sh + "2.bias", {D}, &e->pl_ln_b));
      TRY(load_linear(e, t, sh + "3.weight", {nb, D}, bf, &e->pl_w3, split ? 256 : 128));   // one column tile of its GEMM
      TRY(load_f32(e, t, sh + "3.bias", {nb}, &e->pl_b3, 128));
      e->has_plddt = true;
    }
  }
  if (kind == 1) {
    if (t.find("pairwise_classification_head.linear2.weight")) {
      const std::string ph = "pairwise_classification_head.";
      TRY(load_linear(e, t, ph + "downproject.weight", {128, D}, pf, &e->pw_down));
      TRY(load_linear(e, t, ph + "linear1.weight", {128, 128}, pf, &e->pw_l1));
      TRY(load_f32(e, t, ph + "norm.weight", {128}, &e->pw_ln_w));
      TRY(load_f32(e, t, ph + "norm.bias", {128}, &e->pw_ln_b));
      // rows [distogram 64 | direction 96 | PAE 64]; padded so that the 128-row W16 GEMM tile starting at row 160 stays inside
      TRY(load_linear(e, t, ph + "linear2.weight", {224, 128}, pf, &e->pw_l2, 384));
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
    TRY(load_linear(e, t, ga + "proj.weight", {15 * VH, D}, gf, &e->g_proj));
    TRY(load_linear(e, t, ga + "out_proj.weight", {D, 3 * VH}, gf, &e->g_out));
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

// pTM (and optionally the PAE matrix) of the samples just decoded: pair rows of whole samples at a time through
// linear1 -> GELU -> LayerNorm -> linear2[PAE bins] on the MFMA GEMM, then the bin reduction (csrc/pairwise.hip).
static int pairwise_confidence(esmdiff_engine* e, const int64_t* tokens, float* ptm, float* pae, int B, int L, hipStream_t st) {
  const int64_t LL = (int64_t)L * L;
  // chunk of whole samples: ~1.5 GB of pair rows at most (768 B per row: features, hidden, 64 f32 logits; 1280 B in float32)
  const size_t esz = e->strict ? 4 : 2;
  int cb = (int)std::max<int64_t>(1, std::min<int64_t>(B, (int64_t)(1536ll << 20) / (LL * (int64_t)(256 * esz + 256))));
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

int esmdiff_forward_logits(esmdiff_engine* e, const int64_t* seq, const int64_t* x, const float* t_freq,
                           float* logits_out, int32_t ld_logits, int32_t B, int32_t L, void* stream) {
  if (e && e->kind != 0) return fail(e, ESMDIFF_E_INVALID, "this engine is a structure-token decoder (esmdiff_decoder_create)");
  if (!e) return ESMDIFF_E_INVALID;
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
  hipStream_t st = (hipStream_t)stream;
  const size_t M = (size_t)B * L, D = e->cfg.d_model;
  HIP_TRY(e, hipMemcpyAsync(out, e->x, M * D * sizeof(float), hipMemcpyDeviceToDevice, st));
  // regular bf16 path: the last block's FFN-down delta is added by the final add+LayerNorm in registers; add it here the
  // same way (out = out + dF, one f32 addition per element; the normalised row goes to a scratch buffer nobody reads)
  if (e->last_pending_delta)
    HIP_TRY(e, e->f16 ? ed16::launch_add_layernorm_bf16(out, e->dlt, nullptr, 1, e->final_ln_w, nullptr, e->q, (int)M, (int)D, st)
                      : ed::launch_add_layernorm_bf16(out, e->dlt, nullptr, 1, e->final_ln_w, nullptr, e->q, (int)M, (int)D, st));
  return 0;
}

int esmdiff_get_sequence_logits(esmdiff_engine* e, float* out, int32_t ld_out, int32_t B, int32_t L, void* stream) {
  if (!e) return ESMDIFF_E_INVALID;
  if (e->kind != 0 || !e->has_plddt) return fail(e, ESMDIFF_E_MISSING, "no output_heads.sequence_head.* tensors were in the weight table");
  if (!out || ld_out < e->plddt_bins) return fail(e, ESMDIFF_E_INVALID, "bad output");
  if (B != e->last_B || L != e->last_L || B <= 0)
    return fail(e, ESMDIFF_E_INVALID, "sequence logits of a (%d, %d) forward requested, the last forward was (%d, %d)", B, L, e->last_B, e->last_L);
  HIP_TRY(e, hipMemcpy2DAsync(out, (size_t)ld_out * 4, e->pl_logits, (size_t)e->ld_plddt * 4, (size_t)e->plddt_bins * 4, (size_t)B * L,
                              hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return 0;
}

int esmdiff_ddpm_step(esmdiff_engine* e, int64_t* x_inout, const float* logits, int32_t ld_logits,
                      float mc_t, float mc_s, int32_t final_, const float* u, const esmdiff_rng* rng,
                      int32_t step, int32_t B, int32_t L, void* stream) {
  if (!e) return ESMDIFF_E_INVALID;
  if (!x_inout || !logits) return fail(e, ESMDIFF_E_INVALID, "null pointer");
  if (!final_ && !u && !rng) return fail(e, ESMDIFF_E_INVALID, "need explicit uniforms or an rng");
  if (B <= 0 || L <= 0 || ld_logits < e->cfg.vocab_out) return fail(e, ESMDIFF_E_INVALID, "bad shape");
  if (e->cfg.vocab_out <= ESMDIFF_MASK_ID) return fail(e, ESMDIFF_E_INVALID, "ddpm needs the 4101-way head (mask column)");
  Prof p{e, (hipStream_t)stream};
  p.mark(S_SAMPLER);
  HIP_TRY(e, launch_ddpm_step(x_inout, logits, ld_logits, e->cfg.vocab_out, mc_t, mc_s, final_, u, u ? 0 : 1,
                              rng ? rng->seed : 0, rng ? rng->sample_offset : 0, step, B, L, (hipStream_t)stream));
  p.mark(S_SAMPLER);
  return 0;
}

int esmdiff_ddpm_step_margin(esmdiff_engine* e, int64_t* x_inout, const float* logits, int32_t ld_logits,
                             float mc_t, float mc_s, int32_t final_, const esmdiff_rng* rng, int32_t step,
                             int32_t B, int32_t L, float margin, int32_t* sample_flags, void* stream) {
  if (!e) return ESMDIFF_E_INVALID;
  if (!x_inout || !logits || !sample_flags || !rng) return fail(e, ESMDIFF_E_INVALID, "null pointer");
  if (B <= 0 || L <= 0 || ld_logits < e->cfg.vocab_out) return fail(e, ESMDIFF_E_INVALID, "bad shape");
  if (e->cfg.vocab_out <= ESMDIFF_MASK_ID) return fail(e, ESMDIFF_E_INVALID, "ddpm needs the 4101-way head (mask column)");
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
  if (e->cfg.vocab_out <= ESMDIFF_MASK_ID) return fail(e, ESMDIFF_E_INVALID, "ddpm needs the 4101-way head (mask column)");
  if (int r = check_lens(e, B, L)) return r;   // (padding holds no MASK: the step leaves it as it is)
  if ((sample_flags || sample_min_gap) && !(margin_ratio >= 1.f && margin_diff >= 0.f))
    return fail(e, ESMDIFF_E_INVALID, "margins (%g, %g): a ratio >= 1 for updates, a difference >= 0 for final passes", margin_ratio, margin_diff);
  Prof p{e, (hipStream_t)stream};
  p.mark(S_SAMPLER);
  HIP_TRY(e, launch_ddpm_step_rows(x_inout, logits, ld_logits, e->cfg.vocab_out, params, seed, B, L, margin_ratio, margin_diff,
                                   sample_flags, sample_min_gap, (hipStream_t)stream));
  p.mark(S_SAMPLER);
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
  if (e->cfg.vocab_out <= ESMDIFF_MASK_ID) return fail(e, ESMDIFF_E_INVALID, "the nelbo needs the 4101-way head (mask column)");
  if (int r = check_bl(e, B, L)) return r;      // (row_loss lives in the engine's workspace)
  if (int r = check_lens(e, B, L)) return r;
  Prof p{e, st};
  p.mark(S_SAMPLER);
  HIP_TRY(e, launch_nelbo_rows(logits, ld_logits, e->cfg.vocab_out, xt, x0, weight, loss_mask, e->cur_lens, log_p_out, e->n_rowloss,
                               sample_sum, sample_count, B, L, st));
  p.mark(S_SAMPLER);
  return 0;
}

int esmdiff_q_xt(esmdiff_engine* e, const int64_t* x0, const int64_t* seq, const float* move_chance, const uint8_t* non_moving,
                 const float* u, uint64_t seed, const uint64_t* sample_index, const int32_t* draw, int64_t* xt_out,
                 int64_t* seq_out, int32_t B, int32_t L, void* stream) {
  if (!e) return ESMDIFF_E_INVALID;
  if (e->kind != 0) return fail(e, ESMDIFF_E_INVALID, "this engine is a structure-token decoder (esmdiff_decoder_create)");
  return q_xt_checked(e, x0, seq, move_chance, non_moving, u, seed, sample_index, draw, xt_out, seq_out, B, L, (hipStream_t)stream);
}

int esmdiff_nelbo_rows(esmdiff_engine* e, const float* logits, int32_t ld_logits, const int64_t* xt, const int64_t* x0,
                       const float* weight, const uint8_t* loss_mask, float* log_p_out, float* sample_sum, int32_t* sample_count,
                       int32_t B, int32_t L, void* stream) {
  if (!e) return ESMDIFF_E_INVALID;
  if (e->kind != 0) return fail(e, ESMDIFF_E_INVALID, "this engine is a structure-token decoder (esmdiff_decoder_create)");
  return nelbo_rows_checked(e, logits, ld_logits, xt, x0, weight, loss_mask, log_p_out, sample_sum, sample_count, B, L,
                            (hipStream_t)stream);
}

int esmdiff_nelbo_eval(esmdiff_engine* e, const int64_t* seq, const int64_t* x0, const float* t_freq, const float* move_chance,
                       const float* weight, const uint8_t* non_moving, const float* u, uint64_t seed, const uint64_t* sample_index,
                       const int32_t* draw, const uint8_t* loss_mask, int32_t coupled, float* sample_sum, int32_t* sample_count,
                       float* log_p_out, int32_t B, int32_t L, void* stream) {
  if (!e) return ESMDIFF_E_INVALID;
  if (e->kind != 0) return fail(e, ESMDIFF_E_INVALID, "this engine is a structure-token decoder (esmdiff_decoder_create)");
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
  if (e && e->kind != 0) return fail(e, ESMDIFF_E_INVALID, "this engine is a structure-token decoder (esmdiff_decoder_create)");
  if (!e) return ESMDIFF_E_INVALID;
  if (!seq || !x_inout || !mc_t || !mc_s || !rng) return fail(e, ESMDIFF_E_INVALID, "null pointer");
  if (T <= 0 || T + 1 > e->tfreq_rows) return fail(e, ESMDIFF_E_INVALID, "num_steps %d out of range (1..%d)", T, e->tfreq_rows - 1);
  if (e->cfg.time_conditioning && !t_freq) return fail(e, ESMDIFF_E_INVALID, "t_freq required with time conditioning");
  if (int r = check_bl(e, B, L)) return r;
  if (int r = check_lens(e, B, L)) return r;
  hipStream_t st = (hipStream_t)stream;
  const int F = e->cfg.freq_dim;
  if (t_freq) HIP_TRY(e, hipMemcpyAsync(e->tfreq, t_freq, (size_t)(T + 1) * F * sizeof(float), hipMemcpyHostToDevice, st));
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
        const int rf = forward(e, e->cseq, e->cx, t_freq ? e->tfreq + (size_t)i * F : nullptr, e->logits, e->ld_logits, n_run, L, st);
        e->cur_lens = e->lens_B ? e->lens_dev : nullptr;
        if (rf) return rf;
        p.mark(S_SAMPLER);
        HIP_TRY(e, launch_ddpm_step(e->cx, e->logits, e->ld_logits, e->cfg.vocab_out, 0.f, 0.f, 1, nullptr, 1, rng->seed, rng->sample_offset, i, n_run, L, st, 0));
        p.mark(S_SAMPLER);
        HIP_TRY(e, launch_move_token_rows(e->cx, x_inout, e->idx_dev, n_live, L, 0, st));   // only the live samples go back
        HIP_TRY(e, hipStreamSynchronize(st));                    // idx (host vector) must outlive the H2D copy
        break;
      }
    }
    if (int r = forward(e, seq, x_inout, t_freq ? e->tfreq + (size_t)i * F : nullptr, e->logits, e->ld_logits, Bf, L, st)) return r;
    const int fin = i == T;
    p.mark(S_SAMPLER);
    HIP_TRY(e, launch_ddpm_step(x_inout, e->logits, e->ld_logits, e->cfg.vocab_out, fin ? 0.f : mc_t[i], fin ? 0.f : mc_s[i],
                                fin, nullptr, 1, rng->seed, rng->sample_offset, i, B, L, st, Bf < B ? Bf : 0));
    p.mark(S_SAMPLER);
  }
  return 0;
}

int esmdiff_gibbs_step(esmdiff_engine* e, int64_t* x_inout, const int64_t* seq, const float* logits, int32_t ld_logits,
                       float temperature, float top_p, const int32_t* n_unmask, const float* u, const esmdiff_rng* rng,
                       int32_t step, int32_t B, int32_t L, void* stream) {
  if (!e) return ESMDIFF_E_INVALID;
  if (!x_inout || !seq || !logits || !n_unmask) return fail(e, ESMDIFF_E_INVALID, "null pointer");
  if (!u && !rng) return fail(e, ESMDIFF_E_INVALID, "need explicit uniforms or an rng");
  if (!(temperature >= 0.f)) return fail(e, ESMDIFF_E_INVALID, "temperature must be >= 0 (0 = arg-max of the filtered logits)");
  if (!(top_p > 0.f) || top_p > 1.f) return fail(e, ESMDIFF_E_INVALID, "top_p must be in (0, 1]");
  if (ld_logits < 4096 || e->cfg.vocab_out < 4096 || ld_logits < e->cfg.vocab_out) return fail(e, ESMDIFF_E_INVALID, "bad shape");
  if (int r = check_bl(e, B, L)) return r;
  Prof p{e, (hipStream_t)stream};
  p.mark(S_SAMPLER);
  if (e->g_strategy == 1 && u) return fail(e, ESMDIFF_E_INVALID, "strategy \"random\" draws its positions from the Philox source: pass rng, not explicit uniforms");
  HIP_TRY(e, launch_gibbs_step(x_inout, seq, logits, ld_logits, e->cfg.vocab_out, temperature, top_p, n_unmask, u, u ? 0 : 1, rng ? rng->seed : 0,
                               rng ? rng->sample_offset : 0, step, e->g_sampled, e->g_entropy, B, L, (hipStream_t)stream, 0,
                               e->g_strategy, e->g_inv_on ? e->g_inv_mask : nullptr));
  p.mark(S_SAMPLER);
  return 0;
}

int esmdiff_gibbs_step_rows(esmdiff_engine* e, int64_t* x_inout, const int64_t* seq, const float* logits, int32_t ld_logits,
                            float temperature, float top_p, const esmdiff_gibbs_sample_step* params, uint64_t seed, int32_t B,
                            int32_t L, float pair_bound, float entropy_bound, int32_t* sample_flags, float* sample_gaps,
                            void* stream) {
  if (!e) return ESMDIFF_E_INVALID;
  if (!x_inout || !seq || !logits || !params) return fail(e, ESMDIFF_E_INVALID, "null pointer");
  if (!(temperature >= 0.f)) return fail(e, ESMDIFF_E_INVALID, "temperature must be >= 0 (0 = arg-max of the filtered logits)");
  if (!(top_p > 0.f) || top_p > 1.f) return fail(e, ESMDIFF_E_INVALID, "top_p must be in (0, 1]");
  if (ld_logits < 4096 || e->cfg.vocab_out < 4096 || ld_logits < e->cfg.vocab_out) return fail(e, ESMDIFF_E_INVALID, "bad shape");
  if (int r = check_bl(e, B, L)) return r;
  if (int r = check_lens(e, B, L)) return r;   // (padding holds no MASK: the step leaves it as it is)
  if (pair_bound < 0.f && (sample_flags || sample_gaps))
    return fail(e, ESMDIFF_E_INVALID, "sample_flags / sample_gaps need pair_bound >= 0 (and entropy_bound >= 0)");
  if (pair_bound >= 0.f && !(entropy_bound >= 0.f)) return fail(e, ESMDIFF_E_INVALID, "entropy_bound must be >= 0");
  Prof p{e, (hipStream_t)stream};
  p.mark(S_SAMPLER);
  HIP_TRY(e, launch_gibbs_step_rows(x_inout, seq, logits, ld_logits, e->cfg.vocab_out, temperature, top_p, params, seed, e->g_sampled,
                                    e->g_entropy, B, L, pair_bound, entropy_bound, e->g_rowflag, e->g_rowgap, sample_flags, sample_gaps,
                                    (hipStream_t)stream, e->g_strategy, e->g_inv_on ? e->g_inv_mask : nullptr));
  p.mark(S_SAMPLER);
  return 0;
}

int esmdiff_gibbs_sample(esmdiff_engine* e, const int64_t* seq, int64_t* x_inout, int32_t B, int32_t L, int32_t T,
                         float temperature, float top_p, const int32_t* n_unmask_table, const esmdiff_rng* rng,
                         void* stream) {
  if (e && e->kind != 0) return fail(e, ESMDIFF_E_INVALID, "this engine is a structure-token decoder (esmdiff_decoder_create)");
  if (!e) return ESMDIFF_E_INVALID;
  if (!seq || !x_inout || !n_unmask_table || !rng) return fail(e, ESMDIFF_E_INVALID, "null pointer");
  if (T <= 0 || T > e->tfreq_rows) return fail(e, ESMDIFF_E_INVALID, "num_steps %d out of range (1..%d)", T, e->tfreq_rows);
  if (int r = check_bl(e, B, L)) return r;
  if (int r = check_lens(e, B, L)) return r;
  hipStream_t st = (hipStream_t)stream;
  if (!(temperature >= 0.f)) return fail(e, ESMDIFF_E_INVALID, "temperature must be >= 0 (0 = arg-max of the filtered logits)");
  if (!(top_p > 0.f) || top_p > 1.f) return fail(e, ESMDIFF_E_INVALID, "top_p must be in (0, 1]");
  HIP_TRY(e, hipMemcpyAsync(e->g_nunmask, n_unmask_table, (size_t)T * B * sizeof(int32_t), hipMemcpyHostToDevice, st));
  int shared = 0;
  if (int r = step0_shared_batch(e, seq, x_inout, B, L, st, &shared)) return r;   // (0 with coordinate conditioning)
  for (int i = 0; i < T; ++i) {
    const int Bf = (i == 0 && shared) ? shared : B;
    if (int r = forward(e, seq, x_inout, nullptr, e->logits, e->ld_logits, Bf, L, st)) return r;
    Prof p{e, st};
    p.mark(S_SAMPLER);
    HIP_TRY(e, launch_gibbs_step(x_inout, seq, e->logits, e->ld_logits, e->cfg.vocab_out, temperature, top_p,
                                 e->g_nunmask + (size_t)i * B, nullptr, 1, rng->seed, rng->sample_offset, i, e->g_sampled,
                                 e->g_entropy, B, L, st, Bf < B ? Bf : 0, e->g_strategy, e->g_inv_on ? e->g_inv_mask : nullptr));
    p.mark(S_SAMPLER);
  }
  return 0;
}

int esmdiff_gemm_bf16(const void* A, const void* W, void* out, const float* bias, int32_t M, int32_t N, int32_t K,
                      int32_t ldc, int32_t n_valid, float alpha, int32_t epilogue, void* stream) {
  if (!A || !W || !out) return ESMDIFF_E_INVALID;
  hipError_t s = launch_gemm_bf16((const bf16_t*)A, (const bf16_t*)W, out, bias, M, N, K, ldc, n_valid, alpha, epilogue,
                                  (hipStream_t)stream);
  if (s != hipSuccess) return fail(nullptr, s == hipErrorInvalidValue ? ESMDIFF_E_INVALID : ESMDIFF_E_HIP, "gemm: %s", hipGetErrorString(s));
  return 0;
}

int esmdiff_gemm_f16(const void* A, const void* W, void* out, const float* bias, int32_t M, int32_t N, int32_t K,
                     int32_t ldc, int32_t n_valid, float alpha, int32_t epilogue, void* stream) {
  if (!A || !W || !out) return ESMDIFF_E_INVALID;
  hipError_t s = ed16::launch_gemm_bf16((const bf16_t*)A, (const bf16_t*)W, out, bias, M, N, K, ldc, n_valid, alpha, epilogue,
                                        (hipStream_t)stream);
  if (s != hipSuccess) return fail(nullptr, s == hipErrorInvalidValue ? ESMDIFF_E_INVALID : ESMDIFF_E_HIP, "gemm_f16: %s", hipGetErrorString(s));
  return 0;
}

int esmdiff_gemm_f32(const float* A, int32_t lda, const float* W, float* out, const float* bias, int32_t M, int32_t N,
                     int32_t K, int32_t ldc, int32_t n_valid, float div, int32_t epilogue, void* stream) {
  if (!A || !W || !out) return ESMDIFF_E_INVALID;
  hipError_t s = launch_gemm_f32(A, lda, W, out, bias, M, N, K, ldc, n_valid, div, epilogue, (hipStream_t)stream);
  if (s != hipSuccess) return fail(nullptr, s == hipErrorInvalidValue ? ESMDIFF_E_INVALID : ESMDIFF_E_HIP, "gemm_f32: %s", hipGetErrorString(s));
  return 0;
}

int esmdiff_split_rows(const float* src, int32_t ld, void* a2, float* rs, int32_t M, int32_t K, void* stream) {
  if (!src || !a2 || !rs) return ESMDIFF_E_INVALID;
  hipError_t s = launch_split_rows(src, ld, (uint16_t*)a2, rs, M, K, (hipStream_t)stream);
  if (s != hipSuccess) return fail(nullptr, s == hipErrorInvalidValue ? ESMDIFF_E_INVALID : ESMDIFF_E_HIP, "split_rows: %s", hipGetErrorString(s));
  return 0;
}

int esmdiff_split_weight(const float* src, void* w2, int32_t N, int32_t N_pad, int32_t K, float* inv_scale_out) {
  if (!src || !w2 || !inv_scale_out || N <= 0 || N_pad < N || N_pad % 256 || K <= 0 || K % 128) return ESMDIFF_E_INVALID;
  uint32_t* bits = nullptr;
  if (hipMalloc(&bits, 4) != hipSuccess) return fail(nullptr, ESMDIFF_E_HIP, "split_weight: hipMalloc failed");
  hipError_t s = hipSuccess;
  if (N_pad > N) s = hipMemset((uint16_t*)w2 + (size_t)N * 3 * K, 0, (size_t)(N_pad - N) * 3 * K * 2);
  if (s == hipSuccess) s = split_weight(src, ESMDIFF_F32, (uint16_t*)w2, N, K, bits, inv_scale_out);
  if (s == hipSuccess) s = hipDeviceSynchronize();
  hipFree(bits);
  if (s != hipSuccess) return fail(nullptr, ESMDIFF_E_HIP, "split_weight: %s", hipGetErrorString(s));
  return 0;
}

int esmdiff_gemm_split(const void* a2, const float* rs, const void* w2, float w_inv_scale, float* out, const float* bias,
                       int32_t M, int32_t N, int32_t K, int32_t ldc, float div, int32_t epilogue, void* stream) {
  if (!a2 || !w2 || !out) return ESMDIFF_E_INVALID;
  hipError_t s = launch_gemm256w4_split((const uint16_t*)a2, rs, (const uint16_t*)w2, w_inv_scale, out, bias, M, N, K, ldc, div,
                                        epilogue, (hipStream_t)stream);
  if (s != hipSuccess) return fail(nullptr, s == hipErrorInvalidValue ? ESMDIFF_E_INVALID : ESMDIFF_E_HIP, "gemm_split: %s", hipGetErrorString(s));
  return 0;
}

int esmdiff_gemm_bf16_ws(esmdiff_engine* e, const void* A, const void* W, void* out, const float* bias, int32_t M,
                         int32_t N, int32_t K, int32_t ldc, int32_t n_valid, float alpha, int32_t epilogue, void* stream) {
  if (!e || !A || !W || !out) return ESMDIFF_E_INVALID;
  hipError_t s = launch_gemm_bf16((const bf16_t*)A, (const bf16_t*)W, out, bias, M, N, K, ldc, n_valid, alpha, epilogue,
                                  (hipStream_t)stream, e->gemm_ws[0].partial ? &e->gemm_ws[0] : nullptr);
  if (s != hipSuccess) return fail(e, s == hipErrorInvalidValue ? ESMDIFF_E_INVALID : ESMDIFF_E_HIP, "gemm: %s", hipGetErrorString(s));
  return 0;
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
  if (s != hipSuccess) return fail(e, s == hipErrorInvalidValue ? ESMDIFF_E_INVALID : ESMDIFF_E_HIP, "branch linear + layernorm: %s", hipGetErrorString(s));
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
  } else if (e->f16) {
    HIP_TRY(e, ed16::launch_qk_norm_rope((const bf16_t*)qkv, q_ln_w, k_ln_w, e->rope_cos, e->rope_sin, e->q, e->k, B, L, H, st));
    HIP_TRY(e, ed16::launch_attention(e->q, e->k, (const bf16_t*)qkv, (bf16_t*)ctx, B, L, H, st, dl));
  } else {
    HIP_TRY(e, launch_qk_norm_rope((const bf16_t*)qkv, q_ln_w, k_ln_w, e->rope_cos, e->rope_sin, e->q, e->k, B, L, H, st));
    HIP_TRY(e, launch_attention(e->q, e->k, (const bf16_t*)qkv, (bf16_t*)ctx, B, L, H, st, dl));
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
  HIP_TRY(e, e->f16 ? ed16::launch_qk_norm_rope((const bf16_t*)qkv, q_ln_w, k_ln_w, e->rope_cos, e->rope_sin, (bf16_t*)q,
                                                (bf16_t*)k, B, L, H, (hipStream_t)stream)
                    : ed::launch_qk_norm_rope((const bf16_t*)qkv, q_ln_w, k_ln_w, e->rope_cos, e->rope_sin, (bf16_t*)q,
                                              (bf16_t*)k, B, L, H, (hipStream_t)stream));
  return 0;
}

int esmdiff_add_layernorm(int32_t dtype, float* x, const void* delta, const void* delta2, int32_t write_x, const float* w,
                          const float* b, void* y, int32_t M, int32_t D, void* stream) {
  if (!x || !w || !y) return fail(nullptr, ESMDIFF_E_INVALID, "add_layernorm: null pointer");
  if (dtype != 0 && dtype != 1) return fail(nullptr, ESMDIFF_E_INVALID, "add_layernorm: dtype %d (0 bf16, 1 f16)", dtype);
  if (M <= 0 || D <= 0) return fail(nullptr, ESMDIFF_E_INVALID, "add_layernorm: M=%d D=%d must be positive", M, D);
  const hipError_t s = dtype ? ed16::launch_add_layernorm_bf16(x, (const bf16_t*)delta, (const bf16_t*)delta2, write_x, w, b,
                                                               (bf16_t*)y, M, D, (hipStream_t)stream)
                             : ed::launch_add_layernorm_bf16(x, (const bf16_t*)delta, (const bf16_t*)delta2, write_x, w, b,
                                                             (bf16_t*)y, M, D, (hipStream_t)stream);
  if (s != hipSuccess) return fail(nullptr, s == hipErrorInvalidValue ? ESMDIFF_E_INVALID : ESMDIFF_E_HIP, "add_layernorm: %s", hipGetErrorString(s));
  return 0;
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
    else if (dtype == 1)
      s = ed16::launch_geom_attention((const bf16_t*)P, rot, trans, has_frame, dw, dw + VH, (bf16_t*)out, B, L, VH, st);
    else
      s = ed::launch_geom_attention((const bf16_t*)P, rot, trans, has_frame, dw, dw + VH, (bf16_t*)out, B, L, VH, st);
  }
  const hipError_t s2 = hipStreamSynchronize(st);   // synchronous: the scale buffer and the host copy die here
  if (s == hipSuccess) s = s2;
  hipFree(dw);
  if (s != hipSuccess) return fail(nullptr, s == hipErrorInvalidValue ? ESMDIFF_E_INVALID : ESMDIFF_E_HIP, "geom_attention: %s", hipGetErrorString(s));
  return 0;
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

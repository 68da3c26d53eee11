// engine.h — private to the engine units of libesmdiff_hip.so (never installed): the engine's data model, the section timer and
// the few helpers that cross units.
//   engine.hip          lifetime and state: create / destroy, the setters and getters, the error channel
//   engine_weights.hip  the weight loader of every create: Table, need, load_f32, load_linear (encoder.hip loads through it too)
//   engine_forward.hip  one forward: batch planner, sub-batch view, the float32-grade and the 16-bit launch sequences
//   engine_sample.hip   what runs forwards in a loop or consumes logits: ddpm / gibbs steps and samplers, q_xt, the NELBO
//   engine_decode.hip   the structure decoder's backbone and confidence heads
//   engine_test.hip     kernel-level entries of include/esmdiff_hip_test.h
//   encoder.hip         (a kernel unit) includes this header for its host side: esmdiff_encoder is an Owner with Linear slots
// Everything here that is not a C entry lives in namespace eng; a unit's own helpers stay static / anonymous in that unit.
#pragma once
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
#define ed ed16            // the f16 build of the operand-typed units (ed_half.h, esmdiff_amd/build.py: F16_UNITS): only what
#include "kernels_typed.inc"   // they define is declared in ed16, so a once-only launcher spelled ed16:: does not compile
#undef ed

// The operand-type build of a launcher, chosen by the engine's 16-bit type: ED_KN(e->f16, launch_x(args)) calls ed16::launch_x
// on an f16 engine and ed::launch_x otherwise, with the arguments written once.
#define ED_KN(f16, call) ((f16) ? ed16::call : ed::call)

namespace eng {

enum Section { S_EMBED = 0, S_LN, S_QKV, S_QKROPE, S_ATTN, S_OUT, S_FFN_UP, S_FFN_DOWN, S_HEAD, S_SAMPLER, S_COUNT };

// engine_decode.hip (pairwise_confidence): bytes of pair rows one chunk of whole samples may occupy
constexpr int64_t kDefaultPairChunkBytes = 1536ll << 20;

// What the error channel, dalloc and the weight loader need of their owner: esmdiff_engine and esmdiff_encoder (encoder.hip)
// both start with it.  allocs: what destroy frees.
struct Owner {
  int device = 0;
  std::string err;
  std::vector<void*> allocs;
};

// One linear's weight, held in the one form its owner runs it in.  create_engine chooses the form per group of weights
// (body_form / head_form / plain_form), the encoder one form for all; load_linear fills the slot, and the launch sequences
// dispatch on `form`.  An accessor of another form than the slot's gives null.
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

}  // namespace eng

struct esmdiff_engine : eng::Owner {
  esmdiff_config cfg{};
  int kind = 0;  // 0: ESM3 structure-token transformer (the sampler's network); 1: VQ-VAE structure-token decoder
  // weights
  std::vector<eng::Layer> layers;
  float *e_seq = nullptr, *e_struct = nullptr, *cvec = nullptr;
  float *final_ln_w = nullptr;
  eng::Linear head_w0, head_w3;   // head_w3: rows padded to vocab_pad except as F32
  float *head_b0 = nullptr, *head_ln_w = nullptr, *head_ln_b = nullptr, *head_b3 = nullptr;
  float *sig_w1 = nullptr, *sig_b1 = nullptr, *sig_w2 = nullptr, *sig_b2 = nullptr;
  float *rope_cos = nullptr, *rope_sin = nullptr;
  int vocab_pad = 0;
  // decoder only (kind 1): esm's plddt_head = RegressionHead(d, 50) on the same final hidden state (optional weights)
  bool has_plddt = false;
  int plddt_bins = 0, ld_plddt = 0;
  eng::Linear pl_w0, pl_w3;
  // decoder only: esm's pairwise_classification_head (PairwisePredictionHead(d, 128, 128, 224 bins, no bias)); only the
  // 64 predicted-aligned-error bins (rows 160..223 of linear2) are evaluated: pTM and the PAE matrix (csrc/pairwise.hip)
  bool has_pair = false;
  eng::Linear pw_down, pw_l1, pw_l2;   // W16 or F32, never SPLIT
  bf16_t* pair_qk = nullptr;
  float *pw_ln_w = nullptr, *pw_ln_b = nullptr, *zeros128 = nullptr, *tm_rows = nullptr, *ptm_dev = nullptr;
  bf16_t *pair_x = nullptr, *pair_h = nullptr;   // pair rows of a chunk of samples (allocated on first use)
  float* pair_logits = nullptr;
  int64_t pair_rows_cap = 0;
  int64_t pair_chunk_bytes = eng::kDefaultPairChunkBytes;   // esmdiff_decoder_set_pair_chunk_bytes (tests of the chunk loop)
  float *pl_b0 = nullptr, *pl_ln_w = nullptr, *pl_ln_b = nullptr, *pl_b3 = nullptr, *pl_logits = nullptr;
  // block 0 geometric attention (optional weights; live only while frames are set)
  bool has_geom = false;
  int v_heads = 0;  // rows of geom_attn.proj.weight / 15
  float *g_snorm_w = nullptr, *g_wrot = nullptr, *g_wdist = nullptr;
  eng::Linear g_proj, g_out;   // SPLIT only as a pair: when both shapes fit the split GEMM
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
  // [host] arrays of esmdiff_ddpm_sample (t_freq) and esmdiff_gibbs_sample (n_unmask_table) are copied here before their upload, so that
  // the caller's array is consumed before the entry returns wherever it lives (an upload from PINNED memory would read it later).
  // The upload from this pageable copy is staged by the runtime before hipMemcpyAsync returns: MEASURED, not promised by HIP, at
  // 108 bytes, 4 KB and 1 MB (T = 1025), where the entry also came back without waiting (tests/test_gpu_stream_order.py).  A
  // runtime that read the copy later would see the next call's assign() rewrite it; esmdiff_ddpm_sample's final-skip branch, which
  // uploads from a local vector, does not rely on the staging and waits for the stream instead.
  std::vector<float> tfreq_host;
  std::vector<int32_t> nunmask_host;
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
  // precision = ESMDIFF_PRECISION_F32: float32 weights / activations (engine_forward.hip: strict_part); the 16-bit workspace above stays null
  bool strict = false;
  // precision = ESMDIFF_PRECISION_F32_SPLIT: strict_part with every large linear as three f16 MFMA passes over split
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
  // needed rows (esmdiff_set_option(ESMDIFF_OPT_NEEDED_ROWS); engine_forward.hip: needed_tail): a forward of esmdiff_ddpm_sample runs
  // the last block's branches and the head on the rows that hold MASK.  rows_list / rows_map: launch_mask_row_list's outputs,
  // rows_count: its counts per sub-batch in pinned host memory, ev_rows: recorded behind it.  rows_mapped: the last forward left
  // compact logits (the sampler reads them through rows_map) and x / logits of the other rows stale.
  int needed_rows = 1;
  int32_t *rows_list = nullptr, *rows_map = nullptr, *rows_count = nullptr;
  hipEvent_t ev_rows = nullptr;
  bool rows_mapped = false;
  int64_t stat_tail_rows = 0;   // rows that ran the last block's branches and the head (esmdiff_get_tail_rows)
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

namespace eng {

// ---- helpers that cross units -------------------------------------------------------------------------------------------
// engine.hip: the message goes to the owner, or with o == null to the calling thread's handle-less string (a failed create, a
// kernel-level test entry); returns `code`.  last_error reads it back: esmdiff_last_error and esmdiff_encoder_last_error.
int fail(Owner* o, int code, const char* fmt, ...);
const char* last_error(const Owner* o);
int round_up(int v, int m);
void softplus_host(float* v, int n);
int check_bl(esmdiff_engine* e, int B, int L);
int check_lens(esmdiff_engine* e, int B, int L);
int check_not_decoder(esmdiff_engine* e);
// engine_forward.hip
// needed_rows: the caller reads logits on the rows with xtok == MASK only (through e->rows_map while e->rows_mapped)
int forward(esmdiff_engine* e, const int64_t* seq, const int64_t* xtok, const float* t_freq_dev, float* logits, int ld, int B, int L,
            hipStream_t st, bool needed_rows = false);
int shared_forward_batch(const esmdiff_engine* e, int B, int L);

#define HIP_TRY(e, call)                                                                              \
  do {                                                                                                \
    hipError_t _s = (call);                                                                           \
    if (_s != hipSuccess) return eng::fail(e, ESMDIFF_E_HIP, "%s: %s", #call, hipGetErrorString(_s)); \
  } while (0)

// ---- engine_weights.hip: the one weight loader (dalloc, a template, is defined here) ------------------------------------------
template <typename T>
int dalloc(Owner* o, T** p, size_t n_elems, bool zero = false) {
  void* v = nullptr;
  hipError_t s = hipMalloc(&v, n_elems * sizeof(T) + 256);
  if (s != hipSuccess) return fail(o, ESMDIFF_E_HIP, "hipMalloc(%zu): %s", n_elems * sizeof(T), hipGetErrorString(s));
  if (zero) hipMemset(v, 0, n_elems * sizeof(T) + 256);
  o->allocs.push_back(v);
  *p = reinterpret_cast<T*>(v);
  return 0;
}

// The caller's weight table by name; of two entries with one name the last wins.  A name that is not found as it stands is
// looked up once more behind `prefix` (the engine's "net."); without a prefix the lookup is exact.
struct Table {
  std::map<std::string, const esmdiff_weight*> m;
  std::string prefix;
  Table(const esmdiff_weight* table, int n, const char* prefix = "");
  const esmdiff_weight* find(const std::string& name) const;
};
int64_t numel(const esmdiff_weight* w);
// the named tensor, checked: present, of this shape, f32 or bf16, with data
int need(Owner* o, const Table& t, const std::string& name, std::initializer_list<int64_t> shape, const esmdiff_weight** out);
// vectors and embeddings: float32, the tail up to pad_to elements zero
int load_f32(Owner* o, const Table& t, const std::string& name, std::initializer_list<int64_t> shape, float** dst, int64_t pad_to = 0);
// A linear's weight [rows, K] into its slot in the given form.  W16 and SPLIT zero-pad the rows to pad_rows and, with
// swiglu_h = FH, interleave the FFN-up's gate / up rows for the SwiGLU epilogue; F32 does neither (launch_gemm_f32 bounds
// its rows and the SwiGLU is its own pass).  SPLIT: planes [rows_p, 3 K] + the inverse scale.  f16: the owner's 16-bit
// operand type (W16 only); scratch_bits: the device word the SPLIT form's scale reduction needs.
int load_linear(Owner* o, const Table& t, const std::string& name, std::initializer_list<int64_t> shape, Linear::Form form,
                Linear* dst, int64_t pad_rows = 0, int swiglu_h = 0, bool f16 = false, uint32_t* scratch_bits = nullptr);

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

// the planner's constants (engine_forward.hip: plan_batch; esmdiff_set_small_batch_splitk sizes its planes by the last)
constexpr int kDefaultStreams = 2;
constexpr int64_t kDefaultDualMinTokens = 2200;
constexpr int64_t kDualSmallMaxTokens = 1024;      // the all-small two-queue window reaches up to this many tokens, see forward()
constexpr int64_t kStrictDualMinTokens = 8192;     // F32_SPLIT: two sub-batch streams from this many tokens
constexpr int kSplitkMaxRows = 4096;               // esmdiff_set_small_batch_splitk: K-sliced residual linears up to this many rows

}  // namespace eng

// encoder.hip — VQ-VAE structure-token ENCODER: backbone frames -> structure tokens (gfx950).
//
// Reference call sites: /root/reference/slm/models/utils.py:136-137 (`model.encode(ESMProtein(coordinates=...))` in
// protseq_to_data), reached from /root/reference/slm/sample_esmdiff.py:196-201 to build the DDPM inpainting prior
// (BASELINE configs[4]).  The module is esm==3.0.4's StructureTokenEncoder (un-vendored): restated from memory
// [ESM-RECALL, SURVEY.md 8f-4], PARITY UNPINNED; checked against oracle/encoder_ref.py.
//
//   per residue i: the K = 16 residues nearest to it (CA distance; sequence distance x 100 + 1e6 where coordinates
//   are missing), nearest first, i itself leading -> x[e] = relpos_embedding[clamp(j_e - i, +-32) + 33] ->
//   2 x [ x += geom_attn(x; frames of the 16 residues) ; x += swiglu_ffn(x) ] (both with biases) over that
//   neighbourhood -> row e = 0 -> 0 if i has no frame -> Linear(d, 128) -> nearest codebook vector (4096 x 128);
//   residues without coordinates get MASK (4096).
// The neighbourhoods are independent sequences of length 16: M = B*L*16 rows go through the shared GEMM / LayerNorm /
// geometric-attention kernels; the small glue kernels live here.  Encoding happens once per input structure, so this
// file aims at correctness and reuse, not at the roofline.
// Host side: an esmdiff_encoder is an eng::Owner like an engine (engine.h).  Its weights come in through the engine's loader
// (engine_weights.hip: exact names, one eng::Linear slot per linear in the precision's form), its errors go through eng::fail /
// HIP_TRY, and every glue kernel has one host launcher that encode and the test entries share.
#include "engine.h"

namespace ed {
namespace {

typedef __attribute__((ext_vector_type(4))) float f32x4e;

__device__ __forceinline__ float bf2f_(bf16_t v) { return __uint_as_float((uint32_t)v << 16); }
__device__ __forceinline__ bf16_t f2bf_(float f) {
  uint32_t u = __float_as_uint(f);
  return (bf16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

// one workgroup per (b, i): K selections of the smallest key, lowest index first among equals
__global__ __launch_bounds__(256) void knn_kernel(const float* __restrict__ ca, const uint8_t* __restrict__ has, int L, int K,
                                                  int32_t* __restrict__ edges) {
  extern __shared__ float key[];  // [L] + reduction scratch
  __shared__ float rv[256];
  __shared__ int ri[256];
  const int b = blockIdx.y, i = blockIdx.x, tid = threadIdx.x;
  const float* c = ca + (int64_t)b * L * 3;
  const uint8_t* h = has + (int64_t)b * L;
  const bool hi_ = h[i] != 0;
  const float xi = hi_ ? c[i * 3] : 0.f, yi = hi_ ? c[i * 3 + 1] : 0.f, zi = hi_ ? c[i * 3 + 2] : 0.f;
  for (int j = tid; j < L; j += 256) {
    float v;
    if (hi_ && h[j]) {
      const float dx = xi - c[j * 3], dy = yi - c[j * 3 + 1], dz = zi - c[j * 3 + 2];
      v = sqrtf(dx * dx + dy * dy + dz * dz);
    } else {
      v = fabsf((float)(i - j)) * 1e2f + 1e6f;
    }
    key[j] = v;
  }
  __syncthreads();
  for (int e = 0; e < K; ++e) {
    float bv = INFINITY;
    int bi = 0x7fffffff;
    for (int j = tid; j < L; j += 256)
      if (key[j] < bv) {  // strided ascending: the first hit of a thread is its lowest index
        bv = key[j];
        bi = j;
      }
    rv[tid] = bv;
    ri[tid] = bi;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
      if (tid < s) {
        const float ov = rv[tid + s];
        const int oi = ri[tid + s];
        if (ov < rv[tid] || (ov == rv[tid] && oi < ri[tid])) {
          rv[tid] = ov;
          ri[tid] = oi;
        }
      }
      __syncthreads();
    }
    if (tid == 0) {
      edges[((int64_t)b * L + i) * K + e] = ri[0];
      key[ri[0]] = INFINITY;
    }
    __syncthreads();
  }
}

// x[m] = table[clamp(edge - edge_0, +-bins) + bins + 1]; frames of the neighbours gathered alongside
__global__ __launch_bounds__(256) void neighbourhood_kernel(const int32_t* __restrict__ edges, const float* __restrict__ table,
                                                            const float* __restrict__ rot, const float* __restrict__ trans,
                                                            const uint8_t* __restrict__ has, int L, int K, int D, int bins,
                                                            float* __restrict__ x, float* __restrict__ nrot,
                                                            float* __restrict__ ntrans, uint8_t* __restrict__ nmask) {
  const int64_t m = blockIdx.x;  // (b*L + i)*K + e
  const int64_t bi = m / K;
  const int b = (int)(bi / L);
  const int j = edges[m], j0 = edges[bi * K];
  int diff = j - j0;
  diff = diff < -bins ? -bins : (diff > bins ? bins : diff);
  const float* src = table + (int64_t)(diff + bins + 1) * D;
  float* o = x + m * D;
  for (int c = threadIdx.x * 4; c < D; c += 1024) *reinterpret_cast<f32x4e*>(o + c) = *reinterpret_cast<const f32x4e*>(src + c);
  const int64_t r = (int64_t)b * L + j;
  if (threadIdx.x < 9) nrot[m * 9 + threadIdx.x] = rot[r * 9 + threadIdx.x];
  if (threadIdx.x < 3) ntrans[m * 3 + threadIdx.x] = trans[r * 3 + threadIdx.x];
  if (threadIdx.x == 0) nmask[m] = has[r];
}

__global__ __launch_bounds__(256) void add_bias_bf16_kernel(bf16_t* __restrict__ x, const float* __restrict__ bias, int64_t n, int N) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  x[i] = f2bf_(bf2f_(x[i]) + bias[i % N]);
}

// u bf16 [M, 2H] = [gate | up] (bias added here) -> mid bf16 [M, H] = silu(gate) * up
__global__ __launch_bounds__(256) void bias_swiglu_kernel(const bf16_t* __restrict__ u, const float* __restrict__ bias, int64_t M,
                                                          int H, bf16_t* __restrict__ mid) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * H) return;
  const int64_t m = i / H;
  const int c = (int)(i - m * H);
  const float g = bf2f_(u[m * 2 * H + c]) + bias[c], v = bf2f_(u[m * 2 * H + H + c]) + bias[H + c];
  mid[i] = f2bf_(g / (1.0f + expf(-g)) * v);
}

// z[r] = has[r] ? x[r*K] + delta[r*K] : 0  (the query residue's row of its neighbourhood), as the bf16 operand of pre_vq_proj
__global__ __launch_bounds__(256) void query_rows_kernel(const float* __restrict__ x, const bf16_t* __restrict__ delta,
                                                         const uint8_t* __restrict__ has, int K, int D, bf16_t* __restrict__ z) {
  const int64_t r = blockIdx.x;
  const int64_t m = r * K;
  const bool keep = has[r] != 0;
  for (int c = threadIdx.x; c < D; c += 256) z[r * D + c] = keep ? f2bf_(x[m * D + c] + bf2f_(delta[m * D + c])) : (bf16_t)0;
}

// nearest codebook vector (squared Euclidean distance, lowest index among equals); MASK for residues without a frame
__global__ __launch_bounds__(256) void codebook_kernel(const float* __restrict__ z, const float* __restrict__ code,
                                                       const uint8_t* __restrict__ has, int n_codes, int d_out,
                                                       int64_t* __restrict__ tok) {
  extern __shared__ float zs[];
  __shared__ float rv[256];
  __shared__ int ri[256];
  const int64_t r = blockIdx.x;
  const int tid = threadIdx.x;
  for (int c = tid; c < d_out; c += 256) zs[c] = z[r * d_out + c];
  __syncthreads();
  float bv = INFINITY;
  int bi = 0x7fffffff;
  for (int k = tid; k < n_codes; k += 256) {
    const float* e = code + (int64_t)k * d_out;
    float s = 0.f;
    for (int c = 0; c < d_out; ++c) {
      const float d = zs[c] - e[c];
      s += d * d;
    }
    if (s < bv) {
      bv = s;
      bi = k;
    }
  }
  rv[tid] = bv;
  ri[tid] = bi;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if (tid < s) {
      if (rv[tid + s] < rv[tid] || (rv[tid + s] == rv[tid] && ri[tid + s] < ri[tid])) {
        rv[tid] = rv[tid + s];
        ri[tid] = ri[tid + s];
      }
    }
    __syncthreads();
  }
  if (tid == 0) tok[r] = has[r] ? ri[0] : ESMDIFF_MASK_ID;
}

// z[r] = has[r] ? x[r*K] : 0 in float32 (precision = F32: x already holds every residual)
__global__ __launch_bounds__(256) void query_rows_f32_kernel(const float* __restrict__ x, const uint8_t* __restrict__ has, int K,
                                                             int D, float* __restrict__ z) {
  const int64_t r = blockIdx.x;
  const bool keep = has[r] != 0;
  for (int c = threadIdx.x; c < D; c += 256) z[r * D + c] = keep ? x[r * K * D + c] : 0.f;
}

// ---- host launchers of the glue kernels: each owns its grid, block and LDS size and returns hipGetLastError().
// esmdiff_encoder_encode and the test entries at the end of this file launch through them and nowhere else. ----
hipError_t launch_knn(const float* ca, const uint8_t* has, int B, int L, int K, int32_t* edges, hipStream_t st) {
  hipLaunchKernelGGL(knn_kernel, dim3(L, B), dim3(256), (size_t)L * sizeof(float), st, ca, has, L, K, edges);
  return hipGetLastError();
}

hipError_t launch_neighbourhood(const int32_t* edges, const float* table, const float* rot, const float* trans, const uint8_t* has,
                                int64_t M, int L, int K, int D, int bins, float* x, float* nrot, float* ntrans, uint8_t* nmask,
                                hipStream_t st) {
  hipLaunchKernelGGL(neighbourhood_kernel, dim3((unsigned)M), dim3(256), 0, st, edges, table, rot, trans, has, L, K, D, bins, x, nrot,
                     ntrans, nmask);
  return hipGetLastError();
}

hipError_t launch_add_bias_bf16(bf16_t* x, const float* bias, int64_t M, int N, hipStream_t st) {
  hipLaunchKernelGGL(add_bias_bf16_kernel, dim3((unsigned)((M * N + 255) / 256)), dim3(256), 0, st, x, bias, M * N, N);
  return hipGetLastError();
}

hipError_t launch_bias_swiglu(const bf16_t* u, const float* bias, int64_t M, int H, bf16_t* mid, hipStream_t st) {
  hipLaunchKernelGGL(bias_swiglu_kernel, dim3((unsigned)((M * H + 255) / 256)), dim3(256), 0, st, u, bias, M, H, mid);
  return hipGetLastError();
}

hipError_t launch_query_rows(const float* x, const bf16_t* delta, const uint8_t* has, int64_t R, int K, int D, bf16_t* z,
                             hipStream_t st) {
  hipLaunchKernelGGL(query_rows_kernel, dim3((unsigned)R), dim3(256), 0, st, x, delta, has, K, D, z);
  return hipGetLastError();
}

hipError_t launch_query_rows_f32(const float* x, const uint8_t* has, int64_t R, int K, int D, float* z, hipStream_t st) {
  hipLaunchKernelGGL(query_rows_f32_kernel, dim3((unsigned)R), dim3(256), 0, st, x, has, K, D, z);
  return hipGetLastError();
}

hipError_t launch_codebook(const float* z, const float* code, const uint8_t* has, int64_t R, int n_codes, int d_out, int64_t* tok,
                           hipStream_t st) {
  hipLaunchKernelGGL(codebook_kernel, dim3((unsigned)R), dim3(256), (size_t)d_out * sizeof(float), st, z, code, has, n_codes, d_out, tok);
  return hipGetLastError();
}

struct Block {
  float *s_norm_w, *proj_b, *out_b, *w_rot, *w_dist, *ln_w, *ln_b, *b1, *b3;
  eng::Linear proj, out, up, down;   // W16 (bf16) or F32, as the encoder's precision; the FFN-up in the checkpoint's row order
};

struct Tmp {  // per-call device scratch
  std::vector<void*> p;
  ~Tmp() {
    for (void* q : p) hipFree(q);
  }
  template <typename T>
  T* get(size_t n) {
    void* v = nullptr;
    if (hipMalloc(&v, (n ? n : 1) * sizeof(T) + 256) != hipSuccess) return nullptr;
    p.push_back(v);
    return (T*)v;
  }
};

}  // namespace
}  // namespace ed

using namespace ed;
using namespace eng;

struct esmdiff_encoder : eng::Owner {
  int D = 0, VH = 0, FH = 0, n_layers = 0, d_out = 0, n_codes = 0, knn = 0, bins = 0;
  std::vector<Block> blocks;
  float *relpos = nullptr, *vq_b = nullptr, *code = nullptr;
  Linear vq;             // pre_vq_proj, in the blocks' form
  bool strict = false;   // precision = F32: float32 weights and activations, the linears on the f32-input MFMA (csrc/strict.hip)
};

extern "C" {

const char* esmdiff_encoder_last_error(const esmdiff_encoder* e) { return last_error(e); }

void esmdiff_encoder_destroy(esmdiff_encoder* e) {
  if (!e) return;
  hipSetDevice(e->device);
  hipDeviceSynchronize();
  for (void* p : e->allocs) hipFree(p);
  delete e;
}

int esmdiff_encoder_create(int32_t d_model, int32_t v_heads, int32_t n_layers, int32_t ffn_hidden, int32_t d_out,
                           int32_t n_codes, int32_t knn, int32_t relpos_bins, int32_t precision, const esmdiff_weight* table,
                           int32_t n, int32_t device, esmdiff_encoder** out) {
  if (!table || !out || n <= 0) return fail(nullptr, ESMDIFF_E_INVALID, "null argument");
  if (precision != ESMDIFF_PRECISION_BF16 && precision != ESMDIFF_PRECISION_F32) return fail(nullptr, ESMDIFF_E_INVALID, "precision: 0 (bf16) or 1 (f32)");
  *out = nullptr;
  if (d_model % 256 || d_model > 2048 || v_heads % 128 || ffn_hidden % 128 || d_out % 128 || n_layers <= 0 || knn <= 0 ||
      n_codes <= 0 || relpos_bins <= 0)
    return fail(nullptr, ESMDIFF_E_INVALID, "invalid encoder configuration");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device >= ndev || hipSetDevice(device) != hipSuccess)
    return fail(nullptr, ESMDIFF_E_NODEVICE, "no such HIP device");
  esmdiff_encoder* e = new esmdiff_encoder;
  e->device = device; e->D = d_model; e->VH = v_heads; e->FH = ffn_hidden; e->n_layers = n_layers; e->d_out = d_out;
  e->n_codes = n_codes; e->knn = knn; e->bins = relpos_bins;
  e->strict = precision == ESMDIFF_PRECISION_F32;
  const Linear::Form form = e->strict ? Linear::F32 : Linear::W16;
  const int D = d_model, VH = v_heads, FH = ffn_hidden;
  const Table t(table, n);   // exact names only
  auto bail = [&](int code) {   // the message outlives the encoder in the handle-less string
    const std::string msg = e->err;
    esmdiff_encoder_destroy(e);
    return fail(nullptr, code, "%s", msg.c_str());
  };
#define TRY(x)                         \
  do {                                 \
    if (int _r = (x)) return bail(_r); \
  } while (0)
  TRY(load_f32(e, t, "relative_positional_embedding.embedding.weight", {2 * relpos_bins + 2, D}, &e->relpos));
  e->blocks.resize(n_layers);
  for (int i = 0; i < n_layers; ++i) {
    Block& b = e->blocks[i];
    const std::string p = "transformer.blocks." + std::to_string(i) + ".";
    TRY(load_f32(e, t, p + "geom_attn.s_norm.weight", {D}, &b.s_norm_w));
    TRY(load_linear(e, t, p + "geom_attn.proj.weight", {15 * VH, D}, form, &b.proj));
    TRY(load_f32(e, t, p + "geom_attn.proj.bias", {15 * VH}, &b.proj_b));
    TRY(load_linear(e, t, p + "geom_attn.out_proj.weight", {D, 3 * VH}, form, &b.out));
    TRY(load_f32(e, t, p + "geom_attn.out_proj.bias", {D}, &b.out_b));
    TRY(load_f32(e, t, p + "geom_attn.rotation_scale_per_head", {VH}, &b.w_rot));
    TRY(load_f32(e, t, p + "geom_attn.distance_scale_per_head", {VH}, &b.w_dist));
    TRY(load_f32(e, t, p + "ffn.0.weight", {D}, &b.ln_w));
    TRY(load_f32(e, t, p + "ffn.0.bias", {D}, &b.ln_b));
    TRY(load_linear(e, t, p + "ffn.1.weight", {2 * FH, D}, form, &b.up));   // not interleaved: bias_swiglu reads [gate | up]
    TRY(load_f32(e, t, p + "ffn.1.bias", {2 * FH}, &b.b1));
    TRY(load_linear(e, t, p + "ffn.3.weight", {D, FH}, form, &b.down));
    TRY(load_f32(e, t, p + "ffn.3.bias", {D}, &b.b3));
  }
  TRY(load_linear(e, t, "pre_vq_proj.weight", {d_out, D}, form, &e->vq));
  TRY(load_f32(e, t, "pre_vq_proj.bias", {d_out}, &e->vq_b));
  TRY(load_f32(e, t, "codebook.embeddings", {n_codes, d_out}, &e->code));
  if (hipDeviceSynchronize() != hipSuccess) return bail(fail(e, ESMDIFF_E_HIP, "weight conversion failed"));
#undef TRY
  std::vector<float> hw(VH);
  for (Block& b : e->blocks)
    for (float* p : {b.w_rot, b.w_dist}) {  // softplus once, on the host
      hipMemcpy(hw.data(), p, VH * 4, hipMemcpyDeviceToHost);
      softplus_host(hw.data(), VH);
      hipMemcpy(p, hw.data(), VH * 4, hipMemcpyHostToDevice);
    }
  *out = e;
  return 0;
}

int esmdiff_encoder_encode(esmdiff_encoder* e, const float* ca, const float* rot, const float* trans, const uint8_t* has_frame,
                           int64_t* tokens, int32_t B, int32_t L, void* stream) {
  if (!e || !ca || !rot || !trans || !has_frame || !tokens || B <= 0 || L <= 0) return fail(e, ESMDIFF_E_INVALID, "invalid argument");
  if (L > 8192) return fail(e, ESMDIFF_E_CAPACITY, "L > 8192");
  if (hipSetDevice(e->device) != hipSuccess) return fail(e, ESMDIFF_E_HIP, "hipSetDevice failed");
  hipStream_t st = (hipStream_t)stream;
  const int D = e->D, VH = e->VH, FH = e->FH, K = e->knn < L ? e->knn : L;
  const int64_t R = (int64_t)B * L, M = R * K;
  if (M > (int64_t)1 << 30) return fail(e, ESMDIFF_E_CAPACITY, "B*L*knn too large");
  Tmp t;
  int32_t* edges = t.get<int32_t>(M);
  float *x = t.get<float>(M * D), *nrot = t.get<float>(M * 9), *ntrans = t.get<float>(M * 3), *zq = t.get<float>(R * e->d_out);
  uint8_t* nmask = t.get<uint8_t>(M);
  bf16_t *h = t.get<bf16_t>(M * D), *P = t.get<bf16_t>(M * 15 * VH), *G = t.get<bf16_t>(M * 3 * VH), *dA = t.get<bf16_t>(M * D),
         *dF = t.get<bf16_t>(M * D), *U = t.get<bf16_t>(M * 2 * FH), *mid = t.get<bf16_t>(M * FH), *z = t.get<bf16_t>(R * D);
  if (!edges || !x || !nrot || !ntrans || !zq || !nmask || !h || !P || !G || !dA || !dF || !U || !mid || !z)
    return fail(e, ESMDIFF_E_HIP, "encoder scratch allocation failed");
  HIP_TRY(e, launch_knn(ca, has_frame, B, L, K, edges, st));
  HIP_TRY(e, launch_neighbourhood(edges, e->relpos, rot, trans, has_frame, M, L, K, D, e->bins, x, nrot, ntrans, nmask, st));
  const int Mi = (int)M;
  if (e->strict) {
    // float32 end to end: x is updated in place by the residual epilogues (x + (acc + bias) / 1), the SwiGLU bias rides the
    // FFN-up GEMM's store epilogue.  Same order of operations as oracle/encoder_ref.py.
    float *fh = t.get<float>(M * D), *fP = t.get<float>(M * 15 * VH), *fG = t.get<float>(M * 3 * VH), *fU = t.get<float>(M * 2 * FH),
          *fmid = t.get<float>(M * FH), *fz = t.get<float>(R * D);
    if (!fh || !fP || !fG || !fU || !fmid || !fz) return fail(e, ESMDIFF_E_HIP, "encoder scratch allocation failed");
    for (const Block& b : e->blocks) {
      HIP_TRY(e, launch_layernorm_f32(x, b.s_norm_w, nullptr, fh, Mi, D, st));
      HIP_TRY(e, launch_gemm_f32(fh, D, b.proj.f32(), fP, b.proj_b, Mi, 15 * VH, D, 15 * VH, 15 * VH, 1.f, ESMDIFF_F32EPI_STORE, st));
      HIP_TRY(e, launch_geom_attention_f32(fP, nrot, ntrans, nmask, b.w_rot, b.w_dist, fG, (int)R, K, VH, st));
      HIP_TRY(e, launch_gemm_f32(fG, 3 * VH, b.out.f32(), x, b.out_b, Mi, D, 3 * VH, D, D, 1.f, ESMDIFF_F32EPI_RESID_DIV, st));
      HIP_TRY(e, launch_layernorm_f32(x, b.ln_w, b.ln_b, fh, Mi, D, st));
      HIP_TRY(e, launch_gemm_f32(fh, D, b.up.f32(), fU, b.b1, Mi, 2 * FH, D, 2 * FH, 2 * FH, 1.f, ESMDIFF_F32EPI_STORE, st));
      HIP_TRY(e, launch_swiglu_f32(fU, fmid, Mi, FH, st));
      HIP_TRY(e, launch_gemm_f32(fmid, FH, b.down.f32(), x, b.b3, Mi, D, FH, D, D, 1.f, ESMDIFF_F32EPI_RESID_DIV, st));
    }
    HIP_TRY(e, launch_query_rows_f32(x, has_frame, R, K, D, fz, st));
    HIP_TRY(e, launch_gemm_f32(fz, D, e->vq.f32(), zq, e->vq_b, (int)R, e->d_out, D, e->d_out, e->d_out, 1.f, ESMDIFF_F32EPI_STORE, st));
    HIP_TRY(e, launch_codebook(zq, e->code, has_frame, R, e->n_codes, e->d_out, tokens, st));
    HIP_TRY(e, hipStreamSynchronize(st));
    return 0;
  }
  bool pending = false;
  for (const Block& b : e->blocks) {
    // x += dF (previous block's FFN); h = s_norm(x)
    HIP_TRY(e, launch_add_layernorm_bf16(x, pending ? dF : nullptr, nullptr, 1, b.s_norm_w, nullptr, h, Mi, D, st));
    HIP_TRY(e, launch_gemm_bf16(h, b.proj.w16(), P, nullptr, Mi, 15 * VH, D, 15 * VH, 15 * VH, 1.f, ESMDIFF_EPI_BF16, st));
    HIP_TRY(e, launch_add_bias_bf16(P, b.proj_b, M, 15 * VH, st));
    HIP_TRY(e, launch_geom_attention(P, nrot, ntrans, nmask, b.w_rot, b.w_dist, G, (int)R, K, VH, st));
    HIP_TRY(e, launch_gemm_bf16(G, b.out.w16(), dA, nullptr, Mi, D, 3 * VH, D, D, 1.f, ESMDIFF_EPI_BF16, st));
    HIP_TRY(e, launch_add_bias_bf16(dA, b.out_b, M, D, st));
    // x += dA; h = LN(x); FFN
    HIP_TRY(e, launch_add_layernorm_bf16(x, dA, nullptr, 1, b.ln_w, b.ln_b, h, Mi, D, st));
    HIP_TRY(e, launch_gemm_bf16(h, b.up.w16(), U, nullptr, Mi, 2 * FH, D, 2 * FH, 2 * FH, 1.f, ESMDIFF_EPI_BF16, st));
    HIP_TRY(e, launch_bias_swiglu(U, b.b1, M, FH, mid, st));
    HIP_TRY(e, launch_gemm_bf16(mid, b.down.w16(), dF, nullptr, Mi, D, FH, D, D, 1.f, ESMDIFF_EPI_BF16, st));
    HIP_TRY(e, launch_add_bias_bf16(dF, b.b3, M, D, st));
    pending = true;
  }
  HIP_TRY(e, launch_query_rows(x, dF, has_frame, R, K, D, z, st));
  HIP_TRY(e, launch_gemm_bf16(z, e->vq.w16(), zq, e->vq_b, (int)R, e->d_out, D, e->d_out, e->d_out, 1.f, ESMDIFF_EPI_BIAS_F32, st));
  HIP_TRY(e, launch_codebook(zq, e->code, has_frame, R, e->n_codes, e->d_out, tokens, st));
  HIP_TRY(e, hipStreamSynchronize(st));  // the scratch is freed on return
  return 0;
}

// ---- test entries (include/esmdiff_hip_test.h): the glue kernels above, one at a time, through the launchers that
// esmdiff_encoder_encode calls.  Synchronous; errors go to esmdiff_encoder_last_error(NULL). ----
static int glue_done(hipError_t s, hipStream_t st, const char* name) {
  const hipError_t s2 = hipStreamSynchronize(st);
  if (s == hipSuccess) s = s2;
  return s == hipSuccess ? 0 : fail(nullptr, ESMDIFF_E_HIP, "%s: %s", name, hipGetErrorString(s));
}

int esmdiff_encoder_knn(const float* ca, const uint8_t* has, int32_t B, int32_t L, int32_t knn, int32_t* edges, void* stream) {
  if (!ca || !has || !edges || B <= 0 || L <= 0 || knn <= 0) return fail(nullptr, ESMDIFF_E_INVALID, "encoder_knn: invalid argument");
  if (L > 8192) return fail(nullptr, ESMDIFF_E_INVALID, "encoder_knn: L > 8192");
  const int K = knn < L ? knn : L;
  if ((int64_t)B * L * K > (int64_t)1 << 30) return fail(nullptr, ESMDIFF_E_INVALID, "encoder_knn: B*L*knn too large");
  hipStream_t st = (hipStream_t)stream;
  return glue_done(launch_knn(ca, has, B, L, K, edges, st), st, "knn_kernel");
}

int esmdiff_encoder_neighbourhood(const int32_t* edges, const float* table, const float* rot, const float* trans, const uint8_t* has,
                                  int32_t B, int32_t L, int32_t K, int32_t D, int32_t bins, float* x, float* nrot, float* ntrans,
                                  uint8_t* nmask, void* stream) {
  if (!edges || !table || !rot || !trans || !has || !x || !nrot || !ntrans || !nmask)
    return fail(nullptr, ESMDIFF_E_INVALID, "encoder_neighbourhood: null pointer");
  if (B <= 0 || L <= 0 || K <= 0 || K > L || D <= 0 || D % 4 || bins <= 0)
    return fail(nullptr, ESMDIFF_E_INVALID, "encoder_neighbourhood: B, L, K <= L, D %% 4 == 0 and bins must be positive");
  const int64_t M = (int64_t)B * L * K;
  if (M > (int64_t)1 << 30) return fail(nullptr, ESMDIFF_E_INVALID, "encoder_neighbourhood: B*L*K too large");
  hipStream_t st = (hipStream_t)stream;
  // the kernel gathers rows by edge: every index is checked on the host before the launch
  std::vector<int32_t> he((size_t)M);
  if (hipStreamSynchronize(st) != hipSuccess || hipMemcpy(he.data(), edges, (size_t)M * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess)
    return fail(nullptr, ESMDIFF_E_HIP, "encoder_neighbourhood: reading the edges failed");
  for (int32_t v : he)
    if (v < 0 || v >= L) return fail(nullptr, ESMDIFF_E_INVALID, "encoder_neighbourhood: edge outside 0 .. L-1");
  return glue_done(launch_neighbourhood(edges, table, rot, trans, has, M, L, K, D, bins, x, nrot, ntrans, nmask, st), st,
                   "neighbourhood_kernel");
}

int esmdiff_encoder_nearest_code(const float* z, const float* code, const uint8_t* has, int32_t R, int32_t n_codes, int32_t d_out,
                                 int64_t* tok, void* stream) {
  if (!z || !code || !has || !tok) return fail(nullptr, ESMDIFF_E_INVALID, "encoder_nearest_code: null pointer");
  if (R <= 0 || n_codes <= 0 || d_out <= 0 || d_out > 8192)
    return fail(nullptr, ESMDIFF_E_INVALID, "encoder_nearest_code: R, n_codes and d_out (<= 8192) must be positive");
  hipStream_t st = (hipStream_t)stream;
  return glue_done(launch_codebook(z, code, has, R, n_codes, d_out, tok, st), st, "codebook_kernel");
}

}  // extern "C"


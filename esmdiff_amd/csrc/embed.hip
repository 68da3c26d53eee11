// embed.hip — input stage of the network and the time-conditioning MLP (gfx950).
//
// embed_kernel: /root/reference/slm/models/net.py:445-466.  With the defaults CustomizedESM3.forward
// injects for every track other than sequence and structure (net.py:410-436), esm's EncodeInputs
// collapses to  x[b,l] = E_seq[seq] + E_struct[struct'] + c, where c is one constant vector (built at
// engine create from plddt_projection / structure_per_res_plddt_projection / ss8_embed / sasa_embed)
// and struct' has BOS/PAD/EOS/chainbreak forced from the sequence track (net.py:445-454).  The
// time-conditioning vector (auxiliary_embeddings: sigma_embedder(sigma) tiled over the rows of a sample, model.py:466-471;
// one vector for the whole batch in the sampling loop, one per sample when the caller passes per-sample sigmas) is added in
// the same pass.
// sigma_mlp: TimestepEmbedder.mlp (net.py:489-492): Linear -> SiLU -> Linear on the 256-d sinusoid.
#include "kernels.h"

namespace ed {

typedef __attribute__((ext_vector_type(4))) float f32x4;

__global__ __launch_bounds__(256) void embed_kernel(const int64_t* __restrict__ seq, const int64_t* __restrict__ xtok,
                                                    const float* __restrict__ e_seq, const float* __restrict__ e_struct,
                                                    const float* __restrict__ cvec, const float* __restrict__ cond,
                                                    float* __restrict__ out, int M, int D, int L, int cond_stride) {
  const int row = blockIdx.x;
  if (row >= M) return;
  if (cond) cond += (int64_t)(row / L) * cond_stride;   // cond_stride 0: one vector for all samples
  // ids are validated by the host wrapper (Engine._check_ids); a direct C-ABI caller's out-of-range id is clamped
  // here so that it can never read outside the embedding tables
  const int64_t s = min(max(seq[row], (int64_t)0), (int64_t)63);
  int64_t t = xtok[row];
  if (t == -1) t = ESMDIFF_MASK_ID;
  t = min(max(t, (int64_t)0), (int64_t)(ESMDIFF_VOCAB - 1));
  if (s == 0) t = ESMDIFF_STRUCT_BOS;          // SEQUENCE_BOS
  if (s == 1) t = ESMDIFF_STRUCT_PAD;          // SEQUENCE_PAD
  if (s == 2) t = ESMDIFF_STRUCT_EOS;          // SEQUENCE_EOS
  if (s == 31) t = ESMDIFF_STRUCT_CHAINBREAK;  // SEQUENCE_CHAINBREAK
  const float* a = e_seq + s * D;
  const float* b = e_struct + t * D;
  float* o = out + (int64_t)row * D;
  for (int c = threadIdx.x * 4; c < D; c += 1024) {
    f32x4 v = *reinterpret_cast<const f32x4*>(a + c);
    const f32x4 w = *reinterpret_cast<const f32x4*>(b + c);
    const f32x4 k = *reinterpret_cast<const f32x4*>(cvec + c);
    v[0] = (v[0] + w[0]) + k[0]; v[1] = (v[1] + w[1]) + k[1];
    v[2] = (v[2] + w[2]) + k[2]; v[3] = (v[3] + w[3]) + k[3];
    if (cond) {
      const f32x4 z = *reinterpret_cast<const f32x4*>(cond + c);
      v[0] += z[0]; v[1] += z[1]; v[2] += z[2]; v[3] += z[3];
    }
    *reinterpret_cast<f32x4*>(o + c) = v;
  }
}

// y[r][n] = act(W[n,:] · x[r] + b[n]); one wave per output, f32; blockIdx.y = r (one input vector per sigma).
template <bool SILU>
__global__ __launch_bounds__(256) void gemv_kernel(const float* __restrict__ W, const float* __restrict__ bias,
                                                   const float* __restrict__ x, float* __restrict__ y, int N, int K) {
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (n >= N) return;
  x += (int64_t)blockIdx.y * K;
  y += (int64_t)blockIdx.y * N;
  float acc = 0.f;
  for (int k = lane; k < K; k += 64) acc += W[(int64_t)n * K + k] * x[k];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if (lane == 0) {
    float v = acc + bias[n];
    if (SILU) v = v / (1.0f + expf(-v));
    y[n] = v;
  }
}

hipError_t launch_embed(const int64_t* seq, const int64_t* xtok, const float* e_seq, const float* e_struct,
                        const float* cvec, const float* cond, float* out, int B, int L, int D,
                        hipStream_t stream, int cond_stride) {
  const int M = B * L;
  if (M <= 0) return hipSuccess;
  if (D % 4) return hipErrorInvalidValue;
  hipLaunchKernelGGL(embed_kernel, dim3(M), dim3(256), 0, stream, seq, xtok, e_seq, e_struct, cvec, cond, out, M, D, L,
                     cond_stride);
  return hipGetLastError();
}

hipError_t launch_sigma_mlp(const float* t_freq, const float* w1, const float* b1, const float* w2,
                            const float* b2, float* hidden, float* cond, int F, int D, hipStream_t stream, int n_sigma) {
  // t_freq [n_sigma, F] -> hidden [n_sigma, D] -> cond [n_sigma, D]
  hipLaunchKernelGGL(gemv_kernel<true>, dim3((D + 3) / 4, n_sigma), dim3(256), 0, stream, w1, b1, t_freq, hidden, D, F);
  hipLaunchKernelGGL(gemv_kernel<false>, dim3((D + 3) / 4, n_sigma), dim3(256), 0, stream, w2, b2, hidden, cond, D, D);
  return hipGetLastError();
}

// ---- VQ-VAE structure-token decoder ends ([ESM-RECALL]) -----------------------------------------
// gather_rows: x[row] = table[tok[row]] (esm StructureTokenDecoder.embed: one nn.Embedding over the 4096 + 5 ids)
__global__ __launch_bounds__(256) void gather_rows_kernel(const int64_t* __restrict__ tok, const float* __restrict__ table,
                                                          float* __restrict__ out, int M, int D, int n_rows) {
  const int row = blockIdx.x;
  if (row >= M) return;
  int64_t t = tok[row];
  t = t < 0 ? 0 : (t >= n_rows ? n_rows - 1 : t);
  const float* a = table + t * D;
  float* o = out + (int64_t)row * D;
  for (int c = threadIdx.x * 4; c < D; c += 1024) *reinterpret_cast<f32x4*>(o + c) = *reinterpret_cast<const f32x4*>(a + c);
}

hipError_t launch_gather_rows(const int64_t* tok, const float* table, float* out, int M, int D, int n_rows,
                              hipStream_t stream) {
  if (M <= 0) return hipSuccess;
  hipLaunchKernelGGL(gather_rows_kernel, dim3(M), dim3(256), 0, stream, tok, table, out, M, D, n_rows);
  return hipGetLastError();
}

// dim6_to_backbone: the tail of esm's Dim6RotStructureHead with affine = identity: per residue the 23-vector is
// [trans 3 | x 3 | y 3 | 14 unused]; trans *= trans_scale; x, y /= (|.| + 1e-5); frame = Gram-Schmidt with origin trans,
// first axis along -x ... exactly Affine3D.from_graham_schmidt(neg_x_axis = x + trans, origin = trans, xy_plane =
// y + trans): e0 = normalise(trans - (x + trans)) = -x^, e1 = normalise(y - (y.e0) e0), e2 = e0 x e1; the ideal N / CA / C
// positions in that frame (BB_COORDINATES) are then moved to the global frame:  p = R b + trans.
__global__ __launch_bounds__(256) void dim6_to_backbone_kernel(const float* __restrict__ v, int ld, float* __restrict__ out,
                                                               int M, float trans_scale) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= M) return;
  const float* p = v + (int64_t)row * ld;
  const float t[3] = {p[0] * trans_scale, p[1] * trans_scale, p[2] * trans_scale};
  float x[3] = {p[3], p[4], p[5]}, y[3] = {p[6], p[7], p[8]};
  const float nx = sqrtf(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]) + 1e-5f;
  const float ny = sqrtf(y[0] * y[0] + y[1] * y[1] + y[2] * y[2]) + 1e-5f;
#pragma unroll
  for (int i = 0; i < 3; ++i) { x[i] /= nx; y[i] /= ny; }
  // Gram-Schmidt (eps 1e-12 under the square roots, as in the frame builder of the conditioning path)
  float e0[3] = {-x[0], -x[1], -x[2]};
  const float n0 = sqrtf(e0[0] * e0[0] + e0[1] * e0[1] + e0[2] * e0[2] + 1e-12f);
#pragma unroll
  for (int i = 0; i < 3; ++i) e0[i] /= n0;
  const float d = e0[0] * y[0] + e0[1] * y[1] + e0[2] * y[2];
  float e1[3] = {y[0] - e0[0] * d, y[1] - e0[1] * d, y[2] - e0[2] * d};
  const float n1 = sqrtf(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2] + 1e-12f);
#pragma unroll
  for (int i = 0; i < 3; ++i) e1[i] /= n1;
  const float e2[3] = {e0[1] * e1[2] - e0[2] * e1[1], e0[2] * e1[0] - e0[0] * e1[2], e0[0] * e1[1] - e0[1] * e1[0]};
  const float bb[3][3] = {{0.5256f, 1.3612f, 0.0f}, {0.0f, 0.0f, 0.0f}, {-1.5251f, 0.0f, 0.0f}};  // N, CA, C
  float* o = out + (int64_t)row * 9;
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int i = 0; i < 3; ++i) o[a * 3 + i] = e0[i] * bb[a][0] + e1[i] * bb[a][1] + e2[i] * bb[a][2] + t[i];
}

// plddt_mean: esm's CategoricalMixture(plddt_logits, bins).mean() [ESM-RECALL]: softmax over the n_bins logits of a row
// times the bin centres (i + 0.5) / n_bins of [0, 1].  One thread per row (n_bins = 50).
__global__ __launch_bounds__(256) void plddt_mean_kernel(const float* __restrict__ v, int ld, int n_bins, float* __restrict__ out, int M) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= M) return;
  const float* p = v + (int64_t)row * ld;
  float m = p[0];
  for (int i = 1; i < n_bins; ++i) m = fmaxf(m, p[i]);
  float s = 0.f, a = 0.f;
  for (int i = 0; i < n_bins; ++i) {
    const float e = expf(p[i] - m);
    s += e;
    a += e * ((float)i + 0.5f) / (float)n_bins;
  }
  out[row] = a / s;
}

hipError_t launch_plddt_mean(const float* v, int ld, int n_bins, float* out, int M, hipStream_t stream) {
  if (M <= 0) return hipSuccess;
  hipLaunchKernelGGL(plddt_mean_kernel, dim3((M + 255) / 256), dim3(256), 0, stream, v, ld, n_bins, out, M);
  return hipGetLastError();
}

hipError_t launch_dim6_to_backbone(const float* v, int ld, float* out, int M, float trans_scale, hipStream_t stream) {
  if (M <= 0) return hipSuccess;
  hipLaunchKernelGGL(dim6_to_backbone_kernel, dim3((M + 255) / 256), dim3(256), 0, stream, v, ld, out, M, trans_scale);
  return hipGetLastError();
}

}  // namespace ed

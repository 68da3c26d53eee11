// score.hip — the forward-only half of the reference's validation metric (gfx950): how likely the model finds a structure.
//
// Replaces, around one network forward with one sigma per sample,
//   q_xt                       /root/reference/slm/models/model.py:494-512   (q_xt_kernel)
//   logits_parameterization    /root/reference/slm/models/model.py:527-533
//   gather at x0               /root/reference/slm/models/model.py:432-436
//   loss weighting             /root/reference/slm/models/model.py:438-443   (nelbo_rows_kernel)
//   (loss * loss_mask).sum()   /root/reference/slm/models/model.py:445, per sample (nelbo_reduce_kernel)
// which the reference runs as a dozen elementwise / reduction passes over a (B,L,4101) float tensor.
//
// Mapping of nelbo_rows_kernel: sampler.hip's — one 256-thread workgroup (4 waves) per (b,l) row, the row (4101 floats) read ONCE
// into registers (17 per thread, coalesced dword loads).  A row that is not MASK leaves without touching its logits.  HBM-bound:
// 4·V bytes per masked row, the bytes of ddpm_step_kernel with less arithmetic (no Philox per element, no divide).
//
// Float-operation order of the log-sum-exp: the canonical one of oracle/csrc/sampler_oracle.c (row_logprob), as in
// ddpm_step_kernel operation by operation (mask column + -1e6, wave_max, ed_expf, thread t sums v = t, t + 256, ..., halving tree
// per wave, (s0 + s1) + (s2 + s3), m + ed_logf(s); the two wave reductions are the sampler's own, csrc/ed_wave.h), so that
// log_p = z[x0] - lse is the oracle's logits_parameterization value bit for bit.  Compiled with -ffp-contract=off like sampler.hip.
// No atomics: every output is a function of its own sample alone.
#include "ed_math.h"
#include "ed_wave.h"
#include "kernels.h"

namespace ed {

namespace {

constexpr int SNT = 256;
constexpr int S_MASK_ID = ESMDIFF_MASK_ID;
constexpr int S_SEQ_MASK_ID = 32;        // esm's SEQUENCE_MASK_TOKEN (model.py:382)
constexpr int S_MAX_PER_THREAD = 20;     // V <= 5120, as in sampler.hip

}  // namespace

// xt = moved ? MASK : x0, moved = u < move_chance[b] and not non_moving and l < len[b]; one thread per token.
// u: explicit uniforms [B,L] or the Philox uniform of (seed, sample_index[b], draw[b], l, ESMDIFF_QXT_PHILOX_COLUMN).
__global__ __launch_bounds__(SNT) void q_xt_kernel(const int64_t* x0, const int64_t* seq, const float* __restrict__ move_chance,
                                                   const uint8_t* __restrict__ non_moving, const float* __restrict__ u,
                                                   uint64_t seed, const uint64_t* __restrict__ sample_index,
                                                   const int32_t* __restrict__ draw, const int32_t* __restrict__ lens,
                                                   int64_t* xt, int64_t* seq_out, int64_t n, int L) {
  const int64_t i = (int64_t)blockIdx.x * SNT + threadIdx.x;
  if (i >= n) return;
  const int b = (int)(i / L), l = (int)(i - (int64_t)b * L);
  const float uu = u ? u[i] : ed_philox_uniform(seed, sample_index[b], (uint32_t)draw[b], (uint32_t)l, ESMDIFF_QXT_PHILOX_COLUMN);
  bool moved = uu < move_chance[b];
  if (non_moving && non_moving[i]) moved = false;
  if (lens && l >= lens[b]) moved = false;
  const int64_t x = x0[i];
  xt[i] = moved ? (int64_t)S_MASK_ID : x;
  if (seq_out) seq_out[i] = moved ? (int64_t)S_SEQ_MASK_ID : seq[i];   // coupled_condition_mask, model.py:510-511
}

// log_p[row] = logits_parameterization(logits, xt)[row, x0[row]]; row_loss[row] = log_p * weight[b] (the host passes the signed
// weight: -(dsigma / expm1(sigma)), or +log1p(-exp(-sigma_min)) in the change-of-variables / importance-sampling branch).
template <int PER>
__global__ __launch_bounds__(SNT) void nelbo_rows_kernel(const float* __restrict__ logits, int ld, int V,
                                                         const int64_t* __restrict__ xt, const int64_t* __restrict__ x0,
                                                         const float* __restrict__ weight, float* __restrict__ log_p,
                                                         float* __restrict__ row_loss, int L) {
  const int row = blockIdx.x;
  const int t = threadIdx.x;
  const int64_t xr = xt[row], target = x0[row];
  const bool in_range = target >= 0 && target < V;   // (the host raises on an id outside the vocabulary; never read outside the row)
  if (xr != S_MASK_ID) {   // model.py:530-532: -1e6 everywhere, 0 at the row's own token
    if (t == 0) {
      const float lp = (target == xr) ? 0.0f : -1000000.0f;
      if (log_p) log_p[row] = lp;
      row_loss[row] = lp * weight[row / L];
    }
    return;
  }

  __shared__ float s_red[8];
  const int lane = t & 63, wave = t >> 6;
  const float* z = logits + (int64_t)row * ld;

  float zz[PER];
  float m = -3.402823466e38f;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int v = t + j * SNT;
    float val = -3.402823466e38f;
    if (v < V) {
      val = z[v];
      if (v == S_MASK_ID) val = val + -1000000.0f;  // logits[:, :, mask] += neg_infinity
      m = fmaxf(m, val);
    }
    zz[j] = val;
  }
  m = wave_max(m);
  if (lane == 0) s_red[wave] = m;
  __syncthreads();
  m = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));

  float acc = 0.0f;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int v = t + j * SNT;
    if (v < V) acc = acc + ed_expf(zz[j] - m);
  }
  acc = wave_halving_sum(acc);
  if (lane == 0) s_red[4 + wave] = acc;
  __syncthreads();
  if (t == 0) {
    const float s = (s_red[4] + s_red[5]) + (s_red[6] + s_red[7]);
    const float lse = m + ed_logf(s);
    float lp = -1000000.0f;
    if (in_range) {
      float zx = z[target];   // (the row was just read: a cache hit)
      if (target == S_MASK_ID) zx = zx + -1000000.0f;
      lp = zx - lse;
    }
    if (log_p) log_p[row] = lp;
    row_loss[row] = lp * weight[row / L];
  }
}

// sample_sum[b] = sum_l row_loss[b,l] * loss_mask[b,l], sample_count[b] = sum_l loss_mask[b,l], l < len[b]; one workgroup per
// sample, fixed order: thread t adds l = t, t + 256, ... ascending from 0, halving tree per wave, (w0 + w1) + (w2 + w3).
__global__ __launch_bounds__(SNT) void nelbo_reduce_kernel(const float* __restrict__ row_loss, const uint8_t* __restrict__ loss_mask,
                                                           const int32_t* __restrict__ lens, float* __restrict__ sample_sum,
                                                           int32_t* __restrict__ sample_count, int L) {
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int n = lens ? min(lens[b], L) : L;
  __shared__ float s_sum[4];
  __shared__ int s_cnt[4];
  float acc = 0.0f;
  int cnt = 0;
  for (int l = t; l < L; l += SNT) {
    const int64_t i = (int64_t)b * L + l;
    const int on = (l < n && (!loss_mask || loss_mask[i])) ? 1 : 0;
    acc = acc + row_loss[i] * (float)on;   // (loss * loss_mask), model.py:445
    cnt += on;
  }
  acc = wave_halving_sum(acc);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_down(cnt, off, 64);
  if (lane == 0) {
    s_sum[wave] = acc;
    s_cnt[wave] = cnt;
  }
  __syncthreads();
  if (t == 0) {
    sample_sum[b] = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
    sample_count[b] = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
  }
}

hipError_t launch_q_xt(const int64_t* x0, const int64_t* seq, const float* move_chance, const uint8_t* non_moving, const float* u,
                       uint64_t seed, const uint64_t* sample_index, const int32_t* draw, const int32_t* lens, int64_t* xt,
                       int64_t* seq_out, int B, int L, hipStream_t stream) {
  const int64_t n = (int64_t)B * L;
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(q_xt_kernel, dim3((unsigned)((n + SNT - 1) / SNT)), dim3(SNT), 0, stream, x0, seq, move_chance, non_moving, u,
                     seed, sample_index, draw, lens, xt, seq_out, n, L);
  return hipGetLastError();
}

hipError_t launch_nelbo_rows(const float* logits, int ld, int V, const int64_t* xt, const int64_t* x0, const float* weight,
                             const uint8_t* loss_mask, const int32_t* lens, float* log_p, float* row_loss, float* sample_sum,
                             int32_t* sample_count, int B, int L, hipStream_t stream) {
  const int rows = B * L;
  if (rows <= 0) return hipSuccess;
  const int per = (V + SNT - 1) / SNT;
  if (per > S_MAX_PER_THREAD) return hipErrorInvalidValue;
  dim3 grid(rows), block(SNT);
#define ED_LAUNCH(P) \
  hipLaunchKernelGGL((nelbo_rows_kernel<P>), grid, block, 0, stream, logits, ld, V, xt, x0, weight, log_p, row_loss, L)
  if (per <= 1) ED_LAUNCH(1);
  else if (per <= 4) ED_LAUNCH(4);
  else if (per <= 17) ED_LAUNCH(17);
  else ED_LAUNCH(S_MAX_PER_THREAD);
#undef ED_LAUNCH
  hipError_t s = hipGetLastError();
  if (s != hipSuccess) return s;
  hipLaunchKernelGGL(nelbo_reduce_kernel, dim3(B), block, 0, stream, row_loss, loss_mask, lens, sample_sum, sample_count, L);
  return hipGetLastError();
}

// this unit's compiled copy of csrc/ed_math.h, one element at a time (esmdiff_math_eval, unit 1)
#define ED_MATH_EVAL_UNIT score
#include "ed_math_eval.inc"
#undef ED_MATH_EVAL_UNIT

}  // namespace ed

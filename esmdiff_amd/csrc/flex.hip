// flex.hip — residue flexibility of an ensemble of CA traces, float64, on the device.
//
//   flex_pair_msf_kernel   the reference's pairwise "RMSF" (analysis/apo_analysis.py:252-260) without its (n, n, L) array: for every
//                          pair i < j a proper Kabsch fit of a_i onto a_j on the residues valid in both, and the squared deviation of
//                          every such residue added to a per-wave partial sum.  One WAVE per pair, as superpose_pairs_kernel: the
//                          centroids and the covariance are wave-shuffle reductions, the 3x3 decomposition (ed_kabsch.h) runs
//                          redundantly in every lane.  A pair's deviations live in registers only.
//   flex_reduce_kernel     the second pass: the partials of all waves, summed per residue.
//   flex_fit_kernel        one WAVE per structure: the fit onto one common reference, the whole structure transformed.
//   flex_transforms_kernel the same fit, one WAVE per structure: rot and tr written out (what csrc/aligned.hip applies inside its
//                          kernels), no moved structure.
//   flex_moments_kernel    one WAVE per residue: the mean position over the structures valid there, then (second pass) the mean
//                          squared distance from it.
//
// The order of every sum is a function of (n, L) alone, and nothing is accumulated with atomics, so two runs are bit-identical:
//   pair kernel   Workgroup (t, c), t < T = ceil(n / 2), c < C (the header's ESMDIFF_FLEX_PAIR_CHUNKS), owns rows t and n - 1 - t of the
//                 triangle (together n - 1 pairs whatever t: the triangle is balanced), laid out as one list p = 0 .. n - 2: first
//                 (t, t + 1 + p), then (n - 1 - t, n - t + q).  Its wave w takes p = g, g + 4 C, g + 8 C ... with g = 4 c + w, in that order, and adds each
//                 pair into slot s = 4 (t C + c) + w of the scratch: part[s][l] (f64) and part_count[s][l] (i32).  Residue l of a slot
//                 is only ever touched by lane l % 64 of that one wave, which zeroes it first; there is no barrier in the kernel.
//                 Inside a pair the sums over residues are the strided per-lane sums and xor butterflies of superpose.hip.
//   reduce        Workgroup b owns residues 64 b .. 64 b + 63; its wave w adds the slots s = w, w + 4, w + 8 ... in increasing order,
//                 and the four wave sums are combined as (w0 + w1) + (w2 + w3).
//   moments       Lane k of a residue's wave adds structures k, k + 64 ... in order; xor butterfly across the lanes.
// Memory: 4 T C slots of L (f64 + i32), C = clamp(2048 / T, 1, 16): at most max(8192, 2 n + 2) slots of 12 L bytes, O(n L).  There is
// no limit on L: the structures are read from global memory (a wave's two structures stay in L1 / L2 across its three passes).
#include <math.h>

#include "ed_kabsch.h"
#include "ed_wave.h"
#include "kernels.h"

namespace ed {
namespace {

// The proper Kabsch fit of a onto b on the residues valid in both, by one wave: cnt (the number of those residues; nothing else is
// set when it is below 2), rot, tr with rot a + tr ~ b.  Every lane ends with the same bits.
template <class Valid>
__device__ __forceinline__ void wave_fit(const double* __restrict__ a, const double* __restrict__ b, int L, int lane, Valid valid,
                                         int& cnt, double* rot, double* tr) {
  double sa[3] = {0, 0, 0}, sb[3] = {0, 0, 0};
  cnt = 0;
  for (int l = lane; l < L; l += 64)
    if (valid(l)) {
      ++cnt;
#pragma unroll
      for (int c = 0; c < 3; ++c) sa[c] += a[3 * l + c], sb[c] += b[3 * l + c];
    }
  cnt = wave_sum(cnt);
  if (cnt < 2) return;
  double ca[3], cb[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) ca[c] = wave_sum(sa[c]) / cnt, cb[c] = wave_sum(sb[c]) / cnt;
  double h[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int l = lane; l < L; l += 64)
    if (valid(l)) {
      const double x[3] = {a[3 * l] - ca[0], a[3 * l + 1] - ca[1], a[3 * l + 2] - ca[2]};
      const double y[3] = {b[3 * l] - cb[0], b[3 * l + 1] - cb[1], b[3 * l + 2] - cb[2]};
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) h[3 * r + c] += x[r] * y[c];
    }
#pragma unroll
  for (int k = 0; k < 9; ++k) h[k] = wave_sum(h[k]);
  kabsch_rotation(h, 0, rot);
#pragma unroll
  for (int r = 0; r < 3; ++r) tr[r] = cb[r] - (rot[3 * r] * ca[0] + rot[3 * r + 1] * ca[1] + rot[3 * r + 2] * ca[2]);
}

__global__ __launch_bounds__(256) void flex_pair_msf_kernel(const double* __restrict__ A, const uint8_t* __restrict__ maskA, int n,
                                                            int L, int C, double* __restrict__ part,
                                                            int32_t* __restrict__ part_count) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int t = blockIdx.x, c = blockIdx.y;
  const int64_t slot = 4 * ((int64_t)t * C + c) + wave;
  double* acc = part + slot * L;
  int32_t* acc_n = part_count + slot * L;
  for (int l = lane; l < L; l += 64) acc[l] = 0.0, acc_n[l] = 0;

  const int r1 = n - 1 - t, first = n - 1 - t;             // row t has `first` pairs, row r1 (when it is another row) t more
  const int total = r1 == t ? first : n - 1;
  for (int p = 4 * c + wave; p < total; p += 4 * C) {      // wave-uniform: the whole wave takes a pair or leaves
    const int i = p < first ? t : r1;
    const int j = p < first ? t + 1 + p : r1 + 1 + (p - first);
    const double* a = A + (int64_t)i * L * 3;
    const double* b = A + (int64_t)j * L * 3;
    const uint8_t* ma = maskA ? maskA + (int64_t)i * L : nullptr;
    const uint8_t* mb = maskA ? maskA + (int64_t)j * L : nullptr;
    auto valid = [&](int l) { return !ma || (ma[l] && mb[l]); };
    int cnt;
    double rot[9], tr[3];
    wave_fit(a, b, L, lane, valid, cnt, rot, tr);
    if (cnt < 2) continue;                                 // contributes nothing and is not counted
    for (int l = lane; l < L; l += 64)
      if (valid(l)) {
        double d2 = 0;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const double e = (rot[3 * r] * a[3 * l] + rot[3 * r + 1] * a[3 * l + 1] + rot[3 * r + 2] * a[3 * l + 2] + tr[r]) - b[3 * l + r];
          d2 += e * e;
        }
        acc[l] += d2;
        acc_n[l] += 1;
      }
  }
}

__global__ __launch_bounds__(256) void flex_reduce_kernel(const double* __restrict__ part, const int32_t* __restrict__ part_count,
                                                          int64_t slots, int L, double* __restrict__ sum_sq,
                                                          int64_t* __restrict__ count) {
  __shared__ double s_sum[4][64];
  __shared__ int64_t s_cnt[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l = blockIdx.x * 64 + lane;
  double s = 0;
  int64_t k = 0;
  if (l < L)
    for (int64_t q = wave; q < slots; q += 4) s += part[q * L + l], k += part_count[q * L + l];
  s_sum[wave][lane] = s;
  s_cnt[wave][lane] = k;
  __syncthreads();
  if (wave == 0 && l < L) {
    sum_sq[l] = (s_sum[0][lane] + s_sum[1][lane]) + (s_sum[2][lane] + s_sum[3][lane]);
    count[l] = (s_cnt[0][lane] + s_cnt[1][lane]) + (s_cnt[2][lane] + s_cnt[3][lane]);
  }
}

__global__ __launch_bounds__(256) void flex_fit_kernel(const double* __restrict__ A, const uint8_t* __restrict__ maskA,
                                                       const double* __restrict__ ref, const uint8_t* __restrict__ mask_ref, int n,
                                                       int L, double* __restrict__ aligned, double* __restrict__ rmsd) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;                                      // the whole wave leaves; the kernel has no barrier
  const double* a = A + i * L * 3;
  const uint8_t* ma = maskA ? maskA + i * L : nullptr;
  auto valid = [&](int l) { return (!ma || ma[l]) && (!mask_ref || mask_ref[l]); };
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  int cnt;
  double rot[9], tr[3];
  wave_fit(a, ref, L, lane, valid, cnt, rot, tr);
  if (cnt < 2) {
    if (aligned)
      for (int k = lane; k < 3 * L; k += 64) aligned[i * L * 3 + k] = nan;
    if (lane == 0 && rmsd) rmsd[i] = nan;
    return;
  }
  double acc = 0;
  for (int l = lane; l < L; l += 64) {
    double x[3];                                           // every residue is moved, valid or not; a NaN coordinate stays NaN
#pragma unroll
    for (int r = 0; r < 3; ++r) x[r] = rot[3 * r] * a[3 * l] + rot[3 * r + 1] * a[3 * l + 1] + rot[3 * r + 2] * a[3 * l + 2] + tr[r];
    if (valid(l)) {
      double d2 = 0;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const double e = x[r] - ref[3 * l + r];
        d2 += e * e;
      }
      acc += d2;
    }
    if (aligned)
#pragma unroll
      for (int r = 0; r < 3; ++r) aligned[(i * L + l) * 3 + r] = x[r];
  }
  acc = wave_sum(acc);
  if (lane == 0 && rmsd) rmsd[i] = sqrt(acc / cnt);
}

// flex_fit_kernel's fit and rmsd (the same statements: the same bits), the transform written out instead of the moved structure
__global__ __launch_bounds__(256) void flex_transforms_kernel(const double* __restrict__ A, const uint8_t* __restrict__ maskA,
                                                              const double* __restrict__ ref, const uint8_t* __restrict__ mask_ref,
                                                              int n, int L, double* __restrict__ T, double* __restrict__ rmsd,
                                                              uint8_t* __restrict__ ok) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;                                      // the whole wave leaves; the kernel has no barrier
  const double* a = A + i * L * 3;
  const uint8_t* ma = maskA ? maskA + i * L : nullptr;
  auto valid = [&](int l) { return (!ma || ma[l]) && (!mask_ref || mask_ref[l]); };
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  int cnt;
  double rot[9], tr[3];
  wave_fit(a, ref, L, lane, valid, cnt, rot, tr);
  if (cnt < 2) {
    if (lane < 12) T[i * 12 + lane] = nan;
    if (lane == 0 && rmsd) rmsd[i] = nan;
    if (lane == 0) ok[i] = 0;
    return;
  }
  double acc = 0;
  for (int l = lane; l < L; l += 64) {
    double x[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) x[r] = rot[3 * r] * a[3 * l] + rot[3 * r + 1] * a[3 * l + 1] + rot[3 * r + 2] * a[3 * l + 2] + tr[r];
    if (valid(l)) {
      double d2 = 0;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const double e = x[r] - ref[3 * l + r];
        d2 += e * e;
      }
      acc += d2;
    }
  }
  acc = wave_sum(acc);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 9; ++k) T[i * 12 + k] = rot[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) T[i * 12 + 9 + k] = tr[k];
    ok[i] = 1;
    if (rmsd) rmsd[i] = sqrt(acc / cnt);
  }
}

__global__ __launch_bounds__(256) void flex_moments_kernel(const double* __restrict__ X, const uint8_t* __restrict__ mask, int n, int L,
                                                           double* __restrict__ mean, double* __restrict__ msf,
                                                           int32_t* __restrict__ count) {
  const int lane = threadIdx.x & 63;
  const int l = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (l >= L) return;                                      // the whole wave leaves; the kernel has no barrier
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  auto valid = [&](int i) { return !mask || mask[(int64_t)i * L + l]; };
  double s[3] = {0, 0, 0};
  int cnt = 0;
  for (int i = lane; i < n; i += 64)
    if (valid(i)) {
      const double* x = X + ((int64_t)i * L + l) * 3;
      ++cnt;
#pragma unroll
      for (int c = 0; c < 3; ++c) s[c] += x[c];
    }
  cnt = wave_sum(cnt);
  double m[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double tot = wave_sum(s[c]);
    m[c] = cnt > 0 ? tot / cnt : nan;
  }
  double acc = 0;
  for (int i = lane; i < n; i += 64)
    if (valid(i)) {
      const double* x = X + ((int64_t)i * L + l) * 3;
      const double e0 = x[0] - m[0], e1 = x[1] - m[1], e2 = x[2] - m[2];
      acc += e0 * e0 + e1 * e1 + e2 * e2;
    }
  acc = wave_sum(acc);
  if (lane < 3) mean[3 * l + lane] = lane == 0 ? m[0] : (lane == 1 ? m[1] : m[2]);
  if (lane == 0) {
    msf[l] = cnt > 0 ? acc / cnt : nan;
    count[l] = cnt;
  }
}

}  // namespace
}  // namespace ed

using namespace ed;

extern "C" {

int esmdiff_flex_pair_msf(const double* A, int32_t n, int32_t L, const uint8_t* maskA, double* sum_sq, int64_t* count, void* scratch,
                          int64_t scratch_bytes, void* stream) {
  if (!A || !sum_sq || !count || n < 1 || L < 2) return ESMDIFF_E_INVALID;
  // 2048 workgroups wanted (8 per CU), by splitting a row pair's list into at most 16 chunks: the header's macro, by which the caller
  // sized the scratch
  const int T = (n + 1) / 2, C = ESMDIFF_FLEX_PAIR_CHUNKS(n);
  const int64_t slots = ESMDIFF_FLEX_PAIR_SLOTS(n);
  if (!scratch || scratch_bytes < slots * L * 12) return ESMDIFF_E_CAPACITY;
  double* part = (double*)scratch;                         // f64 [slots, L], then i32 [slots, L]
  int32_t* part_count = (int32_t*)(part + slots * L);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(flex_pair_msf_kernel, dim3((unsigned)T, (unsigned)C), dim3(256), 0, st, A, maskA, n, L, C, part, part_count);
  hipLaunchKernelGGL(flex_reduce_kernel, dim3((unsigned)((L + 63) / 64)), dim3(256), 0, st, part, part_count, slots, L, sum_sq, count);
  return finish_entry(st);
}

int esmdiff_flex_fit(const double* A, int32_t n, int32_t L, const uint8_t* maskA, const double* ref, const uint8_t* mask_ref,
                     double* aligned, double* rmsd, void* stream) {
  if (!A || !ref || n < 1 || L < 2) return ESMDIFF_E_INVALID;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(flex_fit_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, A, maskA, ref, mask_ref, n, L, aligned, rmsd);
  return finish_entry(st);
}

int esmdiff_flex_transforms(const double* A, int32_t n, int32_t L, const uint8_t* maskA, const double* ref, const uint8_t* mask_ref,
                            double* T, double* rmsd, uint8_t* ok, void* stream) {
  if (!A || !ref || !T || !ok || n < 1 || L < 2) return ESMDIFF_E_INVALID;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(flex_transforms_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, A, maskA, ref, mask_ref, n, L, T, rmsd, ok);
  return finish_entry(st);
}

int esmdiff_flex_moments(const double* X, int32_t n, int32_t L, const uint8_t* mask, double* mean, double* msf, int32_t* count,
                         void* stream) {
  if (!X || !mean || !msf || !count || n < 1 || L < 2) return ESMDIFF_E_INVALID;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(flex_moments_kernel, dim3((unsigned)((L + 3) / 4)), dim3(256), 0, st, X, mask, n, L, mean, msf, count);
  return finish_entry(st);
}

}  // extern "C"

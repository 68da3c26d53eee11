// superpose.hip — superposition of ensembles on CA traces, float64, on the device.
//
// What the reference's two headline evaluations compute pair by pair on the host: the Kabsch RMSD of
// /root/reference/slm/utils/geo_utils.py:58-122 (squared_deviation / _find_rigid_alignment), scipy's Rotation.align_vectors on
// sample pairs (analysis/apo_analysis.py:182-260) and one `TMscore -seq` subprocess per pair (slm/utils/tm_utils.py:46-59).
//   superpose_pairs_kernel   one WAVE per pair: the two centroids and the 3x3 covariance are wave-shuffle reductions, the 3x3
//                            decomposition runs redundantly in every lane, the lanes then write the per-residue deviations.
//   tm_pairs_kernel          one WORKGROUP per pair: both structures are compacted to their aligned residues and staged in LDS, the
//                            four waves share the fragment starts of the TM-score search, a selection is one bit per residue
//                            (bit c of lane l = residue l + 64 c), and one workgroup-level max ends it.
// The search rule is stated once in DESIGN.md ("Superposition") and restated in tests/ensemble_ref.py; [TMSCORE-RECALL]: it is
// the TMscore program's heuristic from memory, PARITY UNPINNED.
// Reductions are xor butterflies in a fixed order (every lane ends with the same bits) and nothing is accumulated with atomics:
// two runs are bit-identical, and a pair's result does not depend on which other pairs are in the launch.
#include <math.h>

#include "ed_kabsch.h"
#include "ed_wave.h"
#include "kernels.h"

namespace ed {
namespace {

constexpr int TM_MAX_L = ESMDIFF_TM_MAX_L;
constexpr int TM_MAX_LENGTHS = 12;       // La, La/2, ... > 4, then min(4, La): at most 10 entries for La <= 1280
constexpr int TM_MAX_WIDEN = 16384;      // 0.5 A steps: 8 km; only non-finite coordinates get there

__global__ __launch_bounds__(256) void superpose_pairs_kernel(const double* __restrict__ A, const double* __restrict__ B,
                                                              const uint8_t* __restrict__ maskA,
                                                              const uint8_t* __restrict__ maskB, int n, int m, int L,
                                                              int allow_reflection, double* __restrict__ rmsd,
                                                              double* __restrict__ sd, double* __restrict__ R,
                                                              double* __restrict__ t) {
  const int lane = threadIdx.x & 63;
  const int64_t pair = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pair >= (int64_t)n * m) return;                      // the whole wave leaves; the kernel has no barrier
  const int i = (int)(pair / m), j = (int)(pair % m);
  const double* a = A + (int64_t)i * L * 3;
  const double* b = B + (int64_t)j * L * 3;
  const uint8_t* ma = maskA ? maskA + (int64_t)i * L : nullptr;
  const uint8_t* mb = maskB ? maskB + (int64_t)j * L : nullptr;
  auto valid = [&](int l) { return (!ma || ma[l]) && (!mb || mb[l]); };
  const double nan = __longlong_as_double(0x7ff8000000000000LL);

  double sa[3] = {0, 0, 0}, sb[3] = {0, 0, 0};
  int cnt = 0;
  for (int l = lane; l < L; l += 64)
    if (valid(l)) {
      ++cnt;
#pragma unroll
      for (int c = 0; c < 3; ++c) sa[c] += a[3 * l + c], sb[c] += b[3 * l + c];
    }
  cnt = wave_sum(cnt);
  if (cnt < 2) {
    if (sd)
      for (int l = lane; l < L; l += 64) sd[pair * L + l] = nan;
    if (lane == 0 && rmsd) rmsd[pair] = nan;
    if (lane < 9 && R) R[pair * 9 + lane] = nan;
    if (lane < 3 && t) t[pair * 3 + lane] = nan;
    return;
  }
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
  double rot[9], tr[3];
  kabsch_rotation(h, allow_reflection, rot);
#pragma unroll
  for (int r = 0; r < 3; ++r) tr[r] = cb[r] - (rot[3 * r] * ca[0] + rot[3 * r + 1] * ca[1] + rot[3 * r + 2] * ca[2]);
  double acc = 0;
  for (int l = lane; l < L; l += 64) {
    double d2 = nan;
    if (valid(l)) {
      d2 = 0;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const double e = (rot[3 * r] * a[3 * l] + rot[3 * r + 1] * a[3 * l + 1] + rot[3 * r + 2] * a[3 * l + 2] + tr[r]) - b[3 * l + r];
        d2 += e * e;
      }
      acc += d2;
    }
    if (sd) sd[pair * L + l] = d2;
  }
  acc = wave_sum(acc);
  if (lane == 0 && rmsd) rmsd[pair] = sqrt(acc / cnt);
  if (R)
#pragma unroll
    for (int k = 0; k < 9; ++k)
      if (lane == k) R[pair * 9 + k] = rot[k];
  if (t)
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (lane == k) t[pair * 3 + k] = tr[k];
}

// Dynamic LDS: xa[3][Lp], xb[3][Lp] (coordinate-major, so that the lanes of a wave read consecutive doubles), Lp = L rounded up to 64.
__global__ __launch_bounds__(256) void tm_pairs_kernel(const double* __restrict__ A, const double* __restrict__ B,
                                                       const uint8_t* __restrict__ maskA, const uint8_t* __restrict__ maskB,
                                                       int m, int L, double* __restrict__ tm, double* __restrict__ R,
                                                       double* __restrict__ t) {
  extern __shared__ double lds[];
  __shared__ int s_cnt[TM_MAX_L / 64], s_cnt_b[TM_MAX_L / 64];
  __shared__ double s_best[4], s_rt[4][12];
  __shared__ int s_best_g[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t pair = blockIdx.x;
  const int i = (int)(pair / m), j = (int)(pair % m);
  const int Lp = (L + 63) & ~63, nchunk = Lp >> 6;
  double* xa = lds;
  double* xb = lds + 3 * Lp;
  const double* a = A + (int64_t)i * L * 3;
  const double* b = B + (int64_t)j * L * 3;
  const uint8_t* ma = maskA ? maskA + (int64_t)i * L : nullptr;
  const uint8_t* mb = maskB ? maskB + (int64_t)j * L : nullptr;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);

  // ---- compact the aligned residues (valid in both) into LDS, in residue order
  for (int c = wave; c < nchunk; c += 4) {
    const int l = 64 * c + lane;
    const bool vb = l < L && (!mb || mb[l]), va = vb && (!ma || ma[l]);
    const unsigned long long ba = __ballot(va), bb = __ballot(vb);
    if (lane == 0) s_cnt[c] = __popcll(ba), s_cnt_b[c] = __popcll(bb);
  }
  __syncthreads();
  int La = 0, Ln = 0;
  for (int c = 0; c < nchunk; ++c) La += s_cnt[c], Ln += s_cnt_b[c];
  for (int c = wave; c < nchunk; c += 4) {
    const int l = 64 * c + lane;
    const bool va = l < L && (!mb || mb[l]) && (!ma || ma[l]);
    const unsigned long long ba = __ballot(va);
    int pos = __popcll(ba & ((1ull << lane) - 1));
    for (int k = 0; k < c; ++k) pos += s_cnt[k];
    if (va)
#pragma unroll
      for (int d = 0; d < 3; ++d) xa[d * Lp + pos] = a[3 * l + d], xb[d * Lp + pos] = b[3 * l + d];
  }
  __syncthreads();
  if (La < 2) {                                            // uniform over the workgroup
    if (tid == 0) tm[pair] = nan;
    if (tid < 9 && R) R[pair * 9 + tid] = nan;
    if (tid < 3 && t) t[pair * 3 + tid] = nan;
    return;
  }
  // ---- centre both on the centroid of the aligned set (every wave computes the same bits), so that the raw moments of a
  // selection cancel little
  const int nch = (La + 63) >> 6;
  double c0a[3] = {0, 0, 0}, c0b[3] = {0, 0, 0};
  for (int c = 0; c < nch; ++c) {
    const int idx = 64 * c + lane;
    if (idx < La)
#pragma unroll
      for (int d = 0; d < 3; ++d) c0a[d] += xa[d * Lp + idx], c0b[d] += xb[d * Lp + idx];
  }
#pragma unroll
  for (int d = 0; d < 3; ++d) c0a[d] = wave_sum(c0a[d]) / La, c0b[d] = wave_sum(c0b[d]) / La;
  __syncthreads();
  for (int idx = tid; idx < La; idx += 256)
#pragma unroll
    for (int d = 0; d < 3; ++d) xa[d * Lp + idx] -= c0a[d], xb[d * Lp + idx] -= c0b[d];
  __syncthreads();

  double d0 = 1.24 * cbrt((double)Ln - 15.0) - 1.8;
  if (!(d0 >= 0.5)) d0 = 0.5;
  const double d0s = d0 < 4.5 ? 4.5 : (d0 > 8.0 ? 8.0 : d0);
  const double inv_d02 = 1.0 / (d0 * d0);
  const int need = La < 3 ? La : 3;

  int lens[TM_MAX_LENGTHS], nlen = 0;
  {
    const int lmin = La < 4 ? La : 4;
    for (int l = La; l > lmin && nlen < TM_MAX_LENGTHS - 1; l >>= 1) lens[nlen++] = l;
    lens[nlen++] = lmin;
  }

  double rot[9], tr[3];
  // one Kabsch on the residues whose bit is set; every lane ends with the same rot / tr
  auto fit = [&](unsigned bits) {
    double s[15];
#pragma unroll
    for (int k = 0; k < 15; ++k) s[k] = 0;
    for (int c = 0; c < nch; ++c)
      if ((bits >> c) & 1u) {
        const int idx = 64 * c + lane;
        const double x[3] = {xa[idx], xa[Lp + idx], xa[2 * Lp + idx]}, y[3] = {xb[idx], xb[Lp + idx], xb[2 * Lp + idx]};
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          s[d] += x[d];
          s[3 + d] += y[d];
#pragma unroll
          for (int e = 0; e < 3; ++e) s[6 + 3 * d + e] += x[d] * y[e];
        }
      }
    const int N = wave_sum((int)__popc(bits));
#pragma unroll
    for (int k = 0; k < 15; ++k) s[k] = wave_sum(s[k]);
    double h[9];
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
      for (int e = 0; e < 3; ++e) h[3 * d + e] = s[6 + 3 * d + e] - s[d] * s[3 + e] / N;
    kabsch_rotation(h, 0, rot);
#pragma unroll
    for (int d = 0; d < 3; ++d)
      tr[d] = s[3 + d] / N - (rot[3 * d] * s[0] + rot[3 * d + 1] * s[1] + rot[3 * d + 2] * s[2]) / N;
  };
  // the squared distance of aligned residue idx under (rot, tr)
  auto dist2 = [&](int idx) {
    const double x0 = xa[idx], x1 = xa[Lp + idx], x2 = xa[2 * Lp + idx];
    const double e0 = (rot[0] * x0 + rot[1] * x1 + rot[2] * x2 + tr[0]) - xb[idx];
    const double e1 = (rot[3] * x0 + rot[4] * x1 + rot[5] * x2 + tr[1]) - xb[Lp + idx];
    const double e2 = (rot[6] * x0 + rot[7] * x1 + rot[8] * x2 + tr[2]) - xb[2 * Lp + idx];
    return e0 * e0 + e1 * e1 + e2 * e2;
  };
  auto select = [&](double cut) {
    unsigned bits = 0;
    const double c2 = cut * cut;
    for (int c = 0; c < nch; ++c) {
      const int idx = 64 * c + lane;
      if (idx < La && dist2(idx) < c2) bits |= 1u << c;
    }
    return bits;
  };

  double best = -1.0, best_rot[9], best_tr[3];
  int best_g = 0x7fffffff;
#pragma unroll
  for (int k = 0; k < 9; ++k) best_rot[k] = nan;
#pragma unroll
  for (int k = 0; k < 3; ++k) best_tr[k] = nan;

  int g0 = 0;
  for (int k = 0; k < nlen; ++k) {
    const int len = lens[k], nstart = La - len + 1;
    for (int start = (wave - g0) & 3; start < nstart; start += 4) {    // the waves share the starts: g = g0 + start = wave (mod 4)
      unsigned sel = 0;
      for (int c = 0; c < nch; ++c) {
        const int idx = 64 * c + lane;
        if (idx >= start && idx < start + len) sel |= 1u << c;
      }
      for (int it = 0; it <= 20; ++it) {
        fit(sel);
        double cut = it == 0 ? d0s - 1.0 : d0s + 1.0;
        // score every aligned residue and reselect in one pass
        double sc = 0;
        unsigned nsel = 0;
        const double c2 = cut * cut;
        for (int c = 0; c < nch; ++c) {
          const int idx = 64 * c + lane;
          if (idx < La) {
            const double d2 = dist2(idx);
            sc += 1.0 / (1.0 + d2 * inv_d02);
            if (d2 < c2) nsel |= 1u << c;
          }
        }
        sc = wave_sum(sc) / Ln;
        if (sc > best) {                                   // strict: the earliest (length, start, iteration) keeps a tie
          best = sc;
          best_g = g0 + start;
#pragma unroll
          for (int q = 0; q < 9; ++q) best_rot[q] = rot[q];
#pragma unroll
          for (int q = 0; q < 3; ++q) best_tr[q] = tr[q];
        }
        int cnt = wave_sum((int)__popc(nsel));
        for (int w = 0; cnt < need && w < TM_MAX_WIDEN; ++w) {
          cut += 0.5;
          nsel = select(cut);
          cnt = wave_sum((int)__popc(nsel));
        }
        if (cnt < need) break;                             // non-finite coordinates: the seed is abandoned
        if (it > 0 && !__any(nsel != sel)) break;          // the selection did not change
        sel = nsel;
      }
    }
    g0 += nstart;
  }

  // ---- one workgroup-level max; ties go to the earliest seed, whichever wave ran it
  if (lane == 0) {
    s_best[wave] = best;
    s_best_g[wave] = best_g;
#pragma unroll
    for (int q = 0; q < 9; ++q) s_rt[wave][q] = best_rot[q];
#pragma unroll
    for (int q = 0; q < 3; ++q) s_rt[wave][9 + q] = best_tr[q];
  }
  __syncthreads();
  if (tid == 0) {
    int w = 0;
    for (int k = 1; k < 4; ++k)
      if (s_best[k] > s_best[w] || (s_best[k] == s_best[w] && s_best_g[k] < s_best_g[w])) w = k;
    tm[pair] = s_best[w] >= 0 ? s_best[w] : nan;
    const double* rt = s_rt[w];
    if (R)
      for (int q = 0; q < 9; ++q) R[pair * 9 + q] = rt[q];
    if (t)                                                 // back from the centred coordinates: t = t' - R c0a + c0b
      for (int d = 0; d < 3; ++d)
        t[pair * 3 + d] = rt[9 + d] - (rt[3 * d] * c0a[0] + rt[3 * d + 1] * c0a[1] + rt[3 * d + 2] * c0a[2]) + c0b[d];
  }
}

}  // namespace
}  // namespace ed

using namespace ed;

extern "C" {

int esmdiff_superpose_pairs(const double* A, int32_t n, const double* B, int32_t m, int32_t L, const uint8_t* maskA,
                            const uint8_t* maskB, int32_t allow_reflection, double* rmsd, double* sd, double* R, double* t,
                            void* stream) {
  if (!A || n <= 0 || L <= 0 || (B && m <= 0)) return ESMDIFF_E_INVALID;
  if (!B) B = A, m = n, maskB = maskA;
  const int64_t blocks = ((int64_t)n * m + 3) / 4;
  if (blocks > 0x7fffffff) return ESMDIFF_E_CAPACITY;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(superpose_pairs_kernel, dim3((unsigned)blocks), dim3(256), 0, st, A, B, maskA, maskB, n, m, L,
                     allow_reflection ? 1 : 0, rmsd, sd, R, t);
  return finish_entry(st);
}

int esmdiff_tm_pairs(const double* A, int32_t n, const double* B, int32_t m, int32_t L, const uint8_t* maskA,
                     const uint8_t* maskB, double* tm, double* R, double* t, void* stream) {
  if (!A || !tm || n <= 0 || L <= 0 || (B && m <= 0)) return ESMDIFF_E_INVALID;
  if (L > TM_MAX_L) return ESMDIFF_E_CAPACITY;             // both structures of a pair live in LDS; there is no slow path
  if (!B) B = A, m = n, maskB = maskA;
  const int64_t blocks = (int64_t)n * m;
  if (blocks > 0x7fffffff) return ESMDIFF_E_CAPACITY;
  hipStream_t st = (hipStream_t)stream;
  const int Lp = (L + 63) & ~63;
  hipLaunchKernelGGL(tm_pairs_kernel, dim3((unsigned)blocks), dim3(256), (size_t)6 * Lp * sizeof(double), st, A, B, maskA, maskB,
                     m, L, tm, R, t);
  return finish_entry(st);
}

}  // extern "C"

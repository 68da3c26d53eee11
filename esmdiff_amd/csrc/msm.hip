// msm.hip — the discrete side of the kinetics pipeline on the device: the nearest centre of every frame (k-means assignment), one Lloyd
// step in a single pass over the frames (assignment, cluster sizes, cluster sums and inertia), and the lagged transition counts of a
// label sequence.  float64 and integers; no float atomics: every float sum has a published order.  DESIGN.md §3.28 states the
// definitions, the orders and the tie, NaN and empty-cluster rules; tests/states_ref.py restates the three entries in numpy.
//
// DISTANCE.  Y is f64 [n, d], centres f64 [k, d], d <= ESMDIFF_LAGGED_MAX_DIM, k <= ESMDIFF_KMEANS_MAX_K.  The squared distance of a
// frame to centre j is s = 0, then s = s + (y_c - c_jc) * (y_c - c_jc) for c = 0 ... d - 1: a product, then an add (the unit is compiled
// with -ffp-contract=off).  A lane holds ONE frame's components in registers, padded with zeros to DP = 1, 2, 4, 8 or 16 (a padded
// component adds (0 - 0) * (0 - 0) = +0.0, which changes no bit of s); a wave covers 64 frames and a workgroup 256.
//
// CENTRES.  The centres pass through LDS in tiles of ESMDIFF_KMEANS_CENTRE_TILE, padded the same way: 4096 x 16 doubles do not fit.
// Every lane of a wave reads the same centre, so the LDS reads are broadcasts.  The running (minimum, index) of a lane starts as
// (+inf, -1), survives from tile to tile in registers, and centre j replaces it when s < minimum, STRICTLY: the tiles come in increasing
// j, so the label is the smallest j that attains the minimum whichever tile it is in.  A centre whose distance is not finite, because
// it or the frame has a non-finite component (s is NaN or +inf) or because the squares overflow, is never below the minimum: such a
// centre is never chosen, a frame with a non-finite component keeps -1, and so does every frame when no centre is finite.  The dist2
// of a frame labelled -1 is NaN.
//
// STEP.  The frames are cut into CHUNKS of ESMDIFF_KMEANS_FRAME_CHUNK.  A workgroup owns a chunk and one SLOT of the caller's scratch:
// sums f64 [k, d], counts i64 [k], inertia f64 [1], which it zeroes itself.  It walks the chunk 256 frames at a time: every lane assigns
// its frame and writes label, dist2 and the frame's components to LDS; then thread (g, c) of the 256 / DP groups of DP threads, which
// owns component c of the clusters j = g mod (256 / DP), reads the 256 labels IN ORDER and at every one of its clusters does
// sum[j][c] = sum[j][c] + y_tc in the slot (a load, an add, a store by the one thread that ever touches the address); thread (g, 0)
// counts, and thread 0 keeps the chunk's inertia, the same running sum over dist2 of the frames labelled >= 0.  As in lagged.hip the
// scratch holds as many slots as fit (at least one), the chunks are worked off in ROUNDS of that many, and after every round one
// kernel adds the round's slots to the outputs in increasing chunk index, starting from chunk 0's own sums: an empty cluster gives
// +0.0.  The number of slots decides how much runs at once and nothing else.
//
// TRANSITIONS.  counts[a][b] = the number of t < n - lag with labels[t] = a and labels[t + lag] = b, both >= 0.  A first kernel looks
// for a label >= k and raises a flag in the scratch, which the entry reads back BEFORE anything is written.  Integers, so integer
// atomics: while k * k i32 fit into 64 KiB of LDS (k <= ESMDIFF_TRANSITION_LDS_MAX_K) a workgroup counts its
// ESMDIFF_TRANSITION_FRAME_CHUNK values of t in a private LDS histogram and adds the non-zero cells to the output with 64-bit global
// atomics; above that every pair is one 64-bit global atomic.
#include <math.h>

#include "kernels.h"

namespace ed {
namespace {

constexpr int KM_THREADS = 256, KM_TILE = ESMDIFF_KMEANS_CENTRE_TILE;
static_assert(ESMDIFF_KMEANS_FRAME_CHUNK % KM_THREADS == 0, "a chunk is a whole number of 256-frame blocks");
static_assert(ESMDIFF_TRANSITION_LDS_MAX_K * ESMDIFF_TRANSITION_LDS_MAX_K * 4 <= 65536, "the private histogram fits the LDS of a workgroup");

// One frame's components, padded with zeros; a frame past the end is all zeros (it takes part in the barriers and writes nothing)
template <int DP>
__device__ __forceinline__ void load_frame(const double* Y, int64_t t, bool has, int d, double (&y)[DP]) {
#pragma unroll
  for (int c = 0; c < DP; ++c) y[c] = has && c < d ? Y[t * d + c] : 0.0;
}

// The nearest centre of the frame in y: every thread of the workgroup calls this (the tiles are staged by all of them)
template <int DP>
__device__ __forceinline__ void nearest(const double (&y)[DP], const double* centres, int k, int d, double* s_c, double& best, int& idx) {
  best = INFINITY, idx = -1;
  for (int j0 = 0; j0 < k; j0 += KM_TILE) {
    const int kt = k - j0 < KM_TILE ? k - j0 : KM_TILE;
    __syncthreads();                                       // every wave has read the tile before
    for (int e = threadIdx.x; e < kt * DP; e += KM_THREADS) {
      const int j = e / DP, c = e % DP;
      s_c[e] = c < d ? centres[(int64_t)(j0 + j) * d + c] : 0.0;
    }
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < kt; ++j) {
      const double* cj = s_c + j * DP;
      double s = 0.0;
#pragma unroll
      for (int c = 0; c < DP; ++c) {
        const double t = y[c] - cj[c];
        s = s + t * t;
      }
      if (s < best) best = s, idx = j0 + j;
    }
  }
}

// grid ceil(n / 256)
template <int DP>
__global__ __launch_bounds__(KM_THREADS) void kmeans_assign_kernel(const double* Y, int64_t n, int d, const double* centres, int k, int32_t* labels,
                                                                   double* dist2) {
  __shared__ double s_c[KM_TILE * DP];
  const int64_t t = (int64_t)blockIdx.x * KM_THREADS + threadIdx.x;
  const bool has = t < n;
  double y[DP], best;
  int idx;
  load_frame<DP>(Y, t, has, d, y);
  nearest<DP>(y, centres, k, d, s_c, best, idx);
  if (!has) return;
  labels[t] = idx;
  if (dist2) dist2[t] = idx < 0 ? (double)NAN : best;
}

// grid: the chunks of the round; the workgroup's slot = sums[k, d], counts[k], inertia
template <int DP>
__global__ __launch_bounds__(KM_THREADS) void kmeans_step_kernel(const double* Y, int64_t n, int d, const double* centres, int k, int64_t chunk0,
                                                                 int32_t* labels, double* slots, int64_t slot_stride) {
  __shared__ double s_c[KM_TILE * DP];
  __shared__ double s_y[KM_THREADS * DP];
  __shared__ double s_d2[KM_THREADS];
  __shared__ int s_lab[KM_THREADS];
  constexpr int G = KM_THREADS / DP;
  const int tid = threadIdx.x, g = tid / DP, c = tid % DP;
  const bool sums_mine = c < d, counts_mine = c == 0;
  const int64_t t0 = (chunk0 + blockIdx.x) * ESMDIFF_KMEANS_FRAME_CHUNK;
  const int64_t t1 = t0 + ESMDIFF_KMEANS_FRAME_CHUNK < n ? t0 + ESMDIFF_KMEANS_FRAME_CHUNK : n;
  double* sums = slots + blockIdx.x * slot_stride;
  int64_t* counts = (int64_t*)(sums + (int64_t)k * d);
  double* inertia = sums + (int64_t)k * d + k;

  // a thread zeroes the addresses it owns, and no other thread touches them before the kernel ends
  for (int j = g; j < k; j += G) {
    if (sums_mine) sums[(int64_t)j * d + c] = 0.0;
    if (counts_mine) counts[j] = 0;
  }
  double inert = 0.0;

  for (int64_t tb = t0; tb < t1; tb += KM_THREADS) {
    const int64_t t = tb + tid;
    const bool has = t < t1;
    double y[DP], best;
    int idx;
    load_frame<DP>(Y, t, has, d, y);
    nearest<DP>(y, centres, k, d, s_c, best, idx);         // (its first barrier: every thread has left the scan of the block before)
    s_lab[tid] = has ? idx : -1;
    s_d2[tid] = best;
#pragma unroll
    for (int q = 0; q < DP; ++q) s_y[tid * DP + q] = y[q];
    if (has && labels) labels[t] = idx;
    __syncthreads();

    const int frames = (int)(t1 - tb < KM_THREADS ? t1 - tb : KM_THREADS);
    for (int u = 0; u < frames; ++u) {
      const int lab = s_lab[u];
      if (lab < 0 || (lab & (G - 1)) != g) continue;
      if (sums_mine) {
        double* p = sums + (int64_t)lab * d + c;
        *p = *p + s_y[u * DP + c];
      }
      if (counts_mine) counts[lab] += 1;
    }
    if (tid == 0)
      for (int u = 0; u < frames; ++u)
        if (s_lab[u] >= 0) inert = inert + s_d2[u];
  }
  if (tid == 0) *inertia = inert;
}

// The round's slots onto the outputs, element by element: chunk 0's sums, then + chunk 1's, + chunk 2's, ...
__global__ __launch_bounds__(256) void kmeans_add_kernel(const double* slots, int64_t slot_stride, int used, int first_round, int64_t kd, int k,
                                                         double* sums, int64_t* counts, double* inertia) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= kd + k + 1) return;
  if (e >= kd && e < kd + k) {
    const int64_t* src = (const int64_t*)slots + e;
    int64_t v = first_round ? 0 : counts[e - kd];
    for (int s = 0; s < used; ++s) v += src[s * slot_stride];
    counts[e - kd] = v;
    return;
  }
  double* dst = e < kd ? sums + e : inertia;
  const double* src = slots + e;
  double v = first_round ? src[0] : *dst;
  for (int s = first_round ? 1 : 0; s < used; ++s) v = v + src[s * slot_stride];
  *dst = v;
}

// n = 0: no chunk; the sums of nothing
__global__ __launch_bounds__(256) void kmeans_zero_kernel(int64_t kd, int k, double* sums, int64_t* counts, double* inertia) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < kd) sums[e] = 0.0;
  else if (e < kd + k) counts[e - kd] = 0;
  else if (e == kd + k) *inertia = 0.0;
}

int padded_dim(int d) { return d <= 1 ? 1 : d <= 2 ? 2 : d <= 4 ? 4 : d <= 8 ? 8 : 16; }

void launch_assign(int dp, dim3 grid, hipStream_t st, const double* Y, int64_t n, int d, const double* centres, int k, int32_t* labels, double* dist2) {
#define ED_KM_ASSIGN(DP) hipLaunchKernelGGL(kmeans_assign_kernel<DP>, grid, dim3(KM_THREADS), 0, st, Y, n, d, centres, k, labels, dist2)
  switch (dp) {
    case 1: ED_KM_ASSIGN(1); break;
    case 2: ED_KM_ASSIGN(2); break;
    case 4: ED_KM_ASSIGN(4); break;
    case 8: ED_KM_ASSIGN(8); break;
    default: ED_KM_ASSIGN(16); break;
  }
#undef ED_KM_ASSIGN
}

void launch_step(int dp, dim3 grid, hipStream_t st, const double* Y, int64_t n, int d, const double* centres, int k, int64_t chunk0, int32_t* labels,
                 double* slots, int64_t slot_stride) {
#define ED_KM_STEP(DP) \
  hipLaunchKernelGGL(kmeans_step_kernel<DP>, grid, dim3(KM_THREADS), 0, st, Y, n, d, centres, k, chunk0, labels, slots, slot_stride)
  switch (dp) {
    case 1: ED_KM_STEP(1); break;
    case 2: ED_KM_STEP(2); break;
    case 4: ED_KM_STEP(4); break;
    case 8: ED_KM_STEP(8); break;
    default: ED_KM_STEP(16); break;
  }
#undef ED_KM_STEP
}

// flag[0] = 1 when a label is >= k
__global__ __launch_bounds__(256) void transition_check_kernel(const int32_t* labels, int64_t n, int k, int32_t* flag) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  bool bad = false;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += stride) bad = bad || labels[t] >= k;
  if (bad) flag[0] = 1;
}

// grid: the chunks of m = n - lag values of t; k <= ESMDIFF_TRANSITION_LDS_MAX_K
__global__ __launch_bounds__(256) void transition_lds_kernel(const int32_t* labels, int64_t m, int lag, int k, unsigned long long* counts) {
  __shared__ unsigned int s_hist[ESMDIFF_TRANSITION_LDS_MAX_K * ESMDIFF_TRANSITION_LDS_MAX_K];
  const int cells = k * k;
  for (int e = threadIdx.x; e < cells; e += 256) s_hist[e] = 0u;
  __syncthreads();
  const int64_t t0 = (int64_t)blockIdx.x * ESMDIFF_TRANSITION_FRAME_CHUNK;
  const int64_t t1 = t0 + ESMDIFF_TRANSITION_FRAME_CHUNK < m ? t0 + ESMDIFF_TRANSITION_FRAME_CHUNK : m;
  for (int64_t t = t0 + threadIdx.x; t < t1; t += 256) {
    const int a = labels[t], b = labels[t + lag];
    if (a >= 0 && b >= 0) atomicAdd(&s_hist[a * k + b], 1u);
  }
  __syncthreads();
  for (int e = threadIdx.x; e < cells; e += 256) {
    const unsigned int v = s_hist[e];
    if (v) atomicAdd(&counts[e], (unsigned long long)v);
  }
}

// grid: the same chunks; every pair one global atomic
__global__ __launch_bounds__(256) void transition_global_kernel(const int32_t* labels, int64_t m, int lag, int k, unsigned long long* counts) {
  const int64_t t0 = (int64_t)blockIdx.x * ESMDIFF_TRANSITION_FRAME_CHUNK;
  const int64_t t1 = t0 + ESMDIFF_TRANSITION_FRAME_CHUNK < m ? t0 + ESMDIFF_TRANSITION_FRAME_CHUNK : m;
  for (int64_t t = t0 + threadIdx.x; t < t1; t += 256) {
    const int a = labels[t], b = labels[t + lag];
    if (a >= 0 && b >= 0) atomicAdd(&counts[(int64_t)a * k + b], 1ull);
  }
}

}  // namespace
}  // namespace ed

using namespace ed;

extern "C" {

int esmdiff_kmeans_assign(const double* Y, int32_t n, int32_t d, const double* centres, int32_t k, int32_t* labels, double* dist2, void* stream) {
  if (n < 0 || d < 1 || k < 1 || !centres || (n > 0 && (!Y || !labels))) return ESMDIFF_E_INVALID;
  if (d > ESMDIFF_LAGGED_MAX_DIM || k > ESMDIFF_KMEANS_MAX_K) return ESMDIFF_E_CAPACITY;
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) return finish_entry(st);
  launch_assign(padded_dim(d), dim3((unsigned)(((int64_t)n + KM_THREADS - 1) / KM_THREADS)), st, Y, n, d, centres, k, labels, dist2);
  return finish_entry(st);
}

int esmdiff_kmeans_step(const double* Y, int32_t n, int32_t d, const double* centres, int32_t k, int32_t* labels, int64_t* counts, double* sums,
                        double* inertia, void* scratch, int64_t scratch_bytes, void* stream) {
  if (n < 0 || d < 1 || k < 1 || !centres || !counts || !sums || !inertia || !scratch || (n > 0 && !Y)) return ESMDIFF_E_INVALID;
  if (d > ESMDIFF_LAGGED_MAX_DIM || k > ESMDIFF_KMEANS_MAX_K) return ESMDIFF_E_CAPACITY;
  if (scratch_bytes < ESMDIFF_KMEANS_STEP_SCRATCH_BYTES(k, d, 1)) return ESMDIFF_E_CAPACITY;
  const int64_t kd = (int64_t)k * d, slot = kd + k + 1;
  const int64_t room = scratch_bytes / (slot * 8);
  const int64_t chunks = ESMDIFF_KMEANS_CHUNKS(n);
  hipStream_t st = (hipStream_t)stream;
  const dim3 cells((unsigned)((slot + 255) / 256));
  if (chunks == 0) hipLaunchKernelGGL(kmeans_zero_kernel, cells, dim3(256), 0, st, kd, (int)k, sums, counts, inertia);
  for (int64_t c0 = 0; c0 < chunks; c0 += room) {
    const int used = (int)(chunks - c0 < room ? chunks - c0 : room);
    launch_step(padded_dim(d), dim3((unsigned)used), st, Y, n, d, centres, k, c0, labels, (double*)scratch, slot);
    hipLaunchKernelGGL(kmeans_add_kernel, cells, dim3(256), 0, st, (const double*)scratch, slot, used, (int)(c0 == 0), kd, (int)k, sums, counts,
                       inertia);
  }
  return finish_entry(st);
}

int esmdiff_transition_counts(const int32_t* labels, int32_t n, int32_t k, int32_t lag, int64_t* counts, void* scratch, int64_t scratch_bytes,
                              void* stream) {
  if (n < 0 || k < 1 || lag < 1 || !counts || !scratch || (n > 0 && !labels)) return ESMDIFF_E_INVALID;
  if (k > ESMDIFF_KMEANS_MAX_K || scratch_bytes < ESMDIFF_TRANSITION_SCRATCH_BYTES) return ESMDIFF_E_CAPACITY;
  hipStream_t st = (hipStream_t)stream;
  int32_t* flag = (int32_t*)scratch;
  int32_t bad = 0;
  if (n > 0) {
    if (hipMemsetAsync(flag, 0, ESMDIFF_TRANSITION_SCRATCH_BYTES, st) != hipSuccess) return ESMDIFF_E_HIP;
    int64_t blocks = ((int64_t)n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(transition_check_kernel, dim3((unsigned)blocks), dim3(256), 0, st, labels, (int64_t)n, (int)k, flag);
    if (hipMemcpyAsync(&bad, flag, sizeof(bad), hipMemcpyDeviceToHost, st) != hipSuccess) return ESMDIFF_E_HIP;
    if (hipStreamSynchronize(st) != hipSuccess) return ESMDIFF_E_HIP;
    if (bad) return ESMDIFF_E_INVALID;
  }
  if (hipMemsetAsync(counts, 0, (size_t)k * k * 8, st) != hipSuccess) return ESMDIFF_E_HIP;
  const int64_t m = (int64_t)n - lag;
  if (m > 0) {
    const dim3 grid((unsigned)((m + ESMDIFF_TRANSITION_FRAME_CHUNK - 1) / ESMDIFF_TRANSITION_FRAME_CHUNK));
    if (k <= ESMDIFF_TRANSITION_LDS_MAX_K)
      hipLaunchKernelGGL(transition_lds_kernel, grid, dim3(256), 0, st, labels, m, (int)lag, (int)k, (unsigned long long*)counts);
    else
      hipLaunchKernelGGL(transition_global_kernel, grid, dim3(256), 0, st, labels, m, (int)lag, (int)k, (unsigned long long*)counts);
  }
  return finish_entry(st);
}

}  // extern "C"

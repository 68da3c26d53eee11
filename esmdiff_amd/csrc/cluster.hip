// cluster.hip — GROMOS clustering (Daura et al. 1999; the `gromos` method of `gmx cluster`) of an ensemble on the device.
//
// The neighbour relation is a bit matrix adj u64 [n, W], W = ceil(n / 64): bit (j & 63) of adj[i, j >> 6] says "i and j are
// neighbours"; the padding bits of a row's last word are zero.  DESIGN.md ("Clustering") states the algorithm and the neighbour rule,
// tests/cluster_ref.py restates both on the host in the naive form.
//   cluster_threshold_kernel   one WAVE per (row, word): lane l tests column 64 w + l of a block of matrix rows, one ballot is
//                              the word.  Only words that reach the diagonal or lie above it are touched.
//   cluster_symmetrize_kernel  one WAVE per 64 x 64 tile on or above the diagonal: the tile is transposed with 64 ballots and
//                              stored below the diagonal, over whatever was there.
//   cluster_gromos_kernel      ONE persistent workgroup of 16 waves runs the whole loop.  The neighbour counts of all n structures
//                              (int32, dynamic LDS), the alive mask and the member mask of the cluster being formed (u64 [W] each)
//                              live in LDS.  The counts are popcounts of the rows, taken once; when a structure leaves, one wave
//                              reads its row once and takes one off the count of every neighbour that stays (integer LDS atomics:
//                              the order does not matter).  A structure that has left has count 0, so the arg-max of a cluster is a
//                              plain max reduction of (count << 32) | (0xFFFFFFFF - index): most neighbours first, lowest index
//                              on a tie.  Total: every row is read twice (O(n^2 / 64) words) plus one O(n) arg-max per cluster.
// Integers only: the result is a pure function of adj's upper triangle.
#include "kernels.h"

namespace ed {
namespace {

constexpr int CLUSTER_MAX_W = ESMDIFF_CLUSTER_MAX_N / 64;
constexpr int LOOP_THREADS = 1024, LOOP_WAVES = LOOP_THREADS / 64;
static_assert(CLUSTER_MAX_W <= LOOP_THREADS, "one thread per word forms the member mask");

typedef unsigned long long u64;

__global__ __launch_bounds__(256) void cluster_threshold_kernel(const double* __restrict__ d, int rows, int row0, int n, int W,
                                                                double cutoff, int larger_is_closer, u64* __restrict__ adj) {
  const int lane = threadIdx.x & 63;
  const int64_t unit = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (unit >= (int64_t)rows * W) return;                   // the whole wave leaves; the kernel has no barrier
  const int r = (int)(unit / W), w = (int)(unit % W);
  const int i = row0 + r, j = 64 * w + lane;
  if (64 * w + 63 < i) return;                             // a word wholly below the diagonal: row j's block decides those pairs
  bool nb = false;
  if (j < n && j > i) {
    const double v = d[(int64_t)r * n + j];                // NaN compares false: not neighbours
    nb = larger_is_closer ? v >= cutoff : v <= cutoff;
  }
  nb |= j == i;
  const u64 bits = __ballot(nb);
  if (lane == 0 && bits) adj[(int64_t)i * W + w] |= bits;  // this wave is the only writer of the word
}

// grid (W, W): tile (I = blockIdx.y, J = blockIdx.x), I <= J
__global__ __launch_bounds__(64) void cluster_symmetrize_kernel(u64* __restrict__ adj, int n, int W) {
  const int I = blockIdx.y, J = blockIdx.x, lane = threadIdx.x;
  if (J < I) return;
  const int row = 64 * I + lane;
  u64 r = row < n ? adj[(int64_t)row * W + J] : 0;
  const int cols = n - 64 * J;
  if (cols < 64) r &= (1ull << cols) - 1;                  // padding bits are not trusted either
  if (I == J) {
    r &= ~0ull << lane;                                    // below the diagonal: ignored
    if (row < n) r |= 1ull << lane;
  }
  u64 tr = 0;                                              // lane b: bit k = bit b of lane k's word
  for (int b = 0; b < 64; ++b) {
    const u64 col = __ballot((r >> b) & 1);
    if (lane == b) tr = col;
  }
  if (I == J) {
    if (row < n) adj[(int64_t)row * W + J] = r | tr;
  } else {
    if (row < n) adj[(int64_t)row * W + J] = r;
    const int trow = 64 * J + lane;
    if (trow < n) adj[(int64_t)trow * W + I] = tr;
  }
}

__device__ __forceinline__ u64 wave_max(u64 v, int from) {
  for (int off = from; off >= 1; off >>= 1) {
    const u64 o = __shfl_xor(v, off, 64);
    v = o > v ? o : v;
  }
  return v;
}

// Dynamic LDS: counts int32 [n].
__global__ __launch_bounds__(LOOP_THREADS) void cluster_gromos_kernel(const u64* __restrict__ adj, int n, int W,
                                                                      int32_t* __restrict__ labels, int32_t* __restrict__ centres,
                                                                      int32_t* __restrict__ sizes, int32_t* __restrict__ n_clusters) {
  extern __shared__ int counts[];
  __shared__ u64 s_alive[CLUSTER_MAX_W], s_member[CLUSTER_MAX_W], s_key[LOOP_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  if (tid < W) {
    const int left = n - 64 * tid;
    s_alive[tid] = left >= 64 ? ~0ull : (1ull << left) - 1;
  }
  for (int i = wave; i < n; i += LOOP_WAVES) {
    int c = 0;
    for (int w = lane; w < W; w += 64) c += __popcll(adj[(int64_t)i * W + w]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off, 64);
    if (lane == 0) counts[i] = c;
  }
  __syncthreads();

  int k = 0;
  for (int remaining = n; remaining > 0 && k < n; ++k) {
    // ---- the structure with the most neighbours left; a structure that has left has count 0 and key 0
    u64 key = 0;
    for (int i = tid; i < n; i += LOOP_THREADS) {
      const unsigned c = (unsigned)counts[i];
      const u64 ki = ((u64)c << 32) | (0xFFFFFFFFu - (unsigned)i);
      if (c && ki > key) key = ki;
    }
    key = wave_max(key, 32);
    if (lane == 0) s_key[wave] = key;
    __syncthreads();
    key = wave_max(s_key[lane & (LOOP_WAVES - 1)], LOOP_WAVES / 2);
    if (key == 0) break;                                   // uniform; cannot happen while a structure is left (its own bit counts)
    const int centre = (int)(0xFFFFFFFFu - (unsigned)key), size = (int)(key >> 32);
    // ---- the cluster: the centre's neighbours that are left
    if (tid < W) {
      const u64 m = adj[(int64_t)centre * W + tid] & s_alive[tid];
      s_member[tid] = m;
      s_alive[tid] &= ~m;
    }
    if (tid == 0) centres[k] = centre, sizes[k] = size;
    __syncthreads();
    // ---- every member leaves: one wave reads its row once, the neighbours that stay lose one
    for (int w = wave; w < W; w += LOOP_WAVES) {
      u64 m = s_member[w];                                 // the same word in every lane
      while (m) {
        const int j = 64 * w + __builtin_ctzll(m);
        m &= m - 1;
        if (lane == 0) labels[j] = k, counts[j] = 0;       // j is not alive any more: no wave decrements counts[j]
        for (int x = lane; x < W; x += 64) {
          u64 a = adj[(int64_t)j * W + x] & s_alive[x];
          while (a) {
            atomicSub(&counts[64 * x + __builtin_ctzll(a)], 1);
            a &= a - 1;
          }
        }
      }
    }
    __syncthreads();
    remaining -= size;
  }
  if (tid == 0) *n_clusters = k;
}

}  // namespace
}  // namespace ed

using namespace ed;

extern "C" {

int esmdiff_cluster_threshold(const double* d, int32_t rows, int32_t row0, int32_t n, double cutoff, int32_t larger_is_closer,
                              uint64_t* adj, void* stream) {
  if (!d || !adj || n < 1 || rows < 1 || row0 < 0) return ESMDIFF_E_INVALID;
  if (n > ESMDIFF_CLUSTER_MAX_N) return ESMDIFF_E_CAPACITY;
  if ((int64_t)row0 + rows > n) return ESMDIFF_E_INVALID;
  const int W = (n + 63) / 64;
  const int64_t blocks = ((int64_t)rows * W + 3) / 4;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(cluster_threshold_kernel, dim3((unsigned)blocks), dim3(256), 0, st, d, rows, row0, n, W, cutoff,
                     larger_is_closer ? 1 : 0, (u64*)adj);
  return finish_entry(st);
}

int esmdiff_cluster_gromos(uint64_t* adj, int32_t n, int32_t* labels, int32_t* centres, int32_t* sizes, int32_t* n_clusters,
                           void* stream) {
  if (!adj || !labels || !centres || !sizes || !n_clusters || n < 1) return ESMDIFF_E_INVALID;
  if (n > ESMDIFF_CLUSTER_MAX_N) return ESMDIFF_E_CAPACITY;
  const int W = (n + 63) / 64;
  const int lds = n * (int)sizeof(int32_t);
  if (ensure_dynamic_lds((const void*)cluster_gromos_kernel, lds) != hipSuccess) return ESMDIFF_E_HIP;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(cluster_symmetrize_kernel, dim3(W, W), dim3(64), 0, st, (u64*)adj, n, W);
  if (hipGetLastError() != hipSuccess) return ESMDIFF_E_HIP;
  hipLaunchKernelGGL(cluster_gromos_kernel, dim3(1), dim3(LOOP_THREADS), (size_t)lds, st, (const u64*)adj, n, W, labels, centres,
                     sizes, n_clusters);
  return finish_entry(st);
}

}  // extern "C"

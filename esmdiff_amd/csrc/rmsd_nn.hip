// rmsd_nn.hip — nearest neighbours between two ensembles under the least-squares RMSD, without a rotation and without an (n, m)
// matrix.  float64 throughout; the hot loop is the f64 MFMA v_mfma_f64_16x16x4_f64.  DESIGN.md §3.30 states the definition and the
// order of every sum; tests/neighbours_ref.py restates both entries in numpy.
//
// DEFINITION.  Both sides centred on ONE residue set of N residues:  msd(i, j) = max(0, ((G_a[i] + G_b[j]) - 2 S) / N) with
// G = sum |x - c|^2, s1 >= s2 >= s3 the singular values of H_ij = sum_l a_il b_jl^T and S = (s1 + s2) + sigma s3; sigma = -1 when
// proper rotations are asked for and det H_ij < 0, else +1.
//
// PREPARE.  A wave owns a frame.  Lane l walks the residues l, l + 64, ... in increasing order and adds the selected ones: s = +0.0,
// then s = s + x; then s_l = s_l + s_{l ^ d} for d = 32, 16, 8, 4, 2, 1, after which every lane holds the same bits.  c = s / N.  G is
// the same walk and tree over ((dx dx + dy dy) + dz dz) with d = x - c (no FMA: the unit is compiled with -ffp-contract=off).  P is
// the centred, compacted copy: P[t][comp][k] with k the rank of the residue among the selected, the row zero-padded to
// K = ESMDIFF_RMSD_NN_PADDED(N) (a multiple of 4), so a frame is 3 K consecutive doubles.  A frame with a non-finite selected
// coordinate, or whose G is not finite, gets use = 0, a P row of zeros and info = 0.
//
// NEAREST.  The (n, m) pairs are cut into RECTANGLES of RECT x RECT frames, numbered row-major (B == NULL: only rectangles on and
// above the diagonal, and in them only pairs i < j, each feeding both of its frames).  A workgroup of four waves owns a rectangle and
// walks its TILE x TILE tiles, row tile major; a wave owns a 16 x 16 block of a tile with NINE accumulators, one per entry (r, c) of H.
// The operands are staged through LDS in slabs of NN_KS residues as [16-frame block][comp][4 residues][frame 16], so that the 64 lanes
// of a wave read 64 consecutive doubles as an MFMA operand: lane l holds A[i = l & 15][k = l >> 4].  Per four residues a wave reads
// three A and three B operands and issues nine instructions.  C/D of the f64 MFMA: col = lane & 15, row = (lane >> 4) + 4 reg, so a
// lane ends with all nine entries of H for each of its four pairs and takes their singular values alone: the column norms of the
// one-sided Jacobi of ed_kabsch.h (its V is never read and the compiler drops it).  det H is the triple product of the rotated,
// mutually orthogonal columns (V is a product of rotations: det G = det H), whose sign is safe down to the rounding of s1 s2 s3.
// A frame with use == 0, a frame past the end and a residue past K are staged as zeros without being read.
//
// PARTIALS.  A tile's msd go to LDS; one thread per row walks its 32 columns in increasing j, one thread per column its 32 rows in
// increasing i, into the rectangle's partial (min msd, its index by strict <, sum of sqrt(msd), pairs, counts per cutoff) per row and
// per column.  The rectangle's partials go to a SLOT of the scratch; the scratch holds as many slots as fit, the rectangles are worked
// off in ROUNDS of that many, and after every round one kernel folds the round's slots into the per-frame state in increasing
// rectangle number: for a row that is increasing j, for a column increasing i, and for B == NULL a frame's column partials (j < i)
// come before its row partials (j > i), increasing j again.  The number of slots decides how much runs at once and nothing else.
// Pairs with an unused frame are skipped: they add nothing, not even +0.0.  No float atomics; the histogram is integer atomics.
#include <math.h>

#include "kernels.h"
#include "ed_kabsch.h"

namespace ed {
namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int NN_TILE = ESMDIFF_RMSD_NN_TILE, NN_RECT = ESMDIFF_RMSD_NN_RECT, NN_TILES = NN_RECT / NN_TILE;
constexpr int NN_KS = 16, NN_THREADS = 256, NN_T = ESMDIFF_RMSD_NN_MAX_CUTOFFS, NN_BINS = ESMDIFF_RMSD_NN_MAX_BINS;
constexpr int NN_SIDE = NN_TILE * 3 * NN_KS;               // one staged side of a slab, in doubles
static_assert(NN_TILE == 32 && NN_RECT % NN_TILE == 0, "a tile is 2 x 2 MFMA blocks, a rectangle a whole number of tiles");

struct NnPartial {                                         // one row or column of one rectangle
  double min, sum;
  int32_t arg, pairs;
  uint32_t count[NN_T];
};
struct NnState {                                           // one frame, across rectangles
  double min, sum;
  int64_t pairs;
  int64_t count[NN_T];
  int32_t arg, pad;
};
static_assert(sizeof(NnPartial) * 2 * NN_RECT == ESMDIFF_RMSD_NN_SLOT_BYTES, "the header's slot size");
static_assert(sizeof(NnState) == ESMDIFF_RMSD_NN_STATE_BYTES, "the header's state size");

struct NnArgs {
  const double *PA, *infoA, *PB, *infoB;
  const uint8_t *useA, *useB;
  int32_t n, m, N, K, self, reflect, T, bins;
  double cut[NN_T];
  double width;
  int64_t* hist;
  double *msd, *cross;
  NnPartial* slots;
  int64_t blocksB;                                         // rectangles to a row of rectangles
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v = v + __shfl_xor(v, s, 64);
  return v;
}

// grid ceil(n / 4): a wave owns a frame
__global__ __launch_bounds__(256) void rmsd_prepare_kernel(const double* __restrict__ X, int32_t n, int32_t L, const uint8_t* __restrict__ sel,
                                                           int32_t N, double* __restrict__ P, double* __restrict__ info,
                                                           uint8_t* __restrict__ use) {
  const int lane = threadIdx.x & 63;
  const int64_t t = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (t >= n) return;
  const int K = ESMDIFF_RMSD_NN_PADDED(N);
  const double* frame = X + t * L * 3;
  double* row = P + t * 3 * K;
  double sx = 0.0, sy = 0.0, sz = 0.0;
  bool bad = false;
  for (int base = 0; base < L; base += 64) {
    const int l = base + lane;
    if (l < L && (!sel || sel[l])) {
      const double x = frame[3 * l], y = frame[3 * l + 1], z = frame[3 * l + 2];
      bad |= !(isfinite(x) && isfinite(y) && isfinite(z));
      sx = sx + x, sy = sy + y, sz = sz + z;
    }
  }
  bool dead = __any(bad);
  double G = 0.0, cx = 0.0, cy = 0.0, cz = 0.0;
  if (!dead) {
    cx = wave_sum(sx) / (double)N, cy = wave_sum(sy) / (double)N, cz = wave_sum(sz) / (double)N;
    double g = 0.0;
    int before = 0;
    for (int base = 0; base < L; base += 64) {
      const int l = base + lane;
      const bool on = l < L && (!sel || sel[l]);
      const unsigned long long mask = __ballot(on);
      if (on) {
        const int k = before + __popcll(mask & ((1ull << lane) - 1));
        const double dx = frame[3 * l] - cx, dy = frame[3 * l + 1] - cy, dz = frame[3 * l + 2] - cz;
        g = g + ((dx * dx + dy * dy) + dz * dz);
        if (k < N) row[k] = dx, row[K + k] = dy, row[2 * K + k] = dz;
      }
      before += __popcll(mask);
    }
    G = wave_sum(g);
    dead = !isfinite(G);
  }
  if (dead) {
    for (int k = lane; k < 3 * K; k += 64) row[k] = 0.0;
    G = cx = cy = cz = 0.0;
  } else if (lane < K - N) {
    row[N + lane] = 0.0, row[K + N + lane] = 0.0, row[2 * K + N + lane] = 0.0;
  }
  if (lane == 0) {
    info[t * 4] = cx, info[t * 4 + 1] = cy, info[t * 4 + 2] = cz, info[t * 4 + 3] = G;
    use[t] = dead ? 0 : 1;
  }
}

// (s1 + s2) + sigma s3 of the 3 x 3 h
__device__ __forceinline__ double sv_sum(const double* h, int reflect) {
  double g[9], v[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
#pragma unroll
  for (int i = 0; i < 9; ++i) g[i] = h[i];
  for (int sweep = 0; sweep < 30; ++sweep) {
    bool any = jacobi_rotate<0, 1>(g, v);
    any |= jacobi_rotate<0, 2>(g, v);
    any |= jacobi_rotate<1, 2>(g, v);
    if (!any) break;
  }
  const double a = sqrt(g[0] * g[0] + g[3] * g[3] + g[6] * g[6]);
  const double b = sqrt(g[1] * g[1] + g[4] * g[4] + g[7] * g[7]);
  const double c = sqrt(g[2] * g[2] + g[5] * g[5] + g[8] * g[8]);
  const double hi = fmax(a, fmax(b, c)), lo = fmin(a, fmin(b, c));
  const double mid = fmax(fmin(a, b), fmin(fmax(a, b), c));
  double sigma = 1.0;
  if (!reflect) {
    const double det = g[0] * (g[4] * g[8] - g[5] * g[7]) - g[1] * (g[3] * g[8] - g[5] * g[6]) + g[2] * (g[3] * g[7] - g[4] * g[6]);
    if (det < 0) sigma = -1.0;
  }
  return (hi + mid) + sigma * lo;
}

__device__ __forceinline__ void nn_rectangle(const NnArgs& a, int64_t q, int64_t* R, int64_t* C) {
  if (!a.self) {
    *R = q / a.blocksB, *C = q - *R * a.blocksB;
    return;
  }
  int64_t I = 0, rest = q;
  while (rest >= a.blocksB - I) rest -= a.blocksB - I, ++I;
  *R = I, *C = I + rest;
}

__device__ __forceinline__ void partial_take(NnPartial& p, double msd, int index, const NnArgs& a) {
  const double r = sqrt(msd);
  if (msd < p.min) p.min = msd, p.arg = index;
  p.sum = p.sum + r;
  p.pairs += 1;
#pragma unroll
  for (int t = 0; t < NN_T; ++t) p.count[t] += (t < a.T && r <= a.cut[t]) ? 1u : 0u;
}

// grid (rectangles of the round): the rectangle q0 + blockIdx.x -> slot blockIdx.x
// (two waves a SIMD: 55 KiB of LDS lets two workgroups share a CU, so the register budget is 256)
__global__ __launch_bounds__(NN_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void rmsd_nearest_kernel(const NnArgs a, int64_t q0) {
  __shared__ double s_op[2 * NN_SIDE];                     // the slab of the row side, then of the column side: 24 KiB
  __shared__ double s_msd[NN_TILE][NN_TILE + 1];
  __shared__ NnPartial s_part[2 * NN_RECT];                // rows, then columns
  __shared__ unsigned int s_hist[NN_BINS];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 1, wc = wave & 1;
  int64_t R, C;
  nn_rectangle(a, q0 + blockIdx.x, &R, &C);
  const bool diag_rect = a.self && R == C;
  const double* PB = a.self ? a.PA : a.PB;
  const double* infoB = a.self ? a.infoA : a.infoB;
  const uint8_t* useB = a.self ? a.useA : a.useB;
  const int m = a.self ? a.n : a.m;

  for (int e = tid; e < 2 * NN_RECT; e += NN_THREADS) {
    NnPartial p;
    p.min = INFINITY, p.sum = 0.0, p.arg = -1, p.pairs = 0;
#pragma unroll
    for (int t = 0; t < NN_T; ++t) p.count[t] = 0;
    s_part[e] = p;
  }
  if (a.hist)
    for (int e = tid; e < a.bins; e += NN_THREADS) s_hist[e] = 0;
  __syncthreads();

  const int K = a.K;
  const int64_t fs = 3 * (int64_t)K;                       // a frame of P
  for (int tr = 0; tr < NN_TILES; ++tr) {
    const int64_t row0 = R * NN_RECT + tr * NN_TILE;
    if (row0 >= a.n) break;
    for (int tc = diag_rect ? tr : 0; tc < NN_TILES; ++tc) {
      const int64_t col0 = C * NN_RECT + tc * NN_TILE;
      if (col0 >= m) break;
      const bool diag = diag_rect && tr == tc;
      const bool idle = diag && wr > wc;                   // wave-uniform: every pair of the block has i >= j

      f64x4 acc[9];
#pragma unroll
      for (int e = 0; e < 9; ++e) acc[e] = f64x4{0.0, 0.0, 0.0, 0.0};
      for (int k0 = 0; k0 < K; k0 += NN_KS) {
        __syncthreads();                                   // every wave has read the last slab, and the last tile's msd
#pragma unroll
        for (int rep = 0; rep < 2 * NN_SIDE / NN_THREADS; ++rep) {
          const int e = tid + rep * NN_THREADS;
          const int side = e >= NN_SIDE, o = e - side * NN_SIDE;
          const int k = o & (NN_KS - 1), fc = o >> 4, f = fc / 3, comp = fc - 3 * f;
          const int64_t t = (side ? col0 : row0) + f;
          const bool on = t < (side ? m : a.n) && k0 + k < K && (side ? useB : a.useA)[t];
          const double v = on ? (side ? PB : a.PA)[t * fs + comp * K + k0 + k] : 0.0;
          s_op[side * NN_SIDE + ((((f >> 4) * 3 + comp) * (NN_KS / 4) + (k >> 2)) * 4 + (k & 3)) * 16 + (f & 15)] = v;
        }
        __syncthreads();
        if (idle) continue;
#pragma unroll
        for (int kk = 0; kk < NN_KS / 4; ++kk) {
          if (k0 + 4 * kk >= K) break;
          double fa[3], fb[3];
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            fa[c] = s_op[((wr * 3 + c) * (NN_KS / 4) + kk) * 64 + lane];
            fb[c] = s_op[NN_SIDE + ((wc * 3 + c) * (NN_KS / 4) + kk) * 64 + lane];
          }
#pragma unroll
          for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[3 * r + c] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[r], fb[c], acc[3 * r + c], 0, 0, 0);
        }
      }

      // the lane's four pairs: row (lane >> 4) + 4 reg, column lane & 15 of the wave's block
      const int lj = wc * 16 + (lane & 15);
      const int64_t j = col0 + lj;
      const bool j_on = j < m && useB[j];
      const double Gb = j_on ? infoB[j * 4 + 3] : 0.0;
#pragma unroll 1                                         // ONE copy of the Jacobi: the registers of four would cost a wave per SIMD
      for (int reg = 0; reg < 4; ++reg) {
        const int li = wr * 16 + (lane >> 4) + 4 * reg;
        const int64_t i = row0 + li;
        double msd = -1.0;                                 // no pair
        if (!idle && i < a.n && j < m) {
          double h[9];
#pragma unroll
          for (int e = 0; e < 9; ++e) h[e] = reg == 0 ? acc[e][0] : reg == 1 ? acc[e][1] : reg == 2 ? acc[e][2] : acc[e][3];
          if (a.cross) {
            double* dst = a.cross + (i * m + j) * 9;
#pragma unroll
            for (int e = 0; e < 9; ++e) dst[e] = h[e];
            if (a.self && i != j) {                        // (a diagonal tile computes both: the same bits twice)
              double* mirror = a.cross + (j * m + i) * 9;
#pragma unroll
              for (int e = 0; e < 9; ++e) mirror[e] = h[3 * (e % 3) + e / 3];
            }
          }
          const bool pair = j_on && a.useA[i] && (!a.self || i < j);
          if (pair) {
            const double S = sv_sum(h, a.reflect);
            const double v = ((a.infoA[i * 4 + 3] + Gb) - 2.0 * S) / (double)a.N;
            msd = v > 0.0 ? v : 0.0;
            if (a.hist) {
              const double b = sqrt(msd) / a.width;
              atomicAdd(&s_hist[b >= (double)a.bins ? a.bins - 1 : (int)b], 1u);
            }
          }
          if (a.msd) {
            if (!a.self) {
              a.msd[i * m + j] = pair ? msd : NAN;
            } else if (i < j) {
              a.msd[i * m + j] = a.msd[j * m + i] = pair ? msd : NAN;
            } else if (i == j) {
              a.msd[i * m + j] = a.useA[i] ? 0.0 : NAN;
            }
          }
        }
        s_msd[li][lj] = msd;
      }
      __syncthreads();
      if (tid < NN_TILE) {                                 // a row of the tile, increasing j
        NnPartial p = s_part[tr * NN_TILE + tid];
        for (int c = 0; c < NN_TILE; ++c) {
          const double v = s_msd[tid][c];
          if (v >= 0.0) partial_take(p, v, (int)(col0 + c), a);
        }
        s_part[tr * NN_TILE + tid] = p;
      } else if (tid >= 64 && tid < 64 + NN_TILE) {        // a column of the tile, increasing i
        const int c = tid - 64;
        NnPartial p = s_part[NN_RECT + tc * NN_TILE + c];
        for (int r = 0; r < NN_TILE; ++r) {
          const double v = s_msd[r][c];
          if (v >= 0.0) partial_take(p, v, (int)(row0 + r), a);
        }
        s_part[NN_RECT + tc * NN_TILE + c] = p;
      }
    }
  }
  __syncthreads();
  NnPartial* slot = a.slots + (int64_t)blockIdx.x * 2 * NN_RECT;
  for (int e = tid; e < 2 * NN_RECT; e += NN_THREADS) slot[e] = s_part[e];
  if (a.hist)
    for (int e = tid; e < a.bins; e += NN_THREADS)
      if (s_hist[e]) atomicAdd((unsigned long long*)a.hist + e, (unsigned long long)s_hist[e]);
}

__global__ __launch_bounds__(256) void rmsd_nn_init_kernel(NnState* state, int64_t frames, int64_t* hist, int32_t bins) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < frames) {
    NnState s;
    s.min = INFINITY, s.sum = 0.0, s.pairs = 0, s.arg = -1, s.pad = 0;
#pragma unroll
    for (int t = 0; t < NN_T; ++t) s.count[t] = 0;
    state[e] = s;
  }
  if (hist && e < bins) hist[e] = 0;
}

__device__ __forceinline__ void state_take(NnState& s, const NnPartial& p) {
  if (p.pairs == 0) return;
  if (p.min < s.min) s.min = p.min, s.arg = p.arg;
  s.sum = s.sum + p.sum;
  s.pairs += p.pairs;
#pragma unroll
  for (int t = 0; t < NN_T; ++t) s.count[t] += p.count[t];
}

// One thread a frame (the n of A, then the m of B): the round's slots that hold a partial of the frame, in increasing rectangle number.
__global__ __launch_bounds__(256) void rmsd_nn_fold_kernel(NnState* state, const NnPartial* slots, int32_t n, int32_t m, int32_t self,
                                                           int64_t blocksA, int64_t blocksB, int64_t q0, int64_t used) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)n + (self ? 0 : m)) return;
  NnState s = state[e];
  const int64_t q1 = q0 + used;
  if (!self) {
    if (e < n) {
      const int64_t b = e / NN_RECT, l = e % NN_RECT;
      const int64_t lo = b * blocksB > q0 ? b * blocksB : q0, hi = (b + 1) * blocksB < q1 ? (b + 1) * blocksB : q1;
      for (int64_t q = lo; q < hi; ++q) state_take(s, slots[(q - q0) * 2 * NN_RECT + l]);
    } else {
      const int64_t b = (e - n) / NN_RECT, l = (e - n) % NN_RECT;
      int64_t Rlo = q0 > b ? (q0 - b + blocksB - 1) / blocksB : 0;
      for (int64_t Rr = Rlo; Rr < blocksA; ++Rr) {
        const int64_t q = Rr * blocksB + b;
        if (q >= q1) break;
        state_take(s, slots[(q - q0) * 2 * NN_RECT + NN_RECT + l]);
      }
    }
  } else {
    const int64_t b = e / NN_RECT, l = e % NN_RECT;
    for (int64_t Rr = 0; Rr <= b; ++Rr) {                  // the frame as a column: j < i
      const int64_t q = Rr * blocksA - Rr * (Rr - 1) / 2 + (b - Rr);
      if (q >= q1) break;
      if (q >= q0) state_take(s, slots[(q - q0) * 2 * NN_RECT + NN_RECT + l]);
    }
    const int64_t start = b * blocksA - b * (b - 1) / 2;   // the frame as a row: j > i
    const int64_t lo = start > q0 ? start : q0, hi = start + blocksA - b < q1 ? start + blocksA - b : q1;
    for (int64_t q = lo; q < hi; ++q) state_take(s, slots[(q - q0) * 2 * NN_RECT + l]);
  }
  state[e] = s;
}

__global__ __launch_bounds__(256) void rmsd_nn_write_kernel(const NnState* state, int64_t frames, int32_t T, double* rmsd, int32_t* index,
                                                            double* sum, int64_t* pairs, int64_t* count) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= frames) return;
  const NnState s = state[e];
  if (rmsd) rmsd[e] = s.pairs > 0 ? sqrt(s.min) : NAN;
  if (index) index[e] = s.pairs > 0 ? s.arg : -1;
  if (sum) sum[e] = s.sum;
  if (pairs) pairs[e] = s.pairs;
  if (count) {
#pragma unroll
    for (int t = 0; t < NN_T; ++t)
      if (t < T) count[e * T + t] = s.count[t];
  }
}

}  // namespace
}  // namespace ed

using namespace ed;

extern "C" {

int esmdiff_rmsd_prepare(const double* X, int32_t n, int32_t L, const uint8_t* sel, int32_t n_sel, double* P, double* info, uint8_t* use,
                         void* stream) {
  if (!X || !P || !info || !use || n < 1 || L < 1 || n_sel < 2 || n_sel > L || (!sel && n_sel != L)) return ESMDIFF_E_INVALID;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(rmsd_prepare_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, X, n, L, sel, n_sel, P, info, use);
  return finish_entry(st);
}

int esmdiff_rmsd_nearest(const double* PA, const double* infoA, const uint8_t* useA, int32_t n, const double* PB, const double* infoB,
                         const uint8_t* useB, int32_t m, int32_t n_sel, int32_t allow_reflection, const double* cutoffs, int32_t n_cutoffs,
                         int32_t bins, double width, double* row_rmsd, int32_t* row_index, double* row_sum, int64_t* row_pairs,
                         int64_t* row_count, double* col_rmsd, int32_t* col_index, double* col_sum, int64_t* col_pairs, int64_t* col_count,
                         int64_t* hist, double* msd, double* cross, void* scratch, int64_t scratch_bytes, void* stream) {
  const bool self = !PB;
  if (!PA || !infoA || !useA || n < 1 || n_sel < 2 || n_cutoffs < 0 || n_cutoffs > ESMDIFF_RMSD_NN_MAX_CUTOFFS || bins < 0) return ESMDIFF_E_INVALID;
  if (!self && (!infoB || !useB || m < 1)) return ESMDIFF_E_INVALID;
  if ((n_cutoffs > 0 && !cutoffs) || (bins > 0 && (!hist || !(width > 0.0)))) return ESMDIFF_E_INVALID;
  if (bins > ESMDIFF_RMSD_NN_MAX_BINS) return ESMDIFF_E_CAPACITY;
  if (self) m = 0;
  if (!scratch || scratch_bytes < ESMDIFF_RMSD_NN_SCRATCH_BYTES(n, m, 1)) return ESMDIFF_E_CAPACITY;
  const int64_t frames = (int64_t)n + m, state_bytes = frames * ESMDIFF_RMSD_NN_STATE_BYTES;
  int64_t room = (scratch_bytes - state_bytes) / ESMDIFF_RMSD_NN_SLOT_BYTES;
  if (room > (1 << 20)) room = 1 << 20;

  NnArgs a;
  a.PA = PA, a.infoA = infoA, a.useA = useA, a.PB = PB, a.infoB = infoB, a.useB = useB;
  a.n = n, a.m = m, a.N = n_sel, a.K = ESMDIFF_RMSD_NN_PADDED(n_sel), a.self = self, a.reflect = allow_reflection != 0;
  a.T = n_cutoffs, a.bins = bins, a.width = width;
  for (int t = 0; t < ESMDIFF_RMSD_NN_MAX_CUTOFFS; ++t) a.cut[t] = t < n_cutoffs ? cutoffs[t] : -1.0;
  a.hist = bins > 0 ? hist : nullptr, a.msd = msd, a.cross = cross;
  NnState* state = (NnState*)scratch;
  a.slots = (NnPartial*)((char*)scratch + state_bytes);
  const int64_t blocksA = ((int64_t)n + NN_RECT - 1) / NN_RECT, blocksB = self ? blocksA : ((int64_t)m + NN_RECT - 1) / NN_RECT;
  a.blocksB = blocksB;
  const int64_t rects = self ? blocksA * (blocksA + 1) / 2 : blocksA * blocksB;

  hipStream_t st = (hipStream_t)stream;
  const int64_t init = frames > bins ? frames : bins;
  hipLaunchKernelGGL(rmsd_nn_init_kernel, dim3((unsigned)((init + 255) / 256)), dim3(256), 0, st, state, frames, a.hist, bins);
  for (int64_t q0 = 0; q0 < rects; q0 += room) {
    const int64_t used = rects - q0 < room ? rects - q0 : room;
    hipLaunchKernelGGL(rmsd_nearest_kernel, dim3((unsigned)used), dim3(NN_THREADS), 0, st, a, q0);
    hipLaunchKernelGGL(rmsd_nn_fold_kernel, dim3((unsigned)((frames + 255) / 256)), dim3(256), 0, st, state, (const NnPartial*)a.slots, n, m,
                       (int32_t)self, blocksA, blocksB, q0, used);
  }
  hipLaunchKernelGGL(rmsd_nn_write_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const NnState*)state, (int64_t)n, n_cutoffs,
                     row_rmsd, row_index, row_sum, row_pairs, row_count);
  if (!self)
    hipLaunchKernelGGL(rmsd_nn_write_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, (const NnState*)state + n, (int64_t)m,
                       n_cutoffs, col_rmsd, col_index, col_sum, col_pairs, col_count);
  return finish_entry(st);
}

}  // extern "C"

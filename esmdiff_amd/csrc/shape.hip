// shape.hip — size, shape and scattering of every frame of an ensemble on the device: the centroid and the gyration-tensor sums, the
// Kirkwood sum of inverse distances, the largest distance, the end-to-end distance, the pair-distance histogram of the ensemble, and
// the Debye intensity of every frame at every q.  float64 throughout, INTEGER histogram and counts, float64 sums in a fixed order.
// DESIGN.md §3.25 states the definitions; tests/shape_ref.py restates them in numpy.
//
// A distance is sqrt((dx dx + dy dy) + dz dz) in float64 with the correctly rounded square root and no contraction into FMAs (the
// unit is compiled with -ffp-contract=off), so d, 1 / d, d / width and q d have numpy's bits.  Only sin is the device library's.
// No float atomics anywhere.
//
// Both kernels share one layout.  A WORKGROUP is 8 waves; a frame belongs to a TEAM of W = ESMDIFF_SHAPE_WAVES(L) waves of it, 1 up to
// L = 128 and 8 beyond, so a workgroup holds 8 frames of a short chain (a wave each: 100 000 frames of 58 residues are 12 500
// workgroups, not 100 000 tiny ones) or one frame of a long one.  W depends on L alone and so does every order below.  The team
// stages its frame in LDS as planes x[L], y[L], z[L]: a residue that is masked, or has a NaN coordinate, is NaN in all three planes,
// and a masked coordinate is never read from memory.  A pair whose distance is NaN is not a pair: no mask is read in the inner
// loop.  The read of residue a is a broadcast, the reads of b are 64 consecutive doubles per wave: no bank conflict.
//
//   THE ORDER OF A SUM OVER RESIDUES (centroid, tensor sums, sum of f^2): wave 0 of the team alone; lane l adds the terms of the
//     residues b = l, l + 64, l + 128 ... in increasing b from +0.0, a residue that is not valid adding nothing; the 64 lane sums
//     are combined by the xor butterfly of ed_wave.h (offsets 32, 16 .. 1).
//   THE ORDER OF A SUM OVER PAIRS a < b (sum_inv_d, the Debye sums): wave w of the team takes the rows a = w, w + W, w + 2 W ... in
//     that order; in row a lane l takes b = a + 1 + l, a + 1 + l + 64 ... in increasing b; a lane keeps ONE sum, from +0.0, across
//     all its rows, a pair that is not valid adding nothing; then the butterfly; then, for W = 8, the wave sums as
//     ((w0 + w1) + (w2 + w3)) + ((w4 + w5) + (w6 + w7)).
//
//   shape_frames_kernel  grid (ceil(n / (8 / W))).  Wave 0 of a team counts the valid residues, sums the coordinates, divides once,
//                        and sums the six products about that centroid in a second pass.  Every wave walks its rows for 1 / d, the
//                        largest d (a maximum: no order) and the histogram cell (int)floor(d / width), counted with integer
//                        atomics in a histogram of the workgroup in LDS and flushed, non-empty cells only, with 64-bit integer
//                        atomics on the output (zeroed by the entry).
//   debye_frames_kernel  grid (ceil(n / (8 / W)), ceil(Q / 8)).  The same walk with eight sums per lane in registers, one per q of
//                        the chunk; d is computed once per pair and chunk, then x = q d (one product), s = x == 0 ? 1 : sin(x) / x,
//                        term = (f_a f_b) s.  A q's sum does not know which chunk it is in, nor Q: the same q gives the same bits
//                        in any q array.  I = sum f^2 + 2.0 (pair sum).  Form factors are read from memory (L x Q does not fit
//                        LDS beside the planes), the row a's as wave-uniform loads.
#include <math.h>

#include <cmath>

#include "ed_f64.h"
#include "ed_wave.h"
#include "kernels.h"

namespace ed {
namespace {

typedef unsigned long long u64;

constexpr int SH_THREADS = 512, SH_WAVES = SH_THREADS / 64;
constexpr int SH_QCHUNK = ESMDIFF_DEBYE_Q_CHUNK;
static_assert(SH_QCHUNK == 8, "eight sums per lane");
static_assert(SH_WAVES == 8, "the fixed tree below combines eight wave sums");
static_assert(24 * ESMDIFF_SHAPE_MAX_L + 4 * (ESMDIFF_SHAPE_MAX_BINS + 1) <= 144 * 1024, "the longest chain and the widest histogram fit LDS");

// which frame this thread works on, where in its team (ed_wave.h), and the team's planes
struct Team : WaveTeam {
  int t, frame;
  double *x, *y, *z;
  bool active;
};

__device__ __forceinline__ Team team_of(double* planes, int n, int L) {
  Team m;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  static_cast<WaveTeam&>(m) = wave_team(wave, ESMDIFF_SHAPE_WAVES(L), SH_WAVES);
  m.t = m.w * 64 + m.lane;
  m.frame = blockIdx.x * m.teams + m.team;
  m.active = m.frame < n;
  m.x = planes + (size_t)m.team * 3 * L, m.y = m.x + L, m.z = m.y + L;
  return m;
}

// the team's frame into its planes; the caller puts the barrier behind it
__device__ __forceinline__ void stage(const Team& m, const double* X, const uint8_t* mask, int L) {
  if (!m.active) return;
  for (int b = m.t; b < L; b += m.T) {
    double x = quiet_nan(), y = quiet_nan(), z = quiet_nan();
    const int64_t row = (int64_t)m.frame * L + b;
    if (!mask || mask[row]) {
      const double* p = X + row * 3;
      const double px = p[0], py = p[1], pz = p[2];
      if (px == px && py == py && pz == pz) x = px, y = py, z = pz;
    }
    m.x[b] = x, m.y[b] = y, m.z[b] = z;
  }
}

struct ShapeArgs {
  const double* X;
  const uint8_t* mask;
  int32_t* count;
  double* desc;
  int64_t* hist;
  double width;
  int n, L, bins;
};

// dynamic LDS: f64 [teams][3][L], then (HIST) i32 [bins + 1]
template <bool HIST>
__global__ __launch_bounds__(SH_THREADS) void shape_frames_kernel(const ShapeArgs p) {
  extern __shared__ double s_planes[];
  __shared__ double s_inv[SH_WAVES], s_max[SH_WAVES];
  const int L = p.L;
  const Team m = team_of(s_planes, p.n, L);
  int* s_hist = (int*)(s_planes + (size_t)(SH_WAVES / m.W) * 3 * L);
  if (HIST)
    for (int c = threadIdx.x; c <= p.bins; c += SH_THREADS) s_hist[c] = 0;
  stage(m, p.X, p.mask, L);
  __syncthreads();

  const int wave = threadIdx.x >> 6;
  if (m.active) {
    if (m.w == 0) {                                        // the sums over residues
      int cnt = 0;
      double sx = 0.0, sy = 0.0, sz = 0.0;
      for (int b = m.lane; b < L; b += 64) {
        const double x = m.x[b], y = m.y[b], z = m.z[b];
        const bool ok = x == x;
        cnt += ok ? 1 : 0;
        sx = ok ? sx + x : sx, sy = ok ? sy + y : sy, sz = ok ? sz + z : sz;
      }
      const int N = wave_sum(cnt);
      sx = wave_sum(sx), sy = wave_sum(sy), sz = wave_sum(sz);
      const double cx = N ? sx / (double)N : quiet_nan(), cy = N ? sy / (double)N : quiet_nan(), cz = N ? sz / (double)N : quiet_nan();
      double g[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};       // xx, yy, zz, xy, xz, yz
      for (int b = m.lane; b < L; b += 64) {
        const double dx = m.x[b] - cx, dy = m.y[b] - cy, dz = m.z[b] - cz;
        const bool ok = dx == dx;                          // false for a residue that is not valid, and for all when N = 0
        g[0] = ok ? g[0] + dx * dx : g[0], g[1] = ok ? g[1] + dy * dy : g[1], g[2] = ok ? g[2] + dz * dz : g[2];
        g[3] = ok ? g[3] + dx * dy : g[3], g[4] = ok ? g[4] + dx * dz : g[4], g[5] = ok ? g[5] + dy * dz : g[5];
      }
#pragma unroll
      for (int k = 0; k < 6; ++k) g[k] = wave_sum(g[k]);
      if (m.lane == 0) {
        double* out = p.desc + (int64_t)m.frame * 12;
        p.count[m.frame] = N;
        out[0] = cx, out[1] = cy, out[2] = cz;
#pragma unroll
        for (int k = 0; k < 6; ++k) out[3 + k] = g[k];
        out[11] = dist(m.x[L - 1] - m.x[0], m.y[L - 1] - m.y[0], m.z[L - 1] - m.z[0]);      // NaN unless both ends are valid
      }
    }

    double inv = 0.0, dm = 0.0;                            // the sums over pairs
    for (int a = m.w; a < L - 1; a += m.W) {
      const double ax = m.x[a], ay = m.y[a], az = m.z[a];
      if (!(ax == ax)) continue;                           // the same in every lane
      for (int b = a + 1 + m.lane; b < L; b += 64) {
        const double d = dist(m.x[b] - ax, m.y[b] - ay, m.z[b] - az);
        const bool ok = d == d;
        inv = ok ? inv + 1.0 / d : inv;
        dm = d > dm ? d : dm;                              // false for NaN
        if (HIST && ok) {
          const double cell = floor(d / p.width);
          atomicAdd(&s_hist[cell >= (double)p.bins ? p.bins : (int)cell], 1);
        }
      }
    }
    inv = wave_sum(inv), dm = wave_max(dm);
    if (m.lane == 0) s_inv[wave] = inv, s_max[wave] = dm;
  }
  __syncthreads();

  if (m.active && m.t == 0) {
    double* out = p.desc + (int64_t)m.frame * 12;
    if (m.W == 1) {
      out[9] = s_inv[wave], out[10] = s_max[wave];
    } else {
      double top = s_max[0];
#pragma unroll
      for (int k = 1; k < SH_WAVES; ++k) top = s_max[k] > top ? s_max[k] : top;
      out[9] = tree8(s_inv), out[10] = top;
    }
  }
  if (HIST)
    for (int c = threadIdx.x; c <= p.bins; c += SH_THREADS) {
      const int v = s_hist[c];
      if (v) atomicAdd((u64*)&p.hist[c], (u64)v);
    }
}

struct DebyeArgs {
  const double* X;
  const uint8_t* mask;
  const double *q, *ff;
  double* intensity;
  int n, L, Q;
};

// dynamic LDS: f64 [teams][3][L]
template <bool FF>
__global__ __launch_bounds__(SH_THREADS) void debye_frames_kernel(const DebyeArgs p) {
  extern __shared__ double s_planes[];
  __shared__ double s_sum[SH_WAVES][SH_QCHUNK];
  const int L = p.L, Q = p.Q;
  const Team m = team_of(s_planes, p.n, L);
  const int q0 = blockIdx.y * SH_QCHUNK, nq = min(SH_QCHUNK, Q - q0);
  stage(m, p.X, p.mask, L);
  __syncthreads();

  const int wave = threadIdx.x >> 6;
  double self[SH_QCHUNK];                                  // sum f^2, in wave 0 of the team
  if (m.active) {
    double qv[SH_QCHUNK], acc[SH_QCHUNK];
#pragma unroll
    for (int j = 0; j < SH_QCHUNK; ++j) qv[j] = j < nq ? p.q[q0 + j] : 0.0, acc[j] = 0.0, self[j] = 0.0;

    if (m.w == 0) {
      for (int b = m.lane; b < L; b += 64) {
        const bool ok = m.x[b] == m.x[b];
#pragma unroll
        for (int j = 0; j < SH_QCHUNK; ++j) {
          if (j < nq) {
            const double f = FF ? p.ff[(int64_t)b * Q + q0 + j] : 1.0;
            self[j] = ok ? self[j] + f * f : self[j];
          }
        }
      }
#pragma unroll
      for (int j = 0; j < SH_QCHUNK; ++j) self[j] = wave_sum(self[j]);
    }

    for (int a = m.w; a < L - 1; a += m.W) {
      const double ax = m.x[a], ay = m.y[a], az = m.z[a];
      if (!(ax == ax)) continue;                           // the same in every lane
      double fa[SH_QCHUNK];
#pragma unroll
      for (int j = 0; j < SH_QCHUNK; ++j) fa[j] = (FF && j < nq) ? p.ff[(int64_t)a * Q + q0 + j] : 1.0;
      for (int b = a + 1 + m.lane; b < L; b += 64) {
        const double d = dist(m.x[b] - ax, m.y[b] - ay, m.z[b] - az);
        const bool ok = d == d;
#pragma unroll
        for (int j = 0; j < SH_QCHUNK; ++j) {
          if (j < nq) {                                    // the same in every lane
            const double x = qv[j] * d;
            const double s = x == 0.0 ? 1.0 : sin(x) / x;
            const double term = FF ? (fa[j] * p.ff[(int64_t)b * Q + q0 + j]) * s : s;
            acc[j] = ok ? acc[j] + term : acc[j];
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < SH_QCHUNK; ++j) {
      const double s = wave_sum(acc[j]);
      if (m.lane == 0) s_sum[wave][j] = s;
    }
  }
  __syncthreads();

  if (m.active && m.w == 0 && m.lane < nq) {               // lane j of the team's first wave writes q0 + j
    double pairs = 0.0, own = 0.0;
#pragma unroll
    for (int j = 0; j < SH_QCHUNK; ++j) {
      if (j == m.lane) {
        own = self[j];
        if (m.W == 1) {
          pairs = s_sum[wave][j];
        } else {
          double col[SH_WAVES];
#pragma unroll
          for (int k = 0; k < SH_WAVES; ++k) col[k] = s_sum[k][j];
          pairs = tree8(col);
        }
      }
    }
    p.intensity[(int64_t)m.frame * Q + q0 + m.lane] = own + 2.0 * pairs;
  }
}

int planes_bytes(int L) { return (SH_WAVES / ESMDIFF_SHAPE_WAVES(L)) * 3 * L * (int)sizeof(double); }

}  // namespace
}  // namespace ed

using namespace ed;

extern "C" {

int esmdiff_shape_frames(const double* X, int32_t n, int32_t L, const uint8_t* mask, int32_t* count, double* desc, int64_t* hist,
                         double width, int32_t bins, void* stream) {
  if (!X || !count || !desc || n < 0 || L < 1) return ESMDIFF_E_INVALID;
  if (hist && (bins < 1 || !(width > 0.0) || !std::isfinite(width))) return ESMDIFF_E_INVALID;
  if (L > ESMDIFF_SHAPE_MAX_L || (hist && bins > ESMDIFF_SHAPE_MAX_BINS)) return ESMDIFF_E_CAPACITY;

  hipStream_t st = (hipStream_t)stream;
  if (hist && hipMemsetAsync(hist, 0, (size_t)(bins + 1) * sizeof(int64_t), st) != hipSuccess) return ESMDIFF_E_HIP;
  if (n == 0) return finish_entry(st);
  ShapeArgs p;
  p.X = X, p.mask = mask, p.count = count, p.desc = desc, p.hist = hist, p.width = width, p.n = n, p.L = L, p.bins = hist ? bins : 0;
  const int teams = SH_WAVES / ESMDIFF_SHAPE_WAVES(L), blocks = (n + teams - 1) / teams;
  const int lds = planes_bytes(L) + (hist ? (bins + 1) * (int)sizeof(int) : 0);
  const auto kernel = hist ? shape_frames_kernel<true> : shape_frames_kernel<false>;
  if (ensure_dynamic_lds((const void*)kernel, lds) != hipSuccess) return ESMDIFF_E_HIP;
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(SH_THREADS), (size_t)lds, st, p);
  return finish_entry(st);
}

int esmdiff_debye_frames(const double* X, int32_t n, int32_t L, const uint8_t* mask, const double* q, int32_t Q, const double* ff,
                         double* intensity, void* stream) {
  if (!X || !q || !intensity || n < 0 || L < 1 || Q < 1) return ESMDIFF_E_INVALID;
  if (L > ESMDIFF_SHAPE_MAX_L || Q > ESMDIFF_DEBYE_MAX_Q) return ESMDIFF_E_CAPACITY;
  if (n == 0) return 0;

  DebyeArgs p;
  p.X = X, p.mask = mask, p.q = q, p.ff = ff, p.intensity = intensity, p.n = n, p.L = L, p.Q = Q;
  const int teams = SH_WAVES / ESMDIFF_SHAPE_WAVES(L), blocks = (n + teams - 1) / teams;
  const int chunks = (Q + SH_QCHUNK - 1) / SH_QCHUNK, lds = planes_bytes(L);
  const auto kernel = ff ? debye_frames_kernel<true> : debye_frames_kernel<false>;
  if (ensure_dynamic_lds((const void*)kernel, lds) != hipSuccess) return ESMDIFF_E_HIP;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks, (unsigned)chunks), dim3(SH_THREADS), (size_t)lds, st, p);
  return finish_entry(st);
}

}  // extern "C"

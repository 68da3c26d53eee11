// sasa.hip — solvent accessibility of every frame of an ensemble on the device by Shrake & Rupley's point test, reduced over the frames
// to per-atom sums and per-residue exposure counts, and the co-occurrence counts of any (n, L) table of two-state flags.  float64
// arithmetic, INTEGER outputs, integer atomics only.  DESIGN.md §3.26 states the definitions; tests/sasa_ref.py restates them in numpy
// without any cull.
//
// Atom (a, k) of a frame has the centre c and the expanded radius R = radii[a][k].  Point k of atom i is p = c_i + R_i u_k, one product
// and one add per component and no FMA (the unit is compiled with -ffp-contract=off); it is buried when some other valid atom j of the
// frame has ((dx dx + dy dy) + dz dz) < R_j R_j with d = p - c_j, strictly.  The unit points are an argument: no cosine is evaluated
// here, so both sides hold the same bits and every count equals numpy's.
//
// LAYOUT.  A workgroup is 8 waves.  A frame of NA = L A atoms belongs to a TEAM of W waves, 1 up to NA = 256 and 8 beyond, so a
// workgroup holds 8 frames of a short chain or one frame of a long one.  The team stages its frame in LDS as planes x[NA], y[NA],
// z[NA], R[NA] and a plane of counts (36 bytes an atom: 144 KiB at the limit of 4 096 atoms); an atom of a masked residue, or with a
// NaN coordinate, is NaN in x, y and z, and a masked coordinate is never read from memory.  A WAVE owns an atom i at a time.  Its lanes
// hold the points lane, lane + 64 (a PASS of 128 points; P > 128 takes more passes over the same atom).  The wave walks the frame's
// atoms in chunks of 64 candidates, lane l testing candidate c0 + l for being a neighbour (64 consecutive doubles of each plane: no
// bank conflict); a ballot gives the wave-uniform set of the chunk's neighbours, and only those are tested against the points, their
// planes read at one address by all lanes (an LDS broadcast).  The walk of a pass stops once every point of it is buried.  No list of
// neighbours is stored, so a collapsed structure in which every atom neighbours every other overflows nothing.  Counts are integers:
// no order of summation has to be published.
//
// THE CULL NEVER CHANGES A COUNT.  Candidate j is skipped only when the computed d_ij^2 >= s^2 with
//     s = (R_i + R_j) + m,    m = 1e-6 + 2^-40 ((|x_i| + |y_i| + |z_i|) + (R_i + R_j)),
// and a d_ij^2 that is NaN (centres at infinity) is never skipped.  With eps = 2^-53: the computed point p' differs from c_i + R_i u_k
// by at most 2 eps (|c_i|_1 + 2 R_i) in length (one rounding of the product, one of the sum, per component), and |u_k| <= 1 + 4 eps, so
// |p' - c_i| <= R_i + 2^-50 (|c_i|_1 + R_i).  The computed d_ij^2 and s^2 carry relative errors below 6 eps (differences of two
// float64 are single roundings), so a skipped j has |c_i - c_j| >= s (1 - 6 eps), and by the triangle inequality
// |p' - c_j| >= R_j + m - 6 eps s - 2^-50 (|c_i|_1 + R_i) >= R_j + m / 2, since m >= 2^-40 (|c_i|_1 + R_i + R_j) is a thousand times both
// error terms.  The point test then computes at least (R_j + m / 2)^2 (1 - 6 eps) > R_j^2 (1 + eps) >= fl(R_j R_j), because
// m / 2 >= 2^-41 R_j: not buried, as without the cull.  The absolute 1e-6 is not needed by this argument; it keeps touching spheres
// (d = R_i + R_j exactly, the lattice of the tests) well inside the tested set.  The argument assumes that no square overflows:
// coordinates and radii below 1e150.
#include <math.h>

#include <cmath>

#include "ed_f64.h"
#include "ed_wave.h"
#include "kernels.h"

namespace ed {
namespace {

typedef unsigned long long u64;

constexpr int SA_THREADS = 512, SA_WAVES = SA_THREADS / 64;
constexpr int SA_SMALL = 256;                              // the atoms up to which a frame belongs to one wave
constexpr int SA_ATOM_BYTES = 4 * (int)sizeof(double) + (int)sizeof(int);
constexpr double SA_MARGIN = 1e-6, SA_MARGIN_REL = 1.0 / 1099511627776.0;      // 2^-40
constexpr double SA_FOUR_PI = 12.566370614359172;          // 4.0 * math.pi
static_assert(SA_ATOM_BYTES * ESMDIFF_SASA_MAX_ATOMS <= 144 * 1024, "the largest frame fits LDS");
static_assert(SA_ATOM_BYTES * SA_SMALL * SA_WAVES <= 144 * 1024, "eight short frames fit LDS");

struct SasaArgs {
  const double* X;
  const uint8_t* mask;
  const double *radii, *points;
  int32_t* count;
  int64_t* sum_count;
  int32_t* valid;
  uint8_t* exposed;
  int32_t *exposed_count, *present_count;
  double threshold;
  int n, L, A, P;
};

// dynamic LDS: f64 [teams][4][NA] (x, y, z, R), then i32 [teams][NA] (the exposed points of each atom, -1 for an absent one)
template <int PT>
__global__ __launch_bounds__(SA_THREADS) void sasa_frames_kernel(const SasaArgs p) {
  extern __shared__ double s_planes[];
  const int L = p.L, A = p.A, NA = L * A, P = p.P;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const WaveTeam g = wave_team(wave, NA <= SA_SMALL ? 1 : SA_WAVES, SA_WAVES);
  const int W = g.W, teams = g.teams, team = g.team, w = g.w, T = g.T, t = w * 64 + lane;
  const int64_t frame0 = (int64_t)blockIdx.x * teams, frame = frame0 + team;
  const bool active = frame < p.n;
  double *sx = s_planes + (size_t)team * 4 * NA, *sy = sx + NA, *sz = sy + NA, *sr = sz + NA;
  int* s_count = (int*)(s_planes + (size_t)teams * 4 * NA);

  if (active) {                                            // the team's frame into its planes
    for (int idx = t; idx < NA; idx += T) {
      double x = quiet_nan(), y = quiet_nan(), z = quiet_nan();
      if (!p.mask || p.mask[frame * L + idx / A]) {
        const double* c = p.X + (frame * NA + idx) * 3;
        const double px = c[0], py = c[1], pz = c[2];
        if (px == px && py == py && pz == pz) x = px, y = py, z = pz;
      }
      sx[idx] = x, sy[idx] = y, sz[idx] = z, sr[idx] = p.radii[idx];
      s_count[(size_t)team * NA + idx] = -1;
    }
  }
  __syncthreads();

  if (active) {
    const int passes = (P + 64 * PT - 1) / (64 * PT);
    double ux[PT], uy[PT], uz[PT];
#pragma unroll
    for (int q = 0; q < PT; ++q) {                         // one pass: the points stay in registers for every atom
      const int k = q * 64 + lane;
      const bool in = k < P;
      ux[q] = in ? p.points[k * 3] : 0.0, uy[q] = in ? p.points[k * 3 + 1] : 0.0, uz[q] = in ? p.points[k * 3 + 2] : 0.0;
    }
    for (int i = w; i < NA; i += W) {
      const double cx = sx[i], cy = sy[i], cz = sz[i], Ri = sr[i];
      if (!(cx == cx)) continue;                           // absent, the same in every lane: its count stays -1
      const double reach = (fabs(cx) + fabs(cy)) + fabs(cz);
      int exposed = 0;
      for (int pass = 0; pass < passes; ++pass) {
        double px[PT], py[PT], pz[PT];
        bool open[PT];                                     // a point of this atom that nothing has buried yet
#pragma unroll
        for (int q = 0; q < PT; ++q) {
          const int k = (pass * PT + q) * 64 + lane;
          open[q] = k < P;
          if (passes > 1) ux[q] = open[q] ? p.points[k * 3] : 0.0, uy[q] = open[q] ? p.points[k * 3 + 1] : 0.0, uz[q] = open[q] ? p.points[k * 3 + 2] : 0.0;
          px[q] = cx + Ri * ux[q], py[q] = cy + Ri * uy[q], pz[q] = cz + Ri * uz[q];
        }
        for (int c0 = 0; c0 < NA; c0 += 64) {
          const int j = c0 + lane;
          bool near = false;
          if (j < NA && j != i) {
            const double xj = sx[j], pair = Ri + sr[j];
            const double s = pair + (SA_MARGIN + SA_MARGIN_REL * (reach + pair));
            near = xj == xj && !(sq3(xj - cx, sy[j] - cy, sz[j] - cz) >= s * s);
          }
          u64 m = __ballot(near);
          while (m) {                                      // the chunk's neighbours, one at a time, the same in every lane
            const int b = c0 + __builtin_ctzll(m);
            m &= m - 1;
            const double xb = sx[b], yb = sy[b], zb = sz[b], rb = sr[b], r2 = rb * rb;
#pragma unroll
            for (int q = 0; q < PT; ++q) open[q] = open[q] && !(sq3(px[q] - xb, py[q] - yb, pz[q] - zb) < r2);
          }
          bool some = false;
#pragma unroll
          for (int q = 0; q < PT; ++q) some = some || open[q];
          if (!__any(some)) break;
        }
#pragma unroll
        for (int q = 0; q < PT; ++q) exposed += __popcll(__ballot(open[q]));
      }
      if (lane == 0) s_count[(size_t)team * NA + i] = exposed;
    }
  }
  __syncthreads();

  // the frames of this workgroup together: one atomic per atom and per residue, whatever the number of teams
  for (int idx = tid; idx < NA; idx += SA_THREADS) {
    u64 sum = 0;
    int present = 0;
    for (int g = 0; g < teams && frame0 + g < p.n; ++g) {
      const int c = s_count[(size_t)g * NA + idx];
      if (p.count) p.count[(frame0 + g) * NA + idx] = c;
      if (c >= 0) sum += (u64)c, ++present;
    }
    if (present && p.sum_count) atomicAdd((u64*)&p.sum_count[idx], sum);
    if (present && p.valid) atomicAdd(&p.valid[idx], present);
  }
  if (p.exposed || p.exposed_count || p.present_count) {
    for (int a = tid; a < L; a += SA_THREADS) {
      int ones = 0, defined = 0;
      for (int g = 0; g < teams && frame0 + g < p.n; ++g) {
        const double* radius = s_planes + (size_t)g * 4 * NA + 3 * NA;
        double area = 0.0, alone = 0.0;                    // ((a0 + a1) + a2) + a3: an absent atom adds nothing
        bool any = false;
        for (int k = 0; k < A; ++k) {
          const int c = s_count[(size_t)g * NA + a * A + k];
          if (c < 0) continue;
          const double R = radius[a * A + k], sphere = SA_FOUR_PI * (R * R);
          area = area + (sphere * (double)c) / (double)P;
          alone = alone + (sphere * (double)P) / (double)P;
          any = true;
        }
        const int flag = !any ? 2 : (area / alone > p.threshold ? 1 : 0);
        if (p.exposed) p.exposed[(frame0 + g) * L + a] = (uint8_t)flag;
        ones += flag == 1, defined += flag != 2;
      }
      if (ones && p.exposed_count) atomicAdd(&p.exposed_count[a], ones);
      if (defined && p.present_count) atomicAdd(&p.present_count[a], defined);
    }
  }
}

constexpr int CO_PACK_THREADS = 256, CO_TILE = 16, CO_WORDS = 32;

// grid (words, ceil(L / 64)): 64 frames x 64 residues through LDS, so that the table is read along its rows and balloted along its columns
__global__ __launch_bounds__(CO_PACK_THREADS) void cooccurrence_pack_kernel(const uint8_t* flags, int n, int L, int64_t words, u64* one,
                                                                           u64* defined) {
  __shared__ uint8_t s[64][68];
  const int lane = threadIdx.x & 63, r = threadIdx.x >> 6;
  const int64_t f0 = (int64_t)blockIdx.x * 64;
  const int a0 = blockIdx.y * 64;
  for (int row = r; row < 64; row += CO_PACK_THREADS / 64) {
    const int64_t f = f0 + row;
    const int a = a0 + lane;
    s[row][lane] = (f < n && a < L) ? flags[f * L + a] : (uint8_t)2;
  }
  __syncthreads();
  for (int col = r; col < 64; col += CO_PACK_THREADS / 64) {
    const int v = s[lane][col], a = a0 + col;
    const u64 m1 = __ballot(v == 1), md = __ballot(v < 2);
    if (lane == 0 && a < L) one[(int64_t)a * words + blockIdx.x] = m1, defined[(int64_t)a * words + blockIdx.x] = md;
  }
}

// grid (ceil(L / 16), ceil(L / 16)): thread (ta, tb) of a tile ANDs the words of residues a and b and counts the bits
__global__ __launch_bounds__(CO_TILE * CO_TILE) void cooccurrence_count_kernel(const u64* one, const u64* defined, int L, int64_t words,
                                                                              int32_t* out) {
  __shared__ u64 s_a1[CO_TILE][CO_WORDS + 1], s_ad[CO_TILE][CO_WORDS + 1], s_b1[CO_TILE][CO_WORDS + 1], s_bd[CO_TILE][CO_WORDS + 1];
  const int tid = threadIdx.x, ta = tid / CO_TILE, tb = tid % CO_TILE;
  const int a0 = blockIdx.y * CO_TILE, b0 = blockIdx.x * CO_TILE;
  int both = 0, a_one = 0, both_one = 0;
  for (int64_t w0 = 0; w0 < words; w0 += CO_WORDS) {
    for (int e = tid; e < CO_TILE * CO_WORDS; e += CO_TILE * CO_TILE) {
      const int row = e / CO_WORDS, col = e % CO_WORDS;
      const int64_t word = w0 + col;
      const bool ia = word < words && a0 + row < L, ib = word < words && b0 + row < L;
      s_a1[row][col] = ia ? one[(int64_t)(a0 + row) * words + word] : 0, s_ad[row][col] = ia ? defined[(int64_t)(a0 + row) * words + word] : 0;
      s_b1[row][col] = ib ? one[(int64_t)(b0 + row) * words + word] : 0, s_bd[row][col] = ib ? defined[(int64_t)(b0 + row) * words + word] : 0;
    }
    __syncthreads();
#pragma unroll 8
    for (int col = 0; col < CO_WORDS; ++col) {
      const u64 a1 = s_a1[ta][col], ad = s_ad[ta][col], b1 = s_b1[tb][col], bd = s_bd[tb][col];
      both += __popcll(ad & bd), a_one += __popcll(a1 & bd), both_one += __popcll(a1 & b1);
    }
    __syncthreads();
  }
  const int a = a0 + ta, b = b0 + tb;
  if (a < L && b < L) {
    const int64_t at = (int64_t)a * L + b, plane = (int64_t)L * L;
    out[at] = both, out[plane + at] = a_one, out[2 * plane + at] = both_one;
  }
}

}  // namespace
}  // namespace ed

using namespace ed;

extern "C" {

int esmdiff_sasa_frames(const double* X, int32_t n, int32_t L, int32_t A, const uint8_t* mask, const double* radii, const double* points,
                        int32_t P, double threshold, int32_t* count, int64_t* sum_count, int32_t* valid, uint8_t* exposed,
                        int32_t* exposed_count, int32_t* present_count, void* stream) {
  if (!X || !radii || !points || n < 0 || L < 1 || !(A == 1 || A == 3 || A == 4) || P < 1) return ESMDIFF_E_INVALID;
  if ((exposed || exposed_count || present_count) && threshold != threshold) return ESMDIFF_E_INVALID;
  if ((int64_t)L * A > ESMDIFF_SASA_MAX_ATOMS || P > ESMDIFF_SASA_MAX_POINTS) return ESMDIFF_E_CAPACITY;

  hipStream_t st = (hipStream_t)stream;
  const int NA = L * A;
  if (sum_count && hipMemsetAsync(sum_count, 0, (size_t)NA * sizeof(int64_t), st) != hipSuccess) return ESMDIFF_E_HIP;
  if (valid && hipMemsetAsync(valid, 0, (size_t)NA * sizeof(int32_t), st) != hipSuccess) return ESMDIFF_E_HIP;
  if (exposed_count && hipMemsetAsync(exposed_count, 0, (size_t)L * sizeof(int32_t), st) != hipSuccess) return ESMDIFF_E_HIP;
  if (present_count && hipMemsetAsync(present_count, 0, (size_t)L * sizeof(int32_t), st) != hipSuccess) return ESMDIFF_E_HIP;
  if (n == 0) return finish_entry(st);

  SasaArgs p;
  p.X = X, p.mask = mask, p.radii = radii, p.points = points, p.count = count, p.sum_count = sum_count, p.valid = valid;
  p.exposed = exposed, p.exposed_count = exposed_count, p.present_count = present_count, p.threshold = threshold;
  p.n = n, p.L = L, p.A = A, p.P = P;
  const int teams = NA <= SA_SMALL ? SA_WAVES : 1, blocks = (int)(((int64_t)n + teams - 1) / teams), lds = teams * NA * SA_ATOM_BYTES;
  const auto kernel = P <= 64 ? sasa_frames_kernel<1> : sasa_frames_kernel<2>;
  if (ensure_dynamic_lds((const void*)kernel, lds) != hipSuccess) return ESMDIFF_E_HIP;
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(SA_THREADS), (size_t)lds, st, p);
  return finish_entry(st);
}

int esmdiff_cooccurrence(const uint8_t* flags, int32_t n, int32_t L, int32_t* out, void* scratch, int64_t scratch_bytes, void* stream) {
  if (!flags || !out || n < 0 || L < 1) return ESMDIFF_E_INVALID;
  if (L > ESMDIFF_COOCC_MAX_L) return ESMDIFF_E_CAPACITY;
  const int64_t need = ESMDIFF_COOCC_SCRATCH_BYTES(n, L), words = ((int64_t)n + 63) / 64;
  if (need > 0 && (!scratch || scratch_bytes < need)) return scratch ? ESMDIFF_E_CAPACITY : ESMDIFF_E_INVALID;

  hipStream_t st = (hipStream_t)stream;
  u64 *one = (u64*)scratch, *defined = one + (int64_t)L * words;
  if (words)
    hipLaunchKernelGGL(cooccurrence_pack_kernel, dim3((unsigned)words, (unsigned)((L + 63) / 64)), dim3(CO_PACK_THREADS), 0, st, flags, n, L,
                       words, one, defined);
  const unsigned tiles = (unsigned)((L + CO_TILE - 1) / CO_TILE);
  hipLaunchKernelGGL(cooccurrence_count_kernel, dim3(tiles, tiles), dim3(CO_TILE * CO_TILE), 0, st, one, defined, L, words, out);
  return finish_entry(st);
}

}  // extern "C"

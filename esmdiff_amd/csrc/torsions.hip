// torsions.hip — the backbone torsions phi / psi / omega of N / CA / C backbones, their bond lengths and angles, and the Ramachandran
// maps of an ensemble reduced over its frames: float64 geometry, INTEGER histograms and counts, float64 circular sums in a fixed
// order.  DESIGN.md §3.24 states the definitions; tests/torsions_ref.py restates them in numpy.
//
// Every product and sum is rounded once (the unit is compiled with -ffp-contract=off) and written out in the order the header
// states, so x and y of a dihedral — the two arguments of atan2, the sign that decides cis, the terms of the circular sums — have
// numpy's bits.  Only atan2 itself is the device library's.  No float atomics anywhere.
//
//   torsions_kernel   one thread per (frame, residue), the residue the fastest index: it reads residues i - 1, i, i + 1 (neighbouring
//                     lanes read neighbouring residues: the lines are shared in L1 / L2) and writes its three angles and, if asked,
//                     its six lengths and angles.  Nothing is staged per chain: no limit on L.
//   rama_kernel       one thread per (residue, chunk of frames), the residue the fastest index.  It walks the frames f of its chunk,
//                     c F .. min(n, (c + 1) F) - 1 with F = ESMDIFF_RAMA_CHUNK_FRAMES(n, L), in increasing f with six sums and five
//                     counters in registers; residue_xy below gives it the same x and y as torsions_kernel.  Its histogram cell is
//                     one integer atomic on the global array (zeroed by the entry): a private histogram per workgroup would hold
//                     bins^2 cells per residue and be flushed mostly empty.  (Loading the next frame ahead and one atomic per
//                     run of equal cells were measured and bought 4 %: EXPERIMENTS.md "Torsions".)  The counters end as five
//                     integer atomics on counts (zeroed by the entry).  One chunk: the sums go straight to the output; more: to
//                     the scratch [chunk][residue][6], and
//   rama_fold_kernel  one thread per (residue, sum) adds the chunk sums in increasing chunk index (s = part[0]; s += part[1]; ...),
//                     16 loads in flight at a time: the additions are a chain, the loads need not be.
#include <math.h>

#include <cmath>

#include "ed_f64.h"
#include "kernels.h"

namespace ed {
namespace {

constexpr int TOR_THREADS = 256;
constexpr double DEG = 57.29577951308232;

struct V3 {
  double x, y, z;
};
__device__ __forceinline__ V3 sub(const V3& a, const V3& b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 cross(const V3& a, const V3& b) {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ double dot(const V3& a, const V3& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ bool finite3(const V3& a) { return isfinite(a.x) && isfinite(a.y) && isfinite(a.z); }

struct Residue {
  V3 n, ca, c;
  bool present;
};

// row = frame * L + residue.  A masked residue's coordinates are loaded (the memory is the caller's array) and never used.
__device__ __forceinline__ Residue load_residue(const double* X, const uint8_t* mask, int64_t row, int atoms) {
  const double* p = X + row * (3 * atoms);
  Residue r;
  r.n = {p[0], p[1], p[2]}, r.ca = {p[3], p[4], p[5]}, r.c = {p[6], p[7], p[8]};
  r.present = (!mask || mask[row]) && finite3(r.n) && finite3(r.ca) && finite3(r.c);
  return r;
}

__device__ __forceinline__ Residue absent() {
  Residue r;
  r.n = r.ca = r.c = {0.0, 0.0, 0.0};
  r.present = false;
  return r;
}

// the two arguments of atan2; false: the angle is undefined
__device__ __forceinline__ bool dihedral_xy(const V3& p0, const V3& p1, const V3& p2, const V3& p3, double& x, double& y) {
  const V3 b1 = sub(p1, p0), b2 = sub(p2, p1), b3 = sub(p3, p2);
  const V3 n1 = cross(b1, b2), n2 = cross(b2, b3);
  x = dot(n1, n2);
  y = sqrt(dot(b2, b2)) * dot(b1, n2);
  return isfinite(x) && isfinite(y) && !(x == 0.0 && y == 0.0);
}

struct Torsions {
  double x[3], y[3];       // phi, psi, omega
  bool ok[3];
};

// what both kernels know of residue i of one frame
__device__ __forceinline__ Torsions residue_xy(const Residue& prev, const Residue& cur, const Residue& next, double brk) {
  Torsions t;
  const bool link_prev = prev.present && cur.present && sqrt(dot(sub(cur.n, prev.c), sub(cur.n, prev.c))) <= brk;
  const bool link_next = cur.present && next.present && sqrt(dot(sub(next.n, cur.c), sub(next.n, cur.c))) <= brk;
  t.x[0] = t.x[1] = t.x[2] = t.y[0] = t.y[1] = t.y[2] = 0.0;
  t.ok[0] = link_prev && dihedral_xy(prev.c, cur.n, cur.ca, cur.c, t.x[0], t.y[0]);
  t.ok[1] = link_next && dihedral_xy(cur.n, cur.ca, cur.c, next.n, t.x[1], t.y[1]);
  t.ok[2] = link_next && dihedral_xy(cur.ca, cur.c, next.n, next.ca, t.x[2], t.y[2]);
  return t;
}

// the angle at `mid` between the bonds to a and b
__device__ __forceinline__ double bond_angle(const V3& a, const V3& mid, const V3& b) {
  const V3 u = sub(a, mid), v = sub(b, mid), w = cross(u, v);
  return atan2(sqrt(dot(w, w)), dot(u, v));
}

__device__ __forceinline__ int bin_of(double angle, int bins) {
  const double deg = angle * DEG, w = 360.0 / bins;
  int b = (int)floor((deg + 180.0) / w);
  if (b >= bins) b -= bins;
  if (b < 0) b += bins;
  return min(max(b, 0), bins - 1);          // nothing reaches this with atan2 in [-pi, pi]; the cell stays inside the array whatever
}

struct TorArgs {
  const double* X;
  const uint8_t* mask;
  double *phi, *psi, *omega, *geom;
  double brk;
  int64_t rows;                              // n L
  int L, atoms;
};

__global__ __launch_bounds__(TOR_THREADS) void torsions_kernel(const TorArgs p) {
  const int64_t row = (int64_t)blockIdx.x * TOR_THREADS + threadIdx.x;
  if (row >= p.rows) return;
  const int i = (int)(row % p.L);
  const Residue cur = load_residue(p.X, p.mask, row, p.atoms);
  const Residue prev = i > 0 ? load_residue(p.X, p.mask, row - 1, p.atoms) : absent();
  const Residue next = i + 1 < p.L ? load_residue(p.X, p.mask, row + 1, p.atoms) : absent();
  const Torsions t = residue_xy(prev, cur, next, p.brk);
  p.phi[row] = t.ok[0] ? atan2(t.y[0], t.x[0]) : quiet_nan();
  p.psi[row] = t.ok[1] ? atan2(t.y[1], t.x[1]) : quiet_nan();
  p.omega[row] = t.ok[2] ? atan2(t.y[2], t.x[2]) : quiet_nan();
  if (p.geom) {
    double* g = p.geom + row * 6;
    const bool two = cur.present && next.present;
    const V3 nca = sub(cur.ca, cur.n), cac = sub(cur.c, cur.ca), cn = sub(next.n, cur.c);
    g[0] = cur.present ? sqrt(dot(nca, nca)) : quiet_nan();
    g[1] = cur.present ? sqrt(dot(cac, cac)) : quiet_nan();
    g[2] = two ? sqrt(dot(cn, cn)) : quiet_nan();
    g[3] = cur.present ? bond_angle(cur.n, cur.ca, cur.c) : quiet_nan();
    g[4] = two ? bond_angle(cur.ca, cur.c, next.n) : quiet_nan();
    g[5] = two ? bond_angle(cur.c, next.n, next.ca) : quiet_nan();
  }
}

struct RamaArgs {
  const double* X;
  const uint8_t* mask;
  int32_t *hist, *counts;
  double *sums, *part;                       // part: [chunks][L][6], used when chunks > 1
  double brk;
  int n, L, atoms, bins, frames, chunks;
};

template <bool SUMS>
__global__ __launch_bounds__(TOR_THREADS) void rama_kernel(const RamaArgs p) {
  const int64_t t = (int64_t)blockIdx.x * TOR_THREADS + threadIdx.x;
  if (t >= (int64_t)p.L * p.chunks) return;
  const int i = (int)(t % p.L), chunk = (int)(t / p.L);
  const int f_begin = chunk * p.frames, f_end = (int)min((int64_t)p.n, (int64_t)f_begin + p.frames);   // (chunks - 1) frames < n
  const bool has_prev = i > 0, has_next = i + 1 < p.L;
  int32_t* cells = p.hist + (int64_t)i * p.bins * p.bins;

  int cnt[5] = {0, 0, 0, 0, 0};              // phi, psi, both, omega, cis
  double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int f = f_begin; f < f_end; ++f) {
    const int64_t row = (int64_t)f * p.L + i;
    const Residue cur = load_residue(p.X, p.mask, row, p.atoms);
    const Residue prev = has_prev ? load_residue(p.X, p.mask, row - 1, p.atoms) : absent();
    const Residue next = has_next ? load_residue(p.X, p.mask, row + 1, p.atoms) : absent();
    const Torsions a = residue_xy(prev, cur, next, p.brk);
    if (SUMS) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        if (a.ok[k]) {
          const double r = sqrt(a.x[k] * a.x[k] + a.y[k] * a.y[k]);
          const double co = a.x[k] / r, si = a.y[k] / r;
          const bool first = cnt[k == 2 ? 3 : k] == 0;     // the sum starts from its first term
          s[2 * k] = first ? co : s[2 * k] + co;
          s[2 * k + 1] = first ? si : s[2 * k + 1] + si;
        }
      }
    }
    cnt[0] += a.ok[0] ? 1 : 0;
    cnt[1] += a.ok[1] ? 1 : 0;
    cnt[3] += a.ok[2] ? 1 : 0;
    cnt[4] += (a.ok[2] && a.x[2] > 0.0) ? 1 : 0;
    if (a.ok[0] && a.ok[1]) {
      ++cnt[2];
      const int bp = bin_of(atan2(a.y[0], a.x[0]), p.bins), bq = bin_of(atan2(a.y[1], a.x[1]), p.bins);
      atomicAdd(&cells[bp * p.bins + bq], 1);
    }
  }
#pragma unroll
  for (int k = 0; k < 5; ++k)
    if (cnt[k]) atomicAdd(&p.counts[(int64_t)i * 5 + k], cnt[k]);
  if (SUMS) {
    double* out = p.chunks == 1 ? p.sums + (int64_t)i * 6 : p.part + ((int64_t)chunk * p.L + i) * 6;
#pragma unroll
    for (int k = 0; k < 6; ++k) out[k] = s[k];
  }
}

__global__ __launch_bounds__(TOR_THREADS) void rama_fold_kernel(const RamaArgs p) {
  const int64_t e = (int64_t)blockIdx.x * TOR_THREADS + threadIdx.x;      // (residue, sum)
  const int64_t step = (int64_t)p.L * 6;
  if (e >= step) return;
  double s = p.part[e];
  int c = 1;
  for (; c + 16 <= p.chunks; c += 16) {                                    // 16 loads in flight, added in increasing chunk index
    double v[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = p.part[e + (c + j) * step];
#pragma unroll
    for (int j = 0; j < 16; ++j) s += v[j];
  }
  for (; c < p.chunks; ++c) s += p.part[e + c * step];
  p.sums[e] = s;
}

bool bad_common(const double* X, int32_t n, int32_t L, int32_t atoms, double brk) {
  return !X || n < 0 || L < 1 || (atoms != 3 && atoms != 4) || !(brk > 0.0) || !std::isfinite(brk);
}

}  // namespace
}  // namespace ed

using namespace ed;

extern "C" {

int esmdiff_backbone_torsions(const double* X, int32_t n, int32_t L, int32_t atoms, const uint8_t* mask, double break_distance,
                              double* phi, double* psi, double* omega, double* geom, void* stream) {
  if (bad_common(X, n, L, atoms, break_distance) || !phi || !psi || !omega) return ESMDIFF_E_INVALID;
  if (n == 0) return 0;
  TorArgs p;
  p.X = X, p.mask = mask, p.phi = phi, p.psi = psi, p.omega = omega, p.geom = geom;
  p.brk = break_distance, p.rows = (int64_t)n * L, p.L = L, p.atoms = atoms;
  const int64_t blocks = (p.rows + TOR_THREADS - 1) / TOR_THREADS;
  if (blocks > INT32_MAX) return ESMDIFF_E_CAPACITY;       // grid.x
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(torsions_kernel, dim3((unsigned)blocks), dim3(TOR_THREADS), 0, st, p);
  return finish_entry(st);
}

int esmdiff_ramachandran(const double* X, int32_t n, int32_t L, int32_t atoms, const uint8_t* mask, double break_distance,
                         int32_t bins, int32_t* hist, int32_t* counts, double* sums, void* scratch, int64_t scratch_bytes,
                         void* stream) {
  if (bad_common(X, n, L, atoms, break_distance) || !hist || !counts || bins < 1) return ESMDIFF_E_INVALID;
  if (bins > ESMDIFF_RAMA_MAX_BINS) return ESMDIFF_E_CAPACITY;
  const int chunks = (int)ESMDIFF_RAMA_CHUNKS(n, L);
  const int64_t need = sums ? ESMDIFF_RAMA_SCRATCH_BYTES(n, L) : 0;
  if (need > 0 && (!scratch || scratch_bytes < need)) return ESMDIFF_E_CAPACITY;

  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(hist, 0, (size_t)L * bins * bins * sizeof(int32_t), st) != hipSuccess) return ESMDIFF_E_HIP;
  if (hipMemsetAsync(counts, 0, (size_t)L * 5 * sizeof(int32_t), st) != hipSuccess) return ESMDIFF_E_HIP;
  if (n == 0) {
    if (sums && hipMemsetAsync(sums, 0, (size_t)L * 6 * sizeof(double), st) != hipSuccess) return ESMDIFF_E_HIP;
    return finish_entry(st);
  }
  RamaArgs p;
  p.X = X, p.mask = mask, p.hist = hist, p.counts = counts, p.sums = sums, p.part = (double*)scratch;
  p.brk = break_distance, p.n = n, p.L = L, p.atoms = atoms, p.bins = bins;
  p.frames = (int)ESMDIFF_RAMA_CHUNK_FRAMES(n, L), p.chunks = chunks;
  const int64_t blocks = ((int64_t)L * chunks + TOR_THREADS - 1) / TOR_THREADS;    // L chunks <= 65536 + L
  if (blocks > INT32_MAX) return ESMDIFF_E_CAPACITY;
  hipLaunchKernelGGL(sums ? rama_kernel<true> : rama_kernel<false>, dim3((unsigned)blocks), dim3(TOR_THREADS), 0, st, p);
  if (sums && chunks > 1)
    hipLaunchKernelGGL(rama_fold_kernel, dim3((unsigned)(((int64_t)L * 6 + TOR_THREADS - 1) / TOR_THREADS)), dim3(TOR_THREADS), 0, st, p);
  return finish_entry(st);
}

}  // extern "C"

// dssp.hip — secondary structure of backbones (N, CA, C, O) on the device after Kabsch & Sander 1983: float64 geometry in, hydrogen
// bonds, INTEGER state codes and their per-residue counts out.  DESIGN.md §3.22 states the definition; tests/dssp_ref.py restates it
// in numpy, twice.  [DSSP-RECALL]: the `mkdssp` program is not pinned (no bulges, no rounding of energies, the classic priority).
//
//   present[i]   mask[i] and N, CA, C finite            brk[j] = 0 iff present[j-1], present[j], |C[j-1] - N[j]| <= 2.5   (brk[0] = 1)
//   accept[i]    present[i] and O[i] finite             donate[j] iff brk[j] == 0, accept[j-1], not no_donor[j]
//   H[j]         N[j] + (C[j-1] - O[j-1]) / |C[j-1] - O[j-1]|
//   E(i, j)      27.888 (((1/|O_i N_j| + 1/|C_i H_j|) - 1/|O_i H_j|) - 1/|C_i N_j|) for i != j, i != j-1, |CA_i CA_j| < 9; a distance
//                under 0.5 gives -9.9, and so does an E below -9.9
//   acceptor[j]  the two i of lowest E among those with E < -0.5, ordered by (E, i); an empty slot holds -1 and energy 0.0
// A distance is sqrt((dx dx + dy dy) + dz dz) in float64 with the correctly rounded square root and division and no contraction into
// FMAs (the unit is compiled with -ffp-contract=off), so every energy has numpy's bits.
//
//   dssp_hbond_kernel    grid (structures, chunks of donors), 8 waves.  The acceptor side of the structure (CA, C, O as float64
//                        planes, 72 B per residue) is staged in LDS one tile of <= DSSP_TILE residues at a time, a residue that cannot
//                        accept with NaN in its CA: the CA prefilter is false for it and no mask is read in the inner loop.  The
//                        donor side (N, CA and H of ONE residue) is wave-uniform and lives in registers, so no H plane is staged.  A
//                        wave owns donor j; its lanes run over the tile's i 64 at a time and each keeps its two best (E, i); one
//                        butterfly of those pairs, ordered by (E, i), leaves the wave's two best in every lane.  A chain longer than
//                        one tile takes the tiles in turn: lane 0 starts a later tile from what the wave wrote after the one before
//                        (the order (E, i) is total, so the result does not depend on the tiling).  No floating-point atomics.
//   dssp_assign_kernel   one workgroup per structure.  acceptor[L][2], brk, present, the turn bits and the codes sit in LDS; the
//                        passes (a) .. (g) of §3.22 are separated by barriers and each writes only values that every concurrent
//                        writer agrees on.  Bridges need no L x L array: a partner of i is one of acceptor[i][s], acceptor[i][s] + 1,
//                        acceptor[i+1][s], acceptor[i+1][s] + 1, and the ladder test evaluates the bridge predicate at the
//                        neighbouring pair.  O(L) work per structure.  counts [L, 8] are integer atomics into a table the entry
//                        zeroed: two runs are bit-identical.
#include <math.h>

#include "ed_f64.h"
#include "kernels.h"

namespace ed {
namespace {

constexpr int DSSP_THREADS = 512, DSSP_WAVES = DSSP_THREADS / 64;
constexpr int DSSP_TILE = 2048;                      // acceptors staged at a time: 9 planes of float64 = 144 KiB of the CU's 160 KiB
constexpr int DSSP_ASSIGN_THREADS = 256;
constexpr int DSSP_NONE = 0x7fffffff;                // the index of an empty slot while ordering: after every residue
enum { SS_LOOP = 0, SS_S, SS_T, SS_I, SS_G, SS_B, SS_E, SS_H };

struct DsspArgs {
  const double* X;
  const uint8_t *mask, *no_donor;
  uint8_t* ss;
  int32_t *counts, *acceptor;
  double* energy;
  int n, L;
};

__device__ __forceinline__ bool finite3(const double* p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

// x: the structure's [L][4][3]; mk: its mask row or null
__device__ __forceinline__ bool present_at(const double* x, const uint8_t* mk, int i) {
  if (mk && !mk[i]) return false;
  const double* r = x + (int64_t)i * 12;
  return finite3(r) && finite3(r + 3) && finite3(r + 6);
}

// j >= 1
__device__ __forceinline__ bool break_before(const double* x, const uint8_t* mk, int j) {
  if (!present_at(x, mk, j - 1) || !present_at(x, mk, j)) return true;
  const double *c = x + (int64_t)(j - 1) * 12 + 6, *nn = x + (int64_t)j * 12;
  return !(dist(c[0] - nn[0], c[1] - nn[1], c[2] - nn[2]) <= 2.5);
}

struct Best {
  double e0, e1;
  int i0, i1;
};

__device__ __forceinline__ bool before(double ea, int ia, double eb, int ib) { return ea < eb || (ea == eb && ia < ib); }

__device__ __forceinline__ void insert(Best& b, double e, int i) {
  if (before(e, i, b.e0, b.i0)) {
    b.e1 = b.e0, b.i1 = b.i0;
    b.e0 = e, b.i0 = i;
  } else if (before(e, i, b.e1, b.i1)) {
    b.e1 = e, b.i1 = i;
  }
}

// grid (n, chunks).  Dynamic LDS: f64 [9][tile], tile = min(L, DSSP_TILE): CA x y z, C x y z, O x y z.
__global__ __launch_bounds__(DSSP_THREADS) void dssp_hbond_kernel(const DsspArgs p) {
  extern __shared__ double s_acc[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int L = p.L, tile = min(L, DSSP_TILE);
  const double* x = p.X + (int64_t)blockIdx.x * L * 12;
  const uint8_t* mk = p.mask ? p.mask + (int64_t)blockIdx.x * L : nullptr;
  int32_t* acc_out = p.acceptor + (int64_t)blockIdx.x * L * 2;
  double* en_out = p.energy + (int64_t)blockIdx.x * L * 2;
  const double inf = __longlong_as_double(0x7ff0000000000000ll), nan = quiet_nan();

  for (int t0 = 0; t0 < L; t0 += tile) {
    const int tl = min(tile, L - t0);
    __syncthreads();                                             // the waves are done with the tile before
    for (int r = tid; r < tl; r += DSSP_THREADS) {
      const double* src = x + (int64_t)(t0 + r) * 12;
      const bool accepts = present_at(x, mk, t0 + r) && finite3(src + 9);
#pragma unroll
      for (int c = 0; c < 9; ++c) s_acc[c * tile + r] = accepts ? src[3 + c] : nan;
    }
    __syncthreads();

    for (int j = blockIdx.y * DSSP_WAVES + wave; j < L; j += DSSP_WAVES * gridDim.y) {   // j is the same in every lane of the wave
      bool donates = j >= 1 && !(p.no_donor && p.no_donor[j]) && !break_before(x, mk, j);
      if (donates) donates = finite3(x + (int64_t)(j - 1) * 12 + 9);                     // j-1 is present: it accepts iff its O is finite
      if (!donates) {
        if (t0 == 0 && lane < 2) acc_out[2 * j + lane] = -1, en_out[2 * j + lane] = 0.0;
        continue;
      }
      const double *rj = x + (int64_t)j * 12, *rp = x + (int64_t)(j - 1) * 12;
      const double nx = rj[0], ny = rj[1], nz = rj[2], ax = rj[3], ay = rj[4], az = rj[5];
      const double cox = rp[6] - rp[9], coy = rp[7] - rp[10], coz = rp[8] - rp[11];
      const double co = dist(cox, coy, coz);
      const double hx = nx + cox / co, hy = ny + coy / co, hz = nz + coz / co;

      Best b = {inf, inf, DSSP_NONE, DSSP_NONE};
      if (t0 > 0 && lane == 0) {                                 // what this wave found in the tiles before
        if (acc_out[2 * j] >= 0) b.e0 = en_out[2 * j], b.i0 = acc_out[2 * j];
        if (acc_out[2 * j + 1] >= 0) b.e1 = en_out[2 * j + 1], b.i1 = acc_out[2 * j + 1];
      }
      for (int r0 = 0; r0 < tl; r0 += 64) {
        const int r = r0 + lane, i = t0 + r;
        if (r >= tl || i == j || i == j - 1) continue;
        const double cax = s_acc[r], cay = s_acc[tile + r], caz = s_acc[2 * tile + r];
        if (!(dist(cax - ax, cay - ay, caz - az) < 9.0)) continue;                      // NaN for a residue that cannot accept
        const double cx = s_acc[3 * tile + r], cy = s_acc[4 * tile + r], cz = s_acc[5 * tile + r];
        const double ox = s_acc[6 * tile + r], oy = s_acc[7 * tile + r], oz = s_acc[8 * tile + r];
        const double d_on = dist(ox - nx, oy - ny, oz - nz), d_ch = dist(cx - hx, cy - hy, cz - hz);
        const double d_oh = dist(ox - hx, oy - hy, oz - hz), d_cn = dist(cx - nx, cy - ny, cz - nz);
        double e;
        if (d_on < 0.5 || d_ch < 0.5 || d_oh < 0.5 || d_cn < 0.5) {
          e = -9.9;
        } else {
          e = 27.888 * (((1.0 / d_on + 1.0 / d_ch) - 1.0 / d_oh) - 1.0 / d_cn);
          if (e < -9.9) e = -9.9;
        }
        if (e < -0.5) insert(b, e, i);
      }
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {                  // the lanes' residues are disjoint; every lane ends with the wave's two
        const double oe0 = __shfl_xor(b.e0, off, 64), oe1 = __shfl_xor(b.e1, off, 64);
        const int oi0 = __shfl_xor(b.i0, off, 64), oi1 = __shfl_xor(b.i1, off, 64);
        insert(b, oe0, oi0);
        insert(b, oe1, oi1);
      }
      if (lane == 0) {
        acc_out[2 * j] = b.i0 == DSSP_NONE ? -1 : b.i0, en_out[2 * j] = b.i0 == DSSP_NONE ? 0.0 : b.e0;
        acc_out[2 * j + 1] = b.i1 == DSSP_NONE ? -1 : b.i1, en_out[2 * j + 1] = b.i1 == DSSP_NONE ? 0.0 : b.e1;
      }
    }
  }
}

// One workgroup per structure.  Dynamic LDS: i32 [L][2] acceptors, then u8 [L] each of brk, present, turn bits (1 << (n - 3)), codes.
__global__ __launch_bounds__(DSSP_ASSIGN_THREADS) void dssp_assign_kernel(const DsspArgs p) {
  extern __shared__ int s_hb[];
  const int L = p.L, tid = threadIdx.x;
  uint8_t* s_brk = (uint8_t*)(s_hb + 2 * L);
  uint8_t *s_present = s_brk + L, *s_turn = s_present + L, *s_ss = s_turn + L;
  const double* x = p.X + (int64_t)blockIdx.x * L * 12;
  const uint8_t* mk = p.mask ? p.mask + (int64_t)blockIdx.x * L : nullptr;
  const int32_t* acc = p.acceptor + (int64_t)blockIdx.x * L * 2;

  for (int i = tid; i < L; i += DSSP_ASSIGN_THREADS) {
    s_hb[2 * i] = acc[2 * i], s_hb[2 * i + 1] = acc[2 * i + 1];
    s_present[i] = present_at(x, mk, i);
    s_brk[i] = i == 0 || break_before(x, mk, i);
    s_ss[i] = SS_LOOP;
  }
  __syncthreads();

  auto hb = [&](int i, int j) { return i >= 0 && i < L && j >= 0 && j < L && (s_hb[2 * j] == i || s_hb[2 * j + 1] == i); };
  auto contiguous = [&](int a, int b) {                          // 0 <= a, b < L
    for (int k = a + 1; k <= b; ++k)
      if (s_brk[k]) return false;
    return true;
  };
  auto inner = [&](int i) { return i >= 1 && i <= L - 2 && !s_brk[i] && !s_brk[i + 1]; };
  auto pair_ok = [&](int i, int j) { return inner(i) && inner(j) && (i > j ? i - j : j - i) >= 3; };
  auto parallel = [&](int i, int j) { return pair_ok(i, j) && ((hb(i - 1, j) && hb(j, i + 1)) || (hb(j - 1, i) && hb(i, j + 1))); };
  auto antiparallel = [&](int i, int j) { return pair_ok(i, j) && ((hb(i, j) && hb(j, i)) || (hb(i - 1, j + 1) && hb(j - 1, i + 1))); };

  // turns, and (a): bridges and ladders
  for (int i = tid; i < L; i += DSSP_ASSIGN_THREADS) {
    int t = 0;
#pragma unroll
    for (int n = 3; n <= 5; ++n)
      if (i + n < L && hb(i, i + n) && contiguous(i, i + n)) t |= 1 << (n - 3);
    s_turn[i] = t;
    int code = SS_LOOP;
    for (int c = 0; c < 8; ++c) {                                // the eight residues that can be a partner of i
      const int d = i + (c >> 2);
      if (d >= L) break;
      const int a = s_hb[2 * d + (c & 1)];
      if (a < 0) continue;
      const int j = a + ((c >> 1) & 1);
      if (parallel(i, j)) {
        if (code < SS_B) code = SS_B;
        if (parallel(i - 1, j - 1) || parallel(i + 1, j + 1)) code = SS_E;
      }
      if (antiparallel(i, j)) {
        if (code < SS_B) code = SS_B;
        if (antiparallel(i - 1, j + 1) || antiparallel(i + 1, j - 1)) code = SS_E;
      }
    }
    s_ss[i] = code;
  }
  __syncthreads();

  // (b) H over E / B; (c) G, (d) I only over loop.  A stretch starts at i >= 1 with turn_n(i-1) and turn_n(i), so i + n < L.
  for (int i = tid + 1; i < L; i += DSSP_ASSIGN_THREADS)
    if (s_turn[i - 1] & s_turn[i] & 2)
      for (int k = 0; k < 4; ++k) s_ss[i + k] = SS_H;
  __syncthreads();
#pragma unroll
  for (int n = 3; n <= 5; n += 2) {
    const int bit = 1 << (n - 3), code = n == 3 ? SS_G : SS_I;
    for (int i = tid + 1; i < L; i += DSSP_ASSIGN_THREADS) {
      if (!(s_turn[i - 1] & s_turn[i] & bit)) continue;
      bool free_ = true;
      for (int k = 0; k < n; ++k) free_ = free_ && (s_ss[i + k] == SS_LOOP || s_ss[i + k] == code);   // `code`: a neighbour's write of this pass
      if (free_)
        for (int k = 0; k < n; ++k) s_ss[i + k] = code;
    }
    __syncthreads();
  }

  // (e) T inside every turn, where still loop
  for (int i = tid; i < L; i += DSSP_ASSIGN_THREADS) {
    const int t = s_turn[i];
#pragma unroll
    for (int n = 3; n <= 5; ++n)
      if (t & (1 << (n - 3)))
        for (int k = i + 1; k < i + n; ++k)
          if (s_ss[k] == SS_LOOP) s_ss[k] = SS_T;
  }
  __syncthreads();

  // (f) S, (g) absent residues, the outputs
  for (int i = tid; i < L; i += DSSP_ASSIGN_THREADS) {
    int code = s_ss[i];
    if (code == SS_LOOP && i >= 2 && i <= L - 3 && contiguous(i - 2, i + 2)) {
      const double *a = x + (int64_t)(i - 2) * 12 + 3, *b = x + (int64_t)i * 12 + 3, *c = x + (int64_t)(i + 2) * 12 + 3;
      const double ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2], vx = c[0] - b[0], vy = c[1] - b[1], vz = c[2] - b[2];
      const double cosine = ((ux * vx + uy * vy) + uz * vz) / sqrt(((ux * ux + uy * uy) + uz * uz) * ((vx * vx + vy * vy) + vz * vz));
      if (cosine < 0.3420201433256687) code = SS_S;
    }
    if (!s_present[i]) code = SS_LOOP;
    p.ss[(int64_t)blockIdx.x * L + i] = (uint8_t)code;
    if (p.counts && s_present[i]) atomicAdd(&p.counts[8 * i + code], 1);
  }
}

}  // namespace
}  // namespace ed

using namespace ed;

extern "C" {

int esmdiff_dssp(const double* X, int32_t n, int32_t L, const uint8_t* mask, const uint8_t* no_donor, uint8_t* ss, int32_t* counts,
                 int32_t* acceptor, double* energy, void* stream) {
  if (n < 0 || L < 1 || L > ESMDIFF_DSSP_MAX_L || !ss || !acceptor || !energy || (n > 0 && !X)) return ESMDIFF_E_INVALID;
  hipStream_t st = (hipStream_t)stream;
  if (counts && hipMemsetAsync(counts, 0, (size_t)L * 8 * sizeof(int32_t), st) != hipSuccess) return ESMDIFF_E_HIP;
  if (n == 0) return finish_entry(st);

  DsspArgs p;
  p.X = X, p.mask = mask, p.no_donor = no_donor, p.ss = ss, p.counts = counts, p.acceptor = acceptor, p.energy = energy;
  p.n = n, p.L = L;
  // donors are split over workgroups only while the launch would leave CUs idle (each chunk stages the acceptors again)
  const int max_chunks = (L + DSSP_WAVES - 1) / DSSP_WAVES;
  const int chunks = std::max(1, std::min(max_chunks, 1024 / n));
  const int lds = 9 * (int)sizeof(double) * std::min((int)L, DSSP_TILE);
  if (ensure_dynamic_lds((const void*)dssp_hbond_kernel, lds) != hipSuccess) return ESMDIFF_E_HIP;
  hipLaunchKernelGGL(dssp_hbond_kernel, dim3((unsigned)n, chunks), dim3(DSSP_THREADS), (size_t)lds, st, p);
  if (hipGetLastError() != hipSuccess) return ESMDIFF_E_HIP;
  const int lds2 = 12 * L;
  if (ensure_dynamic_lds((const void*)dssp_assign_kernel, lds2) != hipSuccess) return ESMDIFF_E_HIP;
  hipLaunchKernelGGL(dssp_assign_kernel, dim3((unsigned)n), dim3(DSSP_ASSIGN_THREADS), (size_t)lds2, st, p);
  return finish_entry(st);
}

}  // extern "C"

// contacts.hip — contact maps of an ensemble and native-contact counts of models against natives on the device: float64 distances,
// INTEGER counts, float64 sums in a fixed order.  DESIGN.md §3.23 states the definitions; tests/contacts_ref.py restates them in numpy.
//
// A distance is sqrt((dx dx + dy dy) + dz dz) in float64 with the correctly rounded square root and no contraction into FMAs (the
// unit is compiled with -ffp-contract=off), so every comparison falls as numpy's does.  No float atomics anywhere.
//
//   contact_map_kernel     one WORKGROUP of 256 threads per (64 x 64 tile of the upper triangle of tiles, chunk of frames).  Thread
//                          (ty, tx) of the 16 x 16 grid owns the 4 x 4 pairs a = a0 + ty + 16 i, b = b0 + tx + 16 j: per pair two integer
//                          counters (valid, contact) and two float64 sums (d, d d) in registers.  The tile's two coordinate strips are
//                          staged through LDS 8 frames at a time as planes x[64], y[64], z[64]; a residue that is masked, or past the
//                          end of the chain, is staged as NaN, and a pair whose distance is NaN is not valid in that frame: no mask is
//                          read in the inner loop.  The a-strip reads are broadcasts, the b-strip reads 16 consecutive doubles per
//                          half wave: no bank conflict.  A diagonal tile computes both of its triangles.
//                          Frames f of chunk c are c F .. min(n, (c + 1) F) - 1, F = ESMDIFF_CONTACT_CHUNK_FRAMES(n, L), added one
//                          after another in increasing f; a frame in which the pair is not valid adds nothing.
//                          One chunk: the workgroup writes its tile and the mirrored tile straight to the outputs, no scratch.
//                          More chunks: it writes its partial tile to the scratch, and
//   contact_fold_kernel    one thread per element (a, b) of the L x L maps adds the chunk partials in increasing chunk index
//                          (s = part[0]; s += part[1]; ...), reading the tile of (min, max) for the lower triangle.
//                          Both write 0 where |a - b| < min_sep.
//   native_contacts_kernel the native-pair scan of ed_native_pairs.h, the layout of lddt_pairs_kernel, with the contacts policy: the pair
//                          filter is min_sep and cutoff, the ring holds lambda d0 (one product), and a pair is kept when d < lambda d0.
//                          q_soft (SOFT = true) is the scan's float64 sum of 1 / (1 + exp(beta (d - lambda d0))), a pair whose model
//                          residue is missing adding 0, summed without atomics in the order stated there: lanes, butterfly, rows
//                          a = w, w + 8, w + 16 ... per wave; the eight wave sums are then combined as
//                          ((w0 + w1) + (w2 + w3)) + ((w4 + w5) + (w6 + w7)).  With q_soft the rows are therefore never split over
//                          workgroups (one row chunk).
#include <math.h>

#include "ed_native_pairs.h"

namespace ed {
namespace {

constexpr int CM_TILE = ESMDIFF_CONTACT_TILE;          // 64 residues a side
constexpr int CM_THREADS = 256, CM_GRID = 16, CM_BLOCK = CM_TILE / CM_GRID;   // 16 x 16 threads, 4 x 4 pairs each
constexpr int CM_FRAMES = 8;                           // frames staged per barrier pair: 2 strips x 8 x 3 x 64 f64 = 24 KiB
constexpr int CM_CELLS = CM_TILE * CM_TILE;
static_assert(CM_BLOCK == 4 && CM_GRID * CM_GRID == CM_THREADS, "the thread grid covers the tile");

struct CmArgs {
  const double* X;
  const uint8_t* mask;
  int32_t *valid, *count;                              // the outputs (one chunk) ...
  double *sum_d, *sum_d2;
  int32_t *part_valid, *part_count;                    // ... or the partial tiles [chunks][pair tiles][64 x 64]
  double *part_d, *part_d2;
  double cutoff;
  int n, L, T, frames, chunks, min_sep;
};

// grid (pair tiles, chunks)
template <bool SUMS>
__global__ __launch_bounds__(CM_THREADS) void contact_map_kernel(const CmArgs p) {
  __shared__ double s_xyz[2][CM_FRAMES][3][CM_TILE];
  const int tid = threadIdx.x, tx = tid & (CM_GRID - 1), ty = tid >> 4;
  const int L = p.L;
  int ta = 0, rem = blockIdx.x;                        // pair tile index -> (ta <= tb), rows of the triangle one after another
  while (rem >= p.T - ta) rem -= p.T - ta, ++ta;
  const int tb = ta + rem;
  const int base[2] = {ta * CM_TILE, tb * CM_TILE};
  const int f_begin = blockIdx.y * p.frames, f_end = min(p.n, f_begin + p.frames);

  int valid[CM_BLOCK][CM_BLOCK], count[CM_BLOCK][CM_BLOCK];
  double sd[CM_BLOCK][CM_BLOCK], sd2[CM_BLOCK][CM_BLOCK];
#pragma unroll
  for (int i = 0; i < CM_BLOCK; ++i)
#pragma unroll
    for (int j = 0; j < CM_BLOCK; ++j) valid[i][j] = 0, count[i][j] = 0, sd[i][j] = 0.0, sd2[i][j] = 0.0;

  for (int f0 = f_begin; f0 < f_end; f0 += CM_FRAMES) {
    const int nf = min(CM_FRAMES, f_end - f0);
    __syncthreads();                                   // the previous batch has been consumed
    for (int e = tid; e < 2 * CM_FRAMES * 3 * CM_TILE; e += CM_THREADS) {
      const int strip = e / (CM_FRAMES * 3 * CM_TILE), within = e - strip * (CM_FRAMES * 3 * CM_TILE);
      const int f = within / (3 * CM_TILE), q = within - f * (3 * CM_TILE);
      const int r = q / 3, c = q - 3 * r;
      const int res = base[strip] + r;
      if (f < nf) {
        const int64_t row = (int64_t)(f0 + f) * L + res;
        const bool there = res < L && (!p.mask || p.mask[row]);
        s_xyz[strip][f][c][r] = there ? p.X[row * 3 + c] : quiet_nan();
      }
    }
    __syncthreads();
    for (int f = 0; f < nf; ++f) {
      double a[CM_BLOCK][3], b[CM_BLOCK][3];
#pragma unroll
      for (int i = 0; i < CM_BLOCK; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) a[i][c] = s_xyz[0][f][c][ty + CM_GRID * i], b[i][c] = s_xyz[1][f][c][tx + CM_GRID * i];
#pragma unroll
      for (int i = 0; i < CM_BLOCK; ++i)
#pragma unroll
        for (int j = 0; j < CM_BLOCK; ++j) {
          const double dx = b[j][0] - a[i][0], dy = b[j][1] - a[i][1], dz = b[j][2] - a[i][2];
          const double d2 = sq3(dx, dy, dz);
          const double d = sqrt(d2);
          const bool ok = d == d;                      // NaN: a residue of the pair is missing in this frame
          valid[i][j] += ok ? 1 : 0;
          count[i][j] += d < p.cutoff ? 1 : 0;         // false for NaN
          if (SUMS) sd[i][j] += ok ? d : 0.0, sd2[i][j] += ok ? d2 : 0.0;   // + 0.0 leaves a sum of non-negative terms as it is
        }
    }
  }

  const bool direct = p.chunks == 1;
#pragma unroll
  for (int i = 0; i < CM_BLOCK; ++i)
#pragma unroll
    for (int j = 0; j < CM_BLOCK; ++j) {
      const int ra = ty + CM_GRID * i, rb = tx + CM_GRID * j;
      if (!direct) {                                   // the scratch holds whole tiles: no bound to check
        const int64_t at = ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * CM_CELLS + ra * CM_TILE + rb;
        p.part_valid[at] = valid[i][j], p.part_count[at] = count[i][j];
        if (SUMS) p.part_d[at] = sd[i][j], p.part_d2[at] = sd2[i][j];
        continue;
      }
      const int ga = base[0] + ra, gb = base[1] + rb;
      if (ga >= L || gb >= L) continue;
      const bool zero = (ga > gb ? ga - gb : gb - ga) < p.min_sep;
      const int v = zero ? 0 : valid[i][j], k = zero ? 0 : count[i][j];
      const double s1 = zero ? 0.0 : sd[i][j], s2 = zero ? 0.0 : sd2[i][j];
      const int64_t at = (int64_t)ga * L + gb, mirrored = (int64_t)gb * L + ga;
      p.valid[at] = v, p.count[at] = k;
      if (SUMS) p.sum_d[at] = s1, p.sum_d2[at] = s2;
      if (ta != tb) {                                  // a diagonal tile holds both of its triangles itself
        p.valid[mirrored] = v, p.count[mirrored] = k;
        if (SUMS) p.sum_d[mirrored] = s1, p.sum_d2[mirrored] = s2;
      }
    }
}

template <bool SUMS>
__global__ __launch_bounds__(256) void contact_fold_kernel(const CmArgs p) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int L = p.L;
  if (e >= (int64_t)L * L) return;
  const int a = (int)(e / L), b = (int)(e - (int64_t)a * L);
  int v = 0, k = 0;
  double s1 = 0.0, s2 = 0.0;
  if ((a > b ? a - b : b - a) >= p.min_sep) {
    const int lo = min(a, b), hi = max(a, b);          // the tile of (lo, hi) is in the upper triangle of tiles; a diagonal tile holds (a, b) itself
    const int ta = lo / CM_TILE, tb = hi / CM_TILE;
    const int ra = ta == tb ? a % CM_TILE : lo % CM_TILE, rb = ta == tb ? b % CM_TILE : hi % CM_TILE;
    const int64_t pairs = (int64_t)p.T * (p.T + 1) / 2;
    const int64_t tile = (int64_t)ta * p.T - (int64_t)ta * (ta - 1) / 2 + (tb - ta);
    const int64_t cell = tile * CM_CELLS + ra * CM_TILE + rb, step = pairs * CM_CELLS;
    v = p.part_valid[cell], k = p.part_count[cell];
    if (SUMS) s1 = p.part_d[cell], s2 = p.part_d2[cell];
    for (int c = 1; c < p.chunks; ++c) {               // increasing chunk index
      v += p.part_valid[cell + c * step], k += p.part_count[cell + c * step];
      if (SUMS) s1 += p.part_d[cell + c * step], s2 += p.part_d2[cell + c * step];
    }
  }
  p.valid[e] = v, p.count[e] = k;
  if (SUMS) p.sum_d[e] = s1, p.sum_d2[e] = s2;
}

// ---- native contacts -------------------------------------------------------------------------------------------------------------
static_assert(24 * ESMDIFF_CONTACT_MAX_L <= NP_MODEL_LDS, "one model of the longest chain fits");

struct NcArgs : NativePairArgs {
  int min_sep;                                           // first: with it last native_contacts_kernel<false> measured 1 - 1.6 % slower (EXPERIMENTS.md)
  double* q_soft;
  double cutoff, lambda, beta;
};

template <bool WITH_SOFT>
struct NcPolicy {
  static constexpr bool SOFT = WITH_SOFT;
  const NcArgs p;
  __device__ int min_sep() const { return p.min_sep; }
  __device__ double cutoff() const { return p.cutoff; }
  __device__ double payload(double d0) const { return p.lambda * d0; }   // one float64 product
  __device__ int score(double d, double ld, double& soft) const {
    if (SOFT) {
      const double term = 1.0 / (1.0 + exp(p.beta * (d - ld)));
      soft = d == d ? term : 0.0;
    }
    return d < ld ? 1 : 0;                                 // d is NaN for a masked model residue: never kept
  }
  // one row chunk: this workgroup saw every row of native j
  __device__ void finish(const double* sums, int i0, int tm, int j) const {
    __shared__ double s_q[NP_TILE][NP_WAVES];
    const int tid = threadIdx.x;
    if ((tid & 63) == 0) {
#pragma unroll
      for (int i = 0; i < NP_TILE; ++i) s_q[i][tid >> 6] = sums[i];
    }
    __syncthreads();
    if (tid < tm) p.q_soft[(int64_t)(i0 + tid) * p.m + j] = tree8(s_q[tid]);
  }
};

// one row chunk with SOFT
template <bool SOFT>
__global__ __launch_bounds__(NP_THREADS) void native_contacts_kernel(const NcArgs p) {
  native_pair_scan(p, NcPolicy<SOFT>{p});
}

}  // namespace
}  // namespace ed

using namespace ed;

extern "C" {

int esmdiff_contact_map(const double* X, int32_t n, int32_t L, const uint8_t* mask, double cutoff, int32_t min_sep, int32_t* valid,
                        int32_t* count, double* sum_d, double* sum_d2, void* scratch, int64_t scratch_bytes, void* stream) {
  if (!X || !valid || !count || n < 1 || L < 2 || min_sep < 1 || !(cutoff == cutoff)) return ESMDIFF_E_INVALID;
  if ((sum_d == nullptr) != (sum_d2 == nullptr)) return ESMDIFF_E_INVALID;
  if (L > ESMDIFF_CONTACT_MAX_L) return ESMDIFF_E_CAPACITY;
  const int chunks = ESMDIFF_CONTACT_CHUNKS(n, L);
  const int64_t need = ESMDIFF_CONTACT_SCRATCH_BYTES(n, L);
  if (need > 0 && (!scratch || scratch_bytes < need)) return ESMDIFF_E_CAPACITY;

  CmArgs p;
  p.X = X, p.mask = mask, p.valid = valid, p.count = count, p.sum_d = sum_d, p.sum_d2 = sum_d2;
  p.cutoff = cutoff, p.n = n, p.L = L, p.min_sep = min_sep;
  p.T = ESMDIFF_CONTACT_TILES(L), p.frames = ESMDIFF_CONTACT_CHUNK_FRAMES(n, L), p.chunks = chunks;
  const int64_t pair_tiles = ESMDIFF_CONTACT_PAIR_TILES(L), cells = pair_tiles * chunks * CM_CELLS;
  p.part_d = (double*)scratch, p.part_d2 = p.part_d + cells;               // f64 first: the scratch is 8-byte aligned
  p.part_valid = (int32_t*)(p.part_d2 + cells), p.part_count = p.part_valid + cells;

  hipStream_t st = (hipStream_t)stream;
  const bool sums = sum_d != nullptr;
  hipLaunchKernelGGL(sums ? contact_map_kernel<true> : contact_map_kernel<false>, dim3((unsigned)pair_tiles, (unsigned)chunks),
                     dim3(CM_THREADS), 0, st, p);
  if (chunks > 1) {
    const int64_t blocks = ((int64_t)L * L + 255) / 256;
    hipLaunchKernelGGL(sums ? contact_fold_kernel<true> : contact_fold_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, p);
  }
  return finish_entry(st);
}

int esmdiff_native_contacts(const double* A, int32_t n, const double* B, int32_t m, int32_t L, const uint8_t* maskA,
                            const uint8_t* maskB, double cutoff, int32_t min_sep, double lambda, double beta, int32_t* kept,
                            int32_t* total, int32_t* kept_res, int32_t* total_res, double* q_soft, void* stream) {
  if (!A || !kept || !total || n < 1 || L < 2 || min_sep < 1) return ESMDIFF_E_INVALID;
  if (!(cutoff == cutoff) || !(lambda == lambda) || !(beta == beta)) return ESMDIFF_E_INVALID;
  if (!B) B = A, m = n, maskB = maskA;
  if (m < 1) return ESMDIFF_E_INVALID;
  if (L > ESMDIFF_CONTACT_MAX_L) return ESMDIFF_E_CAPACITY;

  NcArgs p;
  p.A = A, p.B = B, p.maskA = maskA, p.maskB = maskB;
  p.kept = kept, p.total = total, p.kept_res = kept_res, p.total_res = total_res, p.q_soft = q_soft;
  p.cutoff = cutoff, p.lambda = lambda, p.beta = beta;
  p.n = n, p.m = m, p.L = L, p.min_sep = min_sep;
  // never split over row chunks with q_soft (its order of summation)
  return launch_native_pairs(q_soft ? native_contacts_kernel<true> : native_contacts_kernel<false>, p, !q_soft, (hipStream_t)stream);
}

}  // extern "C"

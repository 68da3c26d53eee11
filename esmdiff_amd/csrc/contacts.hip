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
//   native_contacts_kernel the layout of lddt_pairs_kernel: one WORKGROUP of 8 waves per (tile of <= 8 models, native j, chunk of rows),
//                          the tile staged in LDS as planes with masked residues as NaN, a wave per row a, the native's contacts of
//                          the row found 64 candidates at a time (one ballot) and compacted into the wave's ring as (b, lambda d0);
//                          full waves then score the ring against every model of the tile.  kept / total are zeroed by the entry and
//                          summed with integer atomics; the per-residue outputs have one writer each.
//                          q_soft (SOFT = true) is summed without atomics in this order, a function of L alone: the k-th contact of
//                          row a (increasing b) goes to lane k % 64, which adds its terms in increasing k; the 64 lane sums are
//                          combined by the xor butterfly of ed_wave.h (offsets 32, 16 .. 1); wave w adds the row sums of rows
//                          a = w, w + 8, w + 16 ... in that order; the eight wave sums are combined as
//                          ((w0 + w1) + (w2 + w3)) + ((w4 + w5) + (w6 + w7)).  With q_soft the rows are therefore never split over
//                          workgroups (one row chunk).  A pair whose model residue is missing adds 0.
#include <math.h>

#include "ed_wave.h"
#include "kernels.h"

namespace ed {
namespace {

typedef unsigned long long u64;

constexpr int CM_TILE = ESMDIFF_CONTACT_TILE;          // 64 residues a side
constexpr int CM_THREADS = 256, CM_GRID = 16, CM_BLOCK = CM_TILE / CM_GRID;   // 16 x 16 threads, 4 x 4 pairs each
constexpr int CM_FRAMES = 8;                           // frames staged per barrier pair: 2 strips x 8 x 3 x 64 f64 = 24 KiB
constexpr int CM_CELLS = CM_TILE * CM_TILE;
static_assert(CM_BLOCK == 4 && CM_GRID * CM_GRID == CM_THREADS, "the thread grid covers the tile");

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

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
          const double d2 = (dx * dx + dy * dy) + dz * dz;
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
constexpr int NC_TILE = 8;                             // models per workgroup
constexpr int NC_THREADS = 512, NC_WAVES = NC_THREADS / 64;
constexpr int NC_RING = 128;                           // pairs a wave can hold: fewer than 64 waiting + the 64 of one step
constexpr int NC_MODEL_LDS = 144 * 1024;               // dynamic LDS for the tile; the rings and the wave sums take 12.5 KiB of the CU's 160 KiB
static_assert(24 * ESMDIFF_CONTACT_MAX_L <= NC_MODEL_LDS, "one model of the longest chain fits");

struct NcArgs {
  const double *A, *B;
  const uint8_t *maskA, *maskB;
  int32_t *kept, *total, *kept_res, *total_res;
  double* q_soft;
  double cutoff, lambda, beta;
  int n, m, L, tile, tiles, min_sep;
};

__device__ __forceinline__ double dist(double dx, double dy, double dz) { return sqrt((dx * dx + dy * dy) + dz * dz); }

// grid (model tiles x m, row chunks; one row chunk with SOFT).  Dynamic LDS: f64 [tile][3][L].
template <bool SOFT>
__global__ __launch_bounds__(NC_THREADS) void native_contacts_kernel(const NcArgs p) {
  extern __shared__ double s_model[];
  __shared__ double s_ld[NC_WAVES][NC_RING];
  __shared__ int s_b[NC_WAVES][NC_RING];
  __shared__ double s_q[NC_WAVES][NC_TILE];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int L = p.L;
  const int first_tile = blockIdx.x % p.tiles == 0;        // the one tile of native j that reports the native's own counts
  const int j = blockIdx.x / p.tiles, i0 = (blockIdx.x % p.tiles) * p.tile;
  const int tm = min(p.tile, p.n - i0);

  for (int i = 0; i < tm; ++i) {
    const double* src = p.A + (int64_t)(i0 + i) * L * 3;
    const uint8_t* mk = p.maskA ? p.maskA + (int64_t)(i0 + i) * L : nullptr;
    for (int e = tid; e < 3 * L; e += NC_THREADS) {
      const int b = e / 3, c = e - 3 * b;
      s_model[(i * 3 + c) * L + b] = (mk && !mk[b]) ? quiet_nan() : src[e];
    }
  }
  __syncthreads();

  const double* Bj = p.B + (int64_t)j * L * 3;
  const uint8_t* mb = p.maskB ? p.maskB + (int64_t)j * L : nullptr;
  double* ring_ld = s_ld[wave];
  int* ring_b = s_b[wave];
  int ksum[NC_TILE] = {0, 0, 0, 0, 0, 0, 0, 0};
  double qsum[NC_TILE] = {0, 0, 0, 0, 0, 0, 0, 0};
  int tsum = 0;

  for (int a = blockIdx.y * NC_WAVES + wave; a < L; a += NC_WAVES * gridDim.y) {   // a is the same in every lane of the wave
    int acc[NC_TILE] = {0, 0, 0, 0, 0, 0, 0, 0};
    double qacc[NC_TILE] = {0, 0, 0, 0, 0, 0, 0, 0};
    int head = 0, waiting = 0, trow = 0;

    // every lane below `count` takes one waiting pair and scores it against the tile
    auto score = [&](int count) {
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      const bool on = lane < count;
      const int slot = (head + lane) & (NC_RING - 1);
      const int b = on ? ring_b[slot] : a;
      const double ld = on ? ring_ld[slot] : 0.0;
#pragma unroll
      for (int i = 0; i < NC_TILE; ++i) {
        if (i < tm) {
          const double* M = s_model + (i * 3) * L;
          const double d = dist(M[b] - M[a], M[L + b] - M[L + a], M[2 * L + b] - M[2 * L + a]);
          acc[i] += (on && d < ld) ? 1 : 0;                // d is NaN for a masked model residue: never kept
          if (SOFT) {
            const double term = 1.0 / (1.0 + exp(p.beta * (d - ld)));
            qacc[i] += (on && d == d) ? term : 0.0;
          }
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
    };

    if (!mb || mb[a]) {
      const double ax = Bj[3 * a], ay = Bj[3 * a + 1], az = Bj[3 * a + 2];
      for (int b0 = 0; b0 < L; b0 += 64) {
        const int b = b0 + lane;
        const int sep = a > b ? a - b : b - a;
        bool in = false;
        double d0 = 0.0;
        if (b < L && sep >= p.min_sep && (!mb || mb[b])) {
          d0 = dist(Bj[3 * b] - ax, Bj[3 * b + 1] - ay, Bj[3 * b + 2] - az);
          in = d0 < p.cutoff;
        }
        const u64 bits = __ballot(in);
        if (!bits) continue;
        if (in) {
          const int slot = (head + waiting + __popcll(bits & ((1ull << lane) - 1))) & (NC_RING - 1);
          ring_b[slot] = b;
          ring_ld[slot] = p.lambda * d0;                   // one float64 product
        }
        const int found = __popcll(bits);
        waiting += found;                                  // < 64 before, <= 127 now: the ring holds them
        trow += found;
        if (waiting >= 64) {
          score(64);
          head = (head + 64) & (NC_RING - 1);
          waiting -= 64;
        }
      }
      if (waiting > 0) score(waiting);
    }

#pragma unroll
    for (int i = 0; i < NC_TILE; ++i) {
      if (i < tm) {
        const int r = wave_sum(acc[i]);
        ksum[i] += r;
        if (SOFT) qsum[i] += wave_sum(qacc[i]);
        if (lane == 0 && p.kept_res) p.kept_res[((int64_t)(i0 + i) * p.m + j) * L + a] = r;
      }
    }
    tsum += trow;
    if (lane == 0 && first_tile && p.total_res) p.total_res[(int64_t)j * L + a] = trow;
  }

  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < NC_TILE; ++i)
      if (i < tm && ksum[i]) atomicAdd(&p.kept[(int64_t)(i0 + i) * p.m + j], ksum[i]);
    if (first_tile && tsum) atomicAdd(&p.total[j], tsum);
  }
  if (SOFT) {                                              // one row chunk: this workgroup saw every row of native j
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < NC_TILE; ++i) s_q[wave][i] = qsum[i];
    }
    __syncthreads();
    if (tid < tm)
      p.q_soft[(int64_t)(i0 + tid) * p.m + j] = ((s_q[0][tid] + s_q[1][tid]) + (s_q[2][tid] + s_q[3][tid])) +
                                                ((s_q[4][tid] + s_q[5][tid]) + (s_q[6][tid] + s_q[7][tid]));
  }
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
  p.tile = std::max(1, std::min(std::min(NC_TILE, (int)n), NC_MODEL_LDS / (24 * L)));
  const int tiles = p.tiles = (n + p.tile - 1) / p.tile;
  const int64_t groups = (int64_t)tiles * m;
  if (groups > INT32_MAX) return ESMDIFF_E_CAPACITY;       // grid.x
  // rows are split over workgroups only while the launch would leave CUs idle, and never with q_soft (its order of summation)
  const int max_chunks = (L + NC_WAVES - 1) / NC_WAVES;
  const int chunks = q_soft ? 1 : (int)std::max<int64_t>(1, std::min<int64_t>(max_chunks, 1024 / groups));
  const int lds = p.tile * 24 * L;

  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(kept, 0, (size_t)n * m * sizeof(int32_t), st) != hipSuccess) return ESMDIFF_E_HIP;
  if (hipMemsetAsync(total, 0, (size_t)m * sizeof(int32_t), st) != hipSuccess) return ESMDIFF_E_HIP;
  const auto kernel = q_soft ? native_contacts_kernel<true> : native_contacts_kernel<false>;
  if (ensure_dynamic_lds((const void*)kernel, lds) != hipSuccess) return ESMDIFF_E_HIP;
  hipLaunchKernelGGL(kernel, dim3((unsigned)groups, chunks), dim3(NC_THREADS), (size_t)lds, st, p);
  return finish_entry(st);
}

}  // extern "C"

// lddt.hip — all-pairs CA-lDDT (Mariani et al. 2013) of models against natives on the device: superposition-free, float64
// distances, INTEGER outputs.  DESIGN.md §3.20 states the definition; tests/lddt_ref.py restates it in numpy.
//
//   P_j            = {(a, b) ordered : |a - b| >= seq_sep, maskB[j, a] and maskB[j, b], dn = |B[j, a] - B[j, b]| < r0}   (strict)
//   total[j, a]    = #{b : (a, b) in P_j}
//   kept[i, j, a]  = sum over thresholds t of #{b : (a, b) in P_j, maskA[i, a] and maskA[i, b], | |A[i, a] - A[i, b]| - dn | < t}
// A distance is sqrt((dx dx + dy dy) + dz dz) in float64 with the correctly rounded square root and no contraction into FMAs (the
// unit is compiled with -ffp-contract=off), so every count equals numpy's.
//
//   lddt_pairs_kernel   one WORKGROUP of 8 waves per (tile of <= 8 models, native j, chunk of rows).  The tile's coordinates are staged in
//                       LDS as planes x[L], y[L], z[L] per model, a residue masked in the model as NaN: every comparison with it is
//                       false, so it keeps nothing and no mask is read in the inner loop.  A wave owns a row a.  Its lanes run over b
//                       64 at a time and compute the native distance ONCE; the pairs inside r0 (one ballot) are compacted into the
//                       wave's ring in LDS (b and dn), and whenever 64 are waiting — or the row ends — every lane takes one pair and
//                       scores it against all models of the tile.  So the native's pair set is found once per workgroup and the
//                       model loop runs on full waves however sparse the set is.  Per row: one wave64 integer reduction per model.
// kept [n, m] and total [m] are zeroed by the entry and summed with integer atomics (one per wave and model): integer addition is
// associative, two runs are bit-identical.  The per-residue outputs have exactly one writer each.
#include <math.h>

#include "ed_wave.h"
#include "kernels.h"

namespace ed {
namespace {

constexpr int LDDT_TILE = 8;                         // models per workgroup
constexpr int LDDT_THREADS = 512, LDDT_WAVES = LDDT_THREADS / 64;
constexpr int LDDT_RING = 128;                       // pairs a wave can hold: fewer than 64 waiting + the 64 of one step
constexpr int LDDT_MODEL_LDS = 144 * 1024;           // dynamic LDS for the tile; the rings take 12 KiB of the CU's 160 KiB
static_assert(24 * ESMDIFF_LDDT_MAX_L <= LDDT_MODEL_LDS, "one model of the longest chain fits");

typedef unsigned long long u64;

struct LddtArgs {
  const double *A, *B;
  const uint8_t *maskA, *maskB;
  int32_t *kept, *total, *kept_res, *total_res;
  double r0;
  double thr[ESMDIFF_LDDT_MAX_THRESHOLDS];
  int n, m, L, tile, tiles, seq_sep, n_thr;
};

__device__ __forceinline__ double dist(double dx, double dy, double dz) { return sqrt((dx * dx + dy * dy) + dz * dz); }

// grid (model tiles x m, row chunks).  Dynamic LDS: f64 [tile][3][L].  NT: the number of thresholds, 0 = p.n_thr.
template <int NT>
__global__ __launch_bounds__(LDDT_THREADS) void lddt_pairs_kernel(const LddtArgs p) {
  extern __shared__ double s_model[];
  __shared__ double s_dn[LDDT_WAVES][LDDT_RING];
  __shared__ int s_b[LDDT_WAVES][LDDT_RING];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int L = p.L, n_thr = NT ? NT : p.n_thr;
  const int first_tile = blockIdx.x % p.tiles == 0;        // the one tile of native j that reports the native's own counts
  const int j = blockIdx.x / p.tiles, i0 = (blockIdx.x % p.tiles) * p.tile;
  const int tm = min(p.tile, p.n - i0);

  for (int i = 0; i < tm; ++i) {
    const double* src = p.A + (int64_t)(i0 + i) * L * 3;
    const uint8_t* mk = p.maskA ? p.maskA + (int64_t)(i0 + i) * L : nullptr;
    for (int e = tid; e < 3 * L; e += LDDT_THREADS) {
      const int b = e / 3, c = e - 3 * b;
      s_model[(i * 3 + c) * L + b] = (mk && !mk[b]) ? __longlong_as_double(0x7ff8000000000000ll) : src[e];
    }
  }
  __syncthreads();

  const double* Bj = p.B + (int64_t)j * L * 3;
  const uint8_t* mb = p.maskB ? p.maskB + (int64_t)j * L : nullptr;
  double* ring_dn = s_dn[wave];
  int* ring_b = s_b[wave];
  int ksum[LDDT_TILE] = {0, 0, 0, 0, 0, 0, 0, 0};
  int tsum = 0;

  for (int a = blockIdx.y * LDDT_WAVES + wave; a < L; a += LDDT_WAVES * gridDim.y) {   // a is the same in every lane of the wave
    int acc[LDDT_TILE] = {0, 0, 0, 0, 0, 0, 0, 0};
    int head = 0, waiting = 0, trow = 0;

    // every lane below `count` takes one waiting pair and scores it against the tile
    auto score = [&](int count) {
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      const bool on = lane < count;
      const int slot = (head + lane) & (LDDT_RING - 1);
      const int b = on ? ring_b[slot] : a;
      const double dn = on ? ring_dn[slot] : 0.0;
#pragma unroll
      for (int i = 0; i < LDDT_TILE; ++i) {
        if (i < tm) {
          const double* M = s_model + (i * 3) * L;
          const double diff = fabs(dist(M[b] - M[a], M[L + b] - M[L + a], M[2 * L + b] - M[2 * L + a]) - dn);
          int c = 0;
#pragma unroll
          for (int k = 0; k < (NT ? NT : ESMDIFF_LDDT_MAX_THRESHOLDS); ++k)
            c += (k < n_thr && diff < p.thr[k]) ? 1 : 0;   // diff is NaN for a masked model residue: never kept
          acc[i] += on ? c : 0;
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
        double dn = 0.0;
        if (b < L && sep >= p.seq_sep && (!mb || mb[b])) {
          dn = dist(Bj[3 * b] - ax, Bj[3 * b + 1] - ay, Bj[3 * b + 2] - az);
          in = dn < p.r0;
        }
        const u64 bits = __ballot(in);
        if (!bits) continue;
        if (in) {
          const int slot = (head + waiting + __popcll(bits & ((1ull << lane) - 1))) & (LDDT_RING - 1);
          ring_b[slot] = b;
          ring_dn[slot] = dn;
        }
        const int found = __popcll(bits);
        waiting += found;                                  // < 64 before, <= 127 now: the ring holds them
        trow += found;
        if (waiting >= 64) {
          score(64);
          head = (head + 64) & (LDDT_RING - 1);
          waiting -= 64;
        }
      }
      if (waiting > 0) score(waiting);
    }

#pragma unroll
    for (int i = 0; i < LDDT_TILE; ++i) {
      if (i < tm) {
        const int r = wave_sum(acc[i]);
        ksum[i] += r;
        if (lane == 0 && p.kept_res) p.kept_res[((int64_t)(i0 + i) * p.m + j) * L + a] = r;
      }
    }
    tsum += trow;
    if (lane == 0 && first_tile && p.total_res) p.total_res[(int64_t)j * L + a] = trow;
  }

  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < LDDT_TILE; ++i)
      if (i < tm && ksum[i]) atomicAdd(&p.kept[(int64_t)(i0 + i) * p.m + j], ksum[i]);
    if (first_tile && tsum) atomicAdd(&p.total[j], tsum);
  }
}

}  // namespace
}  // namespace ed

using namespace ed;

extern "C" {

int esmdiff_lddt_pairs(const double* A, int32_t n, const double* B, int32_t m, int32_t L, const uint8_t* maskA, const uint8_t* maskB,
                       double r0, const double* thresholds, int32_t n_thresholds, int32_t seq_sep, int32_t* kept, int32_t* total,
                       int32_t* kept_res, int32_t* total_res, void* stream) {
  if (!A || !kept || !total || !thresholds || n < 1 || L < 2 || seq_sep < 1) return ESMDIFF_E_INVALID;
  if (n_thresholds < 1 || n_thresholds > ESMDIFF_LDDT_MAX_THRESHOLDS) return ESMDIFF_E_INVALID;
  if (!B) B = A, m = n, maskB = maskA;
  if (m < 1) return ESMDIFF_E_INVALID;
  if (L > ESMDIFF_LDDT_MAX_L) return ESMDIFF_E_CAPACITY;

  LddtArgs p;
  p.A = A, p.B = B, p.maskA = maskA, p.maskB = maskB;
  p.kept = kept, p.total = total, p.kept_res = kept_res, p.total_res = total_res;
  p.r0 = r0;
  for (int k = 0; k < ESMDIFF_LDDT_MAX_THRESHOLDS; ++k) p.thr[k] = k < n_thresholds ? thresholds[k] : -1.0;
  p.n = n, p.m = m, p.L = L, p.seq_sep = seq_sep, p.n_thr = n_thresholds;
  p.tile = std::max(1, std::min(std::min(LDDT_TILE, (int)n), LDDT_MODEL_LDS / (24 * L)));
  const int tiles = p.tiles = (n + p.tile - 1) / p.tile;
  // rows are split over workgroups only while the launch would leave CUs idle (each chunk stages the tile again)
  const int64_t groups = (int64_t)tiles * m;
  const int max_chunks = (L + LDDT_WAVES - 1) / LDDT_WAVES;
  const int chunks = (int)std::max<int64_t>(1, std::min<int64_t>(max_chunks, 1024 / groups));
  if (groups > INT32_MAX) return ESMDIFF_E_CAPACITY;       // grid.x
  const int lds = p.tile * 24 * L;

  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(kept, 0, (size_t)n * m * sizeof(int32_t), st) != hipSuccess) return ESMDIFF_E_HIP;
  if (hipMemsetAsync(total, 0, (size_t)m * sizeof(int32_t), st) != hipSuccess) return ESMDIFF_E_HIP;
  const auto kernel = n_thresholds == 4 ? lddt_pairs_kernel<4> : lddt_pairs_kernel<0>;
  if (ensure_dynamic_lds((const void*)kernel, lds) != hipSuccess) return ESMDIFF_E_HIP;
  hipLaunchKernelGGL(kernel, dim3((unsigned)groups, chunks), dim3(LDDT_THREADS), (size_t)lds, st, p);
  return finish_entry(st);
}

}  // extern "C"

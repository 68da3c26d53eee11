// ed_native_pairs.h — the native-pair scan of lddt.hip (lddt_pairs_kernel) and contacts.hip (native_contacts_kernel), once.
//
// Both score every model i against every native j over the native's own pair set
//   P_j = {(a, b) ordered : |a - b| >= min_sep, maskB[j, a] and maskB[j, b], d0 = |B[j, a] - B[j, b]| < cutoff}            (strict)
//   total[j, a]   = #{b : (a, b) in P_j}
//   kept[i, j, a] = sum over b with (a, b) in P_j of the policy's integer score of (|A[i, a] - A[i, b]|, payload(d0))
// One WORKGROUP of 8 waves per (tile of <= 8 models, native j, chunk of rows).  The tile's coordinates are staged in LDS as planes
// x[L], y[L], z[L] per model, a residue masked in the model as NaN: every comparison with it is false, so it keeps nothing and no
// mask is read in the inner loop.  A wave owns a row a.  Its lanes run over b 64 at a time and compute the native distance ONCE; the
// pairs inside the cutoff (one ballot) are compacted into the wave's ring in LDS (b and the payload), and whenever 64 are waiting —
// or the row ends — every lane takes one pair and scores it against all models of the tile.  So the native's pair set is found once
// per workgroup and the model loop runs on full waves however sparse the set is.  Per row: one wave64 integer reduction per model.
// kept [n, m] and total [m] are zeroed by launch_native_pairs and summed with integer atomics (one per wave and model): integer
// addition is associative, two runs are bit-identical.  The first tile of a native reports total.  The per-residue outputs have
// exactly one writer each.
//
// A POLICY says what the two analyses do not share.  It is built from the kernel's arguments (a copy of them) and has
//   static constexpr bool SOFT                    whether a float64 sum per (model, native) is kept beside the counts
//   int min_sep() const, double cutoff() const    the pair filter
//   double payload(double d0) const               what the ring holds for a pair of native distance d0
//   int score(double d, double v, double& soft) const
//                                                 the count that the model distance d (NaN: a residue is missing) adds for the payload v;
//                                                 with SOFT also the term it adds to the float64 sum, 0.0 for a missing residue
//   void finish(const double* wave_sum, int i0, int tm, int j) const
//                                                 SOFT only, called by every thread at the end of the kernel: wave_sum[i] is this wave's
//                                                 sum for model i0 + i.  The order up to there is a function of L alone: the k-th pair
//                                                 of row a (increasing b) goes to lane k % 64, which adds its terms in increasing k; the
//                                                 64 lane sums are combined by the xor butterfly of ed_wave.h; wave w adds the row sums
//                                                 of its rows in increasing a.  The caller launches ONE row chunk with SOFT.
#pragma once
#include <algorithm>

#include "ed_f64.h"
#include "ed_wave.h"
#include "kernels.h"

namespace ed {

constexpr int NP_TILE = 8;                               // models per workgroup
constexpr int NP_THREADS = 512, NP_WAVES = NP_THREADS / 64;
constexpr int NP_RING = 128;                             // pairs a wave can hold: fewer than 64 waiting + the 64 of one step
constexpr int NP_MODEL_LDS = 144 * 1024;                 // dynamic LDS for the tile; the rings (and a policy's own) take under 13 KiB of the CU's 160 KiB

struct NativePairArgs {
  const double *A, *B;
  const uint8_t *maskA, *maskB;
  int32_t *kept, *total, *kept_res, *total_res;
  int n, m, L, tile, tiles;
};

// grid (model tiles x m, row chunks).  Dynamic LDS: f64 [tile][3][L].
// p and pol are taken BY VALUE, and a policy holds its kernel's arguments by value: nothing then takes the address of the kernel's
// argument struct, and the compiler reads every field where it is used, as in a kernel that names its own argument.  Bound to
// references, the same source gave kernels 2 % slower on the MI355X (EXPERIMENTS.md, "One native-pair scan").
template <class Policy>
__device__ __forceinline__ void native_pair_scan(const NativePairArgs p, const Policy pol) {
  typedef unsigned long long u64;
  extern __shared__ double s_model[];
  __shared__ double s_v[NP_WAVES][NP_RING];
  __shared__ int s_b[NP_WAVES][NP_RING];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int L = p.L;
  const int first_tile = blockIdx.x % p.tiles == 0;        // the one tile of native j that reports the native's own counts
  const int j = blockIdx.x / p.tiles, i0 = (blockIdx.x % p.tiles) * p.tile;
  const int tm = min(p.tile, p.n - i0);

  for (int i = 0; i < tm; ++i) {
    const double* src = p.A + (int64_t)(i0 + i) * L * 3;
    const uint8_t* mk = p.maskA ? p.maskA + (int64_t)(i0 + i) * L : nullptr;
    for (int e = tid; e < 3 * L; e += NP_THREADS) {
      const int b = e / 3, c = e - 3 * b;
      s_model[(i * 3 + c) * L + b] = (mk && !mk[b]) ? quiet_nan() : src[e];
    }
  }
  __syncthreads();

  const double* Bj = p.B + (int64_t)j * L * 3;
  const uint8_t* mb = p.maskB ? p.maskB + (int64_t)j * L : nullptr;
  double* ring_v = s_v[wave];
  int* ring_b = s_b[wave];
  int ksum[NP_TILE] = {0, 0, 0, 0, 0, 0, 0, 0};
  double qsum[NP_TILE] = {0, 0, 0, 0, 0, 0, 0, 0};
  int tsum = 0;

  for (int a = blockIdx.y * NP_WAVES + wave; a < L; a += NP_WAVES * gridDim.y) {   // a is the same in every lane of the wave
    int acc[NP_TILE] = {0, 0, 0, 0, 0, 0, 0, 0};
    double qacc[NP_TILE] = {0, 0, 0, 0, 0, 0, 0, 0};
    int head = 0, waiting = 0, trow = 0;

    // every lane below `count` takes one waiting pair and scores it against the tile
    auto score = [&](int count) {
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      const bool on = lane < count;
      const int slot = (head + lane) & (NP_RING - 1);
      const int b = on ? ring_b[slot] : a;
      const double v = on ? ring_v[slot] : 0.0;
#pragma unroll
      for (int i = 0; i < NP_TILE; ++i) {
        if (i < tm) {
          const double* M = s_model + (i * 3) * L;
          double soft = 0.0;
          const int c = pol.score(dist(M[b] - M[a], M[L + b] - M[L + a], M[2 * L + b] - M[2 * L + a]), v, soft);
          acc[i] += on ? c : 0;
          if (Policy::SOFT) qacc[i] += on ? soft : 0.0;
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
        if (b < L && sep >= pol.min_sep() && (!mb || mb[b])) {
          d0 = dist(Bj[3 * b] - ax, Bj[3 * b + 1] - ay, Bj[3 * b + 2] - az);
          in = d0 < pol.cutoff();
        }
        const u64 bits = __ballot(in);
        if (!bits) continue;
        if (in) {
          const int slot = (head + waiting + __popcll(bits & ((1ull << lane) - 1))) & (NP_RING - 1);
          ring_b[slot] = b;
          ring_v[slot] = pol.payload(d0);
        }
        const int found = __popcll(bits);
        waiting += found;                                  // < 64 before, <= 127 now: the ring holds them
        trow += found;
        if (waiting >= 64) {
          score(64);
          head = (head + 64) & (NP_RING - 1);
          waiting -= 64;
        }
      }
      if (waiting > 0) score(waiting);
    }

#pragma unroll
    for (int i = 0; i < NP_TILE; ++i) {
      if (i < tm) {
        const int r = wave_sum(acc[i]);
        ksum[i] += r;
        if (Policy::SOFT) qsum[i] += wave_sum(qacc[i]);
        if (lane == 0 && p.kept_res) p.kept_res[((int64_t)(i0 + i) * p.m + j) * L + a] = r;
      }
    }
    tsum += trow;
    if (lane == 0 && first_tile && p.total_res) p.total_res[(int64_t)j * L + a] = trow;
  }

  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < NP_TILE; ++i)
      if (i < tm && ksum[i]) atomicAdd(&p.kept[(int64_t)(i0 + i) * p.m + j], ksum[i]);
    if (first_tile && tsum) atomicAdd(&p.total[j], tsum);
  }
  if constexpr (Policy::SOFT) pol.finish(qsum, i0, tm, j);
}

// What both entries do once their own arguments are checked and A, B, the masks, the outputs, n, m and L are in p: the tile, the
// grid (refused when grid.x would not hold it), kept and total zeroed on the stream, the launch, and the wait of finish_entry.
// Rows are split over workgroups only while the launch would leave CUs idle (each chunk stages the tile again), and never
// without split_rows.
template <class Args>
int launch_native_pairs(void (*kernel)(Args), Args& p, bool split_rows, hipStream_t st) {
  p.tile = std::max(1, std::min(std::min(NP_TILE, p.n), NP_MODEL_LDS / (24 * p.L)));
  p.tiles = (p.n + p.tile - 1) / p.tile;
  const int64_t groups = (int64_t)p.tiles * p.m;
  if (groups > INT32_MAX) return ESMDIFF_E_CAPACITY;       // grid.x
  const int max_chunks = (p.L + NP_WAVES - 1) / NP_WAVES;
  const int chunks = split_rows ? (int)std::max<int64_t>(1, std::min<int64_t>(max_chunks, 1024 / groups)) : 1;
  const int lds = p.tile * 24 * p.L;

  if (hipMemsetAsync(p.kept, 0, (size_t)p.n * p.m * sizeof(int32_t), st) != hipSuccess) return ESMDIFF_E_HIP;
  if (hipMemsetAsync(p.total, 0, (size_t)p.m * sizeof(int32_t), st) != hipSuccess) return ESMDIFF_E_HIP;
  if (ensure_dynamic_lds((const void*)kernel, lds) != hipSuccess) return ESMDIFF_E_HIP;
  hipLaunchKernelGGL(kernel, dim3((unsigned)groups, chunks), dim3(NP_THREADS), (size_t)lds, st, p);
  return finish_entry(st);
}

}  // namespace ed

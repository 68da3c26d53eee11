// lddt.hip — all-pairs CA-lDDT (Mariani et al. 2013) of models against natives on the device: superposition-free, float64
// distances, INTEGER outputs.  DESIGN.md §3.20 states the definition; tests/lddt_ref.py restates it in numpy.
//
//   P_j            = {(a, b) ordered : |a - b| >= seq_sep, maskB[j, a] and maskB[j, b], dn = |B[j, a] - B[j, b]| < r0}   (strict)
//   total[j, a]    = #{b : (a, b) in P_j}
//   kept[i, j, a]  = sum over thresholds t of #{b : (a, b) in P_j, maskA[i, a] and maskA[i, b], | |A[i, a] - A[i, b]| - dn | < t}
// A distance is sqrt((dx dx + dy dy) + dz dz) in float64 with the correctly rounded square root and no contraction into FMAs (the
// unit is compiled with -ffp-contract=off), so every count equals numpy's.
//
//   lddt_pairs_kernel   the native-pair scan of ed_native_pairs.h (one WORKGROUP of 8 waves per tile of <= 8 models, native j and chunk
//                       of rows; the layout, the ring and the integer reductions are described there) with the lDDT policy: the
//                       pair filter is seq_sep and r0, the ring holds dn itself, and a pair scores the number of thresholds t with
//                       | d - dn | < t.  No float64 sum is kept.
#include <math.h>

#include "ed_native_pairs.h"

namespace ed {
namespace {

static_assert(24 * ESMDIFF_LDDT_MAX_L <= NP_MODEL_LDS, "one model of the longest chain fits");

struct LddtArgs : NativePairArgs {
  double r0;
  double thr[ESMDIFF_LDDT_MAX_THRESHOLDS];
  int seq_sep, n_thr;
};

// NT: the number of thresholds, 0 = p.n_thr
template <int NT>
struct LddtPolicy {
  static constexpr bool SOFT = false;
  const LddtArgs p;
  __device__ int min_sep() const { return p.seq_sep; }
  __device__ double cutoff() const { return p.r0; }
  __device__ double payload(double dn) const { return dn; }
  __device__ int score(double d, double dn, double&) const {
    const int n_thr = NT ? NT : p.n_thr;
    const double diff = fabs(d - dn);
    int c = 0;
#pragma unroll
    for (int k = 0; k < (NT ? NT : ESMDIFF_LDDT_MAX_THRESHOLDS); ++k)
      c += (k < n_thr && diff < p.thr[k]) ? 1 : 0;         // diff is NaN for a masked model residue: never kept
    return c;
  }
};

template <int NT>
__global__ __launch_bounds__(NP_THREADS) void lddt_pairs_kernel(const LddtArgs p) {
  native_pair_scan(p, LddtPolicy<NT>{p});
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
  return launch_native_pairs(n_thresholds == 4 ? lddt_pairs_kernel<4> : lddt_pairs_kernel<0>, p, true, (hipStream_t)stream);
}

}  // extern "C"

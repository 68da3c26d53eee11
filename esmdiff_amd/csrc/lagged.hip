// lagged.hip — the time-lagged moments of a trajectory's features on the device, fused from the coordinates: the window means, the raw
// second moments S00 = sum a a^T, S0t = sum a b^T, Stt = sum b b^T with their residual sums, and the projection onto given directions.
// float64 throughout; the hot loop is the f64 MFMA v_mfma_f64_16x16x4_f64.  DESIGN.md §3.27 states the definitions and the order of
// every sum; tests/kinetics_ref.py restates the three entries in numpy.
//
// FEATURES.  pwd_offset = 0: X is f64 [n, D] and f_d(x_t) = X[t][d].  pwd_offset = k >= 1: X is f64 [n, L, 3] and f_d is the distance
// of the d-th pair (i, j >= i + k) in numpy.triu_indices order, sqrt((dx dx + dy dy) + dz dz) with d = x_j - x_i and no FMA (the unit
// is compiled with -ffp-contract=off): the bits of esmdiff_metrics_pwd.  A first kernel writes the pair table (i, j)[D] into the head of
// the caller's scratch; no (n, D) array exists anywhere.
//
// FRAMES.  m = n - lag pairs (t, t + lag), t < m, a_t = f(x_t) - c, b_t = f(x_{t + lag}) - c.  The pairs are cut into CHUNKS of
// ESMDIFF_LAGGED_FRAME_CHUNK consecutive t.  A chunk's sums go to a SLOT of the scratch; the scratch holds as many slots as fit (at
// least one), the chunks are worked off in ROUNDS of that many, and after every round one kernel adds the round's slots to the outputs
// in increasing chunk index, starting from chunk 0's own sums.  The number of slots decides how much runs at once and nothing else:
// every output is a function of (X, c, n, lag) alone.
//
// MOMENTS.  Features are cut into tiles of 64.  A workgroup of eight waves owns a pair of tiles (I, J >= I) and one chunk.  For 32
// frames at a time it stages a_I, b_I, a_J, b_J in LDS (each feature of each frame computed once per tile and window; I == J stages one
// tile) as [16-feature block][frame][16], so that the 64 lanes of a wave read 64 consecutive doubles as an MFMA operand: lane l holds
// A[i = l & 15][k = l >> 4], the feature i of frame k, and B[k = l >> 4][j = l & 15].  A staging thread keeps one feature for the
// whole chunk (its residues, its centre) and walks the frames; the lanes of a wave hold the 64 features of a tile at one frame.  Waves 0, 1 accumulate S00[I, J] = a_I^T a_J, waves 2, 3 Stt[I, J], waves
// 4, 5 S0t[I, J] = a_I^T b_J and waves 6, 7 S0t[J, I] = a_J^T b_I, each wave 32 rows of the tile as 2 x 4 blocks of 16 x 16, over the
// chunk's frames in increasing t, four frames to an instruction.  C/D of the f64 MFMA: col = lane & 15, row = (lane >> 4) + 4 reg.  S00 and Stt are written at [i][j] and
// at [j][i] from the same register, and of a diagonal tile only the elements j >= i are used: both are exactly symmetric.  Frames past
// the chunk and features past D are staged as zeros.  The next 32 frames are computed into registers while the staged ones are multiplied
// (the two waves of a SIMD in opposite order), and written to LDS between two barriers.
//
// SUMS.  A window sum is s = 0, then s = s + (f(x_t) - c) for the chunk's t in increasing order; chunks are added as above.  The means'
// numerators (c = 0) are one thread per feature and chunk.  The residual sums r0, rt (the caller's c) are taken from the staged a_I, b_I
// by wave 6 of the diagonal workgroup (I, I), which has no fourth product: lane l sums feature l of the tile over the staged frames in
// order (a staged zero past the chunk adds nothing).
//
// PROJECTION.  A wave owns a frame.  Lane l holds p_l = 0 and adds (f_d - mean_d) * W[d][k] (a product, then an add) for d = l, l + 64,
// ... in increasing d; then p_l = p_l + p_{l ^ s} for s = 32, 16, 8, 4, 2, 1, after which every lane holds the same bits.  The tree
// depends on D alone, so a frame's row does not depend on the batch it is in.
#include <math.h>

#include "ed_f64.h"
#include "kernels.h"

namespace ed {
namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int LG_TILE = 64, LG_SUB = 16, LG_SUBS = LG_TILE / LG_SUB, LG_FRAMES = 32, LG_THREADS = 512;
constexpr int LG_PLANE = LG_SUBS * LG_FRAMES * LG_SUB;     // one staged tile of one window: [16-feature block][frame][16]
static_assert(ESMDIFF_LAGGED_FRAME_CHUNK % LG_FRAMES == 0, "a chunk is a whole number of staged blocks");
static_assert(ESMDIFF_LAGGED_MAX_D >= (ESMDIFF_LAGGED_MAX_L * (ESMDIFF_LAGGED_MAX_L - 1)) / 2, "every pair list of MAX_L residues is allowed");

struct LagIn {
  const double* X;
  const int2* pairs;     // null: the feature form
  const double* c;       // null: nothing is subtracted
  int64_t n;
  int L, D, lag;
  int64_t m;
};

__device__ __forceinline__ double feature(const LagIn& p, int64_t t, int d) {
  if (!p.pairs) return p.X[t * p.D + d];
  const int2 ij = p.pairs[d];
  const double *a = p.X + (t * p.L + ij.x) * 3, *b = p.X + (t * p.L + ij.y) * 3;
  return dist(b[0] - a[0], b[1] - a[1], b[2] - a[2]);
}

// pairs[d] = the d-th (i, j) of numpy.triu_indices(L, k): row i holds the L - k - i pairs j = i + k ... L - 1
__global__ __launch_bounds__(256) void lagged_pairs_kernel(int L, int k, int D, int2* pairs) {
  const int d = blockIdx.x * 256 + threadIdx.x;
  if (d >= D) return;
  int i = 0, rest = d;
  while (rest >= L - k - i) rest -= L - k - i, ++i;
  pairs[d] = make_int2(i, i + k + rest);
}

// grid (ceil(D / 256), chunks of the round): slot[0][d], slot[1][d] = the chunk's sums of both windows
__global__ __launch_bounds__(256) void lagged_sums_kernel(const LagIn p, int64_t chunk0, double* slots, int64_t slot_stride) {
  const int d = blockIdx.x * 256 + threadIdx.x;
  if (d >= p.D) return;
  const int64_t t0 = (chunk0 + blockIdx.y) * ESMDIFF_LAGGED_FRAME_CHUNK;
  const int64_t t1 = t0 + ESMDIFF_LAGGED_FRAME_CHUNK < p.m ? t0 + ESMDIFF_LAGGED_FRAME_CHUNK : p.m;
  const double c = p.c ? p.c[d] : 0.0;
  double s0 = 0.0, st = 0.0;
  int64_t t = t0;
  for (; t + 8 <= t1; t += 8) {                            // eight frames' loads in flight; the additions in the order of t, one by one
    double v0[8], vt[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v0[u] = feature(p, t + u, d) - c, vt[u] = feature(p, t + u + p.lag, d) - c;
#pragma unroll
    for (int u = 0; u < 8; ++u) s0 = s0 + v0[u], st = st + vt[u];
  }
  for (; t < t1; ++t) {
    s0 = s0 + (feature(p, t, d) - c);
    st = st + (feature(p, t + p.lag, d) - c);
  }
  double* out = slots + blockIdx.y * slot_stride;
  out[d] = s0, out[p.D + d] = st;
}

// One feature of one thread of the staging: where its frames start, how far they are apart, and its centre
struct LagFeature {
  const double *a, *b;   // the feature form: a is the column; the coordinate form: the two residues of frame 0
  double c;
  bool has;
};

__device__ __forceinline__ double feature_at(const LagFeature& f, bool coords, int64_t at) {
  if (!coords) return f.a[at];
  return dist(f.b[at] - f.a[at], f.b[at + 1] - f.a[at + 1], f.b[at + 2] - f.a[at + 2]);
}

// grid (tile pairs, chunks of the round): slot = S00[D, D], S0t[D, D], Stt[D, D], r0[D], rt[D] of the chunk
__global__ __launch_bounds__(LG_THREADS) void lagged_moments_kernel(const LagIn p, int64_t chunk0, double* slots, int64_t slot_stride) {
  __shared__ double s_feat[4 * LG_PLANE];                  // a_I, b_I, a_J, b_J: 64 KiB
  const int D = p.D, tiles = (D + LG_TILE - 1) / LG_TILE;
  int I = 0, rest = blockIdx.x;
  while (rest >= tiles - I) rest -= tiles - I, ++I;
  const int J = I + rest;
  const bool diag = I == J;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t t0 = (chunk0 + blockIdx.y) * ESMDIFF_LAGGED_FRAME_CHUNK;
  const int64_t t1 = t0 + ESMDIFF_LAGGED_FRAME_CHUNK < p.m ? t0 + ESMDIFF_LAGGED_FRAME_CHUNK : p.m;

  // staging: waves 0 - 3 stage tile I and waves 4 - 7 tile J (nothing when I == J); lane l keeps feature l of the tile and wave w walks
  // the frames w & 3, (w & 3) + 4, ...: the 64 lanes of a load read ONE frame (consecutive pairs of it: a dozen cache lines, not four
  // frames' worth), and the frame's address advances by additions alone
  const int side = wave >> 2, fw = wave & 3;
  const bool coords = p.pairs != nullptr, stages = !(diag && side);
  const int64_t stride = coords ? (int64_t)p.L * 3 : D, step = 4 * stride, lag_off = (int64_t)p.lag * stride;
  const int d_mine = (side ? J : I) * LG_TILE + lane;
  LagFeature f;
  f.has = d_mine < D && stages, f.a = f.b = p.X, f.c = 0.0;
  if (f.has) {
    f.c = p.c[d_mine];
    if (coords) {
      const int2 ij = p.pairs[d_mine];
      f.a = p.X + ij.x * 3, f.b = p.X + ij.y * 3;
    } else {
      f.a = p.X + d_mine;
    }
  }
  double* mine = s_feat + 2 * side * LG_PLANE + (lane >> 4) * (LG_FRAMES * LG_SUB) + fw * LG_SUB + (lane & 15);
  int64_t at_block = (t0 + fw) * stride;                   // where this thread's first frame of the block computed next begins

  // products: waves 2 q and 2 q + 1 share product q, rows 0 - 31 and 32 - 63 of its tile: rows from `left`, columns from `right`
  const int product = wave >> 1, half = wave & 1;
  const double* s_aJ = s_feat + (diag ? 0 : 2 * LG_PLANE);
  const double* s_bJ = s_feat + (diag ? 1 : 3) * LG_PLANE;
  const double* left = (product == 0 ? s_feat : product == 1 ? s_feat + LG_PLANE : product == 2 ? s_feat : s_aJ) + 2 * half * (LG_FRAMES * LG_SUB);
  const double* right = product == 0 ? s_aJ : product == 1 ? s_bJ : product == 2 ? s_bJ : s_feat + LG_PLANE;
  const bool spare = product == 3 && diag;                 // no fourth product on the diagonal:
  const bool sums = spare && half == 0;                    // ... one of its waves sums a_I and b_I instead, lane l the feature l of the tile
  const double* column = s_feat + (lane >> 4) * (LG_FRAMES * LG_SUB) + (lane & 15);
  double r0 = 0.0, rt = 0.0;

  f64x4 acc[2][LG_SUBS];
#pragma unroll
  for (int bi = 0; bi < 2; ++bi)
#pragma unroll
    for (int bj = 0; bj < LG_SUBS; ++bj) acc[bi][bj] = f64x4{0.0, 0.0, 0.0, 0.0};

  // A block of 32 frames is computed into registers WHILE the block before it is multiplied out of LDS: the waves that share a SIMD
  // (w and w + 4) take the two halves in opposite order, so that one computes distances while the other feeds the matrix unit.
  constexpr int G = LG_FRAMES / 4;
  double va[G], vb[G];
  auto compute = [&](int64_t tb) {
    int64_t at = at_block;
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const int64_t t = tb + g * 4 + fw;
      va[g] = vb[g] = 0.0;
      if (t < t1 && f.has) {
        va[g] = feature_at(f, coords, at) - f.c;
        vb[g] = feature_at(f, coords, at + lag_off) - f.c;
      }
      at += step;
    }
    at_block += LG_FRAMES * stride;
  };
  auto store = [&]() {
    if (stages) {
#pragma unroll
      for (int g = 0; g < G; ++g) mine[g * 4 * LG_SUB] = va[g], mine[g * 4 * LG_SUB + LG_PLANE] = vb[g];
    }
  };
  auto multiply = [&]() {
    if (sums) {
#pragma unroll 8
      for (int fr = 0; fr < LG_FRAMES; ++fr) r0 = r0 + column[fr * LG_SUB], rt = rt + column[LG_PLANE + fr * LG_SUB];
    } else if (!spare) {
#pragma unroll 2
      for (int kk = 0; kk < LG_FRAMES / 4; ++kk) {
        double a[2], b[LG_SUBS];
#pragma unroll
        for (int q = 0; q < 2; ++q) a[q] = left[q * (LG_FRAMES * LG_SUB) + kk * 64 + lane];
#pragma unroll
        for (int q = 0; q < LG_SUBS; ++q) b[q] = right[q * (LG_FRAMES * LG_SUB) + kk * 64 + lane];
#pragma unroll
        for (int bi = 0; bi < 2; ++bi)
#pragma unroll
          for (int bj = 0; bj < LG_SUBS; ++bj) acc[bi][bj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[bi], b[bj], acc[bi][bj], 0, 0, 0);
      }
    }
  };

  if (stages) compute(t0);
  store();
  __syncthreads();
  for (int64_t tb = t0; tb < t1; tb += LG_FRAMES) {
    const bool more = tb + LG_FRAMES < t1;
    if (wave < 4) {
      if (more && stages) compute(tb + LG_FRAMES);
      multiply();
    } else {
      multiply();
      if (more && stages) compute(tb + LG_FRAMES);
    }
    __syncthreads();                                       // every wave has read this block
    if (more) store();
    __syncthreads();
  }

  const int64_t plane = (int64_t)D * D;
  double* slot = slots + blockIdx.y * slot_stride;
  if (spare) {
    const int d = I * LG_TILE + lane;
    if (sums && d < D) slot[3 * plane + d] = r0, slot[3 * plane + D + d] = rt;
    return;
  }
  double* out = slot + (product == 0 ? 0 : product == 1 ? 2 * plane : plane);
  const int R = (product == 3 ? J : I) * LG_TILE + 2 * half * LG_SUB, C = (product == 3 ? I : J) * LG_TILE;
  const bool symmetric = product < 2;
#pragma unroll
  for (int bi = 0; bi < 2; ++bi)
#pragma unroll
    for (int bj = 0; bj < LG_SUBS; ++bj)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int i = R + bi * LG_SUB + (lane >> 4) + 4 * reg, j = C + bj * LG_SUB + (lane & 15);
        if (i >= D || j >= D) continue;
        const double v = acc[bi][bj][reg];
        if (!symmetric) {
          out[(int64_t)i * D + j] = v;
        } else if (!diag || j >= i) {
          out[(int64_t)i * D + j] = v;
          out[(int64_t)j * D + i] = v;
        }
      }
}

// The round's slots onto the outputs, element by element: chunk 0's sums, then + chunk 1's, + chunk 2's, ...
struct LagOut {
  double* dst[5];
  int64_t at[5], count[5];     // where the segment starts in a slot, and its length
};

__global__ __launch_bounds__(256) void lagged_add_kernel(const LagOut o, int segments, const double* slots, int64_t slot_stride, int used,
                                                         int first_round, int64_t total, double divide_by) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  int s = 0;
  int64_t in = e;
  while (s + 1 < segments && in >= o.count[s]) in -= o.count[s], ++s;
  const double* src = slots + o.at[s] + in;
  double v = first_round ? src[0] : o.dst[s][in];
  for (int k = first_round ? 1 : 0; k < used; ++k) v = v + src[k * slot_stride];
  o.dst[s][in] = divide_by != 0.0 ? v / divide_by : v;
}

constexpr int PJ_WAVES = 4;

// grid ceil(n / 4): a wave owns a frame
__global__ __launch_bounds__(64 * PJ_WAVES) void lagged_project_kernel(const LagIn p, const double* mean, const double* W, int dim, double* Y) {
  const int lane = threadIdx.x & 63;
  const int64_t t = (int64_t)blockIdx.x * PJ_WAVES + (threadIdx.x >> 6);
  if (t >= p.n) return;
  double acc[ESMDIFF_LAGGED_MAX_DIM];
#pragma unroll
  for (int k = 0; k < ESMDIFF_LAGGED_MAX_DIM; ++k) acc[k] = 0.0;
  for (int d = lane; d < p.D; d += 64) {
    const double g = feature(p, t, d) - mean[d];
    const double* w = W + (int64_t)d * dim;
#pragma unroll
    for (int k = 0; k < ESMDIFF_LAGGED_MAX_DIM; ++k)
      if (k < dim) acc[k] = acc[k] + g * w[k];
  }
#pragma unroll
  for (int k = 0; k < ESMDIFF_LAGGED_MAX_DIM; ++k) {
    if (k >= dim) continue;                                // the same in every lane
    double v = acc[k];
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v = v + __shfl_xor(v, s, 64);
    if (lane == 0) Y[t * dim + k] = v;
  }
}

// What the three entries share: the limits, the number of features, and the pair table at the head of the scratch
struct LagPlan {
  LagIn in;
  int64_t chunks;
  double* slots;
};

int lagged_features(int32_t L_or_D, int32_t pwd_offset) {
  if (pwd_offset < 0 || L_or_D < 1) return 0;
  if (pwd_offset == 0) return L_or_D <= ESMDIFF_LAGGED_MAX_D ? L_or_D : 0;
  if (L_or_D > ESMDIFF_LAGGED_MAX_L || pwd_offset >= L_or_D) return 0;
  return (int)ESMDIFF_LAGGED_FEATURES(L_or_D, pwd_offset);
}

int lagged_plan(LagPlan& q, const double* X, int32_t n, int32_t L_or_D, int32_t pwd_offset, int32_t lag, const double* c, void* scratch,
                hipStream_t st) {
  const int D = lagged_features(L_or_D, pwd_offset);
  q.in.X = X, q.in.c = c, q.in.n = n, q.in.L = L_or_D, q.in.D = D, q.in.lag = lag, q.in.m = (int64_t)n - lag;
  q.in.pairs = pwd_offset ? (const int2*)scratch : nullptr;
  q.chunks = (q.in.m + ESMDIFF_LAGGED_FRAME_CHUNK - 1) / ESMDIFF_LAGGED_FRAME_CHUNK;
  q.slots = (double*)((char*)scratch + ESMDIFF_LAGGED_TABLE_BYTES(D));
  if (pwd_offset) hipLaunchKernelGGL(lagged_pairs_kernel, dim3((D + 255) / 256), dim3(256), 0, st, L_or_D, pwd_offset, D, (int2*)scratch);
  return D;
}

}  // namespace
}  // namespace ed

using namespace ed;

extern "C" {

int esmdiff_lagged_means(const double* X, int32_t n, int32_t L_or_D, int32_t pwd_offset, int32_t lag, double* mean0, double* meant,
                         void* scratch, int64_t scratch_bytes, void* stream) {
  const int D = lagged_features(L_or_D, pwd_offset);
  if (!X || !mean0 || !meant || !scratch || D < 1 || lag < 1 || n <= lag) return ESMDIFF_E_INVALID;
  if (scratch_bytes < ESMDIFF_LAGGED_MEANS_SCRATCH_BYTES(D, 1)) return ESMDIFF_E_INVALID;
  const int64_t slot = 2 * (int64_t)D;
  int64_t room = (scratch_bytes - ESMDIFF_LAGGED_TABLE_BYTES(D)) / (slot * 8);
  if (room > 65535) room = 65535;                          // the grid's second dimension

  hipStream_t st = (hipStream_t)stream;
  LagPlan q;
  lagged_plan(q, X, n, L_or_D, pwd_offset, lag, nullptr, scratch, st);
  LagOut o = {};
  o.dst[0] = mean0, o.dst[1] = meant, o.at[0] = 0, o.at[1] = D, o.count[0] = o.count[1] = D;
  for (int64_t c0 = 0; c0 < q.chunks; c0 += room) {
    const int used = (int)(q.chunks - c0 < room ? q.chunks - c0 : room);
    hipLaunchKernelGGL(lagged_sums_kernel, dim3((D + 255) / 256, used), dim3(256), 0, st, q.in, c0, q.slots, slot);
    hipLaunchKernelGGL(lagged_add_kernel, dim3((unsigned)((slot + 255) / 256)), dim3(256), 0, st, o, 2, q.slots, slot, used, (int)(c0 == 0),
                       slot, c0 + used >= q.chunks ? (double)q.in.m : 0.0);
  }
  return finish_entry(st);
}

int esmdiff_lagged_moments(const double* X, int32_t n, int32_t L_or_D, int32_t pwd_offset, int32_t lag, const double* center, double* S00,
                           double* S0t, double* Stt, double* r0, double* rt, void* scratch, int64_t scratch_bytes, void* stream) {
  const int D = lagged_features(L_or_D, pwd_offset);
  if (!X || !center || !S00 || !S0t || !Stt || !r0 || !rt || !scratch || D < 1 || lag < 1 || n <= lag) return ESMDIFF_E_INVALID;
  if (scratch_bytes < ESMDIFF_LAGGED_MOMENTS_SCRATCH_BYTES(D, 1)) return ESMDIFF_E_INVALID;
  const int64_t plane = (int64_t)D * D, slot = 3 * plane + 2 * D;
  int64_t room = (scratch_bytes - ESMDIFF_LAGGED_TABLE_BYTES(D)) / (slot * 8);
  if (room > 65535) room = 65535;                          // the grid's second dimension

  hipStream_t st = (hipStream_t)stream;
  LagPlan q;
  lagged_plan(q, X, n, L_or_D, pwd_offset, lag, center, scratch, st);
  LagOut o = {};
  double* dst[5] = {S00, S0t, Stt, r0, rt};
  for (int s = 0; s < 5; ++s) o.dst[s] = dst[s], o.count[s] = s < 3 ? plane : D, o.at[s] = s < 3 ? s * plane : 3 * plane + (s - 3) * (int64_t)D;
  const int tiles = (D + LG_TILE - 1) / LG_TILE, tile_pairs = tiles * (tiles + 1) / 2;
  for (int64_t c0 = 0; c0 < q.chunks; c0 += room) {
    const int used = (int)(q.chunks - c0 < room ? q.chunks - c0 : room);
    hipLaunchKernelGGL(lagged_moments_kernel, dim3(tile_pairs, used), dim3(LG_THREADS), 0, st, q.in, c0, q.slots, slot);
    hipLaunchKernelGGL(lagged_add_kernel, dim3((unsigned)((slot + 255) / 256)), dim3(256), 0, st, o, 5, q.slots, slot, used, (int)(c0 == 0),
                       slot, 0.0);
  }
  return finish_entry(st);
}

int esmdiff_lagged_project(const double* X, int32_t n, int32_t L_or_D, int32_t pwd_offset, const double* mean, const double* W, int32_t dim,
                           double* Y, void* scratch, int64_t scratch_bytes, void* stream) {
  const int D = lagged_features(L_or_D, pwd_offset);
  if (!X || !mean || !W || !Y || D < 1 || n < 0 || dim < 1 || dim > ESMDIFF_LAGGED_MAX_DIM) return ESMDIFF_E_INVALID;
  if (pwd_offset && (!scratch || scratch_bytes < ESMDIFF_LAGGED_TABLE_BYTES(D))) return ESMDIFF_E_INVALID;
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) return finish_entry(st);
  LagPlan q;
  lagged_plan(q, X, n, L_or_D, pwd_offset, 1, nullptr, scratch, st);
  hipLaunchKernelGGL(lagged_project_kernel, dim3((unsigned)((n + PJ_WAVES - 1) / PJ_WAVES)), dim3(64 * PJ_WAVES), 0, st, q.in, mean, W, (int)dim, Y);
  return finish_entry(st);
}

}  // extern "C"

// aligned.hip — the first and second moments of an ensemble's Cartesian coordinates after a per-frame rigid transform, and the
// projection of the transformed frames onto given directions.  float64 throughout; the hot loop is the f64 MFMA
// v_mfma_f64_16x16x4_f64.  DESIGN.md §3.29 states the definitions and the order of every sum; tests/aligned_ref.py restates both
// entries in numpy.  The design is lagged.hip's with ONE product and a staging that applies the transform.
//
// FEATURES.  X is f64 [n, L, 3], T f64 [n, 12] (row-major rot[9], then tr[3]; what esmdiff_flex_transforms writes) or null.  For
// d = 3 l + c and (x, y, z) = X[t][l]:  f_d(t) = (((R[c][0] x + R[c][1] y) + R[c][2] z) + tr[c]), no FMA (the unit is compiled with
// -ffp-contract=off); T == null: f_d(t) = X[t][l][c] exactly.  a_d(t) = f_d(t) - c_d.  No transformed (n, L, 3) array exists anywhere.
// A frame's T row is the same for the 64 lanes of a staging wave: it is read as ONE load of its 96 bytes (lane l reads T[t][l % 12])
// and broadcast by four wave shuffles, a lane taking the row of its coordinate.  (Twelve loads per lane and frame through a wave-uniform
// pointer stay vector loads, each the whole wave at one address: that form was a third slower, EXPERIMENTS.md "Covariance".)
//
// FRAMES.  The n frames are cut into CHUNKS of ESMDIFF_ALIGNED_FRAME_CHUNK consecutive t.  A chunk's sums go to a SLOT of the scratch;
// the scratch holds as many slots as fit (at least one), the chunks are worked off in ROUNDS of that many, and after every round one
// kernel adds the round's slots to the outputs in increasing chunk index, starting from chunk 0's own sums.  The number of slots
// decides how much runs at once and nothing else: every output is a function of (X, T, use, c, n, L) alone.  A frame with use[t] == 0
// is staged as zeros, without its coordinates or its T row being read: x + 0.0 = x for every x a sum can hold here (a sum starts as
// +0.0 and is never -0.0), so an unused frame changes no bit.
//
// MOMENTS.  Features are cut into tiles of 64.  A workgroup of FOUR waves owns a pair of tiles (I, J >= I) and one chunk.  For 32
// frames at a time it stages a_I and a_J in LDS (I == J stages one tile) as [16-feature block][frame][16], so that the 64 lanes of a
// wave read 64 consecutive doubles as an MFMA operand: lane l holds A[i = l & 15][k = l >> 4], the feature i of frame k, and
// B[k = l >> 4][j = l & 15].  THE SPLIT: with one product instead of lagged's four, wave w owns the 16 rows w of the tile and all 64
// columns, four 16 x 16 blocks: per four frames it reads one A operand and four B operands from LDS and issues four instructions, and
// the workgroup is 256 threads with 32 KiB of LDS, so several of them share a CU and one's staging hides behind another's products.
// Of a diagonal tile wave w skips the blocks left of the diagonal (column block < w), which nothing reads.  The sums run over the
// chunk's frames in increasing t, four frames to an instruction.  C/D of the f64 MFMA: col = lane & 15, row = (lane >> 4) + 4 reg.  S
// is written at [i][j] and at [j][i] from the same register, and of a diagonal tile only the elements j >= i are used: S is exactly
// symmetric.  Frames past the chunk and features past D are staged as zeros.  A staging thread keeps one feature for the whole chunk
// (its residue, its coordinate, its centre) and walks the frames; off the diagonal waves 0, 1 stage tile I and waves 2, 3 tile J
// (frames w & 1, (w & 1) + 2, ...), on the diagonal all four stage tile I (frames w, w + 4, ...).  The next 32 frames are computed
// into registers before the staged ones are multiplied, and written to LDS between two barriers.
//
// SUMS.  r = sum a is taken from the staged a_I by wave 3 of the diagonal workgroup (I, I), which has one block of the product only:
// lane l sums feature l of the tile, s = +0.0, then s = s + a(t) over the staged frames in order.  count is the number of t with
// use[t] != 0 (an integer: no order).
//
// PROJECTION.  A wave owns a frame.  Lane l holds p_l = 0 and adds (f_d - mean_d) * W[d][k] (a product, then an add) for d = l, l + 64,
// ... in increasing d; then p_l = p_l + p_{l ^ s} for s = 32, 16, 8, 4, 2, 1, after which every lane holds the same bits.  The tree
// depends on D alone, so a frame's row does not depend on the batch it is in.  The order of lagged_project_kernel.
#include <math.h>

#include "kernels.h"

namespace ed {
namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int AL_TILE = 64, AL_SUB = 16, AL_SUBS = AL_TILE / AL_SUB, AL_FRAMES = 32, AL_THREADS = 256;
constexpr int AL_PLANE = AL_SUBS * AL_FRAMES * AL_SUB;     // one staged tile: [16-feature block][frame][16]
constexpr int AL_G = AL_FRAMES / 2;                        // the frames of a block one staging thread computes off the diagonal
static_assert(ESMDIFF_ALIGNED_FRAME_CHUNK % AL_FRAMES == 0, "a chunk is a whole number of staged blocks");
static_assert(ESMDIFF_ALIGNED_MAX_L == ESMDIFF_TM_MAX_L, "the cap is the TM kernel's");

// f_d of one frame, the projection's form (a wave reads its frame's T row once, before its loop over d): xyz points at X[t][l], Tt (wave-uniform) at T[t] or null, c = d % 3
__device__ __forceinline__ double aligned_feature(const double* __restrict__ xyz, const double* __restrict__ Tt, int c) {
  if (!Tt) return xyz[c];
  const double r0 = c == 0 ? Tt[0] : c == 1 ? Tt[3] : Tt[6];
  const double r1 = c == 0 ? Tt[1] : c == 1 ? Tt[4] : Tt[7];
  const double r2 = c == 0 ? Tt[2] : c == 1 ? Tt[5] : Tt[8];
  const double tr = c == 0 ? Tt[9] : c == 1 ? Tt[10] : Tt[11];
  return ((r0 * xyz[0] + r1 * xyz[1]) + r2 * xyz[2]) + tr;
}

// one workgroup: count[0] = the frames with use[t] != 0
__global__ __launch_bounds__(256) void aligned_count_kernel(const uint8_t* use, int64_t n, int64_t* count) {
  __shared__ unsigned long long s_total;
  if (threadIdx.x == 0) s_total = 0;
  __syncthreads();
  unsigned long long mine = 0;
  if (use)
    for (int64_t t = threadIdx.x; t < n; t += 256) mine += use[t] != 0;
  atomicAdd(&s_total, mine);
  __syncthreads();
  if (threadIdx.x == 0) count[0] = use ? (int64_t)s_total : n;
}

// grid (tile pairs, chunks of the round): slot = S[D, D], r[D] of the chunk
__global__ __launch_bounds__(AL_THREADS) void aligned_moments_kernel(const double* __restrict__ X, const double* __restrict__ T,
                                                                     const uint8_t* __restrict__ use, int64_t n, int L,
                                                                     const double* __restrict__ center, int64_t chunk0,
                                                                     double* __restrict__ slots, int64_t slot_stride) {
  __shared__ double s_feat[2 * AL_PLANE];                  // a_I, a_J: 32 KiB
  const int D = 3 * L, tiles = (D + AL_TILE - 1) / AL_TILE;
  int I = 0, rest = blockIdx.x;
  while (rest >= tiles - I) rest -= tiles - I, ++I;
  const int J = I + rest;
  const bool diag = I == J;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t t0 = (chunk0 + blockIdx.y) * ESMDIFF_ALIGNED_FRAME_CHUNK;
  const int64_t t1 = t0 + ESMDIFF_ALIGNED_FRAME_CHUNK < n ? t0 + ESMDIFF_ALIGNED_FRAME_CHUNK : n;

  // staging: lane l keeps feature l of its tile; the wave walks the frames fw, fw + nw, ... of a block, so the 64 lanes of a load read
  // ONE frame (192 consecutive doubles of it at most) and one T row
  const int side = diag ? 0 : wave >> 1, nw = diag ? 4 : 2, fw = diag ? wave : wave & 1;
  const int d_mine = (side ? J : I) * AL_TILE + lane;
  const bool has = d_mine < D;
  const int res = has ? d_mine / 3 : 0, comp = has ? d_mine - 3 * res : 0;
  const double c_mine = has ? center[d_mine] : 0.0;
  const int64_t stride = (int64_t)L * 3;
  const double* x_mine = X + res * 3;
  double* mine = s_feat + side * AL_PLANE + (lane >> 4) * (AL_FRAMES * AL_SUB) + (lane & 15);

  const double* left = s_feat + wave * (AL_FRAMES * AL_SUB);               // rows: block `wave` of a_I
  const double* right = s_feat + (diag ? 0 : AL_PLANE);                    // columns: a_J
  const bool sums = diag && wave == AL_SUBS - 1;                           // lane l sums feature l of the tile
  const double* column = s_feat + (lane >> 4) * (AL_FRAMES * AL_SUB) + (lane & 15);
  double r = 0.0;

  f64x4 acc[AL_SUBS];
#pragma unroll
  for (int bj = 0; bj < AL_SUBS; ++bj) acc[bj] = f64x4{0.0, 0.0, 0.0, 0.0};

  // THE BROADCASTS.  A block's 32 flags are one load (lane f reads use[tb + f]) and a ballot: bit f of `on` says that frame tb + f
  // exists and is used, the same in every lane.  A frame's T row is one load (lane l reads T[t][l % 12]: 96 bytes for the wave) and
  // four shuffles, from the lanes 3 c, 3 c + 1, 3 c + 2 and 9 + c; the branches around them are wave-uniform, so the source lanes run.
  const int t_lane = lane % 12;
  double va[AL_G];
  auto compute = [&](int64_t tb) {
    const bool mine_on = lane < AL_FRAMES && tb + lane < t1 && (!use || use[tb + lane]);
    const unsigned long long on = __ballot(mine_on);
#pragma unroll
    for (int g = 0; g < AL_G; ++g) {
      const int fr = g * nw + fw;                          // wave-uniform, as `on` is
      va[g] = 0.0;
      if (fr >= AL_FRAMES || !((on >> fr) & 1)) continue;
      const int64_t t = tb + fr;
      const double* xyz = x_mine + t * stride;
      double f;
      if (T) {
        const double row = T[t * 12 + t_lane];
        const double r0 = __shfl(row, 3 * comp, 64), r1 = __shfl(row, 3 * comp + 1, 64), r2 = __shfl(row, 3 * comp + 2, 64);
        const double tr = __shfl(row, 9 + comp, 64);
        f = ((r0 * xyz[0] + r1 * xyz[1]) + r2 * xyz[2]) + tr;
      } else {
        f = xyz[comp];
      }
      if (has) va[g] = f - c_mine;
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int g = 0; g < AL_G; ++g)
      if (g * nw + fw < AL_FRAMES) mine[(g * nw + fw) * AL_SUB] = va[g];
  };
  auto multiply = [&]() {
    if (sums) {
#pragma unroll 8
      for (int fr = 0; fr < AL_FRAMES; ++fr) r = r + column[fr * AL_SUB];
    }
#pragma unroll 2
    for (int kk = 0; kk < AL_FRAMES / 4; ++kk) {
      const double a = left[kk * 64 + lane];
#pragma unroll
      for (int bj = 0; bj < AL_SUBS; ++bj) {
        if (diag && bj < wave) continue;                   // wave-uniform: left of the diagonal, never read
        const double b = right[bj * (AL_FRAMES * AL_SUB) + kk * 64 + lane];
        acc[bj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[bj], 0, 0, 0);
      }
    }
  };

  compute(t0);
  store();
  __syncthreads();
  for (int64_t tb = t0; tb < t1; tb += AL_FRAMES) {
    const bool more = tb + AL_FRAMES < t1;
    if (more) compute(tb + AL_FRAMES);
    multiply();
    __syncthreads();                                       // every wave has read this block
    if (more) store();
    __syncthreads();
  }

  double* slot = slots + blockIdx.y * slot_stride;
  if (sums) {
    const int d = I * AL_TILE + lane;
    if (d < D) slot[(int64_t)D * D + d] = r;
  }
  const int R = I * AL_TILE + wave * AL_SUB, C = J * AL_TILE;
#pragma unroll
  for (int bj = 0; bj < AL_SUBS; ++bj) {
    if (diag && bj < wave) continue;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int i = R + (lane >> 4) + 4 * reg, j = C + bj * AL_SUB + (lane & 15);
      if (i >= D || j >= D) continue;
      if (diag && j < i) continue;
      const double v = acc[bj][reg];
      slot[(int64_t)i * D + j] = v;
      slot[(int64_t)j * D + i] = v;
    }
  }
}

// The round's slots onto the outputs, element by element: chunk 0's sums, then + chunk 1's, + chunk 2's, ...  A slot is S then r.
__global__ __launch_bounds__(256) void aligned_add_kernel(double* S, double* r, int64_t plane, const double* slots, int64_t slot_stride,
                                                          int used, int first_round, int64_t total) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  double* dst = e < plane ? S + e : r + (e - plane);
  const double* src = slots + e;
  double v = first_round ? src[0] : dst[0];
  for (int k = first_round ? 1 : 0; k < used; ++k) v = v + src[k * slot_stride];
  dst[0] = v;
}

constexpr int AP_WAVES = 4;

// grid ceil(n / 4): a wave owns a frame
__global__ __launch_bounds__(64 * AP_WAVES) void aligned_project_kernel(const double* __restrict__ X, const double* __restrict__ T, int64_t n,
                                                                        int L, const double* __restrict__ mean, const double* __restrict__ W,
                                                                        int dim, double* __restrict__ Y) {
  const int lane = threadIdx.x & 63;
  const int64_t t = (int64_t)blockIdx.x * AP_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (t >= n) return;
  const int D = 3 * L;
  const double* frame = X + t * D;
  const double* Tt = T ? T + t * 12 : nullptr;             // wave-uniform
  double acc[ESMDIFF_ALIGNED_MAX_DIM];
#pragma unroll
  for (int k = 0; k < ESMDIFF_ALIGNED_MAX_DIM; ++k) acc[k] = 0.0;
  for (int d = lane; d < D; d += 64) {
    const int res = d / 3;
    const double g = aligned_feature(frame + res * 3, Tt, d - 3 * res) - mean[d];
    const double* w = W + (int64_t)d * dim;
#pragma unroll
    for (int k = 0; k < ESMDIFF_ALIGNED_MAX_DIM; ++k)
      if (k < dim) acc[k] = acc[k] + g * w[k];
  }
#pragma unroll
  for (int k = 0; k < ESMDIFF_ALIGNED_MAX_DIM; ++k) {
    if (k >= dim) continue;                                // the same in every lane
    double v = acc[k];
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v = v + __shfl_xor(v, s, 64);
    if (lane == 0) Y[t * dim + k] = v;
  }
}

}  // namespace
}  // namespace ed

using namespace ed;

extern "C" {

int esmdiff_aligned_moments(const double* X, int32_t n, int32_t L, const double* T, const uint8_t* use, const double* center, double* S,
                            double* r, int64_t* count, void* scratch, int64_t scratch_bytes, void* stream) {
  if (!X || !center || !S || !r || !count || !scratch || n < 1 || L < 1) return ESMDIFF_E_INVALID;
  if (L > ESMDIFF_ALIGNED_MAX_L) return ESMDIFF_E_CAPACITY;
  if (scratch_bytes < ESMDIFF_ALIGNED_MOMENTS_SCRATCH_BYTES(L, 1)) return ESMDIFF_E_INVALID;
  const int D = 3 * L;
  const int64_t plane = (int64_t)D * D, slot = plane + D;
  int64_t room = scratch_bytes / (slot * 8);
  if (room > 65535) room = 65535;                          // the grid's second dimension

  hipStream_t st = (hipStream_t)stream;
  const int64_t chunks = ((int64_t)n + ESMDIFF_ALIGNED_FRAME_CHUNK - 1) / ESMDIFF_ALIGNED_FRAME_CHUNK;
  const int tiles = (D + AL_TILE - 1) / AL_TILE, tile_pairs = tiles * (tiles + 1) / 2;
  hipLaunchKernelGGL(aligned_count_kernel, dim3(1), dim3(256), 0, st, use, (int64_t)n, count);
  for (int64_t c0 = 0; c0 < chunks; c0 += room) {
    const int used = (int)(chunks - c0 < room ? chunks - c0 : room);
    hipLaunchKernelGGL(aligned_moments_kernel, dim3(tile_pairs, used), dim3(AL_THREADS), 0, st, X, T, use, (int64_t)n, (int)L, center, c0,
                       (double*)scratch, slot);
    hipLaunchKernelGGL(aligned_add_kernel, dim3((unsigned)((slot + 255) / 256)), dim3(256), 0, st, S, r, plane, (const double*)scratch, slot,
                       used, (int)(c0 == 0), slot);
  }
  return finish_entry(st);
}

int esmdiff_aligned_project(const double* X, int32_t n, int32_t L, const double* T, const double* mean, const double* W, int32_t dim,
                            double* Y, void* stream) {
  if (!X || !mean || !W || !Y || n < 0 || L < 1 || dim < 1 || dim > ESMDIFF_ALIGNED_MAX_DIM) return ESMDIFF_E_INVALID;
  if (L > ESMDIFF_ALIGNED_MAX_L) return ESMDIFF_E_CAPACITY;
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) return finish_entry(st);
  hipLaunchKernelGGL(aligned_project_kernel, dim3((unsigned)((n + AP_WAVES - 1) / AP_WAVES)), dim3(64 * AP_WAVES), 0, st, X, T, (int64_t)n, (int)L,
                     mean, W, (int)dim, Y);
  return finish_entry(st);
}

}  // extern "C"

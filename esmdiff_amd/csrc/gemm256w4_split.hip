// gemm256w4_split.hip — the float32-grade "split" linears of the strict path on the four-wave 256x256x64 tile (gfx950):
// v_mfma_f32_32x32x16_f16 over f16 plane triples.  Tile, waves, LDS image and persistence: gemm256w4_common.h; raster and
// LDS-DMA stream: gemm256w4_tile.inc (both shared with the bf16 / f16 kernel of gemm256w4.hip).  Compiled once: the operands are
// f16 whatever the engine's 16-bit type is.
//
// The operands are f16 plane triples per row — A [M, 3K1] = [hi | lo | hi], W [N, 3K1] = [lo | hi | hi] with x ~ hi + lo to
// 2^-22 — so that ONE linear walk over K = 3 K1 accumulates A_hi.W_lo + A_lo.W_hi + A_hi.W_hi (small terms first) into the same
// f32 accumulators: the main loop is a plain 16-bit one and has not one scalar more (a two-plane layout with a jump back for the
// third pass cost 5 SGPRs, the kernel spilled, and hipcc's v_readlane reloads landed directly in front of the inline-asm LDS-DMA
// that consumed them: a VALU-writes-SGPR -> VMEM hazard it does not pad inside asm; tools/check_asm_hazards.py looks for it).
// EPI is one of esmdiff_gemm_f32_epilogue (or 3 / 4, see the launcher), outputs are f32, scaled per row by rs[m] * alpha
// (powers of two: exact).  Operand preparation: gemm_split.hip.
//
//   wave tile  4 x 4 accumulators of 32 x 32 (each holds the TRANSPOSED block: the W fragment is operand 1).
//   k-step     K = 16: 16 MFMAs (j = B fragment outer, i = A fragment inner: 16 independent accumulators back to back, the same
//              accumulator again 16 MFMAs later).  The 8 fragment reads of the NEXT k-step are placed one per MFMA gap
//              behind the first 8 MFMAs, into the other operand set; one s_waitcnt lgkmcnt(0) at the k-step boundary
//              (the reads were issued >= 8 MFMAs = 256 cycles earlier).
//   K-tile     4 k-steps.  Barrier between k-steps 2 and 3: by then every wave holds the fragments of k-step 3 in
//              registers (stage P is no longer read) and its own LDS-DMA of K-tile t+1 has landed (vmcnt(0): issued
//              during k-step 3 of K-tile t-1 and k-step 0 of K-tile t, i.e. >= 2 k-steps = 1024 matrix cycles ago).
//              The 16 LDS-DMA instructions per wave that refill stage P with K-tile t+2 go one per two MFMAs into k-step
//              3 of K-tile t (A pieces) and k-step 0 of K-tile t+1 (W pieces).
#include "gemm256w4_common.h"

namespace ed {

typedef __attribute__((ext_vector_type(16))) float f32x16;

namespace g4 {
// Where the 16 LDS-DMA instructions of a K-tile sit among the MFMAs: the instruction index issued behind MFMA n of k-step ks, or
// -1.  One per two MFMAs over all of k-steps 3 and 0 (the refill of stage P with K-tile t+2 starts in k-step 3 of K-tile t and
// ends in k-step 0 of K-tile t+1; it shares the first gaps with the fragment reads).  The prologue issues the 8 of k-step 3.
constexpr int dma_idx(int ks, int n) {
  if (ks == 3) return (n & 1) ? (n >> 1) : -1;
  if (ks == 0) return (n & 1) ? 8 + (n >> 1) : -1;
  return -1;
}

// KSLICED (launch_gemm256w4_splitk): K slices of the product as extra row blocks.  The grid walks S * m_pad "virtual" rows;
// virtual row block s = m0 / m_pad reads columns s*K .. (s+1)*K of the physical rows m0 - s*m_pad .. of A and of every W row
// (row stride ld_ab = the whole 3 K1 walk), and its f32 partial products go to rows m0 .. of `out` ([S * m_pad, N]).
// Everything but the source addresses is the same kernel.
template <int EPI, bool KSLICED = false>
__global__ __launch_bounds__(256, 1) void gemm256w4_split_kernel(const bf16_t* __restrict__ A, const bf16_t* __restrict__ W,
                                                                 void* __restrict__ out, const float* __restrict__ bias,
                                                                 int M, int N, int K, int ldc, float alpha, int tiles_m,
                                                                 int tiles_n, const float* __restrict__ rs, float div,
                                                                 int ld_ab, int m_pad, int m_real) {
#include "gemm256w4_tile.inc"

  // ---- fragment read addressing (inline-asm ds_read_b128, immediates carry stage / fragment offsets) --------------
  const int frow = lane & 31, khalf = lane >> 5, fsw = (frow >> 1) & 7;
  uint32_t offA[4], offB[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    const uint32_t lo = frow * 128 + (((ks * 2 + khalf) ^ fsw) << 4);
    offA[ks] = lds_base + (wm * 2) * HALF_BYTES + lo;
    offB[ks] = lds_base + ((2 + wn) * 2) * HALF_BYTES + lo;
  }
#define W4_MFMA(acc_, b_, a_)                                                                         \
  do {                                                                                                \
    if (W4_ABL(4)) asm volatile("" : "+a"(acc_) : "v"(b_), "v"(a_));                                  \
    else asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+a"(acc_) : "v"(b_), "v"(a_));      \
  } while (0)
// first k-step of a tile: D = B x A + 0 (no zeroing pass over the 256 accumulator registers)
#define W4_MFMA0(acc_, b_, a_)                                                                        \
  do {                                                                                                \
    if (W4_ABL(4)) asm volatile("" : "=a"(acc_) : "v"(b_), "v"(a_));                                  \
    else asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, 0" : "=a"(acc_) : "v"(b_), "v"(a_));       \
  } while (0)
#define W4_WAIT_LGKM0(s_)                                                                                          \
  asm volatile("s_waitcnt lgkmcnt(0)"                                                                              \
               : "+v"(s_.a[0]), "+v"(s_.a[1]), "+v"(s_.a[2]), "+v"(s_.a[3]), "+v"(s_.b[0]), "+v"(s_.b[1]), "+v"(s_.b[2]), \
                 "+v"(s_.b[3]))

  struct OpSet {
    bf16x8 a[4], b[4];
  };
  OpSet X, Y;
  f32x16 acc[4][4];  // [i: A row block][j: W column block]; holds the TRANSPOSED 32x32 block (W fragment is operand 1)

  // read fragment r (0..3: A row block r, 4..7: W column block r-4) of k-step ks, stage buf, into set S
  auto read_frag = [&](OpSet& S, auto R, auto KS, auto BUF) {
    constexpr int r = decltype(R)::value, ks = decltype(KS)::value, buf = decltype(BUF)::value;
    const uint32_t addr = r < 4 ? offA[ks] : offB[ks];
    bf16x8& dst = r < 4 ? S.a[r & 3] : S.b[r & 3];
    W4_DSR(dst, addr, buf * HALF_BYTES + (r & 3) * 4096);
  };

  // One k-step: 16 MFMAs on set C; the reads of the next k-step (NKS of stage NBUF) into set Nx behind MFMAs 0..7; in k-steps
  // 3 and 0 the LDS-DMA instructions dma_idx(KS, n) of K-tile dma_v into stage DMA_BUF around the odd MFMAs (s_mov m0 in
  // front, the load behind).
  auto kstep = [&](OpSet& C, OpSet& Nx, auto NKS, auto NBUF, auto KS, auto DMA_BUF, auto DMA_NEXT, int dma_v,
                   auto FIRST) {
    constexpr int ks_ = decltype(KS)::value, dbuf = decltype(DMA_BUF)::value;
#define W4_STEP(n)                                                                               \
  {                                                                                              \
    constexpr int j_ = (n) >> 2, i_ = (n)&3;                                                     \
    if constexpr (dma_idx(ks_, (n)) >= 0) dma1(DMA_NEXT, dma_idx(ks_, (n)), dbuf, dma_v, 1);     \
    if constexpr (decltype(FIRST)::value) W4_MFMA0(acc[i_][j_], C.b[j_], C.a[i_]);               \
    else W4_MFMA(acc[i_][j_], C.b[j_], C.a[i_]);                                                 \
    if constexpr ((n) < 8) read_frag(Nx, std::integral_constant<int, (n)>{}, NKS, NBUF);         \
    if constexpr (dma_idx(ks_, (n)) >= 0) dma1(DMA_NEXT, dma_idx(ks_, (n)), dbuf, dma_v, 2);     \
  }
    W4_STEP(0) W4_STEP(1) W4_STEP(2) W4_STEP(3) W4_STEP(4) W4_STEP(5) W4_STEP(6) W4_STEP(7)
    W4_STEP(8) W4_STEP(9) W4_STEP(10) W4_STEP(11) W4_STEP(12) W4_STEP(13) W4_STEP(14) W4_STEP(15)
#undef W4_STEP
  };

  // One K-tile at stage P.  Entry: X holds the fragments of (t, k-step 0).  N0 / N3: the LDS-DMA issued in k-step 0 / 3
  // belongs to the workgroup's next tile (K-tile v0 / v3 of it) instead of K-tile t+1 / t+2 of this one.
  auto ktile = [&](auto P, auto N0, auto N3, int v0, int v3, auto FIRST) {
    using Q = std::integral_constant<int, 1 - decltype(P)::value>;
    // k-step 0 (+ second half of the LDS-DMA of the next K-tile into the other stage)
    kstep(X, Y, I1{}, P, I0{}, Q{}, N0, v0, FIRST);
    W4_WAIT_LGKM0(Y);
    kstep(Y, X, I2{}, P, I1{}, Q{}, N0, v0, TF{});
    W4_WAIT_LGKM0(X);
    kstep(X, Y, I3{}, P, I2{}, Q{}, N0, v0, TF{});
    W4_WAIT_LGKM0(Y);                                  // ... and stage P is fully read by this wave
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's share of the next K-tile has landed
    __builtin_amdgcn_s_barrier();
    // k-step 3: first fragments of the next K-tile (other stage; after the tile's last K-tile they are simply not used) +
    // first half of the LDS-DMA of the K-tile after it into this stage
    kstep(Y, X, I0{}, Q{}, I3{}, P, N3, v3, TF{});
    W4_WAIT_LGKM0(X);
  };

  const uint32_t lhi = lane >> 5, lrow = lane & 31;

  for (int vt = bid; vt < n_tiles; vt += gridDim.x) {
    W4_BEGIN_TILE(vt);
    if (!have_k0) {  // first tile of this workgroup: K-tile 0 and the first half of K-tile 1
#pragma unroll
      for (int idx = 0; idx < 16; ++idx) dma1(TF{}, idx, 0, 0);
#pragma unroll
      for (int idx = 0; idx < 8; ++idx) dma1(TF{}, idx, 1, 1);
      asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      // (a following tile finds both in place: the previous tile's K loop streamed them, its last barrier made K-tile 0
      // visible, and its last k-step read the fragments of this tile's (K-tile 0, k-step 0) from stage 0 into X)
      read_frag(X, I0{}, I0{}, I0{});
      read_frag(X, I1{}, I0{}, I0{});
      read_frag(X, I2{}, I0{}, I0{});
      read_frag(X, I3{}, I0{}, I0{});
      read_frag(X, std::integral_constant<int, 4>{}, I0{}, I0{});
      read_frag(X, std::integral_constant<int, 5>{}, I0{}, I0{});
      read_frag(X, std::integral_constant<int, 6>{}, I0{}, I0{});
      read_frag(X, std::integral_constant<int, 7>{}, I0{}, I0{});
      W4_WAIT_LGKM0(X);
    }

    ktile(I0{}, TF{}, TF{}, 1, 2, TT{});               // first k-step writes the accumulators (C = 0)
    ktile(I1{}, TF{}, TF{}, 2, 3, TF{});
    for (int t = 2; t < nk - 2; t += 2) {              // steady state: no condition anywhere
      ktile(I0{}, TF{}, TF{}, t + 1, t + 2, TF{});
      ktile(I1{}, TF{}, TF{}, t + 2, t + 3, TF{});
    }
    ktile(I0{}, TF{}, TT{}, nk - 1, 0, TF{});          // k-step 3 starts streaming the next tile's K-tile 0
    ktile(I1{}, TT{}, TT{}, 0, 1, TF{});               // ... finishes it, and starts its K-tile 1
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");  // the last MFMAs' results before the compiler's accvgpr reads

    // ---- epilogue: register-direct (each 32x32 accumulator is the transposed output block: a lane holds one output row and
    // 4 consecutive columns per register group) -----------
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (W4_ABL(16)) {
        asm volatile("" ::"a"(acc[i][0]), "a"(acc[i][1]), "a"(acc[i][2]), "a"(acc[i][3]));
        continue;
      }
      const int m = m0 + wm * 128 + i * 32 + lrow;
      const bool live = m < M && !(W4_ABL(8) && alpha != 12345.f);
      const float sc = (rs && m < M) ? rs[m] * alpha : alpha;   // row scale * weight scale, both powers of two
      if constexpr (EPI == 4) {
        // FFN-up with the SwiGLU fused (W rows interleaved gate / up in blocks of 32, as in the bf16 path): mid = silu(g) * u in
        // f32, written as f32 [M, FH] (ldc >= FH).  exp and the reciprocal are the hardware's (1 ulp each).
        // The split row the FFN-down GEMM reads is made from it by split_rows_kernel with the row's OWN power-of-two scale
        // (r05).  r04 wrote the split row right here with one scale per layer taken from the a-priori bound |mid| <= B^2:
        // on weights with trained statistics (LayerNorm gains of 30, FFN units with 50x row norm) that bound sits 2^22 ..
        // 2^33 above the typical element, the f16 pair underflows, and the engine's logits were 100x further from a float64
        // evaluation than the exact-f32 engine's (profiles/r05_split_vs_f64.txt).
#pragma unroll
        for (int jp = 0; jp < 2; ++jp)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float gt = acc[i][2 * jp][g * 4 + e] * sc, up = acc[i][2 * jp + 1][g * 4 + e] * sc;
              v[e] = gt * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(gt * -1.44269504088896341f)) * up;
            }
            if (!live) continue;
            float* o = reinterpret_cast<float*>(out) + (int64_t)m * ldc + (n0 + wn * 128 + jp * 64) / 2 + g * 8 + lhi * 4;
            *reinterpret_cast<f32x4*>(o) = v;
          }
      } else {   // f32 outputs of the split linears: acc * (row scale * weight scale)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            // no column bound: the launcher requires ldc >= N (a bound check per 8-column group becomes 16 hoisted lane
            // masks or scalar flags = 32+ SGPRs, the kernel spills, and hipcc's v_readlane reloads land in front of the
            // inline-asm LDS-DMA that reads them: a VALU-writes-SGPR -> VMEM hazard nobody pads inside asm)
            const int n = n0 + wn * 128 + j * 32 + g * 8 + lhi * 4;
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = acc[i][j][g * 4 + e] * sc;
            if (!live) continue;
            float* o = reinterpret_cast<float*>(out) + (int64_t)m * ldc + n;
            if constexpr (EPI == ESMDIFF_F32EPI_RESID_DIV) {   // x = x + r / scaling_factor (esm's own expression)
              f32x4 x = *reinterpret_cast<const f32x4*>(o);
#pragma unroll
              for (int e = 0; e < 4; ++e) x[e] = x[e] + v[e] / div;
              *reinterpret_cast<f32x4*>(o) = x;
            } else {
              if constexpr (EPI != ESMDIFF_F32EPI_STORE) {   // 3: the launcher's code for STORE with a bias
                const f32x4 bb = *reinterpret_cast<const f32x4*>(bias + n);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] += bb[e];
              }
              *reinterpret_cast<f32x4*>(o) = v;
            }
          }
      }
    }
    W4_END_TILE();
  }
#undef W4_MFMA
#undef W4_MFMA0
#undef W4_WAIT_LGKM0
}
}  // namespace g4

// The split linears.  A3 f16 [M, 3K] = [hi | lo | hi] with per-row scale rs[M] (NULL: 1), W3 f16 [N, 3K] = [lo | hi | hi]
// scaled by 1 / w_scale; out f32 [M, ldc]; N % 256 == 0, K % 128 == 0 (so that 3 K / 64 is even).
hipError_t launch_gemm256w4_split(const uint16_t* A2, const float* rs, const uint16_t* W2, float w_scale, float* out,
                                  const float* bias, int M, int N, int K, int ldc, float div, int epi, hipStream_t stream) {
  using namespace g4;
  if (M <= 0) return hipSuccess;
  if (N % BN != 0 || K % (2 * BK) != 0 || (ldc & 3) || (epi != 4 && ldc < N) || (epi == 4 && ldc < N / 2)) return hipErrorInvalidValue;
  const int tiles_m = (M + BM - 1) / BM, tiles_n = N / BN;
  // (no bias + GELU epilogue here: erff on 256 accumulators spills; the consumer LayerNorm applies the GELU on load)
  auto launch = [&](auto kernel) {
    return launch_persistent(kernel, tiles_m * tiles_n, stream, A2, W2, (void*)out, bias, M, N, 3 * K, ldc, w_scale, tiles_m,
                             tiles_n, rs, div, 0, 0, 0);
  };
  switch (epi) {
    case ESMDIFF_F32EPI_STORE: return bias ? launch(gemm256w4_split_kernel<3>) : launch(gemm256w4_split_kernel<ESMDIFF_F32EPI_STORE>);
    case ESMDIFF_F32EPI_RESID_DIV: return launch(gemm256w4_split_kernel<ESMDIFF_F32EPI_RESID_DIV>);
    case 4: return launch(gemm256w4_split_kernel<4>);   // fused SwiGLU -> mid as f32 [M, ldc >= N / 2] (W rows interleaved gate / up)
    default: return hipErrorInvalidValue;
  }
}

// The same product cut into S slices of the 3 K walk, for launches with too few tiles to fill the chip: parts[s] ([m_pad, N]
// f32, m_pad = M rounded up to 256) = (slice s of A2) . (slice s of W2)^T * w_scale, row scales NOT applied; the caller sums
// the slices in order and applies rs (gemm_split.hip::launch_splitk_reduce_resid).  3 K / S must be a multiple of 128.
hipError_t launch_gemm256w4_splitk(const uint16_t* A2, const uint16_t* W2, float w_scale, float* parts, int M, int N, int K,
                                   int S, hipStream_t stream) {
  using namespace g4;
  if (M <= 0) return hipSuccess;
  if (S < 2 || N % BN != 0 || (3 * K) % S != 0 || ((3 * K) / S) % (2 * BK) != 0 || (3 * K) / S < 6 * BK) return hipErrorInvalidValue;
  const int tiles_m_phys = (M + BM - 1) / BM, tiles_n = N / BN, m_pad = tiles_m_phys * BM;
  const int tiles_m = S * tiles_m_phys;
  return launch_persistent(gemm256w4_split_kernel<ESMDIFF_F32EPI_STORE, true>, tiles_m * tiles_n, stream, A2, W2, (void*)parts,
                           (const float*)nullptr, S * m_pad, N, (3 * K) / S, N, w_scale, tiles_m, tiles_n, (const float*)nullptr,
                           1.f, 3 * K, m_pad, M);
}

}  // namespace ed

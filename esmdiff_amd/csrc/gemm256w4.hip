// gemm256w4.hip — the 256x256x64 bf16 / f16 MFMA GEMM with FOUR waves (one per SIMD) and 128x128 wave tiles (gfx950), main loop
// on v_mfma_f32_16x16x32.  Tile, waves, LDS image and persistence: gemm256w4_common.h; raster and LDS-DMA stream:
// gemm256w4_tile.inc (both shared with the float32-grade kernel of gemm256w4_split.hip).  Compiled once per 16-bit operand type.
//
//   wave tile  8 x 8 accumulators of 16 x 16 (each holds the TRANSPOSED block: lane = output row, 4 columns).  A fragment is
//              one ds_read_b128 per lane: 16 rows x K = 32, lane l holds row l & 15, k = 8 (l >> 4) .. +7.  The DMA's chunk
//              swizzle (row >> 1) & 7 keeps these reads free of bank conflicts: each 16-lane group of a ds_read_b128 meets 16
//              distinct 16-byte bank quads.
//   k-step     K = 32: 64 MFMAs of 16 cycles (j = W block outer, i = A block inner: 64 independent accumulators back to back).
//              The 16 fragment reads of the NEXT k-step go one per two MFMAs behind the first 32, into the other operand set;
//              one s_waitcnt lgkmcnt(0) at the k-step boundary.
//   K-tile     2 k-steps, the barrier between them: by then every wave holds the fragments of k-step 1 in registers (stage P
//              is no longer read) and its own LDS-DMA of K-tile t+1 has landed (vmcnt(0): issued a whole k-step = 1024 matrix
//              cycles ago).  The 16 LDS-DMA instructions per wave that refill stage P with K-tile t+2 go one per four MFMAs
//              into k-step 1 (64 cycles apart).
// Same FLOP per cycle and the same LDS bytes per FLOP as a v_mfma_f32_32x32x16 loop on this tile, and the same results bit for
// bit, but the chip holds a higher clock on this shape under the package power cap (EXPERIMENTS R7.1).
#include "gemm256w4_common.h"

namespace ed {
namespace g4 {
// Gap plan: fragment read behind MFMA n of a k-step (16 reads of the next k-step, one per two MFMAs over the first half), and
// LDS-DMA instruction behind MFMA n of k-step 1 (16 per K-tile, one per four MFMAs; the whole of the next k-step 0 = 1024
// matrix cycles is the landing slack)
constexpr int m16_read(int n) { return (n < 32 && !(n & 1)) ? n >> 1 : -1; }
constexpr int m16_dma(int n) { return (n & 3) == 1 ? n >> 2 : -1; }
template <typename F, int... N>
__device__ __forceinline__ void unroll_seq(F&& f, std::integer_sequence<int, N...>) {
  (f(std::integral_constant<int, N>{}), ...);
}

__device__ __forceinline__ float gelu_erf(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752f)); }
__device__ __forceinline__ float silu_mul(float g, float u) {
  return g * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(g * -1.44269504088896341f)) * u;
}
__device__ __forceinline__ uint32_t pack_bf16x2(float a, float b) { return ed_pack2(a, b); }   // the TU's 16-bit type (ed_half.h)

// rs .. m_real are the arguments of gemm256w4_split_kernel, which this kernel does not read: it keeps the argument block both
// kernels were measured with (the hidden arguments behind it, gridDim among them, stay where they were).
template <int EPI>
__global__ __launch_bounds__(256, 1) void gemm256w4_kernel(const bf16_t* __restrict__ A, const bf16_t* __restrict__ W,
                                                           void* __restrict__ out, const float* __restrict__ bias, int M,
                                                           int N, int K, int ldc, float alpha, int tiles_m, int tiles_n,
                                                           const float* __restrict__ rs, float div, int ld_ab, int m_pad,
                                                           int m_real) {
  constexpr bool KSLICED = false;
#include "gemm256w4_tile.inc"

  // ---- fragment read addressing (inline-asm ds_read_b128, immediates carry stage / fragment offsets) --------------
  // (the next eight lines are the fragment addresses of a 32x32x16 loop, which this kernel does not have: nothing reads them and
  // no instruction is emitted for them, but without them hipcc numbers and orders the scalar setup in front of the main loop
  // differently, and the instruction streams are held to the recorded ones: profiles/r08_gemm_refactor_isa.txt.  Remove them
  // together with the next change that moves the kernels' instructions anyway.)
  const int frow = lane & 31, khalf = lane >> 5, fsw = (frow >> 1) & 7;
  uint32_t offA[4], offB[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    const uint32_t lo = frow * 128 + (((ks * 2 + khalf) ^ fsw) << 4);
    offA[ks] = lds_base + (wm * 2) * HALF_BYTES + lo;
    offB[ks] = lds_base + ((2 + wn) * 2) * HALF_BYTES + lo;
  }
  const int frow16 = lane & 15, lq = lane >> 4, fsw16 = (frow16 >> 1) & 7;
  uint32_t offA16[2], offB16[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    const uint32_t lo = frow16 * 128 + (((ks * 4 + lq) ^ fsw16) << 4);
    offA16[ks] = lds_base + (wm * 2) * HALF_BYTES + lo;
    offB16[ks] = lds_base + ((2 + wn) * 2) * HALF_BYTES + lo;
  }
  struct OpSet16 {
    bf16x8 a[8], b[8];
  };
  OpSet16 X16, Y16;
  f32x4 acc16[8][8];  // [i: A row block][j: W column block]; the TRANSPOSED 16x16 block: lane = output row, 4 columns
#define W4_MFMA16(acc_, b_, a_, FIRST_)                                                                            \
  do {                                                                                                             \
    if (W4_ABL(4)) asm volatile("" : "+a"(acc_) : "v"(b_), "v"(a_));                                               \
    else if constexpr (FIRST_) asm volatile(ED_MFMA_16x16x32_ASM " %0, %1, %2, 0" : "=a"(acc_) : "v"(b_), "v"(a_)); \
    else asm volatile(ED_MFMA_16x16x32_ASM " %0, %1, %2, %0" : "+a"(acc_) : "v"(b_), "v"(a_));                      \
  } while (0)
#define W4_WAIT16(s_)                                                                                               \
  asm volatile("s_waitcnt lgkmcnt(0)"                                                                               \
               : "+v"(s_.a[0]), "+v"(s_.a[1]), "+v"(s_.a[2]), "+v"(s_.a[3]), "+v"(s_.a[4]), "+v"(s_.a[5]), "+v"(s_.a[6]), \
                 "+v"(s_.a[7]), "+v"(s_.b[0]), "+v"(s_.b[1]), "+v"(s_.b[2]), "+v"(s_.b[3]), "+v"(s_.b[4]), "+v"(s_.b[5]), \
                 "+v"(s_.b[6]), "+v"(s_.b[7]))
  // fragment r (0..7: A row block r, 8..15: W column block r - 8) of k-step ks, stage buf, into set S
  auto read_frag16 = [&](OpSet16& S, auto R, auto KS, auto BUF) {
    constexpr int r = decltype(R)::value, ks = decltype(KS)::value, buf = decltype(BUF)::value;
    const uint32_t addr = r < 8 ? offA16[ks] : offB16[ks];
    bf16x8& dst = r < 8 ? S.a[r & 7] : S.b[r & 7];
    W4_DSR(dst, addr, buf * HALF_BYTES + (r & 7) * 2048);
  };
  // One k-step: 64 MFMAs on set C (j = W block outer, i = A block inner); the 16 reads of the next
  // k-step (NKS of stage NBUF) into set Nx; DMA: the 16 LDS-DMA instructions of K-tile dma_v into stage DMA_BUF.
  auto kstep16 = [&](OpSet16& C, OpSet16& Nx, auto NKS, auto NBUF, auto DMA, auto DMA_BUF, auto DMA_NEXT, int dma_v,
                     auto FIRST) {
    unroll_seq([&](auto NC) {
      constexpr int n = decltype(NC)::value, j_ = n >> 3, i_ = n & 7;
      constexpr int d = decltype(DMA)::value ? m16_dma(n) : -1;
      if constexpr (d >= 0) dma1(DMA_NEXT, d, decltype(DMA_BUF)::value, dma_v, 1);   // s_mov m0 (the MFMA is its wait state)
      W4_MFMA16(acc16[i_][j_], C.b[j_], C.a[i_], decltype(FIRST)::value);
      if constexpr (m16_read(n) >= 0) read_frag16(Nx, std::integral_constant<int, m16_read(n)>{}, NKS, NBUF);
      if constexpr (d >= 0) dma1(DMA_NEXT, d, decltype(DMA_BUF)::value, dma_v, 2);
    }, std::make_integer_sequence<int, 64>{});
  };
  // One K-tile at stage P.  Entry: X16 holds the fragments of (t, k-step 0).  The LDS-DMA of k-step 1 refills stage P with
  // K-tile v (of the workgroup's next tile if NXT).
  auto ktile16 = [&](auto P, auto NXT, int v, auto FIRST) {
    using Q = std::integral_constant<int, 1 - decltype(P)::value>;
    kstep16(X16, Y16, I1{}, P, TF{}, P, NXT, v, FIRST);
    W4_WAIT16(Y16);                                    // ... and stage P is fully read by this wave
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's share of the next K-tile (stage Q) has landed
    __builtin_amdgcn_s_barrier();
    // k-step 1: fragments of (t + 1, k-step 0) from stage Q (after the tile's last K-tile: the next tile's K-tile 0, or
    // unused) + the LDS-DMA of K-tile v into stage P
    kstep16(Y16, X16, I0{}, Q{}, TT{}, P, NXT, v, TF{});
    W4_WAIT16(X16);
  };
  auto tile16 = [&]() {
    if (!have_k0) {  // first tile of this workgroup: K-tiles 0 and 1
#pragma unroll
      for (int idx = 0; idx < 16; ++idx) dma1(TF{}, idx, 0, 0);
#pragma unroll
      for (int idx = 0; idx < 16; ++idx) dma1(TF{}, idx, 1, 1);
      asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      unroll_seq([&](auto R) { read_frag16(X16, R, I0{}, I0{}); }, std::make_integer_sequence<int, 16>{});
      W4_WAIT16(X16);
    }  // else: the previous tile's K loop streamed K-tiles 0 and 1 and read (K-tile 0, k-step 0) into X16
    ktile16(I0{}, TF{}, 2, TT{});                      // first k-step writes the accumulators (C = 0)
    ktile16(I1{}, TF{}, 3, TF{});
    for (int t = 2; t < nk - 2; t += 2) {              // steady state: no condition anywhere
      ktile16(I0{}, TF{}, t + 2, TF{});
      ktile16(I1{}, TF{}, t + 3, TF{});
    }
    ktile16(I0{}, TT{}, 0, TF{});                      // the last two K-tiles stream the next tile's K-tiles 0 and 1
    ktile16(I1{}, TT{}, 1, TF{});
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");  // the last MFMAs' results before the compiler's accvgpr reads

    // ---- epilogue: lane = output row m, 4 consecutive columns 4 lq .. of each 16-column block.  For 16-bit outputs
    // v_permlane16_swap pairs two blocks (lane groups 0 / 2 take 8 columns of the first, 1 / 3 of the second): one 16-byte
    // store per lane and block pair.
    auto swap_rows = [](uint32_t& lo_keep, uint32_t& hi_keep) {
      const auto r = __builtin_amdgcn_permlane16_swap(lo_keep, hi_keep, false, false);
      lo_keep = r[0];
      hi_keep = r[1];
    };
    const int pair_col = (lq & 1) * 16 + (lq >> 1) * 8;   // first column of this lane's 8 in a 32-column block pair
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (W4_ABL(16)) {
#pragma unroll
        for (int j = 0; j < 8; ++j) asm volatile("" ::"a"(acc16[i][j]));
        continue;
      }
      const int m = m0 + wm * 128 + i * 16 + frow16;
      const bool live = m < M && !(W4_ABL(8) && alpha != 12345.f);
      if constexpr (EPI == ESMDIFF_EPI_SWIGLU_BF16) {
        // W rows interleaved gate / up in blocks of 32: in 64-column group jp, gate blocks 4 jp + b pair with up blocks 4 jp + 2 + b
#pragma unroll
        for (int jp = 0; jp < 2; ++jp) {
          uint32_t p[2][2];
#pragma unroll
          for (int b = 0; b < 2; ++b) {
            float h[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) h[e] = silu_mul(acc16[i][4 * jp + b][e], acc16[i][4 * jp + 2 + b][e]);
            p[b][0] = pack_bf16x2(h[0], h[1]);
            p[b][1] = pack_bf16x2(h[2], h[3]);
          }
          swap_rows(p[0][0], p[1][0]);
          swap_rows(p[0][1], p[1][1]);
          bf16_t* o = reinterpret_cast<bf16_t*>(out) + (int64_t)m * ldc + (n0 + wn * 128 + jp * 64) / 2 + pair_col;
          if (live) *reinterpret_cast<uint4*>(o) = make_uint4(p[0][0], p[0][1], p[1][0], p[1][1]);
        }
      } else if constexpr (EPI == ESMDIFF_EPI_BF16 || EPI == ESMDIFF_EPI_BIAS_GELU_BF16) {
#pragma unroll
        for (int jp = 0; jp < 4; ++jp) {
          const int nb = n0 + wn * 128 + jp * 32;
          uint32_t p[2][2];
#pragma unroll
          for (int b = 0; b < 2; ++b) {
            float h[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) h[e] = acc16[i][2 * jp + b][e];
            if constexpr (EPI == ESMDIFF_EPI_BF16) {
#pragma unroll
              for (int e = 0; e < 4; ++e) h[e] *= alpha;
            } else {
              const f32x4 bb = *reinterpret_cast<const f32x4*>(bias + nb + b * 16 + lq * 4);
#pragma unroll
              for (int e = 0; e < 4; ++e) h[e] = gelu_erf(h[e] + bb[e]);
            }
            p[b][0] = pack_bf16x2(h[0], h[1]);
            p[b][1] = pack_bf16x2(h[2], h[3]);
          }
          swap_rows(p[0][0], p[1][0]);
          swap_rows(p[0][1], p[1][1]);
          bf16_t* o = reinterpret_cast<bf16_t*>(out) + (int64_t)m * ldc + nb + pair_col;
          if (live) *reinterpret_cast<uint4*>(o) = make_uint4(p[0][0], p[0][1], p[1][0], p[1][1]);
        }
      } else if constexpr (EPI == ESMDIFF_EPI_RESID_F32) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const f32x4 v = acc16[i][j];
          if (!live) continue;
          float* o = reinterpret_cast<float*>(out) + (int64_t)m * ldc + n0 + wn * 128 + j * 16 + lq * 4;
          f32x4 x = *reinterpret_cast<const f32x4*>(o);
#pragma unroll
          for (int e = 0; e < 4; ++e) x[e] += v[e] * alpha;
          *reinterpret_cast<f32x4*>(o) = x;
        }
      }
    }
    if constexpr (EPI == ESMDIFF_EPI_BIAS_F32) {
      // column block outer: one bias load and one column bound (the ragged head: columns >= ldc skipped) per block; in row
      // order the compiler hoists all eight blocks' bias and bounds out of the row loop and spills
      // (addresses: the wave's first row as a scalar base + a 32-bit lane offset, 128 x ldc floats)
      float* const obase = reinterpret_cast<float*>(out) + (int64_t)(m0 + wm * 128) * ldc;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int n = n0 + wn * 128 + j * 16 + lq * 4;
        if (W4_ABL(16)) continue;
        const bool col_ok = n + 4 <= ldc;
        const f32x4 bb = col_ok ? *reinterpret_cast<const f32x4*>(bias + n) : f32x4{};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int r = i * 16 + frow16;
          f32x4 v = acc16[i][j];
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] += bb[e];
          if (col_ok && m0 + wm * 128 + r < M && !(W4_ABL(8) && alpha != 12345.f))
            *reinterpret_cast<f32x4*>(obase + (uint32_t)(r * ldc + n)) = v;
        }
      }
    }
  };

  for (int vt = bid; vt < n_tiles; vt += gridDim.x) {
    W4_BEGIN_TILE(vt);
    tile16();
    W4_END_TILE();
  }
#undef W4_MFMA16
#undef W4_WAIT16
}
}  // namespace g4

hipError_t launch_gemm256w4_bf16(const bf16_t* A, const bf16_t* W, void* out, const float* bias, int M, int N, int K,
                                 int ldc, float alpha, int epilogue, hipStream_t stream) {
  using namespace g4;
  if (M <= 0) return hipSuccess;
  if (N % BN != 0 || K % (2 * BK) != 0 || K < 6 * BK || (ldc & 3)) return hipErrorInvalidValue;
  const int tiles_m = (M + BM - 1) / BM, tiles_n = N / BN;
  auto launch = [&](auto kernel) {
    return launch_persistent(kernel, tiles_m * tiles_n, stream, A, W, out, bias, M, N, K, ldc, alpha, tiles_m, tiles_n,
                             (const float*)nullptr, 1.f, 0, 0, 0);
  };
  switch (epilogue) {
    case ESMDIFF_EPI_BF16: return launch(gemm256w4_kernel<ESMDIFF_EPI_BF16>);
    case ESMDIFF_EPI_RESID_F32: return launch(gemm256w4_kernel<ESMDIFF_EPI_RESID_F32>);
    case ESMDIFF_EPI_SWIGLU_BF16: return launch(gemm256w4_kernel<ESMDIFF_EPI_SWIGLU_BF16>);
    case ESMDIFF_EPI_BIAS_GELU_BF16: return launch(gemm256w4_kernel<ESMDIFF_EPI_BIAS_GELU_BF16>);
    case ESMDIFF_EPI_BIAS_F32: return launch(gemm256w4_kernel<ESMDIFF_EPI_BIAS_F32>);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace ed

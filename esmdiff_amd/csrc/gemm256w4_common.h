// gemm256w4_common.h — what the two four-wave 256x256x64 MFMA GEMM kernels share at namespace scope: gemm256w4.hip (bf16 / f16
// operands, v_mfma_f32_16x16x32 loop) and gemm256w4_split.hip (float32-grade products on f16 plane triples, v_mfma_f32_32x32x16_f16
// loop).  What they share inside the kernel body (tile raster, LDS-DMA stream, next-tile hand-over) is gemm256w4_tile.inc.
//
//   workgroup  256 threads = 4 waves as 2 (M) x 2 (N), one wave per SIMD, one workgroup per CU.  Wave tile 128 x 128 = 256
//              accumulator registers, kept in AGPRs (the MFMAs are inline asm with "a" operands); operands, addresses and
//              everything else live in the 256 VGPRs.  The main loops are hand-placed instruction streams.
//   why        r02 ablations of the 8-wave kernel (profiles/r02_gemm_ablations.txt): the fragment reads cost 22 % of the
//              FFN-up launch (about 15 matrix-pipe cycles per ds_read_b128 per SIMD, i.e. the time to move 1 KiB from LDS
//              into the register file), LDS-DMA issue 11 %, barriers and vmcnt waits nothing.  A 128 x 64 wave tile reads
//              6 fragments per 8 MFMAs of 32x32x16, a 128 x 128 one 8 per 16: a third fewer LDS bytes per MFMA.
//   LDS        128 KiB: four pieces (A rows 0-127, A rows 128-255, W rows 0-127, W rows 128-255) x two stages of 16 KiB; a
//              stage of a piece holds 128 rows x 128 bytes of one K-tile (K = 64), its 16-byte chunks swizzled by
//              (row >> 1) & 7, filled by LDS-DMA (global_load_lds_dwordx4).
//   tiles      persistent; the DMA stream runs across tile boundaries exactly as the K-tile indices continue (K-tile nk is
//              K-tile 0 of the workgroup's next tile).  Needs an even number of K-tiles (K % 128 == 0).
#pragma once
#include <stdlib.h>

#include <type_traits>
#include <utility>

#include "ed_half.h"
#include "kernels.h"

namespace ed {

typedef ed_half8 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

namespace g4 {
constexpr int BM = 256, BN = 256, BK = 64;
constexpr int HALF_BYTES = 128 * BK * 2;     // 16 KiB
constexpr int STAGE_BYTES = 4 * HALF_BYTES;  // 64 KiB
// Raster of the tiles an XCD walks (its 32 CUs run 32 consecutive tiles at a time and share that XCD's 4 MB L2): groups of
// GROUP_M tile rows, column by column: a round is GROUP_M rows x 32 / GROUP_M columns (other group sizes and the column-major
// walk measured no better: profiles/r06_gemm_raster_ab.txt)
constexpr int GROUP_M = 8;
// ablation builds (-DED_ABL4=<bits>, wrong results by construction): 1 no fragment reads, 2 no LDS-DMA, 4 no MFMA,
// 8 no global stores (epilogue arithmetic kept), 16 no epilogue at all
#ifndef ED_ABL4
#define ED_ABL4 0
#endif
#define W4_ABL(bit) (((ED_ABL4) & (bit)) != 0)

// one fragment read (inline asm: the immediate carries the stage / fragment offset)
#define W4_DSR(dst, addr, imm)                                                                    \
  do {                                                                                            \
    if (!W4_ABL(1)) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "i"(imm)); \
    else asm volatile("" : "=v"(dst));                                                            \
  } while (0)

using I0 = std::integral_constant<int, 0>;
using I1 = std::integral_constant<int, 1>;
using I2 = std::integral_constant<int, 2>;
using I3 = std::integral_constant<int, 3>;
using TF = std::false_type;
using TT = std::true_type;

// Launch of a persistent 256x256 kernel: one workgroup per CU, the CU count rounded down to a multiple of 8 (the XCD-aware raster
// deals tiles to 8 XCDs in turn), never more workgroups than tiles; both LDS stages as dynamic shared memory.
inline int persistent_grid(int n_tiles) {
  static const int n_cu = [] {   // (one device model per process: every gfx950 in a node has the same CU count)
    int dev = 0, n = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
    return n >= 8 ? (n / 8) * 8 : 8;
  }();
  return n_tiles < n_cu ? n_tiles : n_cu;
}
template <typename... P, typename... Args>
inline hipError_t launch_persistent(void (*kernel)(P...), int n_tiles, hipStream_t stream, Args... args) {
  const size_t lds = 2 * STAGE_BYTES;
  if (const hipError_t a_ = ensure_dynamic_lds((const void*)kernel, (int)lds); a_ != hipSuccess) return a_;
  hipLaunchKernelGGL(kernel, dim3(persistent_grid(n_tiles)), dim3(256), lds, stream, args...);
  return hipGetLastError();
}
}  // namespace g4
}  // namespace ed

// gemm256w4_tile.inc — the part of the kernel body that gemm256w4_kernel (gemm256w4.hip) and gemm256w4_split_kernel
// (gemm256w4_split.hip) share, included as text at the top of both (as attention_kernel.inc is): the XCD-aware tile raster,
// the LDS-DMA source offsets and instruction stream, and the hand-over to the workgroup's next tile.
//
// Expects in scope: the kernel arguments A, W, M, K, tiles_m, tiles_n, ld_ab, m_pad, m_real and a constexpr bool KSLICED (the
// K-sliced form of the split kernel; the last three arguments are read only then).
// Provides: smem, n_tiles, m0 / n0 (origin of the current tile), lane, wave, wm / wn, lds_base, nk, have_k0, dma1, and the head
// and tail of the persistent loop
//   for (int vt = bid; vt < n_tiles; vt += gridDim.x) { W4_BEGIN_TILE(vt); <K loop and epilogue>; W4_END_TILE(); }
// Text and macros, not lambdas or functions, on purpose: hipcc allocates the registers of the hand-placed main loops differently
// as soon as these statements sit behind a call boundary, even an inlined one (profiles/r08_gemm_refactor_isa.txt).
  extern __shared__ __attribute__((aligned(16))) char smem[];  // 2 x 64 KiB

  const int n_tiles = tiles_m * tiles_n, bid = blockIdx.x;
  auto tile_origin = [&](int vt, int& m0_, int& n0_) {
    const int xcd = vt & 7, qq = n_tiles >> 3, rr = n_tiles & 7;
    const int lin = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + (vt >> 3);
    const int per_group = GROUP_M * tiles_n;
    const int grp = lin / per_group, in_grp = lin - grp * per_group;
    const int gm0 = grp * GROUP_M;
    const int gsz = min(GROUP_M, tiles_m - gm0);
    m0_ = (gm0 + in_grp % gsz) * BM;
    n0_ = (in_grp / gsz) * BN;
  };
  int m0, n0;
  tile_origin(bid, m0, n0);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;

  // ---- LDS-DMA sources.  Piece p = 0,1: A rows 0-127 / 128-255; p = 2,3: W rows.  A piece is 16 instructions of 8 rows;
  // this wave issues i = 0..3, instruction i covering rows (i*4 + wave)*8 + (lane>>3) of the piece. ------------------
  const int srow = lane >> 3;
  const int schunk = (lane & 7) ^ ((wave * 4 + (lane >> 4)) & 7);  // (row >> 1) & 7 of that row
  uint32_t a_off[2][4], w_off[2][4], a_offn[2][4], w_offn[2][4];     // current tile / the workgroup's next tile
  auto set_offsets = [&](uint32_t (&ao)[2][4], uint32_t (&wo)[2][4], int m0_, int n0_) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if constexpr (KSLICED) {   // virtual row block m0_ / m_pad = K slice of the physical rows (gemm256w4_split.hip)
          const int slice = m0_ / m_pad;
          const int am = min(m0_ - slice * m_pad + h * 128 + (i * 4 + wave) * 8 + srow, m_real - 1);
          const int64_t col = (int64_t)slice * K + schunk * 8;
          ao[h][i] = (uint32_t)(((int64_t)am * ld_ab + col) * 2);
          wo[h][i] = (uint32_t)(((int64_t)(n0_ + h * 128 + (i * 4 + wave) * 8 + srow) * ld_ab + col) * 2);
        } else {
          const int am = min(m0_ + h * 128 + (i * 4 + wave) * 8 + srow, M - 1);
          ao[h][i] = (uint32_t)(((int64_t)am * K + schunk * 8) * 2);
          wo[h][i] = (uint32_t)(((int64_t)(n0_ + h * 128 + (i * 4 + wave) * 8 + srow) * K + schunk * 8) * 2);
        }
      }
    }
  };
  set_offsets(a_off, w_off, m0, n0);
  constexpr int kstride = BK * 2;
  const char* Ab = reinterpret_cast<const char*>(A);
  const char* Wb = reinterpret_cast<const char*>(W);
  const uint32_t lds_base = (uint32_t)(uintptr_t)((__attribute__((address_space(3))) char*)smem);
  // One LDS-DMA instruction.  M0 (the LDS destination) is written and consumed inside one statement, or in two: nothing else in
  // these kernels uses M0 (plain ds_read / ds_write do not), so it is not saved and restored around each of the 16 instructions
  // per K-tile.  In the main loops the s_mov m0 (phase 1) goes in front of the MFMA of its gap and the load (phase 2) behind it:
  // the MFMA is the wait state the pair needs, which saves the s_nop; nothing else may write M0 in between, and nothing does.
  // Phase 0 is the prologue's form, both in one statement.  (Cache policies on these loads measured no better than the default:
  // profiles/r03_gemm_cache_policy.txt.)  The A and the W pieces keep an asm statement each, although the two are the same
  // text: with one statement hipcc orders the prologue's scalar address arithmetic of gemm256w4_kernel differently, and the
  // instruction streams of both kernels are held to the recorded ones (profiles/r08_gemm_refactor_isa.txt).
  auto glds = [&](const char* sbase, uint32_t voff, uint32_t lds_dst, int phase, bool is_w) {
    if (phase == 0) {
      if (is_w) asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" : : "s"(lds_dst), "v"(voff), "s"(sbase) : "memory");
      else asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" : : "s"(lds_dst), "v"(voff), "s"(sbase) : "memory");
    } else if (phase == 1) {
      asm volatile("s_mov_b32 m0, %0" : : "s"(lds_dst) : "memory");
    } else {
      if (is_w) asm volatile("global_load_lds_dwordx4 %0, %1" : : "v"(voff), "s"(sbase) : "memory");
      else asm volatile("global_load_lds_dwordx4 %0, %1" : : "v"(voff), "s"(sbase) : "memory");
    }
  };
  int xnext = 0;  // wave-uniform: this workgroup has another tile after the current one
  const int nk = K / BK;
  // LDS-DMA instruction idx = p*4 + i of K-tile v into stage `buf`.  NEXT: v counts K-tiles of the workgroup's NEXT tile
  // (only the last two K-tiles of a tile stream the next tile's first two: the steady-state loop has no condition at all).
  auto dma1 = [&](auto NEXT, int idx, int buf, int v, int phase = 0) {
    if (W4_ABL(2)) return;
    const int p = idx >> 2, i = idx & 3;
    const uint32_t dst = lds_base + (p * 2 + buf) * HALF_BYTES + (i * 4 + wave) * 1024;
    const char* sb = (p < 2 ? Ab : Wb) + (size_t)v * kstride;  // one scalar base per operand and K-tile
    if constexpr (!decltype(NEXT)::value) {
      glds(sb, p < 2 ? a_off[p][i] : w_off[p - 2][i], dst, phase, p >= 2);
    } else {
      if (xnext) glds(sb, p < 2 ? a_offn[p][i] : w_offn[p - 2][i], dst, phase, p >= 2);
    }
  };

  bool have_k0 = false;  // K-tiles 0 and 1 of the current tile were streamed by the previous tile's K loop
// head of the persistent loop: is there a next tile for this workgroup, and where its operands are
#define W4_BEGIN_TILE(vt)                                          \
  const int vtn = (vt) + gridDim.x;                                \
  xnext = __builtin_amdgcn_readfirstlane(vtn < n_tiles ? 1 : 0);   \
  int m0n = 0, n0n = 0;                                            \
  if (xnext) {                                                     \
    tile_origin(vtn, m0n, n0n);                                    \
    set_offsets(a_offn, w_offn, m0n, n0n);                         \
  }
// tail: the next tile (whose K-tiles 0 and 1 the K loop has streamed) becomes the current one
#define W4_END_TILE()                                              \
  if (xnext) {                                                     \
    have_k0 = true;                                                \
    m0 = m0n;                                                      \
    n0 = n0n;                                                      \
    _Pragma("unroll") for (int h = 0; h < 2; ++h)                  \
      _Pragma("unroll") for (int i = 0; i < 4; ++i) {              \
        a_off[h][i] = a_offn[h][i];                                \
        w_off[h][i] = w_offn[h][i];                                \
      }                                                            \
  }

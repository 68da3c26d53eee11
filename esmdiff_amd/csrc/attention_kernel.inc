// attention_kernel.inc — body of the flash-style attention kernel; included by attention.hip once per register budget
// (ED_ATTN_NAME, ED_ATTN_WPE = waves per SIMD the register allocation must allow, ED_ATTN_RAGGED = 1 for the per-sample
// key length form).  See attention.hip for the design.
__global__ __attribute__((amdgpu_flat_work_group_size(64, 640), amdgpu_waves_per_eu(ED_ATTN_WPE, ED_ATTN_WPE))) void ED_ATTN_NAME(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ qkv, bf16_t* __restrict__ ctx,
#if ED_ATTN_RAGGED
    int L, int H, int BH, int nqb, const int32_t* __restrict__ lens) {
#else
    int L, int H, int BH, int nqb) {
#endif
  extern __shared__ __attribute__((aligned(16))) char smem[];  // [stage][K 8K | V 8K], 2 stages (1 when L <= 64)
#ifdef ED_ATTN_TRACE
  // debug build (-DED_ATTN_TRACE): s_memtime stamps of every wave of the first 512 workgroups -> g_attn_trace[wg][wave][32]
  unsigned long long* tbuf = blockIdx.x < 512 ? g_attn_trace + ((size_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 32 : nullptr;
  int tslot = 0;
#define ED_TR(dep)                                                                                    \
  do {                                                                                                \
    unsigned long long t_;                                                                            \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) : "v"(dep) : "memory");            \
    if (tbuf && (threadIdx.x & 63) == 0 && tslot < 32) tbuf[tslot] = t_;                              \
    ++tslot;                                                                                          \
  } while (0)
  ED_TR(0.f);
#else
#define ED_TR(dep) do { } while (0)
#endif

  // XCD-aware block mapping (block id i runs on XCD i % 8, each XCD has its own L2): the nqb query blocks of one (batch,
  // head) get ids 8 apart, i.e. the SAME XCD and neighbouring dispatch slots, so the K/V rows they all stream are fetched
  // from HBM once and served from that XCD's L2 to the others (66 KB per head at L = 258).  With the plain (qblock, bh)
  // grid the three query blocks of a head sat on three XCDs and K/V crossed the fabric three times: 632 MB per launch
  // instead of 316 MB — the kernel was bandwidth-bound on its own re-reads.
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int bh = (slot / nqb) * 8 + xcd, qb = slot - (slot / nqb) * nqb;
  if (bh >= BH) return;
  const int b = bh / H, h = bh - b * H;
#if ED_ATTN_RAGGED
  // ragged batch: sample b is valid on tokens [0, Lv); keys from Lv on are masked like keys >= L, query rows from Lv on are
  // written as zeros.  Every valid query sees the tiles, clamps and tail variant of a launch at L = Lv: bit-identical rows.
  const int Lv = lens ? lens[b] : L;
#else
  const int Lv = L;
#endif
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int NW = __builtin_amdgcn_readfirstlane((int)blockDim.x >> 6);
  const int q0 = (qb * NW + wave) * 32;
  const bool active = q0 < Lv;  // wave-uniform
  const int qi = lane & 31, hi = lane >> 5;

  const int D = H * 64;
  const bf16_t* kbase = k + (int64_t)b * L * D + h * 64;                 // K of this (batch, head), token 0; row stride D
  const int ldq = 3 * D;                                                 // qkv row stride (elements)
  const bf16_t* vbase = qkv + (int64_t)b * L * ldq + 2 * H * 64 + h * 64;  // V of this (batch, head), token 0

  // ---- LDS-DMA: per tile 8 instructions for K (64 rows x 128 B) + 8 for V, dealt round-robin to the NW waves ------
  // instruction g (row group, 0..7) covers rows g*8 + (lane>>3), 16-byte slot lane&7
  const int srow = lane >> 3;
  const int vchunk = (lane & 7) ^ (2 * (srow & 3));  // V: logical chunk stored at slot lane&7 of row r (r & 3 == srow & 3)
  auto stage = [&](int buf, int kt) {
    char* base = smem + buf * (2 * KV_BYTES);
    for (int g = wave; g < 8; g += NW) {  // wave-uniform
      char* d = base + g * 1024;
      const int schunk = (lane & 7) ^ (((lane >> 4) + 4 * (g & 1)) & 7);  // (row >> 1) & 7 with row = g*8 + srow
      const int tok = min(kt * KV_TILE + g * 8 + srow, Lv - 1);  // keys >= Lv are masked / get weight 0; any finite row will do
      glds16a(kbase + (int64_t)tok * D + schunk * 8, d);
      glds16a(vbase + (int64_t)tok * ldq + vchunk * 8, d + KV_BYTES);
    }
  };

  // ---- Q^T fragments (B operand): lane -> query qi, d chunk ks*2 + hi -------------------------
  bf16x8 qf[4];
  {
    const bf16_t* qrow = q + ((int64_t)b * L + min(q0 + qi, Lv - 1)) * D + h * 64;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(qrow + (ks * 2 + hi) * 8);
  }

  f32x16 o[2];
#pragma unroll
  for (int d = 0; d < 2; ++d)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[d][r] = 0.f;
  float m_run = -1e30f, l_run = 0.f;

  const int fsw = (qi >> 1) & 7;
  // transpose-read addressing: lane (g = lane>>4, i = lane&15) supplies V[key0 + 4*(g>>1) + (i>>2)][d0 + 16*(g&1) +
  // 4*(i&3) ..+3] and receives d = d0 + (lane&31), keys key0 + 4*hi + 0..3 (key0 a multiple of 8, so row&3 = i>>2)
  const int tg = lane >> 4, ti = lane & 15;
  const int tr_row = 4 * (tg >> 1) + (ti >> 2);                    // + key0
  const int tr_c = 2 * (tg & 1) + ((ti & 3) >> 1);                 // 16-byte chunk within the 32-d half
  const int tr_swz = 2 * (ti >> 2);                                // 2 * (row & 3)
  int tr_off[2];
#pragma unroll
  for (int d = 0; d < 2; ++d) tr_off[d] = tr_row * 128 + (((d * 4 + tr_c) ^ tr_swz) << 4) + (ti & 1) * 8;
#if ED_ATTN_RAGGED
  // zero context rows [r0, min(r0 + 32, L)) of this (batch, head): lane (qi, hi) writes row r0 + qi, columns 4 hi + 8 g + 32 d ..+3
  auto zero_rows = [&](int r0) {
    const int qrow = r0 + qi;
    if (qrow >= L) return;
    bf16_t* dst = ctx + ((int64_t)b * L + qrow) * (H * 64) + h * 64;
#pragma unroll
    for (int d = 0; d < 2; ++d)
#pragma unroll
      for (int g = 0; g < 4; ++g) *reinterpret_cast<uint2*>(dst + d * 32 + g * 8 + 4 * hi) = make_uint2(0u, 0u);
  };
  if (qb * NW * 32 >= Lv) {  // workgroup-uniform: every query of this workgroup is padding, nothing to stage
    if (q0 < L) zero_rows(q0);
    return;
  }
#endif
  const int nkt = (Lv + KV_TILE - 1) / KV_TILE;
  stage(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // Rescale threshold (log2 units): the running max is only raised when a tile's max exceeds it by more than
  // THR, so P <= 2^THR instead of <= 1 (exact in f32 accumulation; bf16 P keeps its relative precision) and the
  // 32-register O rescale is skipped on almost every tile.  The decision sits between S and P of the SAME tile
  // and no P·V is pending across it, so everything at the old scale (O and l) is rescaled exactly once.
  constexpr float THR = 8.0f;
  auto tile = [&](int kt, auto MASKED, auto HALF) {  // HALF: at most 32 valid keys left (e.g. L = 258: keys 256, 257)
    constexpr int NT = decltype(HALF)::value ? 1 : 2;
    const int cur = ED_ATTN_ABL & 2 ? 0 : (kt & 1);
    ED_TR(l_run);                                   // tile start
    if (kt + 1 < nkt && !(ED_ATTN_ABL & 2)) stage(cur ^ 1, kt + 1);
    if (active) {
      const char* kl = smem + cur * (2 * KV_BYTES);
      const char* vl = kl + KV_BYTES;
      f32x16 s[2];
#pragma unroll
      for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int r = 0; r < 16; ++r) s[t][r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          const bf16x8 kf =
              *reinterpret_cast<const bf16x8*>(kl + (t * 32 + qi) * 128 + (((ks * 2 + hi) ^ fsw) << 4));
          s[t] = ED_MFMA_32x32x16(kf, qf[ks], s[t]);
        }
      }
      if constexpr (decltype(MASKED)::value) {  // keys >= Lv exist only in the last tile
        const int lim = Lv - kt * KV_TILE - 4 * hi;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (t * 32 + (r & 3) + 8 * (r >> 2) >= lim) s[t][r] = -1e30f;
      }
      float mx = s[0][0];
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[t][r]);
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      ED_TR(mx);                                    // scores and their maximum are there (QK^T done)
      if (!__all(mx - m_run <= THR)) {
        const float m_new = fmaxf(m_run, mx);
        const float alpha = fast_exp2(m_run - m_new);
        m_run = m_new;
        l_run *= alpha;
#pragma unroll
        for (int d = 0; d < 2; ++d)
#pragma unroll
          for (int r = 0; r < 16; ++r) o[d][r] *= alpha;
      }
      float ps = 0.f;
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          s[t][r] = (ED_ATTN_ABL & 1) ? s[t][r] - m_run : fast_exp2(s[t][r] - m_run);
          ps += s[t][r];
        }
      l_run += ps;
#pragma unroll
      for (int kk = 0; kk < 2 * NT; ++kk) {
        const int t = kk >> 1, r0 = (kk & 1) * 8;
        union { uint32_t u[4]; bf16x8 v; } pb;
#pragma unroll
        for (int e = 0; e < 4; ++e) pb.u[e] = pk_bf16(s[t][r0 + 2 * e], s[t][r0 + 2 * e + 1]);
#pragma unroll
        for (int d = 0; d < 2; ++d) {
          union { bf16x4 h[2]; bf16x8 v; } va;
          va.h[0] = lds_read_tr16(vl + kk * 16 * 128 + tr_off[d]);        // keys kk*16 + 4*hi + 0..3
          va.h[1] = lds_read_tr16(vl + (kk * 16 + 8) * 128 + tr_off[d]);  // keys kk*16 + 8 + 4*hi + 0..3
          if (!(ED_ATTN_ABL & 8)) o[d] = ED_MFMA_32x32x16(va.v, pb.v, o[d]);
          else asm volatile("" :: "v"(va.v), "v"(pb.v));
        }
      }
    }
    ED_TR(o[1][15]);                                // softmax + P.V done
    if (!(ED_ATTN_ABL & 4)) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      ED_TR(l_run);                                 // own share of the next tile landed
      __syncthreads();
    }
    ED_TR(l_run);                                   // past the barrier
  };
  for (int kt = 0; kt + 1 < nkt; ++kt) tile(kt, std::false_type{}, std::false_type{});
  const int tail = Lv - (nkt - 1) * KV_TILE;  // valid keys of the last tile, 1..64
  if (tail <= 32) tile(nkt - 1, std::true_type{}, std::true_type{});
  else if (tail < KV_TILE) tile(nkt - 1, std::true_type{}, std::false_type{});
  else tile(nkt - 1, std::false_type{}, std::false_type{});

  ED_TR(l_run);
#if ED_ATTN_RAGGED
  if (!active) {
    if (q0 < L) zero_rows(q0);
    return;
  }
#else
  if (!active) return;
#endif
  const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
  const float inv = 1.0f / l_tot;
  const int qrow = q0 + qi;
#if ED_ATTN_RAGGED
  if (qrow >= Lv && qrow < L) zero_rows(q0);
#endif
  if (qrow < Lv) {
    bf16_t* dst = ctx + ((int64_t)b * L + qrow) * (H * 64) + h * 64;
#pragma unroll
    for (int d = 0; d < 2; ++d)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        uint2 p;
        p.x = pk_bf16(o[d][g * 4 + 0] * inv, o[d][g * 4 + 1] * inv);
        p.y = pk_bf16(o[d][g * 4 + 2] * inv, o[d][g * 4 + 3] * inv);
        *reinterpret_cast<uint2*>(dst + d * 32 + g * 8 + 4 * hi) = p;
      }
  }
}


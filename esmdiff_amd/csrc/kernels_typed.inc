// kernels_typed.inc — the launchers of the units compiled once per 16-bit operand type (build.py: F16_UNITS; ed_half.h), and
// nothing else: included by kernels.h (namespace ed, bf16) and by engine.h a second time under `#define ed ed16` (f16), so every
// name declared here is defined in both namespaces.  No include guard.
namespace ed {

// ---- gemm.hip --------------------------------------------------------------------------------
// out = epilogue(A[M,K] · W[N,K]^T); K % 64 == 0, N % 128 == 0 (weights are padded at load time).
// ws (optional): split-K workspace for the small-M path — room for f32 partial tiles, owned by ONE launch queue
// (concurrent launches need their own).  Without it every tile runs its whole K range.
// n_valid is informative only: neither kernel reads it.  ESMDIFF_EPI_BIAS_F32 skips a 4-column group only when it would cross
// ldc; columns n_valid .. ldc-1 are written from the (zero-padded) weight rows and the bias, so the caller allocates ldc for them.
using GemmWorkspace = ::EdGemmWorkspace;   // (one type for both operand-type builds, kernels.h)
hipError_t launch_gemm_bf16(const bf16_t* A, const bf16_t* W, void* out, const float* bias, int M, int N,
                            int K, int ldc, int n_valid, float alpha, int epilogue, hipStream_t stream,
                            const GemmWorkspace* ws = nullptr);

// the kernel launch_gemm_bf16 would pick for (M, N, K), as text
void describe_gemm(int M, int N, int K, size_t ws_floats, char* out, size_t cap);
// ... and as numbers: 256x256 kernel or not, rows per tile, K slices, LDS stages (esmdiff_describe_gemm_choice)
void describe_gemm_choice(int M, int N, int K, size_t ws_floats, int* w4, int* rows, int* S, int* stages);

// Row count below which a (sub-)batch takes the small-batch path (DESIGN 3.8).
inline int small_max_rows() {
  return 1152;  // r02: 1 024 -> 1 152 (+4 % at 1 032 - 1 080 rows; 2 048 loses 5 - 20 % from 1 440 rows)
}

// Small-batch path (M < small_max_rows()): the product as S raw f32 K-slice planes in `ws` (plane stride `stride` floats, row stride
// N), consumed by launch_add_partials_layernorm_bf16.  S = gemm_partial_splits(N, K), a function of the shape only.
using GemmPartials = ::EdGemmPartials;
int gemm_partial_splits(int N, int K);
hipError_t launch_gemm_partials(const bf16_t* A, const bf16_t* W, const GemmWorkspace* ws, int M, int N, int K,
                                hipStream_t stream, GemmPartials* res);

// gemm256w4.hip: the same tile with 4 waves x 128x128 wave tiles, hand-placed v_mfma_f32_16x16x32 main loop, accumulators in
// AGPRs; K % 128 == 0
hipError_t launch_gemm256w4_bf16(const bf16_t* A, const bf16_t* W, void* out, const float* bias, int M, int N,
                                 int K, int ldc, float alpha, int epilogue, hipStream_t stream);

// ---- norm.hip --------------------------------------------------------------------------------
hipError_t launch_layernorm_bf16(const float* x, const float* w, const float* b, bf16_t* y, int M, int D,
                                 hipStream_t stream);
// v = (x + delta) + delta2 (bf16 or null each); x = v if write_x; y = LayerNorm(v) * w (+ b)
hipError_t launch_add_layernorm_bf16(float* x, const bf16_t* delta, const bf16_t* delta2, int write_x, const float* w,
                                     const float* b, bf16_t* y, int M, int D, hipStream_t stream);
// the same on M compact rows: v[i] = (x[rows[i]] + delta[rows[i]]) + delta2[i] (delta / delta2 16-bit or null; x, delta full-size,
// delta2 compact); x_out[i] = v[i]; y[i] = LayerNorm(v[i]) * w (+ b)
hipError_t launch_add_layernorm_rows_bf16(const float* x, const bf16_t* delta, const int32_t* rows, const bf16_t* delta2, float* x_out,
                                          const float* w, const float* b, bf16_t* y, int M, int D, hipStream_t stream);
// x += alpha * (P[0] + P[1] + ... + P[S-1]) (f32 K-slice planes of a branch linear); x written back;
// y = LayerNorm(x) * w (+ b)
hipError_t launch_add_partials_layernorm_bf16(float* x, const GemmPartials& P, int N, float alpha, const float* w,
                                              const float* b, bf16_t* y, int M, int D, hipStream_t stream);
hipError_t launch_layernorm_bf16_in(const bf16_t* x, const float* w, const float* b, bf16_t* y, int M, int D,
                                    hipStream_t stream);
// qkv bf16 [M,3D] -> q,k bf16 [M,D] token-major (LayerNorm over D, rotary, q pre-scaled); v stays in qkv
hipError_t launch_qk_norm_rope(const bf16_t* qkv, const float* q_ln_w, const float* k_ln_w,
                               const float* rope_cos, const float* rope_sin, bf16_t* q, bf16_t* k,
                               int B, int L, int H, hipStream_t stream);

// ---- attention.hip ---------------------------------------------------------------------------
// q,k [B*L, H*64] token-major, v read in place from qkv [B*L, 3*H*64] (columns 2*H*64 ..) -> ctx bf16 [B*L, H*64].
// lens (device, [B], each in 1..L, or null = all L): sample b is valid on tokens [0, lens[b]); keys beyond are masked and
// its context rows from lens[b] on are written as zeros.
hipError_t launch_attention(const bf16_t* q, const bf16_t* k, const bf16_t* qkv, bf16_t* ctx, int B, int L,
                            int H, hipStream_t stream, const int32_t* lens = nullptr);

// ---- geom.hip --------------------------------------------------------------------------------
// P bf16 [B*L, 15*VH] (proj output) + frames -> out bf16 [B*L, 3*VH]; w_rot / w_dist = softplus(scale) per head
hipError_t launch_geom_attention(const bf16_t* P, const float* rot, const float* trans, const uint8_t* fmask,
                                 const float* w_rot, const float* w_dist, bf16_t* out, int B, int L, int VH,
                                 hipStream_t stream);

hipError_t launch_geom_attention_f32(const float* P, const float* rot, const float* trans, const uint8_t* fmask,
                                     const float* w_rot, const float* w_dist, float* out, int B, int L, int VH,
                                     hipStream_t stream);

// ---- convert.hip (weight preparation at engine create) ---------------------------------------
hipError_t launch_to_bf16(const void* src, int src_dtype, bf16_t* dst, int64_t n, hipStream_t stream);
hipError_t launch_to_f32(const void* src, int src_dtype, float* dst, int64_t n, hipStream_t stream);
// dst rows: blocks of 32: [gate 32t..32t+31 | up 32t..32t+31]; src [2H, K]: gate rows 0..H-1, up rows H..2H-1
hipError_t launch_interleave_swiglu(const void* src, int src_dtype, bf16_t* dst, int H, int K,
                                    hipStream_t stream);

}  // namespace ed

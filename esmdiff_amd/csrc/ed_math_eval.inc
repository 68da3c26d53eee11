// ed_math_eval.inc — the shared math of csrc/ed_math.h, evaluated element by element INSIDE the unit that includes this file
// (esmdiff_math_eval in esmdiff_hip_test.h; tests/test_gpu_shared_math.py).  sampler.hip, score.hip and gibbs.hip each inline their own
// copy of ed_math.h under their own compiler flags; the bit-exact tests of those units rest on every copy giving the host's bits.
// This body is instantiated once per unit, so what it measures is that unit's copy.
//
// The including unit defines ED_MATH_EVAL_UNIT (sampler / score / gibbs) first, inside namespace ed, after ed_math.h and kernels.h.
//   kind 0  out f32 = ed_expf(in f32)
//   kind 1  out f32 = ed_logf(in f32)
//   kind 2  out f32 = 1e-10f - ed_logf(in f32 + 1e-10f): the race's noise, as the three kernels write it
//   kind 3  out f32 = ed_philox_uniform(seed, sample, step, l, v) of in, records of esmdiff_math_eval_philox
#define ED_MATH_EVAL_CAT2(a, b) a##b
#define ED_MATH_EVAL_CAT(a, b) ED_MATH_EVAL_CAT2(a, b)
#define ED_MATH_EVAL_KERNEL ED_MATH_EVAL_CAT(math_eval_kernel_, ED_MATH_EVAL_UNIT)
#define ED_MATH_EVAL_LAUNCH ED_MATH_EVAL_CAT(launch_math_eval_, ED_MATH_EVAL_UNIT)

__global__ __launch_bounds__(256) void ED_MATH_EVAL_KERNEL(int kind, const void* __restrict__ in, float* __restrict__ out, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    float y;
    if (kind == 3) {
      const esmdiff_math_eval_philox r = static_cast<const esmdiff_math_eval_philox*>(in)[i];
      y = ed_philox_uniform(r.seed, r.sample, r.step, r.l, r.v);
    } else {
      const float x = static_cast<const float*>(in)[i];
      if (kind == 0) {
        y = ed_expf(x);
      } else if (kind == 1) {
        y = ed_logf(x);
      } else {
        y = 1e-10f - ed_logf(x + 1e-10f);
      }
    }
    out[i] = y;
  }
}

hipError_t ED_MATH_EVAL_LAUNCH(int kind, const void* in, float* out, int64_t n, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  const int64_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(ED_MATH_EVAL_KERNEL, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, stream, kind, in, out, n);
  return hipGetLastError();
}

#undef ED_MATH_EVAL_LAUNCH
#undef ED_MATH_EVAL_KERNEL
#undef ED_MATH_EVAL_CAT
#undef ED_MATH_EVAL_CAT2

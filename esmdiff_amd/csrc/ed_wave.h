// ed_wave.h — the two wave-level reductions of the canonical row order (oracle/csrc/sampler_oracle.c), shared by the units that
// must reproduce it bit for bit: sampler.hip (ddpm_step_kernel) and score.hip (nelbo_rows_kernel, nelbo_reduce_kernel).
// Device only; wave64.
#pragma once
#include <hip/hip_runtime.h>

namespace ed {

__device__ __forceinline__ float wave_halving_sum(float v) {
  // t[i] = t[i] + t[i+off], off = 32..1; lane 0 ends with the canonical tree value
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_down(v, off, 64);
  return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

}  // namespace ed

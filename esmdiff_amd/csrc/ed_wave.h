// ed_wave.h — the wave-level reductions that more than one unit uses.  Device only; wave64.
//   wave_halving_sum, wave_max   the canonical row order (oracle/csrc/sampler_oracle.c), for the units that must reproduce it bit
//                                for bit: sampler.hip (ddpm_step_kernel) and score.hip (nelbo_rows_kernel, nelbo_reduce_kernel)
//   wave_sum (double, int)       the xor butterfly of superpose.hip and lddt.hip: a fixed order, every lane ends with the same bits
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

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
  return v;
}

}  // namespace ed

// ed_wave.h — the wave-level reductions that more than one unit uses.  Device only; wave64.
//   wave_halving_sum, wave_max   the canonical row order (oracle/csrc/sampler_oracle.c), for the units that must reproduce it bit
//                                for bit: sampler.hip (ddpm_step_kernel) and score.hip (nelbo_rows_kernel, nelbo_reduce_kernel)
//   wave_sum (double, int)       the xor butterfly of superpose.hip and lddt.hip: a fixed order, every lane ends with the same bits
//   wave_max (double), tree8     the largest of 64 float64 (no order), and the fixed tree that combines eight wave sums
//   WaveTeam, wave_team          the team arithmetic of the frame-per-team kernels (shape.hip, sasa.hip)
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

__device__ __forceinline__ double wave_max(double v) {   // a compare and a select, not fmax: NaN never replaces a number
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double o = __shfl_xor(v, off, 64);
    v = o > v ? o : v;
  }
  return v;
}

__device__ __forceinline__ double tree8(const double* s) { return ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7])); }

// Where a thread of wave `wave` (wave-uniform: readfirstlane(threadIdx.x >> 6)) stands when a workgroup of `waves` waves is cut into
// teams of W waves (W divides `waves`), a frame per team.
struct WaveTeam {
  int W, teams, team;                                    // waves per team, teams per workgroup, this thread's team
  int w, lane, T;                                        // its wave in the team and lane in the wave; the team's threads: thread w * 64 + lane of T
};

__device__ __forceinline__ WaveTeam wave_team(int wave, int W, int waves) {
  WaveTeam g;
  g.W = W, g.teams = waves / W, g.team = wave / W;
  g.w = wave % W, g.lane = threadIdx.x & 63, g.T = 64 * W;
  return g;
}

}  // namespace ed

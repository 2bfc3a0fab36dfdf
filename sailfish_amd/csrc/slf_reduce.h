// Deterministic double-precision sums inside a workgroup, shared by the kernels that leave sums on the device
// (slf_stats.hip, slf_force.hip): no floating-point atomics, the launch shape alone fixes the order of every addition --
// lane -> wave (shuffle tree) -> workgroup (LDS, wave order).  Device code only.
#pragma once
#include <hip/hip_runtime.h>

namespace slf {

// sum over the 64 lanes of a wave, fixed tree; the total is in lane 0
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = v + __shfl_down(v, off, 64);
  return v;
}

// Sum of the N values every thread of the workgroup holds: wave trees, then thread 0 adds the waves in index order.
// Valid in thread 0 only.  red: N * (blockDim.x / 64) doubles of LDS.
template <int N>
__device__ __forceinline__ void block_sum(double (&v)[N], double* red) {
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6, nwaves = ((int)blockDim.x + 63) >> 6;
#pragma unroll
  for (int k = 0; k < N; k++) {
    v[k] = wave_sum(v[k]);
    if (lane == 0) red[k * nwaves + wave] = v[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < N; k++) {
      double s = red[k * nwaves];
      for (int w = 1; w < nwaves; w++) s = s + red[k * nwaves + w];
      v[k] = s;
    }
  }
}

}  // namespace slf

// The fixed-order workgroup sum of the optimizer's gradient norm and of the evaluation metrics (device code).
#pragma once
#include <hip/hip_runtime.h>

// K sums over a workgroup of 64 * WAVES threads in a fixed order: the lanes of a wave by halving (offset 32 down to 1),
// then the waves 0, 1, ... WAVES - 1; valid in thread 0.  Every caller's result depends on exactly this order: no xor
// butterfly, no atomics.
//   * The leading barrier lets a kernel call this more than once (an earlier call's reader of wave_sum is done).  The
//     optimizer's kernels call it once and did without that barrier: it costs them nothing that shows.
//   * The wave total starts from wave 0's sum, where the optimizer's own copy started from 0.0.  The two differ only
//     when every wave's sum is -0.0, and the optimizer's partials are sums of squares: never -0.0.
template <int WAVES, int K, typename T>
__device__ inline void block_sum(T (&acc)[K]) {
  __shared__ T wave_sum[K][WAVES];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    for (int off = 32; off > 0; off >>= 1) acc[k] += __shfl_down(acc[k], off, 64);
    if ((threadIdx.x & 63) == 0) wave_sum[k][threadIdx.x >> 6] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      T total = wave_sum[k][0];
      for (int w = 1; w < WAVES; ++w) total += wave_sum[k][w];
      acc[k] = total;
    }
  }
}

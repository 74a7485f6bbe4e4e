// f64 reductions and the ragged-row length shared by the waveform metric
// kernels (metrics.hip, stoi.hip).  Every sum has one fixed order.
#pragma once

#include "common.h"

namespace hvit {

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Sum of one value per thread of a 256-thread workgroup, in every thread:
// butterfly per wave, then the four wave sums in ascending order.  One call
// per kernel: nothing guards red against a second use.
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
  v = wave_sum_f64(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__device__ __forceinline__ int row_len(const int* lengths, int b, int L) {
  const int len = lengths ? lengths[b] : L;
  return len < 0 ? 0 : (len > L ? L : len);
}

}  // namespace hvit

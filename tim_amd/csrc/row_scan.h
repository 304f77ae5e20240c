// The in-place scan of a row_offsets array, shared by the units that list candidates by count + scan + emit (detect.hip,
// twostream.hip).  Each unit gets its own internal copy of the kernel (anonymous namespace).
#pragma once

#include "common.h"

namespace {

// row_offsets[1 .. R] hold the counts: inclusive scan in place, row_offsets[0] = 0.  One block, 1024 elements per round with
// a carry; the order of the additions is fixed (integers anyway).
__global__ __launch_bounds__(1024) void det_scan_kernel(int* __restrict__ row_offsets, int R) {
  __shared__ int wsum[16];
  __shared__ int carry_s;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (tid == 0) { row_offsets[0] = 0; carry_s = 0; }
  __syncthreads();
  for (int base = 0; base < R; base += 1024) {
    const int i = base + tid;
    int v = i < R ? row_offsets[i + 1] : 0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int u = __shfl_up(v, o, 64);
      if (lane >= o) v += u;
    }
    if (lane == 63) wsum[w] = v;
    __syncthreads();
    int before = carry_s;
#pragma unroll
    for (int k = 0; k < 16; ++k) if (k < w) before += wsum[k];
    v += before;
    if (i < R) row_offsets[i + 1] = v;
    __syncthreads();                       // every thread has read carry_s and wsum
    if (tid == 1023) carry_s = v;
    __syncthreads();
  }
}

}  // namespace

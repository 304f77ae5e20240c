// What the units that list candidates by count + scan + emit share (detect.hip, twostream.hip): the reproducible score,
// the proposal decode, the grid, the in-place scan of a row_offsets array and the bound of an emit.  Each unit gets its own
// internal copy (anonymous namespace) and sets `#pragma clang fp contract(off)` ahead of the include; the arithmetic here
// uses the explicitly rounded intrinsics, so no product is fused into the add that follows it either way.
#pragma once

#include <math.h>

#include "common.h"

namespace {

constexpr int kWavesPerBlock = 4;
constexpr int kMaxBlocks = 2048;   // memory-bound grid: cap the grid and stride over the rows

// the float64 sigmoid rounded once to fp32: reproducible on a CPU, which the device's 1-ulp expf is not
__device__ __forceinline__ float cand_sigmoid(float x) {
  return (float)__ddiv_rn(1.0, __dadd_rn(1.0, exp(-(double)x)));
}

// numpy.round(v, 3) on float64
__device__ __forceinline__ double cand_round3(double v) { return __ddiv_rn(rint(__dmul_rn(v, 1000.0)), 1000.0); }

__device__ __forceinline__ float cand_clamp(float v, float hi) {
  if (v != v) return v;                       // torch.clamp propagates NaN (such a proposal fails the width test)
  return fminf(fmaxf(v, 0.0f), hi);
}

// one end of a proposal in seconds, NOT rounded: fp32 clamp, one fp32 product, fp64 add of the window's start
__device__ __forceinline__ double cand_decode(float reg, float max_time, float window_size, double window_start) {
  return __dadd_rn((double)__fmul_rn(cand_clamp(reg, max_time), window_size), window_start);
}

__device__ __forceinline__ unsigned long long lanes_below(int lane) { return (1ull << lane) - 1ull; }

// one past the last slot row r may write: never past this row's slots nor past the buffers, so a count taken on other
// inputs cannot make an emit write out of bounds, it can only cut the row short
__device__ __forceinline__ long long cand_row_end(const int* __restrict__ row_offsets, int r, long long capacity) {
  return min((long long)row_offsets[r + 1], capacity);
}

// one wavefront per row
int cand_grid(int R) {
  const int blocks = (R + kWavesPerBlock - 1) / kWavesPerBlock;
  return blocks < 1 ? 1 : (blocks > kMaxBlocks ? kMaxBlocks : blocks);
}

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

int cand_scan(int* row_offsets, int R, hipStream_t s) {
  hipLaunchKernelGGL(det_scan_kernel, dim3(1), dim3(1024), 0, s, row_offsets, R);
  TIM_CHECK_LAUNCH();
  return TIMHIP_OK;
}

}  // namespace

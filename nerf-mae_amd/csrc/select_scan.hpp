// Workgroup prefix sum and radix-select pick for workgroups of SEL_T = 1024 lanes, shared by fcos_post.hip (top-k of the scores) and rpn.hip
// (the sampler's cut).  Integer sums only: the results do not depend on the order of the atomics that filled the histogram.
#pragma once
#include "common.hpp"

constexpr int SEL_T = 1024;

// exclusive prefix sum of v over the 1024 lanes of the workgroup (lane order), and the total; wsum: 16 ints of LDS
__device__ __forceinline__ int block_scan_excl(int v, int& total, int* wsum) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(inc, o, 64);
    if (lane >= o) inc += u;
  }
  __syncthreads();                         // wsum of the previous call has been read
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < SEL_T / 64; ++i) { const int s = wsum[i]; base += i < w ? s : 0; tot += s; }
  total = tot;
  return base + inc - v;
}

// the digit holding the r-th largest entry of hist[0 .. 2047] counted from the top bin, and r within that bin -> sh[0], sh[1]
__device__ __forceinline__ void radix_pick(const int* hist, int r, int* wsum, int* sh) {
  const int t = threadIdx.x, a = 2047 - 2 * t, b = a - 1;
  const int ha = hist[a], hb = hist[b];
  int total;
  const int before = block_scan_excl(ha + hb, total, wsum);
  if (before < r && r <= before + ha + hb) {           // exactly one lane, because 1 <= r <= total
    const bool first = r <= before + ha;
    sh[0] = first ? a : b;
    sh[1] = first ? r - before : r - before - ha;
  }
  __syncthreads();
}

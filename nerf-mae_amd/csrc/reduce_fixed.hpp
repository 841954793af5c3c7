// Fixed-order fp32 reductions of the detector losses (fcos.hip, rpn.hip, roi_head.hip) and the row softmax of the RoI stage (roi_head.hip, roi_post.hip).  A
// loss is summed in two launches: every workgroup of 256 lanes leaves K partial sums (block_sum_fixed), then one workgroup adds the partials (final_sum_fixed)
// and its kernel normalises.  No atomics: the order of the additions depends only on the number of workgroups, so two runs give the same bits.
#pragma once
#include "common.hpp"

namespace {

// sums v[0 .. K-1] over the workgroup of 256: a shuffle tree over each wave, then (w0 + w1) + (w2 + w3) over the waves -> out[0 .. K-1] (thread 0)
template <int K>
__device__ __forceinline__ void block_sum_fixed(float (&v)[K], float* __restrict__ out) {
  __shared__ float red[K][4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] += __shfl_down(v[k], o, 64);
  }
  const int t = threadIdx.x;
  if ((t & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) red[k][t >> 6] = v[k];
  }
  __syncthreads();
  if (t == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) out[k] = (red[k][0] + red[k][1]) + (red[k][2] + red[k][3]);
  }
}

// one workgroup of 256: the sums of partials[nblocks][K] -> total (every thread): lane t adds rows t, t + 256, .. in ascending order, then a tree over the
// lanes in LDS from 128 down to 1
template <int K>
__device__ __forceinline__ void final_sum_fixed(const float* __restrict__ partials, int nblocks, float (&total)[K]) {
  __shared__ float s[K][256];
  const int t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < K; ++k) total[k] = 0.f;
  for (int i = t; i < nblocks; i += 256) {
#pragma unroll
    for (int k = 0; k < K; ++k) total[k] += partials[K * i + k];
  }
#pragma unroll
  for (int k = 0; k < K; ++k) s[k][t] = total[k];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) {
#pragma unroll
      for (int k = 0; k < K; ++k) s[k][t] += s[k][t + o];
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < K; ++k) total[k] = s[k][0];
}

// softmax of a row of n logits in two passes: mx = the largest, sum = the sum of expf(x[c] - mx); the probability of class c is expf(x[c] - mx) / sum
__device__ __forceinline__ void row_softmax(const float* __restrict__ x, int n, float& mx, float& sum) {
  mx = x[0];
  for (int c = 1; c < n; ++c) mx = fmaxf(mx, x[c]);
  sum = 0.f;
  for (int c = 0; c < n; ++c) sum += expf(x[c] - mx);
}

}  // namespace

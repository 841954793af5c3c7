// Exact top-k of 32-bit keys by one workgroup of SEL_T = 1024 lanes: workgroup prefix sum, three-pass radix select of the k-th largest key, and the ordered
// compaction that applies the cut.  Used by fcos_post_select (fcos_post.hip: stored keys), rpn_post_select (rpn_post.hip: keys re-formed from the logits) and
// rpn_sample (rpn.hip: one select per class, flags in place of slots).  Integer sums only: the results do not depend on the order of the atomics that filled
// a histogram.  The tie rule lives here: of the keys equal to the k-th largest, the first need_eq in element order are taken.
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
__device__ __forceinline__ void hist_clear(int* hist) {
  hist[threadIdx.x] = 0; hist[threadIdx.x + SEL_T] = 0;
  __syncthreads();
}

// The k-th largest key K of the taking-part elements of 0 .. n-1 (1 <= k <= their number) and how many of the keys == K belong to the k largest; digits of
// 11 + 11 + 10 bits, each histogram scanned from the top.  key_at(q, key) gives element q's key, or false when q does not take part.  hist: 2048 ints of LDS,
// wsum: 16, sh: 2.  radix_select_rest expects the histogram of the first digit (key >> 21) in hist, complete behind a barrier: callers that form their
// keys in a pass of their own fill it there; radix_select fills it itself.
struct RadixCut { unsigned K; int need_eq; };
template <typename KeyAt>
__device__ __forceinline__ RadixCut radix_select_rest(int* hist, int* wsum, int* sh, int k, int n, KeyAt key_at) {
  const int t = threadIdx.x;
  unsigned key;
  radix_pick(hist, k, wsum, sh);
  const unsigned d0 = (unsigned)sh[0];
  int r = sh[1];
  __syncthreads();
  hist_clear(hist);
  for (int q = t; q < n; q += SEL_T)
    if (key_at(q, key) && (key >> 21) == d0) atomicAdd(&hist[(key >> 10) & 2047u], 1);
  __syncthreads();
  radix_pick(hist, r, wsum, sh);
  const unsigned d01 = (d0 << 11) | (unsigned)sh[0];
  r = sh[1];
  __syncthreads();
  hist_clear(hist);
  for (int q = t; q < n; q += SEL_T)
    if (key_at(q, key) && (key >> 10) == d01) atomicAdd(&hist[1024 + (key & 1023u)], 1);      // the upper half of the bins, so that radix_pick's scan order holds
  __syncthreads();
  radix_pick(hist, r, wsum, sh);
  const RadixCut c{(d01 << 10) | (unsigned)(sh[0] - 1024), sh[1]};
  __syncthreads();
  return c;
}
template <typename KeyAt>
__device__ __forceinline__ RadixCut radix_select(int* hist, int* wsum, int* sh, int k, int n, KeyAt key_at) {
  unsigned key;
  hist_clear(hist);
  for (int q = threadIdx.x; q < n; q += SEL_T)
    if (key_at(q, key)) atomicAdd(&hist[key >> 21], 1);
  __syncthreads();
  return radix_select_rest(hist, wsum, sh, k, n, key_at);
}

// The tie rule on one chunk of 1024 elements in ascending order: this lane's element is taken if it already is (sel) or its key equals K (eq) and fewer
// than need_eq such keys come before it; run_eq counts them over the chunks.
__device__ __forceinline__ bool tie_take(bool sel, bool eq, int need_eq, int& run_eq, int* wsum) {
  int tot;
  const int rank = run_eq + block_scan_excl(eq ? 1 : 0, tot, wsum);
  run_eq += tot;
  return sel || (eq && rank < need_eq);
}
// One chunk of the ordered compaction: gt / eq: this lane's key is above / at the cut; tie (uniform): a tie rule is in force, else eq is not looked at and
// its scan is skipped.  Returns whether the element is taken, and in pos its position among all taken so far (run_sel counts them).
__device__ __forceinline__ bool compact_step(bool gt, bool eq, bool tie, int need_eq, int& run_eq, int& run_sel, int* wsum, int& pos) {
  const bool sel = tie ? tie_take(gt, eq, need_eq, run_eq, wsum) : gt;
  int tot;
  pos = run_sel + block_scan_excl(sel ? 1 : 0, tot, wsum);
  run_sel += tot;
  return sel;
}

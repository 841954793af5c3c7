// Bit-matrix NMS over boxes in descending score, shared by rotated_iou.hip (obb_nms_*), fcos_post.hip and roi_post.hip (one matrix per scene) and rpn_post.hip
// (one per scene and level).  Word (i, j) of a matrix of row_words 64-bit words per row has bit k set iff iou(i, 64 j + k) > threshold and 64 j + k > i.  Only
// the upper triangle of 64 x 64 blocks is launched: one workgroup of 256 lanes per block, one wave per word (lane k takes column 64 j + k, the ballot is the
// word); words strictly below the diagonal block are zero by definition, never read and never written.  A mask workgroup finds its block (tri_block), stages
// the block's row and column boxes in LDS and forms its words (nms_mask_tile); the three post-processing files, whose boxes are reached through the caller's
// sort order, stage with nms_stage_sorted, and rotated_iou.hip, which has categories and no order, stages on its own.  The walk (nms_greedy_walk) is one
// workgroup of 256 lanes: per block of 64 rows it resolves the block's own dependencies from the 64 diagonal words, then ORs the rows of the kept boxes into
// the removed-set in LDS.
#pragma once
#include "obb_geom.hpp"             // BoxTile, stage_box, tile_iou

namespace {

// workgroup b of the upper triangle of nw x nw blocks, row block by row block: block row `by` has the words j = by .. nw-1
__device__ __forceinline__ void tri_block(int b, int nw, int& by, int& j) {
  by = 0; j = b;
  while (j >= nw - by) { j -= nw - by; ++by; }       // uniform, at most nw <= 256 steps
  j += by;
}

// Workgroup b of the upper triangle of nw x nw blocks over nb boxes: its position -> (r0, c0 = 64 j, j), and its row and column boxes -> rows, cols, ready
// behind a barrier.  Sorted position i is row clamp(order[i], lo, hi) of boxes, rows of `stride` floats with the box at float `col`; positions past nb are
// zero boxes.  Returns false, uniformly and before any staging, when the block's columns start beyond nb (r0 <= c0): it has no word to write.
struct NmsBlock { int r0, c0, j; };
template <bool AABB>
__device__ __forceinline__ bool nms_stage_sorted(int b, int nw, const float* __restrict__ boxes, int stride, int col, const long* __restrict__ order, long lo, long hi, int nb,
                                                 BoxTile* rows, BoxTile* cols, NmsBlock& at) {
  int by;
  tri_block(b, nw, by, at.j);
  at.r0 = by * 64; at.c0 = at.j * 64;
  if (at.c0 >= nb) return false;
  const int t = threadIdx.x;
  if (t < 128) {
    const int i = (t < 64 ? at.c0 : at.r0 - 64) + t;
    BoxTile& dst = t < 64 ? cols[t] : rows[t - 64];
    if (i < nb) stage_box<AABB>(boxes + col, min(max(order[i], lo), hi), hi + 1, dst, stride);
    else zero_box(dst);
  }
  __syncthreads();
  return true;
}

// the words (r0 .. r0+63, j) of a matrix of nb boxes at m0, from the staged row and column boxes (c0 = 64 j); rcat / cat: the staged categories of the rows and
// the categories of all boxes, a pair matching only within a category, or both null
template <bool AABB>
__device__ __forceinline__ void nms_mask_tile(const BoxTile* rows, const BoxTile* cols, int r0, int c0, int j, int nb, float thr, unsigned long long* __restrict__ m0, int row_words,
                                              const int* rcat, const int* __restrict__ cat) {
  const int t = threadIdx.x, k = t & 63, col = c0 + k;
  const BoxTile bc = cols[k];
  const int ccat = (cat && col < nb) ? cat[col] : 0;
#pragma unroll 1
  for (int r = t >> 6; r < 64; r += 4) {
    const int row = r0 + r;
    if (row >= nb) break;                              // uniform over the wave
    bool hit = false;
    if (col > row && col < nb && (!rcat || ccat == rcat[r])) hit = tile_iou<AABB>(rows[r], bc) > thr;
    const unsigned long long word = __ballot(hit);
    if (k == 0) m0[(long)row * row_words + j] = word;
  }
}

// the greedy walk over the N boxes of the matrix at m0: the kept positions, ascending, -> kp[0 .. cnt-1]; returns cnt, the same in every thread.
// removed: 256 words of LDS (N <= 16384), diag: 64
__device__ __forceinline__ int nms_greedy_walk(const unsigned long long* __restrict__ m0, int row_words, int N, int* kp, unsigned long long* removed, unsigned long long* diag) {
  const int t = threadIdx.x, nw = (N + 63) >> 6;
  __syncthreads();                         // removed[] of a previous walk has been read
  removed[t] = 0ull;
  int cnt = 0;
  for (int c = 0; c < nw; ++c) {
    __syncthreads();                       // removed[] of the previous block is complete; diag[] is free
    if (t < 64) diag[t] = c * 64 + t < N ? m0[(long)(c * 64 + t) * row_words + c] : 0ull;
    __syncthreads();
    unsigned long long r = removed[c];
    const int left = N - c * 64;
    if (left < 64) r |= ~0ull << left;     // positions past N count as removed
    for (int k = 0; k < 64; ++k)           // row k's word only has bits above k, so bit k of r is final when it is read
      if (!((r >> k) & 1ull)) r |= diag[k];
    const unsigned long long kept = ~r;
    if (t < 64 && ((kept >> t) & 1ull)) kp[cnt + __popcll(kept & ((1ull << t) - 1ull))] = c * 64 + t;
    cnt += __popcll(kept);
    const int nrem = nw - c - 1;           // words after the diagonal one
    for (int q = t; q < 64 * nrem; q += 256) {
      const int k = q / nrem, w = c + 1 + q % nrem;
      if ((kept >> k) & 1ull) {
        const unsigned long long m = m0[(long)(c * 64 + k) * row_words + w];
        if (m) atomicOr(&removed[w], m);
      }
    }
  }
  return cnt;
}

}  // namespace

// Detection evaluation of the reference's nerf_rpn/eval.py: evaluate_box_proposals_recall (eval.py:14-81) and evaluate_box_proposals_ap (eval.py:319-395), as gfx950
// kernels over the dense results of the two detectors (boxes [N][cap] rows in descending score, counts [N]) and padded ground truth (gt [N][Gmax], gt_counts [N]):
//   det_eval_iou     the IoU matrix of every scene, stored ground-truth-major, iouT[n][g][row], and per detection (max IoU, arg-max gt);
//   det_eval_match   the greedy matching of eval.py:39-56 for every (scene, limit) -> gt_overlaps [N][L][Gmax], counted [N][L];
//   det_eval_claims  the true-positive test of eval.py:355-366 for every scene and T thresholds, without the walk -> one byte-mask per detection;
//   det_eval_pr      eval.py:368-387 over the globally sorted true-positive bits: cumulative counts, recalls, precisions, the VOC area.
// fp32 geometry (stage_box / tile_iou of obb_geom.hpp, 6 or 7 columns), integer and fp64 bookkeeping.  No float atomics; the only atomics are integer minima in
// LDS, whose result does not depend on their order: two runs are bit-identical.  Nothing reads a count back to the host.  Every kernel stays inside its own
// arrays for any input: counts are clamped to [0, cap], gt_counts to [0, Gmax], an arg-max outside [0, Gmax) is read as "none".
//
// Box rows.  A detection row has row_stride floats with the box in columns col_offset .. col_offset + ncols - 1, so the FCOS rows (level, box) are read in place.
//
// IoU.  A workgroup of 256 lanes owns 256 detections of one scene (one per lane, in registers) and loops over the scene's ground truth in tiles of 64 staged in
// LDS.  An IoU that is not > 0 (NaN from a degenerate box included) is stored as +0, so every stored value is an ordered, non-negative float.  The row best
// takes the lowest ground-truth index on ties (torch's first occurrence); it is (0, -1) without ground truth and for rows past counts[n].
//
// Greedy match, per (scene n, limit l): P = min(counts[n], limit_l), G = gt_counts[n].  P == 0 or G == 0: the scene is skipped as in eval.py:28, counted = 0 and all
// Gmax slots are -1.  Else counted = G, and min(P, G) times the largest remaining IoU is recorded and its row and column are retired; slots up to G are 0
// (eval.py:37), slots past G are -1.  The choice among equal maxima is torch's on the CPU: max(dim=0) takes the lowest row per column, the max over the columns
// the lowest column, so the key is (IoU descending, gt ascending, row ascending).  Per column the best remaining (IoU, row) lives in LDS with a bitmap of the
// used rows; a step reduces the columns, retires, and rescans only the columns whose best row was the retired one (one wave per such column, contiguous reads
// of iouT).  The matrix itself stays in global memory.
//
// Claims, per scene: K = min(counts[n], top_k) detections are kept (top_k <= 0: all).  In the global score order detection i is a true positive at threshold t
// iff m_i > t and no earlier detection of its scene with the same arg-max a_i also has m > t (gt_used is per scene, and a detection that fails the threshold
// claims nothing).  Hence tp_i = m_i > t and i == min{ j < K : a_j == a_i, m_j > t }: an integer atomicMin per (threshold, gt) in LDS, then one compare.  A
// detection without ground truth (a = -1) is a false positive; the reference raises IndexError there.
//
// Precision / recall, one workgroup per threshold over bits [M] in the global order, of which the first n_det[0] count (kept detections first): forward chunks
// of 1024 with a carry give tp and fp = position + 1 - tp exactly (int32); recalls = float(tp) / float(num_gt), precisions = float(tp) / float(tp + fp) as torch
// divides integers.  Backward chunks give the running maximum of the precisions from the right (the envelope of eval.py:379-380) and the area: recall changes
// exactly at the true positives, by 1 / num_gt, so ap = (sum over the true positives, right to left, of the envelope) / num_gt, in fp64 with a fixed order
// (lanes by a shuffle tree, waves in order, chunks in order).  n_det == 0 gives ap = 0; num_gt == 0 with detections gives NaN recalls and ap, as the reference.
#include "common.hpp"
#include "kernels.hpp"
#include "obb_geom.hpp"
#include "select_scan.hpp"

namespace {

constexpr int DE_ROWS = 256, DE_GT_TILE = 64, DE_MATCH_T = 256, DE_PR_T = SEL_T;

struct DeLimits { int n, v[NMH_DET_EVAL_MAX_LIMITS]; };
struct DeThresh { int n; float v[NMH_DET_EVAL_MAX_THRESH]; };

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

template <bool AABB>
__global__ __launch_bounds__(DE_ROWS) void det_eval_iou_kernel(int cap, int row_stride, int col_offset, const float* __restrict__ boxes, const int* __restrict__ counts, int Gmax,
                                                               const float* __restrict__ gt, const int* __restrict__ gt_counts, float* __restrict__ iouT,
                                                               float* __restrict__ best_iou, int* __restrict__ best_gt) {
  constexpr int C = AABB ? 6 : 7;
  __shared__ BoxTile cols[DE_GT_TILE];
  const int t = threadIdx.x, n = blockIdx.y, row = blockIdx.x * DE_ROWS + t;
  const int P = clampi(counts[n], 0, cap), G = clampi(gt_counts[n], 0, Gmax);
  const bool live = row < P;
  BoxTile me;
  stage_box<AABB>(boxes + (long)n * cap * row_stride + col_offset, live ? row : 0, live ? 1L + row : 0L, me, row_stride);
  float best = -1.f;
  int arg = -1;
  for (int g0 = 0; g0 < G; g0 += DE_GT_TILE) {                 // uniform
    __syncthreads();                                           // the previous tile has been read
    if (t < DE_GT_TILE) stage_box<AABB>(gt + (long)n * Gmax * C, g0 + t, G, cols[t]);
    __syncthreads();
    const int ng = min(DE_GT_TILE, G - g0);
    if (live) {
#pragma unroll 1
      for (int k = 0; k < ng; ++k) {
        float v = tile_iou<AABB>(me, cols[k]);
        v = v > 0.f ? v : 0.f;
        iouT[((long)n * Gmax + g0 + k) * cap + row] = v;
        if (v > best) { best = v; arg = g0 + k; }
      }
    }
  }
  if (row < cap) {
    best_iou[(long)n * cap + row] = arg >= 0 ? best : 0.f;
    best_gt[(long)n * cap + row] = arg;
  }
}

// ---- 64-bit (value, index) keys: the larger key wins; 0 is "nothing" ---------------------------------------------------------------------------------
// hi = bits of a non-negative float + 1, lo = ~index: the larger value first, then the LOWER index
__device__ __forceinline__ unsigned long long de_key(float v, int idx) { return ((unsigned long long)(__float_as_uint(v) + 1u) << 32) | (unsigned)~idx; }
__device__ __forceinline__ int de_key_index(unsigned long long k) { return (int)~(unsigned)(k & 0xffffffffull); }
__device__ __forceinline__ float de_key_value(unsigned long long k) { return __uint_as_float((unsigned)(k >> 32) - 1u); }
__device__ __forceinline__ unsigned long long wave_max_key(unsigned long long k) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned hi = __shfl_xor((unsigned)(k >> 32), o, 64), lo = __shfl_xor((unsigned)(k & 0xffffffffull), o, 64);
    const unsigned long long other = ((unsigned long long)hi << 32) | lo;
    k = other > k ? other : k;
  }
  return k;
}

// best remaining (IoU, row) of column `col` (its P contiguous floats), by one wave; the same in every lane
__device__ __forceinline__ unsigned long long de_scan_column(const float* __restrict__ col, int P, const unsigned* used) {
  const int lane = threadIdx.x & 63;
  unsigned long long k = 0ull;
  for (int r = lane; r < P; r += 64) {
    if ((used[r >> 5] >> (r & 31)) & 1u) continue;
    const float v = col[r];
    const unsigned long long c = de_key(v > 0.f ? v : 0.f, r);
    k = c > k ? c : k;
  }
  return wave_max_key(k);
}

__global__ __launch_bounds__(DE_MATCH_T) void det_eval_match_kernel(int cap, int Gmax, const int* __restrict__ counts, const int* __restrict__ gt_counts, const float* __restrict__ iouT,
                                                                    DeLimits L, float* __restrict__ gt_overlaps, int* __restrict__ counted) {
  __shared__ unsigned long long colkey[NMH_DET_EVAL_MAX_GT];    // best remaining (IoU, row) of the column; 0: the column is retired
  __shared__ unsigned used[NMH_OBB_NMS_MAX / 32];
  __shared__ unsigned long long wred[DE_MATCH_T / 64];
  const int t = threadIdx.x, w = t >> 6, lane = t & 63, n = blockIdx.y, l = blockIdx.x;
  const int G = clampi(gt_counts[n], 0, Gmax);
  int P = clampi(counts[n], 0, cap);
  if (L.v[l] >= 0) P = min(P, L.v[l]);                          // a negative limit: no cut
  float* __restrict__ out = gt_overlaps + ((long)n * L.n + l) * Gmax;
  const bool skip = P == 0 || G == 0;                           // uniform
  if (t == 0) counted[n * L.n + l] = skip ? 0 : G;
  const int steps = skip ? 0 : min(P, G);
  for (int j = steps + t; j < Gmax; j += DE_MATCH_T) out[j] = (skip || j >= G) ? -1.f : 0.f;
  if (skip) return;
  const float* __restrict__ mat = iouT + (long)n * Gmax * cap;
  for (int i = t; i < NMH_OBB_NMS_MAX / 32; i += DE_MATCH_T) used[i] = 0u;
  __syncthreads();
  for (int g = w; g < G; g += DE_MATCH_T / 64) {                // uniform per wave
    const unsigned long long k = de_scan_column(mat + (long)g * cap, P, used);
    if (lane == 0) colkey[g] = k;
  }
  for (int j = 0; j < steps; ++j) {
    __syncthreads();                                            // colkey is complete
    unsigned long long k = 0ull;                                // (IoU, gt) of the best column: the larger IoU, then the lower gt
    for (int g = t; g < G; g += DE_MATCH_T) {
      const unsigned long long ck = colkey[g];
      if (ck) { const unsigned long long c = (ck & 0xffffffff00000000ull) | (unsigned)~g; k = c > k ? c : k; }
    }
    k = wave_max_key(k);
    if (lane == 0) wred[w] = k;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < DE_MATCH_T / 64; ++i) k = wred[i] > k ? wred[i] : k;
    // min(P, G) steps leave a live row and a live column at every step, so k != 0; the clamps keep any input in bounds
    const int gs = clampi(de_key_index(k), 0, G - 1);
    const int rs = clampi(de_key_index(colkey[gs]), 0, P - 1);
    __syncthreads();                                            // everyone has read colkey[gs] and wred
    if (t == 0) {
      out[j] = k ? de_key_value(k) : 0.f;
      used[rs >> 5] |= 1u << (rs & 31);
      colkey[gs] = 0ull;
    }
    __syncthreads();
    if (j + 1 == steps) break;
    for (int g = w; g < G; g += DE_MATCH_T / 64) {              // uniform per wave
      const unsigned long long ck = colkey[g];
      if (ck == 0ull || de_key_index(ck) != rs) continue;
      const unsigned long long k2 = de_scan_column(mat + (long)g * cap, P, used);
      if (lane == 0) colkey[g] = k2;
    }
  }
}

__global__ __launch_bounds__(256) void det_eval_claims_kernel(int cap, int Gmax, const int* __restrict__ counts, const float* __restrict__ best_iou, const int* __restrict__ best_gt,
                                                              DeThresh T, int top_k, unsigned char* __restrict__ tp_mask, unsigned char* __restrict__ kept) {
  __shared__ int first[NMH_DET_EVAL_MAX_THRESH][NMH_DET_EVAL_MAX_GT];     // the lowest rank that passes the threshold, per gt
  const int t = threadIdx.x, n = blockIdx.x;
  int K = clampi(counts[n], 0, cap);
  if (top_k > 0) K = min(K, top_k);
  const int G = min(Gmax, NMH_DET_EVAL_MAX_GT);
  for (int i = t; i < T.n * NMH_DET_EVAL_MAX_GT; i += 256) (&first[0][0])[i] = 0x7fffffff;
  __syncthreads();
  const long sb = (long)n * cap;
  for (int i = t; i < K; i += 256) {
    const int a = best_gt[sb + i];
    const float m = best_iou[sb + i];
    if (a < 0 || a >= G) continue;
    for (int q = 0; q < T.n; ++q)
      if (m > T.v[q]) atomicMin(&first[q][a], i);
  }
  __syncthreads();
  for (int i = t; i < cap; i += 256) {
    unsigned bits = 0u;
    if (i < K) {
      const int a = best_gt[sb + i];
      const float m = best_iou[sb + i];
      if (a >= 0 && a < G)
        for (int q = 0; q < T.n; ++q) bits |= (m > T.v[q] && first[q][a] == i) ? 1u << q : 0u;
    }
    tp_mask[sb + i] = (unsigned char)bits;
    kept[sb + i] = i < K ? 1 : 0;
  }
}

__global__ __launch_bounds__(DE_PR_T) void det_eval_pr_kernel(long M, const unsigned char* __restrict__ bits, const int* __restrict__ n_det, const int* __restrict__ num_gt,
                                                              int* __restrict__ tp_cum, int* __restrict__ fp_cum, float* __restrict__ recalls, float* __restrict__ precisions,
                                                              double* __restrict__ ap) {
  __shared__ int wsum[DE_PR_T / 64];
  __shared__ double wmax[DE_PR_T / 64], wadd[DE_PR_T / 64];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, q = blockIdx.x;
  const long n = min(max((long)n_det[0], 0L), M);
  const float fgt = (float)num_gt[0];
  int* __restrict__ tpc = tp_cum + (long)q * M;
  int* __restrict__ fpc = fp_cum + (long)q * M;
  float* __restrict__ rec = recalls + (long)q * M;
  float* __restrict__ pre = precisions + (long)q * M;
  const long chunks = (n + DE_PR_T - 1) / DE_PR_T;
  int carry = 0;
  for (long c = 0; c < chunks; ++c) {                           // uniform
    const long i = c * DE_PR_T + t;
    const int b = i < n ? (bits[i] >> q) & 1 : 0;
    int total;
    const int tp = carry + block_scan_excl(b, total, wsum) + b;
    carry += total;
    if (i < n) {
      const int fp = (int)(i + 1) - tp;
      tpc[i] = tp; fpc[i] = fp;
      rec[i] = (float)tp / fgt;
      pre[i] = (float)tp / (float)(tp + fp);
    }
  }
  for (long i = n + t; i < M; i += DE_PR_T) { tpc[i] = 0; fpc[i] = 0; rec[i] = 0.f; pre[i] = 0.f; }
  // right to left: the envelope and the sum over the true positives
  double right = 0.0, sum = 0.0;                                // the sentinel precision behind the last detection is 0
  for (long c = chunks - 1; c >= 0; --c) {                      // uniform
    const long i = c * DE_PR_T + t;
    int tp = 0, b = 0;
    double p = 0.0;
    if (i < n) { tp = tpc[i]; b = (bits[i] >> q) & 1; p = (double)tp / (double)(i + 1); }      // this lane's own writes of the forward pass
    double env = p;                                             // maximum over this lane and the lanes after it in the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const double u = __shfl_down(env, o, 64);
      if (lane + o < 64) env = fmax(env, u);
    }
    __syncthreads();                                            // wmax, wadd of the previous chunk have been read
    if (lane == 0) wmax[w] = env;
    __syncthreads();
    double after = right;
    for (int k = DE_PR_T / 64 - 1; k > w; --k) after = fmax(after, wmax[k]);
    env = fmax(env, after);
    double term = b ? env : 0.0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) term += __shfl_xor(term, o, 64);
    if (lane == 0) wadd[w] = term;
    __syncthreads();
    for (int k = DE_PR_T / 64 - 1; k >= 0; --k) { sum += wadd[k]; right = fmax(right, wmax[k]); }
  }
  if (t == 0) ap[q] = n > 0 ? sum / (double)num_gt[0] : 0.0;
}

}  // namespace

int k_det_eval_iou(int ncols, int N, int cap, int row_stride, int col_offset, const float* boxes, const int* counts, int Gmax, const float* gt, const int* gt_counts, float* iouT,
                   float* best_iou, int* best_gt, hipStream_t st) {
  const dim3 grid((unsigned)((cap + DE_ROWS - 1) / DE_ROWS), (unsigned)N);
  if (ncols == 6) hipLaunchKernelGGL(det_eval_iou_kernel<true>, grid, dim3(DE_ROWS), 0, st, cap, row_stride, col_offset, boxes, counts, Gmax, gt, gt_counts, iouT, best_iou, best_gt);
  else hipLaunchKernelGGL(det_eval_iou_kernel<false>, grid, dim3(DE_ROWS), 0, st, cap, row_stride, col_offset, boxes, counts, Gmax, gt, gt_counts, iouT, best_iou, best_gt);
  NMH_CHECK_LAUNCH();
  return 0;
}

int k_det_eval_match(int N, int cap, int Gmax, const int* counts, const int* gt_counts, const float* iouT, int nlimits, const int* limits, float* gt_overlaps, int* counted,
                     hipStream_t st) {
  DeLimits L;
  L.n = nlimits;
  for (int i = 0; i < NMH_DET_EVAL_MAX_LIMITS; ++i) L.v[i] = i < nlimits ? limits[i] : 0;
  hipLaunchKernelGGL(det_eval_match_kernel, dim3((unsigned)nlimits, (unsigned)N), dim3(DE_MATCH_T), 0, st, cap, Gmax, counts, gt_counts, iouT, L, gt_overlaps, counted);
  NMH_CHECK_LAUNCH();
  return 0;
}

int k_det_eval_claims(int N, int cap, int Gmax, const int* counts, const float* best_iou, const int* best_gt, int nthresh, const float* thresholds, int top_k, unsigned char* tp_mask,
                      unsigned char* kept, hipStream_t st) {
  DeThresh T;
  T.n = nthresh;
  for (int i = 0; i < NMH_DET_EVAL_MAX_THRESH; ++i) T.v[i] = i < nthresh ? thresholds[i] : 0.f;
  hipLaunchKernelGGL(det_eval_claims_kernel, dim3((unsigned)N), dim3(256), 0, st, cap, Gmax, counts, best_iou, best_gt, T, top_k, tp_mask, kept);
  NMH_CHECK_LAUNCH();
  return 0;
}

int k_det_eval_pr(long M, const unsigned char* bits, const int* n_det, const int* num_gt, int nthresh, int* tp_cum, int* fp_cum, float* recalls, float* precisions, double* ap,
                  hipStream_t st) {
  hipLaunchKernelGGL(det_eval_pr_kernel, dim3((unsigned)nthresh), dim3(DE_PR_T), 0, st, M, bits, n_det, num_gt, tp_cum, fp_cum, recalls, precisions, ap);
  NMH_CHECK_LAUNCH();
  return 0;
}

// Post-processing of the second (RoI) stage of the reference's two-stage detector: Trainer.filter_proposals (nerf_rpn/run_rpn_detect.py:403-439) over
// clip_boxes_to_mesh / remove_small_boxes / nms (model/utils.py:215-367), with the softmax (detector.py:606) and the decode (detector.py:609-611, roi_decode.hpp)
// of Classification_Model's evaluation forward in front of it, as gfx950 kernels:
//   roi_post_select     one lane per (scene, row): softmax, decode, clip, size filter, score threshold -> candidate box, score, sort key;
//   roi_post_nms_mask   the suppression bit matrices of all scenes in one launch (nms_bits.hpp);
//   roi_post_nms_scan   the greedy walk of all scenes in one launch, with the write of the results in its epilogue.
// fp32 throughout; nothing goes to scratch; no float atomics; every kernel writes all of its outputs for any input; the host never waits.
//
// Layout.  N scenes of R rows: pred_scores [N R][K] logits, pred_bbox_deltas [N R][B], rois [N R][1 + B] (level, box), B = 6 (x0,y0,z0,x1,y1,z1) or 7
// (x,y,z,w,h,d,theta); counts [N] (clamped to 0 .. R here): scene n's rows 0 .. counts[n]-1 exist; mesh_sizes [N][3] int32.
//
// Semantics, per existing row:
//   p = softmax(logits) by a max pass and a sum pass; the row's score is s = p[1];
//   box: is_reg: roi_decode_box(deltas, RoI's box) (dw, dh, dd clipped at log 2000, the angle wrapped), else the RoI's own box;
//   6 columns: every coordinate clamped to [0, mesh_size[axis]]; 7 columns: not clipped, and the row is dropped unless its centre lies in [0, mesh_size] on
//   all three axes (the ALIGNED reading: the reference's clip_boxes_to_mesh shortens only `boxes`, so its later indexing pairs boxes with the wrong scores
//   whenever a centre is outside; rpn_post.hip takes the same reading);
//   dropped if a side < min_size (6 columns: x1 - x0 ..; 7: w, h, d);
//   threshold_mode 0 (ANY, the reference's reading): passes iff max_c p[c] >= score_thresh; 1 (OBJECT): iff p[1] >= score_thresh.
//   The reference thresholds the 2-D tensor of probabilities: torch.where(scores >= thr)[0] on [rows, K] returns a row once per passing column, so a row
//   survives iff ANY class probability passes, the background's included (with K = 2 and thr = 0.5 every row survives), and a row with two passing columns
//   appears twice.  The second copy has IoU 1 with the first and shares its fate in the NMS, so for nms_thresh < 1 the SET of results is that of ANY without
//   duplicates.  OBJECT is the reading the code evidently intended.
//   A row whose score is NaN is dropped, and so is a row whose box, before the clamp, has a coordinate that is NaN or infinite (DEFINED here: the reference's
//   clamp would hand a NaN on to its NMS; fminf / fmaxf would turn it into 0, a made-up box).
// Sort key (int32): 0 for a dropped row and for a row past counts[n]; else the bits of s plus 1 (s >= 0, so integer order is score order and every surviving
// key is > 0).  The caller sorts the keys of each scene: stable, descending.  Surviving rows therefore come first, in decreasing score, equal scores in
// ascending row index (the reference's argsort leaves ties open; DEFINED here).  The surviving count of a scene is the number of sorted keys > 0, found by
// binary search in device memory by the NMS kernels.
// NMS, per scene over the sorted survivors: a box is suppressed iff its IoU with a kept box is > nms_thresh (pair geometry: obb_geom.hpp, 6- or 7-column
// form); bit matrix and walk of nms_bits.hpp, rows of ceil(R / 64) words; the grid is the upper triangle for R, and a workgroup whose columns start beyond
// the scene's surviving count exits at once.  R <= 16384 (256 words of removed-set).  No post-NMS cut (the reference has none here).
// Results: boxes [N][R][B], scores [N][R], index [N][R] (the source row within the scene), counts_out [N]; rows 0 .. counts_out[n]-1 in descending score,
// rows past them zero with index -1.
#include "common.hpp"
#include "kernels.hpp"
#include "nms_bits.hpp"
#include "reduce_fixed.hpp"
#include "roi_decode.hpp"

namespace {

template <bool ORIENTED>
__global__ __launch_bounds__(256) void roi_post_select_kernel(int N, int R, int K, const float* __restrict__ logits, const float* __restrict__ deltas, const float* __restrict__ rois,
                                                              const int* __restrict__ counts, const int* __restrict__ mesh, float score_thresh, float min_size, int is_reg, int mode,
                                                              float* __restrict__ cand_boxes, float* __restrict__ cand_scores, int* __restrict__ keys) {
  constexpr int B = ORIENTED ? 7 : 6;
  const long m = (long)blockIdx.x * 256 + threadIdx.x;
  if (m >= (long)N * R) return;
  const int scene = (int)(m / R), r = (int)(m - (long)scene * R);
  const bool exists = r < min(max(counts[scene], 0), R);
  float o[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float s = 0.f;
  bool ok = false;
  if (exists) {
    const float* __restrict__ x = logits + m * K;
    float mx, sum;
    row_softmax(x, K, mx, sum);
    s = expf(x[1] - mx) / sum;
    const float pmax = 1.f / sum;                      // exp(mx - mx) / sum
    const float* __restrict__ e = rois + m * (1 + B) + 1;
    if (is_reg) roi_decode_box<ORIENTED>(deltas + m * B, e, o);
    else {
#pragma unroll
      for (int c = 0; c < B; ++c) o[c] = e[c];
    }
    const float sx = (float)mesh[scene * 3], sy = (float)mesh[scene * 3 + 1], sz = (float)mesh[scene * 3 + 2];
    bool finite = true;                                // before the clamp, which would turn a NaN coordinate into 0
#pragma unroll
    for (int c = 0; c < B; ++c) finite = finite && fabsf(o[c]) <= 3.402823466e38f;
    if (ORIENTED) {
      ok = o[0] >= 0.f && o[0] <= sx && o[1] >= 0.f && o[1] <= sy && o[2] >= 0.f && o[2] <= sz && o[3] >= min_size && o[4] >= min_size && o[5] >= min_size;
    } else {
      o[0] = fminf(fmaxf(o[0], 0.f), sx); o[1] = fminf(fmaxf(o[1], 0.f), sy); o[2] = fminf(fmaxf(o[2], 0.f), sz);
      o[3] = fminf(fmaxf(o[3], 0.f), sx); o[4] = fminf(fmaxf(o[4], 0.f), sy); o[5] = fminf(fmaxf(o[5], 0.f), sz);
      ok = o[3] - o[0] >= min_size && o[4] - o[1] >= min_size && o[5] - o[2] >= min_size;
    }
    ok = ok && finite && s == s && (mode == 0 ? pmax : s) >= score_thresh;
  }
#pragma unroll
  for (int c = 0; c < B; ++c) cand_boxes[m * B + c] = o[c];
  cand_scores[m] = s;
  keys[m] = ok ? (int)(__float_as_uint(s) + 1u) : 0;
}

// the number of keys > 0 in front of the scene's descending keys
__device__ __forceinline__ int surviving(const int* __restrict__ sorted_keys, int R) {
  int lo = 0, hi = R;                                  // the first position whose key is not > 0
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (sorted_keys[mid] > 0) lo = mid + 1; else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ long source_row(const long* __restrict__ order, long sb, int R, int i) { return min(max(order[sb + i], 0L), (long)R - 1); }

template <bool AABB>
__global__ __launch_bounds__(256) void roi_post_nms_mask_kernel(int R, const float* __restrict__ cand_boxes, const int* __restrict__ sorted_keys, const long* __restrict__ order, float thr,
                                                                unsigned long long* __restrict__ mask) {
  constexpr int B = AABB ? 6 : 7;
  __shared__ BoxTile rows[64], cols[64];
  const int scene = blockIdx.y, rw = (R + 63) >> 6;
  const long sb = (long)scene * R;
  const int nb = surviving(sorted_keys + sb, R);
  NmsBlock at;
  if (!nms_stage_sorted<AABB>(blockIdx.x, rw, cand_boxes + sb * B, B, 0, order + sb, 0L, (long)R - 1, nb, rows, cols, at)) return;
  nms_mask_tile<AABB>(rows, cols, at.r0, at.c0, at.j, nb, thr, mask + sb * rw, rw, nullptr, nullptr);
}

// one workgroup per scene; R <= 16384 (256 words of removed-set)
__global__ __launch_bounds__(256) void roi_post_nms_scan_kernel(int R, int row_floats, const float* __restrict__ cand_boxes, const float* __restrict__ cand_scores,
                                                                const int* __restrict__ sorted_keys, const long* __restrict__ order, const unsigned long long* __restrict__ mask, int* keep,
                                                                float* __restrict__ boxes, float* __restrict__ scores, int* __restrict__ index, int* __restrict__ counts_out) {
  __shared__ unsigned long long removed[256], diag[64];
  const int t = threadIdx.x, scene = blockIdx.x, rw = (R + 63) >> 6;
  const long sb = (long)scene * R;
  const int nb = surviving(sorted_keys + sb, R);
  int* kp = keep + sb;
  const int cnt = nms_greedy_walk(mask + sb * rw, rw, nb, kp, removed, diag);      // the same in every thread
  __syncthreads();                         // kp[] is complete and visible to the workgroup
  for (int r = t; r < R; r += 256) {
    float* __restrict__ dst = boxes + (sb + r) * row_floats;
    if (r < cnt) {
      const long src = source_row(order, sb, R, kp[r]);
      for (int c = 0; c < row_floats; ++c) dst[c] = cand_boxes[(sb + src) * row_floats + c];
      scores[sb + r] = cand_scores[sb + src];
      index[sb + r] = (int)src;
    } else {
      for (int c = 0; c < row_floats; ++c) dst[c] = 0.f;
      scores[sb + r] = 0.f;
      index[sb + r] = -1;
    }
  }
  if (t == 0) counts_out[scene] = cnt;
}

bool roi_post_dims_ok(int N, int R, int ncols) { return N >= 1 && N <= NMH_FCOS_MAX_SCENES && R >= 1 && R <= NMH_OBB_NMS_MAX && (ncols == 6 || ncols == 7); }

}  // namespace

int k_roi_post_select(int N, int R, int n_classes, int ncols, const float* pred_scores, const float* pred_bbox_deltas, const float* rois, const int* counts, const int* mesh_sizes,
                      float score_thresh, float min_size, int is_reg, int threshold_mode, float* cand_boxes, float* cand_scores, int* keys, hipStream_t st) {
  if (!roi_post_dims_ok(N, R, ncols) || n_classes < 2 || n_classes > NMH_ROI_MAX_CLASSES || (threshold_mode != 0 && threshold_mode != 1)) return -4;
  const dim3 grid((unsigned)(((long)N * R + 255) / 256));
  if (ncols == 7) hipLaunchKernelGGL(roi_post_select_kernel<true>, grid, dim3(256), 0, st, N, R, n_classes, pred_scores, pred_bbox_deltas, rois, counts, mesh_sizes, score_thresh, min_size,
                                     is_reg, threshold_mode, cand_boxes, cand_scores, keys);
  else hipLaunchKernelGGL(roi_post_select_kernel<false>, grid, dim3(256), 0, st, N, R, n_classes, pred_scores, pred_bbox_deltas, rois, counts, mesh_sizes, score_thresh, min_size, is_reg,
                          threshold_mode, cand_boxes, cand_scores, keys);
  NMH_CHECK_LAUNCH();
  return 0;
}

int k_roi_post_nms(int N, int R, int ncols, const float* cand_boxes, const float* cand_scores, const int* sorted_keys, const long* order, float nms_thresh, unsigned long long* mask,
                   int* keep, float* boxes, float* scores, int* index, int* counts_out, hipStream_t st) {
  if (!roi_post_dims_ok(N, R, ncols)) return -4;
  const unsigned rw = (unsigned)((R + 63) / 64);
  const dim3 grid(rw * (rw + 1) / 2, (unsigned)N);
  if (ncols == 6) hipLaunchKernelGGL(roi_post_nms_mask_kernel<true>, grid, dim3(256), 0, st, R, cand_boxes, sorted_keys, order, nms_thresh, mask);
  else hipLaunchKernelGGL(roi_post_nms_mask_kernel<false>, grid, dim3(256), 0, st, R, cand_boxes, sorted_keys, order, nms_thresh, mask);
  NMH_CHECK_LAUNCH();
  hipLaunchKernelGGL(roi_post_nms_scan_kernel, dim3((unsigned)N), dim3(256), 0, st, R, ncols, cand_boxes, cand_scores, sorted_keys, order, mask, keep, boxes, scores, index, counts_out);
  NMH_CHECK_LAUNCH();
  return 0;
}

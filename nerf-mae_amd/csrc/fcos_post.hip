// FCOS inference post-processing of the reference's 3-D detector head (FCOSPostProcessor, nerf_rpn/model/fcos/inference.py:11-195, over
// clip_boxes_to_mesh / remove_small_boxes / nms of fcos/utils.py:109-209 and decode_fcos_obb, fcos/utils.py:12-61), as gfx950 kernels:
//   fcos_post_select     forward_for_single_feature_map (inference.py:48-129) for every (level, scene) in one launch: threshold, exact top-k,
//                        ordered compaction with decode, clip, size filter and sqrt fused;
//   fcos_post_nms_mask   the suppression bit matrices of all scenes in one launch (nms, fcos/utils.py:109-124, over box_iou_3d);
//   fcos_post_nms_scan   the greedy walk of all scenes in one launch, with the post-NMS cut (select_over_all_levels, inference.py:164-195)
//                        and the write of the results in its epilogue.
// fp32 throughout; nothing goes to scratch; every kernel writes only its own outputs for any input; the host never waits.
//
// Layout.  Level k has n_k locations per scene and keeps at most t_k = min(pre_nms_top_n, n_k) of them; cap = t_0 + .. + t_{L-1}.  Head outputs
// are read in place as in fcos.hip: channel c of level k at ((b C + c) n_k + q).  locations is one [n_k][3] array per level and is read (the
// reference's constructor has no strides, so locations are not re-derived).  Scene b owns cap rows of every per-scene array; level k owns
// the slots o_k .. o_k + t_k - 1 of them, o_k = t_0 + .. + t_{k-1}.
//
// Semantics, per (level k, scene b):
//   p = sigmoid(cls), c = sigmoid(ctr); a location is a candidate iff it is valid (mask byte != 0, or no masks) and p > pre_nms_thresh
//   (the unmultiplied score, as in the reference); s = p c; kept: the min(pre_nms_top_n, #candidates) candidates of largest s;
//   6 columns: (X - r0, Y - r1, Z - r2, X + r3, Y + r4, Z + r5), each axis clamped to [0, grid_sizes[b][axis]];
//   8 columns: the decode of fcos.hip (fcos_decode.hpp) at the location, theta by atan2, not clipped (as in the reference);
//   a kept box with a side < min_size is dropped (6 columns: x1 - x0 .., 8 columns: w, l, h); score = sqrt(s).
// Per scene: the levels concatenated; NMS with nms_thresh (suppressed iff IoU with a kept box > nms_thresh; the pair geometry of
// obb_geom.hpp, 6- or 7-column form); if fpn_post_nms_top_n > 0 and more boxes than that remain, those with score >= the
// fpn_post_nms_top_n-th largest remaining score stay (the reference's kthvalue rule: ties at the cut all stay).
// Where the reference leaves the result open (topk(sorted=False), argsort), it is DEFINED here: the pre-NMS order is level-major, then
// ascending location index; a tie at a top-k cut goes to the lower location index; the NMS order is the stable descending sort of the
// scores (the caller's sort; a dropped or unused slot carries the score -1 and sorts last).
//
// Algorithm.  select: one workgroup of 1024 lanes per (level, scene).  Pass 0 forms the key of every location (0: no candidate, else the bits
// of s plus 1: s >= 0, so unsigned order is score order), stores it, counts the candidates and fills the first histogram.  If there are more
// candidates than t_k, the radix select of select_scan.hpp finds the t_k-th largest key over the stored keys; its ordered compaction gives every
// kept location its slot, ties at the cut to the lower index.  A kept box dropped by min_size keeps its slot with score -1, so slots never depend
// on an atomic; two runs are bit-identical.
// nms: the bit matrix and the walk of nms_bits.hpp, rows of cap/64 words for every scene; the grid is the upper triangle for cap, and a
// workgroup whose columns start beyond the scene's count (read from device memory) exits at once.
#include "common.hpp"
#include "kernels.hpp"
#include "nms_bits.hpp"
#include "fcos_decode.hpp"
#include "select_scan.hpp"
#include "levels4.hpp"

namespace {

struct PostGeom {            // kernel argument, by value
  int L, N, cap;
  int n[4], top[4], off[4];  // locations, kept at most, first slot
  long p0[4];                // first key of (level, scene 0)
};

template <bool ORIENTED>
__global__ __launch_bounds__(SEL_T) void fcos_post_select_kernel(PostGeom G, Ptr4<const float> cls, Ptr4<const float> reg, Ptr4<const float> ctr, Ptr4<const float> locs,
                                                                 Ptr4<const unsigned char> masks, int have_masks, const int* __restrict__ sizes, float thr, float min_size,
                                                                 unsigned* __restrict__ keys, float* __restrict__ pre_boxes, float* __restrict__ pre_scores,
                                                                 int* __restrict__ pre_counts) {
  constexpr int C = ORIENTED ? 8 : 6, ROW = ORIENTED ? 8 : 7;
  __shared__ int hist[2048];
  __shared__ int wsum[SEL_T / 64];
  __shared__ int sh[2];
  const int t = threadIdx.x, lvl = blockIdx.x / G.N, scene = blockIdx.x - lvl * G.N;
  const int n = pick4(G.n, lvl), top = pick4(G.top, lvl), off = pick4(G.off, lvl);
  const float* __restrict__ pc = pick4(cls.p, lvl) + (long)scene * n;
  const float* __restrict__ pt = pick4(ctr.p, lvl) + (long)scene * n;
  const float* __restrict__ pr = pick4(reg.p, lvl) + (long)scene * C * n;
  const float* __restrict__ pl = pick4(locs.p, lvl);
  const unsigned char* __restrict__ pm = have_masks ? pick4(masks.p, lvl) + (long)scene * n : nullptr;
  unsigned* __restrict__ kk = keys + pick4(G.p0, lvl) + (long)scene * n;

  // pass 0: keys, the candidate count, the histogram of the top 11 bits
  hist_clear(hist);
  int mine = 0;
  for (int q = t; q < n; q += SEL_T) {
    const float p = sigmoid_stable(pc[q]);
    const bool cand = (!pm || pm[q] != 0) && p > thr;
    unsigned key = 0u;
    if (cand) {
      key = __float_as_uint(p * sigmoid_stable(pt[q])) + 1u;
      atomicAdd(&hist[key >> 21], 1);
      ++mine;
    }
    kk[q] = key;                           // read back below by this lane only
  }
  int ncand;
  block_scan_excl(mine, ncand, wsum);      // its barriers also complete hist
  RadixCut cut{0u, 0};                     // keep key > K, and the first need_eq of key == K
  const int k = min(top, ncand);
  if (ncand > top) cut = radix_select_rest(hist, wsum, sh, k, n, [&](int q, unsigned& key) { key = kk[q]; return true; });      // uniform: a cut is needed

  // ordered compaction with decode, clip, size filter and sqrt
  int run_eq = 0, run_sel = 0, emitted = 0;
  const float fl = (float)lvl;
  for (int base = 0; base < n && run_sel < k; base += SEL_T) {       // uniform
    const int q = base + t;
    const unsigned key = q < n ? kk[q] : 0u;
    int pos;
    const bool sel = compact_step(key > cut.K, key == cut.K, cut.need_eq > 0, cut.need_eq, run_eq, run_sel, wsum, pos);
    if (sel && pos < top) {                // pos < k <= top for every input whose keys are ordinary numbers
      const float X = pl[(long)q * 3], Y = pl[(long)q * 3 + 1], Z = pl[(long)q * 3 + 2];
      float r[8], o[7];
#pragma unroll
      for (int c = 0; c < C; ++c) r[c] = pr[(long)c * n + q];
      bool ok;
      if (ORIENTED) {
        const Dec d = fcos_decode(r);
        const bool zero = d.mx == 0.f && d.my == 0.f;
        o[0] = X + d.o.x; o[1] = Y + d.o.y; o[2] = Z + d.o.z; o[3] = d.o.w; o[4] = d.o.l; o[5] = d.o.h; o[6] = atan2f(d.my, zero ? 1e-7f : d.mx);
        ok = o[3] >= min_size && o[4] >= min_size && o[5] >= min_size;
      } else {
        const float sx = (float)sizes[scene * 3], sy = (float)sizes[scene * 3 + 1], sz = (float)sizes[scene * 3 + 2];
        o[0] = clampf(X - r[0], 0.f, sx); o[1] = clampf(Y - r[1], 0.f, sy); o[2] = clampf(Z - r[2], 0.f, sz);
        o[3] = clampf(X + r[3], 0.f, sx); o[4] = clampf(Y + r[4], 0.f, sy); o[5] = clampf(Z + r[5], 0.f, sz);
        o[6] = 0.f;
        ok = o[3] - o[0] >= min_size && o[4] - o[1] >= min_size && o[5] - o[2] >= min_size;
      }
      const long slot = (long)scene * G.cap + off + pos;
      float* __restrict__ row = pre_boxes + slot * ROW;
      row[0] = fl;
#pragma unroll
      for (int c = 0; c < ROW - 1; ++c) row[1 + c] = o[c];
      pre_scores[slot] = ok ? sqrtf(__uint_as_float(key - 1u)) : -1.f;
      emitted += ok ? 1 : 0;
    }
  }
  // the level's unused slots
  for (int s = run_sel + t; s < top; s += SEL_T) {
    const long slot = (long)scene * G.cap + off + s;
#pragma unroll
    for (int c = 0; c < ROW; ++c) pre_boxes[slot * ROW + c] = 0.f;
    pre_scores[slot] = -1.f;
  }
  int total;
  block_scan_excl(emitted, total, wsum);
  if (t == 0) pre_counts[lvl * G.N + scene] = total;
}

// ---- NMS of every scene: the scene's boxes are rows order[b][0 .. n_b - 1] of pre_boxes[b] (the caller's stable descending sort) ------------
__device__ __forceinline__ int scene_count(const PostGeom& G, const int* __restrict__ pre_counts, int scene) {
  int nb = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) nb += k < G.L ? pre_counts[k * G.N + scene] : 0;
  return min(nb, G.cap);
}

template <bool AABB>
__global__ __launch_bounds__(256) void fcos_post_nms_mask_kernel(PostGeom G, const float* __restrict__ pre_boxes, const long* __restrict__ order, const int* __restrict__ pre_counts,
                                                                 float thr, unsigned long long* __restrict__ mask) {
  constexpr int ROW = AABB ? 7 : 8;
  __shared__ BoxTile rows[64], cols[64];
  const int scene = blockIdx.y, capw = (G.cap + 63) >> 6;
  const int nb = scene_count(G, pre_counts, scene);
  const long sb = (long)scene * G.cap;
  NmsBlock at;                                         // col 1: past the level column
  if (!nms_stage_sorted<AABB>(blockIdx.x, capw, pre_boxes + sb * ROW, ROW, 1, order + sb, 0L, (long)G.cap - 1, nb, rows, cols, at)) return;
  nms_mask_tile<AABB>(rows, cols, at.r0, at.c0, at.j, nb, thr, mask + sb * capw, capw, nullptr, nullptr);
}

// one workgroup per scene; cap <= 16384 (256 words of removed-set)
__global__ __launch_bounds__(256) void fcos_post_nms_scan_kernel(PostGeom G, int row_floats, const float* __restrict__ pre_boxes, const float* __restrict__ sorted_scores,
                                                                 const long* __restrict__ order, const int* __restrict__ pre_counts, const unsigned long long* __restrict__ mask,
                                                                 int post_top_n, int* keep, float* __restrict__ boxes, float* __restrict__ scores, int* __restrict__ counts) {
  __shared__ unsigned long long removed[256], diag[64];
  __shared__ int extra;
  const int t = threadIdx.x, scene = blockIdx.x, capw = (G.cap + 63) >> 6;
  const int N = scene_count(G, pre_counts, scene);
  const long sb = (long)scene * G.cap;
  const unsigned long long* __restrict__ m0 = mask + sb * capw;
  int* kp = keep + sb;
  if (t == 0) extra = 0;
  const int cnt = nms_greedy_walk(m0, capw, N, kp, removed, diag);      // the same in every thread
  __syncthreads();                         // kp[] is complete and visible to the workgroup
  // post-NMS cut: kept boxes are in decreasing score, so those with score >= the post_top_n-th are a prefix
  int m = cnt;
  if (post_top_n > 0 && cnt > post_top_n) {
    const float cut = sorted_scores[sb + kp[post_top_n - 1]];
    int more = 0;
    for (int i = post_top_n + t; i < cnt; i += 256) more += sorted_scores[sb + kp[i]] >= cut ? 1 : 0;
    if (more) atomicAdd(&extra, more);     // an integer sum: the order does not matter
    __syncthreads();
    m = post_top_n + extra;
  }
  for (int r = t; r < G.cap; r += 256) {
    float* __restrict__ dst = boxes + (sb + r) * row_floats;
    if (r < m) {
      const int i = kp[r];
      const long src = min(max(order[sb + i], 0L), (long)G.cap - 1);
      for (int c = 0; c < row_floats; ++c) dst[c] = pre_boxes[(sb + src) * row_floats + c];
      scores[sb + r] = sorted_scores[sb + i];
    } else {
      for (int c = 0; c < row_floats; ++c) dst[c] = 0.f;
      scores[sb + r] = 0.f;
    }
  }
  if (t == 0) counts[scene] = m;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
int make_post_geom(int nlevels, const int* level_n, int N, int pre_top_n, PostGeom& G) {
  if (nlevels < 1 || nlevels > 4 || N < 1 || N > NMH_FCOS_MAX_SCENES || !level_n || pre_top_n < 1) return -4;
  G.L = nlevels; G.N = N;
  long cap = 0, p0 = 0;
  for (int k = 0; k < 4; ++k) {
    const int j = k < nlevels ? k : nlevels - 1;
    const long n = level_n[j];
    if (n < 1 || n > (1L << 30)) return -4;
    G.n[k] = (int)n; G.top[k] = (int)(n < pre_top_n ? n : pre_top_n);
    G.off[k] = (int)cap; G.p0[k] = p0;
    if (k < nlevels) { cap += G.top[k]; p0 += n * N; }
    if (p0 >= (1L << 40)) return -4;
  }
  if (cap > NMH_OBB_NMS_MAX) return -4;
  G.cap = (int)cap;
  return 0;
}

}  // namespace

long k_fcos_post_cap(int nlevels, const int* level_n, int N, int pre_top_n) {
  PostGeom G;
  return make_post_geom(nlevels, level_n, N, pre_top_n, G) ? -1 : G.cap;
}

int k_fcos_post_select(int nlevels, const int* level_n, int N, int ncols, int pre_top_n, const float* const* cls, const float* const* reg, const float* const* ctr,
                       const float* const* locs, const unsigned char* const* masks, const int* sizes, float pre_thresh, float min_size, unsigned* keys, float* pre_boxes,
                       float* pre_scores, int* pre_counts, hipStream_t st) {
  PostGeom G;
  if (make_post_geom(nlevels, level_n, N, pre_top_n, G) || (ncols != 6 && ncols != 8)) return -4;
  if (!all_set(nlevels, cls) || !all_set(nlevels, reg) || !all_set(nlevels, ctr) || !all_set(nlevels, locs)) return -4;
  if ((masks && !all_set(nlevels, masks)) || (ncols == 6 && !sizes)) return -4;
  const Ptr4<const float> Cl = make_ptrs<const float>(nlevels, cls), R = make_ptrs<const float>(nlevels, reg), Ct = make_ptrs<const float>(nlevels, ctr),
                          Lo = make_ptrs<const float>(nlevels, locs);
  const Ptr4<const unsigned char> M = make_ptrs<const unsigned char>(nlevels, masks);
  const dim3 grid((unsigned)(nlevels * N));
  if (ncols == 8) hipLaunchKernelGGL(fcos_post_select_kernel<true>, grid, dim3(SEL_T), 0, st, G, Cl, R, Ct, Lo, M, masks ? 1 : 0, sizes, pre_thresh, min_size, keys, pre_boxes, pre_scores, pre_counts);
  else hipLaunchKernelGGL(fcos_post_select_kernel<false>, grid, dim3(SEL_T), 0, st, G, Cl, R, Ct, Lo, M, masks ? 1 : 0, sizes, pre_thresh, min_size, keys, pre_boxes, pre_scores, pre_counts);
  NMH_CHECK_LAUNCH();
  return 0;
}

int k_fcos_post_nms(int nlevels, const int* level_n, int N, int ncols, int pre_top_n, const float* pre_boxes, const float* sorted_scores, const long* order, const int* pre_counts,
                    float nms_thresh, int post_top_n, unsigned long long* mask, int* keep, float* boxes, float* scores, int* counts, hipStream_t st) {
  PostGeom G;
  if (make_post_geom(nlevels, level_n, N, pre_top_n, G) || (ncols != 6 && ncols != 8)) return -4;
  const unsigned capw = (unsigned)((G.cap + 63) / 64);
  const dim3 grid(capw * (capw + 1) / 2, (unsigned)N);
  if (ncols == 6) hipLaunchKernelGGL(fcos_post_nms_mask_kernel<true>, grid, dim3(256), 0, st, G, pre_boxes, order, pre_counts, nms_thresh, mask);
  else hipLaunchKernelGGL(fcos_post_nms_mask_kernel<false>, grid, dim3(256), 0, st, G, pre_boxes, order, pre_counts, nms_thresh, mask);
  NMH_CHECK_LAUNCH();
  hipLaunchKernelGGL(fcos_post_nms_scan_kernel, dim3((unsigned)N), dim3(256), 0, st, G, ncols == 6 ? 7 : 8, pre_boxes, sorted_scores, order, pre_counts, mask, post_top_n, keep, boxes,
                     scores, counts);
  NMH_CHECK_LAUNCH();
  return 0;
}

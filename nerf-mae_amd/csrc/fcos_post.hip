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
// of s plus 1: s >= 0, so unsigned order is score order), stores it and counts the candidates.  If there are more candidates than t_k, a radix
// select finds the t_k-th largest key K from three LDS histograms (11 + 11 + 10 bits, integer atomics: the sums do not depend on their order),
// each scanned from the top by a workgroup prefix sum.  The compaction walks the locations in chunks of 1024 in ascending order; two
// workgroup prefix sums per chunk give every lane the number of keys == K before it (the first t_k - #(key > K) of them are kept: the tie
// rule) and its slot.  A kept box dropped by min_size keeps its slot with score -1, so slots never depend on an atomic; two runs are bit-identical.
// nms: word (i, j) of a scene's matrix per wave, as obb_nms_mask of rotated_iou.hip, rows of cap/64 words for every scene; the grid is the
// upper triangle for cap, and a workgroup whose columns start beyond the scene's count (read from device memory) exits at once.
#include "common.hpp"
#include "kernels.hpp"
#include "obb_geom.hpp"
#include "fcos_decode.hpp"
#include "select_scan.hpp"          // SEL_T, block_scan_excl, radix_pick

namespace {

struct PostGeom {            // kernel argument, by value
  int L, N, cap;
  int n[4], top[4], off[4];  // locations, kept at most, first slot
  long p0[4];                // first key of (level, scene 0)
};
template <typename T> struct PPtr4 { T* p[4]; };
template <typename T> __device__ __forceinline__ T ppick4(const T (&a)[4], int i) { return i == 0 ? a[0] : (i == 1 ? a[1] : (i == 2 ? a[2] : a[3])); }

__device__ __forceinline__ float post_sigmoid(float x) {
  const float e = expf(-fabsf(x)), r = 1.f / (1.f + e);
  return x >= 0.f ? r : e * r;
}

template <bool ORIENTED>
__global__ __launch_bounds__(SEL_T) void fcos_post_select_kernel(PostGeom G, PPtr4<const float> cls, PPtr4<const float> reg, PPtr4<const float> ctr, PPtr4<const float> locs,
                                                                 PPtr4<const unsigned char> masks, int have_masks, const int* __restrict__ sizes, float thr, float min_size,
                                                                 unsigned* __restrict__ keys, float* __restrict__ pre_boxes, float* __restrict__ pre_scores,
                                                                 int* __restrict__ pre_counts) {
  constexpr int C = ORIENTED ? 8 : 6, ROW = ORIENTED ? 8 : 7;
  __shared__ int hist[2048];
  __shared__ int wsum[SEL_T / 64];
  __shared__ int sh[2];
  const int t = threadIdx.x, lvl = blockIdx.x / G.N, scene = blockIdx.x - lvl * G.N;
  const int n = ppick4(G.n, lvl), top = ppick4(G.top, lvl), off = ppick4(G.off, lvl);
  const float* __restrict__ pc = ppick4(cls.p, lvl) + (long)scene * n;
  const float* __restrict__ pt = ppick4(ctr.p, lvl) + (long)scene * n;
  const float* __restrict__ pr = ppick4(reg.p, lvl) + (long)scene * C * n;
  const float* __restrict__ pl = ppick4(locs.p, lvl);
  const unsigned char* __restrict__ pm = have_masks ? ppick4(masks.p, lvl) + (long)scene * n : nullptr;
  unsigned* __restrict__ kk = keys + ppick4(G.p0, lvl) + (long)scene * n;

  // pass 0: keys, the candidate count, the histogram of the top 11 bits
  hist[t] = 0; hist[t + SEL_T] = 0;
  __syncthreads();
  int mine = 0;
  for (int q = t; q < n; q += SEL_T) {
    const float p = post_sigmoid(pc[q]);
    const bool cand = (!pm || pm[q] != 0) && p > thr;
    unsigned key = 0u;
    if (cand) {
      key = __float_as_uint(p * post_sigmoid(pt[q])) + 1u;
      atomicAdd(&hist[key >> 21], 1);
      ++mine;
    }
    kk[q] = key;                           // read back below by this lane only
  }
  int ncand;
  block_scan_excl(mine, ncand, wsum);      // its barriers also complete hist
  unsigned K = 0u;                         // keep key > K, and the first need_eq of key == K
  int need_eq = 0;
  const int k = min(top, ncand);
  if (ncand > top) {                       // uniform: a cut is needed
    radix_pick(hist, k, wsum, sh);
    const unsigned d0 = (unsigned)sh[0];
    int r = sh[1];
    __syncthreads();
    hist[t] = 0; hist[t + SEL_T] = 0;
    __syncthreads();
    for (int q = t; q < n; q += SEL_T) {
      const unsigned key = kk[q];
      if ((key >> 21) == d0) atomicAdd(&hist[(key >> 10) & 2047u], 1);
    }
    __syncthreads();
    radix_pick(hist, r, wsum, sh);
    const unsigned d01 = (d0 << 11) | (unsigned)sh[0];
    r = sh[1];
    __syncthreads();
    hist[t] = 0; hist[t + SEL_T] = 0;
    __syncthreads();
    for (int q = t; q < n; q += SEL_T) {
      const unsigned key = kk[q];
      if ((key >> 10) == d01) atomicAdd(&hist[1024 + (key & 1023u)], 1);      // the upper half of the bins, so that radix_pick's scan order holds
    }
    __syncthreads();
    radix_pick(hist, r, wsum, sh);
    K = (d01 << 10) | (unsigned)(sh[0] - 1024);
    need_eq = sh[1];
    __syncthreads();
  }

  // ordered compaction with decode, clip, size filter and sqrt
  int run_eq = 0, run_sel = 0, emitted = 0;
  const float fl = (float)lvl;
  for (int base = 0; base < n && run_sel < k; base += SEL_T) {       // uniform
    const int q = base + t;
    const unsigned key = q < n ? kk[q] : 0u;
    bool sel = key > K;
    if (need_eq > 0) {                     // uniform
      const bool eq = key == K;
      int tot;
      const int rank = run_eq + block_scan_excl(eq ? 1 : 0, tot, wsum);
      run_eq += tot;
      sel = sel || (eq && rank < need_eq);
    }
    int tot;
    const int pos = run_sel + block_scan_excl(sel ? 1 : 0, tot, wsum);
    run_sel += tot;
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
__device__ __forceinline__ void stage_row(const float* __restrict__ row, BoxTile& dst) {
  if (AABB) {
#pragma unroll
    for (int k = 0; k < 6; ++k) dst.v[k] = row[k];
    dst.v[6] = dst.v[7] = 0.f;
  } else {
    const Obb o = obb_load(row);
    dst.v[0] = o.x; dst.v[1] = o.y; dst.v[2] = o.z; dst.v[3] = o.w; dst.v[4] = o.l; dst.v[5] = o.h; dst.v[6] = o.cs; dst.v[7] = o.sn;
  }
}

template <bool AABB>
__global__ __launch_bounds__(256) void fcos_post_nms_mask_kernel(PostGeom G, const float* __restrict__ pre_boxes, const long* __restrict__ order, const int* __restrict__ pre_counts,
                                                                 float thr, unsigned long long* __restrict__ mask) {
  constexpr int ROW = AABB ? 7 : 8;
  __shared__ BoxTile rows[64], cols[64];
  const int t = threadIdx.x, scene = blockIdx.y, capw = (G.cap + 63) >> 6;
  const int nb = scene_count(G, pre_counts, scene);
  int by = 0, j = blockIdx.x;
  while (j >= capw - by) { j -= capw - by; ++by; }    // uniform, at most capw <= 256 steps
  j += by;
  const int r0 = by * 64, c0 = j * 64;
  if (c0 >= nb) return;                                // uniform; r0 <= c0
  const long sb = (long)scene * G.cap;
  if (t < 128) {
    const int i = (t < 64 ? c0 : r0 - 64) + t;
    BoxTile& dst = t < 64 ? cols[t] : rows[t - 64];
    if (i < nb) {
      const long src = min(max(order[sb + i], 0L), (long)G.cap - 1);
      stage_row<AABB>(pre_boxes + (sb + src) * ROW + 1, dst);
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) dst.v[k] = 0.f;
    }
  }
  __syncthreads();
  const int k = t & 63, col = c0 + k;
  const BoxTile bc = cols[k];
#pragma unroll 1
  for (int r = t >> 6; r < 64; r += 4) {
    const int row = r0 + r;
    if (row >= nb) break;                              // uniform over the wave
    bool hit = false;
    if (col > row && col < nb) hit = tile_iou<AABB>(rows[r], bc) > thr;
    const unsigned long long word = __ballot(hit);
    if (k == 0) mask[(sb + row) * capw + j] = word;
  }
}

// one workgroup per scene; cap <= 16384 (256 words of removed-set)
__global__ __launch_bounds__(256) void fcos_post_nms_scan_kernel(PostGeom G, int row_floats, const float* __restrict__ pre_boxes, const float* __restrict__ sorted_scores,
                                                                 const long* __restrict__ order, const int* __restrict__ pre_counts, const unsigned long long* __restrict__ mask,
                                                                 int post_top_n, int* keep, float* __restrict__ boxes, float* __restrict__ scores, int* __restrict__ counts) {
  __shared__ unsigned long long removed[256], diag[64];
  __shared__ int extra;
  const int t = threadIdx.x, scene = blockIdx.x, capw = (G.cap + 63) >> 6;
  const int N = scene_count(G, pre_counts, scene), nw = (N + 63) >> 6;
  const long sb = (long)scene * G.cap;
  const unsigned long long* __restrict__ m0 = mask + sb * capw;
  int* kp = keep + sb;
  removed[t] = 0ull;
  if (t == 0) extra = 0;
  int cnt = 0;                             // the same in every thread
  for (int c = 0; c < nw; ++c) {
    __syncthreads();                       // removed[] of the previous block is complete; diag[] is free
    if (t < 64) diag[t] = c * 64 + t < N ? m0[(long)(c * 64 + t) * capw + c] : 0ull;
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
        const unsigned long long m = m0[(long)(c * 64 + k) * capw + w];
        if (m) atomicOr(&removed[w], m);
      }
    }
  }
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
template <typename T> PPtr4<T> post_ptrs(int nlevels, T* const* tab) {
  PPtr4<T> r;
  for (int k = 0; k < 4; ++k) r.p[k] = tab ? tab[k < nlevels ? k : nlevels - 1] : nullptr;
  return r;
}
template <typename T> bool post_all_set(int nlevels, T* const* tab) {
  if (!tab) return false;
  for (int k = 0; k < nlevels; ++k) if (!tab[k]) return false;
  return true;
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
  if (!post_all_set(nlevels, cls) || !post_all_set(nlevels, reg) || !post_all_set(nlevels, ctr) || !post_all_set(nlevels, locs)) return -4;
  if ((masks && !post_all_set(nlevels, masks)) || (ncols == 6 && !sizes)) return -4;
  const PPtr4<const float> Cl = post_ptrs<const float>(nlevels, cls), R = post_ptrs<const float>(nlevels, reg), Ct = post_ptrs<const float>(nlevels, ctr),
                           Lo = post_ptrs<const float>(nlevels, locs);
  const PPtr4<const unsigned char> M = post_ptrs<const unsigned char>(nlevels, masks);
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

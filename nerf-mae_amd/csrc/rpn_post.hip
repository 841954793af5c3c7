// Inference path of the reference's anchor-based 3-D RegionProposalNetwork (everything behind `if not self.training:` in nerf_rpn/model/rpn.py:507-512), as
// gfx950 kernels:
//   rpn_decode           box_coder.decode_list (coder/base_bbox_coder.py:55-86) of every anchor, one lane per anchor: [N][n][6|7], anchor order, not clipped;
//   rpn_post_select      _get_top_n_idx (rpn.py:292-301) and the per-box half of filter_proposals (rpn.py:303-357: padding mask, top-k per level, sigmoid,
//                        clip_boxes_to_mesh, remove_small_boxes, score threshold) for every (level, scene) in one launch; only the selected anchors are decoded;
//   rpn_post_nms_mask    the suppression bit matrices of batched_nms (model/utils.py:215-265): one matrix per (scene, level), all in one launch;
//   rpn_post_nms_scan    the greedy walks of all scenes in one launch, and in its epilogue keep[:post_nms_top_n] (rpn.py:363) with the write of the results.
// fp32 throughout; nothing goes to scratch; every kernel writes only its own outputs for any input; the host never waits.
//
// Layout.  Levels, anchors and head tensors as in rpn.hip: level k has n_k = W H D A anchors per scene, anchor i = loc A + a in ANCHOR order, and lies in the
// objectness tensor (N, A, W, H, D) at MEMORY offset a nloc + loc; regression is (N, A C, W, H, D), channel a C + c.  Level k keeps t_k = min(pre_nms_top_n, n_k)
// anchors; cap = t_0 + .. + t_{L-1}.  Scene b owns cap rows of every per-scene array; level k owns the slots o_k .. o_k + t_k - 1, o_k = t_0 + .. + t_{k-1}.
//
// Selection, per (level k, scene b).  The key of an anchor is its raw objectness logit (sigmoid is monotone): the fp32 bits with the order-preserving
// transform (negative: all bits flipped; else the sign bit set), so unsigned order is float order with -0 below +0.  With ori_sizes, an anchor whose grid index
// is not below ceil(ori / stride) on every axis (the test of rpn_anchor) is MASKED: key 0, below every logit, -inf (key 0x007fffff) included.  A NaN logit is
// read as -inf wherever it is used (key, order, score 0).  Kept are the t_k largest keys.  A masked anchor is therefore still selected when fewer unmasked
// anchors exist than t_k; its score is exactly 0.  This is what the reference does: -inf objectness, topk(min(pre_nms_top_n, n_k)), sigmoid(-inf) = 0, and
// 0 >= score_thresh at the default 0.0.  The reference leaves the tie winner at the cut and the slot order within a level open; they are DEFINED here by the
// memory order: a tie at the cut goes to the lower memory offset, and slot o_k + j holds the j-th selected anchor in ascending memory offset.
// For the selected anchors only: the decode (rpn_decode.hpp); 6 columns: each axis clamped to [0, mesh_size[axis]]; 7 columns: not clipped, and a box whose
// centre lies outside [0, mesh_size] on any axis is dropped; a box with a side below min_size (6 columns: the differences; 7: w, h, d) is dropped; score =
// sigmoid(logit) (0 for a masked anchor), and a box with score < score_thresh is dropped.  A dropped box keeps its slot, marked empty (all-zero row, sort key
// with low word 0), so slots never depend on an atomic; two runs are bit-identical.  Every row also carries the anchor's index in the scene's concatenated
// anchors in rpn_assign's order, off_k + loc A + a.
// Sort key (int64): high word L - 1 - level, low word 0 for an empty slot, 1 for a masked anchor, else the transformed logit.  The caller's stable descending
// sort of the [N][cap] keys is therefore level-major, within a level by descending logit with ties to the lower slot, the empty slots of a level last.
//
// Algorithm of the selection.  One workgroup of 1024 lanes per (level, scene), walking the level in memory order so that reads are coalesced.  No key array is
// stored: every pass re-reads the logits (L2-resident) and re-forms the keys.  If n_k > t_k, the radix select of select_scan.hpp finds the t_k-th largest key;
// its ordered compaction walks chunks of 1024 in ascending offset and gives every kept anchor its slot, ties at the cut to the lower offset.
//
// NMS.  A box is suppressed iff its IoU with a kept box of the SAME level is greater than nms_thresh (pair geometry: obb_geom.hpp, 6- or 7-column form).
// Pairs from different levels never reach the geometry: level k of scene b has its own bit matrix of t_k rows of ceil(t_k / 64) words over the level's
// sorted boxes (nms_bits.hpp); only the upper triangles of 64 x 64 blocks are launched and a workgroup whose columns start beyond the level's count exits at once.  The scan is
// one workgroup per scene that walks its levels one after the other (nms_greedy_walk on each), leaving per level the kept positions in descending key.
// Epilogue: the global order is descending logit with ties to the lower slot; a survivor's rank is its rank in its own level plus, for every other level,
// the number of that level's survivors before it, found by binary search in that level's descending keys (equal keys: the lower level first).  Survivors of
// rank < post_nms_top_n are written to row rank: boxes, score, level, anchor index; rows past the count are zero.  No atomics on anything that is ordered.
#include "common.hpp"
#include "kernels.hpp"
#include "nms_bits.hpp"
#include "select_scan.hpp"
#include "rpn_geom.hpp"
#include "rpn_decode.hpp"

namespace {

struct RpnPostGeom {         // kernel argument, by value
  int cap, mesh[3];
  int top[4], off[4];        // kept at most, first slot
  int tw[4], blk0[4];        // words per mask row, first mask workgroup of the level (upper triangle of tw x tw blocks)
  long moff[4], mtot;        // first mask word of the level within a scene, mask words per scene
  int mblocks;
};

__device__ __forceinline__ unsigned rpn_order_bits(float x) {           // NaN reads as -inf
  const unsigned u = x != x ? 0xff800000u : __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// the padding test on a location, with the limits ceil(ori / stride) taken once per workgroup
struct RpnLim { int H, D, lx, ly, lz; bool on; };
__device__ __forceinline__ RpnLim rpn_limits(const RpnGeom& G, const int* __restrict__ ori, int lvl, int scene) {
  RpnLim m;
  m.H = pick4(G.H, lvl); m.D = pick4(G.D, lvl); m.on = ori != nullptr;
  m.lx = m.ly = m.lz = 0;
  if (ori) {
    const int sx = pick4(G.sx, lvl), sy = pick4(G.sy, lvl), sz = pick4(G.sz, lvl);
    m.lx = (ori[scene * 3] + sx - 1) / sx; m.ly = (ori[scene * 3 + 1] + sy - 1) / sy; m.lz = (ori[scene * 3 + 2] + sz - 1) / sz;
  }
  return m;
}
__device__ __forceinline__ bool rpn_loc_valid(const RpnLim& m, int loc) {
  if (!m.on) return true;
  const int d = loc % m.D, h = (loc / m.D) % m.H, w = loc / (m.D * m.H);
  return w < m.lx && h < m.ly && d < m.lz;
}
// key of memory offset q of the level (q < n): 0 masked, else the transformed logit (>= 0x007fffff)
__device__ __forceinline__ unsigned rpn_key_at(const float* __restrict__ po, const RpnLim& m, int nloc, int q) {
  return rpn_loc_valid(m, q % nloc) ? rpn_order_bits(po[q]) : 0u;
}

template <bool ORIENTED>
__global__ __launch_bounds__(SEL_T) void rpn_post_select_kernel(RpnGeom G, RpnBase B, RpnPostGeom P, Ptr4<const float> obj, Ptr4<const float> reg, const int* __restrict__ ori,
                                                                float score_thresh, float min_size, long* __restrict__ pre_keys, float* __restrict__ pre_boxes,
                                                                float* __restrict__ pre_scores, int* __restrict__ pre_index, int* __restrict__ pre_counts) {
  constexpr int C = ORIENTED ? 8 : 6, ROW = ORIENTED ? 7 : 6;
  __shared__ int hist[2048];
  __shared__ int wsum[SEL_T / 64];
  __shared__ int sh[2];
  __shared__ float sh_base[RPN_MAX_A * 3];
  const int t = threadIdx.x, lvl = blockIdx.x / G.N, scene = blockIdx.x - lvl * G.N;
  const int n = pick4(G.n, lvl), nloc = pick4(G.nloc, lvl), A = pick4(G.A, lvl), top = pick4(P.top, lvl), off = pick4(P.off, lvl);
  const float* __restrict__ po = pick4(obj.p, lvl) + (long)scene * n;
  const float* __restrict__ pr = pick4(reg.p, lvl) + (long)scene * n * C;
  const RpnLim lim = rpn_limits(G, ori, lvl, scene);
  rpn_stage_base(B, lvl, A, sh_base);

  const bool all = n <= top;               // uniform: no cut is needed, every anchor is kept
  RadixCut cut{0u, 0};                     // else: keep key > K, and the first need_eq of key == K
  if (!all) cut = radix_select(hist, wsum, sh, top, n, [&](int q, unsigned& key) { key = rpn_key_at(po, lim, nloc, q); return true; });

  // ordered compaction with decode, clip, centre, size and score filters
  int run_eq = 0, run_sel = 0, emitted = 0;
  const long hi = (long)(G.L - 1 - lvl) << 32;
  for (int base = 0; base < n && run_sel < top; base += SEL_T) {       // uniform
    const int q = base + t;
    const unsigned key = q < n ? rpn_key_at(po, lim, nloc, q) : 0u;
    int pos;                               // the barriers of the step also complete sh_base in the first chunk
    const bool sel = compact_step(q < n && (all || key > cut.K), q < n && key == cut.K, !all, cut.need_eq, run_eq, run_sel, wsum, pos);
    if (sel && pos < top) {
      const int a = q / nloc, loc = q - a * nloc;
      RAt at;
      at.lvl = lvl; at.scene = scene; at.i = loc * A + a; at.active = true;
      bool valid;
      const Box6 anc = rpn_anchor(G, sh_base, nullptr, at, valid);
      float r[8], o[7];
#pragma unroll
      for (int c = 0; c < C; ++c) r[c] = pr[((long)a * C + c) * nloc + loc];
      if (!ORIENTED) r[6] = r[7] = 0.f;
      const bool masked = key == 0u;
      float x = po[q];
      x = x != x ? -INFINITY : x;
      const float score = masked ? 0.f : sigmoid_stable(x);
      const float mx = (float)P.mesh[0], my = (float)P.mesh[1], mz = (float)P.mesh[2];
      bool ok;
      if (ORIENTED) {
        rpn_decode_obb(r, anc, o);
        ok = o[0] >= 0.f && o[0] <= mx && o[1] >= 0.f && o[1] <= my && o[2] >= 0.f && o[2] <= mz && o[3] >= min_size && o[4] >= min_size && o[5] >= min_size;
      } else {
        rpn_decode_aabb(r, anc, o);
        o[0] = fminf(fmaxf(o[0], 0.f), mx); o[1] = fminf(fmaxf(o[1], 0.f), my); o[2] = fminf(fmaxf(o[2], 0.f), mz);
        o[3] = fminf(fmaxf(o[3], 0.f), mx); o[4] = fminf(fmaxf(o[4], 0.f), my); o[5] = fminf(fmaxf(o[5], 0.f), mz);
        ok = o[3] - o[0] >= min_size && o[4] - o[1] >= min_size && o[5] - o[2] >= min_size;
      }
      ok = ok && score >= score_thresh;
      const long slot = (long)scene * P.cap + off + pos;
#pragma unroll
      for (int c = 0; c < ROW; ++c) pre_boxes[slot * ROW + c] = ok ? o[c] : 0.f;
      pre_scores[slot] = ok ? score : 0.f;
      pre_index[slot] = ok ? pick4(G.off, lvl) + at.i : 0;
      pre_keys[slot] = hi | (long)(ok ? (masked ? 1u : key) : 0u);
      emitted += ok ? 1 : 0;
    }
  }
  // the level's unused slots (none for an input whose keys select t_k anchors; kept so that every slot is written for any input)
  for (int s = run_sel + t; s < top; s += SEL_T) {
    const long slot = (long)scene * P.cap + off + s;
#pragma unroll
    for (int c = 0; c < ROW; ++c) pre_boxes[slot * ROW + c] = 0.f;
    pre_scores[slot] = 0.f;
    pre_index[slot] = 0;
    pre_keys[slot] = hi;
  }
  int total;
  block_scan_excl(emitted, total, wsum);
  if (t == 0) pre_counts[lvl * G.N + scene] = total;
}

// every anchor's decode, anchor order, not clipped
template <bool ORIENTED>
__global__ __launch_bounds__(256) void rpn_decode_kernel(RpnGeom G, RpnBase B, Ptr4<const float> reg, float* __restrict__ boxes) {
  constexpr int C = ORIENTED ? 8 : 6, ROW = ORIENTED ? 7 : 6;
  __shared__ float sh_base[RPN_MAX_A * 3];
  const RAt q = rpn_where(G);
  const int A = pick4(G.A, q.lvl), nloc = pick4(G.nloc, q.lvl);
  rpn_stage_base(B, q.lvl, A, sh_base);
  __syncthreads();
  bool valid;
  const Box6 anc = rpn_anchor(G, sh_base, nullptr, q, valid);
  if (!q.active) return;
  const int a = q.i % A, loc = q.i / A;
  const float* __restrict__ pr = pick4(reg.p, q.lvl) + ((long)q.scene * A + a) * C * nloc + loc;
  float r[8], o[7];
#pragma unroll
  for (int c = 0; c < C; ++c) r[c] = pr[(long)c * nloc];
  if (ORIENTED) rpn_decode_obb(r, anc, o);
  else { r[6] = r[7] = 0.f; rpn_decode_aabb(r, anc, o); }
  float* __restrict__ dst = boxes + ((long)q.scene * G.ntot + pick4(G.off, q.lvl) + q.i) * ROW;
#pragma unroll
  for (int c = 0; c < ROW; ++c) dst[c] = o[c];
}

// ---- NMS: level k's boxes of scene b are rows order[b][o_k + 0 .. nb - 1] of pre_boxes[b] (the caller's stable descending sort of the keys) --------------
__device__ __forceinline__ int level_count(const RpnGeom& G, const RpnPostGeom& P, const int* __restrict__ pre_counts, int lvl, int scene) {
  return min(max(pre_counts[lvl * G.N + scene], 0), pick4(P.top, lvl));
}
__device__ __forceinline__ long sorted_slot(const RpnPostGeom& P, const long* __restrict__ order, long sb, int off, int top, int i) {
  return min(max(order[sb + off + i], (long)off), (long)off + top - 1);          // within the level's slots for any input
}

template <bool AABB>
__global__ __launch_bounds__(256) void rpn_post_nms_mask_kernel(RpnGeom G, RpnPostGeom P, const float* __restrict__ pre_boxes, const long* __restrict__ order,
                                                                const int* __restrict__ pre_counts, float thr, unsigned long long* __restrict__ mask) {
  constexpr int ROW = AABB ? 6 : 7;
  __shared__ BoxTile rows[64], cols[64];
  const int scene = blockIdx.y, lvl = level_of_block(P.blk0, G.L, blockIdx.x);
  const int tw = pick4(P.tw, lvl), top = pick4(P.top, lvl), off = pick4(P.off, lvl);
  const int nb = level_count(G, P, pre_counts, lvl, scene);
  const long sb = (long)scene * P.cap;
  NmsBlock at;                                         // the clamp keeps a position within the level's slots for any input
  if (!nms_stage_sorted<AABB>((int)blockIdx.x - pick4(P.blk0, lvl), tw, pre_boxes + sb * ROW, ROW, 0, order + sb + off, (long)off, (long)off + top - 1, nb, rows, cols, at)) return;
  nms_mask_tile<AABB>(rows, cols, at.r0, at.c0, at.j, nb, thr, mask + (long)scene * P.mtot + pick4(P.moff, lvl), tw, nullptr, nullptr);
}

// one workgroup per scene; t_k <= 16384 (256 words of removed-set)
__global__ __launch_bounds__(256) void rpn_post_nms_scan_kernel(RpnGeom G, RpnPostGeom P, int row_floats, const float* __restrict__ pre_boxes, const float* __restrict__ pre_scores,
                                                                const int* __restrict__ pre_index, const long* __restrict__ sorted_keys, const long* __restrict__ order,
                                                                const int* __restrict__ pre_counts, const unsigned long long* __restrict__ mask, int post_top_n, int* keep,
                                                                float* __restrict__ boxes, float* __restrict__ scores, int* __restrict__ levels, int* __restrict__ index,
                                                                int* __restrict__ counts) {
  __shared__ unsigned long long removed[256], diag[64];
  __shared__ int kept_n[4];
  const int t = threadIdx.x, scene = blockIdx.x;
  const long sb = (long)scene * P.cap;
  for (int lvl = 0; lvl < G.L; ++lvl) {    // uniform
    const int tw = pick4(P.tw, lvl), off = pick4(P.off, lvl);
    const int N = level_count(G, P, pre_counts, lvl, scene);
    const int cnt = nms_greedy_walk(mask + (long)scene * P.mtot + pick4(P.moff, lvl), tw, N, keep + sb + off, removed, diag);      // the same in every thread
    if (t == 0) kept_n[lvl] = cnt;
  }
  __syncthreads();                         // keep[] and kept_n[] are complete and visible to the workgroup
  int total = 0;
  for (int lvl = 0; lvl < G.L; ++lvl) total += kept_n[lvl];
  const int m = min(total, max(post_top_n, 0));
  // merge: rank in the global order (descending key, ties to the lower slot = the lower level, then the level's own order)
  for (int lvl = 0; lvl < G.L; ++lvl) {
    const int off = pick4(P.off, lvl), top = pick4(P.top, lvl);
    for (int j = t; j < kept_n[lvl]; j += 256) {
      const int pos = keep[sb + off + j];
      const unsigned key = (unsigned)(sorted_keys[sb + off + pos] & 0xffffffffl);
      int rank = j;
      for (int l2 = 0; l2 < G.L; ++l2) {
        if (l2 == lvl) continue;
        const int off2 = pick4(P.off, l2);
        int lo = 0, hi = kept_n[l2];       // the first entry of level l2 that does NOT come before this box
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          const unsigned k2 = (unsigned)(sorted_keys[sb + off2 + keep[sb + off2 + mid]] & 0xffffffffl);
          if (k2 > key || (k2 == key && l2 < lvl)) lo = mid + 1; else hi = mid;
        }
        rank += lo;
      }
      if (rank < m) {
        const long src = sb + sorted_slot(P, order, sb, off, top, pos), dst = sb + rank;
        for (int c = 0; c < row_floats; ++c) boxes[dst * row_floats + c] = pre_boxes[src * row_floats + c];
        scores[dst] = pre_scores[src];
        levels[dst] = lvl;
        index[dst] = pre_index[src];
      }
    }
  }
  for (int r = m + t; r < P.cap; r += 256) {
    for (int c = 0; c < row_floats; ++c) boxes[(sb + r) * row_floats + c] = 0.f;
    scores[sb + r] = 0.f;
    levels[sb + r] = 0;
    index[sb + r] = 0;
  }
  if (t == 0) counts[scene] = m;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
int make_post(const RpnGeom& G, int pre_top_n, const int* mesh, RpnPostGeom& P) {
  if (pre_top_n < 1) return -4;
  long cap = 0, moff = 0, blocks = 0;
  for (int k = 0; k < 4; ++k) {
    const int top = G.n[k] < pre_top_n ? G.n[k] : pre_top_n, tw = (top + 63) / 64;
    P.top[k] = top; P.off[k] = (int)cap; P.tw[k] = tw; P.moff[k] = moff; P.blk0[k] = (int)blocks;
    if (k < G.L) { cap += top; moff += (long)top * tw; blocks += (long)tw * (tw + 1) / 2; }
    if (cap > NMH_OBB_NMS_MAX) return -4;
  }
  P.cap = (int)cap; P.mtot = moff; P.mblocks = (int)blocks;
  for (int c = 0; c < 3; ++c) {
    P.mesh[c] = mesh ? mesh[c] : 0;
    if (mesh && (mesh[c] < 1 || mesh[c] >= (1 << 24))) return -4;
  }
  return 0;
}

}  // namespace

long k_rpn_post_cap(int nlevels, const int* dims, int N, int pre_top_n) {
  RpnGeom G;
  RpnPostGeom P;
  return (make_geom(nlevels, dims, N, G) || make_post(G, pre_top_n, nullptr, P)) ? -1 : P.cap;
}
long k_rpn_post_mask_words(int nlevels, const int* dims, int N, int pre_top_n) {
  RpnGeom G;
  RpnPostGeom P;
  return (make_geom(nlevels, dims, N, G) || make_post(G, pre_top_n, nullptr, P)) ? -1 : P.mtot * N;
}

int k_rpn_decode(int nlevels, const int* dims, const float* base, int N, int ncols, const float* const* reg, float* boxes, hipStream_t st) {
  RpnGeom G;
  RpnBase B;
  if (make_geom(nlevels, dims, N, G) || make_base(nlevels, dims, base, B) || (ncols != 6 && ncols != 8) || !all_set(nlevels, reg)) return -4;
  const Ptr4<const float> R = make_ptrs<const float>(nlevels, reg);
  if (ncols == 8) hipLaunchKernelGGL(rpn_decode_kernel<true>, dim3(G.nblocks), dim3(256), 0, st, G, B, R, boxes);
  else hipLaunchKernelGGL(rpn_decode_kernel<false>, dim3(G.nblocks), dim3(256), 0, st, G, B, R, boxes);
  NMH_CHECK_LAUNCH();
  return 0;
}

int k_rpn_post_select(int nlevels, const int* dims, const float* base, int N, int ncols, int pre_top_n, const float* const* obj, const float* const* reg, const int* ori,
                      const int* mesh, float score_thresh, float min_size, long* pre_keys, float* pre_boxes, float* pre_scores, int* pre_index, int* pre_counts, hipStream_t st) {
  RpnGeom G;
  RpnBase B;
  RpnPostGeom P;
  if (!mesh || make_geom(nlevels, dims, N, G) || make_base(nlevels, dims, base, B) || make_post(G, pre_top_n, mesh, P) || (ncols != 6 && ncols != 8)) return -4;
  if (!all_set(nlevels, obj) || !all_set(nlevels, reg)) return -4;
  const Ptr4<const float> O = make_ptrs<const float>(nlevels, obj), R = make_ptrs<const float>(nlevels, reg);
  const dim3 grid((unsigned)(nlevels * N));
  if (ncols == 8) hipLaunchKernelGGL(rpn_post_select_kernel<true>, grid, dim3(SEL_T), 0, st, G, B, P, O, R, ori, score_thresh, min_size, pre_keys, pre_boxes, pre_scores, pre_index, pre_counts);
  else hipLaunchKernelGGL(rpn_post_select_kernel<false>, grid, dim3(SEL_T), 0, st, G, B, P, O, R, ori, score_thresh, min_size, pre_keys, pre_boxes, pre_scores, pre_index, pre_counts);
  NMH_CHECK_LAUNCH();
  return 0;
}

int k_rpn_post_nms(int nlevels, const int* dims, int N, int ncols, int pre_top_n, const float* pre_boxes, const float* pre_scores, const int* pre_index, const long* sorted_keys,
                   const long* order, const int* pre_counts, float nms_thresh, int post_top_n, unsigned long long* mask, int* keep, float* boxes, float* scores, int* levels,
                   int* index, int* counts, hipStream_t st) {
  RpnGeom G;
  RpnPostGeom P;
  if (make_geom(nlevels, dims, N, G) || make_post(G, pre_top_n, nullptr, P) || (ncols != 6 && ncols != 8) || post_top_n < 1) return -4;
  const dim3 grid((unsigned)P.mblocks, (unsigned)N);
  if (ncols == 6) hipLaunchKernelGGL(rpn_post_nms_mask_kernel<true>, grid, dim3(256), 0, st, G, P, pre_boxes, order, pre_counts, nms_thresh, mask);
  else hipLaunchKernelGGL(rpn_post_nms_mask_kernel<false>, grid, dim3(256), 0, st, G, P, pre_boxes, order, pre_counts, nms_thresh, mask);
  NMH_CHECK_LAUNCH();
  hipLaunchKernelGGL(rpn_post_nms_scan_kernel, dim3((unsigned)N), dim3(256), 0, st, G, P, ncols == 6 ? 6 : 7, pre_boxes, pre_scores, pre_index, sorted_keys, order, pre_counts, mask,
                     post_top_n, keep, boxes, scores, levels, index, counts);
  NMH_CHECK_LAUNCH();
  return 0;
}

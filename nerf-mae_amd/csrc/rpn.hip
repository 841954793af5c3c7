// Training path of the reference's anchor-based 3-D RegionProposalNetwork, as gfx950 kernels:
//   rpn_gtmax / rpn_assign   assign_targets_to_anchors (nerf_rpn/model/rpn.py:240-290) over batched_box_iou / box_iou_3d (model/utils.py:371-458),
//                            Matcher(fg, bg, allow_low_quality_matches=True) (model/utils.py:98-211), obb2hbb_3d (coder/misc.py:85-93), the padding
//                            masks of AnchorGenerator3D.get_padding_masks (anchor.py:124-152) and the coders' encode: AABBCoder.encode_single
//                            (coder/AABB_coder.py:7-56) or MidpointOffsetCoder.encode_single / bbox2delta_sp (coder/midpoint_offset_coder.py:106-158);
//   rpn_sample               BalancedPositiveNegativeSampler (model/utils.py:35-95), with a counter-based hash in place of torch.randperm;
//   rpn_loss                 compute_loss (rpn.py:389-419): BCE-with-logits over the sampled anchors and smooth-L1 (beta 1/9) over the sampled
//                            positives, both divided by the number of sampled anchors; forward and backward.
// fp32 throughout; nothing goes to scratch; every kernel writes only its own outputs for any input; the host never waits.
//
// Anchors are never stored.  Level k has a grid (W, H, D), per-axis strides (sx, sy, sz) = mesh_size // grid, and A base anchors given by their half
// extents (hx, hy, hz): the reference's table is (-w, -h, -d, w, h, d) / 2 rounded half to even, which is symmetric.  Anchor i of the level,
// i = ((w H + h) D + d) A + a, is (w sx - hx, h sy - hy, d sz - hz, w sx + hx, h sy + hy, d sz + hz): centred at index * stride.  A scene's anchors
// are its levels concatenated, n = sum over k of W H D A; the dense index of (scene b, level k, anchor i) is b n + off_k + i.  Head outputs are read
// in place: objectness of level k is (N, A, W, H, D), element (b, a, loc) at (b A + a) nloc + loc; regression is (N, A C, W, H, D), channel a C + c.
//
// Assignment.  Ground-truth boxes are one [G_total][6|7] array, scene b owning rows off[b] .. off[b+1]-1, staged in LDS 64 at a time.  6 columns: the box;
// 7 columns (x, y, z, w, l, h, theta): the box obb2hbb_3d gives.  iou = inter / (vol_gt + vol_anchor - inter) in the reference's order of operations,
// without contraction, by ONE device function, so that the two passes see the same bits.  valid: with ori_sizes, index < ceil(ori / stride) on every
// axis; else always.
//   pass 1: gtmax[g] = max over the scene's valid anchors of iou, by a wave reduction, an LDS atomicMax per wave and one global atomicMax per
//           workgroup and box on the bit pattern (iou >= 0, so unsigned order is float order; a maximum does not depend on order);
//   pass 2: best, arg = max over the scene's boxes, ties to the lowest index (DEFINED here; torch.max leaves it open);
//           m = arg if best >= fg, -1 if best < bg, else -2;  if iou(anchor, g) == gtmax[g] for some g (bitwise): m = arg (the low-quality restore;
//           a box that no valid anchor touches has gtmax 0 and restores every valid anchor that does not touch it, as the reference does);
//           label = 1 if m >= 0, 0 if m == -1, -1 if m == -2;  not valid: m = -1, label = -1;  a scene without boxes: m = -1, label = 0 (-1 if not valid),
//           targets 0;  else targets = encode(box max(m, 0), anchor).
// Sampling.  One workgroup of 1024 lanes per scene.  Candidates: label >= 1 (positive) and label == 0 (negative).  num_pos = min(#pos, want_pos),
// num_neg = min(#neg, batch - num_pos).  Every candidate has the key hash(seed, counter, scene, index), recomputed wherever it is needed; the num_*
// smallest keys of a class are taken, found by the radix select of select_scan.hpp over the complemented key; equal keys at the cut go to the lower
// anchor index.  flags: 0 unsampled, 1 positive, 2 negative.  A second launch of one lane adds 1 to the counter.
// Loss.  One lane per head element (b, a, loc), so the dense gradients are written coalesced.  s = number of flags != 0 over all scenes;
//   objectness = sum over flags != 0 of bce_with_logits(x, flag == 1) / s;  box_reg = sum over flags == 1 and c of smooth_l1(pred - target; 1/9) / s;
//   both 0 when s == 0 (the reference gives NaN there).  Forward: per-workgroup partial sums, then a fixed-order pass of one workgroup.  Backward: one
//   pass that writes every element of both gradients, exactly 0 where flag == 0.
//   One forward and one backward kernel template, rpn_loss_fwd_kernel / rpn_loss_bwd_kernel<TERM, P2D>, over the five box terms (smooth-L1 with 6 or 8 columns,
//   iou / linear_iou, giou, diou) and the 2-D projection term as a compile-time flag, and one final kernel over 3 or 5 sums.  What the variants do not share is
//   under `if constexpr`: the instantiations without the flag are the kernels without the term (smooth-L1: no base table in LDS, no barrier, three sums), and the
//   eight nmh_rpn_*loss* entries of the C ABI forward to one launcher pair.
// IoU-type box losses (nmh_rpn_iou_loss: RotatedIOULoss over the decoded proposals, rpn.py:133-164, 214-217, 400-417, 518-520; 8 columns only).  The same
//   lane map, sums and objectness; the box term of a lane with flag == 1 is taken between A = rpn_decode_obb(its 8 deltas, its anchor) and B = the scene's
//   box row max(matched_idxs, 0), both (x, y, z, w, l, h, theta):  iou -log((inter3d + 1) / (u3d + 1)), linear_iou 1 - that ratio, giou / diou
//   obb_pair_loss<OBB_GIOU_SMALLEST | OBB_DIOU_SMALLEST> (obb_geom.hpp), summed and divided by s.  Only flagged positives decode (the reference decodes
//   every anchor and reads the sampled ones): a wave without one skips the geometry.  A flagged positive whose scene has no box row for it, or that
//   lies in the padding (either is possible only with flags that the sampler did not draw), contributes 0 and has zero box gradient.  Backward:
//   g_reg / s through obb_pair_grad (box A only) and rpn_decode_obb_bwd (rpn_decode.hpp); every element of both gradients is written, dreg exactly 0
//   where flag != 1.
// 2-D projection term (nmh_rpn_loss2d, nmh_rpn_iou_loss2d: the third return of compute_loss, rpn.py:421-453), opt-in, for every box loss above and both box kinds.
//   The same lane map and the same first two sums; a lane with flag == 1 adds T (proj2d.hpp) between the UNCLIPPED decode of its deltas (rpn_decode_aabb /
//   rpn_decode_obb) and its matched box row, under the cameras of res = max(mesh_size).  P = number of flags == 1;  loss_2d = sum T / P / res, 0 when P == 0
//   (the reference gives NaN).  A flagged positive without a box row or in the padding counts in P and contributes 0 to the 2-D sum and, under the IoU types,
//   to the box sum; under smooth-L1 it still adds its smooth-L1 term, which needs no box row.  scalars =
//   (objectness, box, sampled anchors, 2-D, P).  Backward: one pass, g_2d / P / res through proj2d_term_grad and the decode's backward, added to the box
//   term's gradient in registers, so that every element of both gradients is still written exactly once.
#include "common.hpp"
#include "kernels.hpp"
#include "select_scan.hpp"
#include "reduce_fixed.hpp"
#include "rpn_geom.hpp"
#include "rpn_shared.hpp"
#include "rpn_decode.hpp"
#include "proj2d.hpp"
#include <type_traits>

namespace {

constexpr int RPN_CHUNK = 64;
struct RpnOffs { int off[NMH_FCOS_MAX_SCENES + 1]; };   // kernel argument, by value: scene b owns box rows off[b] .. off[b+1]-1; the entries past N repeat off[N]
// offs: HOST [N+1], starting at 0 and not descending (else -4)
int make_offs(int N, const int* offs, RpnOffs& S) {
  if (!offs || offs[0] != 0) return -4;
  for (int b = 0; b < N; ++b) if (offs[b + 1] < offs[b]) return -4;
  for (int b = 0; b <= NMH_FCOS_MAX_SCENES; ++b) S.off[b] = offs[b < N ? b : N];
  return 0;
}

template <bool ORIENTED>
__device__ __forceinline__ Box6 rpn_gt(const float* __restrict__ b) {
  Box6 g;
  if (ORIENTED) {
    const float cs = cosf(b[6]), sn = sinf(b[6]);
    const float bx = fabsf(b[3] / 2.f * cs) + fabsf(b[4] / 2.f * sn), by = fabsf(b[3] / 2.f * sn) + fabsf(b[4] / 2.f * cs), bz = b[5] / 2.f;
    g.x0 = b[0] - bx; g.y0 = b[1] - by; g.z0 = b[2] - bz; g.x1 = b[0] + bx; g.y1 = b[1] + by; g.z1 = b[2] + bz;
  } else {
    g.x0 = b[0]; g.y0 = b[1]; g.z0 = b[2]; g.x1 = b[3]; g.y1 = b[4]; g.z1 = b[5];
  }
  g.vol = (g.x1 - g.x0) * (g.y1 - g.y0) * (g.z1 - g.z0);
  return g;
}

// ---- assignment ------------------------------------------------------------------------------------------------------------------------
template <bool ORIENTED>
__global__ __launch_bounds__(256) void rpn_gtmax_kernel(RpnGeom G, RpnBase B, RpnOffs S, const float* __restrict__ boxes, const int* __restrict__ ori, unsigned* __restrict__ gtmax) {
  __shared__ Box6 sb[RPN_CHUNK];
  __shared__ unsigned smax[RPN_CHUNK];
  __shared__ float sh_base[RPN_MAX_A * 3];
  const RAt q = rpn_where(G);
  const int t = threadIdx.x;
  rpn_stage_base(B, q.lvl, pick4(G.A, q.lvl), sh_base);
  __syncthreads();
  bool valid;
  const Box6 a = rpn_anchor(G, sh_base, ori, q, valid);
  const int g0 = S.off[q.scene], g1 = S.off[q.scene + 1];
  for (int c = g0; c < g1; c += RPN_CHUNK) {         // uniform over the workgroup
    __syncthreads();
    if (t < RPN_CHUNK) {
      smax[t] = 0u;
      if (c + t < g1) sb[t] = rpn_gt<ORIENTED>(boxes + (long)(c + t) * (ORIENTED ? 7 : 6));
    }
    __syncthreads();
    const int m = min(RPN_CHUNK, g1 - c);
    for (int k = 0; k < m; ++k) {                    // every lane, so that the shuffles converge
      unsigned bits = valid ? __float_as_uint(rpn_iou(sb[k], a)) : 0u;
      if (__any(bits != 0u)) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) bits = max(bits, (unsigned)__shfl_xor((int)bits, o, 64));
        if ((t & 63) == 0) atomicMax(&smax[k], bits);
      }
    }
    __syncthreads();
    if (t < m && smax[t] != 0u) atomicMax(&gtmax[c + t], smax[t]);
  }
}

// bbox2delta_sp: ga = the largest corner x among the corners within 0.1 of the lowest y (others count as -1000), gb likewise for y at the largest x
__device__ __forceinline__ void rpn_encode_obb(const float* __restrict__ g, const Box6& a, float (&o)[8]) {
  const float px = (a.x0 + a.x1) * 0.5f, py = (a.y0 + a.y1) * 0.5f, pz = (a.z0 + a.z1) * 0.5f;
  const float pw = a.x1 - a.x0, ph = a.y1 - a.y0, pd = a.z1 - a.z0;
  const float x = g[0], y = g[1], w = g[3], h = g[4], cs = cosf(g[6]), sn = sinf(g[6]);
  const float bx = fabsf(w / 2.f * cs) + fabsf(h / 2.f * sn), by = fabsf(w / 2.f * sn) + fabsf(h / 2.f * cs);
  const float hx0 = x - bx, hy0 = y - by, hx1 = x + bx, hy1 = y + by;
  const float gx = (hx0 + hx1) * 0.5f, gy = (hy0 + hy1) * 0.5f, gw = hx1 - hx0, gh = hy1 - hy0;
  const float v1x = w / 2.f * cs, v1y = -w / 2.f * sn, v2x = -h / 2.f * sn, v2y = -h / 2.f * cs;
  const float X[4] = {x + v1x + v2x, x + v1x - v2x, x - v1x - v2x, x - v1x + v2x}, Y[4] = {y + v1y + v2y, y + v1y - v2y, y - v1y - v2y, y - v1y + v2y};
  const float ymin = fminf(fminf(Y[0], Y[1]), fminf(Y[2], Y[3])), xmax = fmaxf(fmaxf(X[0], X[1]), fmaxf(X[2], X[3]));
  float ga = -3.0e38f, gb = -3.0e38f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    ga = fmaxf(ga, fabsf(Y[k] - ymin) > 0.1f ? -1000.f : X[k]);
    gb = fmaxf(gb, fabsf(X[k] - xmax) > 0.1f ? -1000.f : Y[k]);
  }
  o[0] = (gx - px) / pw; o[1] = (gy - py) / ph; o[2] = (g[2] - pz) / pd;
  o[3] = logf(gw / pw); o[4] = logf(gh / ph); o[5] = logf(g[5] / pd);
  o[6] = (ga - gx) / gw; o[7] = (gb - gy) / gh;
}

template <bool ORIENTED>
__global__ __launch_bounds__(256) void rpn_assign_kernel(RpnGeom G, RpnBase B, RpnOffs S, const float* __restrict__ boxes, const int* __restrict__ ori, const unsigned* __restrict__ gtmax,
                                                         float fg, float bg, float* __restrict__ labels, int* __restrict__ midx, float* __restrict__ targets) {
  constexpr int C = ORIENTED ? 8 : 6, NC = ORIENTED ? 7 : 6;
  __shared__ Box6 sb[RPN_CHUNK];
  __shared__ unsigned sm[RPN_CHUNK];
  __shared__ float sh_base[RPN_MAX_A * 3];
  const RAt q = rpn_where(G);
  const int t = threadIdx.x;
  rpn_stage_base(B, q.lvl, pick4(G.A, q.lvl), sh_base);
  __syncthreads();
  bool valid;
  const Box6 a = rpn_anchor(G, sh_base, ori, q, valid);
  const int g0 = S.off[q.scene], g1 = S.off[q.scene + 1];
  float best = -1.f;
  int bi = 0;
  bool restore = false;
  for (int c = g0; c < g1; c += RPN_CHUNK) {         // uniform over the workgroup
    __syncthreads();
    if (t < RPN_CHUNK && c + t < g1) {
      sb[t] = rpn_gt<ORIENTED>(boxes + (long)(c + t) * NC);
      sm[t] = gtmax[c + t];
    }
    __syncthreads();
    const int m = min(RPN_CHUNK, g1 - c);
    if (valid) {
      for (int k = 0; k < m; ++k) {
        const float iou = rpn_iou(sb[k], a);
        if (iou > best) { best = iou; bi = c + k - g0; }
        restore = restore || __float_as_uint(iou) == sm[k];
      }
    }
  }
  if (!q.active) return;
  const long p = (long)q.scene * G.ntot + pick4(G.off, q.lvl) + q.i;
  float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int m = -1;
  float lab = valid ? 0.f : -1.f;
  if (g1 > g0) {
    if (valid) {
      m = best >= fg ? bi : (best < bg ? -1 : -2);
      if (restore) m = bi;
      lab = m >= 0 ? 1.f : (m == -1 ? 0.f : -1.f);
    }
    const float* __restrict__ g = boxes + (long)(g0 + max(m, 0)) * NC;
    if (ORIENTED) rpn_encode_obb(g, a, o);
    else rpn_encode_aabb(g, a, o);
  }
  labels[p] = lab;
  midx[p] = m;
#pragma unroll
  for (int k = 0; k < C; ++k) targets[p * C + k] = o[k];
}

// ---- sampling ----------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int rpn_class(float label) { return label >= 1.f ? 0 : (label == 0.f ? 1 : -1); }

enum { SEL_NONE = 0, SEL_ALL = 1, SEL_CUT = 2 };

__global__ __launch_bounds__(SEL_T) void rpn_sample_kernel(const float* __restrict__ labels, int n, int batch, int want_pos, const long* __restrict__ rng, unsigned char* __restrict__ flags,
                                                           int* __restrict__ counts) {
  __shared__ int hist[2][2048];
  __shared__ int wsum[SEL_T / 64];
  __shared__ int sh[2];
  const int t = threadIdx.x, scene = blockIdx.x;
  const float* __restrict__ lab = labels + (long)scene * n;
  unsigned char* __restrict__ fl = flags + (long)scene * n;
  const unsigned long long stream = rpn_stream(rng[0], rng[1], scene);

  // pass 0: the candidates of both classes and the histograms of the top 11 bits
  hist[1][t] = 0; hist[1][t + SEL_T] = 0;
  hist_clear(hist[0]);
  int mine[2] = {0, 0};
  for (int q = t; q < n; q += SEL_T) {
    const int c = rpn_class(lab[q]);
    if (c >= 0) {
      atomicAdd(&hist[c][rpn_key(stream, q) >> 21], 1);
      if (c == 0) ++mine[0]; else ++mine[1];
    }
  }
  int have[2];
  block_scan_excl(mine[0], have[0], wsum);           // its barriers also complete hist
  block_scan_excl(mine[1], have[1], wsum);
  int num[2];
  num[0] = min(have[0], max(want_pos, 0));
  num[1] = min(have[1], max(batch - num[0], 0));

  // per class: take key > K, and need_eq of the eq_have keys == K (the lowest indices)
  int mode[2];
  unsigned K[2] = {0u, 0u};
  int need_eq[2] = {0, 0}, eq_have[2] = {0, 0};
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    mode[c] = num[c] == 0 ? SEL_NONE : (num[c] >= have[c] ? SEL_ALL : SEL_CUT);
    if (mode[c] != SEL_CUT) continue;                // uniform
    const RadixCut cut = radix_select_rest(hist[c], wsum, sh, num[c], n, [&](int q, unsigned& key) {
      if (rpn_class(lab[q]) != c) return false;
      key = rpn_key(stream, q);
      return true;
    });
    K[c] = cut.K; need_eq[c] = cut.need_eq;
    eq_have[c] = hist[c][1024 + (cut.K & 1023u)];     // the last histogram is left in place
  }

  // flags; only a tie at a cut that is not taken whole needs the order of the indices
  const bool ordered0 = mode[0] == SEL_CUT && need_eq[0] < eq_have[0], ordered1 = mode[1] == SEL_CUT && need_eq[1] < eq_have[1];
  int run0 = 0, run1 = 0;
  for (int base = 0; base < n; base += SEL_T) {      // uniform
    const int q = base + t;
    const int c = q < n ? rpn_class(lab[q]) : -1;
    const unsigned key = c >= 0 ? rpn_key(stream, q) : 0u;
    const int md = c == 0 ? mode[0] : (c == 1 ? mode[1] : SEL_NONE);
    const unsigned Kc = c == 0 ? K[0] : K[1];
    const bool eq = md == SEL_CUT && key == Kc;
    bool sel = md == SEL_ALL || (md == SEL_CUT && key > Kc);
    sel = ordered0 ? tie_take(sel, eq && c == 0, need_eq[0], run0, wsum) : sel || (eq && c == 0);       // uniform
    sel = ordered1 ? tie_take(sel, eq && c == 1, need_eq[1], run1, wsum) : sel || (eq && c == 1);       // uniform
    if (q < n) fl[q] = sel ? (unsigned char)(c == 0 ? 1 : 2) : (unsigned char)0;
  }
  if (t == 0) { counts[scene * 2] = num[0]; counts[scene * 2 + 1] = num[1]; }
}

// ---- losses ------------------------------------------------------------------------------------------------------------------------------
// head order: lane j of (level, scene) is head element (a, loc) = (j / nloc, j % nloc), anchor i = loc A + a
struct RHead { int lvl, scene, j, a, loc, nloc, A; long p; bool active; };
__device__ __forceinline__ RHead rpn_head_where(const RpnGeom& G) {
  const RAt q = rpn_where(G);
  RHead r;
  r.lvl = q.lvl; r.scene = q.scene; r.j = q.i; r.active = q.active;
  r.nloc = pick4(G.nloc, q.lvl); r.A = pick4(G.A, q.lvl);
  const int j = q.active ? q.i : 0;
  r.a = j / r.nloc; r.loc = j - r.a * r.nloc;
  r.p = (long)q.scene * G.ntot + pick4(G.off, q.lvl) + (long)r.loc * r.A + r.a;
  return r;
}

// TERM: what the box loss is.  Smooth-L1 on the encoded targets (6 or 8 columns), or an IoU type between the decoded proposal and the matched box row (8 columns).
enum { RPN_BOX_SL1_AABB = 0, RPN_BOX_SL1_OBB = 1, RPN_BOX_IOU = 2, RPN_BOX_GIOU = 3, RPN_BOX_DIOU = 4 };
template <int TERM> struct Rpn2d {
  static constexpr bool ORIENTED = TERM != RPN_BOX_SL1_AABB, SL1 = TERM <= RPN_BOX_SL1_OBB;
  static constexpr int C = ORIENTED ? 8 : 6, NC = ORIENTED ? 7 : 6;
  static constexpr int MODE = TERM == RPN_BOX_GIOU ? OBB_GIOU_SMALLEST : (TERM == RPN_BOX_DIOU ? OBB_DIOU_SMALLEST : OBB_IOU);
};

// the IoU-type box term of one flagged positive and its gradient over the 8 deltas: A = the decode of the anchor's deltas, B = the matched box row
template <int MODE>
__device__ __forceinline__ float rpn_iou_term(const float (&r)[8], const Box6& a, const float* __restrict__ b, int linear) {
  float o[7];
  rpn_decode_obb(r, a, o);
  const Obb A = obb_load(o), B = obb_load(b);
  const PairOut p = obb_pair(A, B);
  if (MODE == OBB_IOU) {
    const float q = (p.inter3d + 1.f) / (p.u3d + 1.f);
    return linear ? 1.f - q : -logf(q);
  }
  float X[8], Y[8];
  obb_corners(A, X, Y, 0);
  obb_corners(B, X, Y, 4);
  Encl E;
  return obb_pair_loss<MODE>(A, B, p, X, Y, E);
}
template <int MODE>
__device__ __forceinline__ void rpn_iou_term_grad(const float (&r)[8], const Box6& a, const float* __restrict__ b, int linear, float (&gr)[8]) {
  float o[7];
  rpn_decode_obb(r, a, o);
  const Obb A = obb_load(o), B = obb_load(b);
  BoxGrad ga, gb;
  if (MODE == OBB_IOU) {
    const PairOut p = obb_pair(A, B);
    const float u1 = p.u3d + 1.f, q = (p.inter3d + 1.f) / u1, gq = linear ? -1.f : -1.f / q;
    obb_pair_grad<OBB_IOU>(A, B, gq * p.u3d / u1, gq * (p.iou - 1.f) / (u1 * u1), 0.f, false, ga, gb);
  } else {
    obb_pair_grad<MODE>(A, B, 0.f, 0.f, 1.f, false, ga, gb);
  }
  rpn_decode_obb_bwd(r, a, ga, gr);
}

// what a flagged positive needs beyond its head values: its anchor, and its box row of NC columns (NULL: it contributes nothing)
template <int NC>
__device__ __forceinline__ const float* rpn_pair(const RpnGeom& G, const float* __restrict__ sh_base, const RpnOffs& S, const RHead& w, const float* __restrict__ boxes,
                                                 const int* __restrict__ ori, const int* __restrict__ midx, Box6& a) {
  bool valid;
  a = rpn_anchor(G, sh_base, ori, RAt{w.lvl, w.scene, w.loc * w.A + w.a, true}, valid);
  const int g0 = S.off[w.scene], g1 = S.off[w.scene + 1], row = g0 + max(midx[w.p], 0);
  return valid && row < g1 ? boxes + (long)row * NC : nullptr;
}

// T between the unclipped decode of the deltas and the box row b, and its gradient over the deltas
template <bool ORIENTED>
__device__ __forceinline__ float rpn_2d_term(const float (&r)[8], const Box6& a, const float* __restrict__ b, const Proj2dCams& cams) {
  float o[7];
  if (ORIENTED) {
    rpn_decode_obb(r, a, o);
    return proj2d_term(obb_load(o), obb_load(b), cams);
  }
  rpn_decode_aabb(r, a, o);
  const float p[6] = {o[0], o[1], o[2], o[3], o[4], o[5]}, t[6] = {b[0], b[1], b[2], b[3], b[4], b[5]};
  return proj2d_term(p, t, cams);
}
template <bool ORIENTED>
__device__ __forceinline__ void rpn_2d_term_grad(const float (&r)[8], const Box6& a, const float* __restrict__ b, const Proj2dCams& cams, float (&gr)[8]) {
  float o[7];
  if (ORIENTED) {
    rpn_decode_obb(r, a, o);
    BoxGrad g;
    proj2d_term_grad(obb_load(o), obb_load(b), cams, g);
    rpn_decode_obb_bwd(r, a, g, gr);
  } else {
    rpn_decode_aabb(r, a, o);
    const float p[6] = {o[0], o[1], o[2], o[3], o[4], o[5]}, t[6] = {b[0], b[1], b[2], b[3], b[4], b[5]};
    float g[6];
    proj2d_term_grad(p, t, cams, g);
    rpn_decode_aabb_bwd(r, a, g, gr);
  }
}

// One forward and one backward kernel over (box term, with or without the 2-D term).  PAIR: a flagged positive looks up its anchor and its box row, which
// smooth-L1 without the 2-D term never does: that instantiation stages no base table and has no barrier before the loss.  Every instantiation takes the same
// arguments; what a variant does not read (B, S, boxes, midx, linear without PAIR; targets of the IoU types; cams, res, g_2d without the term) rides along unread.
// LATE: the IoU types without the term read their deltas (the backward also its scale) only once the lane has a box row; every other variant reads them before the
// lookup.  That is not an optimisation: it keeps every instantiation on the bits it has always produced.  The backward of the decode and of the pair geometry is
// free to contract, and where the compiler forms the fused multiply-adds moves with the position of these reads (with one position for all variants the IoU types'
// box gradients changed in their last bits).
template <int TERM, bool P2D>
__global__ __launch_bounds__(256) void rpn_loss_fwd_kernel(RpnGeom G, RpnBase B, RpnOffs S, Ptr4<const float> obj, Ptr4<const float> reg, const unsigned char* __restrict__ flags,
                                                           const float* __restrict__ targets, const float* __restrict__ boxes, const int* __restrict__ ori,
                                                           const int* __restrict__ midx, int linear, Proj2dCams cams, float* __restrict__ partials) {
  using K = Rpn2d<TERM>;
  constexpr int C = K::C, NS = P2D ? 5 : 3;
  constexpr bool PAIR = P2D || !K::SL1, LATE = !P2D && !K::SL1;
  __shared__ float sh_base[RPN_MAX_A * 3];
  const RHead w = rpn_head_where(G);
  if constexpr (PAIR) {
    rpn_stage_base(B, w.lvl, w.A, sh_base);
    __syncthreads();
  }
  float v[NS] = {};                     // objectness, box regression, sampled anchors; with the term: 2-D projection, sampled positives
  const int f = w.active ? flags[w.p] : 0;
  if (f != 0) {
    const float x = pick4(obj.p, w.lvl)[(long)w.scene * w.A * w.nloc + w.j];
    v[0] = fmaxf(x, 0.f) - (f == 1 ? x : 0.f) + log1pf(expf(-fabsf(x)));
    v[2] = 1.f;
    if (f == 1) {                       // a wave without a flagged positive skips this
      if constexpr (P2D) v[4] = 1.f;
      float r[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if constexpr (!LATE) {
        const float* __restrict__ rp = pick4(reg.p, w.lvl) + ((long)w.scene * w.A + w.a) * C * w.nloc + w.loc;
#pragma unroll
        for (int k = 0; k < C; ++k) r[k] = rp[(long)k * w.nloc];
      }
      if constexpr (K::SL1) {
#pragma unroll
        for (int k = 0; k < C; ++k) v[1] += rpn_sl1(r[k] - targets[w.p * C + k]);
      }
      if constexpr (PAIR) {
        Box6 a;
        const float* __restrict__ b = rpn_pair<K::NC>(G, sh_base, S, w, boxes, ori, midx, a);
        if (b) {
          if constexpr (LATE) {
            const float* __restrict__ rp = pick4(reg.p, w.lvl) + ((long)w.scene * w.A + w.a) * C * w.nloc + w.loc;
#pragma unroll
            for (int k = 0; k < C; ++k) r[k] = rp[(long)k * w.nloc];
          }
          if constexpr (!K::SL1) v[1] = rpn_iou_term<K::MODE>(r, a, b, linear);
          if constexpr (P2D) v[3] = rpn_2d_term<K::ORIENTED>(r, a, b, cams);
        }
      }
    }
  }
  block_sum_fixed(v, partials + NS * (long)blockIdx.x);
}

// one workgroup: fixed-order sum of the per-workgroup partials -> scalars = (objectness loss, box loss, number of sampled anchors); NS 5, with the 2-D term:
// also (2-D loss, number of sampled positives)
template <int NS>
__global__ __launch_bounds__(256) void rpn_loss_final_kernel(const float* __restrict__ partials, int nblocks, float res, float* __restrict__ scalars) {
  float sum[NS];
  final_sum_fixed(partials, nblocks, sum);
  if (threadIdx.x != 0) return;
  const float cnt = sum[2];
  scalars[0] = cnt > 0.f ? sum[0] / cnt : 0.f;
  scalars[1] = cnt > 0.f ? sum[1] / cnt : 0.f;
  scalars[2] = cnt;
  if constexpr (NS == 5) {
    const float pos = sum[4];
    scalars[3] = pos > 0.f ? sum[3] / pos / res : 0.f;
    scalars[4] = pos;
  }
}

template <int TERM, bool P2D>
__global__ __launch_bounds__(256) void rpn_loss_bwd_kernel(RpnGeom G, RpnBase B, RpnOffs S, Ptr4<const float> obj, Ptr4<const float> reg, const unsigned char* __restrict__ flags,
                                                           const float* __restrict__ targets, const float* __restrict__ boxes, const int* __restrict__ ori,
                                                           const int* __restrict__ midx, int linear, Proj2dCams cams, float res, const float* __restrict__ scalars,
                                                           const float* __restrict__ g_obj, const float* __restrict__ g_reg, const float* __restrict__ g_2d, Ptr4<float> dobj,
                                                           Ptr4<float> dreg) {
  using K = Rpn2d<TERM>;
  constexpr int C = K::C;
  constexpr bool PAIR = P2D || !K::SL1, LATE = !P2D && !K::SL1;
  __shared__ float sh_base[RPN_MAX_A * 3];
  const RHead w = rpn_head_where(G);
  if constexpr (PAIR) {
    rpn_stage_base(B, w.lvl, w.A, sh_base);
    __syncthreads();
  }
  if (!w.active) return;
  const long at = (long)w.scene * w.A * w.nloc + w.j, rat = ((long)w.scene * w.A + w.a) * C * w.nloc + w.loc;
  const int f = flags[w.p];
  const float cnt = scalars[2], pos = P2D ? scalars[4] : 0.f;
  float go = 0.f, gr[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (f != 0 && cnt > 0.f) {
    const float x = pick4(obj.p, w.lvl)[at];
    go = (sigmoid_stable(x) - (f == 1 ? 1.f : 0.f)) * (g_obj ? g_obj[0] : 0.f) / cnt;
    if (f == 1) {                       // a wave without a flagged positive skips this
      float sc = 0.f, sc2 = 0.f, r[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if constexpr (!LATE) {
        const float* __restrict__ rp = pick4(reg.p, w.lvl) + rat;
        sc = (g_reg ? g_reg[0] : 0.f) / cnt;
        if constexpr (P2D) sc2 = (g_2d ? g_2d[0] : 0.f) / pos / res;
#pragma unroll
        for (int k = 0; k < C; ++k) r[k] = rp[(long)k * w.nloc];
      }
      if constexpr (K::SL1) {
#pragma unroll
        for (int k = 0; k < C; ++k) gr[k] = rpn_sl1_grad(r[k] - targets[w.p * C + k]) * sc;
      }
      if constexpr (PAIR) {
        Box6 a;
        const float* __restrict__ b = rpn_pair<K::NC>(G, sh_base, S, w, boxes, ori, midx, a);
        if (b) {
          float g2[8];
          if constexpr (LATE) {
            const float* __restrict__ rp = pick4(reg.p, w.lvl) + rat;
            sc = (g_reg ? g_reg[0] : 0.f) / cnt;
#pragma unroll
            for (int k = 0; k < C; ++k) r[k] = rp[(long)k * w.nloc];
          }
          if constexpr (!K::SL1) {
            rpn_iou_term_grad<K::MODE>(r, a, b, linear, g2);
#pragma unroll
            for (int k = 0; k < 8; ++k) gr[k] = g2[k] * sc;
          }
          if constexpr (P2D) {
            rpn_2d_term_grad<K::ORIENTED>(r, a, b, cams, g2);
#pragma unroll
            for (int k = 0; k < 8; ++k) gr[k] += g2[k] * sc2;
          }
        }
      }
    }
  }
  pick4(dobj.p, w.lvl)[at] = go;
  float* __restrict__ dp = pick4(dreg.p, w.lvl) + rat;
#pragma unroll
  for (int k = 0; k < C; ++k) dp[(long)k * w.nloc] = gr[k];
}

}  // namespace

long k_rpn_num_blocks(int nlevels, const int* dims, int N) {
  RpnGeom G;
  return make_geom(nlevels, dims, N, G) ? -1 : G.nblocks;
}

int k_rpn_assign(int nlevels, const int* dims, const float* base, int N, int ncols, const float* boxes, const int* offs, const int* ori, float fg, float bg, unsigned* gtmax,
                 float* labels, int* midx, float* targets, hipStream_t st) {
  RpnGeom G;
  RpnBase B;
  RpnOffs S;
  if (make_geom(nlevels, dims, N, G) || make_base(nlevels, dims, base, B) || (ncols != 6 && ncols != 7) || make_offs(N, offs, S) || !(bg <= fg)) return -4;
  const int total = offs[N];
  if (total > 0 && (!boxes || !gtmax)) return -4;
  if (total > 0) {
    const int rc = k_fill_f32((float*)gtmax, 0.f, total, st);        // an unsigned 0 has the bits of 0.f
    if (rc) return rc;
    if (ncols == 7) hipLaunchKernelGGL(rpn_gtmax_kernel<true>, dim3(G.nblocks), dim3(256), 0, st, G, B, S, boxes, ori, gtmax);
    else hipLaunchKernelGGL(rpn_gtmax_kernel<false>, dim3(G.nblocks), dim3(256), 0, st, G, B, S, boxes, ori, gtmax);
    NMH_CHECK_LAUNCH();
  }
  if (ncols == 7) hipLaunchKernelGGL(rpn_assign_kernel<true>, dim3(G.nblocks), dim3(256), 0, st, G, B, S, boxes, ori, gtmax, fg, bg, labels, midx, targets);
  else hipLaunchKernelGGL(rpn_assign_kernel<false>, dim3(G.nblocks), dim3(256), 0, st, G, B, S, boxes, ori, gtmax, fg, bg, labels, midx, targets);
  NMH_CHECK_LAUNCH();
  return 0;
}

int k_rpn_sample(int N, long n, const float* labels, int batch, int want_pos, long* rng, unsigned char* flags, int* counts, hipStream_t st) {
  if (N < 1 || N > NMH_FCOS_MAX_SCENES || n < 1 || n > (1L << 30) || batch < 0 || want_pos < 0) return -4;
  hipLaunchKernelGGL(rpn_sample_kernel, dim3(N), dim3(SEL_T), 0, st, labels, (int)n, batch, want_pos, rng, flags, counts);
  NMH_CHECK_LAUNCH();
  hipLaunchKernelGGL(rpn_rng_advance_kernel, dim3(1), dim3(64), 0, st, rng);
  NMH_CHECK_LAUNCH();
  return 0;
}

namespace {
struct RpnLossArgs {             // the by-value arguments of the loss kernels
  RpnGeom G;
  RpnBase B;
  RpnOffs S;
  Ptr4<const float> obj, reg;
  Proj2dCams cams;
};
// loss_type < 0: smooth-L1 on the encoded targets (ncols 6 | 8); else 0 iou, 1 linear_iou, 2 giou, 3 diou (ncols 8 only)
int term_of(int ncols, int loss_type) {
  if (loss_type < 0) return ncols == 6 ? RPN_BOX_SL1_AABB : (ncols == 8 ? RPN_BOX_SL1_OBB : -1);
  return ncols != 8 || loss_type > 3 ? -1 : (loss_type <= 1 ? RPN_BOX_IOU : (loss_type == 2 ? RPN_BOX_GIOU : RPN_BOX_DIOU));
}

// the by-value arguments of both loss kernels and the box term; cams NULL: without the 2-D term.  Smooth-L1 needs targets; the IoU types and the 2-D term need
// what the box-row lookup reads (base, offs, midx, and boxes if there is a row); the 2-D term needs res > 0.
int make_loss_args(int nlevels, const int* dims, const float* base, int N, int ncols, int loss_type, const float* const* obj, const float* const* reg, const float* targets,
                   const float* boxes, const int* offs, const int* midx, const float* cams, float res, RpnLossArgs& q, int& term) {
  term = term_of(ncols, loss_type);
  if (term < 0 || make_geom(nlevels, dims, N, q.G) || !all_set(nlevels, obj) || !all_set(nlevels, reg)) return -4;
  const bool sl1 = term <= RPN_BOX_SL1_OBB;
  if (sl1 && !targets) return -4;
  if ((!sl1 || cams) && (make_base(nlevels, dims, base, q.B) || make_offs(N, offs, q.S) || !midx || (offs[N] > 0 && !boxes))) return -4;
  if (cams) {
    if (!(res > 0.f)) return -4;
    for (int k = 0; k < 48; ++k) q.cams.m[k / 12][k % 12] = cams[k];
  }
  q.obj = make_ptrs<const float>(nlevels, obj); q.reg = make_ptrs<const float>(nlevels, reg);
  return 0;
}

// (term, with the 2-D term or not) -> launch(the two as compile-time constants)
template <typename F> void loss_dispatch(int term, bool p2d, F&& launch) {
  auto both = [&](auto T) {
    if (p2d) launch(T, std::true_type{});
    else launch(T, std::false_type{});
  };
  switch (term) {
    case RPN_BOX_SL1_AABB: both(std::integral_constant<int, RPN_BOX_SL1_AABB>{}); break;
    case RPN_BOX_SL1_OBB: both(std::integral_constant<int, RPN_BOX_SL1_OBB>{}); break;
    case RPN_BOX_IOU: both(std::integral_constant<int, RPN_BOX_IOU>{}); break;
    case RPN_BOX_GIOU: both(std::integral_constant<int, RPN_BOX_GIOU>{}); break;
    default: both(std::integral_constant<int, RPN_BOX_DIOU>{}); break;
  }
}
}  // namespace

int k_rpn_loss_fwd(int nlevels, const int* dims, const float* base, int N, int ncols, int loss_type, const float* const* obj, const float* const* reg, const unsigned char* flags,
                   const float* targets, const float* boxes, const int* offs, const int* ori, const int* midx, const float* cams, float res, float* partials, float* scalars,
                   hipStream_t st) {
  RpnLossArgs q{};
  int term;
  const int linear = loss_type == 1;
  if (make_loss_args(nlevels, dims, base, N, ncols, loss_type, obj, reg, targets, boxes, offs, midx, cams, res, q, term)) return -4;
  loss_dispatch(term, cams != nullptr, [&](auto T, auto P) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(rpn_loss_fwd_kernel<decltype(T)::value, decltype(P)::value>), dim3(q.G.nblocks), dim3(256), 0, st, q.G, q.B, q.S, q.obj, q.reg, flags, targets, boxes, ori, midx,
                       linear, q.cams, partials);
  });
  NMH_CHECK_LAUNCH();
  if (cams) hipLaunchKernelGGL(rpn_loss_final_kernel<5>, dim3(1), dim3(256), 0, st, partials, q.G.nblocks, res, scalars);
  else hipLaunchKernelGGL(rpn_loss_final_kernel<3>, dim3(1), dim3(256), 0, st, partials, q.G.nblocks, res, scalars);
  NMH_CHECK_LAUNCH();
  return 0;
}

int k_rpn_loss_bwd(int nlevels, const int* dims, const float* base, int N, int ncols, int loss_type, const float* const* obj, const float* const* reg, const unsigned char* flags,
                   const float* targets, const float* boxes, const int* offs, const int* ori, const int* midx, const float* cams, float res, const float* scalars,
                   const float* g_obj, const float* g_reg, const float* g_2d, float* const* dobj, float* const* dreg, hipStream_t st) {
  RpnLossArgs q{};
  int term;
  const int linear = loss_type == 1;
  if (make_loss_args(nlevels, dims, base, N, ncols, loss_type, obj, reg, targets, boxes, offs, midx, cams, res, q, term) || !all_set(nlevels, dobj) ||
      !all_set(nlevels, dreg)) return -4;
  const Ptr4<float> DO = make_ptrs<float>(nlevels, dobj), DR = make_ptrs<float>(nlevels, dreg);
  loss_dispatch(term, cams != nullptr, [&](auto T, auto P) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(rpn_loss_bwd_kernel<decltype(T)::value, decltype(P)::value>), dim3(q.G.nblocks), dim3(256), 0, st, q.G, q.B, q.S, q.obj, q.reg, flags, targets, boxes, ori, midx,
                       linear, q.cams, res, scalars, g_obj, g_reg, g_2d, DO, DR);
  });
  NMH_CHECK_LAUNCH();
  return 0;
}

// Oriented 3-D box IoU / GIoU / DIoU losses and rotated NMS of the reference's downstream detectors, as gfx950 kernels:
//   cal_iou_3d / cal_giou_3d / cal_diou_3d (nerf_rpn/model/rotated_iou/oriented_iou_loss.py:82-148, over box_intersection_2d.py and
//     min_enclosing_box.py:25-166; called by fcos/loss.py:135-171 and rpn.py:143-156): obb_iou_fwd / obb_iou_bwd, one box pair per lane;
//   box_iou_3d (fcos/utils.py:229-255, utils.py): obb_iou_pairwise, the [N,M] matrix without the N x M x 7 repeat;
//   nms / batched_nms (fcos/utils.py:109-158): obb_nms_mask (suppression bit matrix) + obb_nms_scan (greedy walk on the device).
//
// Semantics.  A box is (x, y, z, w, l, h, theta) fp32, theta in RADIANS about the third axis (the RoIAlign op of rotated.hip takes
// degrees).  Its bird's-eye-view (BEV) rectangle has the corners of box2corners_th: local (+-w/2, +-l/2) in the order (+,+), (-,+), (-,-),
// (+,-), rotated counter-clockwise by theta, translated by (x, y).  For a pair:
//   inter2d   = area of the intersection of the two BEV rectangles
//   z_overlap = max(0, min(zmax1, zmax2) - max(zmin1, zmin2)),   zmax = z + h/2, zmin = z - h/2
//   inter3d   = inter2d * z_overlap,   u3d = w1 l1 h1 + w2 l2 h2 - inter3d,   iou3d = inter3d / u3d
//   z_range   = max(0, max(zmax1, zmax2) - min(zmin1, zmin2))
// Enclosing rectangle (w_c, h_c) of the eight BEV corners:
//   "aligned":  the axis-aligned extent (x extent, y extent);
//   "smallest": for every line through two of the eight corners except the four diagonals (24 candidates, in the order i < j of
//     min_enclosing_box.py:43-48), proj = extent of the eight corners along the line, dist = their extent across it; candidates with
//     proj * dist == 0 (or coincident points) are left out; the first candidate of minimum proj * dist gives (w_c, h_c) = (proj, dist).
//   GIoU: v_c = z_range w_c h_c,  loss = 1 - iou3d + (v_c - u3d) / v_c          (giou = 1 - loss is formed by the caller)
//   DIoU: loss = 1 - iou3d + d2 / c2,  d2 = |centre1 - centre2|^2 in 3-D,  c2 = w_c^2 + h_c^2 + z_range^2
// The 6-column form of the pairwise and NMS kernels is (x1, y1, z1, x2, y2, z2) with the closed form of _box_inter_union_3d
// (fcos/utils.py:285-297).
//
// Algorithm.  No vertex list exists anywhere, so there is no vertex count to bound and no per-lane array (nothing goes to scratch).
//   Area.  Box 1 is expressed in the frame of box 2, where box 2 is [-a, a] x [-b, b].  For a counter-clockwise polygon P,
//     area(P and box 2) = - sum over the edges of P of the integral of clamp(y, -b, b) dx over the part of the edge with |x| <= a
//     (per vertical line the slice of P is an interval, and its part inside [-b, b] is clamp(top) - clamp(bottom)).  On an edge the integrand
//     is piecewise linear with breaks where y crosses -b and b: three trapezoids, exact, no cancellation between terms of one edge.  Each
//     edge contributes on its own, so touching or coincident edges cannot be counted twice and nothing needs sorting.
//   Disjoint pairs.  The formula's terms cancel only to rounding, so a separating-axis test on the four edge normals (and, in the pairwise
//     and NMS kernels, first the z overlap and the BEV circumscribed circles) decides "no overlap" and gives exactly 0.
//   Area gradient.  The derivative of the intersection area under a motion of one box is the integral of the outward normal velocity over
//     the parts of THAT box's edges inside the other (no pass through the clipping).  Each edge of box 1 is clipped to box 2 in box 2's
//     frame (Liang-Barsky, closed), giving the part [t0, t1] of an edge of length L with outward normal n:
//       d/d(centre) += n (t1 - t0) L;   d/d(size along n) += (t1 - t0) L / 2;   d/d(theta) -= L^2 ((t1 - 1/2)^2 - (t0 - 1/2)^2) / 2
//     and the same with the roles exchanged for box 2.  A pair that the separating-axis test rejects gets exactly 0.
//   Enclosing rectangle gradient.  (w_c, h_c) of the winning candidate are differentiated by hand: to the two extreme corners along and
//     across the line, and through the line's direction to its two corners; corner gradients are then taken to (x, y, w, l, theta) of the
//     box the corner belongs to.  Which corner is extreme is found by unrolled compares on compile-time indices.
//   min / max of the z bounds split a gradient evenly on a tie, as torch.min / torch.max do.
// DEVIATIONS from the reference.  Two identical boxes give iou3d >= 1 - 1e-4 (the reference's vertex method can count touching corners
// twice and overflow its nine index slots there).  The reference's stabilisers (1e-8 in t and in the slope, 1e-14 under the root) are not
// reproduced; they move results by about 1e-8 relative.  For any input, non-finite values and non-positive sizes included, every kernel
// writes only its own outputs; the values for such input are unspecified.
//
// NMS.  Boxes arrive ordered by descending score.  mask[i][j] (64-bit words, ceil(N/64) per row) has bit k set iff
// iou(i, 64 j + k) > threshold, 64 j + k > i (and category equal, when categories are given: an offset-coordinates trick is not valid for
// rotated boxes).  Words with j < floor(i / 64) (strictly below the diagonal block) are all zero by definition, are never read by the scan and
// are NOT written: only the upper triangle of 64 x 64 blocks is launched.  One wave computes one word: lane k takes column 64 j + k and the ballot is the word.  The scan is one workgroup; per
// block of 64 rows it resolves the block's own dependencies from the 64 diagonal words, then ORs the rows of the kept boxes into the
// removed-set in LDS.  Kept positions and their count are written to device memory; the host is not involved.
#include "common.hpp"
#include "kernels.hpp"

namespace {

enum { OBB_IOU = 0, OBB_GIOU_SMALLEST = 1, OBB_GIOU_ALIGNED = 2, OBB_DIOU_SMALLEST = 3, OBB_DIOU_ALIGNED = 4 };

struct Obb { float x, y, z, w, l, h, cs, sn; };
__device__ __forceinline__ Obb obb_load(const float* __restrict__ b) {
  Obb o;
  o.x = b[0]; o.y = b[1]; o.z = b[2]; o.w = b[3]; o.l = b[4]; o.h = b[5];
  o.sn = sinf(b[6]); o.cs = cosf(b[6]);
  return o;
}

// box A in the frame of box B: centre (px, py), cos / sin of thetaA - thetaB
struct Rel { float px, py, c, s; };
__device__ __forceinline__ Rel obb_rel(const Obb& A, const Obb& B) {
  const float dx = A.x - B.x, dy = A.y - B.y;
  Rel r;
  r.px = dx * B.cs + dy * B.sn;
  r.py = dy * B.cs - dx * B.sn;
  r.c = A.cs * B.cs + A.sn * B.sn;
  r.s = A.sn * B.cs - A.cs * B.sn;
  return r;
}
// a normal of B separates the two rectangles (touching counts as separated)
__device__ __forceinline__ bool obb_separated(const Rel& r, float hw, float hl, float a, float b) {
  const float ac = fabsf(r.c), as = fabsf(r.s);
  return fabsf(r.px) >= a + hw * ac + hl * as || fabsf(r.py) >= b + hw * as + hl * ac;
}
__device__ __forceinline__ float clampf(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

// - integral of clamp(y, -b, b) dx over the part of the edge (xa,ya) -> (xb,yb) with |x| <= a
__device__ __forceinline__ float obb_edge_area(float xa, float ya, float xb, float yb, float a, float b) {
  const float dx = xb - xa, dy = yb - ya;
  if (dx == 0.f) return 0.f;
  const float tA = (-a - xa) / dx, tB = (a - xa) / dx;
  const float t0 = fmaxf(0.f, fminf(tA, tB)), t1 = fminf(1.f, fmaxf(tA, tB));
  if (!(t1 > t0)) return 0.f;
  float s1 = t0, s2 = t0;
  if (dy != 0.f) {
    const float ta = (-b - ya) / dy, tb = (b - ya) / dy;
    s1 = clampf(fminf(ta, tb), t0, t1);
    s2 = clampf(fmaxf(ta, tb), t0, t1);
  }
  const float f0 = clampf(ya + t0 * dy, -b, b), f1 = clampf(ya + s1 * dy, -b, b), f2 = clampf(ya + s2 * dy, -b, b), f3 = clampf(ya + t1 * dy, -b, b);
  return -0.5f * ((f0 + f1) * (s1 - t0) + (f1 + f2) * (s2 - s1) + (f2 + f3) * (t1 - s2)) * dx;
}
// area of (rectangle of half sizes hw, hl at pose r) and [-a,a] x [-b,b]
__device__ __forceinline__ float obb_clip_area(const Rel& r, float hw, float hl, float a, float b) {
  const float ux = r.c * hw, uy = r.s * hw, vx = -r.s * hl, vy = r.c * hl;
  const float x0 = r.px + ux + vx, y0 = r.py + uy + vy, x1 = r.px - ux + vx, y1 = r.py - uy + vy;
  const float x2 = r.px - ux - vx, y2 = r.py - uy - vy, x3 = r.px + ux - vx, y3 = r.py + uy - vy;
  const float s = obb_edge_area(x0, y0, x1, y1, a, b) + obb_edge_area(x1, y1, x2, y2, a, b) + obb_edge_area(x2, y2, x3, y3, a, b) + obb_edge_area(x3, y3, x0, y0, a, b);
  return fmaxf(s, 0.f);
}
// BEV intersection area of two boxes; exactly 0 when a separating axis exists
__device__ __forceinline__ float obb_inter2d(const Obb& A, const Obb& B, bool& overlap) {
  const Rel r = obb_rel(A, B), q = obb_rel(B, A);
  overlap = !obb_separated(r, 0.5f * A.w, 0.5f * A.l, 0.5f * B.w, 0.5f * B.l) && !obb_separated(q, 0.5f * B.w, 0.5f * B.l, 0.5f * A.w, 0.5f * A.l);
  return overlap ? obb_clip_area(r, 0.5f * A.w, 0.5f * A.l, 0.5f * B.w, 0.5f * B.l) : 0.f;
}

// the part [t0, t1] of the segment p + t d, t in [0, 1], inside [-a,a] x [-b,b] (closed); empty: t1 <= t0
__device__ __forceinline__ void obb_lb_axis(float p, float q, float& t0, float& t1) {
  if (p == 0.f) { if (q < 0.f) t1 = -1.f; }
  else if (p < 0.f) t0 = fmaxf(t0, q / p);
  else t1 = fminf(t1, q / p);
}
__device__ __forceinline__ float obb_edge_clip(float x, float y, float dx, float dy, float a, float b, float& t0) {
  float t1 = 1.f;
  t0 = 0.f;
  obb_lb_axis(-dx, x + a, t0, t1);
  obb_lb_axis(dx, a - x, t0, t1);
  obb_lb_axis(-dy, y + b, t0, t1);
  obb_lb_axis(dy, b - y, t0, t1);
  return t1;
}
// gradient of the intersection area with respect to the pose of the box at r (half sizes hw, hl) inside [-a,a] x [-b,b]:
// (gx, gy) in the frame of the other box, gw, gl for the full sizes, gt for the angle
struct AreaGrad { float gx, gy, gw, gl, gt; };
__device__ __forceinline__ void obb_edge_grad(float x, float y, float tx, float ty, float L, float a, float b, float& len, float& mom) {
  // edge from (x, y) along the unit tangent (tx, ty), length L -> clipped length, and integral of s ds with s measured from the middle
  float t0;
  const float t1 = obb_edge_clip(x, y, tx * L, ty * L, a, b, t0);
  const bool ok = t1 > t0;
  len = ok ? (t1 - t0) * L : 0.f;
  mom = ok ? 0.5f * L * L * (t1 - t0) * (t1 + t0 - 1.f) : 0.f;
}
__device__ __forceinline__ AreaGrad obb_area_grad(const Rel& r, float hw, float hl, float a, float b) {
  const float ux = r.c, uy = r.s, vx = -r.s, vy = r.c;       // the box's own axes
  const float x0 = r.px + ux * hw + vx * hl, y0 = r.py + uy * hw + vy * hl, x1 = r.px - ux * hw + vx * hl, y1 = r.py - uy * hw + vy * hl;
  const float x2 = r.px - ux * hw - vx * hl, y2 = r.py - uy * hw - vy * hl, x3 = r.px + ux * hw - vx * hl, y3 = r.py + uy * hw - vy * hl;
  float l0, m0, l1, m1, l2, m2, l3, m3;
  obb_edge_grad(x0, y0, -ux, -uy, 2.f * hw, a, b, l0, m0);   // normal +v
  obb_edge_grad(x1, y1, -vx, -vy, 2.f * hl, a, b, l1, m1);   // normal -u
  obb_edge_grad(x2, y2, ux, uy, 2.f * hw, a, b, l2, m2);     // normal -v
  obb_edge_grad(x3, y3, vx, vy, 2.f * hl, a, b, l3, m3);     // normal +u
  AreaGrad g;
  g.gx = vx * (l0 - l2) + ux * (l3 - l1);
  g.gy = vy * (l0 - l2) + uy * (l3 - l1);
  g.gw = 0.5f * (l1 + l3);
  g.gl = 0.5f * (l0 + l2);
  g.gt = -(m0 + m1 + m2 + m3);
  return g;
}

// the eight BEV corners, box 1 then box 2
__device__ __forceinline__ void obb_corners(const Obb& o, float (&X)[8], float (&Y)[8], int at) {
  const float ux = 0.5f * o.w * o.cs, uy = 0.5f * o.w * o.sn, vx = -0.5f * o.l * o.sn, vy = 0.5f * o.l * o.cs;
  X[at + 0] = o.x + ux + vx; Y[at + 0] = o.y + uy + vy;
  X[at + 1] = o.x - ux + vx; Y[at + 1] = o.y - uy + vy;
  X[at + 2] = o.x - ux - vx; Y[at + 2] = o.y - uy - vy;
  X[at + 3] = o.x + ux - vx; Y[at + 3] = o.y + uy - vy;
}
__host__ __device__ constexpr bool obb_diagonal(int i, int j) { return (i == 0 && j == 2) || (i == 1 && j == 3) || (i == 4 && j == 6) || (i == 5 && j == 7); }

// the enclosing rectangle: (w, h) and the direction it was measured along (unit e), with the line's corner pair (li, lj; -1: none) and
// length n for the gradient
struct Encl { float w, h, ex, ey, n; int li, lj; };
template <bool SMALLEST>
__device__ __forceinline__ Encl obb_enclosing(const float (&X)[8], const float (&Y)[8]) {
  Encl E;
  E.li = E.lj = -1; E.n = 1.f; E.ex = 1.f; E.ey = 0.f;
  if (!SMALLEST) {
    float xl = X[0], xh = X[0], yl = Y[0], yh = Y[0];
#pragma unroll
    for (int k = 1; k < 8; ++k) { xl = fminf(xl, X[k]); xh = fmaxf(xh, X[k]); yl = fminf(yl, Y[k]); yh = fmaxf(yh, Y[k]); }
    E.w = xh - xl; E.h = yh - yl;
    return E;
  }
  float best = 3.0e38f, bpe = 0.f, bde = 0.f, bn2 = 1.f, bdx = 1.f, bdy = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
#pragma unroll
    for (int j = i + 1; j < 8; ++j) {
      if (obb_diagonal(i, j)) continue;
      const float dx = X[j] - X[i], dy = Y[j] - Y[i], n2 = dx * dx + dy * dy;
      float al = dx * X[0] + dy * Y[0], ah = al, cl = dx * Y[0] - dy * X[0], ch = cl;
#pragma unroll
      for (int k = 1; k < 8; ++k) {
        const float u = dx * X[k] + dy * Y[k], v = dx * Y[k] - dy * X[k];
        al = fminf(al, u); ah = fmaxf(ah, u); cl = fminf(cl, v); ch = fmaxf(ch, v);
      }
      const float pe = ah - al, de = ch - cl, area = pe * de / n2;
      if (n2 > 0.f && area > 0.f && area < best) { best = area; bpe = pe; bde = de; bn2 = n2; bdx = dx; bdy = dy; E.li = i; E.lj = j; }
    }
  }
  const float n = sqrtf(bn2);
  E.w = bpe / n; E.h = bde / n; E.n = n; E.ex = bdx / n; E.ey = bdy / n;
  return E;
}

// forward quantities of one pair
struct PairOut { float inter2d, zo, inter3d, v1, v2, u3d, iou, zr; bool overlap; };
__device__ __forceinline__ PairOut obb_pair(const Obb& A, const Obb& B) {
  PairOut p;
  const float zx1 = A.z + 0.5f * A.h, zn1 = A.z - 0.5f * A.h, zx2 = B.z + 0.5f * B.h, zn2 = B.z - 0.5f * B.h;
  p.zo = fmaxf(fminf(zx1, zx2) - fmaxf(zn1, zn2), 0.f);
  p.zr = fmaxf(fmaxf(zx1, zx2) - fminf(zn1, zn2), 0.f);
  p.inter2d = obb_inter2d(A, B, p.overlap);
  p.inter3d = p.inter2d * p.zo;
  p.v1 = A.w * A.l * A.h; p.v2 = B.w * B.l * B.h;
  p.u3d = p.v1 + p.v2 - p.inter3d;
  p.iou = p.inter3d / p.u3d;
  return p;
}

template <int MODE>
__global__ __launch_bounds__(256) void obb_iou_fwd_kernel(const float* __restrict__ b1, const float* __restrict__ b2, long n, float* __restrict__ iou, float* __restrict__ u3d,
                                                          float* __restrict__ zr, float* __restrict__ loss, float* __restrict__ wc, float* __restrict__ hc,
                                                          float* __restrict__ c1, float* __restrict__ c2) {
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const Obb A = obb_load(b1 + p * 7), B = obb_load(b2 + p * 7);
  const PairOut o = obb_pair(A, B);
  iou[p] = o.iou;
  if (u3d) u3d[p] = o.u3d;
  if (zr) zr[p] = o.zr;
  if (MODE == OBB_IOU && !c1 && !c2) return;
  float X[8], Y[8];
  obb_corners(A, X, Y, 0);
  obb_corners(B, X, Y, 4);
  if (c1) {
#pragma unroll
    for (int k = 0; k < 4; ++k) { c1[p * 8 + 2 * k] = X[k]; c1[p * 8 + 2 * k + 1] = Y[k]; }
  }
  if (c2) {
#pragma unroll
    for (int k = 0; k < 4; ++k) { c2[p * 8 + 2 * k] = X[4 + k]; c2[p * 8 + 2 * k + 1] = Y[4 + k]; }
  }
  if (MODE == OBB_IOU) return;
  const Encl E = obb_enclosing<MODE == OBB_GIOU_SMALLEST || MODE == OBB_DIOU_SMALLEST>(X, Y);
  float ls;
  if (MODE == OBB_GIOU_SMALLEST || MODE == OBB_GIOU_ALIGNED) {
    const float vc = o.zr * E.w * E.h;
    ls = 1.f - o.iou + (vc - o.u3d) / vc;
  } else {
    const float dx = A.x - B.x, dy = A.y - B.y, dz = A.z - B.z;
    ls = 1.f - o.iou + (dx * dx + dy * dy + dz * dz) / (E.w * E.w + E.h * E.h + o.zr * o.zr);
  }
  loss[p] = ls;
  if (wc) wc[p] = E.w;
  if (hc) hc[p] = E.h;
}

// gradient of min(a, b) (MIN) or max(a, b) with respect to a; the tie is split evenly
template <bool MIN> __device__ __forceinline__ float pick_a(float a, float b) { return a == b ? 0.5f : ((MIN ? a < b : a > b) ? 1.f : 0.f); }

struct BoxGrad { float x, y, z, w, l, h, t; };
// corner gradients (Gx, Gy)[at .. at+3] -> gradient of the box they belong to
__device__ __forceinline__ void obb_corner_grads_to_box(const Obb& o, const float (&X)[8], const float (&Y)[8], const float (&Gx)[8], const float (&Gy)[8], int at, BoxGrad& g) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float sx = (k == 0 || k == 3) ? 0.5f : -0.5f, sy = (k < 2) ? 0.5f : -0.5f;
    const float gx = Gx[at + k], gy = Gy[at + k];
    g.x += gx; g.y += gy;
    g.w += sx * (gx * o.cs + gy * o.sn);
    g.l += sy * (gy * o.cs - gx * o.sn);
    g.t += gy * (X[at + k] - o.x) - gx * (Y[at + k] - o.y);
  }
}

template <int MODE>
__global__ __launch_bounds__(256) void obb_iou_bwd_kernel(const float* __restrict__ b1, const float* __restrict__ b2, long n, const float* __restrict__ g_iou,
                                                          const float* __restrict__ g_u3d, const float* __restrict__ g_loss, int g_one, float* __restrict__ d1, float* __restrict__ d2) {
  constexpr bool ENC = MODE != OBB_IOU, GIOU = MODE == OBB_GIOU_SMALLEST || MODE == OBB_GIOU_ALIGNED;
  constexpr bool SMALLEST = MODE == OBB_GIOU_SMALLEST || MODE == OBB_DIOU_SMALLEST;
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const Obb A = obb_load(b1 + p * 7), B = obb_load(b2 + p * 7);
  const PairOut o = obb_pair(A, B);
  // bit k of g_one: incoming gradient k is ONE value for every pair (the expanded gradient of a sum())
  const float gi_in = g_iou ? g_iou[(g_one & 1) ? 0 : p] : 0.f, gu_in = g_u3d ? g_u3d[(g_one & 2) ? 0 : p] : 0.f, gl = (ENC && g_loss) ? g_loss[(g_one & 4) ? 0 : p] : 0.f;
  BoxGrad ga{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, gb{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const float zx1 = A.z + 0.5f * A.h, zn1 = A.z - 0.5f * A.h, zx2 = B.z + 0.5f * B.h, zn2 = B.z - 0.5f * B.h;

  float gi = gi_in - gl;          // loss = 1 - iou + ...
  float gU = gu_in - gi * o.inter3d / (o.u3d * o.u3d);
  float gzr = 0.f, gw = 0.f, gh = 0.f;
  float X[8], Y[8];
  Encl E;
  if (ENC) {
    obb_corners(A, X, Y, 0);
    obb_corners(B, X, Y, 4);
    E = obb_enclosing<SMALLEST>(X, Y);
    if (GIOU) {                   // loss = 2 - iou - u3d / vc
      const float vc = o.zr * E.w * E.h;
      gU -= gl / vc;
      const float gvc = gl * o.u3d / (vc * vc);
      gzr = gvc * E.w * E.h; gw = gvc * o.zr * E.h; gh = gvc * o.zr * E.w;
    } else {
      const float dx = A.x - B.x, dy = A.y - B.y, dz = A.z - B.z;
      const float c2 = E.w * E.w + E.h * E.h + o.zr * o.zr, dd = dx * dx + dy * dy + dz * dz;
      const float gd = 2.f * gl / c2;
      ga.x += gd * dx; ga.y += gd * dy; ga.z += gd * dz;
      gb.x -= gd * dx; gb.y -= gd * dy; gb.z -= gd * dz;
      const float gc2 = -2.f * gl * dd / (c2 * c2);
      gw = gc2 * E.w; gh = gc2 * E.h; gzr = gc2 * o.zr;
    }
  }
  // u3d = v1 + v2 - inter3d
  ga.w += gU * A.l * A.h; ga.l += gU * A.w * A.h; ga.h += gU * A.w * A.l;
  gb.w += gU * B.l * B.h; gb.l += gU * B.w * B.h; gb.h += gU * B.w * B.l;
  const float gI = gi / o.u3d - gU;
  // inter3d = inter2d * zo
  if (o.zo > 0.f) {
    const float gzo = gI * o.inter2d;
    const float tx = pick_a<true>(zx1, zx2), tn = pick_a<false>(zn1, zn2);   // share of box 1 in min(zmax) and max(zmin)
    const float gzx1 = gzo * tx, gzx2 = gzo * (1.f - tx), gzn1 = -gzo * tn, gzn2 = -gzo * (1.f - tn);
    ga.z += gzx1 + gzn1; ga.h += 0.5f * (gzx1 - gzn1);
    gb.z += gzx2 + gzn2; gb.h += 0.5f * (gzx2 - gzn2);
  }
  if (ENC && o.zr > 0.f) {
    const float tx = pick_a<false>(zx1, zx2), tn = pick_a<true>(zn1, zn2);   // max(zmax), min(zmin)
    const float gzx1 = gzr * tx, gzx2 = gzr * (1.f - tx), gzn1 = -gzr * tn, gzn2 = -gzr * (1.f - tn);
    ga.z += gzx1 + gzn1; ga.h += 0.5f * (gzx1 - gzn1);
    gb.z += gzx2 + gzn2; gb.h += 0.5f * (gzx2 - gzn2);
  }
  if (o.overlap) {
    const float gA = gI * o.zo;
    const AreaGrad q1 = obb_area_grad(obb_rel(A, B), 0.5f * A.w, 0.5f * A.l, 0.5f * B.w, 0.5f * B.l);
    ga.x += gA * (q1.gx * B.cs - q1.gy * B.sn); ga.y += gA * (q1.gx * B.sn + q1.gy * B.cs);
    ga.w += gA * q1.gw; ga.l += gA * q1.gl; ga.t += gA * q1.gt;
    if (d2) {
      const AreaGrad q2 = obb_area_grad(obb_rel(B, A), 0.5f * B.w, 0.5f * B.l, 0.5f * A.w, 0.5f * A.l);
      gb.x += gA * (q2.gx * A.cs - q2.gy * A.sn); gb.y += gA * (q2.gx * A.sn + q2.gy * A.cs);
      gb.w += gA * q2.gw; gb.l += gA * q2.gl; gb.t += gA * q2.gt;
    }
  }
  if (ENC) {
    // w = e . (P_a - P_b), h = f . (P_c - P_d), f = perp(e); e = (P_lj - P_li) / n for the smallest rectangle, fixed (1, 0) for the aligned one
    const float ex = E.ex, ey = E.ey, fx = -E.ey, fy = E.ex;
    float uh = ex * X[0] + ey * Y[0], ul = uh, vh = fx * X[0] + fy * Y[0], vl = vh, v_at_uh = vh, v_at_ul = vh, u_at_vh = uh, u_at_vl = uh;
    int ia = 0, ib = 0, ic = 0, id = 0;
#pragma unroll
    for (int k = 1; k < 8; ++k) {
      const float u = ex * X[k] + ey * Y[k], v = fx * X[k] + fy * Y[k];
      if (u > uh) { uh = u; v_at_uh = v; ia = k; }
      if (u < ul) { ul = u; v_at_ul = v; ib = k; }
      if (v > vh) { vh = v; u_at_vh = u; ic = k; }
      if (v < vl) { vl = v; u_at_vl = u; id = k; }
    }
    // through the direction: dw/dd = (f . D_w) f / n, dh/dd = -(e . D_h) f / n
    const float gdir = SMALLEST ? (gw * (v_at_uh - v_at_ul) - gh * (u_at_vh - u_at_vl)) / E.n : 0.f;
    float Gx[8], Gy[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float sw = (float)(k == ia) - (float)(k == ib), sh = (float)(k == ic) - (float)(k == id), sd = (float)(k == E.lj) - (float)(k == E.li);
      Gx[k] = gw * ex * sw + gh * fx * sh + gdir * fx * sd;
      Gy[k] = gw * ey * sw + gh * fy * sh + gdir * fy * sd;
    }
    obb_corner_grads_to_box(A, X, Y, Gx, Gy, 0, ga);
    if (d2) obb_corner_grads_to_box(B, X, Y, Gx, Gy, 4, gb);
  }
  if (d1) { float* q = d1 + p * 7; q[0] = ga.x; q[1] = ga.y; q[2] = ga.z; q[3] = ga.w; q[4] = ga.l; q[5] = ga.h; q[6] = ga.t; }
  if (d2) { float* q = d2 + p * 7; q[0] = gb.x; q[1] = gb.y; q[2] = gb.z; q[3] = gb.w; q[4] = gb.l; q[5] = gb.h; q[6] = gb.t; }
}

// ---- all pairs: tiles of 16 rows x 64 columns, both box tiles staged in LDS with their sin / cos taken once -------------------------
constexpr int PW_ROWS = 16, PW_COLS = 64;
struct BoxTile { float v[8]; };   // 7 columns: x y z w l h cos sin; 6 columns: x1 y1 z1 x2 y2 z2
template <bool AABB>
__device__ __forceinline__ void stage_box(const float* __restrict__ src, long i, long n, BoxTile& dst) {
  if (i < n) {
    if (AABB) {
#pragma unroll
      for (int k = 0; k < 6; ++k) dst.v[k] = src[i * 6 + k];
      dst.v[6] = dst.v[7] = 0.f;
    } else {
      const Obb o = obb_load(src + i * 7);
      dst.v[0] = o.x; dst.v[1] = o.y; dst.v[2] = o.z; dst.v[3] = o.w; dst.v[4] = o.l; dst.v[5] = o.h; dst.v[6] = o.cs; dst.v[7] = o.sn;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) dst.v[k] = 0.f;
  }
}
template <bool AABB>
__device__ __forceinline__ float tile_iou(const BoxTile& a, const BoxTile& b) {
  if (AABB) {
    const float ix = fmaxf(fminf(a.v[3], b.v[3]) - fmaxf(a.v[0], b.v[0]), 0.f), iy = fmaxf(fminf(a.v[4], b.v[4]) - fmaxf(a.v[1], b.v[1]), 0.f);
    const float iz = fmaxf(fminf(a.v[5], b.v[5]) - fmaxf(a.v[2], b.v[2]), 0.f);
    const float inter = ix * iy * iz;
    const float va = (a.v[3] - a.v[0]) * (a.v[4] - a.v[1]) * (a.v[5] - a.v[2]), vb = (b.v[3] - b.v[0]) * (b.v[4] - b.v[1]) * (b.v[5] - b.v[2]);
    return inter / (va + vb - inter);
  }
  const Obb A{a.v[0], a.v[1], a.v[2], a.v[3], a.v[4], a.v[5], a.v[6], a.v[7]}, B{b.v[0], b.v[1], b.v[2], b.v[3], b.v[4], b.v[5], b.v[6], b.v[7]};
  // cheap rejection: no z overlap, or the circumscribed circles of the BEV rectangles are disjoint
  const float zo = fminf(A.z + 0.5f * A.h, B.z + 0.5f * B.h) - fmaxf(A.z - 0.5f * A.h, B.z - 0.5f * B.h);
  if (!(zo > 0.f)) return 0.f;
  const float dx = A.x - B.x, dy = A.y - B.y, rr = 0.5f * (sqrtf(A.w * A.w + A.l * A.l) + sqrtf(B.w * B.w + B.l * B.l));
  if (dx * dx + dy * dy >= rr * rr) return 0.f;
  bool overlap;
  const float inter = obb_inter2d(A, B, overlap) * zo;
  if (!overlap) return 0.f;
  return inter / (A.w * A.l * A.h + B.w * B.l * B.h - inter);
}

template <bool AABB>
__global__ __launch_bounds__(256) void obb_iou_pairwise_kernel(const float* __restrict__ b1, const float* __restrict__ b2, int N, int M, float* __restrict__ iou) {
  __shared__ BoxTile rows[PW_ROWS], cols[PW_COLS];
  const int t = threadIdx.x;
  const long r0 = (long)blockIdx.y * PW_ROWS, c0 = (long)blockIdx.x * PW_COLS;
  if (t < PW_COLS) stage_box<AABB>(b2, c0 + t, M, cols[t]);
  else if (t < PW_COLS + PW_ROWS) stage_box<AABB>(b1, r0 + (t - PW_COLS), N, rows[t - PW_COLS]);
  __syncthreads();
  const int c = t & (PW_COLS - 1);
  if (c0 + c >= M) return;
  const BoxTile bc = cols[c];
#pragma unroll 1
  for (int r = t >> 6; r < PW_ROWS; r += 4) {
    if (r0 + r >= N) break;
    iou[(r0 + r) * M + c0 + c] = tile_iou<AABB>(rows[r], bc);
  }
}

// ---- NMS: word (i, j) of the suppression matrix per wave, 64 rows x 64 columns per block ------------------------------------------------
template <bool AABB>
__global__ __launch_bounds__(256) void obb_nms_mask_kernel(const float* __restrict__ boxes, const int* __restrict__ cat, int N, float thr, unsigned long long* __restrict__ mask) {
  __shared__ BoxTile rows[64], cols[64];
  __shared__ int rcat[64];
  const int t = threadIdx.x, nw = (N + 63) >> 6;
  // the grid is the upper triangle of the nw x nw blocks, row block by row block: block row `by` has the words j = by .. nw-1
  int by = 0, j = blockIdx.x;
  while (j >= nw - by) { j -= nw - by; ++by; }      // uniform, at most nw <= 256 steps
  j += by;
  const long r0 = (long)by * 64, c0 = (long)j * 64;
  if (t < 64) stage_box<AABB>(boxes, c0 + t, N, cols[t]);
  else if (t < 128) { stage_box<AABB>(boxes, r0 + (t - 64), N, rows[t - 64]); rcat[t - 64] = (cat && r0 + (t - 64) < N) ? cat[r0 + (t - 64)] : 0; }
  __syncthreads();
  const int k = t & 63;
  const long col = c0 + k;
  const BoxTile bc = cols[k];
  const int ccat = (cat && col < N) ? cat[col] : 0;
#pragma unroll 1
  for (int r = t >> 6; r < 64; r += 4) {
    const long row = r0 + r;
    if (row >= N) break;                   // uniform over the wave
    bool hit = false;
    if (col > row && col < N && ccat == rcat[r]) hit = tile_iou<AABB>(rows[r], bc) > thr;
    const unsigned long long word = __ballot(hit);
    if (k == 0) mask[row * nw + j] = word;
  }
}

// one workgroup; N <= 16384 (256 words of removed-set)
__global__ __launch_bounds__(256) void obb_nms_scan_kernel(const unsigned long long* __restrict__ mask, int N, int* __restrict__ keep, int* __restrict__ count) {
  __shared__ unsigned long long removed[256], diag[64];
  const int t = threadIdx.x, nw = (N + 63) >> 6;
  removed[t] = 0ull;
  int cnt = 0;                             // the same in every thread
  for (int c = 0; c < nw; ++c) {
    __syncthreads();                       // removed[] of the previous block is complete; diag[] is free
    if (t < 64) diag[t] = c * 64 + t < N ? mask[(long)(c * 64 + t) * nw + c] : 0ull;
    __syncthreads();
    unsigned long long r = removed[c];
    const int left = N - c * 64;
    if (left < 64) r |= ~0ull << left;     // positions past N count as removed
    for (int k = 0; k < 64; ++k)           // row k's word only has bits above k, so bit k of r is final when it is read
      if (!((r >> k) & 1ull)) r |= diag[k];
    const unsigned long long kept = ~r;
    if (t < 64 && ((kept >> t) & 1ull)) keep[cnt + __popcll(kept & ((1ull << t) - 1ull))] = c * 64 + t;
    cnt += __popcll(kept);
    const int nrem = nw - c - 1;           // words after the diagonal one
    for (int q = t; q < 64 * nrem; q += 256) {
      const int k = q / nrem, w = c + 1 + q % nrem;
      if ((kept >> k) & 1ull) {
        const unsigned long long m = mask[(long)(c * 64 + k) * nw + w];
        if (m) atomicOr(&removed[w], m);
      }
    }
  }
  if (t == 0) *count = cnt;
}

template <int MODE>
void launch_fwd(const float* b1, const float* b2, long n, float* iou, float* u3d, float* zr, float* loss, float* wc, float* hc, float* c1, float* c2, hipStream_t st) {
  hipLaunchKernelGGL(obb_iou_fwd_kernel<MODE>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, b1, b2, n, iou, u3d, zr, loss, wc, hc, c1, c2);
}
template <int MODE>
void launch_bwd(const float* b1, const float* b2, long n, const float* gi, const float* gu, const float* gl, int g_one, float* d1, float* d2, hipStream_t st) {
  hipLaunchKernelGGL(obb_iou_bwd_kernel<MODE>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, b1, b2, n, gi, gu, gl, g_one, d1, d2);
}

}  // namespace

int k_obb_iou_fwd(int mode, const float* b1, const float* b2, long n, float* iou, float* u3d, float* zr, float* loss, float* wc, float* hc, float* c1, float* c2, hipStream_t st) {
  if (n <= 0 || (n + 255) / 256 >= (1L << 31)) return -4;
  switch (mode) {
    case OBB_IOU: launch_fwd<OBB_IOU>(b1, b2, n, iou, u3d, zr, loss, wc, hc, c1, c2, st); break;
    case OBB_GIOU_SMALLEST: launch_fwd<OBB_GIOU_SMALLEST>(b1, b2, n, iou, u3d, zr, loss, wc, hc, c1, c2, st); break;
    case OBB_GIOU_ALIGNED: launch_fwd<OBB_GIOU_ALIGNED>(b1, b2, n, iou, u3d, zr, loss, wc, hc, c1, c2, st); break;
    case OBB_DIOU_SMALLEST: launch_fwd<OBB_DIOU_SMALLEST>(b1, b2, n, iou, u3d, zr, loss, wc, hc, c1, c2, st); break;
    case OBB_DIOU_ALIGNED: launch_fwd<OBB_DIOU_ALIGNED>(b1, b2, n, iou, u3d, zr, loss, wc, hc, c1, c2, st); break;
    default: return -4;
  }
  NMH_CHECK_LAUNCH();
  return 0;
}

int k_obb_iou_bwd(int mode, const float* b1, const float* b2, long n, const float* gi, const float* gu, const float* gl, int g_one, float* d1, float* d2, hipStream_t st) {
  if (n <= 0 || (n + 255) / 256 >= (1L << 31)) return -4;
  switch (mode) {
    case OBB_IOU: launch_bwd<OBB_IOU>(b1, b2, n, gi, gu, gl, g_one, d1, d2, st); break;
    case OBB_GIOU_SMALLEST: launch_bwd<OBB_GIOU_SMALLEST>(b1, b2, n, gi, gu, gl, g_one, d1, d2, st); break;
    case OBB_GIOU_ALIGNED: launch_bwd<OBB_GIOU_ALIGNED>(b1, b2, n, gi, gu, gl, g_one, d1, d2, st); break;
    case OBB_DIOU_SMALLEST: launch_bwd<OBB_DIOU_SMALLEST>(b1, b2, n, gi, gu, gl, g_one, d1, d2, st); break;
    case OBB_DIOU_ALIGNED: launch_bwd<OBB_DIOU_ALIGNED>(b1, b2, n, gi, gu, gl, g_one, d1, d2, st); break;
    default: return -4;
  }
  NMH_CHECK_LAUNCH();
  return 0;
}

int k_obb_iou_pairwise(int ncols, const float* b1, const float* b2, int N, int M, float* iou, hipStream_t st) {
  if (N <= 0 || M <= 0 || (ncols != 6 && ncols != 7)) return -4;
  const long gy = ((long)N + PW_ROWS - 1) / PW_ROWS;
  if (gy > 65535) return -4;
  const dim3 grid((unsigned)((M + PW_COLS - 1) / PW_COLS), (unsigned)gy);
  if (ncols == 6) hipLaunchKernelGGL(obb_iou_pairwise_kernel<true>, grid, dim3(256), 0, st, b1, b2, N, M, iou);
  else hipLaunchKernelGGL(obb_iou_pairwise_kernel<false>, grid, dim3(256), 0, st, b1, b2, N, M, iou);
  NMH_CHECK_LAUNCH();
  return 0;
}

int k_obb_nms_mask(int ncols, const float* boxes, const int* cat, int N, float thr, unsigned long long* mask, hipStream_t st) {
  if (N <= 0 || N > NMH_OBB_NMS_MAX || (ncols != 6 && ncols != 7)) return -4;
  const unsigned nw = (unsigned)((N + 63) / 64);
  if (ncols == 6) hipLaunchKernelGGL(obb_nms_mask_kernel<true>, dim3(nw * (nw + 1) / 2), dim3(256), 0, st, boxes, cat, N, thr, mask);
  else hipLaunchKernelGGL(obb_nms_mask_kernel<false>, dim3(nw * (nw + 1) / 2), dim3(256), 0, st, boxes, cat, N, thr, mask);
  NMH_CHECK_LAUNCH();
  return 0;
}

int k_obb_nms_scan(const unsigned long long* mask, int N, int* keep, int* count, hipStream_t st) {
  if (N <= 0 || N > NMH_OBB_NMS_MAX) return -4;
  hipLaunchKernelGGL(obb_nms_scan_kernel, dim3(1), dim3(256), 0, st, mask, N, keep, count);
  NMH_CHECK_LAUNCH();
  return 0;
}

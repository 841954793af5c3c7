// Device functions of the oriented 3-D box pair geometry (IoU / GIoU / DIoU values and hand-written gradients), shared by rotated_iou.hip and
// fcos.hip.  Semantics and algorithm: the header comment of rotated_iou.hip.  Everything is __forceinline__ and lives in registers.
#pragma once
#include "common.hpp"

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

// loss of one pair in mode MODE (untouched in OBB_IOU mode) and, when asked for, the enclosing rectangle
template <int MODE>
__device__ __forceinline__ float obb_pair_loss(const Obb& A, const Obb& B, const PairOut& o, const float (&X)[8], const float (&Y)[8], Encl& E) {
  E = obb_enclosing<MODE == OBB_GIOU_SMALLEST || MODE == OBB_DIOU_SMALLEST>(X, Y);
  if (MODE == OBB_GIOU_SMALLEST || MODE == OBB_GIOU_ALIGNED) {
    const float vc = o.zr * E.w * E.h;
    return 1.f - o.iou + (vc - o.u3d) / vc;
  }
  const float dx = A.x - B.x, dy = A.y - B.y, dz = A.z - B.z;
  return 1.f - o.iou + (dx * dx + dy * dy + dz * dz) / (E.w * E.w + E.h * E.h + o.zr * o.zr);
}

// gradients of (gi_in iou + gu_in u3d + gl loss) of one pair with respect to box A (ga) and, if want_b, box B (gb); the geometry is recomputed
template <int MODE>
__device__ __forceinline__ void obb_pair_grad(const Obb& A, const Obb& B, float gi_in, float gu_in, float gl, bool want_b, BoxGrad& ga, BoxGrad& gb) {
  constexpr bool ENC = MODE != OBB_IOU, GIOU = MODE == OBB_GIOU_SMALLEST || MODE == OBB_GIOU_ALIGNED;
  constexpr bool SMALLEST = MODE == OBB_GIOU_SMALLEST || MODE == OBB_DIOU_SMALLEST;
  const PairOut o = obb_pair(A, B);
  ga = BoxGrad{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  gb = BoxGrad{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
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
    if (want_b) {
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
    if (want_b) obb_corner_grads_to_box(B, X, Y, Gx, Gy, 4, gb);
  }
}

// ---- a box staged in LDS for the all-pairs and NMS kernels (rotated_iou.hip, nms_bits.hpp), its sin / cos taken once ------------------------------
struct BoxTile { float v[8]; };   // 7 columns: x y z w l h cos sin; 6 columns: x1 y1 z1 x2 y2 z2
__device__ __forceinline__ void zero_box(BoxTile& dst) {
#pragma unroll
  for (int k = 0; k < 8; ++k) dst.v[k] = 0.f;
}
// row i of src (rows of `stride` floats, the box in the first 6 | 7), zeros for i >= n
template <bool AABB>
__device__ __forceinline__ void stage_box(const float* __restrict__ src, long i, long n, BoxTile& dst, int stride = AABB ? 6 : 7) {
  if (i >= n) return zero_box(dst);
  if (AABB) {
#pragma unroll
    for (int k = 0; k < 6; ++k) dst.v[k] = src[i * stride + k];
    dst.v[6] = dst.v[7] = 0.f;
  } else {
    const Obb o = obb_load(src + i * stride);
    dst.v[0] = o.x; dst.v[1] = o.y; dst.v[2] = o.z; dst.v[3] = o.w; dst.v[4] = o.l; dst.v[5] = o.h; dst.v[6] = o.cs; dst.v[7] = o.sn;
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

}  // namespace

// The 2-D projection regression term of the reference's two detectors as device functions, shared by the row operator (proj2d.hip) and by the fused losses
// of rpn.hip and fcos.hip:
//   cameras   get_w2cs(res) (nerf_rpn/model/rpn.py:58-85, identical in fcos/utils.py:300-353): centroid c = (res/2, res/2, res/2), four positions
//             c + (+-res, +-res, res) in the order (+,+), (+,-), (-,+), (-,-), rotation look_at_rotation(pos, at = c, up = (0, 0, 1)) with columns x, y, z
//             (z = normalize(pos - c), x = normalize(cross(up, z)), y = normalize(cross(z, x))), c2w = [R | pos], w2c = its inverse, and the intrinsics
//             K = [[600, 0, 320], [0, 600, 240], [0, 0, 1]] (rpn.py:422-423).  A camera travels as the ONE 3x4 matrix K [R^T | -R^T pos], formed in
//             float64 on the host and rounded to fp32 once (the reference rounds w2c and multiplies by K in fp32);
//   project   (rpn.py:88-102): (a, b, d) = M (x, y, z, 1), uv = (a / d, b / d); no clamp and no sign test on the depth;
//   points    two opposite corners of a box: 6 columns (x0, y0, z0), (x1, y1, z1); 7 columns (obb2points_3d, fcos/utils.py:373-379) centre -+ v with
//             v = (w/2 cos - l/2 sin, w/2 sin + l/2 cos, h/2);
//   term      T = sum over 4 cameras, 2 points and 2 coordinates of smooth_l1(uv_pred - uv_target; beta 1/9) (rpn.py:446-452, fcos/loss.py:463-470).
// Plain fp32, free to contract; one lane owns one pair of boxes; nothing but the caller's registers is written.
#pragma once
#include "obb_geom.hpp"
#include "rpn_shared.hpp"

struct Proj2dCams { float m[4][12]; };          // kernel argument, by value: K [R^T | -R^T pos] of the four cameras, row-major 3x4

namespace {

// HOST: the four cameras of get_w2cs(res), in float64
inline void proj2d_make_cams(double res, Proj2dCams& C) {
  const double c = res / 2, sg[4][2] = {{1, 1}, {1, -1}, {-1, 1}, {-1, -1}};
  for (int k = 0; k < 4; ++k) {
    const double pos[3] = {c + sg[k][0] * res, c + sg[k][1] * res, c + res};
    double z[3] = {pos[0] - c, pos[1] - c, pos[2] - c};
    const double nz = sqrt(z[0] * z[0] + z[1] * z[1] + z[2] * z[2]);
    for (double& v : z) v /= nz;
    double x[3] = {-z[1], z[0], 0.0};            // cross((0, 0, 1), z)
    const double nx = sqrt(x[0] * x[0] + x[1] * x[1]);
    for (double& v : x) v /= nx;
    double y[3] = {z[1] * x[2] - z[2] * x[1], z[2] * x[0] - z[0] * x[2], z[0] * x[1] - z[1] * x[0]};
    const double ny = sqrt(y[0] * y[0] + y[1] * y[1] + y[2] * y[2]);
    for (double& v : y) v /= ny;
    const double* R[3] = {x, y, z};              // the rows of R^T
    double w2c[3][4];
    for (int i = 0; i < 3; ++i) {
      w2c[i][3] = 0.0;
      for (int j = 0; j < 3; ++j) { w2c[i][j] = R[i][j]; w2c[i][3] -= R[i][j] * pos[j]; }
    }
    for (int j = 0; j < 4; ++j) {
      C.m[k][j] = (float)(600.0 * w2c[0][j] + 320.0 * w2c[2][j]);
      C.m[k][4 + j] = (float)(600.0 * w2c[1][j] + 240.0 * w2c[2][j]);
      C.m[k][8 + j] = (float)w2c[2][j];
    }
  }
}

struct P2Pts { float p[2][3]; };

__device__ __forceinline__ P2Pts proj2d_points(const float (&b)[6]) {
  P2Pts q;
#pragma unroll
  for (int k = 0; k < 3; ++k) { q.p[0][k] = b[k]; q.p[1][k] = b[3 + k]; }
  return q;
}
__device__ __forceinline__ P2Pts proj2d_points(const Obb& o) {
  const float vx = 0.5f * o.w * o.cs - 0.5f * o.l * o.sn, vy = 0.5f * o.w * o.sn + 0.5f * o.l * o.cs, vz = 0.5f * o.h;
  P2Pts q;
  q.p[0][0] = o.x - vx; q.p[0][1] = o.y - vy; q.p[0][2] = o.z - vz;
  q.p[1][0] = o.x + vx; q.p[1][1] = o.y + vy; q.p[1][2] = o.z + vz;
  return q;
}

// One point of prediction (p) and target (t) under one camera: the differences (du, dv) of their pixel coordinates, the prediction's pixel (up, vp) and
// ip = 1 / its depth.  With (a, b, d) = M (x, y, z, 1):  a_p / d_p - a_t / d_t = ((a_p - a_t) - u_t (d_p - d_t)) / d_p, and a_p - a_t = M[0][:3] (p - t): the
// difference is formed from p - t, not from two pixel coordinates of 1e2 .. 1e3, so it keeps its relative accuracy when the two boxes are close, and it is
// exactly 0 for identical points.
struct P2Proj { float du, dv, up, vp, ip; };
__device__ __forceinline__ P2Proj proj2d_project(const float (&m)[12], const float (&p)[3], const float (&t)[3]) {
  const float e[3] = {p[0] - t[0], p[1] - t[1], p[2] - t[2]};
  const float at = m[0] * t[0] + m[1] * t[1] + m[2] * t[2] + m[3], bt = m[4] * t[0] + m[5] * t[1] + m[6] * t[2] + m[7], dt = m[8] * t[0] + m[9] * t[1] + m[10] * t[2] + m[11];
  const float da = m[0] * e[0] + m[1] * e[1] + m[2] * e[2], db = m[4] * e[0] + m[5] * e[1] + m[6] * e[2], dd = m[8] * e[0] + m[9] * e[1] + m[10] * e[2];
  const float ut = at / dt, vt = bt / dt;
  P2Proj q;
  q.ip = 1.f / (dt + dd);
  q.du = (da - ut * dd) * q.ip; q.dv = (db - vt * dd) * q.ip;
  q.up = ut + q.du; q.vp = vt + q.dv;
  return q;
}

__device__ __forceinline__ float proj2d_term_pts(const P2Pts& P, const P2Pts& T, const Proj2dCams& C) {
  float sum = 0.f;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const P2Proj q = proj2d_project(C.m[c], P.p[k], T.p[k]);
      sum += rpn_sl1(q.du) + rpn_sl1(q.dv);
    }
  }
  return sum;
}
// d T / d (the two points of the prediction): through the smooth-L1, the quotient and the matrix
__device__ __forceinline__ void proj2d_term_pts_grad(const P2Pts& P, const P2Pts& T, const Proj2dCams& C, float (&g)[2][3]) {
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    g[k][0] = g[k][1] = g[k][2] = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float (&m)[12] = C.m[c];
      const P2Proj q = proj2d_project(m, P.p[k], T.p[k]);
      const float gu = rpn_sl1_grad(q.du) * q.ip, gv = rpn_sl1_grad(q.dv) * q.ip;       // u = a / d: du/da = 1/d, du/dd = -u/d
#pragma unroll
      for (int j = 0; j < 3; ++j) g[k][j] += gu * (m[j] - q.up * m[8 + j]) + gv * (m[4 + j] - q.vp * m[8 + j]);
    }
  }
}

// T of a pair of boxes and its gradient over the prediction: 6 box columns ...
__device__ __forceinline__ float proj2d_term(const float (&pred)[6], const float (&target)[6], const Proj2dCams& C) {
  return proj2d_term_pts(proj2d_points(pred), proj2d_points(target), C);
}
__device__ __forceinline__ void proj2d_term_grad(const float (&pred)[6], const float (&target)[6], const Proj2dCams& C, float (&g)[6]) {
  float gp[2][3];
  proj2d_term_pts_grad(proj2d_points(pred), proj2d_points(target), C, gp);
#pragma unroll
  for (int k = 0; k < 3; ++k) { g[k] = gp[0][k]; g[3 + k] = gp[1][k]; }
}
// ... or oriented boxes, the gradient over (x, y, z, w, l, h, theta): the points are centre -+ v, d v / d theta = (-vy, vx, 0)
__device__ __forceinline__ float proj2d_term(const Obb& pred, const Obb& target, const Proj2dCams& C) {
  return proj2d_term_pts(proj2d_points(pred), proj2d_points(target), C);
}
__device__ __forceinline__ void proj2d_term_grad(const Obb& pred, const Obb& target, const Proj2dCams& C, BoxGrad& g) {
  float gp[2][3];
  proj2d_term_pts_grad(proj2d_points(pred), proj2d_points(target), C, gp);
  const float gvx = gp[1][0] - gp[0][0], gvy = gp[1][1] - gp[0][1], gvz = gp[1][2] - gp[0][2];
  const float vx = 0.5f * pred.w * pred.cs - 0.5f * pred.l * pred.sn, vy = 0.5f * pred.w * pred.sn + 0.5f * pred.l * pred.cs;
  g.x = gp[0][0] + gp[1][0]; g.y = gp[0][1] + gp[1][1]; g.z = gp[0][2] + gp[1][2];
  g.w = 0.5f * (gvx * pred.cs + gvy * pred.sn);
  g.l = 0.5f * (gvy * pred.cs - gvx * pred.sn);
  g.h = 0.5f * gvz;
  g.t = gvy * vx - gvx * vy;
}

}  // namespace

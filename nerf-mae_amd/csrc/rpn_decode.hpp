// The two box decoders of the reference's RPN as device functions over an anchor (Box6 of rpn_geom.hpp) and its C regression values, shared by the
// kernels of rpn_post.hip (and meant for the differentiable decode that the IoU-type regression losses need):
//   rpn_decode_aabb   AABBCoder.decode_single (coder/AABB_coder.py:86-137): C = 6 -> (x0, y0, z0, x1, y1, z1), not clipped;
//   rpn_decode_obb    MidpointOffsetCoder.decode_single = delta_sp2bbox (coder/midpoint_offset_coder.py:160-223, wh_ratio_clip 16/1000) with rectpoly2obb
//                     and regular_obb (coder/misc.py:5-43): C = 8 -> (x, y, z, w, h, d, theta), not clipped.
// fp32, the reference's order of operations, no contraction (a multiply and an add stay two roundings, as in the reference's tensor arithmetic).
// Non-finite deltas give unspecified values; nothing but the caller's registers is written.
#pragma once
#include "rpn_geom.hpp"

namespace {

constexpr float RPN_XFORM_CLIP = 7.600902459542082f;       // log(2000)
constexpr float RPN_RATIO_CLIP = 4.135166556742356f;       // |log(16 / 1000)|
constexpr float RPN_REF_PI = 3.141592f;                    // the reference's own constant (coder/misc.py:3), on purpose

__device__ __forceinline__ void rpn_decode_aabb(const float (&r)[8], const Box6& a, float (&o)[7]) {
#pragma clang fp contract(off)
  const float w = a.x1 - a.x0, h = a.y1 - a.y0, d = a.z1 - a.z0;
  const float cx = a.x0 + 0.5f * w, cy = a.y0 + 0.5f * h, cz = a.z0 + 0.5f * d;
  const float dw = fminf(r[3], RPN_XFORM_CLIP), dh = fminf(r[4], RPN_XFORM_CLIP), dd = fminf(r[5], RPN_XFORM_CLIP);
  const float px = r[0] * w + cx, py = r[1] * h + cy, pz = r[2] * d + cz;
  const float hw = 0.5f * (expf(dw) * w), hh = 0.5f * (expf(dh) * h), hd = 0.5f * (expf(dd) * d);
  o[0] = px - hw; o[1] = py - hh; o[2] = pz - hd; o[3] = px + hw; o[4] = py + hh; o[5] = pz + hd;
  o[6] = 0.f;
}

__device__ __forceinline__ float rpn_clamp(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

__device__ __forceinline__ void rpn_decode_obb(const float (&r)[8], const Box6& a, float (&o)[7]) {
#pragma clang fp contract(off)
  const float dw = rpn_clamp(r[3], -RPN_RATIO_CLIP, RPN_RATIO_CLIP), dh = rpn_clamp(r[4], -RPN_RATIO_CLIP, RPN_RATIO_CLIP), dd = rpn_clamp(r[5], -RPN_RATIO_CLIP, RPN_RATIO_CLIP);
  const float px = (a.x0 + a.x1) * 0.5f, py = (a.y0 + a.y1) * 0.5f, pz = (a.z0 + a.z1) * 0.5f;
  const float pw = a.x1 - a.x0, ph = a.y1 - a.y0, pd = a.z1 - a.z0;
  const float gw = pw * expf(dw), gh = ph * expf(dh), gd = pd * expf(dd);
  const float gx = px + pw * r[0], gy = py + ph * r[1], gz = pz + pd * r[2];
  const float x1 = gx - gw * 0.5f, y1 = gy - gh * 0.5f, x2 = gx + gw * 0.5f, y2 = gy + gh * 0.5f;
  const float da = rpn_clamp(r[6], -0.5f, 0.5f), db = rpn_clamp(r[7], -0.5f, 0.5f);
  // the four midpoints (ga, y1), (x2, gb), (_ga, y2), (x1, _gb) about the centre, scaled to the longest half-diagonal
  float X[4] = {(gx + da * gw) - gx, x2 - gx, (gx - da * gw) - gx, x1 - gx};
  float Y[4] = {y1 - gy, (gy + db * gh) - gy, y2 - gy, (gy - db * gh) - gy};
  float len[4], mx = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) { len[k] = sqrtf(X[k] * X[k] + Y[k] * Y[k]); mx = fmaxf(mx, len[k]); }
#pragma unroll
  for (int k = 0; k < 4; ++k) { const float s = mx / len[k]; X[k] = X[k] * s + gx; Y[k] = Y[k] * s + gy; }
  // rectpoly2obb
  float th = atan2f(-(Y[1] - Y[0]), X[1] - X[0] + 1e-7f);
  const float cs = cosf(th), sn = sinf(th);
  const float x = (X[0] + X[1] + X[2] + X[3]) / 4.f, y = (Y[0] + Y[1] + Y[2] + Y[3]) / 4.f;
  float xl = 3.0e38f, xh = -3.0e38f, yl = 3.0e38f, yh = -3.0e38f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float ux = X[k] - x, uy = Y[k] - y;
    const float rx = ux * cs + uy * -sn, ry = ux * sn + uy * cs;
    xl = fminf(xl, rx); xh = fmaxf(xh, rx); yl = fminf(yl, ry); yh = fmaxf(yh, ry);
  }
  const float w = xh - xl, h = yh - yl;
  // regular_obb: the longer side first, theta into [-pi/2, pi/2) by the floor modulo
  const bool keep = w > h;
  th = keep ? th : th + RPN_REF_PI / 2.f;
  float m = fmodf(th - (-RPN_REF_PI / 2.f), RPN_REF_PI);
  if (m < 0.f) m += RPN_REF_PI;
  o[0] = x; o[1] = y; o[2] = gz; o[3] = keep ? w : h; o[4] = keep ? h : w; o[5] = gd; o[6] = m + (-RPN_REF_PI / 2.f);
}

}  // namespace

// The two box decoders of the reference's RPN as device functions over an anchor (Box6 of rpn_geom.hpp) and its C regression values, shared by the
// kernels of rpn_post.hip and by the IoU-type regression losses of rpn.hip, which differentiate the oriented one:
//   rpn_decode_aabb     AABBCoder.decode_single (coder/AABB_coder.py:86-137): C = 6 -> (x0, y0, z0, x1, y1, z1), not clipped;
//   rpn_decode_obb      MidpointOffsetCoder.decode_single = delta_sp2bbox (coder/midpoint_offset_coder.py:160-223, wh_ratio_clip 16/1000) with rectpoly2obb
//                       and regular_obb (coder/misc.py:5-43): C = 8 -> (x, y, z, w, h, d, theta), not clipped;
//   rpn_decode_obb_bwd  its hand-written backward (what autograd does for the reference): conventions at the function;
//   rpn_decode_aabb_bwd the backward of rpn_decode_aabb, for the 2-D projection term of the axis-aligned RPN.
// fp32; the forwards keep the reference's order of operations, no contraction (a multiply and an add stay two roundings, as in the reference's tensor
// arithmetic).  Non-finite deltas give unspecified values; nothing but the caller's registers is written.
#pragma once
#include "rpn_geom.hpp"
#include "obb_geom.hpp"

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

// 1 where a clamp to [lo, hi] passes the gradient (lo <= v <= hi, as torch.clamp), else 0
__device__ __forceinline__ float rpn_clamp_pass(float v, float lo, float hi) { return v >= lo && v <= hi ? 1.f : 0.f; }

// Backward of rpn_decode_aabb: the gradient g over (x0, y0, z0, x1, y1, z1) -> gr, the gradient over the 6 deltas (gr[6], gr[7] = 0).  The clip of the size
// deltas to log(2000) passes the gradient where v <= log(2000), as torch.clamp(max=) does.
__device__ __forceinline__ void rpn_decode_aabb_bwd(const float (&r)[8], const Box6& a, const float (&g)[6], float (&gr)[8]) {
  const float e[3] = {a.x1 - a.x0, a.y1 - a.y0, a.z1 - a.z0};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    gr[k] = (g[k] + g[3 + k]) * e[k];
    gr[3 + k] = (g[3 + k] - g[k]) * 0.5f * expf(fminf(r[3 + k], RPN_XFORM_CLIP)) * e[k] * rpn_clamp_pass(r[3 + k], -INFINITY, RPN_XFORM_CLIP);
  }
  gr[6] = gr[7] = 0.f;
}

// Backward of rpn_decode_obb: the gradient g over (x, y, z, w, h, d, theta) of the decoded box -> gr, the gradient over the 8 deltas.  The forward is
// recomputed about the centre (gx, gy), in fp32 and free to contract: only the forward is bound to the reference's rounding.
//   - a clamp passes the gradient where lo <= v <= hi and gives 0 outside;
//   - the centre is (gx, gy): the four scaled midpoints are P, Q, -P, -Q, so their mean is the centre identically and its gradient goes to gx, gy alone;
//   - the longest half-diagonal is a tie between identical functions (len[0] = len[2], len[1] = len[3]), and so are the extremes over the four rotated
//     corners (the scaled polygon is a rectangle): each goes to the FIRST index that attains it, which is the same derivative as any other routing;
//   - the w > h swap exchanges the two side gradients, theta's passes 1:1 through the swap's constant and through the floor modulo; a box on the swap's
//     or the modulo's boundary is the same box on either side, so a decision that differs from the forward kernel's in its last bit changes nothing;
//   - the 1e-7 of atan2's second argument stays.
__device__ __forceinline__ void rpn_decode_obb_bwd(const float (&r)[8], const Box6& a, const BoxGrad& g, float (&gr)[8]) {
  const float dw = rpn_clamp(r[3], -RPN_RATIO_CLIP, RPN_RATIO_CLIP), dh = rpn_clamp(r[4], -RPN_RATIO_CLIP, RPN_RATIO_CLIP), dd = rpn_clamp(r[5], -RPN_RATIO_CLIP, RPN_RATIO_CLIP);
  const float pw = a.x1 - a.x0, ph = a.y1 - a.y0, pd = a.z1 - a.z0;
  const float gw = pw * expf(dw), gh = ph * expf(dh), gd = pd * expf(dd);
  const float da = rpn_clamp(r[6], -0.5f, 0.5f), db = rpn_clamp(r[7], -0.5f, 0.5f);
  const float Xo[4] = {da * gw, 0.5f * gw, -da * gw, -0.5f * gw}, Yo[4] = {-0.5f * gh, db * gh, 0.5f * gh, -db * gh};
  float len[4], mx = 0.f;
  int kmax = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    len[k] = sqrtf(Xo[k] * Xo[k] + Yo[k] * Yo[k]);
    if (len[k] > mx) { mx = len[k]; kmax = k; }
  }
  float U[4], V[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) { const float s = mx / len[k]; U[k] = Xo[k] * s; V[k] = Yo[k] * s; }
  const float ny = -(V[1] - V[0]), nx = U[1] - U[0] + 1e-7f, n2 = nx * nx + ny * ny;
  const float th = atan2f(ny, nx), cs = cosf(th), sn = sinf(th);
  float rx[4], ry[4];
  int ixh = 0, ixl = 0, iyh = 0, iyl = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) { rx[k] = U[k] * cs - V[k] * sn; ry[k] = U[k] * sn + V[k] * cs; }
  float xh = rx[0], xl = rx[0], yh = ry[0], yl = ry[0], ry_xh = ry[0], ry_xl = ry[0], rx_yh = rx[0], rx_yl = rx[0];
#pragma unroll
  for (int k = 1; k < 4; ++k) {
    if (rx[k] > xh) { xh = rx[k]; ry_xh = ry[k]; ixh = k; }
    if (rx[k] < xl) { xl = rx[k]; ry_xl = ry[k]; ixl = k; }
    if (ry[k] > yh) { yh = ry[k]; rx_yh = rx[k]; iyh = k; }
    if (ry[k] < yl) { yl = ry[k]; rx_yl = rx[k]; iyl = k; }
  }
  const bool keep = xh - xl > yh - yl;
  const float gW = keep ? g.w : g.l, gH = keep ? g.l : g.w;
  // w = rx[ixh] - rx[ixl], h = ry[iyh] - ry[iyl];  d rx / d theta = -ry, d ry / d theta = rx
  const float gth = g.t - gW * (ry_xh - ry_xl) + gH * (rx_yh - rx_yl);
  const float tu = -gth * ny / n2, tv = -gth * nx / n2;     // theta's gradient over U[1] - U[0] and V[1] - V[0]
  float gXo[4], gYo[4], gmx = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float sw = (float)(k == ixh) - (float)(k == ixl), sh = (float)(k == iyh) - (float)(k == iyl), st = (float)(k == 1) - (float)(k == 0);
    const float gu = gW * sw * cs + gH * sh * sn + tu * st, gv = -gW * sw * sn + gH * sh * cs + tv * st;
    const float s = mx / len[k], gs = gu * Xo[k] + gv * Yo[k];        // U = Xo s, V = Yo s, s = mx / len
    gmx += gs / len[k];
    const float gl = -gs * s / len[k];
    gXo[k] = gu * s + gl * Xo[k] / len[k];
    gYo[k] = gv * s + gl * Yo[k] / len[k];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k == kmax) { gXo[k] += gmx * Xo[k] / len[k]; gYo[k] += gmx * Yo[k] / len[k]; }
  }
  const float ax = gXo[0] - gXo[2], bx = gXo[1] - gXo[3], ay = gYo[2] - gYo[0], by = gYo[1] - gYo[3];
  const float ggw = ax * da + 0.5f * bx, ggh = by * db + 0.5f * ay;
  gr[0] = g.x * pw; gr[1] = g.y * ph; gr[2] = g.z * pd;
  gr[3] = ggw * gw * rpn_clamp_pass(r[3], -RPN_RATIO_CLIP, RPN_RATIO_CLIP);
  gr[4] = ggh * gh * rpn_clamp_pass(r[4], -RPN_RATIO_CLIP, RPN_RATIO_CLIP);
  gr[5] = g.h * gd * rpn_clamp_pass(r[5], -RPN_RATIO_CLIP, RPN_RATIO_CLIP);
  gr[6] = ax * gw * rpn_clamp_pass(r[6], -0.5f, 0.5f);
  gr[7] = by * gh * rpn_clamp_pass(r[7], -0.5f, 0.5f);
}

}  // namespace

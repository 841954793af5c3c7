// decode_fcos_obb (nerf_rpn/model/fcos/utils.py:12-61) on the device, shared by the training losses (fcos.hip) and the inference
// post-processing (fcos_post.hip).  Semantics: the header of fcos.hip.
#pragma once
#include "obb_geom.hpp"

namespace {

// decode at a zero location, with what the backward needs
struct Dec { Obb o; float x0, x1, y0, y1, vxr, vyr, v0x, v0y, v1x, v1y, d0, d1, dmax, mx, my, n, ex, ey, el, r6, r7; };
__device__ __forceinline__ Dec fcos_decode(const float (&r)[8]) {
  Dec d;
  d.x0 = -r[0]; d.y0 = -r[1]; d.x1 = r[3]; d.y1 = r[4];
  const float z0 = -r[2], z1 = r[5];
  d.r6 = r[6]; d.r7 = r[7];
  d.vxr = (d.x1 + d.x0) / 2.f + r[6] * (d.x1 - d.x0);
  d.vyr = (d.y1 + d.y0) / 2.f + r[7] * (d.y1 - d.y0);
  const float vx = fminf(fmaxf(d.vxr, d.x0), d.x1), vy = fminf(fmaxf(d.vyr, d.y0), d.y1);
  const float cx = (d.x0 + d.x1) / 2.f, cy = (d.y0 + d.y1) / 2.f;
  d.v0x = vx - cx; d.v0y = d.y1 - cy; d.v1x = d.x1 - cx; d.v1y = vy - cy;
  d.d0 = sqrtf(d.v0x * d.v0x + d.v0y * d.v0y); d.d1 = sqrtf(d.v1x * d.v1x + d.v1y * d.v1y);
  d.dmax = fmaxf(d.d0, d.d1);
  const float s0 = d.dmax / (d.d0 + 1e-7f), s1 = d.dmax / (d.d1 + 1e-7f);
  const float a0x = d.v0x * s0, a0y = d.v0y * s0, a1x = d.v1x * s1, a1y = d.v1y * s1;
  d.ex = a0x - a1x; d.ey = a0y - a1y;
  d.el = sqrtf(d.ex * d.ex + d.ey * d.ey);
  d.mx = 0.5f * (a0x + a1x); d.my = 0.5f * (a0y + a1y);
  d.n = sqrtf(d.mx * d.mx + d.my * d.my);
  d.o.x = cx; d.o.y = cy; d.o.z = (z0 + z1) / 2.f;
  d.o.w = 2.f * d.n; d.o.l = d.el; d.o.h = z1 - z0;
  const bool zero = d.mx == 0.f && d.my == 0.f;
  d.o.cs = zero ? 1.f : d.mx / d.n;
  d.o.sn = zero ? 0.f : d.my / d.n;
  return d;
}

}  // namespace

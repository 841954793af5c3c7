// The box decode of the RoI stage, shared by roi_head.hip (roi_decode) and roi_post.hip (roi_post_select): RotatedCoder.decode_single
// (coder/rotated_coder.py:57-121) and AABBCoder.decode_single (coder/AABB_coder.py:86-137).  d: the 6 | 7 deltas, e: the RoI's box, o: the decoded box.
// dw, dh, dd are clipped at log(2000); the angle is wrapped into (-pi/2, pi/2].
#pragma once
#include "common.hpp"

template <bool ORIENTED>
__device__ __forceinline__ void roi_decode_box(const float* __restrict__ d, const float* __restrict__ e, float* __restrict__ o) {
  constexpr float CLIP = 7.600902459542082f, PI = 3.14159265358979323846f;      // log(2000)
  const float dw = fminf(d[3], CLIP), dh = fminf(d[4], CLIP), dd = fminf(d[5], CLIP);
  if (ORIENTED) {
    const float cs = cosf(e[6]), sn = sinf(e[6]);
    o[0] = d[0] * e[3] * cs - d[1] * e[4] * sn + e[0];
    o[1] = d[0] * e[3] * sn + d[1] * e[4] * cs + e[1];
    o[2] = d[2] * e[5] + e[2];
    o[3] = expf(dw) * e[3]; o[4] = expf(dh) * e[4]; o[5] = expf(dd) * e[5];
    float a = fmodf(2.f * PI * d[6] + e[6], PI);       // Python's %: the result has the sign of the divisor
    if (a < 0.f) a += PI;
    o[6] = a > PI / 2.f ? a - PI : a;
  } else {
    const float w = e[3] - e[0], h = e[4] - e[1], dp = e[5] - e[2];
    const float cx = d[0] * w + (e[0] + 0.5f * w), cy = d[1] * h + (e[1] + 0.5f * h), cz = d[2] * dp + (e[2] + 0.5f * dp);
    const float hw = 0.5f * (expf(dw) * w), hh = 0.5f * (expf(dh) * h), hd = 0.5f * (expf(dd) * dp);
    o[0] = cx - hw; o[1] = cy - hh; o[2] = cz - hd; o[3] = cx + hw; o[4] = cy + hh; o[5] = cz + hd;
  }
}

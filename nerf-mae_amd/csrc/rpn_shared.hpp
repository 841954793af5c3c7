// Device code shared by the two stages of the anchor-based detector (rpn.hip: first stage, roi_head.hip: second stage): the axis-aligned IoU, the
// AABBCoder encode, the counter-based hash of the samplers with the launch that advances its counter, and the smooth-L1 of the box losses.
#pragma once
#include "common.hpp"
#include "rpn_geom.hpp"

namespace {

// the one IoU of both passes: no contraction, so the same inputs give the same bits in either kernel
__device__ __forceinline__ float rpn_iou(const Box6& g, const Box6& a) {
#pragma clang fp contract(off)
  const float w = fmaxf(fminf(g.x1, a.x1) - fmaxf(g.x0, a.x0), 0.f);
  const float h = fmaxf(fminf(g.y1, a.y1) - fmaxf(g.y0, a.y0), 0.f);
  const float d = fmaxf(fminf(g.z1, a.z1) - fmaxf(g.z0, a.z0), 0.f);
  const float inter = w * h * d;
  const float uni = g.vol + a.vol - inter;
  const float iou = inter / uni;
  return iou > 0.f ? iou : 0.f;              // 0 / 0, -0 and malformed boxes: no overlap, with the bits of +0
}

__device__ __forceinline__ void rpn_encode_aabb(const float* __restrict__ g, const Box6& a, float (&o)[8]) {
  const float ew = a.x1 - a.x0, eh = a.y1 - a.y0, ed = a.z1 - a.z0;
  const float ex = a.x0 + 0.5f * ew, ey = a.y0 + 0.5f * eh, ez = a.z0 + 0.5f * ed;
  const float gw = g[3] - g[0], gh = g[4] - g[1], gd = g[5] - g[2];
  const float gx = g[0] + 0.5f * gw, gy = g[1] + 0.5f * gh, gz = g[2] + 0.5f * gd;
  o[0] = (gx - ex) / ew; o[1] = (gy - ey) / eh; o[2] = (gz - ez) / ed;
  o[3] = logf(gw / ew); o[4] = logf(gh / eh); o[5] = logf(gd / ed);
  o[6] = o[7] = 0.f;
}

// ---- the samplers' hash: a stream per (seed, counter, scene), a key per index -------------------------------------------------------------
__device__ __forceinline__ unsigned long long rpn_mix64(unsigned long long x) {      // the splitmix64 finaliser
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27; x *= 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
__device__ __forceinline__ unsigned long long rpn_stream(long seed, long counter, int scene) {
  return rpn_mix64(rpn_mix64((unsigned long long)seed + 0x9E3779B97F4A7C15ull * ((unsigned long long)counter + 1ull)) ^ ((unsigned long long)(scene + 1) << 40));
}
// complemented hash: the largest of these are the smallest keys
__device__ __forceinline__ unsigned rpn_key(unsigned long long stream, int idx) { return ~(unsigned)(rpn_mix64(stream + (unsigned long long)idx * 0xD1342543DE82EF95ull) >> 32); }
__global__ void rpn_rng_advance_kernel(long* __restrict__ rng) {
  if (threadIdx.x == 0 && blockIdx.x == 0) rng[1] = rng[1] + 1;
}


constexpr float RPN_BETA = 1.f / 9.f;
__device__ __forceinline__ float rpn_sl1(float d) { const float a = fabsf(d); return a < RPN_BETA ? 0.5f * d * d / RPN_BETA : a - 0.5f * RPN_BETA; }
__device__ __forceinline__ float rpn_sl1_grad(float d) { return fabsf(d) < RPN_BETA ? d / RPN_BETA : (d > 0.f ? 1.f : -1.f); }

}  // namespace

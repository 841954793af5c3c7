// Level geometry of the RPN kernels (rpn.hip, rpn_post.hip): the by-value kernel arguments, the workgroup -> (level, scene, anchor) map (level_item of
// levels4.hpp with the anchor's bound), the anchor derived from its index with the padding test, and the host-side builders of the arguments (the per-level
// pointer plumbing: levels4.hpp).  Layouts and semantics: the header of rpn.hip.
#pragma once
#include "common.hpp"
#include "kernels.hpp"
#include "levels4.hpp"

namespace {

constexpr int RPN_MAX_A = NMH_RPN_MAX_ANCHORS;

struct RpnGeom {             // kernel argument, by value
  int L, N;
  int W[4], H[4], D[4], sx[4], sy[4], sz[4], A[4];
  int nloc[4], n[4], off[4]; // locations, anchors, first anchor of the level within a scene
  int blk0[4], bps[4];       // first workgroup of the level, workgroups per scene
  int ntot, nblocks;
};
struct RpnBase { float h[4][RPN_MAX_A][3]; };       // kernel argument, by value: half extents

struct RAt { int lvl, scene, i; bool active; };
__device__ __forceinline__ RAt rpn_where(const RpnGeom& G) {
  const LevelItem at = level_item(G.blk0, G.bps, G.L);
  return RAt{at.lvl, at.scene, at.i, at.i < pick4(G.n, at.lvl)};
}

struct Box6 { float x0, y0, z0, x1, y1, z1, vol; };

// the level's half extents -> LDS (the workgroup is within one level)
__device__ __forceinline__ void rpn_stage_base(const RpnBase& B, int lvl, int A, float* __restrict__ sh) {
  const float* __restrict__ src = &B.h[0][0][0] + lvl * RPN_MAX_A * 3;
  for (int k = threadIdx.x; k < A * 3; k += 256) sh[k] = src[k];
}

// anchor i of the level (anchor order) and whether it lies within the scene's original size
__device__ __forceinline__ Box6 rpn_anchor(const RpnGeom& G, const float* __restrict__ sh_base, const int* __restrict__ ori, const RAt& q, bool& valid) {
  const int A = pick4(G.A, q.lvl), Dk = pick4(G.D, q.lvl), Hk = pick4(G.H, q.lvl);
  const int sx = pick4(G.sx, q.lvl), sy = pick4(G.sy, q.lvl), sz = pick4(G.sz, q.lvl);
  const int i = q.active ? q.i : 0;
  const int a = i % A, loc = i / A, d = loc % Dk, h = (loc / Dk) % Hk, w = loc / (Dk * Hk);
  const float cx = (float)(w * sx), cy = (float)(h * sy), cz = (float)(d * sz);
  const float hx = sh_base[a * 3], hy = sh_base[a * 3 + 1], hz = sh_base[a * 3 + 2];
  Box6 b;
  b.x0 = cx - hx; b.y0 = cy - hy; b.z0 = cz - hz; b.x1 = cx + hx; b.y1 = cy + hy; b.z1 = cz + hz;
  b.vol = (b.x1 - b.x0) * (b.y1 - b.y0) * (b.z1 - b.z0);
  valid = q.active;
  if (ori) {
    const int ox = ori[q.scene * 3], oy = ori[q.scene * 3 + 1], oz = ori[q.scene * 3 + 2];
    valid = valid && w < (ox + sx - 1) / sx && h < (oy + sy - 1) / sy && d < (oz + sz - 1) / sz;
  }
  return b;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
// dims: [nlevels][7] = (W, H, D, sx, sy, sz, A)
int make_geom(int nlevels, const int* dims, int N, RpnGeom& G) {
  if (nlevels < 1 || nlevels > 4 || N < 1 || N > NMH_FCOS_MAX_SCENES || !dims) return -4;
  G.L = nlevels; G.N = N;
  long blocks = 0, off = 0;
  for (int k = 0; k < 4; ++k) {
    const int* d = dims + 7 * (k < nlevels ? k : nlevels - 1);
    for (int j = 0; j < 7; ++j) if (d[j] < 1) return -4;
    if (d[6] > RPN_MAX_A) return -4;
    const long nloc = (long)d[0] * d[1] * d[2], n = nloc * d[6];
    if (nloc > (1L << 28) || n > (1L << 30)) return -4;
    G.W[k] = d[0]; G.H[k] = d[1]; G.D[k] = d[2]; G.sx[k] = d[3]; G.sy[k] = d[4]; G.sz[k] = d[5]; G.A[k] = d[6];
    if ((long)d[0] * d[3] >= (1L << 24) || (long)d[1] * d[4] >= (1L << 24) || (long)d[2] * d[5] >= (1L << 24)) return -4;   // centres are exact in fp32
    G.nloc[k] = (int)nloc; G.n[k] = (int)n;
    G.bps[k] = (int)((n + 255) / 256);
    G.blk0[k] = (int)blocks; G.off[k] = (int)off;
    if (k < nlevels) { blocks += (long)G.bps[k] * N; off += n; }
    if (blocks >= (1L << 31) - 1 || off > (1L << 30)) return -4;
  }
  G.ntot = (int)off; G.nblocks = (int)blocks;
  return 0;
}
// base: [sum over levels of A][3] half extents, level by level
int make_base(int nlevels, const int* dims, const float* base, RpnBase& B) {
  if (!base) return -4;
  for (int k = 0; k < 4; ++k) for (int a = 0; a < RPN_MAX_A; ++a) for (int c = 0; c < 3; ++c) B.h[k][a][c] = 1.f;
  int at = 0;
  for (int k = 0; k < nlevels; ++k) {
    for (int a = 0; a < dims[7 * k + 6]; ++a, ++at) {
      for (int c = 0; c < 3; ++c) {
        const float v = base[at * 3 + c];
        if (!(v > 0.f) || !(v < 1e6f)) return -4;
        B.h[k][a][c] = v;
      }
    }
  }
  return 0;
}

}  // namespace

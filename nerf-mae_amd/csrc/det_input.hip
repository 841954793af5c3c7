// Input pipeline of the detection stack: what the reference's BaseDataset.augment_rpn_inputs does to a scene and its boxes before the detector sees
// them (nerf_rpn/datasets.py:173-244), including the small-angle rotation + scaling of oriented-box training data, rotate_and_scale_scene (:478-524).
//   grid_prepare_rs: nmh_grid_prepare's one pass (misc.hip) with the trilinear resample of rotate_and_scale_scene folded in.
//   boxes_augment:   the box side of the same augmentations, one launch per batch.
#include "common.hpp"
#include "kernels.hpp"
#include <cmath>

// ---- scene: stored (W,L,H,4) -> /255 | density->alpha -> channels first -> rot -> flips -> resample -> zero padding, one pass -------------------------
// The reference resamples the augmented grid (extents r0,r1,r2 = A0,A1,H) with F.grid_sample(align_corners=True) at
//   X = linspace(-1,1,r0)[i] * r0/2 (likewise Y, Z);  q = scale * Rz(angle) (X,Y,Z);  normalised = q / (r/2);  voxel = (normalised + 1)/2 * (r - 1)
// (datasets.py:481-512).  With ci = i - (r0-1)/2 (so X = ci * r0/(r0-1)) this collapses to an affine map of (ci, cj) for axes 0, 1 and of ck for axis 2:
//   a0 = s cos a * ci - s sin a * (r1/(r1-1)) ((r0-1)/r0) * cj + (r0-1)/2
//   a1 = s sin a * (r0/(r0-1)) ((r1-1)/r1) * ci + s cos a * cj + (r1-1)/2          a2 = s * ck + (r2-1)/2
// The coefficients are formed on the host in double and the three coordinates are evaluated in double here (5 FMAs per voxel, nothing against 8 gathered
// taps), so the coordinate rounding that dominates the reference's own fp32 error (extent * 2^-23 voxels per axis) does not occur; the blend is fp32.
// Taps outside [0, r) contribute 0 (grid_sample's zero padding).  Each tap goes back to the stored voxel through the inverse flips and rotation exactly as
// grid_prepare_kernel does, and is converted (/255, or alpha on channel 3) before blending.  a2 depends on k only and the last axis is never permuted:
// neighbouring k lanes read neighbouring stored voxels (scale ~ 1), four nearly contiguous source rows per output row.
struct RsGeom { double m00, m01, m10, m11, s, c0, c1, c2; };

template <typename S>
__device__ __forceinline__ float4 rs_tap(const S* __restrict__ src, int t0, int t1, int t2, int A0, int A1, int L, int H, bool rot, bool f0, bool f1, bool dens) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if ((unsigned)t0 < (unsigned)A0 && (unsigned)t1 < (unsigned)A1 && (unsigned)t2 < (unsigned)H) {
    const int ii = f0 ? A0 - 1 - t0 : t0, jj = f1 ? A1 - 1 - t1 : t1;
    int w, l;
    if (rot) { w = jj; l = A0 - 1 - ii; } else { w = ii; l = jj; }
    const long si = (((long)w * L + l) * H + t2) * 4;
    if constexpr (sizeof(S) == 1) {
      const uchar4 u = *reinterpret_cast<const uchar4*>(src + si);
      v = make_float4(u.x * (1.0f / 255.0f), u.y * (1.0f / 255.0f), u.z * (1.0f / 255.0f), u.w * (1.0f / 255.0f));
    } else {
      v = *reinterpret_cast<const float4*>(src + si);
      if (dens) v.w = fminf(fmaxf(1.0f - expf(-expf(v.w) / 100.0f), 0.0f), 1.0f);
    }
  }
  return v;
}
__device__ __forceinline__ float4 lerp4(float4 a, float4 b, float f) {
  const float g = 1.0f - f;
  return make_float4(a.x * g + b.x * f, a.y * g + b.y * f, a.z * g + b.z * f, a.w * g + b.w * f);
}

template <typename S>
__global__ __launch_bounds__(256) void grid_prepare_rs_kernel(const S* __restrict__ src, int W, int L, int H, float* __restrict__ dst, int R, int flags, RsGeom g) {
  const bool rot = flags & 1, f0 = flags & 2, f1 = flags & 4, dens = flags & 8;
  const int A0 = rot ? L : W, A1 = rot ? W : L;
  const long R3 = (long)R * R * R;
  for (long o = (long)blockIdx.x * 256 + threadIdx.x; o < R3; o += (long)gridDim.x * 256) {
    const int k = (int)(o % R);
    const long t = o / R;
    const int j = (int)(t % R), i = (int)(t / R);
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < A0 && j < A1 && k < H) {
      const double ci = (double)i - g.c0, cj = (double)j - g.c1, ck = (double)k - g.c2;
      const double a0 = fma(g.m00, ci, fma(g.m01, cj, g.c0)), a1 = fma(g.m10, ci, fma(g.m11, cj, g.c1)), a2 = fma(g.s, ck, g.c2);
      const double b0 = floor(a0), b1 = floor(a1), b2 = floor(a2);
      // all eight taps out of range (or a coordinate that is not a number): zero, and no integer conversion of an unbounded value
      if (b0 >= -1.0 && b0 <= (double)(A0 - 1) && b1 >= -1.0 && b1 <= (double)(A1 - 1) && b2 >= -1.0 && b2 <= (double)(H - 1)) {
        const int x0 = (int)b0, y0 = (int)b1, z0 = (int)b2;
        const float fx = (float)(a0 - b0), fy = (float)(a1 - b1), fz = (float)(a2 - b2);
        const float4 v00 = lerp4(rs_tap(src, x0, y0, z0, A0, A1, L, H, rot, f0, f1, dens), rs_tap(src, x0, y0, z0 + 1, A0, A1, L, H, rot, f0, f1, dens), fz);
        const float4 v01 = lerp4(rs_tap(src, x0, y0 + 1, z0, A0, A1, L, H, rot, f0, f1, dens), rs_tap(src, x0, y0 + 1, z0 + 1, A0, A1, L, H, rot, f0, f1, dens), fz);
        const float4 v10 = lerp4(rs_tap(src, x0 + 1, y0, z0, A0, A1, L, H, rot, f0, f1, dens), rs_tap(src, x0 + 1, y0, z0 + 1, A0, A1, L, H, rot, f0, f1, dens), fz);
        const float4 v11 = lerp4(rs_tap(src, x0 + 1, y0 + 1, z0, A0, A1, L, H, rot, f0, f1, dens), rs_tap(src, x0 + 1, y0 + 1, z0 + 1, A0, A1, L, H, rot, f0, f1, dens), fz);
        r = lerp4(lerp4(v00, v01, fy), lerp4(v10, v11, fy), fx);
      }
    }
    dst[o] = r.x; dst[R3 + o] = r.y; dst[2 * R3 + o] = r.z; dst[3 * R3 + o] = r.w;
  }
}

int k_grid_prepare_rs(int src_u8, const void* src, int W, int L, int H, float* dst, int R, int flags, float angle, float scale, hipStream_t st) {
  const bool rot = flags & 1;
  const int A0 = rot ? L : W, A1 = rot ? W : L;
  if (A0 > R || A1 > R || H > R || W < 2 || L < 2 || H < 2) return -2;     // linspace(-1, 1, r) needs r >= 2
  const double c = std::cos((double)angle), s = std::sin((double)angle), sc = (double)scale;
  const double r0 = A0, r1 = A1, r2 = H;
  RsGeom g;
  g.m00 = sc * c; g.m01 = -sc * s * (r1 / (r1 - 1.0)) * ((r0 - 1.0) / r0);
  g.m10 = sc * s * (r0 / (r0 - 1.0)) * ((r1 - 1.0) / r1); g.m11 = sc * c;
  g.s = sc; g.c0 = (r0 - 1.0) / 2.0; g.c1 = (r1 - 1.0) / 2.0; g.c2 = (r2 - 1.0) / 2.0;
  const long R3 = (long)R * R * R;
  const unsigned nb = (unsigned)((R3 + 255) / 256 < 8192 ? (R3 + 255) / 256 : 8192);
  if (src_u8) hipLaunchKernelGGL(grid_prepare_rs_kernel<unsigned char>, dim3(nb), dim3(256), 0, st, (const unsigned char*)src, W, L, H, dst, R, flags, g);
  else hipLaunchKernelGGL(grid_prepare_rs_kernel<float>, dim3(nb), dim3(256), 0, st, (const float*)src, W, L, H, dst, R, flags, g);
  NMH_CHECK_LAUNCH();
  return 0;
}

// ---- boxes: the same augmentations on [sum G, 6 | 7] fp32 boxes of a batch, one launch, the per-scene table as kernel arguments --------------------------
// fp32 throughout, in the reference's order of operations (datasets.py:206-233, 514-522, z_up=True); e0, e1, e2 are the grid's extents after rot / flips.
//   6 columns (xmin,ymin,zmin,xmax,ymax,zmax): rot swaps x/y, then (xmin, xmax) = e0 - (xmax, xmin); a flip of axis a: (min_a, max_a) = e_a - (max_a, min_a).
//   7 columns (x,y,z,w,l,h,theta): rot swaps x/y and w/l, x = e0 - x, theta unchanged; a flip mirrors the centre and negates theta;
//   rot-scale: theta -= angle, dims /= scale, centre = (centre - e/2) @ (Rz(angle)/scale) + e/2 -- a row vector times the matrix.
// cos/scale, sin/scale and 1/scale are formed on the host in double and rounded once.
#define NMH_BOX_SCENES 64
struct BoxScene { int first, count, flags, has_rs; float e0, e1, e2, angle, scale, mc, ms, mz; };
struct BoxTable { BoxScene s[NMH_BOX_SCENES]; };

template <int cols>
__global__ __launch_bounds__(256) void boxes_augment_kernel(const float* __restrict__ in, float* __restrict__ out, int n_scenes, int rows, BoxTable tb) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= rows) return;
  int si = -1;
  for (int n = 0; n < n_scenes; ++n)
    if (row >= tb.s[n].first && row < tb.s[n].first + tb.s[n].count) si = n;
  float b[7];
#pragma unroll
  for (int c = 0; c < cols; ++c) b[c] = in[(long)row * cols + c];
  if (si >= 0) {
    const BoxScene sc = tb.s[si];
    const bool rot = sc.flags & 1, f0 = sc.flags & 2, f1 = sc.flags & 4;
    if (cols == 6) {
      if (rot) {
        const float x0 = b[1], y0 = b[0], x1 = b[4], y1 = b[3];
        b[0] = sc.e0 - x1; b[1] = y0; b[3] = sc.e0 - x0; b[4] = y1;
      }
      if (f0) { const float lo = b[0], hi = b[3]; b[0] = sc.e0 - hi; b[3] = sc.e0 - lo; }
      if (f1) { const float lo = b[1], hi = b[4]; b[1] = sc.e1 - hi; b[4] = sc.e1 - lo; }
    } else {
      if (rot) {
        const float x = b[1], y = b[0], w = b[4], l = b[3];
        b[0] = sc.e0 - x; b[1] = y; b[3] = w; b[4] = l;
      }
      if (f0) { b[0] = sc.e0 - b[0]; b[6] = -b[6]; }
      if (f1) { b[1] = sc.e1 - b[1]; b[6] = -b[6]; }
      if (sc.has_rs) {
        b[6] = b[6] - sc.angle;
        b[3] = b[3] / sc.scale; b[4] = b[4] / sc.scale; b[5] = b[5] / sc.scale;
        const float h0 = sc.e0 / 2.0f, h1 = sc.e1 / 2.0f, h2 = sc.e2 / 2.0f;
        const float ox = b[0] - h0, oy = b[1] - h1, oz = b[2] - h2;
        b[0] = (ox * sc.mc + oy * sc.ms) + h0;
        b[1] = (oy * sc.mc - ox * sc.ms) + h1;
        b[2] = oz * sc.mz + h2;
      }
    }
  }
#pragma unroll
  for (int c = 0; c < cols; ++c) out[(long)row * cols + c] = b[c];
}

// itab: [n_scenes][7] = first row, count, flags, has_rs, e0, e1, e2;  ftab: [n_scenes][2] = angle, scale (host memory, copied into the launch arguments)
int k_boxes_augment(const float* boxes, float* out, int cols, int total_rows, int n_scenes, const int* itab, const float* ftab, hipStream_t st) {
  if ((cols != 6 && cols != 7) || n_scenes < 0 || n_scenes > NMH_BOX_SCENES || total_rows < 0) return -2;
  if (total_rows == 0) return 0;
  BoxTable tb{};
  for (int n = 0; n < n_scenes; ++n) {
    BoxScene& s = tb.s[n];
    const int* it = itab + 7 * n;
    s.first = it[0]; s.count = it[1]; s.flags = it[2]; s.has_rs = it[3];
    if (s.first < 0 || s.count < 0 || (long)s.first + s.count > total_rows || (s.has_rs && cols != 7)) return -2;
    s.e0 = (float)it[4]; s.e1 = (float)it[5]; s.e2 = (float)it[6];
    s.angle = ftab[2 * n]; s.scale = ftab[2 * n + 1];
    if (s.has_rs) {
      if (!(s.scale != 0.0f)) return -2;
      const double a = (double)s.angle, k = (double)s.scale;
      s.mc = (float)(std::cos(a) / k); s.ms = (float)(std::sin(a) / k); s.mz = (float)(1.0 / k);
    }
  }
  if (cols == 6) hipLaunchKernelGGL(boxes_augment_kernel<6>, dim3((total_rows + 255) / 256), dim3(256), 0, st, boxes, out, n_scenes, total_rows, tb);
  else hipLaunchKernelGGL(boxes_augment_kernel<7>, dim3((total_rows + 255) / 256), dim3(256), 0, st, boxes, out, n_scenes, total_rows, tb);
  NMH_CHECK_LAUNCH();
  return 0;
}

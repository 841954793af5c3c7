// The two native ops of the reference's downstream (nerf_rpn) path, as gfx950 kernels:
//   rotated 3-D RoIAlign, forward and input gradient (nerf_rpn/model/rotated_align/src/cuda_3d/ROIAlignRotated3D_cuda.cu, bound by
//     rotated_align/roi_align_rotate_3d.py, used by detector.py:192-193);
//   polygon vertex sort of the oriented-box IoU losses (nerf_rpn/model/rotated_iou/cuda_op/sort_vert_kernel.cu, called from
//     box_intersection_2d.py:141).
//
// RoIAlign.  rois [N][8] fp32 = {batch index, centre (w,l,h), size (w,l,h), angle in degrees}.  Centre and size are multiplied by
// spatial_scale (no rounding), each size is clamped to >= 1.  Output bin (pw,pl,ph) is the mean over a gw x gl x gh grid of sample points,
// g = sampling_ratio if > 0 else ceil(size / pooled) per axis.  A sample at ROI-local (xx,yy,zz) maps to
//   x = xx cos(t) + yy sin(t) + cw,  y = yy cos(t) - xx sin(t) + cl,  z = zz + ch          (rotation about the h axis only)
// and contributes 0 if any coordinate is < -1 or > extent; otherwise the coordinate is clamped to >= 0, low = (int)coord, and at
// low >= extent - 1 both corners collapse to extent - 1 with fraction 0; then trilinear weights.  The backward scatters
// dout * weight / count to the same eight corners.
// DEVIATION from the reference: voxel (x,y,z) of a (W,L,H) map is element (x*L + y)*H + z here.  The reference's forward uses
// (x*W + y)*L + z and its backward x*L for the low-y and x*W for the high-y corners; all agree only for W = L = H, and on any other map
// the reference reads and writes the wrong voxels (and can leave the allocation).  Identical on cubic maps, correct on the rest.
// An ROI whose batch index is outside [0, B) (or not finite, or whose size is not finite) is skipped: zero output, no gradient.
// sin/cos are taken by sincospif(deg / 180), exact at multiples of 90 degrees.
//
// Two layouts over one sampling core (roi_decode / for_each_sample):
//   channels-last (B,W,L,H,C) fp32|bf16 -> [N,PW,PL,PH,C]: the product form (the FPN neck computes its maps channels-last).  A group of
//     G lanes owns one bin; lanes run along C, so every corner is one contiguous row segment and the sample arithmetic is uniform over the
//     group (the whole wave from C = 512 on in the forward, C = 64 in the backward).  Forward: 8 channels per lane per load (16 / 32 B).
//     Backward: the gradient is fp32 whatever dt is and is written with no-return fp32 atomic adds, one dword per lane, consecutive lanes
//     on consecutive channels: each wave-instruction is min(C, 64) * 4 contiguous bytes (256 B from C = 64 on), the shape
//     global_atomic_add_f32 runs at full rate in.  The caller zeroes the gradient.
//   NCWLH fp32, the reference's own layout: the compatibility form, one lane per output element, scalar corner reads and scalar atomics.
//
// Vertex sort.  vertices [B,N,M,2] fp32 (centred by the caller), mask [B,N,M] bytes, num_valid [B,N] int32 -> idx [B,N,9] int32, one
// polygon per lane.  pad = first j >= 8 with mask[j] == 0 (M - 1 if there is none).  num_valid < 3: nine pads.  Otherwise entries
// 0..nv-1 are the masked vertices in increasing polar angle over [0, 2 pi), chosen by selection: entry j is the smallest vertex strictly
// greater than entry j-1, the first one found among equals (two vertices closer than 1e-8 in both coordinates are equal, so a later
// duplicate is never selected; when nothing is left the entry is 0, as in the reference).  Entry nv repeats entry 0, the rest are pad.
// num_valid == 8 and entries 0-3 reappearing in entries 4-7 (two identical boxes): entry 4 = entry 0, entries 5-8 = pad.
// The order is decided by half-plane, then by the sign of the cross product -- no division, no arc tangent.  The reference's comparison
// has no result when a y is exactly 0 (control falls off the end of its function); here it is defined by the angle: y = 0, x > 0 is
// angle 0 (first of the upper half-plane), y = 0, x < 0 is angle pi (first of the lower half-plane); the origin counts as angle 0.
#include "common.hpp"
#include "kernels.hpp"

namespace {

struct RoiGeom {
  int b;                 // batch index, validated
  float cw, cl, ch;      // centre, scaled
  float sw, sl, sh;      // start of the ROI-local frame (-size / 2)
  float bw, bl, bh;      // bin size
  int gw, gl, gh;        // sample grid per bin
  float cs, sn;
};

__device__ __forceinline__ bool roi_decode(const float* __restrict__ r, float scale, int B, int PW, int PL, int PH, int sr, RoiGeom& q) {
  const float fb = r[0];
  if (!(fb >= 0.f && fb < (float)B)) return false;
  q.b = (int)fb;
  q.cw = r[1] * scale; q.cl = r[2] * scale; q.ch = r[3] * scale;
  const float rw = fmaxf(r[4] * scale, 1.f), rl = fmaxf(r[5] * scale, 1.f), rh = fmaxf(r[6] * scale, 1.f);
  if (!(rw <= 3.0e38f && rl <= 3.0e38f && rh <= 3.0e38f)) return false;
  q.sw = -rw / 2.f; q.sl = -rl / 2.f; q.sh = -rh / 2.f;
  q.bw = rw / (float)PW; q.bl = rl / (float)PL; q.bh = rh / (float)PH;
  q.gw = sr > 0 ? sr : (int)ceilf(rw / (float)PW);
  q.gl = sr > 0 ? sr : (int)ceilf(rl / (float)PL);
  q.gh = sr > 0 ? sr : (int)ceilf(rh / (float)PH);
  sincospif(r[7] / 180.f, &q.sn, &q.cs);
  return true;
}

// one axis of a sample: false -> the sample contributes nothing
__device__ __forceinline__ bool axis_corners(float v, int ext, int& lo, int& hi, float& frac) {
  if (!(v >= -1.f && v <= (float)ext)) return false;
  v = fmaxf(v, 0.f);
  lo = (int)v;
  if (lo >= ext - 1) { lo = hi = ext - 1; frac = 0.f; }
  else { hi = lo + 1; frac = v - (float)lo; }
  return true;
}

// f(vox, w): the eight corner voxels (x*L + y)*H + z and trilinear weights of every contributing sample of bin (pw,pl,ph)
template <typename F>
__device__ __forceinline__ void for_each_sample(const RoiGeom& q, int pw, int pl, int ph, int W, int L, int H, F&& f) {
  for (int ix = 0; ix < q.gw; ++ix) {
    const float xx = q.sw + (float)pw * q.bw + ((float)ix + .5f) * q.bw / (float)q.gw;
    for (int iy = 0; iy < q.gl; ++iy) {
      const float yy = q.sl + (float)pl * q.bl + ((float)iy + .5f) * q.bl / (float)q.gl;
      const float x = xx * q.cs + yy * q.sn + q.cw;
      const float y = yy * q.cs - xx * q.sn + q.cl;
      int x0, x1, y0, y1;
      float lx, ly;
      if (!axis_corners(x, W, x0, x1, lx) || !axis_corners(y, L, y0, y1, ly)) continue;
      const int r00 = (x0 * L + y0) * H, r01 = (x0 * L + y1) * H, r10 = (x1 * L + y0) * H, r11 = (x1 * L + y1) * H;
      const float w00 = (1.f - lx) * (1.f - ly), w01 = (1.f - lx) * ly, w10 = lx * (1.f - ly), w11 = lx * ly;
      for (int iz = 0; iz < q.gh; ++iz) {
        const float z = q.sh + (float)ph * q.bh + ((float)iz + .5f) * q.bh / (float)q.gh + q.ch;
        int z0, z1;
        float lz;
        if (!axis_corners(z, H, z0, z1, lz)) continue;
        const float hz = 1.f - lz;
        const int vox[8] = {r00 + z0, r00 + z1, r01 + z0, r01 + z1, r10 + z0, r10 + z1, r11 + z0, r11 + z1};
        const float w[8] = {w00 * hz, w00 * lz, w01 * hz, w01 * lz, w10 * hz, w10 * lz, w11 * hz, w11 * lz};
        f(vox, w);
      }
    }
  }
}

__device__ __forceinline__ void bin_coords(long bin, int PW, int PL, int PH, int& n, int& pw, int& pl, int& ph) {
  ph = (int)(bin % PH); bin /= PH;
  pl = (int)(bin % PL); bin /= PL;
  pw = (int)(bin % PW);
  n = (int)(bin / PW);
}

struct RoiDims { int N, B, W, L, H, C, PW, PL, PH, sr; float scale; };

// ---- channels-last forward: G lanes per bin (G a power of two <= 64), 8 channels per lane per pass ------------------------------
template <typename T>
__global__ __launch_bounds__(256) void roi_fwd_cl_kernel(const T* __restrict__ x, const float* __restrict__ rois, T* __restrict__ out, RoiDims d, int lgG, long nbins) {
  const int G = 1 << lgG, lig = threadIdx.x & (G - 1);
  const long bin = (long)blockIdx.x * (256 >> lgG) + (threadIdx.x >> lgG);
  if (bin >= nbins) return;
  int n, pw, pl, ph;
  bin_coords(bin, d.PW, d.PL, d.PH, n, pw, pl, ph);
  RoiGeom q;
  const bool ok = roi_decode(rois + (long)n * 8, d.scale, d.B, d.PW, d.PL, d.PH, d.sr, q);
  const float count = ok ? (float)q.gw * (float)q.gl * (float)q.gh : 1.f;
  const T* xb = x + (ok ? (long)q.b * d.W * d.L * d.H * d.C : 0);
  for (int c0 = lig * 8; c0 < d.C; c0 += G * 8) {
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (ok) for_each_sample(q, pw, pl, ph, d.W, d.L, d.H, [&](const int (&vox)[8], const float (&w)[8]) {
      float v[8][8];
#pragma unroll
      for (int k = 0; k < 8; ++k) Vec8<T>::load(xb + (long)vox[k] * d.C + c0, v[k]);
#pragma unroll
      for (int k = 0; k < 8; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += w[k] * v[k][j];
    });
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] /= count;
    Vec8<T>::store(out + bin * d.C + c0, acc);
  }
}

// ---- channels-last backward: G lanes per bin (G = min(64, C rounded up to a power of two)), one dword per lane per atomic --------
template <typename T>
__global__ __launch_bounds__(256) void roi_bwd_cl_kernel(const T* __restrict__ dout, const float* __restrict__ rois, float* __restrict__ dx, RoiDims d, int lgG, long nbins) {
  const int G = 1 << lgG, lig = threadIdx.x & (G - 1);
  const long bin = (long)blockIdx.x * (256 >> lgG) + (threadIdx.x >> lgG);
  if (bin >= nbins) return;
  int n, pw, pl, ph;
  bin_coords(bin, d.PW, d.PL, d.PH, n, pw, pl, ph);
  RoiGeom q;
  if (!roi_decode(rois + (long)n * 8, d.scale, d.B, d.PW, d.PL, d.PH, d.sr, q)) return;
  const float count = (float)q.gw * (float)q.gl * (float)q.gh;
  float* dxb = dx + (long)q.b * d.W * d.L * d.H * d.C;
  for (int c0 = lig; c0 < d.C; c0 += 4 * G) {     // channels c0 + k*G, k < 4, of this lane
    float g[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) g[k] = c0 + k * G < d.C ? to_f<T>(dout[bin * d.C + c0 + k * G]) / count : 0.f;
    for_each_sample(q, pw, pl, ph, d.W, d.L, d.H, [&](const int (&vox)[8], const float (&w)[8]) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (w[j] == 0.f) continue;
        float* p = dxb + (long)vox[j] * d.C + c0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (c0 + k * G < d.C) atomicAdd(p + k * G, w[j] * g[k]);
      }
    });
  }
}

// ---- NCWLH fp32 (the reference's layout): one lane per output element (n, c, pw, pl, ph) -----------------------------------------
__global__ __launch_bounds__(256) void roi_fwd_nc_kernel(const float* __restrict__ x, const float* __restrict__ rois, float* __restrict__ out, RoiDims d, long total) {
  const long nb = (long)d.PW * d.PL * d.PH;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long nc = i / nb;
    const int c = (int)(nc % d.C);
    int n, pw, pl, ph;
    bin_coords(nc / d.C * nb + i % nb, d.PW, d.PL, d.PH, n, pw, pl, ph);
    RoiGeom q;
    float acc = 0.f;
    if (roi_decode(rois + (long)n * 8, d.scale, d.B, d.PW, d.PL, d.PH, d.sr, q)) {
      const float* xb = x + ((long)q.b * d.C + c) * d.W * d.L * d.H;
      for_each_sample(q, pw, pl, ph, d.W, d.L, d.H, [&](const int (&vox)[8], const float (&w)[8]) {
#pragma unroll
        for (int k = 0; k < 8; ++k) acc += w[k] * xb[vox[k]];
      });
      acc /= (float)q.gw * (float)q.gl * (float)q.gh;
    }
    out[i] = acc;
  }
}
__global__ __launch_bounds__(256) void roi_bwd_nc_kernel(const float* __restrict__ dout, const float* __restrict__ rois, float* __restrict__ dx, RoiDims d, long total) {
  const long nb = (long)d.PW * d.PL * d.PH;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long nc = i / nb;
    const int c = (int)(nc % d.C);
    int n, pw, pl, ph;
    bin_coords(nc / d.C * nb + i % nb, d.PW, d.PL, d.PH, n, pw, pl, ph);
    RoiGeom q;
    if (!roi_decode(rois + (long)n * 8, d.scale, d.B, d.PW, d.PL, d.PH, d.sr, q)) continue;
    const float g = dout[i] / ((float)q.gw * (float)q.gl * (float)q.gh);
    float* dxb = dx + ((long)q.b * d.C + c) * d.W * d.L * d.H;
    for_each_sample(q, pw, pl, ph, d.W, d.L, d.H, [&](const int (&vox)[8], const float (&w)[8]) {
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (w[k] != 0.f) atomicAdd(dxb + vox[k], w[k] * g);
    });
  }
}

inline int lg2_ceil(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }
inline bool roi_dims_ok(const RoiDims& d) {
  // voxel indices are ints inside the kernels: one batch item of one channel must fit
  return d.B > 0 && d.W > 0 && d.L > 0 && d.H > 0 && d.C > 0 && d.PW > 0 && d.PL > 0 && d.PH > 0 && (long)d.W * d.L * d.H < (1L << 31);
}

// ---- vertex sort ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int vs_half(float x, float y) { return (y > 0.f || (y == 0.f && x >= 0.f)) ? 0 : 1; }
// a strictly before b in polar angle over [0, 2 pi)
__device__ __forceinline__ bool vs_less(float ax, float ay, float bx, float by) {
  if (fabsf(ax - bx) < 1e-8f && fabsf(ay - by) < 1e-8f) return false;
  const int ha = vs_half(ax, ay), hb = vs_half(bx, by);
  if (ha != hb) return ha < hb;
  return ax * by - ay * bx > 0.f;
}

__global__ __launch_bounds__(256) void sort_vertices_kernel(const float2* __restrict__ vertices, const unsigned char* __restrict__ mask, const int* __restrict__ num_valid,
                                                            int* __restrict__ idx, long npoly, int M) {
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npoly) return;
  const float2* v = vertices + p * M;
  const unsigned char* mk = mask + p * M;
  unsigned bits = 0;
  for (int k = 0; k < M; ++k) bits |= (mk[k] ? 1u : 0u) << k;
  int pad = M - 1;
  for (int j = M - 1; j >= 8; --j) if (!((bits >> j) & 1u)) pad = j;
  int nv = num_valid[p];
  nv = nv > 8 ? 8 : nv;
  int o[9];
#pragma unroll
  for (int j = 0; j < 9; ++j) o[j] = pad;
  if (nv >= 3) {
    float px = 0.f, py = 0.f;   // the previous entry
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (j < nv) {
        int take = 0;
        bool have = false;
        float mx = 0.f, my = 0.f;
        for (int k = 0; k < M; ++k) {
          if (!((bits >> k) & 1u)) continue;
          const float2 c = v[k];
          if (j > 0 && !vs_less(px, py, c.x, c.y)) continue;
          if (!have || vs_less(c.x, c.y, mx, my)) { have = true; mx = c.x; my = c.y; take = k; }
        }
        o[j] = take;
        if (have) { px = mx; py = my; }
        else { const float2 c = v[0]; px = c.x; py = c.y; }
      }
    }
#pragma unroll
    for (int j = 3; j < 9; ++j) if (j == nv) o[j] = o[0];
    if (nv == 8) {
      int counter = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int k = 4; k < 8; ++k) counter += o[k] == o[j];
      if (counter == 4) {
        o[4] = o[0];
        o[5] = o[6] = o[7] = o[8] = pad;
      }
    }
  }
  int* op = idx + p * 9;
#pragma unroll
  for (int j = 0; j < 9; ++j) op[j] = o[j];
}

}  // namespace

int k_roi_align_rotated_3d_fwd(int layout, int dt, const void* x, const float* rois, void* out, int N, int B, int W, int L, int H, int C, int PW, int PL, int PH,
                               float spatial_scale, int sampling_ratio, hipStream_t st) {
  const RoiDims d{N, B, W, L, H, C, PW, PL, PH, sampling_ratio, spatial_scale};
  if (!roi_dims_ok(d) || (layout != 0 && layout != 1) || (dt != NMH_DT_F32 && dt != NMH_DT_BF16)) return -4;
  const long nbins = (long)N * PW * PL * PH;
  if (layout == 1) {
    if (dt != NMH_DT_F32) return -4;
    const long total = nbins * C, blocks = (total + 255) / 256;
    hipLaunchKernelGGL(roi_fwd_nc_kernel, dim3((unsigned)(blocks > (1L << 20) ? (1L << 20) : blocks)), dim3(256), 0, st, (const float*)x, rois, (float*)out, d, total);
  } else {
    if (C % 8) return -2;
    const int lgG = lg2_ceil(C / 8 > 64 ? 64 : C / 8);
    const long per = 256 >> lgG, blocks = (nbins + per - 1) / per;
    if (blocks >= (1L << 31)) return -4;
    if (dt == NMH_DT_BF16) hipLaunchKernelGGL(roi_fwd_cl_kernel<bf16_t>, dim3((unsigned)blocks), dim3(256), 0, st, (const bf16_t*)x, rois, (bf16_t*)out, d, lgG, nbins);
    else hipLaunchKernelGGL(roi_fwd_cl_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, st, (const float*)x, rois, (float*)out, d, lgG, nbins);
  }
  NMH_CHECK_LAUNCH();
  return 0;
}

int k_roi_align_rotated_3d_bwd(int layout, int dt, const void* dout, const float* rois, float* dx, int N, int B, int W, int L, int H, int C, int PW, int PL, int PH,
                               float spatial_scale, int sampling_ratio, hipStream_t st) {
  const RoiDims d{N, B, W, L, H, C, PW, PL, PH, sampling_ratio, spatial_scale};
  if (!roi_dims_ok(d) || (layout != 0 && layout != 1) || (dt != NMH_DT_F32 && dt != NMH_DT_BF16)) return -4;
  const long nbins = (long)N * PW * PL * PH;
  if (layout == 1) {
    if (dt != NMH_DT_F32) return -4;
    const long total = nbins * C, blocks = (total + 255) / 256;
    hipLaunchKernelGGL(roi_bwd_nc_kernel, dim3((unsigned)(blocks > (1L << 20) ? (1L << 20) : blocks)), dim3(256), 0, st, (const float*)dout, rois, dx, d, total);
  } else {
    if (C % 8) return -2;
    const int lgG = lg2_ceil(C > 64 ? 64 : C);
    const long per = 256 >> lgG, blocks = (nbins + per - 1) / per;
    if (blocks >= (1L << 31)) return -4;
    if (dt == NMH_DT_BF16) hipLaunchKernelGGL(roi_bwd_cl_kernel<bf16_t>, dim3((unsigned)blocks), dim3(256), 0, st, (const bf16_t*)dout, rois, dx, d, lgG, nbins);
    else hipLaunchKernelGGL(roi_bwd_cl_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, st, (const float*)dout, rois, dx, d, lgG, nbins);
  }
  NMH_CHECK_LAUNCH();
  return 0;
}

int k_sort_vertices(const float* vertices, const unsigned char* mask, const int* num_valid, int* idx, int B, int N, int M, hipStream_t st) {
  if (M < 9 || M > 32) return -4;
  const long npoly = (long)B * N;
  hipLaunchKernelGGL(sort_vertices_kernel, dim3((unsigned)((npoly + 255) / 256)), dim3(256), 0, st, (const float2*)vertices, mask, num_valid, idx, npoly, M);
  NMH_CHECK_LAUNCH();
  return 0;
}

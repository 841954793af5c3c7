// Second (RoI) stage of the reference's two-stage detector (nerf_rpn/model/detector.py), as gfx950 kernels:
//   roi_match / roi_sample / roi_gather   ProposalTargetLayer._sample_rois_pytorch (detector.py:60-167) over batched_box_iou (model/utils.py:371-458)
//   roi_level_map                         LevelMapper.__call__ (level_mapper.py:47-59), the remap=True branch of ROIPool.forward (detector.py:222-236)
//   roi_pool fwd / bwd                    ROIPool.normal_forward (detector.py:407-438) and ROIPool.rotated_forward (detector.py:264-404), 'pooling'
//   roi_interp fwd / bwd                  ROIPool.rotated_forward (detector.py:264-404), 'interpolation'
//   roi_loss fwd / bwd                    Classification_Model.compute_loss (detector.py:536-559) over RotatedCoder / AABBCoder.encode_single
//   roi_decode                            RotatedCoder.decode_single (coder/rotated_coder.py:57-121), AABBCoder.decode_single (coder/AABB_coder.py:86-137)
// fp32 throughout; every kernel writes only its own outputs for any input and clamps every index it forms;
// the host never waits.  B = 6 (x0,y0,z0,x1,y1,z1) or 7 (x,y,z,w,h,d,theta).
//
// Targets.  Proposals are dense: boxes [N][cap][B], levels [N][cap], counts [N]; scene b's rows 0 .. min(counts[b], cap)-1 exist.  Ground truth is one
// [G][B] array with labels [G] (fp32), scene b owning rows off[b] .. off[b+1]-1, staged in LDS 64 at a time.
//   match:  miou, arg = max over the scene's boxes of IoU, ties to the lowest index; rpn_iou (rpn_shared.hpp) or tile_iou (obb_geom.hpp).  A scene
//           without boxes has miou 0, arg 0.  Rows that do not exist: miou -1, arg -1.
//   sample: one workgroup of 1024 lanes per scene.  Candidates among the existing rows: foreground miou >= fg, else background miou < bg.  Their index
//           lists are written in index order to a workspace.  Both present: nf = min(want_fg, #fg) foreground rows without replacement (the nf
//           smallest keys hash(seed, counter, scene, index), radix select of select_scan.hpp, ties at the cut to the lower index) fill slots 0 .. nf-1 in
//           index order; slot j >= nf takes background candidate floor(u_j #bg), u_j = hash2(seed, counter, scene, j) / 2^32: with replacement.  Only one
//           class present: every slot draws from it with replacement.  Neither: every slot is -1.  counts2 = (foreground slots, background slots).
//           A second launch of one lane adds 1 to the counter.
//   gather: keep [N][R] -> labels (sampling: the matched box's label in the foreground slots, 0 behind them; evaluation, R = cap and keep[r] = r:
//           1 if miou >= fg else 0), rois [N][R][1+B] (level, box), gt_rois [N][R][B]; keep -1: label -1 and zeros.
// Pooling.  Maps: per level (N, C, W, H, D), scale[k] mesh units per voxel.  rois [M][1+B], M = N R, scene m / R, level (int)rois[m][0] or the override
// (remap); a level outside 0 .. L-1 gives zeros.  out, arg: [M][C][ow][oh][od].  A lane owns one output cell and 8 channels, cells fastest over the lanes.
//   axis-aligned: half = (hi - lo) / 2 * (1 + e), mid = (hi + lo) / 2, box' = mid -+ 0.5 half (the reference's arithmetic: its "enlarged" box has
//           (1 + e) / 2 of the side), p0 = floor(lo' / scale), p1 = floor(hi' / scale), crop [max(p0, 0), min(p1 + 1, size)) (the reference wraps a
//           negative p0; DEVIATION: clamped, an empty crop gives zeros), s = crop size, k = ceil(s / out), cell o = points [o k, (o + 1) k) of the crop;
//           out = max over the cell's points, and over a 0 if the cell reaches past s (the zero padding).  arg = the voxel's index in its map.
//   oriented: whd' = whd (1 + e), g = clamp(ceil(whd' / scale), 1, ROI_MAX_GRID) points per axis; point i sits at R_z(theta) (i - (g - 1) / 2) + centre /
//           scale; value = sum over the 8 floor/ceil corner combinations of f(corner clamped) (1 - |dx| |dy| |dz|), / 8 (NOT trilinear: the reference's
//           own rule), 0 if the point is outside [0, size - 1] on any axis; cells and padding as above.  arg = (ix g_y + iy) g_z + iz.
//   A value wins over a zero of the padding or of a masked point when equal; among values the first in (x, y, z) order wins; arg = -1 where a zero won.
//   backward: one lane per output element; arg >= 0: the gradient goes to the voxel (axis-aligned) or through the point's eight corner weights (oriented),
//           with fp32 atomic adds into a gradient the caller zeroed.  RoIs get no gradient.
// Interpolation (oriented only; ROIPool.rotated_forward with 'interpolation', detector.py:264-404).  The oriented sampling grid above (sizes, points, the 8-corner
//   value, 0 at a point outside the map), resampled to (ow, oh, od) as F.interpolate(mode="trilinear", align_corners=True) does.  Per axis, g points and O outputs:
//   s = (g - 1) / (O - 1) if O > 1 else 0, src = s o, i0 = min((int)src, g - 1), i1 = i0 + (i0 < g - 1), l1 = clamp(src - i0, 0, 1), l0 = 1 - l1; out = sum
//   over the 8 grid points (i0 | i1)^3 of their values times the products of l0 / l1: at most 64 map reads per channel.  O == 1 takes grid point 0 (the grid's
//   corner, not its centre) and g == 1 the single point: the reference's behaviour.  No arg-max and no padding; points of weight 0 are not read.  Lanes as in
//   the pooling forward.
//   backward: one lane per output element; the geometry is formed again from the RoI (nothing but the RoIs and the level override is saved) and the gradient
//           goes through the resampling weights and each point's eight corner weights with fp32 atomic adds into a gradient the caller zeroed.
// Loss.  One lane per row m.  valid: 0 <= label < n_classes; positive: valid and label > 0.  objectness = sum over valid of (logsumexp(scores) -
//   scores[label]) / #valid; box = sum over positive and columns of smooth_l1(delta - encode(gt_roi, roi); 1/9) / #positive; each 0 when its count is 0.
//   Forward: per-workgroup partial sums in a fixed order, then a fixed-order pass of one workgroup; it also writes the targets [M][B] (0 in rows that are
//   not valid).  Backward: one pass that writes every element of both gradients.
#include "common.hpp"
#include "kernels.hpp"
#include "select_scan.hpp"
#include "reduce_fixed.hpp"
#include "levels4.hpp"
#include "rpn_geom.hpp"
#include "rpn_shared.hpp"
#include "obb_geom.hpp"
#include "roi_decode.hpp"

namespace {

constexpr int ROI_CHUNK = 64;
constexpr int ROI_CPL = 8;                    // channels per lane of the pooling forward
constexpr int ROI_MAX_GRID = NMH_ROI_MAX_GRID;
struct RoiOffs { int off[NMH_FCOS_MAX_SCENES + 1]; };

__device__ __forceinline__ Box6 roi_box6(const float* __restrict__ v) {
  Box6 b;
  b.x0 = v[0]; b.y0 = v[1]; b.z0 = v[2]; b.x1 = v[3]; b.y1 = v[4]; b.z1 = v[5];
  b.vol = (b.x1 - b.x0) * (b.y1 - b.y0) * (b.z1 - b.z0);
  return b;
}

// ---- matching ----------------------------------------------------------------------------------------------------------------------------
template <bool ORIENTED>
__global__ __launch_bounds__(256) void roi_match_kernel(RoiOffs S, int cap, const float* __restrict__ boxes, const int* __restrict__ counts, const float* __restrict__ gt,
                                                        float* __restrict__ miou, int* __restrict__ arg) {
  constexpr int B = ORIENTED ? 7 : 6;
  __shared__ BoxTile sb[ROI_CHUNK];
  const int t = threadIdx.x, scene = blockIdx.y, q = blockIdx.x * 256 + t;
  const int n = min(max(counts[scene], 0), cap);
  BoxTile a;
  Box6 own = {};                                      // the lane's own box, formed once: the axis-aligned form compares Box6, the oriented one BoxTile
  if constexpr (ORIENTED) stage_box<false>(boxes + (long)scene * cap * B, q, n, a);
  else if (q < n) own = roi_box6(boxes + ((long)scene * cap + q) * B);
  const int g0 = S.off[scene], g1 = S.off[scene + 1];
  float best = -1.f;
  int bi = 0;
  for (int c = g0; c < g1; c += ROI_CHUNK) {          // uniform over the workgroup
    __syncthreads();
    if (t < ROI_CHUNK) stage_box<!ORIENTED>(gt, c + t, g1, sb[t]);
    __syncthreads();
    const int m = min(ROI_CHUNK, g1 - c);
    if (q < n) {
      for (int k = 0; k < m; ++k) {
        const float iou = ORIENTED ? tile_iou<false>(a, sb[k]) : rpn_iou(roi_box6(sb[k].v), own);
        if (iou > best) { best = iou; bi = c + k - g0; }
      }
    }
  }
  if (q >= cap) return;
  const long p = (long)scene * cap + q;
  miou[p] = q < n ? fmaxf(best, 0.f) : -1.f;
  arg[p] = q < n ? bi : -1;
}

// ---- sampling ----------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int roi_class(const float* __restrict__ m, int q, int n, float fg, float bg) {
  if (q >= n) return -1;
  const float v = m[q];
  return v >= fg ? 0 : (v < bg ? 1 : -1);
}
// draw j of a stream, uniform in 0 .. cnt-1: floor(h cnt / 2^32)
__device__ __forceinline__ int roi_draw(unsigned long long stream2, int j, int cnt) {
  const unsigned h = (unsigned)(rpn_mix64(stream2 + (unsigned long long)j * 0xD1342543DE82EF95ull) >> 32);
  return (int)(((unsigned long long)h * (unsigned long long)cnt) >> 32);
}

__global__ __launch_bounds__(SEL_T) void roi_sample_kernel(const float* __restrict__ miou, const int* __restrict__ counts, int cap, int R, int want_fg, float fg, float bg,
                                                           const long* __restrict__ rng, int* lists, int* __restrict__ keep, int* __restrict__ counts2) {
  __shared__ int hist[2048];
  __shared__ int wsum[SEL_T / 64];
  __shared__ int sh[2];
  const int t = threadIdx.x, scene = blockIdx.x;
  const int n = min(max(counts[scene], 0), cap);
  const float* __restrict__ m = miou + (long)scene * cap;
  int* list0 = lists + (long)scene * 2 * cap;
  int* list1 = list0 + cap;
  int* __restrict__ kp = keep + (long)scene * R;
  const unsigned long long stream = rpn_stream(rng[0], rng[1], scene), stream2 = rpn_mix64(stream ^ 0x5851F42D4C957F2Dull);

  // the candidates of both classes, in index order
  int have0 = 0, have1 = 0;
  for (int base = 0; base < n; base += SEL_T) {       // uniform
    const int q = base + t, c = roi_class(m, q, n, fg, bg);
    int tot;
    const int r0 = have0 + block_scan_excl(c == 0 ? 1 : 0, tot, wsum);
    have0 += tot;
    const int r1 = have1 + block_scan_excl(c == 1 ? 1 : 0, tot, wsum);
    have1 += tot;
    if (c == 0) list0[r0] = q;
    if (c == 1) list1[r1] = q;
  }
  __syncthreads();                                    // the lists are read by other lanes of this workgroup

  int nf = 0, nb = 0;
  if (have0 > 0 && have1 > 0) { nf = min(min(max(want_fg, 0), have0), R); nb = R - nf; }
  else if (have0 > 0) nf = R;
  else if (have1 > 0) nb = R;
  if (t == 0) { counts2[scene * 2] = nf; counts2[scene * 2 + 1] = nb; }

  if (have0 > 0 && have1 > 0) {
    if (nf >= have0) {
      for (int j = t; j < nf; j += SEL_T) kp[j] = list0[j];
    } else if (nf > 0) {                              // uniform
      const RadixCut cut = radix_select(hist, wsum, sh, nf, n, [&](int q, unsigned& key) {
        if (roi_class(m, q, n, fg, bg) != 0) return false;
        key = rpn_key(stream, q);
        return true;
      });
      int run_eq = 0, run_sel = 0;
      for (int base = 0; base < n; base += SEL_T) {   // uniform
        const int q = base + t;
        const bool cand = roi_class(m, q, n, fg, bg) == 0;
        const unsigned key = cand ? rpn_key(stream, q) : 0u;
        int pos;
        const bool sel = compact_step(cand && key > cut.K, cand && key == cut.K, true, cut.need_eq, run_eq, run_sel, wsum, pos);
        if (sel && pos < nf) kp[pos] = q;
      }
    }
    for (int j = nf + t; j < R; j += SEL_T) kp[j] = list1[roi_draw(stream2, j, have1)];
  } else if (have0 > 0) {
    for (int j = t; j < R; j += SEL_T) kp[j] = list0[roi_draw(stream2, j, have0)];
  } else if (have1 > 0) {
    for (int j = t; j < R; j += SEL_T) kp[j] = list1[roi_draw(stream2, j, have1)];
  } else {
    for (int j = t; j < R; j += SEL_T) kp[j] = -1;
  }
}

template <int B>
__global__ __launch_bounds__(256) void roi_gather_kernel(RoiOffs S, int cap, int R, int is_sample, const float* __restrict__ boxes, const int* __restrict__ levels,
                                                         const int* __restrict__ counts, const float* __restrict__ gt, const float* __restrict__ gt_labels,
                                                         const float* __restrict__ miou, const int* __restrict__ arg, float fg, int* __restrict__ keep, const int* __restrict__ counts2,
                                                         float* __restrict__ labels, float* __restrict__ rois, float* __restrict__ gt_rois) {
  const int scene = blockIdx.y, r = blockIdx.x * 256 + threadIdx.x;
  if (r >= R) return;
  const int n = min(max(counts[scene], 0), cap);
  const long p = (long)scene * R + r;
  int k = is_sample ? keep[p] : r;
  if (k < 0 || k >= n) k = -1;
  keep[p] = k;
  float lab = -1.f, ro[1 + B], gr[B];
#pragma unroll
  for (int c = 0; c < 1 + B; ++c) ro[c] = 0.f;
#pragma unroll
  for (int c = 0; c < B; ++c) gr[c] = 0.f;
  if (k >= 0) {
    const long src = (long)scene * cap + k;
    ro[0] = (float)levels[src];
#pragma unroll
    for (int c = 0; c < B; ++c) ro[1 + c] = boxes[src * B + c];
    const int g0 = S.off[scene], G = S.off[scene + 1] - g0, a = arg[src];
    float glab = 0.f;
    if (a >= 0 && a < G) {
      glab = gt_labels[g0 + a];
#pragma unroll
      for (int c = 0; c < B; ++c) gr[c] = gt[(long)(g0 + a) * B + c];
    }
    lab = is_sample ? (r < counts2[scene * 2] ? glab : 0.f) : (miou[src] >= fg ? 1.f : 0.f);
  }
  labels[p] = lab;
#pragma unroll
  for (int c = 0; c < 1 + B; ++c) rois[p * (1 + B) + c] = ro[c];
#pragma unroll
  for (int c = 0; c < B; ++c) gt_rois[p * B + c] = gr[c];
}

// ---- level mapper --------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void roi_level_map_kernel(long M, const float* __restrict__ boxes, int stride, int off, int k_min, int k_max, float s0, float lvl0, float eps,
                                                            int* __restrict__ out) {
  const long m = (long)blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  const float* __restrict__ b = boxes + m * stride + off;
  const float s = powf(b[3] * b[4] * b[5], 1.f / 3.f);
  float l = floorf(lvl0 + log2f(s / s0) + eps);
  l = fminf(fmaxf(l, (float)k_min), (float)k_max);     // NaN -> k_min
  out[m] = (int)l - k_min;
}

// ---- pooling -------------------------------------------------------------------------------------------------------------------------------
struct RoiPoolGeom {          // kernel argument, by value
  int L, N, C, R;
  long M;
  int W[4], H[4], D[4];
  float scale[4];
  int ow, oh, od, ncell, bpr; // cells per RoI, workgroups per RoI (forward)
  float enlarge;              // 1 + enlarge_scale
};

struct RoiAxis { int lo, s, k; };          // first point (axis-aligned: voxel), points, pooling kernel
// the RoI's level, or -1
__device__ __forceinline__ int roi_level(const RoiPoolGeom& G, const float* __restrict__ roi, const int* __restrict__ lvl_override, long m) {
  const float lf = roi[0];
  const int lvl = lvl_override ? lvl_override[m] : (lf >= 0.f && lf < 4.f ? (int)lf : -1);
  return lvl >= 0 && lvl < G.L ? lvl : -1;
}
__device__ __forceinline__ int roi_floor_int(float v) { return (int)floorf(fminf(fmaxf(v, -1.0e9f), 1.0e9f)); }

__device__ __forceinline__ void roi_axes_aabb(const RoiPoolGeom& G, const float* __restrict__ b, int lvl, RoiAxis (&ax)[3]) {
  const float sc = pick4(G.scale, lvl);
  const int dim[3] = {pick4(G.W, lvl), pick4(G.H, lvl), pick4(G.D, lvl)}, out[3] = {G.ow, G.oh, G.od};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float half = (b[3 + a] - b[a]) / 2.f * G.enlarge, mid = (b[3 + a] + b[a]) / 2.f;
    const int p0 = roi_floor_int((-0.5f * half + mid) / sc), p1 = roi_floor_int((0.5f * half + mid) / sc);
    const int lo = max(p0, 0), hi = min(p1 + 1, dim[a]);
    ax[a].lo = lo; ax[a].s = max(hi - lo, 0); ax[a].k = (ax[a].s + out[a] - 1) / out[a];
  }
}
struct RoiPose { float cx, cy, cz, cs, sn, hx, hy, hz; };
__device__ __forceinline__ void roi_axes_obb(const RoiPoolGeom& G, const float* __restrict__ b, int lvl, RoiAxis (&ax)[3], RoiPose& P) {
  const float sc = pick4(G.scale, lvl);
  const int out[3] = {G.ow, G.oh, G.od};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float e = ceilf(b[3 + a] * G.enlarge / sc);
    const int g = e >= 1.f ? (e < (float)ROI_MAX_GRID ? (int)e : ROI_MAX_GRID) : 1;      // NaN -> 1
    ax[a].lo = 0; ax[a].s = g; ax[a].k = (g + out[a] - 1) / out[a];
  }
  P.cx = b[0] / sc; P.cy = b[1] / sc; P.cz = b[2] / sc;
  P.cs = cosf(b[6]); P.sn = sinf(b[6]);
  P.hx = (float)(ax[0].s - 1) / 2.f; P.hy = (float)(ax[1].s - 1) / 2.f; P.hz = (float)(ax[2].s - 1) / 2.f;
}
// point (ix, iy, iz) of an oriented RoI -> the eight clamped corner voxels and their weights (already / 8); false: outside the map
__device__ __forceinline__ bool roi_point(const RoiPose& P, int ix, int iy, int iz, int W, int H, int D, int (&vox)[8], float (&w)[8]) {
  const float px = (float)ix - P.hx, py = (float)iy - P.hy, pz = (float)iz - P.hz;
  const float X = P.cs * px - P.sn * py + P.cx, Y = P.sn * px + P.cs * py + P.cy, Z = pz + P.cz;
  if (!(X >= 0.f && X <= (float)(W - 1) && Y >= 0.f && Y <= (float)(H - 1) && Z >= 0.f && Z <= (float)(D - 1))) return false;
  const float fx[2] = {floorf(X), ceilf(X)}, fy[2] = {floorf(Y), ceilf(Y)}, fz[2] = {floorf(Z), ceilf(Z)};
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int vx = min(max((int)fx[a], 0), W - 1), vy = min(max((int)fy[b], 0), H - 1), vz = min(max((int)fz[c], 0), D - 1);
        vox[a * 4 + b * 2 + c] = (vx * H + vy) * D + vz;
        w[a * 4 + b * 2 + c] = (1.f - fabsf(X - fx[a]) * fabsf(Y - fy[b]) * fabsf(Z - fz[c])) * 0.125f;
      }
  return true;
}

template <bool ORIENTED>
__global__ __launch_bounds__(256) void roi_pool_fwd_kernel(RoiPoolGeom G, Ptr4<const float> maps, const float* __restrict__ rois, const int* __restrict__ lvl_override,
                                                           float* __restrict__ out, int* __restrict__ argout) {
  constexpr int B = ORIENTED ? 7 : 6;
  const long m = blockIdx.x / G.bpr;
  const int wi = (blockIdx.x - (int)(m * G.bpr)) * 256 + (int)threadIdx.x;
  const int nchunk = (G.C + ROI_CPL - 1) / ROI_CPL;
  if (m >= G.M || wi >= G.ncell * nchunk) return;
  const int cell = wi % G.ncell, c0 = (wi / G.ncell) * ROI_CPL;
  const int scene = (int)(m / G.R);
  const float* __restrict__ roi = rois + m * (1 + B);
  const int lvl = roi_level(G, roi, lvl_override, m);
  float best[ROI_CPL];
  int barg[ROI_CPL];
#pragma unroll
  for (int c = 0; c < ROI_CPL; ++c) { best[c] = -INFINITY; barg[c] = -1; }
  bool zero = true;                          // a zero takes part in the cell's maximum
  if (lvl >= 0) {
    const int W = pick4(G.W, lvl), H = pick4(G.H, lvl), D = pick4(G.D, lvl);
    const long vol = (long)W * H * D;
    const float* __restrict__ f = pick4(maps.p, lvl) + ((long)scene * G.C + c0) * vol;
    RoiAxis ax[3];
    RoiPose P;
    if (ORIENTED) roi_axes_obb(G, roi + 1, lvl, ax, P);
    else roi_axes_aabb(G, roi + 1, lvl, ax);
    const int oz = cell % G.od, oy = (cell / G.od) % G.oh, ox = cell / (G.od * G.oh);
    const int x0 = ox * ax[0].k, x1 = min(x0 + ax[0].k, ax[0].s), y0 = oy * ax[1].k, y1 = min(y0 + ax[1].k, ax[1].s), z0 = oz * ax[2].k, z1 = min(z0 + ax[2].k, ax[2].s);
    const bool empty = ax[0].s == 0 || ax[1].s == 0 || ax[2].s == 0;
    zero = empty || x0 + ax[0].k > ax[0].s || y0 + ax[1].k > ax[1].s || z0 + ax[2].k > ax[2].s;
    if (!empty) {
      for (int x = x0; x < x1; ++x)
        for (int y = y0; y < y1; ++y)
          for (int z = z0; z < z1; ++z) {
            if (ORIENTED) {
              int vox[8];
              float w[8];
              if (!roi_point(P, x, y, z, W, H, D, vox, w)) { zero = true; continue; }
              const int id = (x * ax[1].s + y) * ax[2].s + z;
#pragma unroll
              for (int c = 0; c < ROI_CPL; ++c) {
                if (c0 + c < G.C) {
                  float v = 0.f;
#pragma unroll
                  for (int j = 0; j < 8; ++j) v += f[c * vol + vox[j]] * w[j];
                  if (v > best[c]) { best[c] = v; barg[c] = id; }
                }
              }
            } else {
              const int id = ((ax[0].lo + x) * H + ax[1].lo + y) * D + ax[2].lo + z;       // within the map: lo + s <= size on every axis
#pragma unroll
              for (int c = 0; c < ROI_CPL; ++c) {
                if (c0 + c < G.C) {
                  const float v = f[c * vol + id];
                  if (v > best[c]) { best[c] = v; barg[c] = id; }
                }
              }
            }
          }
    }
  }
#pragma unroll
  for (int c = 0; c < ROI_CPL; ++c) {
    if (c0 + c < G.C) {
      const bool z = barg[c] < 0 || (zero && best[c] < 0.f);
      const long o = (m * G.C + c0 + c) * G.ncell + cell;
      out[o] = z ? 0.f : best[c];
      argout[o] = z ? -1 : barg[c];
    }
  }
}

template <bool ORIENTED>
__global__ __launch_bounds__(256) void roi_pool_bwd_kernel(RoiPoolGeom G, long total, const float* __restrict__ dout, const int* __restrict__ argout, const float* __restrict__ rois,
                                                           const int* __restrict__ lvl_override, Ptr4<float> dmaps) {
  constexpr int B = ORIENTED ? 7 : 6;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int id = argout[e];
  if (id < 0) return;
  const long mc = e / G.ncell, m = mc / G.C;
  const int c = (int)(mc - m * G.C), scene = (int)(m / G.R);
  const float* __restrict__ roi = rois + m * (1 + B);
  const int lvl = roi_level(G, roi, lvl_override, m);
  if (lvl < 0) return;
  float* __restrict__ d = pick4(dmaps.p, lvl);
  if (!d) return;
  const int W = pick4(G.W, lvl), H = pick4(G.H, lvl), D = pick4(G.D, lvl);
  const long vol = (long)W * H * D;
  d += ((long)scene * G.C + c) * vol;
  const float g = dout[e];
  if (!ORIENTED) {
    if (id < vol) atomicAdd(d + id, g);
    return;
  }
  RoiAxis ax[3];
  RoiPose P;
  roi_axes_obb(G, roi + 1, lvl, ax, P);
  const int iz = id % ax[2].s, iy = (id / ax[2].s) % ax[1].s, ix = id / (ax[2].s * ax[1].s);
  int vox[8];
  float w[8];
  if (ix >= ax[0].s || !roi_point(P, ix, iy, iz, W, H, D, vox, w)) return;
#pragma unroll
  for (int j = 0; j < 8; ++j) atomicAdd(d + vox[j], w[j] * g);
}

// ---- interpolation (oriented) ------------------------------------------------------------------------------------------------------------------
struct RoiLerp { int i0, i1; float l0, l1; };          // one axis of F.interpolate(trilinear, align_corners=True): grid points i0 <= i1 < g and their weights
__device__ __forceinline__ RoiLerp roi_lerp(int g, int O, int o) {
  const float s = O > 1 ? (float)(g - 1) / (float)(O - 1) : 0.f, src = s * (float)o;
  RoiLerp r;
  r.i0 = min((int)src, g - 1);
  r.i1 = r.i0 + (r.i0 < g - 1 ? 1 : 0);
  r.l1 = fminf(fmaxf(src - (float)r.i0, 0.f), 1.f);
  r.l0 = 1.f - r.l1;
  return r;
}
// the up to 8 grid points of one output cell: fn(weight of the point, its eight corner voxels, their weights); points of weight 0 and masked points are left out
template <class F>
__device__ __forceinline__ void roi_interp_points(const RoiPoolGeom& G, const float* __restrict__ box, int lvl, int cell, F&& fn) {
  const int W = pick4(G.W, lvl), H = pick4(G.H, lvl), D = pick4(G.D, lvl);
  RoiAxis ax[3];
  RoiPose P;
  roi_axes_obb(G, box, lvl, ax, P);
  const int oz = cell % G.od, oy = (cell / G.od) % G.oh, ox = cell / (G.od * G.oh);
  const RoiLerp lx = roi_lerp(ax[0].s, G.ow, ox), ly = roi_lerp(ax[1].s, G.oh, oy), lz = roi_lerp(ax[2].s, G.od, oz);
  for (int j = 0; j < 8; ++j) {
    const bool a = j & 4, b = j & 2, c = j & 1;
    const float wt = (a ? lx.l1 : lx.l0) * (b ? ly.l1 : ly.l0) * (c ? lz.l1 : lz.l0);
    if (wt == 0.f) continue;
    int vox[8];
    float w[8];
    if (!roi_point(P, a ? lx.i1 : lx.i0, b ? ly.i1 : ly.i0, c ? lz.i1 : lz.i0, W, H, D, vox, w)) continue;
    fn(wt, vox, w);
  }
}

__global__ __launch_bounds__(256) void roi_interp_fwd_kernel(RoiPoolGeom G, Ptr4<const float> maps, const float* __restrict__ rois, const int* __restrict__ lvl_override,
                                                             float* __restrict__ out) {
  const long m = blockIdx.x / G.bpr;
  const int wi = (blockIdx.x - (int)(m * G.bpr)) * 256 + (int)threadIdx.x;
  const int nchunk = (G.C + ROI_CPL - 1) / ROI_CPL;
  if (m >= G.M || wi >= G.ncell * nchunk) return;
  const int cell = wi % G.ncell, c0 = (wi / G.ncell) * ROI_CPL;
  const int scene = (int)(m / G.R);
  const float* __restrict__ roi = rois + m * 8;
  const int lvl = roi_level(G, roi, lvl_override, m);
  float acc[ROI_CPL];
#pragma unroll
  for (int c = 0; c < ROI_CPL; ++c) acc[c] = 0.f;
  if (lvl >= 0) {
    const long vol = (long)pick4(G.W, lvl) * pick4(G.H, lvl) * pick4(G.D, lvl);
    const float* __restrict__ f = pick4(maps.p, lvl) + ((long)scene * G.C + c0) * vol;
    roi_interp_points(G, roi + 1, lvl, cell, [&](float wt, const int (&vox)[8], const float (&w)[8]) {
#pragma unroll
      for (int c = 0; c < ROI_CPL; ++c) {
        if (c0 + c < G.C) {
          float v = 0.f;
#pragma unroll
          for (int j = 0; j < 8; ++j) v += f[c * vol + vox[j]] * w[j];
          acc[c] += wt * v;
        }
      }
    });
  }
#pragma unroll
  for (int c = 0; c < ROI_CPL; ++c)
    if (c0 + c < G.C) out[(m * G.C + c0 + c) * G.ncell + cell] = acc[c];
}

// one lane per output element, as the pooling backward; the geometry is formed again from the RoI
__global__ __launch_bounds__(256) void roi_interp_bwd_kernel(RoiPoolGeom G, long total, const float* __restrict__ dout, const float* __restrict__ rois,
                                                             const int* __restrict__ lvl_override, Ptr4<float> dmaps) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const long mc = e / G.ncell, m = mc / G.C;
  const int cell = (int)(e - mc * G.ncell), c = (int)(mc - m * G.C);
  const float* __restrict__ roi = rois + m * 8;
  const int lvl = roi_level(G, roi, lvl_override, m);
  if (lvl < 0) return;
  float* __restrict__ d = pick4(dmaps.p, lvl);
  if (!d) return;
  const long vol = (long)pick4(G.W, lvl) * pick4(G.H, lvl) * pick4(G.D, lvl);
  d += ((m / G.R) * G.C + c) * vol;
  const float g = dout[e];
  roi_interp_points(G, roi + 1, lvl, cell, [&](float wt, const int (&vox)[8], const float (&w)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) atomicAdd(d + vox[j], w[j] * (wt * g));
  });
}

// ---- losses ----------------------------------------------------------------------------------------------------------------------------------
// RotatedCoder.encode_single
__device__ __forceinline__ void roi_encode_obb(const float* __restrict__ g, const float* __restrict__ e, float (&o)[8]) {
  const float dx = g[0] - e[0], dy = g[1] - e[1], dz = g[2] - e[2], cs = cosf(e[6]), sn = sinf(e[6]);
  o[0] = (cs * dx + sn * dy) / e[3];
  o[1] = (-sn * dx + cs * dy) / e[4];
  o[2] = dz / e[5];
  o[3] = logf(g[3] / e[3]); o[4] = logf(g[4] / e[4]); o[5] = logf(g[5] / e[5]);
  o[6] = (g[6] - e[6]) / 6.28318530717958647692f;
  o[7] = 0.f;
}

__device__ __forceinline__ int roi_label(float lab, int ncls) { return lab >= 0.f && lab < (float)ncls ? (int)lab : -1; }

template <bool ORIENTED>
__global__ __launch_bounds__(256) void roi_loss_fwd_kernel(long M, int ncls, const float* __restrict__ scores, const float* __restrict__ deltas, const float* __restrict__ labels,
                                                           const float* __restrict__ rois, int rstride, const float* __restrict__ gt_rois, float* __restrict__ targets,
                                                           float* __restrict__ partials) {
  constexpr int B = ORIENTED ? 7 : 6;
  const long m = (long)blockIdx.x * 256 + threadIdx.x;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  if (m < M) {
    const int li = roi_label(labels[m], ncls);
    float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (li >= 0) {
      const float* __restrict__ s = scores + m * ncls;
      float mx, sum;
      row_softmax(s, ncls, mx, sum);
      v[0] = mx + logf(sum) - s[li];
      v[2] = 1.f;
      const float* __restrict__ e = rois + m * rstride + (rstride - B);
      if (ORIENTED) roi_encode_obb(gt_rois + m * B, e, o);
      else rpn_encode_aabb(gt_rois + m * B, roi_box6(e), o);
      if (li > 0) {
        v[3] = 1.f;
#pragma unroll
        for (int k = 0; k < B; ++k) v[1] += rpn_sl1(deltas[m * B + k] - o[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < B; ++k) targets[m * B + k] = o[k];
  }
  block_sum_fixed(v, partials + 4 * (long)blockIdx.x);
}

// one workgroup: fixed-order sum of the partials -> scalars = (objectness loss, box loss, valid rows, positive rows)
__global__ __launch_bounds__(256) void roi_loss_final_kernel(const float* __restrict__ partials, int nblocks, float* __restrict__ scalars) {
  float sum[4];
  final_sum_fixed(partials, nblocks, sum);
  if (threadIdx.x != 0) return;
  scalars[0] = sum[2] > 0.f ? sum[0] / sum[2] : 0.f;
  scalars[1] = sum[3] > 0.f ? sum[1] / sum[3] : 0.f;
  scalars[2] = sum[2];
  scalars[3] = sum[3];
}

template <int B>
__global__ __launch_bounds__(256) void roi_loss_bwd_kernel(long M, int ncls, const float* __restrict__ scores, const float* __restrict__ deltas, const float* __restrict__ labels,
                                                           const float* __restrict__ targets, const float* __restrict__ scalars, const float* __restrict__ g_obj,
                                                           const float* __restrict__ g_reg, float* __restrict__ dscores, float* __restrict__ ddeltas) {
  const long m = (long)blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  const int li = roi_label(labels[m], ncls);
  const float nv = scalars[2], np = scalars[3];
  const float* __restrict__ s = scores + m * ncls;
  float* __restrict__ ds = dscores + m * ncls;
  if (li >= 0 && nv > 0.f && g_obj) {
    const float sc = g_obj[0] / nv;
    float mx, sum;
    row_softmax(s, ncls, mx, sum);
    for (int c = 0; c < ncls; ++c) ds[c] = (expf(s[c] - mx) / sum - (c == li ? 1.f : 0.f)) * sc;
  } else {
    for (int c = 0; c < ncls; ++c) ds[c] = 0.f;
  }
  const bool pos = li > 0 && np > 0.f && g_reg;
  const float sc = pos ? g_reg[0] / np : 0.f;
#pragma unroll
  for (int k = 0; k < B; ++k) ddeltas[m * B + k] = pos ? rpn_sl1_grad(deltas[m * B + k] - targets[m * B + k]) * sc : 0.f;
}

// ---- decode ----------------------------------------------------------------------------------------------------------------------------------
template <bool ORIENTED>
__global__ __launch_bounds__(256) void roi_decode_kernel(long M, const float* __restrict__ deltas, const float* __restrict__ rois, int rstride, float* __restrict__ out) {
  constexpr int B = ORIENTED ? 7 : 6;
  const long m = (long)blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  roi_decode_box<ORIENTED>(deltas + m * B, rois + m * rstride + (rstride - B), out + m * B);
}

int roi_offs(int N, const int* offs, RoiOffs& S) {
  if (N < 1 || N > NMH_FCOS_MAX_SCENES || !offs || offs[0] != 0) return -4;
  for (int b = 0; b < N; ++b) if (offs[b + 1] < offs[b]) return -4;
  for (int b = 0; b <= NMH_FCOS_MAX_SCENES; ++b) S.off[b] = offs[b < N ? b : N];
  return 0;
}

// dims: [nlevels][3] = (W, H, D)
int roi_pool_geom(int nlevels, const int* dims, const float* scales, int N, int C, int R, int ow, int oh, int od, float enlarge, RoiPoolGeom& G) {
  if (nlevels < 1 || nlevels > 4 || !dims || !scales || N < 1 || N > NMH_FCOS_MAX_SCENES || C < 1 || R < 1 || ow < 1 || oh < 1 || od < 1) return -4;
  if ((long)ow * oh * od > NMH_ROI_MAX_CELLS || !(enlarge > 0.f)) return -4;
  G.L = nlevels; G.N = N; G.C = C; G.R = R; G.M = (long)N * R;
  for (int k = 0; k < 4; ++k) {
    const int j = k < nlevels ? k : nlevels - 1;
    const int* d = dims + 3 * j;
    if (d[0] < 1 || d[1] < 1 || d[2] < 1 || (long)d[0] * d[1] * d[2] >= (1L << 31) || !(scales[j] > 0.f)) return -4;
    G.W[k] = d[0]; G.H[k] = d[1]; G.D[k] = d[2]; G.scale[k] = scales[j];
  }
  G.ow = ow; G.oh = oh; G.od = od; G.ncell = ow * oh * od;
  const int nchunk = (C + ROI_CPL - 1) / ROI_CPL;
  const long per = ((long)G.ncell * nchunk + 255) / 256;
  if (per * G.M >= (1L << 31) - 1 || G.M * C * G.ncell >= (1L << 40)) return -4;
  G.bpr = (int)per;
  G.enlarge = enlarge;
  return 0;
}

}  // namespace

int k_roi_targets(int N, int cap, int ncols, int R, int is_sample, const float* boxes, const int* levels, const int* counts, const float* gt, const float* gt_labels, const int* offs,
                  int want_fg, float fg, float bg, long* rng, float* miou, int* arg, int* lists, int* keep, int* counts2, float* labels, float* rois, float* gt_rois,
                  hipStream_t st) {
  RoiOffs S;
  if (roi_offs(N, offs, S) || cap < 1 || cap > (1 << 24) || R < 1 || R > (1 << 24) || (ncols != 6 && ncols != 7) || (!is_sample && R != cap)) return -4;
  if (offs[N] > 0 && (!gt || !gt_labels)) return -4;
  if (is_sample && rng && !lists) return -4;
  const dim3 grid_cap((cap + 255) / 256, N), grid_r((R + 255) / 256, N);
  if (ncols == 7) hipLaunchKernelGGL(roi_match_kernel<true>, grid_cap, dim3(256), 0, st, S, cap, boxes, counts, gt, miou, arg);
  else hipLaunchKernelGGL(roi_match_kernel<false>, grid_cap, dim3(256), 0, st, S, cap, boxes, counts, gt, miou, arg);
  NMH_CHECK_LAUNCH();
  if (is_sample && rng) {            // without rng the caller has filled keep and counts2
    hipLaunchKernelGGL(roi_sample_kernel, dim3(N), dim3(SEL_T), 0, st, miou, counts, cap, R, want_fg, fg, bg, rng, lists, keep, counts2);
    NMH_CHECK_LAUNCH();
    hipLaunchKernelGGL(rpn_rng_advance_kernel, dim3(1), dim3(64), 0, st, rng);
    NMH_CHECK_LAUNCH();
  }
  if (ncols == 7) hipLaunchKernelGGL(roi_gather_kernel<7>, grid_r, dim3(256), 0, st, S, cap, R, is_sample, boxes, levels, counts, gt, gt_labels, miou, arg, fg, keep, counts2, labels, rois, gt_rois);
  else hipLaunchKernelGGL(roi_gather_kernel<6>, grid_r, dim3(256), 0, st, S, cap, R, is_sample, boxes, levels, counts, gt, gt_labels, miou, arg, fg, keep, counts2, labels, rois, gt_rois);
  NMH_CHECK_LAUNCH();
  return 0;
}

int k_roi_level_map(long M, const float* boxes, int stride, int ncols, int k_min, int k_max, float canonical_scale, float canonical_level, float eps, int* out, hipStream_t st) {
  if (M < 1 || M >= (1L << 38) || (ncols != 6 && ncols != 7) || stride < ncols || stride > ncols + 1 || k_max < k_min || !(canonical_scale > 0.f)) return -4;
  hipLaunchKernelGGL(roi_level_map_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, M, boxes, stride, stride - ncols, k_min, k_max, canonical_scale, canonical_level, eps, out);
  NMH_CHECK_LAUNCH();
  return 0;
}

int k_roi_pool_fwd(int nlevels, const int* dims, const float* scales, int N, int C, int R, int ncols, int ow, int oh, int od, float enlarge, const float* const* maps, const float* rois,
                   const int* lvl_override, float* out, int* argout, hipStream_t st) {
  RoiPoolGeom G;
  if (roi_pool_geom(nlevels, dims, scales, N, C, R, ow, oh, od, enlarge, G) || (ncols != 6 && ncols != 7) || !all_set(nlevels, maps)) return -4;
  const Ptr4<const float> P = make_ptrs<const float>(nlevels, maps);
  const dim3 grid((unsigned)(G.M * G.bpr));
  if (ncols == 7) hipLaunchKernelGGL(roi_pool_fwd_kernel<true>, grid, dim3(256), 0, st, G, P, rois, lvl_override, out, argout);
  else hipLaunchKernelGGL(roi_pool_fwd_kernel<false>, grid, dim3(256), 0, st, G, P, rois, lvl_override, out, argout);
  NMH_CHECK_LAUNCH();
  return 0;
}

int k_roi_pool_bwd(int nlevels, const int* dims, const float* scales, int N, int C, int R, int ncols, int ow, int oh, int od, float enlarge, const float* dout, const int* argout,
                   const float* rois, const int* lvl_override, float* const* dmaps, hipStream_t st) {
  RoiPoolGeom G;
  if (roi_pool_geom(nlevels, dims, scales, N, C, R, ow, oh, od, enlarge, G) || (ncols != 6 && ncols != 7) || !dmaps) return -4;
  Ptr4<float> P;
  for (int k = 0; k < 4; ++k) P.p[k] = k < nlevels ? dmaps[k] : nullptr;       // a null level takes no gradient
  const long total = G.M * C * G.ncell;
  if ((total + 255) / 256 >= (1L << 31) - 1) return -4;
  if (ncols == 7) hipLaunchKernelGGL(roi_pool_bwd_kernel<true>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, G, total, dout, argout, rois, lvl_override, P);
  else hipLaunchKernelGGL(roi_pool_bwd_kernel<false>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, G, total, dout, argout, rois, lvl_override, P);
  NMH_CHECK_LAUNCH();
  return 0;
}

int k_roi_interp_fwd(int nlevels, const int* dims, const float* scales, int N, int C, int R, int ncols, int ow, int oh, int od, float enlarge, const float* const* maps, const float* rois,
                     const int* lvl_override, float* out, hipStream_t st) {
  RoiPoolGeom G;
  if (roi_pool_geom(nlevels, dims, scales, N, C, R, ow, oh, od, enlarge, G) || ncols != 7 || !all_set(nlevels, maps)) return -4;
  hipLaunchKernelGGL(roi_interp_fwd_kernel, dim3((unsigned)(G.M * G.bpr)), dim3(256), 0, st, G, make_ptrs<const float>(nlevels, maps), rois, lvl_override, out);
  NMH_CHECK_LAUNCH();
  return 0;
}

int k_roi_interp_bwd(int nlevels, const int* dims, const float* scales, int N, int C, int R, int ncols, int ow, int oh, int od, float enlarge, const float* dout, const float* rois,
                     const int* lvl_override, float* const* dmaps, hipStream_t st) {
  RoiPoolGeom G;
  if (roi_pool_geom(nlevels, dims, scales, N, C, R, ow, oh, od, enlarge, G) || ncols != 7 || !dmaps) return -4;
  Ptr4<float> P;
  for (int k = 0; k < 4; ++k) P.p[k] = k < nlevels ? dmaps[k] : nullptr;       // a null level takes no gradient
  const long total = G.M * C * G.ncell;
  if ((total + 255) / 256 >= (1L << 31) - 1) return -4;
  hipLaunchKernelGGL(roi_interp_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, G, total, dout, rois, lvl_override, P);
  NMH_CHECK_LAUNCH();
  return 0;
}

long k_roi_loss_blocks(long M) { return M < 1 || M >= (1L << 38) ? -1 : (M + 255) / 256; }

int k_roi_loss_fwd(long M, int n_classes, int ncols, const float* scores, const float* deltas, const float* labels, const float* rois, int roi_stride, const float* gt_rois,
                   float* targets, float* partials, float* scalars, hipStream_t st) {
  const long nb = k_roi_loss_blocks(M);
  if (nb < 1 || n_classes < 1 || n_classes > NMH_ROI_MAX_CLASSES || (ncols != 6 && ncols != 7) || roi_stride < ncols || roi_stride > ncols + 1) return -4;
  if (ncols == 7) hipLaunchKernelGGL(roi_loss_fwd_kernel<true>, dim3((unsigned)nb), dim3(256), 0, st, M, n_classes, scores, deltas, labels, rois, roi_stride, gt_rois, targets, partials);
  else hipLaunchKernelGGL(roi_loss_fwd_kernel<false>, dim3((unsigned)nb), dim3(256), 0, st, M, n_classes, scores, deltas, labels, rois, roi_stride, gt_rois, targets, partials);
  NMH_CHECK_LAUNCH();
  hipLaunchKernelGGL(roi_loss_final_kernel, dim3(1), dim3(256), 0, st, partials, (int)nb, scalars);
  NMH_CHECK_LAUNCH();
  return 0;
}

int k_roi_loss_bwd(long M, int n_classes, int ncols, const float* scores, const float* deltas, const float* labels, const float* targets, const float* scalars, const float* g_obj,
                   const float* g_reg, float* dscores, float* ddeltas, hipStream_t st) {
  const long nb = k_roi_loss_blocks(M);
  if (nb < 1 || n_classes < 1 || n_classes > NMH_ROI_MAX_CLASSES || (ncols != 6 && ncols != 7)) return -4;
  if (ncols == 7) hipLaunchKernelGGL(roi_loss_bwd_kernel<7>, dim3((unsigned)nb), dim3(256), 0, st, M, n_classes, scores, deltas, labels, targets, scalars, g_obj, g_reg, dscores, ddeltas);
  else hipLaunchKernelGGL(roi_loss_bwd_kernel<6>, dim3((unsigned)nb), dim3(256), 0, st, M, n_classes, scores, deltas, labels, targets, scalars, g_obj, g_reg, dscores, ddeltas);
  NMH_CHECK_LAUNCH();
  return 0;
}

int k_roi_decode(long M, int ncols, const float* deltas, const float* rois, int roi_stride, float* out, hipStream_t st) {
  const long nb = k_roi_loss_blocks(M);
  if (nb < 1 || (ncols != 6 && ncols != 7) || roi_stride < ncols || roi_stride > ncols + 1) return -4;
  if (ncols == 7) hipLaunchKernelGGL(roi_decode_kernel<true>, dim3((unsigned)nb), dim3(256), 0, st, M, deltas, rois, roi_stride, out);
  else hipLaunchKernelGGL(roi_decode_kernel<false>, dim3((unsigned)nb), dim3(256), 0, st, M, deltas, rois, roi_stride, out);
  NMH_CHECK_LAUNCH();
  return 0;
}

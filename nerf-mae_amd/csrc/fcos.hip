// FCOS training losses and target assignment of the reference's 3-D detector head, as gfx950 kernels:
//   fcos_assign   FCOSLossComputation.prepare_targets, compute_targets_for_locations[_obb], get_sample_region, compute_centerness_targets
//                 (nerf_rpn/model/fcos/loss.py:210-445), compute_locations / compute_padding_masks (fcos/fcos.py:282-299), with encode_fcos_obb
//                 (fcos/utils.py:64-105);
//   fcos_focal    torchvision.ops.sigmoid_focal_loss(reduction="sum") / num_pos_avg (loss.py:538-542), forward and backward;
//   fcos_pos      IOULoss (loss.py:77-132) / RotatedIOULoss (loss.py:135-171) over decode_fcos_obb (fcos/utils.py:12-61), the additional
//                 SmoothL1 (loss.py:570-577) and the centerness BCE (loss.py:565-568), forward and backward;
//   fcos_obb_encode / fcos_obb_decode   encode_fcos_obb / decode_fcos_obb on their own.
// fp32 throughout; one lane owns one (scene, location); nothing goes to scratch; every kernel writes only its own outputs for any input.
//
// Dense layout.  Level k has feature size (w, l, h), n_k = w l h locations and stride s_k; there are N scenes and 1..4 levels.  The dense
// index of (level k, scene b, location q) is p = N (n_0 + .. + n_{k-1}) + b n_k + q, the order of the per-level (N, 1, w, l, h) tensors
// flattened and concatenated (the reference's labels_level_first).  Location q = (i l + j) h + k3 sits at (s i + s/2, s j + s/2, s k3 + s/2)
// (integer division); locations are never stored.  P = N sum n_k.  Head outputs are read in place: channel c of level k at
// ((b C + c) n_k + q); gradients are written in the same layout.
//
// Assignment.  Ground-truth boxes are one [G_total][6|7] array, scene b owning rows off[b] .. off[b+1]-1.  Per box, once per workgroup and
// staged in LDS in chunks of 64:
//   6 columns (x0,y0,z0,x1,y1,z1): the AABB is the box;
//   7 columns (x,y,z,w,l,h,theta): BEV corners as box2corners_th; AABB = their extent and z -+ h/2; with xt = corner x where ymax - y <= 0.1
//     (else -1e6), yt = corner y where xmax - x <= 0.1 (else 1e6): vx = max xt, vy = min yt; if isclose(vx, xmax) and isclose(vy, ymin)
//     (|a-b| <= 1e-8 + 1e-5 |b|) then (vx, vy) = (xmax, ymin); alpha = (vx - x) / (xmax - xmin), beta = (vy - y) / (ymax - ymin);
//   volume = product of the AABB's extents.
// Per location (X,Y,Z) and box: d = (X-x0, Y-y0, Z-z0, x1-X, y1-Y, z1-Z).  in_box: radius > 0: with c = AABB centre and r = s_k radius the
// region [max(c-r, lo), min(c+r, hi)] per axis, min of the six distances to it > 0; else min d > 0.  in_range: lo_k <= max d <= hi_k with
// (lo, hi) = (-1,16), (16,32), (32,64), (64,1e8) for level 0..3.  Winner: smallest volume among in_box and in_range and volume < 1e8, ties
// to the lowest index.  label = 1 with a winner else 0; targets = d of the winner (then alpha, beta), zeros without one; norm_targets divides
// the six distances by s_k; gt_index = the winner's row within its scene or -1; centerness = sqrt(prod over axes of min/max of the two
// opposite targets), 0 without a winner; valid = mask byte if masks are given, else location < size on all axes if sizes are given, else 1.
// scalars = (number of valid positives, sum of their centerness): per-workgroup partials, then a fixed-order pass of one workgroup.
//
// Losses.  norm_pos = max(scalars[0] / world, 1), norm_ctr = scalars[1] / world.
//   cls  = sum over valid of focal(x, label) / norm_pos;  focal = a_t ce (1 - p_t)^2, alpha 0.25, gamma 2 (torchvision 0.13.1)
//   reg  = sum over valid positives of ctr_target (term + [l1]) / norm_ctr, 0 if scalars[1] == 0
//   ctr  = sum over valid positives of bce_with_logits(c, ctr_target) / norm_pos
//   term, 6 columns: IOULoss with +1.0 smoothing and 1e-7 (iou: -log, linear_iou: 1 - ious, giou: 1 - gious)
//   term, 8 columns: A = decode(pred), B = decode(target) at a zero location; iou: -log((inter3d + 1) / (u3d + 1)), linear_iou: 1 - that,
//     giou / diou: the "smallest" enclosing forms of obb_geom.hpp.  decode keeps the clamp of vx, vy to the AABB, the 1e-7 in the
//     normalisation and mid (0,0) -> (1e-7, 0); cos / sin of theta are taken from mid directly.  The gradient goes by hand through the pair
//     geometry and the decode; clamp passes to the bound it hits, max(d0, d1) splits a tie evenly.  l1 = SmoothL1(beta 1) on columns 6:8.
//   fcos_pos2d (8 columns only, opt-in): term += proj2d_weight T(A, B) / 160 / 16 with T the 2-D projection term of proj2d.hpp between the same two decoded
//     boxes under the cameras of get_w2cs(160), whatever the scene size (compute_2d_projection_loss, loss.py:447-475, 579-585: the reference's literal);
//     its gradient goes through fcos_decode_bwd with the pair geometry's.
// Backward kernels recompute everything from the inputs and write every element of the gradients: exactly 0 where label == 0 or !valid.
#include "common.hpp"
#include "kernels.hpp"
#include "obb_geom.hpp"
#include "fcos_decode.hpp"
#include "levels4.hpp"
#include "reduce_fixed.hpp"
#include "proj2d.hpp"

namespace {

constexpr float FCOS_INF = 100000000.f;
constexpr int FCOS_CHUNK = 64;

struct FcosGeom {            // kernel argument, by value
  int L, N;
  int w[4], l[4], h[4], s[4], n[4];
  int blk0[4], bpl[4];       // first workgroup of the level, workgroups per scene
  long p0[4];                // dense index of (level, scene 0, location 0)
  int nblocks;
};
struct FcosOffs { int off[NMH_FCOS_MAX_SCENES + 1]; };

struct Where { int lvl, scene, loc, n; long p; bool active; };
__device__ __forceinline__ Where fcos_where(const FcosGeom& G) {
  const LevelItem at = level_item(G.blk0, G.bpl, G.L);
  Where q;
  q.lvl = at.lvl; q.scene = at.scene; q.loc = at.i;
  q.n = pick4(G.n, q.lvl);
  q.active = q.loc < q.n;
  q.p = pick4(G.p0, q.lvl) + (long)q.scene * q.n + q.loc;
  return q;
}

// one workgroup: fixed-order sum of the per-workgroup partials, then the normalisation
enum { FIN_SCALARS = 0, FIN_CLS = 1, FIN_POS = 2 };
__global__ __launch_bounds__(256) void fcos_final_kernel(const float* __restrict__ partials, int nblocks, int what, float world, float* __restrict__ scalars, float* __restrict__ out0,
                                                         float* __restrict__ out1) {
  float sum[2];
  final_sum_fixed(partials, nblocks, sum);
  if (threadIdx.x != 0) return;
  const float a = sum[0], b = sum[1];
  if (what == FIN_SCALARS) { scalars[0] = a; scalars[1] = b; return; }
  const float norm_pos = fmaxf(scalars[0] / world, 1.f), csum = scalars[1];
  if (what == FIN_CLS) { out0[0] = a / norm_pos; return; }
  out0[0] = csum > 0.f ? a / (csum / world) : 0.f;
  out1[0] = b / norm_pos;
}

// ---- encode / decode ---------------------------------------------------------------------------------------------------------------------
struct GtBox { float x0, y0, z0, x1, y1, z1, vol, alpha, beta; };
__device__ __forceinline__ GtBox fcos_gt_aabb(const float* __restrict__ b) {
  GtBox g;
  g.x0 = b[0]; g.y0 = b[1]; g.z0 = b[2]; g.x1 = b[3]; g.y1 = b[4]; g.z1 = b[5];
  g.vol = (g.x1 - g.x0) * (g.y1 - g.y0) * (g.z1 - g.z0);
  g.alpha = g.beta = 0.f;
  return g;
}
__device__ __forceinline__ bool fcos_isclose(float a, float b) { return fabsf(a - b) <= 1e-8f + 1e-5f * fabsf(b); }
__device__ __forceinline__ GtBox fcos_gt_obb(const float* __restrict__ b) {
  const float x = b[0], y = b[1], z = b[2], w = b[3], l = b[4], h = b[5], sn = sinf(b[6]), cs = cosf(b[6]);
  const float ux = 0.5f * w * cs, uy = 0.5f * w * sn, vx_ = -0.5f * l * sn, vy_ = 0.5f * l * cs;
  const float X[4] = {x + ux + vx_, x - ux + vx_, x - ux - vx_, x + ux - vx_}, Y[4] = {y + uy + vy_, y - uy + vy_, y - uy - vy_, y + uy - vy_};
  GtBox g;
  g.x0 = fminf(fminf(X[0], X[1]), fminf(X[2], X[3])); g.x1 = fmaxf(fmaxf(X[0], X[1]), fmaxf(X[2], X[3]));
  g.y0 = fminf(fminf(Y[0], Y[1]), fminf(Y[2], Y[3])); g.y1 = fmaxf(fmaxf(Y[0], Y[1]), fmaxf(Y[2], Y[3]));
  g.z0 = z - h / 2.f; g.z1 = z + h / 2.f;
  float vx = -3.0e38f, vy = 3.0e38f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    vx = fmaxf(vx, g.y1 - Y[k] > 0.1f ? -1e6f : X[k]);
    vy = fminf(vy, g.x1 - X[k] > 0.1f ? 1e6f : Y[k]);
  }
  if (fcos_isclose(vx, g.x1) && fcos_isclose(vy, g.y0)) { vx = g.x1; vy = g.y0; }
  g.alpha = (vx - x) / (g.x1 - g.x0);
  g.beta = (vy - y) / (g.y1 - g.y0);
  g.vol = (g.x1 - g.x0) * (g.y1 - g.y0) * (g.z1 - g.z0);
  return g;
}

// gradient of the decoded box (x, y, z, w, l, h, theta) -> gradient of the eight regression values
__device__ __forceinline__ void fcos_decode_bwd(const Dec& d, const BoxGrad& g, float (&gr)[8]) {
  const bool zero = d.mx == 0.f && d.my == 0.f;
  const float in = zero ? 0.f : 1.f / d.n, mx = zero ? 1e-7f : d.mx, n2 = mx * mx + d.my * d.my;
  // w = 2 |mid|, theta = atan2(my, mx); the (0,0) -> 1e-7 assignment cuts the gradient of mx there
  float gmx = 2.f * g.w * d.mx * in + (zero ? 0.f : -g.t * d.my / n2), gmy = 2.f * g.w * d.my * in + g.t * mx / n2;
  // l = |a0 - a1|
  const float il = d.el > 0.f ? 1.f / d.el : 0.f, gex = g.l * d.ex * il, gey = g.l * d.ey * il;
  const float ga0x = gex + 0.5f * gmx, ga0y = gey + 0.5f * gmy, ga1x = -gex + 0.5f * gmx, ga1y = -gey + 0.5f * gmy;
  // a0 = v0 dmax / (d0 + eps), a1 = v1 dmax / (d1 + eps)
  const float q0 = 1.f / (d.d0 + 1e-7f), q1 = 1.f / (d.d1 + 1e-7f), s0 = d.dmax * q0, s1 = d.dmax * q1;
  const float gs0 = ga0x * d.v0x + ga0y * d.v0y, gs1 = ga1x * d.v1x + ga1y * d.v1y;
  const float gdmax = gs0 * q0 + gs1 * q1, share0 = pick_a<false>(d.d0, d.d1);
  const float gd0 = -gs0 * d.dmax * q0 * q0 + gdmax * share0, gd1 = -gs1 * d.dmax * q1 * q1 + gdmax * (1.f - share0);
  const float i0 = d.d0 > 0.f ? 1.f / d.d0 : 0.f, i1 = d.d1 > 0.f ? 1.f / d.d1 : 0.f;
  const float gv0x = ga0x * s0 + gd0 * d.v0x * i0, gv0y = ga0y * s0 + gd0 * d.v0y * i0, gv1x = ga1x * s1 + gd1 * d.v1x * i1, gv1y = ga1y * s1 + gd1 * d.v1y * i1;
  // v0 = (vx - cx, y1 - cy), v1 = (x1 - cx, vy - cy); box centre = (cx, cy)
  const float gcx = g.x - gv0x - gv1x, gcy = g.y - gv0y - gv1y;
  float gx0 = 0.5f * gcx, gx1 = 0.5f * gcx + gv1x, gy0 = 0.5f * gcy, gy1 = 0.5f * gcy + gv0y;
  // vx = clamp(vxr, x0, x1), vxr = (x1 + x0) / 2 + r6 (x1 - x0)
  float gr6 = 0.f, gr7 = 0.f;
  if (d.vxr < d.x0) gx0 += gv0x;
  else if (d.vxr > d.x1) gx1 += gv0x;
  else { gx0 += gv0x * (0.5f - d.r6); gx1 += gv0x * (0.5f + d.r6); gr6 = gv0x * (d.x1 - d.x0); }
  if (d.vyr < d.y0) gy0 += gv1y;
  else if (d.vyr > d.y1) gy1 += gv1y;
  else { gy0 += gv1y * (0.5f - d.r7); gy1 += gv1y * (0.5f + d.r7); gr7 = gv1y * (d.y1 - d.y0); }
  // z0 = -r2, z1 = r5: centre (z0 + z1) / 2, h = z1 - z0
  gr[0] = -gx0; gr[1] = -gy0; gr[2] = -(0.5f * g.z - g.h);
  gr[3] = gx1; gr[4] = gy1; gr[5] = 0.5f * g.z + g.h;
  gr[6] = gr6; gr[7] = gr7;
}

__global__ __launch_bounds__(256) void fcos_obb_encode_kernel(const float* __restrict__ loc, const float* __restrict__ boxes, long n, float* __restrict__ out) {
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const GtBox g = fcos_gt_obb(boxes + p * 7);
  const float X = loc[p * 3], Y = loc[p * 3 + 1], Z = loc[p * 3 + 2];
  float* q = out + p * 8;
  q[0] = X - g.x0; q[1] = Y - g.y0; q[2] = Z - g.z0; q[3] = g.x1 - X; q[4] = g.y1 - Y; q[5] = g.z1 - Z; q[6] = g.alpha; q[7] = g.beta;
}
__global__ __launch_bounds__(256) void fcos_obb_decode_fwd_kernel(const float* __restrict__ loc, const float* __restrict__ reg, long n, float* __restrict__ out) {
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  float r[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) r[k] = reg[p * 8 + k];
  const Dec d = fcos_decode(r);
  const bool zero = d.mx == 0.f && d.my == 0.f;
  float* q = out + p * 7;
  q[0] = loc[p * 3] + d.o.x; q[1] = loc[p * 3 + 1] + d.o.y; q[2] = loc[p * 3 + 2] + d.o.z;
  q[3] = d.o.w; q[4] = d.o.l; q[5] = d.o.h; q[6] = atan2f(d.my, zero ? 1e-7f : d.mx);
}
__global__ __launch_bounds__(256) void fcos_obb_decode_bwd_kernel(const float* __restrict__ reg, const float* __restrict__ gbox, long n, float* __restrict__ dreg) {
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  float r[8], gr[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) r[k] = reg[p * 8 + k];
  const Dec d = fcos_decode(r);
  const float* g = gbox + p * 7;
  const BoxGrad G{g[0], g[1], g[2], g[3], g[4], g[5], g[6]};
  fcos_decode_bwd(d, G, gr);
#pragma unroll
  for (int k = 0; k < 8; ++k) dreg[p * 8 + k] = gr[k];
}

// ---- assignment ------------------------------------------------------------------------------------------------------------------------
template <bool ORIENTED>
__global__ __launch_bounds__(256) void fcos_assign_kernel(FcosGeom G, FcosOffs S, const float* __restrict__ boxes, const int* __restrict__ sizes, Ptr4<const unsigned char> masks,
                                                          int have_masks, float radius, int norm_targets, float* __restrict__ labels, float* __restrict__ targets,
                                                          int* __restrict__ gt_index, float* __restrict__ ctr_t, unsigned char* __restrict__ valid, float* __restrict__ partials) {
  constexpr int C = ORIENTED ? 8 : 6;
  __shared__ GtBox sb[FCOS_CHUNK];
  const Where q = fcos_where(G);
  const int t = threadIdx.x, lw = pick4(G.l, q.lvl), hw = pick4(G.h, q.lvl), s = pick4(G.s, q.lvl);
  const int i3 = q.loc % hw, i2 = (q.loc / hw) % lw, i1 = q.loc / (hw * lw);
  const int xi = s * i1 + s / 2, yi = s * i2 + s / 2, zi = s * i3 + s / 2;
  const float X = (float)xi, Y = (float)yi, Z = (float)zi;
  const float lo = q.lvl == 0 ? -1.f : (q.lvl == 1 ? 16.f : (q.lvl == 2 ? 32.f : 64.f)), hi = q.lvl == 0 ? 16.f : (q.lvl == 1 ? 32.f : (q.lvl == 2 ? 64.f : FCOS_INF));
  const float rs = (float)s * radius;
  const int g0 = S.off[q.scene], g1 = S.off[q.scene + 1];
  float best = FCOS_INF;
  int bi = -1;
  GtBox win{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int c = g0; c < g1; c += FCOS_CHUNK) {        // uniform over the workgroup
    __syncthreads();
    if (t < FCOS_CHUNK && c + t < g1) sb[t] = ORIENTED ? fcos_gt_obb(boxes + (long)(c + t) * 7) : fcos_gt_aabb(boxes + (long)(c + t) * 6);
    __syncthreads();
    const int m = min(FCOS_CHUNK, g1 - c);
    if (q.active) {
      for (int k = 0; k < m; ++k) {
        const GtBox b = sb[k];
        const float dl = X - b.x0, dt = Y - b.y0, df = Z - b.z0, dr = b.x1 - X, db = b.y1 - Y, da = b.z1 - Z;
        float mn;
        if (radius > 0.f) {
          const float cx = (b.x0 + b.x1) / 2.f, cy = (b.y0 + b.y1) / 2.f, cz = (b.z0 + b.z1) / 2.f;
          const float ax = fmaxf(cx - rs, b.x0), ay = fmaxf(cy - rs, b.y0), az = fmaxf(cz - rs, b.z0);
          const float bx = fminf(cx + rs, b.x1), by = fminf(cy + rs, b.y1), bz = fminf(cz + rs, b.z1);
          mn = fminf(fminf(fminf(X - ax, bx - X), fminf(Y - ay, by - Y)), fminf(Z - az, bz - Z));
        } else {
          mn = fminf(fminf(fminf(dl, dr), fminf(dt, db)), fminf(df, da));
        }
        const float mx = fmaxf(fmaxf(fmaxf(dl, dr), fmaxf(dt, db)), fmaxf(df, da));
        if (mn > 0.f && mx >= lo && mx <= hi && b.vol < best) { best = b.vol; bi = c + k - g0; win = b; }
      }
    }
  }
  bool ok = false;
  float ct = 0.f;
  if (q.active) {
    float d[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (bi >= 0) {
      d[0] = X - win.x0; d[1] = Y - win.y0; d[2] = Z - win.z0; d[3] = win.x1 - X; d[4] = win.y1 - Y; d[5] = win.z1 - Z; d[6] = win.alpha; d[7] = win.beta;
      if (norm_targets) {
        const float fs = (float)s;
#pragma unroll
        for (int k = 0; k < 6; ++k) d[k] = d[k] / fs;
      }
      ct = sqrtf((fminf(d[0], d[3]) / fmaxf(d[0], d[3])) * (fminf(d[1], d[4]) / fmaxf(d[1], d[4])) * (fminf(d[2], d[5]) / fmaxf(d[2], d[5])));
    }
    bool v = true;
    if (have_masks) v = pick4(masks.p, q.lvl)[(long)q.scene * q.n + q.loc] != 0;
    else if (sizes) v = xi < sizes[q.scene * 3] && yi < sizes[q.scene * 3 + 1] && zi < sizes[q.scene * 3 + 2];
    labels[q.p] = bi >= 0 ? 1.f : 0.f;
    gt_index[q.p] = bi;
    ctr_t[q.p] = ct;
    valid[q.p] = v ? 1 : 0;
#pragma unroll
    for (int k = 0; k < C; ++k) targets[q.p * C + k] = d[k];
    ok = v && bi >= 0;
  }
  float sum[2] = {ok ? 1.f : 0.f, ok ? ct : 0.f};
  block_sum_fixed(sum, partials + 2 * (long)blockIdx.x);
}

// ---- focal loss ------------------------------------------------------------------------------------------------------------------------
// softplus(x), sigmoid(x), sigmoid(-x)
__device__ __forceinline__ void fcos_sig(float x, float& sp, float& p, float& q) {
  const float e = expf(-fabsf(x)), r = 1.f / (1.f + e);
  sp = fmaxf(x, 0.f) + log1pf(e);
  p = x >= 0.f ? r : e * r;
  q = x >= 0.f ? e * r : r;
}
__global__ __launch_bounds__(256) void fcos_focal_fwd_kernel(FcosGeom G, Ptr4<const float> cls, const float* __restrict__ labels, const unsigned char* __restrict__ valid,
                                                             float* __restrict__ partials) {
  const Where w = fcos_where(G);
  float v = 0.f;
  if (w.active && valid[w.p]) {
    const float x = pick4(cls.p, w.lvl)[(long)w.scene * w.n + w.loc];
    float sp, p, q;
    fcos_sig(x, sp, p, q);
    v = labels[w.p] > 0.f ? 0.25f * (sp - x) * q * q : 0.75f * sp * p * p;
  }
  float sum[2] = {v, 0.f};               // the second sum is not used
  block_sum_fixed(sum, partials + 2 * (long)blockIdx.x);
}
__global__ __launch_bounds__(256) void fcos_focal_bwd_kernel(FcosGeom G, Ptr4<const float> cls, const float* __restrict__ labels, const unsigned char* __restrict__ valid,
                                                             const float* __restrict__ scalars, float world, const float* __restrict__ g_out, Ptr4<float> dcls) {
  const Where w = fcos_where(G);
  if (!w.active) return;
  const long at = (long)w.scene * w.n + w.loc;
  float d = 0.f;
  if (valid[w.p]) {
    const float x = pick4(cls.p, w.lvl)[at];
    float sp, p, q;
    fcos_sig(x, sp, p, q);
    d = labels[w.p] > 0.f ? 0.25f * q * q * (-2.f * p * (sp - x) - q) : 0.75f * p * p * (p + 2.f * q * sp);
    d *= (g_out ? g_out[0] : 0.f) / fmaxf(scalars[0] / world, 1.f);
  }
  pick4(dcls.p, w.lvl)[at] = d;
}

// ---- regression and centerness on the positives ------------------------------------------------------------------------------------------
enum { FCOS_AABB = 0, FCOS_OBB_IOU = 1, FCOS_OBB_GIOU = 2, FCOS_OBB_DIOU = 3 };   // kernel template; loss_type within: 0 iou, 1 linear_iou, 2 giou, 3 diou
__device__ __forceinline__ float smooth_l1(float d) { const float a = fabsf(d); return a < 1.f ? 0.5f * d * d : a - 0.5f; }
__device__ __forceinline__ float smooth_l1_grad(float d) { return fabsf(d) < 1.f ? d : (d > 0.f ? 1.f : -1.f); }

// IOULoss term of one location; gp: its gradient with respect to the prediction (when GRAD)
template <bool GRAD>
__device__ __forceinline__ float fcos_aabb_term(const float (&p)[8], const float (&t)[8], int loss_type, float (&gp)[8]) {
  const float tw = t[0] + t[3], th = t[1] + t[4], td = t[2] + t[5], pw = p[0] + p[3], ph = p[1] + p[4], pd = p[2] + p[5];
  const float tv = tw * th * td, pv = pw * ph * pd;
  const float wi = fminf(p[0], t[0]) + fminf(p[3], t[3]), hi = fminf(p[4], t[4]) + fminf(p[1], t[1]), di = fminf(p[2], t[2]) + fminf(p[5], t[5]);
  const float gw = fmaxf(p[0], t[0]) + fmaxf(p[3], t[3]), gh = fmaxf(p[4], t[4]) + fmaxf(p[1], t[1]), gd = fmaxf(p[2], t[2]) + fmaxf(p[5], t[5]);
  const float ac = gw * gh * gd + 1e-7f, vi = wi * hi * di, vu = tv + pv - vi, ious = (vi + 1.f) / (vu + 1.f);
  const float loss = loss_type == 0 ? -logf(ious) : (loss_type == 1 ? 1.f - ious : 1.f - (ious - (ac - vu) / ac));
  if (GRAD) {
    const float gious = loss_type == 0 ? -1.f / ious : -1.f;
    float gvu = -gious * (vi + 1.f) / ((vu + 1.f) * (vu + 1.f)), gvi = gious / (vu + 1.f), gac = 0.f;
    if (loss_type == 2) { gvu -= 1.f / ac; gac = vu / (ac * ac); }     // loss = 2 - ious - vu / ac
    gvi -= gvu;
    const float gpw = gvu * ph * pd, gph = gvu * pw * pd, gpd = gvu * pw * ph;
    const float gwi = gvi * hi * di, ghi = gvi * wi * di, gdi = gvi * wi * hi, ggw = gac * gh * gd, ggh = gac * gw * gd, ggd = gac * gw * gh;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const int ax = k % 3;
      const float a = ax == 0 ? gpw : (ax == 1 ? gph : gpd), b = ax == 0 ? gwi : (ax == 1 ? ghi : gdi), c = ax == 0 ? ggw : (ax == 1 ? ggh : ggd);
      gp[k] = a + b * pick_a<true>(p[k], t[k]) + c * pick_a<false>(p[k], t[k]);
    }
    gp[6] = gp[7] = 0.f;
  }
  return loss;
}

// oriented term of one location
template <int KIND>
__device__ __forceinline__ float fcos_obb_term(const float (&p)[8], const float (&t)[8], int loss_type) {
  const Dec A = fcos_decode(p), B = fcos_decode(t);
  const PairOut o = obb_pair(A.o, B.o);
  if (KIND == FCOS_OBB_IOU) {
    const float r = (o.inter3d + 1.f) / (o.u3d + 1.f);
    return loss_type == 0 ? -logf(r) : 1.f - r;
  }
  float X[8], Y[8];
  obb_corners(A.o, X, Y, 0);
  obb_corners(B.o, X, Y, 4);
  Encl E;
  return obb_pair_loss<KIND == FCOS_OBB_GIOU ? OBB_GIOU_SMALLEST : OBB_DIOU_SMALLEST>(A.o, B.o, o, X, Y, E);
}
template <int KIND>
__device__ __forceinline__ void fcos_obb_term_grad(const float (&p)[8], const float (&t)[8], int loss_type, float (&gp)[8]) {
  const Dec A = fcos_decode(p), B = fcos_decode(t);
  BoxGrad ga, gb;
  if (KIND == FCOS_OBB_IOU) {
    const PairOut o = obb_pair(A.o, B.o);
    const float u1 = o.u3d + 1.f, r = (o.inter3d + 1.f) / u1, gr = loss_type == 0 ? -1.f / r : -1.f;
    obb_pair_grad<OBB_IOU>(A.o, B.o, gr * o.u3d / u1, gr * (o.iou - 1.f) / (u1 * u1), 0.f, false, ga, gb);
  } else {
    obb_pair_grad<KIND == FCOS_OBB_GIOU ? OBB_GIOU_SMALLEST : OBB_DIOU_SMALLEST>(A.o, B.o, 0.f, 0.f, 1.f, false, ga, gb);
  }
  fcos_decode_bwd(A, ga, gp);
}

constexpr float FCOS_2D_RES = 160.f;      // the reference's literal: the cameras and the divisor, whatever the scene size
struct Fcos2d { Proj2dCams cams; float weight; };        // read only by the kernels with P2D

template <int KIND, bool P2D>
__global__ __launch_bounds__(256) void fcos_pos_fwd_kernel(FcosGeom G, Ptr4<const float> reg, Ptr4<const float> ctr, const float* __restrict__ labels, const float* __restrict__ targets,
                                                           const float* __restrict__ ctr_t, const unsigned char* __restrict__ valid, int loss_type, int add_l1, Fcos2d p2d,
                                                           float* __restrict__ partials) {
  constexpr int C = KIND == FCOS_AABB ? 6 : 8;
  const Where w = fcos_where(G);
  float v[2] = {0.f, 0.f};              // regression, centerness
  if (w.active && valid[w.p] && labels[w.p] > 0.f) {
    const float* rp = pick4(reg.p, w.lvl) + (long)w.scene * C * w.n + w.loc;
    float p[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, t[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, gp[8];
#pragma unroll
    for (int k = 0; k < C; ++k) { p[k] = rp[(long)k * w.n]; t[k] = targets[w.p * C + k]; }
    const float ct = ctr_t[w.p];
    float term = KIND == FCOS_AABB ? fcos_aabb_term<false>(p, t, loss_type, gp) : fcos_obb_term<KIND>(p, t, loss_type);
    if (KIND != FCOS_AABB && add_l1) term += smooth_l1(p[6] - t[6]) + smooth_l1(p[7] - t[7]);
    if constexpr (P2D) term += p2d.weight * (proj2d_term(fcos_decode(p).o, fcos_decode(t).o, p2d.cams) / FCOS_2D_RES / 16.f);
    v[0] = term * ct;
    const float c = pick4(ctr.p, w.lvl)[(long)w.scene * w.n + w.loc];
    v[1] = fmaxf(c, 0.f) - c * ct + log1pf(expf(-fabsf(c)));
  }
  block_sum_fixed(v, partials + 2 * (long)blockIdx.x);
}

template <int KIND, bool P2D>
__global__ __launch_bounds__(256) void fcos_pos_bwd_kernel(FcosGeom G, Ptr4<const float> reg, Ptr4<const float> ctr, const float* __restrict__ labels, const float* __restrict__ targets,
                                                           const float* __restrict__ ctr_t, const unsigned char* __restrict__ valid, int loss_type, int add_l1, Fcos2d p2d,
                                                           const float* __restrict__ scalars, float world, const float* __restrict__ g_reg, const float* __restrict__ g_ctr,
                                                           Ptr4<float> dreg, Ptr4<float> dctr) {
  constexpr int C = KIND == FCOS_AABB ? 6 : 8;
  const Where w = fcos_where(G);
  if (!w.active) return;
  float gp[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, gc = 0.f;
  const long at = (long)w.scene * w.n + w.loc, rat = (long)w.scene * C * w.n + w.loc;
  if (valid[w.p] && labels[w.p] > 0.f) {
    const float* rp = pick4(reg.p, w.lvl) + rat;
    float p[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, t[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < C; ++k) { p[k] = rp[(long)k * w.n]; t[k] = targets[w.p * C + k]; }
    const float ct = ctr_t[w.p], csum = scalars[1];
    const float sr = csum > 0.f ? (g_reg ? g_reg[0] : 0.f) * ct / (csum / world) : 0.f;
    if (KIND == FCOS_AABB) fcos_aabb_term<true>(p, t, loss_type, gp);
    else fcos_obb_term_grad<KIND>(p, t, loss_type, gp);
    if (KIND != FCOS_AABB && add_l1) { gp[6] += smooth_l1_grad(p[6] - t[6]); gp[7] += smooth_l1_grad(p[7] - t[7]); }
    if constexpr (P2D) {
      const Dec A = fcos_decode(p);
      BoxGrad g;
      float g2[8];
      proj2d_term_grad(A.o, fcos_decode(t).o, p2d.cams, g);
      fcos_decode_bwd(A, g, g2);
      const float s2 = p2d.weight / FCOS_2D_RES / 16.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) gp[k] += s2 * g2[k];
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) gp[k] *= sr;
    const float c = pick4(ctr.p, w.lvl)[at];
    float sp, sg, sq;
    fcos_sig(c, sp, sg, sq);
    gc = (sg - ct) * (g_ctr ? g_ctr[0] : 0.f) / fmaxf(scalars[0] / world, 1.f);
  }
  float* dp = pick4(dreg.p, w.lvl) + rat;
#pragma unroll
  for (int k = 0; k < C; ++k) dp[(long)k * w.n] = gp[k];
  pick4(dctr.p, w.lvl)[at] = gc;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
int make_geom(int nlevels, const int* dims, int N, FcosGeom& G) {
  if (nlevels < 1 || nlevels > 4 || N < 1 || N > NMH_FCOS_MAX_SCENES || !dims) return -4;
  G.L = nlevels; G.N = N;
  long blocks = 0, p0 = 0;
  for (int k = 0; k < 4; ++k) {
    const int j = k < nlevels ? k : nlevels - 1;
    const long w = dims[4 * j], l = dims[4 * j + 1], h = dims[4 * j + 2], s = dims[4 * j + 3], n = w * l * h;
    if (w < 1 || l < 1 || h < 1 || s < 1 || n > (1L << 30)) return -4;
    G.w[k] = (int)w; G.l[k] = (int)l; G.h[k] = (int)h; G.s[k] = (int)s; G.n[k] = (int)n;
    G.bpl[k] = (int)((n + 255) / 256);
    G.blk0[k] = (int)blocks; G.p0[k] = p0;
    if (k < nlevels) { blocks += (long)G.bpl[k] * N; p0 += n * N; }
    if (blocks >= (1L << 31) - 1 || p0 >= (1L << 40)) return -4;
  }
  G.nblocks = (int)blocks;
  return 0;
}
void launch_final(const float* partials, int nblocks, int what, float world, float* scalars, float* out0, float* out1, hipStream_t st) {
  hipLaunchKernelGGL(fcos_final_kernel, dim3(1), dim3(256), 0, st, partials, nblocks, what, world, scalars, out0, out1);
}

}  // namespace

long k_fcos_num_blocks(int nlevels, const int* dims, int N) {
  FcosGeom G;
  return make_geom(nlevels, dims, N, G) ? -1 : G.nblocks;
}

int k_fcos_assign(int nlevels, const int* dims, int N, int ncols, const float* boxes, const int* offs, const int* sizes, const unsigned char* const* masks, float radius,
                  int norm_targets, float* labels, float* targets, int* gt_index, float* ctr_t, unsigned char* valid, float* partials, float* scalars, hipStream_t st) {
  FcosGeom G;
  if (make_geom(nlevels, dims, N, G) || (ncols != 6 && ncols != 7) || !offs || offs[0] != 0) return -4;
  FcosOffs S;
  for (int b = 0; b <= NMH_FCOS_MAX_SCENES; ++b) S.off[b] = offs[b < N ? b : N];
  for (int b = 0; b < N; ++b) if (offs[b + 1] < offs[b]) return -4;
  if (offs[N] > 0 && !boxes) return -4;
  if (masks && !all_set(nlevels, masks)) return -4;
  const Ptr4<const unsigned char> M = make_ptrs<const unsigned char>(nlevels, masks);
  if (ncols == 7) hipLaunchKernelGGL(fcos_assign_kernel<true>, dim3(G.nblocks), dim3(256), 0, st, G, S, boxes, sizes, M, masks ? 1 : 0, radius, norm_targets, labels, targets, gt_index, ctr_t, valid, partials);
  else hipLaunchKernelGGL(fcos_assign_kernel<false>, dim3(G.nblocks), dim3(256), 0, st, G, S, boxes, sizes, M, masks ? 1 : 0, radius, norm_targets, labels, targets, gt_index, ctr_t, valid, partials);
  NMH_CHECK_LAUNCH();
  launch_final(partials, G.nblocks, FIN_SCALARS, 1.f, scalars, nullptr, nullptr, st);
  NMH_CHECK_LAUNCH();
  return 0;
}

int k_fcos_focal_fwd(int nlevels, const int* dims, int N, const float* const* cls, const float* labels, const unsigned char* valid, const float* scalars, float world, float* partials,
                     float* loss, hipStream_t st) {
  FcosGeom G;
  if (make_geom(nlevels, dims, N, G) || !all_set(nlevels, cls) || !(world >= 1.f)) return -4;
  hipLaunchKernelGGL(fcos_focal_fwd_kernel, dim3(G.nblocks), dim3(256), 0, st, G, make_ptrs<const float>(nlevels, cls), labels, valid, partials);
  NMH_CHECK_LAUNCH();
  launch_final(partials, G.nblocks, FIN_CLS, world, const_cast<float*>(scalars), loss, nullptr, st);
  NMH_CHECK_LAUNCH();
  return 0;
}

int k_fcos_focal_bwd(int nlevels, const int* dims, int N, const float* const* cls, const float* labels, const unsigned char* valid, const float* scalars, float world, const float* g_loss,
                     float* const* dcls, hipStream_t st) {
  FcosGeom G;
  if (make_geom(nlevels, dims, N, G) || !all_set(nlevels, cls) || !all_set(nlevels, dcls) || !(world >= 1.f)) return -4;
  hipLaunchKernelGGL(fcos_focal_bwd_kernel, dim3(G.nblocks), dim3(256), 0, st, G, make_ptrs<const float>(nlevels, cls), labels, valid, scalars, world, g_loss, make_ptrs<float>(nlevels, dcls));
  NMH_CHECK_LAUNCH();
  return 0;
}

static int pos_kind(int ncols, int loss_type) {
  if (ncols == 6) return loss_type >= 0 && loss_type <= 2 ? FCOS_AABB : -1;
  if (ncols != 8) return -1;
  return loss_type == 0 || loss_type == 1 ? FCOS_OBB_IOU : (loss_type == 2 ? FCOS_OBB_GIOU : (loss_type == 3 ? FCOS_OBB_DIOU : -1));
}

// proj2d_weight < 0: the entries without the 2-D term
int k_fcos_pos_fwd(int nlevels, const int* dims, int N, int ncols, int loss_type, int add_l1, const float* const* reg, const float* const* ctr, const float* labels, const float* targets,
                   const float* ctr_t, const unsigned char* valid, const float* scalars, float world, float* partials, float* reg_loss, float* ctr_loss, hipStream_t st) {
  return k_fcos_pos2d_fwd(nlevels, dims, N, ncols, loss_type, add_l1, -1.f, reg, ctr, labels, targets, ctr_t, valid, scalars, world, partials, reg_loss, ctr_loss, st);
}
int k_fcos_pos2d_fwd(int nlevels, const int* dims, int N, int ncols, int loss_type, int add_l1, float proj2d_weight, const float* const* reg, const float* const* ctr, const float* labels,
                     const float* targets, const float* ctr_t, const unsigned char* valid, const float* scalars, float world, float* partials, float* reg_loss, float* ctr_loss,
                     hipStream_t st) {
  FcosGeom G;
  const int kind = pos_kind(ncols, loss_type);
  const bool with2d = proj2d_weight >= 0.f;
  if (make_geom(nlevels, dims, N, G) || kind < 0 || !all_set(nlevels, reg) || !all_set(nlevels, ctr) || !(world >= 1.f) || (with2d && ncols != 8)) return -4;
  const Ptr4<const float> R = make_ptrs<const float>(nlevels, reg), Cn = make_ptrs<const float>(nlevels, ctr);
  Fcos2d W = {};
  if (with2d) { proj2d_make_cams(FCOS_2D_RES, W.cams); W.weight = proj2d_weight; }
#define FCOS_FWD(K, P) hipLaunchKernelGGL((fcos_pos_fwd_kernel<K, P>), dim3(G.nblocks), dim3(256), 0, st, G, R, Cn, labels, targets, ctr_t, valid, loss_type, add_l1, W, partials)
#define FCOS_FWD2(K) if (with2d) FCOS_FWD(K, true); else FCOS_FWD(K, false)
  switch (kind) {
    case FCOS_AABB: FCOS_FWD(FCOS_AABB, false); break;
    case FCOS_OBB_IOU: FCOS_FWD2(FCOS_OBB_IOU); break;
    case FCOS_OBB_GIOU: FCOS_FWD2(FCOS_OBB_GIOU); break;
    default: FCOS_FWD2(FCOS_OBB_DIOU); break;
  }
#undef FCOS_FWD2
#undef FCOS_FWD
  NMH_CHECK_LAUNCH();
  launch_final(partials, G.nblocks, FIN_POS, world, const_cast<float*>(scalars), reg_loss, ctr_loss, st);
  NMH_CHECK_LAUNCH();
  return 0;
}

int k_fcos_pos_bwd(int nlevels, const int* dims, int N, int ncols, int loss_type, int add_l1, const float* const* reg, const float* const* ctr, const float* labels, const float* targets,
                   const float* ctr_t, const unsigned char* valid, const float* scalars, float world, const float* g_reg, const float* g_ctr, float* const* dreg, float* const* dctr,
                   hipStream_t st) {
  return k_fcos_pos2d_bwd(nlevels, dims, N, ncols, loss_type, add_l1, -1.f, reg, ctr, labels, targets, ctr_t, valid, scalars, world, g_reg, g_ctr, dreg, dctr, st);
}
int k_fcos_pos2d_bwd(int nlevels, const int* dims, int N, int ncols, int loss_type, int add_l1, float proj2d_weight, const float* const* reg, const float* const* ctr, const float* labels,
                     const float* targets, const float* ctr_t, const unsigned char* valid, const float* scalars, float world, const float* g_reg, const float* g_ctr, float* const* dreg,
                     float* const* dctr, hipStream_t st) {
  FcosGeom G;
  const int kind = pos_kind(ncols, loss_type);
  const bool with2d = proj2d_weight >= 0.f;
  if (make_geom(nlevels, dims, N, G) || kind < 0 || !all_set(nlevels, reg) || !all_set(nlevels, ctr) || !all_set(nlevels, dreg) || !all_set(nlevels, dctr) || !(world >= 1.f) ||
      (with2d && ncols != 8)) return -4;
  const Ptr4<const float> R = make_ptrs<const float>(nlevels, reg), Cn = make_ptrs<const float>(nlevels, ctr);
  const Ptr4<float> DR = make_ptrs<float>(nlevels, dreg), DC = make_ptrs<float>(nlevels, dctr);
  Fcos2d W = {};
  if (with2d) { proj2d_make_cams(FCOS_2D_RES, W.cams); W.weight = proj2d_weight; }
#define FCOS_BWD(K, P) hipLaunchKernelGGL((fcos_pos_bwd_kernel<K, P>), dim3(G.nblocks), dim3(256), 0, st, G, R, Cn, labels, targets, ctr_t, valid, loss_type, add_l1, W, scalars, world, g_reg, g_ctr, DR, DC)
#define FCOS_BWD2(K) if (with2d) FCOS_BWD(K, true); else FCOS_BWD(K, false)
  switch (kind) {
    case FCOS_AABB: FCOS_BWD(FCOS_AABB, false); break;
    case FCOS_OBB_IOU: FCOS_BWD2(FCOS_OBB_IOU); break;
    case FCOS_OBB_GIOU: FCOS_BWD2(FCOS_OBB_GIOU); break;
    default: FCOS_BWD2(FCOS_OBB_DIOU); break;
  }
#undef FCOS_BWD2
#undef FCOS_BWD
  NMH_CHECK_LAUNCH();
  return 0;
}

int k_fcos_obb_encode(const float* loc, const float* boxes, long n, float* out, hipStream_t st) {
  if (n <= 0 || (n + 255) / 256 >= (1L << 31)) return -4;
  hipLaunchKernelGGL(fcos_obb_encode_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, loc, boxes, n, out);
  NMH_CHECK_LAUNCH();
  return 0;
}
int k_fcos_obb_decode_fwd(const float* loc, const float* reg, long n, float* out, hipStream_t st) {
  if (n <= 0 || (n + 255) / 256 >= (1L << 31)) return -4;
  hipLaunchKernelGGL(fcos_obb_decode_fwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, loc, reg, n, out);
  NMH_CHECK_LAUNCH();
  return 0;
}
int k_fcos_obb_decode_bwd(const float* reg, const float* gbox, long n, float* dreg, hipStream_t st) {
  if (n <= 0 || (n + 255) / 256 >= (1L << 31)) return -4;
  hipLaunchKernelGGL(fcos_obb_decode_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, reg, gbox, n, dreg);
  NMH_CHECK_LAUNCH();
  return 0;
}
